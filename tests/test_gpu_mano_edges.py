"""The MANO loss pass (csrc/mano.hip, csrc/mano_joint_pass.h) and its reverse (csrc/mano_bwd.hip) against the float64 reference of
tests/mano_pass_ref.py, at every output and at their edges.  The C entries are called directly, on buffers with SPARE sentinel rows behind R:

  forward  mhe_mano_joints_f32 (terms [R,4]), mhe_mano_joints_mods_f32 (mods uv, xyz, uv|xyz; terms [R,5]), mhe_mano_joints_chamfer_f32,
           mhe_mano_decode_f32 - mano_joints16_kernel, four hypotheses per wave; with MHE_MANO_FOUR=0 (a fresh child process)
           mano_joints_kernel<4> / <5>, one hypothesis per wave
  reverse  mhe_mano_joints_bwd_f32, mhe_mano_joints_mods_bwd_f32, mhe_mano_joints_chamfer_bwd_f32 - mano_joints_bwd_kernel, per-row g_det

  a. every output at ragged row counts (the last row quad has 1, 2, 3 and 4 live 16-lane groups; R below, at and across 16 and 64; N = 1 and
     B = 1), rows >= R of every buffer bit-equal to the sentinel (every launch of this file checks that)
  b. null outputs: a call that asks for one output gives the bits of the full call; mhe_mano_decode_f32's joint outputs are those of
     mhe_mano_joints_f32 and its mesh that of mhe_mano_verts_f32 on its z
  c. numerical edges, forward and reverse: all axis-angles exactly zero (Rodrigues at its + 1e-8), tiny angles, |th3| next to pi, the priors on
     and beside their faces, the Laplace dead zone |d| <= 1e-4, vis other than 0 / 1 / 2, exp(log s) at +-3 and large translations, inv_norm,
     the clamp of obj_count, a vertex on a joint and tied vertices
  d. R = 8192 + 7: the second trip of the grid-stride loops
  e. the one-hypothesis-per-wave forward kernels

Bounds: none comes from the kernels.  Per tensor and case max(3 max|f32 reference - f64 reference|, 2e-6 max|f64 reference|), the rule of
test_generic_lbs_at_smpl_size_matches_oracle (the f32 reference is the same code in float32 on the CPU; 3 covers another association and fused
multiply-adds); z is a pure copy, bound 0.  The largest |diff| / bound of every entry is printed before it is asserted (`pytest -s`).

Measured on an MI355X, the largest |diff| / bound per entry over every test of this file (no bound had to be widened, no kernel was changed):
  mhe_mano_joints_f32 0.210   mhe_mano_joints_mods_f32 0.210   mhe_mano_joints_chamfer_f32 0.210 (dist included)
  mhe_mano_joints_bwd_f32 0.247   mhe_mano_joints_mods_bwd_f32 0.349   mhe_mano_joints_chamfer_bwd_f32 0.454
  mano_joints_kernel<4> 0.197   mano_joints_kernel<5> 0.197 (MHE_MANO_FOUR=0);   mhe_mano_decode_f32's mesh against mhe_mano_verts_f32: measured difference 0 (asserted: within max(3 e_f32, 2e-6) of the extent)
Sensitivity (one-token changes of the arithmetic in a scratch build, each run once through this file): the reverse without `&& fabsf(d) > 1e-4f`
fails test_laplace_dead_zone; the reverse's t_cam operands swapped, `999.f * aJ` and the loss pass's `49.f * vbt * vbt` each fail 17-18 tests (a, c, d);
the one-hypothesis-per-wave kernel's t_cam operands swapped fail test_one_hypothesis_per_wave_kernels_in_a_fresh_process.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mano_pass_ref as mr
from edge_measure import Measure
from mhentropy_amd import synth

SENT, SPARE = -7.0, 40                     # the value behind row R of every output buffer, and how many rows of it
KEYS = ("z", "xyz", "uv", "terms", "log_p", "norms", "joints_mm")
CW = 10.0                                  # chamfer_w of the reverse cases (the reference's w_chamfer)
SHAPES = [(1, 1), (1, 2), (1, 3), (5, 1), (1, 7), (3, 5), (1, 17), (2, 33), (3, 23)]          # (B, N)
# R = 8192 + 7.  launch16 (mano.hip) caps the grid at 512 workgroups of 16 rows = 8192 rows, joints_bwd_launch (mano_bwd.hip) and the
# one-hypothesis-per-wave forward (joints_launch) at 2048 workgroups of 4 rows = 8192 rows: rows 8192 .. 8198 run on the second loop trip
R_BIG = 512 * 16 + 7
assert R_BIG == 2048 * 4 + 7
ROWS_BIG = np.concatenate([np.arange(16), np.arange(R_BIG - 23, R_BIG)])          # the rows the reference is called on: 0..15, 8176..8198


def M(kernel):
    return Measure(kernel, "mano-edges")


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
def _case(name, B, N, seed, th45_scale=0.8, zero_mean=False):
    """R = N B random rows (row r is hypothesis r // B of image r % B), the targets of synth.batch, d loss / d log_p[r] = g[r % B] / N"""
    rng = np.random.default_rng(seed)
    R = N * B
    th45 = rng.normal(0, th45_scale, (R, 45)).astype(np.float32)
    det = (rng.normal(0, 1.0, (B, 16)) * np.array([1.0] * 3 + [0.03] * 10 + [0.2] * 3)).astype(np.float32)
    _, y = synth.batch(seed, B, with_image=False)
    return SimpleNamespace(name=name, R=R, B=B, N=N, th45=th45, det=det, crop_uv=y["crop_uv"].copy(), vis=y["vis"].copy(), pose3d=y["pose3d"].copy(),
                           g=rng.normal(0, 1, B).astype(np.float32), lap_b=0.03, lap_b3=0.05, alpha=50.0, zero_mean=zero_mean, cham=None)


_REF = {}


def _ref(c, mods, dtype=torch.float64, cham=False, grad=False, inv_norm=False, image_size=256.0, rows=None):
    """the reference of case c (of its rows `rows`), computed once"""
    key = (c.name, mods, dtype, cham, grad, inv_norm, image_size, None if rows is None else rows.tobytes())
    if key not in _REF:
        img = None if rows is None else rows % c.B
        _REF[key] = mr.mano_pass(c.th45 if rows is None else c.th45[rows], c.det, c.crop_uv, c.vis, c.pose3d, mods=mods, laplace_b=c.lap_b,
                                 laplace_b_3d=c.lap_b3, th45_alpha=c.alpha, inv_norm=inv_norm, image_size=image_size, dtype=dtype,
                                 zero_mean=c.zero_mean, img=img, chamfer=c.cham if cham else None, chamfer_w=CW if cham else 0.0, grad=grad,
                                 g_log_p=c.g, row_w=1.0 / c.N)
    return _REF[key]


def _objects(c, VO, counts, rows=None, plant=None):
    """object targets in the units of the data (tests/chamfer_ref.py: bone scale in m, root and vertices in mm, the vertices within 90 mm of
    the root; the root on a 1/8 mm grid so that root + 2 is exact in float32).  Drawn again from the next seed until every minimum of the
    REFERENCE's case has its runner-up CH_GAP away: 50 times what separates an f32 evaluation of these distances from f64 (2e-6: coordinates
    of ~500 mm, distances of ~50 mm), so the kernels' argmins are the reference's and only planted ties are ties."""
    xyz = torch.as_tensor(_ref(c, 1, rows=rows)["xyz"]).view(-1, 21, 3)
    img = (np.arange(c.R) if rows is None else rows) % c.B
    for seed in range(400):
        rng = np.random.default_rng(7000 + seed)
        scale = rng.uniform(0.025, 0.04, c.B).astype(np.float32)
        root = (np.round((rng.uniform(-80.0, 80.0, (c.B, 3)) + np.array([0.0, 0.0, 500.0])) * 8) / 8).astype(np.float32)
        obj = (root[:, None, :] + rng.uniform(-90.0, 90.0, (c.B, VO, 3))).astype(np.float32)
        if plant is not None:
            plant(xyz.numpy(), scale, root, obj)
        cham = (scale, root, obj, None if counts is None else np.asarray(counts, np.int32))
        if mr.chamfer_rows(xyz, img, *cham)[1] >= mr.CH_GAP:
            return cham
    raise AssertionError("no draw with every minimum of the reference determined")


# ---- launches ------------------------------------------------------------------------------------------------------------------------------------
def _raw(entry, *args):
    """the C entry itself: tensors as device addresses, None as null, the current stream appended -> status"""
    from mhentropy_amd import _lib
    conv = [C.c_void_p(0 if a is None else a.data_ptr()) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    return getattr(_lib.lib(), entry)(*conv, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _call(entry, *args):
    from mhentropy_amd import _lib
    rc = _raw(entry, *args)
    assert rc == 0, (entry, rc, _lib.lib().mhe_last_error().decode())
    torch.cuda.synchronize()


def _collect(buf, R, what):
    out = {}
    for k, t in buf.items():
        if t is not None:
            t = t.cpu()
            assert bool((t[R:] == SENT).all()), "%s: %s written behind row R = %d" % (what, k, R)
            out[k] = t[:R, 0].clone() if k in ("log_p", "dist") else t[:R].clone()
    return out


def _operands(c):
    from mhentropy_amd import _lib  # noqa: F401  (the library must be there: no fallback)
    d = SimpleNamespace(th45=_dev(c.th45), det=_dev(c.det), crop_uv=_dev(c.crop_uv), vis=_dev(c.vis), pose3d=_dev(c.pose3d), g=_dev(c.g),
                        blob=_dev(mr.packed_tables(c.zero_mean)))
    d.cham = (None,) * 4 if c.cham is None else tuple(_dev(a) for a in c.cham)
    return d


def _fwd(c, entry, mods=1, want=KEYS, inv_norm=0, image_size=256.0, mm=0):
    """entry: "f32" | "mods" | "chamfer" | "decode" -> {output: CPU tensor [R, ...]} of the outputs in `want` (+ dist, + verts)"""
    from mhentropy_amd import _lib
    R, B, d = c.R, c.B, _operands(c)
    wid = dict(z=61, xyz=63, uv=42, terms=4 if entry in ("f32", "decode") else 5, log_p=1, norms=2, joints_mm=63)
    buf = {k: (torch.full((R + SPARE, wid[k]), SENT, device="cuda") if k in want else None) for k in KEYS}
    o = [buf[k] for k in KEYS]
    if entry == "f32":
        _call("mhe_mano_joints_f32", d.th45, d.det, d.crop_uv, d.vis, d.blob, *o, R, B, c.lap_b, c.alpha, inv_norm, image_size)
    elif entry == "mods":
        _call("mhe_mano_joints_mods_f32", d.th45, d.det, d.crop_uv, d.vis, d.pose3d, d.blob, *o, R, B, mods, c.lap_b, c.lap_b3, c.alpha, inv_norm, image_size)
    elif entry == "chamfer":
        buf["dist"] = torch.full((R + SPARE, 1), SENT, device="cuda")
        _call("mhe_mano_joints_chamfer_f32", d.th45, d.det, d.crop_uv, d.vis, d.pose3d, d.blob, *d.cham, *o, buf["dist"], R, B, c.cham[2].shape[1], mods,
              c.lap_b, c.lap_b3, c.alpha, inv_norm, image_size)
    else:
        buf["verts"] = torch.full((R + SPARE, 778 * 3), SENT, device="cuda")
        ws = torch.empty(_lib.lib().mhe_mano_verts_workspace_floats(R), device="cuda")
        _call("mhe_mano_decode_f32", d.th45, d.det, d.crop_uv, d.vis, d.blob, *o, buf["verts"], ws, R, B, c.lap_b, c.alpha, inv_norm, image_size, mm)
    return _collect(buf, R, "%s %s mods %d" % (c.name, entry, mods))


def _bwd(c, entry, mods=1, alpha=None):
    """entry: "f32" | "mods" | "chamfer" -> g_th45 [R,45], g_det [R,16] (one row per hypothesis)"""
    R, B, d = c.R, c.B, _operands(c)
    alpha = c.alpha if alpha is None else alpha
    buf = {"g_th45": torch.full((R + SPARE, 45), SENT, device="cuda"), "g_det": torch.full((R + SPARE, 16), SENT, device="cuda")}
    o, w = (d.g, buf["g_th45"], buf["g_det"]), 1.0 / c.N
    if entry == "f32":
        _call("mhe_mano_joints_bwd_f32", d.th45, d.det, d.crop_uv, d.vis, d.blob, *o, R, B, c.lap_b, alpha, w)
    elif entry == "mods":
        _call("mhe_mano_joints_mods_bwd_f32", d.th45, d.det, d.crop_uv, d.vis, d.pose3d, d.blob, *o, R, B, mods, c.lap_b, c.lap_b3, alpha, w)
    else:
        _call("mhe_mano_joints_chamfer_bwd_f32", d.th45, d.det, d.crop_uv, d.vis, d.pose3d, d.blob, *d.cham, *o, R, B, c.cham[2].shape[1], mods, c.lap_b,
              c.lap_b3, alpha, w, CW)
    return _collect(buf, R, "%s %s reverse mods %d" % (c.name, entry, mods))


def _add(m, label, got, c, mods, keys, cham=False, grad=False, rows=None, terms="terms5", **kw):
    """got[k] (its rows `rows`) against the float64 reference, bound from the float32 reference"""
    r64, r32 = (_ref(c, mods, dt, cham, grad, rows=rows, **kw) for dt in (torch.float64, torch.float32))
    for k in keys:
        rk = terms if k == "terms" else k
        g = np.asarray(got[k])
        m.add("%s %s" % (label, k), g if rows is None else g[rows], r64[rk], mr.bound(r64, r32, rk))


def _all_entries(c, ms, rows=None, mods_fwd=(1, 2, 3), mods_bwd=(2, 3)):
    """every forward and reverse entry on case c (c.cham set), every output against the reference; -> the outputs by (entry, mods)"""
    got = {}
    got["f32", 1] = o = _fwd(c, "f32")
    _add(ms["mhe_mano_joints_f32"], c.name, o, c, 1, KEYS, rows=rows, terms="terms4")
    for mods in mods_fwd:
        got["mods", mods] = o = _fwd(c, "mods", mods)
        _add(ms["mhe_mano_joints_mods_f32"], "%s mods %d" % (c.name, mods), o, c, mods, KEYS, rows=rows)
    got["chamfer", 3] = o = _fwd(c, "chamfer", 3)
    _add(ms["mhe_mano_joints_chamfer_f32"], c.name, o, c, 3, KEYS + ("dist",), cham=True, rows=rows)
    for k in KEYS:          # the Chamfer term touches dist alone
        assert torch.equal(o[k], got["mods", 3][k]), (c.name, k)
    G = ("g_th45", "g_det")
    got["bwd f32", 1] = o = _bwd(c, "f32")
    _add(ms["mhe_mano_joints_bwd_f32"], c.name, o, c, 1, G, grad=True, rows=rows)
    for mods in mods_bwd:
        got["bwd mods", mods] = o = _bwd(c, "mods", mods)
        _add(ms["mhe_mano_joints_mods_bwd_f32"], "%s mods %d" % (c.name, mods), o, c, mods, G, grad=True, rows=rows)
    got["bwd chamfer", 3] = o = _bwd(c, "chamfer", 3)
    _add(ms["mhe_mano_joints_chamfer_bwd_f32"], c.name, o, c, 3, G, cham=True, grad=True, rows=rows)
    return got


ENTRIES = ("mhe_mano_joints_f32", "mhe_mano_joints_mods_f32", "mhe_mano_joints_chamfer_f32", "mhe_mano_joints_bwd_f32",
           "mhe_mano_joints_mods_bwd_f32", "mhe_mano_joints_chamfer_bwd_f32")


def _measures(tag):
    return {e: M("%s (%s)" % (e, tag)) for e in ENTRIES}


def _report(ms):
    for m in ms.values():
        if m.rows:
            m.report()


_RAGGED = {}


def _ragged(B, N):
    """the case of shape (B, N) with its object targets (VO = 9; per-image counts 0 .. 11 at every other shape: 0 acts as 1, 10 and 11 as 9)"""
    if (B, N) not in _RAGGED:
        c = _case("ragged_B%d_N%d" % (B, N), B, N, 100 * B + N)
        cnt = np.random.default_rng(B * 7 + N).integers(0, 12, B)
        c.cham = _objects(c, 9, cnt if (B + N) % 2 else None)
        _RAGGED[B, N] = c
    return _RAGGED[B, N]


# ---- a. every output at ragged row counts -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,N", SHAPES, ids=["B%d_N%d" % s for s in SHAPES])
def test_every_output_at_ragged_row_counts(gpu_lib, B, N):
    """the seven entries' outputs on R = N B rows against float64, nothing written behind row R (a dead 16-lane group of mano_joints16_kernel
    redoes row R - 1 and must store nothing: SPARE rows of every buffer keep the sentinel).
    Measured on an MI355X: forward entries 0.192, mhe_mano_joints_bwd_f32 0.247, _mods_bwd_f32 0.344, _chamfer_bwd_f32 0.263 (the worst of the nine shapes)"""
    c = _ragged(B, N)
    ms = _measures("ragged rows")
    _all_entries(c, ms)
    _report(ms)


# ---- b. null outputs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_subset_of_the_outputs_is_the_full_call_bit_for_bit(gpu_lib):
    """R = 7: every single output, and the pair (terms, log_p), requested alone - the other pointers null - through mhe_mano_joints_f32 (uv, terms
    [R,4]) and mhe_mano_joints_mods_f32 (uv | xyz)"""
    c = _ragged(1, 7)
    for entry, mods in (("f32", 1), ("mods", 3)):
        full = _fwd(c, entry, mods)
        for want in [(k,) for k in KEYS] + [("terms", "log_p")]:
            part = _fwd(c, entry, mods, want=want)
            assert set(part) == set(want)
            for k in want:
                assert torch.equal(part[k], full[k]), (entry, want, k)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 5, 7])
def test_decode_is_the_joint_pass_and_the_mesh_of_its_z(gpu_lib, R):
    """mhe_mano_decode_f32: joint outputs bit-equal to mhe_mano_joints_f32's; the mesh (both modes) against mhe_mano_verts_f32 on its z within
    max(3 e_f32, 2e-6) of the mesh's extent, e_f32 = the f32 oracle's distance from f64 (the bound test_gpu_kernels.py holds both meshes to)"""
    from mhentropy_amd import ops
    from oracle import network_ref
    c = _ragged(1, R)
    joints = _fwd(c, "f32")
    z = torch.as_tensor(_ref(c, 1)["z"])
    with torch.no_grad():
        v64 = network_ref.decode(mr.tables(torch.float64), z)["verts"]
        v32 = network_ref.decode(mr.tables(torch.float32), z.float())["verts"].double()
    ext = float(v64.abs().max())
    tol = max(3 * float((v32 - v64).abs().max()) / ext, 2e-6)
    for mm in (0, 1):
        o = _fwd(c, "decode", mm=mm)
        for k in KEYS:
            assert torch.equal(o[k], joints[k]), (k, mm)
        mesh = ops.mano_verts(_dev(o["z"].numpy()), _dev(mr.packed_tables()), mm=bool(mm)).cpu().view(R, -1)
        scale = float(mesh.abs().max())
        err = float((o["verts"] - mesh).abs().max()) / scale
        print("mano-edges: mhe_mano_decode_f32 R=%d mm=%d: mesh vs mhe_mano_verts_f32 %.2e of its extent (bound %.2e)" % (R, mm, err, tol))
        assert err <= tol, (R, mm, err, tol)
        if not mm:
            assert float((o["verts"].double() - v64.reshape(R, -1)).abs().max()) / ext <= tol


# ---- c. numerical edges -------------------------------------------------------------------------------------------------------------------------
def _rows_case(name, R, seed, **kw):
    """R rows with a det row each (B = R, N = 1)"""
    return _case(name, R, 1, seed, **kw)


@pytest.mark.gpu
def test_zero_pose_tiny_angles_and_th3_next_to_pi(gpu_lib):
    """tables packed with hands_mean = 0.  Row 0: th45 = 0 and th3 = 0, all 16 axis-angles exactly zero (Rodrigues at its + 1e-8 epsilon,
    forward and through the quaternion in reverse); rows 1-3: the wrist alone at 1e-6, 1e-4, 1e-2; rows 4-6: one PCA coefficient at 1e-6,
    1e-4, 1e-2 (every finger joint at about a tenth of that); rows 7, 8: |th3| = pi - 1e-3 and pi + 1e-3 (the ball prior's face; a half
    angle next to pi / 2); row 9: th3 = 0 under a random th45.
    Measured on an MI355X: forward entries 0.115, reverse 0.192 / 0.181 / 0.255 (bwd, mods_bwd, chamfer_bwd); every value finite"""
    c = _rows_case("zero_pose", 10, 41, zero_mean=True)
    c.th45[:9] = 0.0
    c.det[:7, :3] = 0.0
    c.det[9, :3] = 0.0
    for i, a in enumerate((1e-6, 1e-4, 1e-2)):
        c.det[1 + i, 0] = a
        c.th45[4 + i, (0, 7, 44)[i]] = a
    axis = np.array([0.6, 0.0, 0.8])
    c.det[7, :3], c.det[8, :3] = (np.pi - 1e-3) * axis, (np.pi + 1e-3) * axis
    r64 = _ref(c, 3, grad=True)
    assert (r64["terms5"][:7, 2] == 0).all() and r64["terms5"][7, 2] == 0 and r64["terms5"][8, 2] < 0          # th3 inside / outside the ball
    assert np.isfinite(r64["g_th45"]).all() and np.abs(r64["g_th45"][0]).max() > 0.0
    c.cham = _objects(c, 9, None)
    ms = _measures("zero pose")
    got = _all_entries(c, ms)
    for o in got.values():
        for k, v in o.items():
            assert bool(torch.isfinite(v).all()), k
    assert float(got["mods", 3]["terms"][:8, 2].abs().max()) == 0.0
    _report(ms)


@pytest.mark.gpu
def test_priors_on_and_beside_their_faces(gpu_lib):
    """|th45| at 2 exactly, 2 -+ 1e-3 and 5; |bt| at 0.03 -+ 1e-5 and 0.2; |th3| at pi -+ 1e-3 and 3 pi, both signs (float32 rounding moves
    these by 2.4e-7, 1.9e-9 and 2.4e-7: never across a face).  Exactly on a face the gradient of the prior is 0 on both sides: there the
    kernel's g_th45 has the bits of a run with th45_alpha = 0, beside it (2 + 1e-3, 5) it has not.
    Measured on an MI355X: forward entries 0.210, reverse 0.215 / 0.349 / 0.197"""
    c = _rows_case("prior_faces", 6, 42)
    v45 = np.array([2.0, 2.0 - 1e-3, 2.0 + 1e-3, 5.0], np.float32)
    vbt = np.array([0.03 - 1e-5, 0.03 + 1e-5, 0.2], np.float32)
    for r in range(6):
        sgn = 1.0 if r % 2 == 0 else -1.0
        for i in range(4):
            c.th45[r, (5 * r + 11 * i) % 45] = sgn * v45[i]
        for i in range(3):
            c.det[r, 3 + (r + 3 * i) % 10] = -sgn * vbt[i]
    axis = np.array([0.0, -0.8, 0.6])
    for r, rad in enumerate((np.pi - 1e-3, np.pi + 1e-3, 3 * np.pi)):
        c.det[r, :3] = rad * axis * (1.0 if r != 1 else -1.0)
    on_face, beside = np.abs(c.th45) == 2.0, (np.abs(c.th45) > 2.0005)
    assert on_face.sum() == 6 and beside.sum() >= 12
    r64 = _ref(c, 3, grad=True)
    assert (r64["terms5"][:, 3] < -50).all() and (r64["terms5"][:, 4] < -50).all() and (r64["terms5"][[1, 2], 2] < 0).all() and r64["terms5"][0, 2] == 0
    c.cham = _objects(c, 9, None)
    ms = _measures("prior faces")
    got = _all_entries(c, ms)
    free = _bwd(c, "mods", 3, alpha=0.0)["g_th45"]
    with_prior = got["bwd mods", 3]["g_th45"]
    assert torch.equal(with_prior[torch.as_tensor(on_face)], free[torch.as_tensor(on_face)])
    assert bool((with_prior[torch.as_tensor(beside)] != free[torch.as_tensor(beside)]).all())
    _report(ms)


@pytest.mark.gpu
def test_laplace_dead_zone(gpu_lib):
    """targets set to the kernel's own uv / xyz of a first call, and to that value +- 5e-5 (inside |d| <= 1e-4) and +- 3e-4 (outside), coordinate
    by coordinate, every joint visible.  The offsets are two orders of magnitude from the threshold and from the kernel's float32 error, so the
    reference falls on the same side - asserted on the reference's own uv / xyz before anything is compared.  Forward terms and the reverse's
    `fabsf(d) > 1e-4f` branch, 2D and 3D.
    Measured on an MI355X: forward entries 0.193, reverse 0.143 / 0.128 / 0.346 - g_det[13] needed no wider bound"""
    c = _rows_case("dead_zone", 4, 43)
    c.vis[:] = 1.0
    first = _fwd(c, "mods", 3, want=("uv", "xyz"))
    offs = np.array([0.0, 5e-5, -5e-5, 3e-4, -3e-4])
    for key, tgt in (("uv", "crop_uv"), ("xyz", "pose3d")):
        own = first[key].numpy()
        off = offs[(np.arange(own.size).reshape(own.shape) + np.arange(own.shape[0])[:, None]) % 5]
        setattr(c, tgt, (own.astype(np.float64) + off).astype(np.float32))
        r64 = _ref(c, 3)
        d = getattr(c, tgt).astype(np.float64) - r64[key]
        inside = np.abs(off) < 1e-4
        assert (np.abs(d)[inside] < 1e-4 - 3e-5).all() and (np.abs(d)[~inside] > 1e-4 + 1e-4).all(), key
        assert (np.sign(d[~inside]) == np.sign(off[~inside])).all(), key
        c.name = "dead_zone, %s set" % tgt          # a reference is cached under the case's name: new targets, new name
    r64 = _ref(c, 3, grad=True)
    assert np.abs(r64["g_det"][:, 13:]).max() > 0.0          # the coordinates outside the zone pull on the camera
    c.cham = _objects(c, 9, None)
    ms = _measures("dead zone")
    _all_entries(c, ms)
    _report(ms)


@pytest.mark.gpu
def test_visibility_values_other_than_one_are_masked(gpu_lib):
    """vis rows of 0, 1, 2, 0.5 and 1 + 2^-23: only 1 counts.  Then an all-zero vis: terms[:, 0] (and the xyz term) exactly 0, the gradient is the
    priors' alone - the camera columns of g_det exactly 0, and the same bits whatever the targets are.
    Measured on an MI355X: forward entries 0.155, reverse 0.236 / 0.159 / 0.258; vis = 0: forward 0.155, reverse 0.070"""
    c = _rows_case("vis_values", 5, 44, th45_scale=1.5)
    for r, v in enumerate((0.0, 1.0, 2.0, 0.5, np.float32(1.0) + np.float32(2.0 ** -23))):
        c.vis[r] = v
    assert c.vis[4, 0] != 1.0 and c.vis.dtype == np.float32
    r64 = _ref(c, 3, grad=True)
    assert (r64["terms5"][[0, 2, 3, 4], :2] == 0).all() and (r64["terms5"][1, :2] < -10).all() and (r64["terms5"][:, 3] < 0).all()
    c.cham = _objects(c, 9, None)
    ms = _measures("vis")
    got = _all_entries(c, ms)
    for key in (("f32", 1), ("mods", 3)):
        assert float(got[key]["terms"][[0, 2, 3, 4], 0].abs().max()) == 0.0 and float(got[key]["terms"][1, 0]) < -10.0
    z = _rows_case("vis_zero", 5, 44, th45_scale=1.5)
    z.vis[:] = 0.0
    zs = _measures("vis = 0")
    o = _fwd(z, "mods", 3)
    _add(zs["mhe_mano_joints_mods_f32"], "vis = 0", o, z, 3, KEYS)
    assert float(o["terms"][:, :2].abs().max()) == 0.0
    g = _bwd(z, "mods", 3)
    _add(zs["mhe_mano_joints_mods_bwd_f32"], "vis = 0", g, z, 3, ("g_th45", "g_det"), grad=True)
    assert float(g["g_det"][:, 13:].abs().max()) == 0.0 and float(g["g_th45"].abs().max()) > 0.0
    z.crop_uv, z.pose3d = z.crop_uv + 0.25, z.pose3d - 0.5
    g2 = _bwd(z, "mods", 3)
    assert torch.equal(g2["g_th45"], g["g_th45"]) and torch.equal(g2["g_det"], g["g_det"])
    _report(ms)
    _report(zs)


@pytest.mark.gpu
def test_camera_extremes_and_inv_norm(gpu_lib):
    """log s = +3 and -3 (exp: 20 and 0.05), translations of +-40; inv_norm = True with image_size 256 and 224 in the uv output (and, as the
    kernel defines it, in the uv likelihood).
    Measured on an MI355X: forward entries 0.120 (inv_norm included), reverse 0.181 / 0.192 / 0.129"""
    c = _rows_case("camera", 4, 45)
    c.det[:, 13] = (3.0, -3.0, 3.0, -3.0)
    c.det[:, 14] = (40.0, -40.0, 0.1, 0.0)
    c.det[:, 15] = (-40.0, 0.2, 40.0, 0.0)
    c.cham = _objects(c, 9, None)
    ms = _measures("camera")
    _all_entries(c, ms)
    for size in (256.0, 224.0):
        kw = dict(inv_norm=True, image_size=size)
        o = _fwd(c, "f32", inv_norm=1, image_size=size)
        _add(ms["mhe_mano_joints_f32"], "inv_norm %d" % size, o, c, 1, KEYS, terms="terms4", **kw)
        o = _fwd(c, "mods", 3, inv_norm=1, image_size=size)
        _add(ms["mhe_mano_joints_mods_f32"], "inv_norm %d" % size, o, c, 3, KEYS, **kw)
        r = _ref(c, 3, **kw)
        assert np.array_equal(r["uv"], r["uv_inv"]) and np.abs(r["uv"] - size / 2).max() > size
    _report(ms)


def _plant(xyz, scale, root, obj):
    """image 2: vertex 3 ON the root joint (joint 12, whose normalised coordinates are exactly 0 in the kernel and in the reference: a zero
    distance in both, zero sub-gradient).  Image 3: vertices 4 and 6 at root -+ 2 mm along x, exactly equidistant from joint 12 in both
    arithmetics (the root is on a 1/8 mm grid) - the lowest index wins; vertices 5 and 7 the same point 3 mm from where the reference has joint
    5 of the image's first row: tied for that joint's minimum whatever the rounding, and only one of them may count.  (Two DIFFERENT points
    cannot be exactly equidistant from a joint other than the root in float32 and in float64 at once: the joint itself differs by rounding.)"""
    if obj.shape[1] < 8:
        return
    obj[2, 3] = root[2]
    obj[3, 4], obj[3, 6] = root[3] + np.float32([-2, 0, 0]), root[3] + np.float32([2, 0, 0])
    a5 = xyz[3, 5] * (float(scale[3]) * 1000.0) + root[3]
    obj[3, 5] = obj[3, 7] = (a5 + np.array([3.0, 0.0, 0.0])).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("VO", [1, 64, 65])
def test_chamfer_count_clamp_zero_distance_and_ties(gpu_lib, VO):
    """obj_count = 0 (acts as 1), 1, VO and VO + 5 (acts as VO) on the four images of one launch, in the loss pass and in the reverse;
    a vertex on a joint and tied vertices (see _plant).  VO = 64, 65: the reverse's 64-vertex rounds end exactly / one vertex into the second.
    Measured on an MI355X: mhe_mano_joints_chamfer_f32 0.119 at VO = 1, 64, 65; mhe_mano_joints_chamfer_bwd_f32 0.255, 0.332, 0.454"""
    c = _case("chamfer_VO%d" % VO, 4, 2, 46)
    c.cham = _objects(c, VO, [0, 1, VO, VO + 5], plant=_plant)
    r64 = _ref(c, 3, cham=True, grad=True)
    if VO >= 8:
        xyz = torch.as_tensor(r64["xyz"]).view(-1, 21, 3)
        a = xyz[[2, 3]].numpy() * (c.cham[0][[2, 3]].astype(np.float64) * 1000.0)[:, None, None] + c.cham[1][[2, 3], None, :]
        d = np.linalg.norm(a[:, :, None, :] - c.cham[2][[2, 3]].astype(np.float64)[:, None], axis=-1)          # (2, 21, VO)
        assert d[0, 12, 3] == 0.0 and d[0, 12].argmin() == 3
        assert d[1, 12, 4] == 2.0 and d[1, 12, 6] == 2.0 and d[1, 12].min() == 2.0 and d[1, 5, 5] == d[1, 5, 7] == d[1, 5].min()
    # the clamp is the reference's: the same distances with the counts written out
    same = mr.mano_pass(c.th45, c.det, chamfer=c.cham[:3] + (np.array([1, 1, VO, VO], np.int32),))["dist"]
    assert np.array_equal(same, r64["dist"])
    ms = _measures("chamfer VO = %d" % VO)
    got = _all_entries(c, ms, mods_fwd=(3,), mods_bwd=(3,))
    share = float((got["bwd chamfer", 3]["g_th45"] - got["bwd mods", 3]["g_th45"]).abs().max() / got["bwd chamfer", 3]["g_th45"].abs().max())
    assert share > 1e-2, share          # the term is a visible part of the gradient under test
    for mods in (1, 2):
        o = _fwd(c, "chamfer", mods)
        _add(ms["mhe_mano_joints_chamfer_f32"], "mods %d" % mods, o, c, mods, KEYS + ("dist",), cham=True)
        g = _bwd(c, "chamfer", mods)
        _add(ms["mhe_mano_joints_chamfer_bwd_f32"], "mods %d" % mods, g, c, mods, ("g_th45", "g_det"), cham=True, grad=True)
    _report(ms)


# ---- d. the second trip of the grid-stride loops ------------------------------------------------------------------------------------------------
def _big():
    """B = 1, R = 8199 random rows under tables with hands_mean = 0; row 8192, the first of the second trip, has th45 = 0 (its 15 finger
    axis-angles exactly zero; th3 is the image's), row 8193 lies outside the th45 box (+-2.5, +-5)"""
    c = _case("second_trip", 1, R_BIG, 47, zero_mean=True)
    c.th45[8192] = 0.0
    c.th45[8193] = np.where(np.arange(45) % 2 == 0, 2.5, -5.0)
    return c


@pytest.mark.gpu
def test_rows_past_8192_on_the_second_loop_trip(gpu_lib):
    """R = 8192 + 7 (see R_BIG): every forward output and g_th45 / per-row g_det on rows 0..15 and 8176..8198 against float64 (the pass is
    row-independent: the reference gets just those rows), the sentinel behind row 8198; the four-hypotheses forward 4- and 5-wide (mods uv,
    uv | xyz) and with the Chamfer term, the three reverse instantiations.
    Measured on an MI355X: forward entries 0.197, reverse 0.177 / 0.173 / 0.187; the second trip's rows have the bits of a 7-row launch"""
    c = _big()
    c.cham = _objects(c, 5, [4], rows=ROWS_BIG)
    ms = _measures("R = %d" % R_BIG)
    got = _all_entries(c, ms, rows=ROWS_BIG, mods_fwd=(1, 3), mods_bwd=(3,))
    # both trips of a wave give a row's bits whichever trip it is on: the rows of the second trip alone, as a launch of 7 rows
    tail = _case("second_trip_tail", 1, 7, 47, zero_mean=True)
    tail.th45, tail.det, tail.crop_uv, tail.vis, tail.pose3d, tail.g, tail.N = c.th45[8192:], c.det, c.crop_uv, c.vis, c.pose3d, c.g, c.N
    o = _fwd(tail, "mods", 3)
    for k in KEYS:
        assert torch.equal(o[k], got["mods", 3][k][8192:]), k
    g = _bwd(tail, "mods", 3)
    for k in ("g_th45", "g_det"):
        assert torch.equal(g[k], got["bwd mods", 3][k][8192:]), k
    _report(ms)


# ---- e. MHE_MANO_FOUR=0: read once per process, hence a fresh child ------------------------------------------------------------------------------
def _one_wave_child(out_path):
    """runs in the child: mano_joints_kernel<4> / <5> at the shapes of (a) and at R = 8199 (the sentinel tail is asserted here), and the status and
    message of the two requests this kernel family refuses"""
    from mhentropy_amd import _lib
    res = {}
    for c in [_case("ragged_B%d_N%d" % s, s[0], s[1], 100 * s[0] + s[1]) for s in SHAPES] + [_big()]:
        for entry in ("f32", "mods"):
            for k, v in _fwd(c, entry, 1).items():
                res["%s|%s|%s" % (c.name, entry, k)] = v.numpy() if c.R < R_BIG else v.numpy()[ROWS_BIG]
    c = _case("ragged_B3_N5", 3, 5, 305)
    d = _operands(c)
    o = torch.full((c.R + SPARE, 63), SENT, device="cuda")
    lp = torch.full((c.R + SPARE,), SENT, device="cuda")
    res["rc_xyz"] = np.int64(_raw("mhe_mano_joints_mods_f32", d.th45, d.det, d.crop_uv, d.vis, d.pose3d, d.blob, None, o, None, None, lp, None, None,
                                  c.R, c.B, 3, 0.03, 0.05, 50.0, 0, 256.0))
    res["msg_xyz"] = np.array(_lib.lib().mhe_last_error().decode())
    verts = torch.full((c.R + SPARE, 778 * 3), SENT, device="cuda")
    ws = torch.empty(_lib.lib().mhe_mano_verts_workspace_floats(c.R), device="cuda")
    res["rc_decode"] = np.int64(_raw("mhe_mano_decode_f32", d.th45, d.det, d.crop_uv, d.vis, d.blob, None, o, None, None, lp, None, None, verts, ws,
                                     c.R, c.B, 0.03, 50.0, 0, 256.0, 0))
    res["msg_decode"] = np.array(_lib.lib().mhe_last_error().decode())
    torch.cuda.synchronize()
    res["untouched"] = np.bool_(bool((o == SENT).all()) and bool((lp == SENT).all()) and bool((verts == SENT).all()))
    np.savez(out_path, **res)


@pytest.mark.gpu
def test_one_hypothesis_per_wave_kernels_in_a_fresh_process(gpu_lib):
    """MHE_MANO_FOUR=0 selects mano_joints_kernel<4> (mhe_mano_joints_f32) and <5> (mhe_mano_joints_mods_f32, mods = uv): every output at the
    shapes of (a) and on rows 0..15, 8176..8198 of R = 8199 against the same float64 reference; mods with xyz and mhe_mano_decode_f32 are
    refused with a status and a message, nothing written.
    Measured on an MI355X: mano_joints_kernel<4> 0.197, mano_joints_kernel<5> 0.197"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {here!r}); import test_gpu_mano_edges as T; T._one_wave_child(sys.argv[1])"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "one_wave.npz")
        p = subprocess.run([sys.executable, "-c", code, out], env={**os.environ, "MHE_MANO_FOUR": "0"}, timeout=300, capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        got = dict(np.load(out))
    assert int(got["rc_xyz"]) == 1 and "uv likelihood only" in str(got["msg_xyz"]) and str(got["msg_xyz"]).startswith("mhe_mano_joints_mods_f32")
    assert int(got["rc_decode"]) == 1 and "mhe_mano_decode_f32" in str(got["msg_decode"]) and "MHE_MANO_FOUR" in str(got["msg_decode"])
    assert bool(got["untouched"])
    ms = {"f32": M("mano_joints_kernel<4>"), "mods": M("mano_joints_kernel<5>")}
    for c in [_ragged(*s) for s in SHAPES] + [_big()]:
        rows = ROWS_BIG if c.R == R_BIG else None
        for entry in ("f32", "mods"):
            o = {k: got["%s|%s|%s" % (c.name, entry, k)] for k in KEYS}
            r64, r32 = (_ref(c, 1, dt, rows=rows) for dt in (torch.float64, torch.float32))
            for k in KEYS:
                rk = {"terms": "terms4" if entry == "f32" else "terms5"}.get(k, k)
                ms[entry].add("%s %s" % (c.name, k), o[k], r64[rk], mr.bound(r64, r32, rk))
    for m in ms.values():
        m.report()
