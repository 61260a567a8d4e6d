"""The body-model kernels (csrc/body.hip, csrc/lbs_skin.hip, csrc/lbs_skin_bwd.hip, the skinning half of csrc/body_kp.hip) against the float64
reference of tests/body_edge_ref.py at every size class their launchers distinguish.  The C entries are called directly, on the layouts
BodyLayer.__init__ makes restated at a free pitch VP; every output buffer has SPARE sentinel rows behind R and every launch checks their bits.

  a. pose kernels: mhe_lbs_pose_f32 (the whole workspace row and the joints), mhe_lbs_pose_bwd_f32, mhe_lbs_transforms_bwd_f32 at every model
     class with J >= 2, and at R = 8192 + 7 (the second trip of their grid-stride loops) for (2, 1) and (24, 10)
  b. forward: mhe_lbs_skin_mfma_f32, mhe_lbs_skin_kp_mfma_f32, mhe_lbs_skin_err_mfma_f32 and the scalar-operand mhe_lbs_skin_f32, mhe_lbs_skin_kp_f32,
     mhe_lbs_skin_err_f32 over body_edge_ref.CASES (19 model classes (J, nb) x 2 of the 9 vertex classes (NV, VP); rows 1, 31, 32, 33, 65; scales
     1, -2.5, 1000; 1, 31, 32, 33, 64 keypoints with and without a vertex tensor; B = 1 and B = R) and ERR_CASES (32, 16 and 48 rows per image)
  c. exact cases: the dyadic models through all six entries, bit-equal to the reference; error against the reference vertices exactly 0
  d. padding isolation: the table columns NV..VP-1 filled with 1e3 give the bits of the zero-padded run, forward, reverse and table builders
  e. determinism: a second set of launches gives the same bits
  f. reverse: mhe_lbs_bwd_tables_f32 (a re-arrangement: bound 0), mhe_lbs_skin_bwd_f32 at every launch_coef<NT>, mhe_lbs_keypoints_bwd_f32

Bounds: none comes from the kernels.  Per tensor and case max(3 max|f32 reference - f64 reference|, 2e-6 max|f64 reference|)
(body_edge_ref.bound: the rule of test_generic_lbs_at_smpl_size_matches_oracle and test_gpu_mano_edges.py); the exact cases have bound 0.  The
largest |diff| / bound of every entry is printed before it is asserted (`pytest -s`).

Where mhe_lbs_skin_kp_supported says 0 - (32, 64): the pieces, store tiles and staging tiles take 165,888 bytes of LDS, above 160 KiB - the
matrix-core keypoint entry must refuse and write nothing; the scalar entry is then the one under test.  J = 1 has no pose-blend table: the entries
refuse a null v_posedirs, so the test passes one unused float.

The exact cases compare bits with -0 and +0 taken as one number (a sum of signed zeros takes its sign from where the sum starts); the padding and
determinism tests compare raw bits.

The one bound that is wider than the rule: the vertex error.  err is a mean of Euclidean norms, 1-Lipschitz in every vertex, and the vertices it is
taken from are themselves only asked to be within rule(vertices) =: bv, so another correct f32 evaluation may differ by sqrt(3) bv; rule(err) alone
is 3 times ONE f32 draw of that cancellation and with NV = 1 (one norm per row, a target 2 % away) a draw can be small.  Bound: rule(err) +
sqrt(3) bv.  Under rule(err) alone the largest ratios were 1.927 (mhe_lbs_skin_err_mfma_f32, J3_nb13_NV1_VP32; its vertex was at 0.48 of bv) and
0.750 (mhe_lbs_skin_err_f32); under the bound used they are 0.227 and 0.139.  No other bound was widened, no kernel and no predicate was changed:
the new size classes turned up no wrong result.

Measured on an MI355X, the largest |diff| / bound per entry over every test of this file:
  mhe_lbs_pose_f32 0.176 (R = 8199: 0.094)   mhe_lbs_pose_bwd_f32 0.336 (0.084)   mhe_lbs_transforms_bwd_f32 0.269 (0.226)
  mhe_lbs_skin_mfma_f32 0.500   mhe_lbs_skin_kp_mfma_f32 0.703   mhe_lbs_skin_err_mfma_f32 0.227
  mhe_lbs_skin_f32 0.529   mhe_lbs_skin_kp_f32 0.529   mhe_lbs_skin_err_f32 0.139
  mhe_lbs_bwd_tables_f32 0 (exact)   mhe_lbs_skin_bwd_f32 0.236   mhe_lbs_keypoints_bwd_f32 0.141
  exact cases, padding isolation, determinism: every comparison bit-equal
Sensitivity (one-token changes of values - never of an address, a bound, a loop count or a launch size - in a scratch build, each run once through
this file):
  lbs_skin.hip, keypoint product `MFMA(ah, Kf[s][n][2], ..)` -> `MFMA(al, ..)`: test_forward_entries (mhe_lbs_skin_kp_mfma_f32 at 1.408); not the
    exact cases, whose one-hot regressor has no third piece
  lbs_skin.hip, blend product `MFMA(am, Bf[d][2 * c], ..)` -> `Bf[d][2 * c + 1]`: test_forward_entries (mhe_lbs_skin_mfma_f32 at 9.3); not the exact
    cases, whose coefficients have no second piece
  lbs_skin.hip, transform product `MFMA(gh, Wp[js][0], ..)` -> `Wp[0][0]` (the second joint k-step with the first one's weights):
    test_forward_entries and test_exact_cases, from the first JS = 2 model on (95 of 96 values of J20_nb10_NV1_VP32)
  body.hip, lbs_skin_vertex `affine_row(.., acc[h][0], .., acc[h][1], ..)` with the two swapped: test_forward_entries and test_exact_cases (scalar entries)
  body.hip, lbs_pose_bwd_kernel `GJ[3 * p + c] -= u` -> `+= u`: test_pose_kernels and test_pose_kernels_second_loop_trip (g_betas)
  lbs_skin_bwd.hip, `MFMA32(ua[a] * xb[bb], ..)` -> `ua[bb] * xb[a]`: test_reverse_entries (g_tf)
  lbs_skin.hip, lbs_split_tables_kernel `h = k == NP + nb ? th : tl` -> `tl : th`: NOT caught, and cannot be: both template slots meet a coefficient
    of 1.0 in the same accumulator, so the pieces th, tm, tl are added whichever slot holds them - an equivalent program
`(J + 1) / 2` -> `J / 2` in lbs_skin_bwd.hip was not tried: JK sets a loop count and JP an LDS pitch.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import body_edge_ref as br
from edge_measure import Measure

pytestmark = pytest.mark.gpu
SENT, SPARE = br.SENT, br.SPARE
SENT_BITS = int(np.float32(SENT).view(np.int32))
BY_NAME = {c["name"]: c for c in br.CASES + br.ERR_CASES}
FWD = ("mhe_lbs_skin_mfma_f32", "mhe_lbs_skin_kp_mfma_f32", "mhe_lbs_skin_err_mfma_f32", "mhe_lbs_skin_f32", "mhe_lbs_skin_kp_f32", "mhe_lbs_skin_err_f32")


def M(kernel):
    return Measure(kernel, "body-edges")


def _dev(a):
    return None if a is None else torch.as_tensor(np.array(a, order="C")).cuda()          # a C-ordered copy: the entries take dense row-major memory


def _launch(entry, *args):
    from mhentropy_amd import ops
    ops.launch(entry, *args)          # _lib.lib(), ops._ptr per tensor, the current stream, ops.check
    torch.cuda.synchronize()


def _buf(rows, width):
    return torch.full((rows + SPARE, width), SENT, device="cuda")


def _take(t, rows, what):
    """the first `rows` rows of an output buffer (float32 numpy), after checking that every row behind them still holds the sentinel's bits"""
    t = t.cpu()
    assert bool((t[rows:].view(torch.int32) == SENT_BITS).all()), "%s: written behind row %d" % (what, rows)
    return t[:rows].numpy().copy()


# ---- models and inputs on the device ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _model(name, dyadic=False, fill=0.0):
    """the kernel-side tables of a case and what the table builders make of them (split, ksplit, bwd), their sizes checked against the helper's"""
    from mhentropy_amd import _lib
    L, c = _lib.lib(), BY_NAME[name]
    J, nb, NV, VP, NK = c["J"], c["nb"], c["NV"], c["VP"], c["NK"]
    t = br.tables(c["seed"], NV, J, nb, NK, dyadic)
    m = SimpleNamespace(t=t, **{k: _dev(v) for k, v in br.layouts(t, VP, fill).items()})
    if J == 1:
        m.vpd = torch.zeros(1, device="cuda")          # no pose-blend coefficients: never read, but the entries refuse a null pointer
    assert L.mhe_lbs_workspace_floats(c["R"], J, nb) == c["R"] * br.ws_stride(J, nb)
    n = L.mhe_lbs_split_floats(J, nb, VP)
    assert n == br.split_floats(J, nb, VP), (name, n)
    m.split = _buf(n, 1)
    _launch("mhe_lbs_split_tables_f32", m.vt, m.vsd, m.vpd, m.vw, m.split, J, nb, VP)
    _take(m.split, n, name + " split tables")
    if NK:
        m.reg = _dev(t["keypoint_regressor"])
        n = L.mhe_lbs_kp_split_floats(NK, VP)
        assert n == br.kp_split_floats(NK, VP), (name, n)
        m.ksplit = _buf(n, 1)
        _launch("mhe_lbs_kp_split_tables_f32", m.reg, m.ksplit, NK, NV, VP)
        _take(m.ksplit, n, name + " keypoint split tables")
    if J >= 2:
        n = L.mhe_lbs_bwd_tables_floats(J, nb, VP)
        assert n == br.bwd_tables_floats(J, nb, VP), (name, n)
        m.bwd = _buf(n, 1)
        _launch("mhe_lbs_bwd_tables_f32", m.vsd, m.vpd, m.vw, m.bwd, J, nb, NV, VP)
        m.bwd_host = _take(m.bwd, n, name + " reverse tables")[:, 0]
    else:
        assert L.mhe_lbs_bwd_tables_floats(J, nb, VP) == 0          # the reverse takes 1 < J
    return m


def _scale(c, dyadic):
    return c["scale"] if not dyadic else (0.5, 4.0)[c["seed"] % 2]


def _pose(name, dyadic=False, R=None):
    """mhe_lbs_pose_f32 on the case's rows -> (workspace buffer on the device, ws (R, stride) and joints (R, 3 J) float32 numpy)"""
    c, m = BY_NAME[name], _model(name, dyadic)
    R = c["R"] if R is None else R
    J, nb = c["J"], c["nb"]
    rot, betas = br.inputs(c["seed"], R, J, nb, dyadic)
    ws, joints = _buf(R, br.ws_stride(J, nb)), _buf(R, 3 * J)
    _launch("mhe_lbs_pose_f32", _dev(rot), _dev(betas), m.jt, m.jsd, m.parents, ws, joints, R, J, nb)
    w, j = _take(ws, R, name + " workspace"), _take(joints, R, name + " joints")
    used = 9 * (J - 1) + nb + 15 * J
    assert (w[:, used:].view(np.int32) == SENT_BITS).all(), name + ": the workspace row's padding was written"
    return ws, w[:, :used], j


@functools.lru_cache(None)
def _ref(name, dyadic=False, f32=False):
    c = BY_NAME[name]
    t = br.tables(c["seed"], c["NV"], c["J"], c["nb"], c["NK"], dyadic)
    rot, betas = br.inputs(c["seed"], c["R"], c["J"], c["nb"], dyadic)
    return br.forward(t, rot, betas, _scale(c, dyadic), torch.float32 if f32 else torch.float64)


@functools.lru_cache(None)
def _err_inputs(name, dyadic=False):
    """(target (B, NV, 3), center (R, 3) or None, B).  Random model: the target is an image's first hypothesis, perturbed by 2 % of the scale (the
    other hypotheses of an image are other poses); CASES alternate B = 1 / B = R and a null / given centre.  Dyadic: B = R, the reference vertices"""
    c = BY_NAME[name]
    R, k = c["R"], c["seed"] % 100
    v = _ref(name, dyadic)["verts"]
    if dyadic:
        return v.astype(np.float32), None, R
    B = c.get("B", 1 if k % 2 == 0 else R)
    rng = np.random.default_rng(c["seed"] + 9300)
    s = abs(c["scale"])
    target = (v[::R // B] + rng.normal(0, 0.02 * s, (B, c["NV"], 3))).astype(np.float32)
    center = rng.normal(0, 0.05 * s, (R, 3)).astype(np.float32) if (k // 2) % 2 else None
    return target, center, B


def _err_ref(name, dyadic, f32):
    c, (target, center, B) = BY_NAME[name], _err_inputs(name, dyadic)
    dt = torch.float32 if f32 else torch.float64
    cv = lambda a: None if a is None else torch.as_tensor(np.array(a)).to(dt)
    return br.err_rows(cv(_ref(name, dyadic, f32)["verts"]), cv(target), cv(center), 1.0, c["R"] // B).double().numpy()


@functools.lru_cache(None)
def _forward(name, dyadic=False, fill=0.0, fresh=0):
    """the pose kernel, then all six forward entries on its workspace rows -> {key: float32 numpy}: verts of the three vertex-writing entries, kp with
    and without a vertex tensor, err.  `fresh` is a cache key only: another set of launches"""
    from mhentropy_amd import _lib
    L, c, m = _lib.lib(), BY_NAME[name], _model(name, dyadic, fill)
    J, nb, NV, VP, NK, R, scale = c["J"], c["nb"], c["NV"], c["VP"], c["NK"], c["R"], _scale(c, dyadic)
    ws, w, j = _pose(name, dyadic)
    out = {"ws": w, "joints": j}
    assert L.mhe_lbs_skin_mfma_supported(R, J, nb, NV, VP) == int(br.skin_lds(J, nb) <= br.LDS_LIMIT) == 1
    v = _buf(R, NV * 3)
    _launch("mhe_lbs_skin_mfma_f32", ws, m.split, v, R, J, nb, NV, VP, scale)
    out["mfma.verts"] = _take(v, R, name + " skin_mfma")
    v = _buf(R, NV * 3)
    _launch("mhe_lbs_skin_f32", ws, m.vt, m.vsd, m.vpd, m.vw, v, R, J, nb, NV, VP, scale)
    out["scalar.verts"] = _take(v, R, name + " skin")
    for want in (1, 0) if NK else ():
        tag = ".kp" if want else ".kp_only"
        ok = L.mhe_lbs_skin_kp_supported(R, J, nb, NV, VP, NK, want)
        assert ok == int(br.kp_lds(J, nb, NK) <= br.LDS_LIMIT), (name, ok, br.kp_lds(J, nb, NK))
        v, k = _buf(R, NV * 3) if want else None, _buf(R, NK * 3)
        if ok:
            _launch("mhe_lbs_skin_kp_mfma_f32", ws, m.split, m.ksplit, v, k, R, J, nb, NV, VP, NK, scale)
            out["mfma" + tag] = _take(k, R, name + " kp_mfma keypoints")
            if want:
                out["mfma.kp_verts"] = _take(v, R, name + " kp_mfma verts")
        else:          # the entry refuses with a message and launches nothing
            from mhentropy_amd import ops
            rc = L.mhe_lbs_skin_kp_mfma_f32(ops._ptr(ws), ops._ptr(m.split), ops._ptr(m.ksplit), ops._ptr(v), ops._ptr(k), R, J, nb, NV, VP, NK, scale, ops._stream())
            torch.cuda.synchronize()
            assert rc != 0 and b"not supported" in L.mhe_last_error(), name
            assert bool((k.cpu().view(torch.int32) == SENT_BITS).all()), name + ": the refused launch wrote keypoints"
        v, k = _buf(R, NV * 3) if want else None, _buf(R, NK * 3)
        _launch("mhe_lbs_skin_kp_f32", ws, m.vt, m.vsd, m.vpd, m.vw, m.reg, v, k, R, J, nb, NV, VP, NK, scale)
        out["scalar" + tag] = _take(k, R, name + " kp keypoints")
        if want:
            out["scalar.kp_verts"] = _take(v, R, name + " kp verts")
    variants = [_err_inputs(name, dyadic)]
    if dyadic:
        variants.append((variants[0][0][:1], None, 1))          # one image: only row 0 is its own target
    for i, (target, center, B) in enumerate(variants):
        assert L.mhe_lbs_skin_err_supported(R, J, nb, NV, VP, B) == 1
        tg, cn = _dev(target), _dev(center)
        e = _buf(R, 1)
        _launch("mhe_lbs_skin_err_mfma_f32", ws, m.split, tg, cn, e, R, B, J, nb, NV, VP, scale)
        out["mfma.err%d" % i] = _take(e, R, name + " err_mfma")[:, 0]
        e = _buf(R, 1)
        _launch("mhe_lbs_skin_err_f32", ws, m.vt, m.vsd, m.vpd, m.vw, tg, cn, e, R, B, J, nb, NV, VP, scale)
        out["scalar.err%d" % i] = _take(e, R, name + " err")[:, 0]
    return out


def _rev_inputs(name):
    c = BY_NAME[name]
    rng = np.random.default_rng(c["seed"] + 9400)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    return f(c["R"], c["NV"], 3), f(c["R"], c["NK"], 3)


@functools.lru_cache(None)
def _reverse(name, fill=0.0, fresh=0):
    """mhe_lbs_skin_bwd_f32 on random vertex gradients (with the reverse tables of the case's padding fill), mhe_lbs_keypoints_bwd_f32 with
    accumulate 0 and 1 -> {key: float32 numpy}"""
    c, m = BY_NAME[name], _model(name, False, fill)
    J, nb, NV, VP, NK, R = c["J"], c["nb"], c["NV"], c["VP"], c["NK"], c["R"]
    ws = _pose(name)[0]
    gv, gk = _rev_inputs(name)
    g_tf, g_pm, g_bt = _buf(R, J * 12), _buf(R, 9 * (J - 1)), _buf(R, nb)
    _launch("mhe_lbs_skin_bwd_f32", ws, m.vt, m.vsd, m.vpd, m.vw, m.bwd, _dev(gv), g_tf, g_pm, g_bt, R, J, nb, NV, VP, c["scale"])
    out = {"tables": m.bwd_host, "g_tf": _take(g_tf, R, name + " g_transforms"), "g_pm": _take(g_pm, R, name + " g_posemap"),
           "g_bt": _take(g_bt, R, name + " g_betas")}
    for acc in (0, 1):
        o = _buf(R, NV * 3)
        o[:R] = _dev(gv).view(R, NV * 3) if acc else SENT
        _launch("mhe_lbs_keypoints_bwd_f32", m.reg, _dev(gk), o, R, NK, NV, acc)
        out["gv%d" % acc] = _take(o, R, name + " keypoints_bwd")
    return out


def _same_bits(a, b, what, zero_sign=True):
    """zero_sign=False: -0 and +0 count as the same number (a sum of signed zeros takes its sign from the order and the start of the sum)"""
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, what
    if not zero_sign:
        a, b = a + np.float32(0), b + np.float32(0)
    bad = a.view(np.int32) != b.view(np.int32)
    assert not bad.any(), "%s: %d of %d values differ in their bits, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], a[tuple(np.argwhere(bad)[0])], b[tuple(np.argwhere(bad)[0])])


# ---- a. pose kernels -----------------------------------------------------------------------------------------------------------------------------
def _pose_case(ms, name, R=None, rows=None):
    """the three pose entries on the rows of case `name` (R rows; the reference on `rows` only)"""
    c, m = BY_NAME[name], _model(name)
    J, nb = c["J"], c["nb"]
    R = c["R"] if R is None else R
    rows = np.arange(R) if rows is None else rows
    rot, betas = br.inputs(c["seed"], R, J, nb)
    _, w, j = _pose(name, R=R)
    ref = [br.forward(m.t, rot[rows], betas[rows], 1.0, dt) for dt in (torch.float64, torch.float32)]
    NP = 9 * (J - 1)
    for key, lo, hi in (("pm", 0, NP), ("betas", NP, NP + nb), ("A", NP + nb, NP + nb + 12 * J), ("joints", NP + nb + 12 * J, NP + nb + 15 * J)):
        ms[0].add("%s R=%d %s" % (name, R, key), w[rows, lo:hi], ref[0]["ws"][:, lo:hi], br.bound(ref[0]["ws"][:, lo:hi], ref[1]["ws"][:, lo:hi]))
    ms[0].add("%s R=%d joints out" % (name, R), j[rows], ref[0]["joints"].reshape(len(rows), -1), br.bound(ref[0]["joints"], ref[1]["joints"]))
    rng = np.random.default_rng(c["seed"] + 9500)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    gj, gtf, gpm, gbi = f(R, J, 3), f(R, J, 12), f(R, NP), f(R, nb)
    d_rot, d_bt = _dev(rot), _dev(betas)
    g_rot, g_bt = _buf(R, J * 9), _buf(R, nb)
    _launch("mhe_lbs_pose_bwd_f32", d_rot, d_bt, m.jt, m.jsd, m.parents, _dev(gj), g_rot, g_bt, R, J, nb)
    got = {"g_rot": _take(g_rot, R, name + " pose_bwd g_rotmats"), "g_betas": _take(g_bt, R, name + " pose_bwd g_betas")}
    ref = [br.reverse(m.t, rot[rows], betas[rows], g_joints=gj[rows], dtype=dt) for dt in (torch.float64, torch.float32)]
    for key in got:
        ms[1].add("%s R=%d %s" % (name, R, key), got[key][rows], ref[0][key].reshape(len(rows), -1), br.bound(ref[0][key], ref[1][key]))
    with_j, with_b = c["seed"] % 2 == 0, c["seed"] % 3 != 0          # g_joints / g_betas_in given or null
    g_rot, g_bt = _buf(R, J * 9), _buf(R, nb)
    _launch("mhe_lbs_transforms_bwd_f32", d_rot, d_bt, m.jt, m.jsd, m.parents, _dev(gj) if with_j else None, _dev(gtf), _dev(gpm),
            _dev(gbi) if with_b else None, g_rot, g_bt, R, J, nb)
    got = {"g_rot": _take(g_rot, R, name + " transforms_bwd g_rotmats"), "g_betas": _take(g_bt, R, name + " transforms_bwd g_betas")}
    ref = [br.transforms_reverse(m.t, rot[rows], betas[rows], gtf[rows], gpm[rows], gj[rows] if with_j else None, gbi[rows] if with_b else None, dt)
           for dt in (torch.float64, torch.float32)]
    for key in got:
        ms[2].add("%s R=%d %s" % (name, R, key), got[key][rows], ref[0][key].reshape(len(rows), -1), br.bound(ref[0][key], ref[1][key]))


def test_pose_kernels():
    ms = [M("mhe_lbs_pose_f32"), M("mhe_lbs_pose_bwd_f32"), M("mhe_lbs_transforms_bwd_f32")]
    for c in br.CASES:
        if c["J"] >= 2:
            _pose_case(ms, c["name"])
    for m in ms:
        m.report()


def test_pose_kernels_second_loop_trip():
    """R = 8192 + 7: rows 8192 .. 8198 are a workgroup's second trip; rows 0..15 and the last 23 are compared"""
    ms = [M("mhe_lbs_pose_f32 (R = 8199)"), M("mhe_lbs_pose_bwd_f32 (R = 8199)"), M("mhe_lbs_transforms_bwd_f32 (R = 8199)")]
    for J, nb in br.BIG_MODELS:
        name = next(c["name"] for c in br.CASES if (c["J"], c["nb"]) == (J, nb))
        _pose_case(ms, name, br.R_BIG, br.ROWS_BIG)
    for m in ms:
        m.report()


# ---- b. forward ----------------------------------------------------------------------------------------------------------------------------------
def test_forward_entries():
    ms = {e: M(e) for e in FWD}
    for c in br.CASES + br.ERR_CASES:
        name = c["name"]
        got, r64, r32 = _forward(name), _ref(name), _ref(name, f32=True)
        flat = lambda a: a.reshape(c["R"], -1)
        bv = br.bound(r64["verts"], r32["verts"])
        ms[FWD[0]].add(name + " verts", got["mfma.verts"], flat(r64["verts"]), bv)
        ms[FWD[3]].add(name + " verts", got["scalar.verts"], flat(r64["verts"]), bv)
        if c["NK"]:
            bk = br.bound(r64["kp"], r32["kp"])
            for path, e in (("mfma", FWD[1]), ("scalar", FWD[4])):
                for key in (".kp", ".kp_only"):
                    if path + key in got:
                        ms[e].add(name + key, got[path + key], flat(r64["kp"]), bk)
                if path + ".kp_verts" in got:
                    ms[e].add(name + " verts", got[path + ".kp_verts"], flat(r64["verts"]), bv)
            assert ("mfma.kp" in got) == ((c["J"], c["nb"]) != (32, 64)), name
            if "mfma.kp" in got:          # the keypoint variant's vertices are the plain kernel's, with and without them its keypoints are the same
                _same_bits(got["mfma.kp_verts"], got["mfma.verts"], name + " kp_mfma verts against skin_mfma")
                _same_bits(got["mfma.kp"], got["mfma.kp_only"], name + " kp_mfma with / without a vertex tensor")
            _same_bits(got["scalar.kp_verts"], got["scalar.verts"], name + " kp verts against skin")
            _same_bits(got["scalar.kp"], got["scalar.kp_only"], name + " kp with / without a vertex tensor")
        e64, e32 = _err_ref(name, False, False), _err_ref(name, False, True)
        be = br.bound(e64, e32) + np.sqrt(3.0) * bv          # the rule, and what the rule allows the vertices (see the module's docstring)
        ms[FWD[2]].add(name + " err", got["mfma.err0"], e64, be)
        ms[FWD[5]].add(name + " err", got["scalar.err0"], e64, be)
    for m in ms.values():
        m.report()


# ---- c. exact cases ------------------------------------------------------------------------------------------------------------------------------
def test_exact_cases():
    """the dyadic models: every product and partial sum is representable (tests/test_body_edge_ref_host.py), in the scalar kernels' fmaf chains and
    in the matrix-core kernels, whose bf16 pieces of these operands are exact (values of at most 8 significant bits have no second piece; the
    transforms' translations, of at most 19 bits, and the staged vertices fill three) and whose sums over k add exact products to representable
    partial sums.  So vertices, keypoints and the pose kernel's row are the reference's bits and a vertex error against them is exactly 0"""
    for c in br.CASES:
        name = c["name"]
        got, ref = _forward(name, True), _ref(name, True)
        f = lambda a: a.reshape(c["R"], -1).astype(np.float32)
        assert np.array_equal(f(ref["verts"]).astype(np.float64), ref["verts"].reshape(c["R"], -1))
        _same_bits(got["ws"], f(ref["ws"]), name + " workspace row", False)
        _same_bits(got["joints"], f(ref["joints"]), name + " joints", False)
        for key in ("mfma.verts", "scalar.verts", "mfma.kp_verts", "scalar.kp_verts"):
            if key in got:
                _same_bits(got[key], f(ref["verts"]), name + " " + key, False)
        for key in ("mfma.kp", "mfma.kp_only", "scalar.kp", "scalar.kp_only"):
            if key in got:
                _same_bits(got[key], f(ref["kp"]), name + " " + key, False)
        assert ("mfma.kp" in got) == ((c["J"], c["nb"]) != (32, 64)), name
        for path in ("mfma", "scalar"):
            assert (got[path + ".err0"] == 0).all(), (name, path, "error against the reference vertices", got[path + ".err0"])
            assert got[path + ".err1"][0] == 0, (name, path, "row 0 against its own vertices, one image", got[path + ".err1"][0])


# ---- d. padding isolation, e. determinism ----------------------------------------------------------------------------------------------------------
def test_padding_isolation():
    """the table columns NV .. VP-1 filled with 1e3: forward (lanes without a vertex compute finite values that only a zero regressor piece, a select
    or a store mask keep out), the reverse and both table builders' zero-past-NV give the bits of the zero-padded run"""
    for c in br.CASES + br.ERR_CASES:
        a, b = _forward(c["name"]), _forward(c["name"], fill=1e3)
        assert a.keys() == b.keys()
        for key in a:
            _same_bits(a[key], b[key], "%s %s with the padding at 1e3" % (c["name"], key))
    for c in br.CASES:
        if c["J"] >= 2:
            a, b = _reverse(c["name"]), _reverse(c["name"], fill=1e3)
            for key in a:
                _same_bits(a[key], b[key], "%s reverse %s with the padding at 1e3" % (c["name"], key))


def test_two_launches_give_the_same_bits():
    for c in br.CASES + br.ERR_CASES:
        a, b = _forward(c["name"]), _forward(c["name"], fresh=1)
        for key in a:
            _same_bits(a[key], b[key], "%s %s, second launch" % (c["name"], key))
    for c in br.CASES:
        if c["J"] >= 2:
            a, b = _reverse(c["name"]), _reverse(c["name"], fresh=1)
            for key in a:
                _same_bits(a[key], b[key], "%s reverse %s, second launch" % (c["name"], key))


# ---- f. reverse ----------------------------------------------------------------------------------------------------------------------------------
def test_reverse_entries():
    ms = [M("mhe_lbs_bwd_tables_f32"), M("mhe_lbs_skin_bwd_f32"), M("mhe_lbs_keypoints_bwd_f32")]
    seen = set()
    for c in br.CASES:
        if c["J"] < 2:
            continue
        name, R = c["name"], c["R"]
        seen.add(br.nt(c["J"], c["nb"]))
        got = _reverse(name)
        t = br.tables(c["seed"], c["NV"], c["J"], c["nb"], c["NK"])
        rot, betas = br.inputs(c["seed"], R, c["J"], c["nb"])
        gv, gk = _rev_inputs(name)
        ms[0].add(name, got["tables"], br.bwd_tables(t, c["VP"]), 0.0)
        ref = [br.reverse(t, rot, betas, c["scale"], g_verts=gv, dtype=dt) for dt in (torch.float64, torch.float32)]
        for key in ("g_tf", "g_pm", "g_bt"):
            ms[1].add(name + " " + key, got[key], ref[0][key].reshape(R, -1), br.bound(ref[0][key], ref[1][key]))
        for acc in (0, 1):
            ref = [br.keypoints_reverse(t, gk, gv if acc else None, dt) for dt in (torch.float64, torch.float32)]
            ms[2].add("%s accumulate=%d" % (name, acc), got["gv%d" % acc], ref[0].reshape(R, -1), br.bound(ref[0], ref[1]))
    assert seen == set(range(1, 12))          # every launch_coef<NT> ran
    for m in ms:
        m.report()
