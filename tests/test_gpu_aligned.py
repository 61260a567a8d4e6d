"""GPU: the aligned evaluation (MHEntLoss(aligned=True), hand/criteria.py:62-87, align_w_scale hand/utils.py:502-525) through every
layer - the Procrustes kernels (csrc/procrustes.hip) against the reference-generated fixtures tests/golden/criteria_aligned_*.npz and the
float64 restatement, the split metrics entry point, the criterion, graph capture, and argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, assert_close
from mhentropy_amd import synth
from test_aligned_oracle import align_f64

pytestmark = pytest.mark.gpu
# Tolerances, relative to the largest |coordinate| of the compared tensor unless stated.  Measured on MI355X against the float64
# restatement: aligned rows 1.4e-7 (joints, N=200 B=256) and 1.0e-7 (meshes, N=200 B=16), R 1.7e-7 absolute; the reference's own
# float32 rows sit up to 8e-7 from float64 (test_aligned_oracle).
TOL_ALIGN = 4e-6
TOL_R = 2e-5          # absolute, on R's entries
TOL_METRIC = 5e-5     # the 14 metrics against the reference's (the suite's ceiling is 5e-4)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def _hands(rng, B, P, N):
    """targets ~0.6 m from the origin at a ~0.1 m extent (HO3D metres), hypotheses in normalised units: rotated, scaled, shifted and
    perturbed copies of the target shape"""
    shape = rng.normal(0, 0.03, (B, P, 3))
    tgt = shape + np.array([0.05, -0.1, 0.6]) + rng.normal(0, 0.02, (B, 1, 3))
    pred = np.empty((N, B, P, 3))
    for b in range(B):
        Q = _rot(rng)
        pred[:, b] = (shape[b] @ Q.T) * 30.0 + rng.normal(0, 0.3, (N, 1, 3)) + rng.normal(0, 0.2, (N, P, 3))
    return tgt.reshape(B, -1).astype(np.float32), pred.reshape(N, B, -1).astype(np.float32)


@pytest.mark.parametrize("tag", ["small", "shipped"])
@pytest.mark.parametrize("case", ["base", "mirror"])
def test_align_kernel_matches_reference_vectors(gpu_lib, tag, case):
    """joints (rows_kernel) and meshes (wave_kernel) against the reference's aligned outputs, R and s; the mirror case keeps det R = -1"""
    from mhentropy_amd import ops
    g, d = load_golden(f"criteria_aligned_{tag}"), load_golden(f"mhent_{tag}")
    for lbl, src in (("xyz", "sample_xyz"), ("verts", "sample_verts")):
        tgt = g[f"{case}_pose3d"] if lbl == "xyz" else g[f"{case}_verts"]
        out, R, s = ops.procrustes_align(_dev(d[src]), _dev(tgt), want_transform=True)
        assert_close(out.cpu(), g[f"{case}_{lbl}_aligned"], TOL_ALIGN, what=f"{case} {lbl} aligned")
        assert_close(R.cpu(), g[f"{case}_R_{lbl}"], 0, TOL_R, what=f"{case} {lbl} R")
        assert_close(s.cpu(), g[f"{case}_s_{lbl}"], 1e-5, what=f"{case} {lbl} s")
        if case == "mirror":
            assert (torch.linalg.det(R[0].double()) < -0.999).all()


@pytest.mark.parametrize("lbl,N,B,P", [("joints", 200, 256, 21), ("verts", 200, 16, 778)])
def test_align_kernel_vs_f64_at_metrics_pass_size(gpu_lib, lbl, N, B, P):
    """the iteration's metrics pass (N = 200, B = 256 joints) and a mesh batch (N = 200, B = 16) against the float64 restatement"""
    from mhentropy_amd import ops
    tgt, pred = _hands(np.random.default_rng(P), B, P, N)
    out, R, s = ops.procrustes_align(_dev(pred), _dev(tgt), want_transform=True)
    al, R64, s64 = align_f64(tgt, pred)
    err = np.abs(out.cpu().numpy() - al).max() / np.abs(al).max()
    print(f"{lbl}: max rel err vs f64 {err:.2e}, R {np.abs(R.cpu().numpy() - R64).max():.2e}")
    assert err <= TOL_ALIGN
    assert_close(R.cpu(), R64, 0, TOL_R, what="R")
    assert_close(s.cpu(), s64, 1e-5, what="s")


@pytest.mark.parametrize("P", [21, 778])
def test_rigid_mirrored_and_zero_targets(gpu_lib, P):
    """a rigidly transformed and scaled copy aligns back onto the target (error ~0); a mirrored copy does too, with det R = -1 as in
    scipy; an all-zero target gives s = 0 and exactly t1 = 0, finite"""
    from mhentropy_amd import ops
    rng = np.random.default_rng(11)
    N, B = 5, 3
    tgt = (rng.normal(0, 0.03, (B, P, 3)) + np.array([0.1, 0.2, 0.6])).astype(np.float32)
    rig, mir = np.empty((N, B, P, 3)), np.empty((N, B, P, 3))
    for n in range(N):
        for b in range(B):
            Q = _rot(rng)
            rig[n, b] = tgt[b] @ Q.T * 25.0 + rng.normal(0, 1, 3)
            mir[n, b] = tgt[b] @ (Q @ np.diag([1.0, -1.0, 1.0])).T * 25.0 + rng.normal(0, 1, 3)
    tt = _dev(tgt.reshape(B, -1))
    for name, pred, det in (("rigid", rig, 1.0), ("mirror", mir, -1.0)):
        out, R, s = ops.procrustes_align(_dev(pred.reshape(N, B, -1).astype(np.float32)), tt, want_transform=True)
        err = (out.cpu().reshape(N, B, P, 3) - torch.as_tensor(tgt)[None]).abs().max().item()
        assert err < 1e-6, (name, err)                      # metres, on a 0.6 m offset (f32 ulp there: 6e-8)
        assert torch.allclose(torch.linalg.det(R.double().cpu()), torch.full((N, B), det, dtype=torch.float64), atol=1e-5), name
    out, R, s = ops.procrustes_align(_dev(rig.reshape(N, B, -1).astype(np.float32)), torch.zeros(B, P * 3, device="cuda"),
                                     want_transform=True)
    assert torch.isfinite(out).all() and torch.isfinite(R).all()
    assert torch.equal(s, torch.zeros_like(s)) and torch.equal(out, torch.zeros_like(out))
    # a target of one point repeated: t1 exactly, wherever it is
    t1 = torch.tensor([0.1, -0.2, 0.7], device="cuda")
    out = ops.procrustes_align(_dev(rig.reshape(N, B, -1).astype(np.float32)), t1.repeat(B, P))
    assert torch.equal(out.reshape(N, B, P, 3), t1.expand(N, B, P, 3))


def _criterion_inputs(d, g, case):
    out = {"log_p": _dev(d["loss_log_p"]), "xyz": _dev(d["sample_xyz"]), "uv": _dev(d["sample_uv"]), "verts": _dev(d["sample_verts"])}
    y = {k: _dev(d["y_" + k]) for k in ("crop_uv", "vis", "st", "scale")}
    y["pose3d"], y["verts"] = _dev(g[f"{case}_pose3d"]), _dev(g[f"{case}_verts"])
    return out, y


@pytest.mark.parametrize("tag", ["small", "shipped"])
@pytest.mark.parametrize("case", ["base", "mirror"])
def test_criterion_aligned_matches_reference(gpu_lib, tag, case):
    """MHEntLoss(aligned=True): the 14 metrics and the aligned xyz / verts written into the caller's dict against the reference; the
    tensors passed in are not written"""
    from mhentropy_amd.criteria import MHEntLoss
    g, d = load_golden(f"criteria_aligned_{tag}"), load_golden(f"mhent_{tag}")
    out, y = _criterion_inputs(d, g, case)
    before = {k: v.clone() for k, v in out.items()}
    given = dict(out)
    tot, losses, met = MHEntLoss(aligned=True)(out, y)
    for k, v in given.items():
        assert torch.equal(v, before[k]), k
    assert out["xyz"] is not given["xyz"] and out["verts"] is not given["verts"] and out["uv"] is given["uv"]
    assert_close(out["xyz"].cpu(), g[f"{case}_xyz_aligned"], TOL_ALIGN, what="xyz")
    assert_close(out["verts"].cpu(), g[f"{case}_verts_aligned"], TOL_ALIGN, what="verts")
    assert len(met) == 14
    for k, v in met.items():
        assert_close(v.cpu(), g[f"{case}_metric_{k}"], TOL_METRIC, 1e-6, what=k)
    # a batch without a target mesh leaves verts as it is (criteria.py:76-78)
    out2 = {k: v for k, v in given.items()}
    MHEntLoss(aligned=True)(out2, {k: v for k, v in y.items() if k != "verts"})
    assert out2["verts"] is given["verts"]


def test_unaligned_is_bit_identical_to_ops_metrics_and_split_form(gpu_lib):
    """aligned=False is the metrics kernel as before, bit for bit; the split entry point with one array twice gives the same bits;
    two aligned evaluations give the same bits"""
    from mhentropy_amd import ops
    from mhentropy_amd.criteria import MHEntLoss, METRIC_KEYS
    rng = np.random.default_rng(5)
    N, B = 200, 64
    tgt, xyz = _hands(rng, B, 21, N)
    _, yn = synth.batch(5, B, with_image=False)
    y = {k: _dev(v) for k, v in yn.items()}
    y["pose3d"] = _dev(tgt)
    o = {"log_p": torch.zeros(B, device="cuda"), "xyz": _dev(xyz), "uv": _dev(rng.normal(128, 30, (N, B, 42)).astype(np.float32))}
    ref = ops.metrics(o["xyz"], o["uv"], y["pose3d"], y["scale"], y["crop_uv"], y["vis"])
    _, _, met = MHEntLoss()(dict(o), y)
    assert all(torch.equal(met[k], ref[i]) for i, k in enumerate(METRIC_KEYS))
    split = ops.metrics_split(o["xyz"], o["xyz"], o["uv"], y["pose3d"], y["scale"], y["crop_uv"], y["vis"])
    assert torch.equal(split, ref)
    runs = [MHEntLoss(aligned=True)(dict(o), y)[2] for _ in range(2)]
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in METRIC_KEYS)
    # the aligned joints move the error rows only
    for k in METRIC_KEYS:
        same = torch.equal(runs[0][k], met[k])
        assert same == (k.startswith("eucLoss_2d") or k.endswith("_std")), k


def test_graphed_step_with_aligned_criterion_matches_eager(gpu_lib):
    """GraphedStep(..., test_samples=n, criterion=MHEntLoss(aligned=True)) (ResNet-18, 128x128, B=8, lr 0), the batch carrying a target
    mesh: the replayed metrics equal the aligned criterion evaluated eagerly on the replay's own hypotheses, bit for bit - the aligned
    criterion captures (no host synchronisation)"""
    from mhentropy_amd.criteria import MHEntLoss
    from mhentropy_amd.train import TrainStep, GraphedStep
    from test_gpu_train import _model_and_state
    B, N, n = 8, 4, 6
    xn, yn = synth.batch(31, B, image_size=128)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    y["verts"] = _dev(np.random.default_rng(31).normal(0, 0.03, (B, 2334)).astype(np.float32) + np.float32(0.6))
    z0 = torch.as_tensor(synth.noise(31, N * B)).cuda()
    ts = TrainStep(_model_and_state("resnet18", 64, 2)[0], lr=0.0)
    crit = MHEntLoss(aligned=True)
    gs = GraphedStep(ts, x.clone(), {k: v.clone() for k, v in y.items()}, noise=z0, N=N, test_samples=n, criterion=crit)
    o = gs.replay()
    torch.cuda.synchronize()
    _, _, gm = o["criterion"]
    assert len(gm) == 14
    # the metrics pass draws fresh hypotheses every replay: evaluate the replay's own hypotheses eagerly
    _, _, em = crit({k: o[k] for k in ("log_p", "xyz", "uv", "verts")}, y)
    for k in em:
        assert torch.equal(gm[k], em[k]), k
        assert torch.isfinite(gm[k]).all(), k


def test_cpu_tensors_host_pointers_and_aliasing_are_refused(gpu_lib):
    from mhentropy_amd import _lib, ops
    L = gpu_lib
    with pytest.raises(_lib.MheError):
        ops.procrustes_align(torch.zeros(2, 3, 63), torch.zeros(3, 63))
    with pytest.raises(_lib.MheError):
        ops.procrustes_align(torch.zeros(2, 3, 63, device="cuda"), torch.zeros(3, 63))
    with pytest.raises(_lib.MheError):
        ops.procrustes_align(torch.zeros(2, 3, 63, device="cuda", dtype=torch.float64), torch.zeros(3, 63, device="cuda"))
    with pytest.raises(_lib.MheError):
        ops.procrustes_align(torch.zeros(2, 3, 63, device="cuda"), torch.zeros(3, 60, device="cuda"))
    # the C entry points themselves: host memory is an argument error, not a fault
    N, B, P = 2, 3, 21
    hp, ht, ho = (np.zeros(n, np.float32) for n in (N * B * P * 3, B * P * 3, N * B * P * 3))
    nws = L.mhe_procrustes_workspace_floats(B, P)
    ws = torch.empty(nws, device="cuda")
    hptr = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mhe_procrustes_align_f32(hptr(hp), hptr(ht), hptr(ho), None, None, C.c_void_p(ws.data_ptr()), nws, N, B, P, s0)
    assert rc != 0 and b"device memory" in L.mhe_last_error()
    dp, dt = torch.zeros(N, B, P * 3, device="cuda"), torch.zeros(B, P * 3, device="cuda")
    rc = L.mhe_procrustes_align_f32(C.c_void_p(dp.data_ptr()), C.c_void_p(dt.data_ptr()), C.c_void_p(dp.data_ptr() + 4), None, None,
                                    C.c_void_p(ws.data_ptr()), nws, N, B, P, s0)
    assert rc != 0 and b"overlap" in L.mhe_last_error()
    rc = L.mhe_procrustes_align_f32(C.c_void_p(dp.data_ptr()), C.c_void_p(dt.data_ptr()), C.c_void_p(torch.empty_like(dp).data_ptr()), None,
                                    None, C.c_void_p(ws.data_ptr()), nws - 1, N, B, P, s0)
    assert rc != 0 and b"workspace" in L.mhe_last_error()
    hx = np.zeros(N * B * 63, np.float32)
    rc = L.mhe_metrics_split_f32(hptr(hx), hptr(hx), hptr(hx), hptr(hx), hptr(hx), hptr(hx), hptr(hx), hptr(hx), N, B, s0)
    assert rc != 0 and b"device memory" in L.mhe_last_error()
    torch.cuda.synchronize()
    # the library still works afterwards (no error left behind for the next launch check)
    out = ops.procrustes_align(dp + 1.0, dt)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
