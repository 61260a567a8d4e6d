"""GPU tests of the body head's evaluation path: the mesh error accumulated inside the skinning kernels (BodyLayer.vertex_error: csrc/lbs_skin.hip
mhe_lbs_skin_err_mfma_f32, csrc/body.hip mhe_lbs_skin_err_f32), body.point_errors / body.min_of_n (csrc/body_eval.hip) and BodyFlowHead.evaluate.
Everything against float64 on the CPU over the oracle chain (oracle/rot6d_ref.py -> oracle/body_ref.py -> the error's definition), computed once
per case and shared.  The scalar-operand kernel (MHE_LBS_MFMA=0) runs in ONE fresh child process for all cases, under a timeout.

Bounds: RTOL = 1e-4 of the reference's largest value, the project's bound for f32 kernels against f64 (tests/test_gpu_body_keypoints.py).  For
pa_mpjpe the reference itself is close to zero against the data (predictions are similarity transforms of the targets plus 1 % noise), so the
f32 rounding of coordinates of the targets' size enters absolutely: + 1e-5 of the target's extent, the bound set for an exact similarity."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import assert_close
from mhentropy_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-4
CASES = {"mano_13x5": ("mano", 13, 5), "body_13x5": ("body203", 13, 5), "body_2x32": ("body203", 2, 32)}
VARIANTS = ((False, 1.0), (True, 1.0), (True, 0.7))          # (center given, scale)


def _cu(a):
    return torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared case arrays are read-only)


@functools.lru_cache(None)
def _tables(name):
    """'mano': MANO-sized (J = 16, NV = 778: one k-step of joints) with the 21-row keypoint regressor of the reference wrapper's layout;
    'body203': synthetic_body_tables(NV=203, J=24): two joint k-steps, NV no multiple of 32, VP = 256 > NV"""
    from mhentropy_amd import body
    from oracle import mano_ref
    if name == "body203":
        return body.synthetic_body_tables(5, NV=203, J=24, keypoints=17)
    t = synth.mano_tables(0)
    reg = np.zeros((21, 778), np.float32)
    for src, dst in mano_ref.WRAPPER_JOINT_MAP.items():
        reg[dst] = t["J_regressor"][src]
    for dst, vid in mano_ref.WRAPPER_TIP_VERTS.items():
        reg[dst, vid] = 1.0
    return {"v_template": t["v_template"], "shapedirs": t["shapedirs"], "posedirs": t["posedirs"], "J_regressor": t["J_regressor"],
            "weights": t["weights"], "parents": np.asarray(mano_ref.PARENTS), "keypoint_regressor": reg}


def _tb64(tables):
    return {k: (torch.as_tensor(np.asarray(v, np.float64)) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v)) for k, v in tables.items()}


def _err64(verts, target, center, scale, K):
    """the definition in f64: verts (R,NV,3), target (B,NV,3), center (R,3) or None -> (R,)"""
    verts, target = np.asarray(verts, np.float64), np.asarray(target, np.float64)
    d = scale * verts - np.repeat(target, K, 0)
    if center is not None:
        d = d - np.asarray(center, np.float64)[:, None, :]
    return np.sqrt((d * d).sum(-1)).mean(-1)


@functools.lru_cache(None)
def _case(name):
    """inputs and the f64 oracle vertices of one case (computed once, never modified)"""
    from oracle import body_ref, rot6d_ref
    tname, B, K = CASES[name]
    t = _tables(tname)
    J, NV, R = t["weights"].shape[1], t["v_template"].shape[0], B * K
    rng = np.random.default_rng(sorted(CASES).index(name) + 70)
    p6 = rng.normal(0, 1, (R, 6 * J)).astype(np.float32)
    betas = rng.normal(0, 1, (R, 10)).astype(np.float32)
    rm = rot6d_ref.rotation_from_ortho6d(torch.as_tensor(p6).view(R, J, 6))
    v64 = body_ref.lbs(_tb64(t), rm.double(), torch.as_tensor(betas).double())[0].numpy()
    target = (v64[::K] + rng.normal(0, 0.02, (B, NV, 3))).astype(np.float32)          # the image's first hypothesis, perturbed
    center = rng.normal(0, 0.05, (R, 3)).astype(np.float32)
    for a in (p6, betas, v64, target, center):
        a.setflags(write=False)
    return {"tables": tname, "B": B, "K": K, "R": R, "NV": NV, "p6": p6, "betas": betas, "v64": v64, "target": target, "center": center}


@functools.lru_cache(None)
def _layer(tname):
    from mhentropy_amd import body
    return body.BodyLayer(_tables(tname)).cuda()


def _run_case(name, vi):
    c = _case(name)
    with_center, scale = VARIANTS[vi]
    return _layer(c["tables"]).vertex_error(_cu(c["betas"]), pose6d=_cu(c["p6"]), target_verts=_cu(c["target"]),
                                            center=_cu(c["center"]) if with_center else None, scale=scale)


def _ref_case(name, vi):
    c = _case(name)
    with_center, scale = VARIANTS[vi]
    return _err64(c["v64"], c["target"], c["center"] if with_center else None, scale, c["K"])


def _scalar_child(out_path):
    """runs in the child process (MHE_LBS_MFMA=0): every case and variant through the scalar-operand kernel"""
    assert os.environ.get("MHE_LBS_MFMA") == "0"
    res = {}
    for name in CASES:
        for vi in range(len(VARIANTS)):
            res[f"{name}|{vi}"] = _run_case(name, vi).cpu().numpy()
    np.savez(out_path, **res)


@functools.lru_cache(None)
def _scalar_results():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "scalar.npz")
        here = os.path.dirname(os.path.abspath(__file__))
        code = f"import sys; sys.path.insert(0, {here!r}); import test_gpu_body_eval as T; T._scalar_child(sys.argv[1])"
        p = subprocess.run([sys.executable, "-c", code, out], env={**os.environ, "MHE_LBS_MFMA": "0"}, timeout=300, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        return dict(np.load(out))


# ---- 1. vertex error against f64, both kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vi", range(len(VARIANTS)))
@pytest.mark.parametrize("name", sorted(CASES))
def test_vertex_error_matches_f64_oracle(gpu_lib, monkeypatch, name, vi):
    """worst measured |err - f64| / max f64 over all cases and variants: matrix-core kernel 2.0e-7, scalar-operand kernel 1.8e-7 (bound 1e-4)"""
    monkeypatch.delenv("MHE_LBS_MFMA", raising=False)
    c = _case(name)
    assert gpu_lib.mhe_lbs_skin_err_supported(c["R"], _layer(c["tables"]).J, 10, c["NV"], _layer(c["tables"]).VP, c["B"]) == 1
    got, ref = _run_case(name, vi).cpu().numpy(), _ref_case(name, vi)
    assert got.shape == (c["R"],)
    print(f"vertex_error {name} center={VARIANTS[vi][0]} scale={VARIANTS[vi][1]}: matrix-core max|diff|/max {np.abs(got - ref).max() / ref.max():.2e}")
    assert_close(got, ref, RTOL, what=f"vertex_error (matrix-core) {name} {VARIANTS[vi]}")


@pytest.mark.parametrize("vi", range(len(VARIANTS)))
@pytest.mark.parametrize("name", sorted(CASES))
def test_vertex_error_scalar_kernel_matches_f64_oracle(gpu_lib, name, vi):
    got, ref = _scalar_results()[f"{name}|{vi}"], _ref_case(name, vi)
    print(f"vertex_error {name} center={VARIANTS[vi][0]} scale={VARIANTS[vi][1]}: scalar-operand max|diff|/max {np.abs(got - ref).max() / ref.max():.2e}")
    assert_close(got, ref, RTOL, what=f"vertex_error (MHE_LBS_MFMA=0) {name} {VARIANTS[vi]}")


# ---- 2. against the GPU's own vertices -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_vertex_error_matches_own_vertices(gpu_lib, monkeypatch, name):
    """the f64 error of the GPU's own 'vertices' differs from vertex_error by the rounding of the norm and of the sum only; worst measured
    |diff| / max 1.8e-7 (bound 1e-4)"""
    monkeypatch.delenv("MHE_LBS_MFMA", raising=False)
    c = _case(name)
    layer = _layer(c["tables"])
    for vi, (with_center, scale) in enumerate(VARIANTS):
        verts = layer(_cu(c["betas"]), pose6d=_cu(c["p6"]), scale=scale)["vertices"].cpu().numpy()
        ref = _err64(verts, c["target"], c["center"] if with_center else None, 1.0, c["K"])          # (the vertices are scaled already)
        got = _run_case(name, vi).cpu().numpy()
        print(f"vertex_error {name} {VARIANTS[vi]}: against own vertices max|diff|/max {np.abs(got - ref).max() / ref.max():.2e}")
        assert_close(got, ref, RTOL, what=f"vertex_error vs own vertices {name} {VARIANTS[vi]}")


# ---- 3. determinism, 4. padded lanes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_vertex_error_is_deterministic_and_padding_is_isolated(gpu_lib, monkeypatch, name):
    monkeypatch.delenv("MHE_LBS_MFMA", raising=False)
    c = _case(name)
    layer, B, NV = _layer(c["tables"]), c["B"], c["NV"]
    a, b = _run_case(name, 1), _run_case(name, 1)
    assert torch.equal(a, b), "two calls differ"
    assert torch.isfinite(a).all()
    # the targets as a slice of a larger buffer that is NaN everywhere else: what a lane without a vertex (v >= NV, up to VP and beyond the last
    # image's end) could read if it read past its mesh
    n, pad = B * NV * 3, 3 * 64 * 4
    big = torch.full((pad + n + pad,), float("nan"), device="cuda")
    big[pad:pad + n] = _cu(c["target"]).reshape(-1)
    view = big[pad:pad + n].view(B, NV, 3)
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + 4 * pad
    got = layer.vertex_error(_cu(c["betas"]), pose6d=_cu(c["p6"]), target_verts=view, center=_cu(c["center"]))
    assert torch.equal(got, a), "a lane without a vertex contributed"
    # a NaN at a REAL vertex does reach its image's rows, and only those (the check above is not vacuous)
    t2 = _cu(c["target"]).clone()
    t2[1, NV - 1, 2] = float("nan")
    e2 = layer.vertex_error(_cu(c["betas"]), pose6d=_cu(c["p6"]), target_verts=t2, center=_cu(c["center"])).view(B, c["K"])
    assert torch.isnan(e2[1]).all() and torch.equal(e2[0], a.view(B, -1)[0]) and (B < 3 or torch.equal(e2[2:], a.view(B, -1)[2:]))


# ---- 5. point errors --------------------------------------------------------------------------------------------------------------------------
def _procrustes64(pred, tgt):
    """the documented convention in f64 numpy: both centred and normalised (+ 1e-8), M = tgt0^T pred0 = U S V^T, R = U V^T (no determinant
    correction), s = tr S; the prediction mapped into the target's frame"""
    t1, t2 = tgt.mean(0), pred.mean(0)
    a, b = tgt - t1, pred - t2
    s1, s2 = np.linalg.norm(a) + 1e-8, np.linalg.norm(b) + 1e-8
    a, b = a / s1, b / s2
    u, w, vt = np.linalg.svd(a.T @ b)
    return (b @ (u @ vt).T) * w.sum() * s1 + t1


def _similar(rng, tgt, K, noise):
    """K proper similarity transforms (rotation, scale, shift) of every target, plus noise"""
    B, P = tgt.shape[:2]
    out = np.empty((B, K, P, 3))
    for b in range(B):
        for k in range(K):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            q = q * np.sign(np.linalg.det(q))
            out[b, k] = rng.uniform(0.5, 2.0) * tgt[b] @ q.T + rng.normal(0, 0.5, 3) + rng.normal(0, noise, (P, 3))
    return out


@pytest.mark.parametrize("P", [1, 17, 64])
def test_point_errors_match_f64(gpu_lib, P):
    """worst measured: mpjpe |diff| / max 1.2e-7; pa_mpjpe |diff| 2.1e-8 of the target's extent; exact similarity pa_mpjpe 2.6e-7 of the extent
    (bound 1e-5)"""
    from mhentropy_amd import body
    B, K = 3, 7
    rng = np.random.default_rng(P)
    tgt = rng.normal(0, 0.3, (B, P, 3)).astype(np.float32)
    ext = float(np.abs(tgt).max())
    pts = _similar(rng, tgt.astype(np.float64), K, 0.01 * ext).astype(np.float32)
    t64, p64 = tgt.astype(np.float64), pts.astype(np.float64)
    pa_ref = np.array([[np.linalg.norm(_procrustes64(p64[b, k], t64[b]) - t64[b], axis=-1).mean() for k in range(K)] for b in range(B)])
    for root in (None, 0, (0, P - 1) if P > 1 else (0,)):
        got = body.point_errors(_cu(pts), _cu(tgt), root=root)
        assert got["mpjpe"].shape == (B, K) and got["pa_mpjpe"].shape == (B, K)
        idx = [] if root is None else [root] if isinstance(root, int) else list(root)
        pc = p64 - (p64[:, :, idx].mean(2, keepdims=True) if idx else 0.0)
        tc = t64 - (t64[:, idx].mean(1, keepdims=True) if idx else 0.0)
        ref = np.linalg.norm(pc - tc[:, None], axis=-1).mean(-1)
        m, pa = got["mpjpe"].cpu().numpy(), got["pa_mpjpe"].cpu().numpy()
        print(f"point_errors P={P} root={root}: mpjpe max|diff|/max {np.abs(m - ref).max() / max(ref.max(), 1e-30):.2e}   "
              f"pa_mpjpe max|diff|/extent {np.abs(pa - pa_ref).max() / ext:.2e}")
        assert_close(m, ref, RTOL, what=f"mpjpe P={P} root={root}")
        assert_close(pa, pa_ref, RTOL, 1e-5 * ext, what=f"pa_mpjpe P={P} root={root}")
        assert torch.equal(got["mpjpe"], body.point_errors(_cu(pts), _cu(tgt), root=root)["mpjpe"])
    exact = _similar(rng, t64, K, 0.0).astype(np.float32)
    pa = body.point_errors(_cu(exact), _cu(tgt))["pa_mpjpe"].cpu().numpy()
    print(f"point_errors P={P}: exact similarity pa_mpjpe max / extent {pa.max() / ext:.2e}")
    assert np.isfinite(pa).all() and pa.max() <= 1e-5 * ext


# ---- 6. min of n ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,ns", [(37, (1,)), (37, (37,)), (37, (1, 2, 5, 10, 25, 30, 36, 37)), (150, (1, 64, 65, 129, 150)), (1, (1,))])
def test_min_of_n_matches_cummin(gpu_lib, K, ns):
    from mhentropy_amd import body
    B = 5
    gen = torch.Generator().manual_seed(K + len(ns))
    err = torch.rand(B, K, generator=gen)
    err[1] = torch.linspace(1, 0, K) if K > 1 else err[1]          # the minimum keeps moving to the last entry
    err[2] = torch.linspace(0, 1, K) if K > 1 else err[2]          # ... stays at the first
    if K >= 37:                                                    # exact duplicates: the lowest index wins
        err[3] = 0.75
        err[3, [4, 9, 30]] = 0.25
        err[3, [20, 33]] = 0.125
    val, idx = body.min_of_n(err.cuda(), ns)
    assert val.shape == (B, len(ns)) and idx.shape == (B, len(ns)) and val.dtype == torch.float32 and idx.dtype == torch.int32
    cm = torch.cummin(err, 1).values[:, [n - 1 for n in ns]]
    assert torch.equal(val.cpu(), cm)
    idx = idx.cpu().long()
    assert bool((idx >= 0).all()) and bool((idx < torch.tensor(ns)[None]).all())
    assert torch.equal(err.gather(1, idx), val.cpu())
    if K >= 37:
        want = [4 if n <= 20 else 20 for n in ns if n > 4]
        assert idx[3, [i for i, n in enumerate(ns) if n > 4]].tolist() == want
        assert all(idx[3, i] == 0 for i, n in enumerate(ns) if n <= 4)
    assert idx[2].tolist() == [0] * len(ns) and idx[1].tolist() == [n - 1 for n in ns]


# ---- 7. the public call ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_equals_the_composition_of_public_pieces(gpu_lib, monkeypatch):
    """peak allocation growth measured: 0.122 MB with target_verts, 0.094 MB without; one (R, NV, 3) tensor is 0.224 MB (R = 24, NV = 778)"""
    from mhentropy_amd import body
    monkeypatch.delenv("MHE_LBS_MFMA", raising=False)
    torch.manual_seed(11)
    t = _tables("mano")
    head = body.BodyFlowHead(t, context_features=64, hidden=64, num_layers=2, num_blocks=1).cuda().eval()
    B, K, NK, NV, D, ns, root = 4, 6, 21, 778, 96, (1, 3, 6), (1, 5)
    rng = np.random.default_rng(7)
    feats, betas = _cu(rng.normal(0, 0.5, (B, 64)).astype(np.float32)), _cu(rng.normal(0, 1, (B, 10)).astype(np.float32))
    noise = _cu(rng.normal(0, 1, (B, K, D)).astype(np.float32))
    tk, tv = _cu(rng.normal(0, 0.1, (B, NK, 3)).astype(np.float32)), _cu(rng.normal(0, 0.1, (B, NV, 3)).astype(np.float32))
    keep = noise.clone()
    res = head.evaluate(feats, K, tk, target_verts=tv, betas=betas, noise=noise, ns=ns, root=root)
    assert torch.equal(noise, keep), "the caller's noise was written"
    assert set(res) == {"pose6d", "log_prob", "mpjpe", "pa_mpjpe", "pve", "min_mpjpe", "min_pa_mpjpe", "min_pve", "argmin_mpjpe", "argmin_pa_mpjpe",
                        "argmin_pve"}
    assert not any(v.requires_grad for v in res.values())
    # the same thing from the public pieces, on the same noise with row 0 at the mode
    z = noise.clone()
    z[:, 0] = 0.0
    with torch.no_grad():
        out = head(feats, K, betas=betas, noise=z, want_verts=True, want_keypoints=True)
    assert torch.equal(res["pose6d"], out["pose6d"]) and torch.equal(res["log_prob"], out["log_prob"])
    pe = body.point_errors(out["keypoints"], tk, root=root)
    assert torch.equal(res["mpjpe"], pe["mpjpe"]) and torch.equal(res["pa_mpjpe"], pe["pa_mpjpe"])
    kp64, v64, tk64, tv64 = (a.cpu().double().numpy() for a in (out["keypoints"], out["vertices"], tk, tv))
    cen, tcen = kp64[:, :, list(root)].mean(2), tk64[:, list(root)].mean(1)
    m_ref = np.linalg.norm((kp64 - cen[:, :, None]) - (tk64 - tcen[:, None])[:, None], axis=-1).mean(-1)
    assert_close(res["mpjpe"].cpu().numpy(), m_ref, RTOL, what="evaluate: mpjpe")
    pve_ref = _err64(v64.reshape(B * K, NV, 3), tv64 - tcen[:, None], cen.reshape(B * K, 3), 1.0, K).reshape(B, K)
    assert_close(res["pve"].cpu().numpy(), pve_ref, RTOL, what="evaluate: pve")
    for k in ("mpjpe", "pa_mpjpe", "pve"):
        val, idx = body.min_of_n(res[k], ns)
        assert torch.equal(res["min_" + k], val) and torch.equal(res["argmin_" + k], idx)
        assert torch.equal(val.cpu(), torch.cummin(res[k].cpu(), 1).values[:, [n - 1 for n in ns]])
    # mode_first: hypothesis 0 is the explicit zero-noise row; mode_first=False leaves the noise as given
    r0 = head.evaluate(feats, K, tk, target_verts=tv, betas=betas, noise=z, ns=ns, root=root, mode_first=False)
    for k in res:
        assert torch.equal(res[k], r0[k]), k
    raw = head.evaluate(feats, K, tk, betas=betas, noise=noise, ns=ns, root=root, mode_first=False)
    assert "pve" not in raw and not torch.equal(raw["pose6d"][:, 0], res["pose6d"][:, 0]) and torch.equal(raw["pose6d"][:, 1:], res["pose6d"][:, 1:])
    drawn = head.evaluate(feats, K, tk, ns=ns)
    assert torch.equal(drawn["pose6d"][:, 0], head.evaluate(feats, K, tk, ns=ns)["pose6d"][:, 0]), "hypothesis 0 does not depend on the draw"
    # no (R, NV, 3) tensor: the peak with target_verts stays below the peak without + one vertex tensor
    def growth(**kw):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        r = head.evaluate(feats, K, tk, betas=betas, noise=noise, ns=ns, root=root, **kw)
        torch.cuda.synchronize()
        del r
        return torch.cuda.max_memory_allocated() - before
    g0, g1 = growth(), growth(target_verts=tv)
    print(f"evaluate: peak allocation growth {g1 / 1e6:.3f} MB with target_verts, {g0 / 1e6:.3f} MB without; one (R, NV, 3) tensor {B * K * NV * 12 / 1e6:.3f} MB")
    assert g1 < g0 + B * K * NV * 12
