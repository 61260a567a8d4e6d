"""CPU: the silhouette distance's host side - the f64 restatement the GPU tests compare with (tests/silhouette_ref.py) against a brute-force
loop form and against central finite differences, the choice of seeds (the restatement evaluated in f32 already stays within the index cap and
within the bounds the kernel is held to), the three C entries (csrc/silhouette.hip) declared, exported and bound with matching arity and refusing
bad arguments before any launch, and the Python error paths of criteria.silhouette_dist / silhouette_select, raised on CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

import silhouette_ref as sr
from conftest import ROOT
from mhentropy_amd import _lib, criteria, ops

NEW = {"mhe_silhouette_pixels": 8, "mhe_silhouette_dist_f32": 13, "mhe_silhouette_dist_bwd_f32": 14}


def _tiny(seed, N=2, B=2, V=3, S=4, k=2):
    rng = np.random.default_rng(seed)
    mask = rng.uniform(0, 1, (B, S * k, S * k)) < 0.45
    mask[1, :k, :k] = True
    verts = rng.normal(0, 0.5, (N, B, V, 3)).astype(np.float32)
    logs_t = np.concatenate([rng.normal(0.2, 0.2, (N, B, 1)), rng.normal(0, 0.1, (N, B, 2))], -1).astype(np.float32)
    return verts, logs_t, mask


def test_restatement_agrees_with_the_brute_force_loops():
    for seed in (1, 2, 3):
        verts, logs_t, mask = _tiny(seed)
        if seed == 2:
            mask[0] = False                                   # an empty mask: 0
        if seed == 3:
            verts[1, 1, 2, 1] = np.inf                        # a non-finite vertex: NaN for that row only
        ref = sr.silhouette(verts, logs_t, mask, 4)
        dist, inside, cover, idx_v, idx_m = sr.brute(verts, logs_t, mask, 4)
        for a, b in ((ref["dist"], dist), (ref["inside"], inside), (ref["cover"], cover)):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b)) <= 1e-14
        ok = ~np.isnan(dist)
        assert np.array_equal(ref["idx_v"][ok], idx_v[ok]) and np.array_equal(ref["idx_m"][ok], idx_m[ok])
        assert np.isnan(dist).sum() == (1 if seed == 3 else 0)
        if seed == 2:
            assert (ref["dist"][:, 0] == 0).all() and (ref["idx_v"][:, 0] == -1).all() and ref["count"][0] == 0
    # a float mask: the threshold is on the box mean, >= 0.5
    m = np.zeros((1, 4, 4), np.float32)
    m[0, :2, :2] = [[1, 1], [0, 0]]          # mean 0.5: kept
    m[0, 2:, 2:] = [[1, 0.75], [0, 0]]       # mean 0.4375: dropped
    pixels, count = sr.pixel_list(m, 2)
    assert count[0] == 1 and pixels[0].tolist() == [0, -1, -1, -1]
    pixels, count = sr.pixel_list(np.ones((1, 4, 4), bool), 4)
    assert count[0] == 16 and pixels[0, 5] == (1 << 16) | 1 and pixels[0, 3] == 3


def test_autograd_gradient_agrees_with_central_differences():
    verts, logs_t, mask = _tiny(5, N=2, B=2, V=3)
    S, eps = 4, 1e-6
    g = np.array([[1.0, -0.7], [0.4, 1.3]])
    ref = sr.silhouette(verts, logs_t, mask, S)
    gv, gl = sr.grad(verts, logs_t, mask, S, g)
    at = sr.grad(verts, logs_t, mask, S, g, (ref["idx_v"], ref["idx_m"]))
    assert np.abs(at[0] - gv).max() <= 1e-14 and np.abs(at[1] - gl).max() <= 1e-14          # at its own indices: the same gradient
    assert (gv[..., 2] == 0).all() and np.abs(gv).max() > 0.05 and np.abs(gl).max() > 0.05

    def total(v, lt):
        return float((g * sr.silhouette(v, lt, mask, S)["dist"]).sum())
    v64, l64 = verts.astype(np.float64), logs_t.astype(np.float64)
    for arr, grad, other in ((v64, gv, l64), (l64, gl, v64)):
        for i in np.ndindex(arr.shape):
            hi, lo = arr.copy(), arr.copy()
            hi[i] += eps
            lo[i] -= eps
            fd = (total(hi, other) - total(lo, other)) / (2 * eps) if arr is v64 else (total(other, hi) - total(other, lo)) / (2 * eps)
            assert abs(fd - grad[i]) <= 1e-7, (i, fd, grad[i])          # away from ties: the argmins do not move within eps


@pytest.mark.parametrize("name", list(sr.CASES))
def test_seeds_keep_the_f32_restatement_within_the_caps(name):
    """the inputs of the GPU tests: evaluated in f32 on the CPU the restatement itself stays within the index cap, its stray indices are
    near-ties, and it meets the bounds the kernel is held to (they are four times what was measured of it)"""
    fwd, rev, share, excess = sr.f32_deviation(name)
    print(f"{name}: f32 restatement vs f64: forward {fwd:.3e} (bound {sr.FWD_RTOL:.3e}), reverse {rev:.3e} (bound {sr.REV_RTOL[name]:.3e}), "
          f"index mismatch share {share:.5f}, excess {excess:.3e}")
    assert share <= sr.MISMATCH_CAP and excess <= sr.FWD_RTOL
    assert fwd <= sr.FWD_RTOL and rev <= sr.REV_RTOL[name]
    case, ref = sr.reference(name)
    kw = sr.CASES[name]
    if kw.get("inside_only"):
        assert (ref["d_v"] == 0).all() and (ref["inside"] == 0).all()
    elif kw["V"] >= 64:
        p = sr.project(torch.as_tensor(np.nan_to_num(case["verts"])).double(), torch.as_tensor(np.array(case["logs_t"])).double(), torch.float64)
        assert (p.abs() > 1).any() and (ref["d_v"] == 0).any() and (ref["d_v"] > 0).any()          # partly outside the image, partly inside the mask


def test_symbols_declared_and_bound_with_matching_arity():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhe.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, arity in NEW.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/mhe.h"
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == arity, name
    assert L.mhe_abi_version() == 4
    assert "silhouette.hip" in __import__("mhentropy_amd.build", fromlist=["SOURCES"]).SOURCES
    assert all(callable(f) for f in (ops.silhouette_pixels, ops.silhouette_dist, ops.silhouette_dist_bwd, criteria.silhouette_dist, criteria.silhouette_select))


def test_entries_refuse_bad_arguments_before_any_launch():
    L, Z = _lib.lib(), None
    N, B, V, S, H = 3, 2, 21, 8, 16
    f = lambda *s: torch.zeros(*s)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    A = lambda t: Z if t is None else _lib.C.c_void_p(t.data_ptr())          # host addresses: every call below must return before a kernel could read them
    mask, pix, cnt = torch.zeros(B, H, H, dtype=torch.uint8), i(B, S * S), i(B)
    vt, lt, dist, parts, iv, im = f(N, B, V, 3), f(N, B, 3), f(N, B), f(N, B, 2), i(N, B, V), i(N, B, S * S)
    gd, gv, gl = f(N, B), f(N, B, V, 3), f(N, B, 3)

    def pixels(m=mask, fl=0, p=pix, c=cnt, b=B, h=H, s=S):
        return L.mhe_silhouette_pixels(A(m), fl, A(p), A(c), b, h, s, Z)

    def fwd(verts=vt, logs=lt, p=pix, c=cnt, d=dist, n=N, b=B, v=V, s=S):
        return L.mhe_silhouette_dist_f32(A(verts), A(logs), A(p), A(c), A(d), A(parts), A(iv), A(im), n, b, v, s, Z)

    def bwd(verts=vt, p=pix, idx_v=iv, idx_m=im, g=gd, out=gv, out_l=gl, n=N, b=B, v=V, s=S):
        return L.mhe_silhouette_dist_bwd_f32(A(verts), A(lt), A(p), A(cnt), A(idx_v), A(idx_m), A(g), A(out), A(out_l), n, b, v, s, Z)
    bad = {"null mask": dict(m=None), "null pixels": dict(p=None), "null count": dict(c=None), "flag": dict(fl=2), "B = 0": dict(b=0), "S = 0": dict(s=0),
           "S = 65": dict(s=65, h=130), "H not a multiple": dict(h=20), "H < S": dict(h=4), "H too large": dict(h=8192), "overlap": dict(p=cnt)}
    for what, kw in bad.items():
        assert pixels(**kw) == 1 and b"mhe_silhouette_pixels" in L.mhe_last_error(), what          # MHE_ERR_ARG
    bad = {"null verts": dict(verts=None), "null logs_t": dict(logs=None), "null pixels": dict(p=None), "null count": dict(c=None), "null dist": dict(d=None),
           "V = 0": dict(v=0), "V = 779": dict(v=779), "S = 0": dict(s=0), "S = 65": dict(s=65), "N = 0": dict(n=0), "N B overflow": dict(n=1 << 16, b=1 << 16),
           "dist overlaps verts": dict(d=vt), "dist overlaps pixels": dict(d=pix)}
    for what, kw in bad.items():
        assert fwd(**kw) == 1 and b"mhe_silhouette_dist_f32" in L.mhe_last_error(), what
    assert fwd(v=779) == 1 and b"V in 1..778" in L.mhe_last_error()
    assert fwd(d=vt) == 1 and b"overlaps" in L.mhe_last_error()
    bad = {"null verts": dict(verts=None), "null pixels": dict(p=None), "null idx_v": dict(idx_v=None), "null idx_m": dict(idx_m=None), "null g_dist": dict(g=None),
           "null g_verts": dict(out=None), "null g_logs_t": dict(out_l=None), "V = 779": dict(v=779), "S = 65": dict(s=65), "B = 0": dict(b=0),
           "g_verts overlaps verts": dict(out=vt), "g_logs_t overlaps g_dist": dict(out_l=gd)}
    for what, kw in bad.items():
        assert bwd(**kw) == 1 and b"mhe_silhouette_dist_bwd_f32" in L.mhe_last_error(), what


def _cpu_case():
    case = sr.make_case(**sr.CASES["v65_s8_35_rows"])
    return torch.as_tensor(np.nan_to_num(case["verts"])), torch.as_tensor(np.array(case["logs_t"])), torch.as_tensor(np.array(case["mask"]))


def test_silhouette_dist_error_paths_on_cpu_tensors():
    v, lt, mask = _cpu_case()          # (7, 5, 65, 3), (7, 5, 3), (5, 8, 8)
    for form in (v, v.reshape(7, 5, -1)):
        with pytest.raises(_lib.MheError, match="CUDA/HIP"):          # valid shapes pass the checks and reach the device check
            criteria.silhouette_dist(form, lt, mask, size=8)
    for wrong in (v[None], v[0, 0], v[..., :2], v.reshape(7, 5, 65 * 3)[..., :-1], "verts"):
        with pytest.raises(ValueError, match="verts must be"):
            criteria.silhouette_dist(wrong, lt, mask, size=8)
    for wrong in (torch.zeros(7, 5, 779, 3), torch.zeros(7, 5, 0, 3)):
        with pytest.raises(ValueError, match="V=(779|0) vertices"):
            criteria.silhouette_dist(wrong, lt, mask, size=8)
    for wrong in (lt[:, :4], lt[..., :2], lt[0]):
        with pytest.raises(ValueError, match="logs_t must be"):
            criteria.silhouette_dist(v, wrong, mask, size=8)
    for wrong in (mask[:4], mask[:, :4], mask[0]):
        with pytest.raises(ValueError, match="hand_mask must be"):
            criteria.silhouette_dist(v, lt, wrong, size=8)
    for size in (3, 16, 64):
        with pytest.raises(ValueError, match="not a multiple of size"):
            criteria.silhouette_dist(v, lt, mask, size=size)
    for size in (0, 65, 8.0):
        with pytest.raises(ValueError, match="size="):
            criteria.silhouette_dist(v, lt, mask, size=size)


def test_silhouette_select_error_paths_on_cpu_tensors():
    v, lt, mask = _cpu_case()
    out, tgt = {"verts": v.reshape(7, 5, -1), "logs_t": lt, "faces": torch.zeros(4, 3)}, {"hand_mask": mask}
    for q in (0, 8, 1.0):
        with pytest.raises(ValueError, match="Q="):
            criteria.silhouette_select(out, tgt, Q=q, size=8)
    for k in ("verts", "logs_t"):
        with pytest.raises(ValueError, match=k):
            criteria.silhouette_select({a: b for a, b in out.items() if a != k}, tgt, size=8)
    with pytest.raises(ValueError, match="hand_mask"):
        criteria.silhouette_select(out, {}, size=8)
    with pytest.raises(ValueError, match="not a multiple of size"):
        criteria.silhouette_select(out, tgt, Q=1)
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        criteria.silhouette_select(out, tgt, Q=1, size=8)
