"""CPU: the hand-object Chamfer distance's host side - the golden fixture of the reference's chamfer_dist against the f64 restatement the GPU
tests compare with (tests/chamfer_ref.py), the two C entries (csrc/chamfer.hip) declared, exported and bound with matching arity and refusing bad
arguments before any launch, and the Python error paths of criteria.chamfer_dist / MHEntChamferLoss / chamfer_select, which are
all raised on CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

import chamfer_ref
from conftest import ROOT, load_golden
from mhentropy_amd import _lib, criteria, ops

NEW = ("mhe_chamfer_f32", "mhe_chamfer_bwd_f32")


def test_restatement_reproduces_the_reference_fixture():
    g = load_golden("chamfer_small")
    N, B, P, VO = (int(v) for v in g["shape"])
    assert g["points"].shape == (N, B, P, 3) and g["obj"].shape == (B, VO, 3) and g["dist"].shape == (N, B) and g["dist_3d"].shape == (B,)
    case = chamfer_ref.make_case(int(g["seed"]), N, B, P, VO)
    for k in ("points", "scale", "root", "obj"):
        assert np.array_equal(case[k], g[k]), k          # the fixture's inputs are the seeded case the GPU tests run
    mine = chamfer_ref.chamfer64(g["points"], g["scale"], g["root"], g["obj"])
    assert np.abs(mine["dist"] - g["dist"]).max() <= 1e-6 * np.abs(g["dist"]).max()
    n = int(g["hypothesis_3d"])
    one = chamfer_ref.chamfer64(g["points"][n:n + 1], g["scale"], g["root"], g["obj"])
    assert np.abs(one["dist"][0] - g["dist_3d"]).max() <= 1e-6 * np.abs(g["dist_3d"]).max()
    assert mine["gap"] > chamfer_ref.GAP


def test_symbols_declared_and_bound_with_matching_arity():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhe.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in NEW:
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/mhe.h"
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == 15, name
    assert L.mhe_abi_version() == 4
    assert "chamfer.hip" in __import__("mhentropy_amd.build", fromlist=["SOURCES"]).SOURCES
    assert callable(ops.chamfer) and callable(ops.chamfer_bwd) and callable(criteria.chamfer_dist) and callable(criteria.chamfer_select)


def test_entries_refuse_bad_arguments_before_any_launch():
    L, Z = _lib.lib(), None
    N, B, P, VO = 3, 2, 21, 37
    f = lambda *s: torch.zeros(*s)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    A = lambda t: _lib.C.c_void_p(t.data_ptr())          # host addresses: every call below must return before a kernel could read them
    pts, sc, rt, ob, dist, parts = f(N, B, P, 3), f(B), f(B, 3), f(B, VO, 3), f(N, B), f(N, B, 2)
    ip, io, gd, gp = i(N, B, P), i(N, B, VO), f(N, B), f(N, B, P, 3)

    def fwd(points=pts, scale=sc, root=rt, obj=ob, d=dist, n=N, b=B, p=P, vo=VO):
        return L.mhe_chamfer_f32(*(Z if t is None else A(t) for t in (points, scale, root, obj)), Z, Z if d is None else A(d), A(parts), A(ip), A(io),
                                 n, b, p, vo, 1000.0, Z)

    def bwd(points=pts, idx_p=ip, idx_o=io, g=gd, out=gp, n=N, b=B, p=P, vo=VO):
        return L.mhe_chamfer_bwd_f32(Z if points is None else A(points), A(sc), A(rt), A(ob), Z, *(Z if t is None else A(t) for t in (idx_p, idx_o, g, out)),
                                     n, b, p, vo, 1000.0, Z)
    bad = {"null points": dict(points=None), "null scale": dict(scale=None), "null root": dict(root=None), "null obj": dict(obj=None), "null dist": dict(d=None),
           "P = 0": dict(p=0), "P = 779": dict(p=779), "VO = 0": dict(vo=0), "N B overflow": dict(n=1 << 16, b=1 << 16), "N = 0": dict(n=0),
           "dist overlaps points": dict(d=pts), "dist overlaps obj": dict(d=ob)}
    for what, kw in bad.items():
        assert fwd(**kw) == 1 and b"mhe_chamfer_f32" in L.mhe_last_error(), what          # MHE_ERR_ARG
    assert fwd(p=779) == 1 and b"P in 1..778" in L.mhe_last_error()
    assert fwd(d=pts) == 1 and b"overlaps" in L.mhe_last_error()
    bad = {"null points": dict(points=None), "null idx_p": dict(idx_p=None), "null idx_o": dict(idx_o=None), "null g_dist": dict(g=None),
           "null g_points": dict(out=None), "P = 0": dict(p=0), "P = 779": dict(p=779), "VO = 0": dict(vo=0), "N B overflow": dict(n=1 << 16, b=1 << 16),
           "g_points overlaps points": dict(out=pts)}
    for what, kw in bad.items():
        assert bwd(**kw) == 1 and b"mhe_chamfer_bwd_f32" in L.mhe_last_error(), what


def _cpu_case():
    case = chamfer_ref.make_case(101, 3, 2, 21, 37)
    return torch.as_tensor(np.array(case["points"])), {k: torch.as_tensor(np.array(v)) for k, v in chamfer_ref.target_of(case).items()}


def test_chamfer_dist_error_paths_on_cpu_tensors():
    pts, tgt = _cpu_case()
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        criteria.chamfer_dist(pts, tgt)
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        criteria.chamfer_dist(pts[0], tgt)
    with pytest.raises(ValueError, match="object_verts"):
        criteria.chamfer_dist(pts, {k: v for k, v in tgt.items() if k != "object_verts"})
    for wrong in (pts[0, 0], pts[None], pts[..., :2], pts.reshape(3, 2, 63)):
        with pytest.raises(ValueError, match="norm_rel_xyz"):
            criteria.chamfer_dist(wrong, tgt)
    with pytest.raises(ValueError, match="K=779"):
        criteria.chamfer_dist(torch.zeros(1, 2, 779, 3), tgt)
    with pytest.raises(ValueError, match="images"):
        criteria.chamfer_dist(pts[:, :1], tgt)
    with pytest.raises(ValueError, match="object_verts"):
        criteria.chamfer_dist(pts, dict(tgt, object_verts=tgt["object_verts"][:, :-1]))
    for count in ([0, 5], [37, 38], [-1, 1]):
        with pytest.raises(ValueError, match="outside 1..VO=37"):
            criteria.chamfer_dist(pts, dict(tgt, object_count=torch.tensor(count, dtype=torch.int32)))
    with pytest.raises(ValueError, match="int32"):
        criteria.chamfer_dist(pts, dict(tgt, object_count=torch.tensor([5, 5])))
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):          # a valid count passes the checks and reaches the device check
        criteria.chamfer_dist(pts, dict(tgt, object_count=torch.tensor([1, 37], dtype=torch.int32)))


def test_criterion_and_selection_error_paths_on_cpu_tensors():
    pts, tgt = _cpu_case()
    N, B = pts.shape[:2]
    out = {"log_p": torch.zeros(B), "xyz": pts.reshape(N, B, 63), "uv": torch.zeros(N, B, 42)}
    with pytest.raises(ValueError, match="object_verts"):
        criteria.MHEntChamferLoss()(dict(out), {k: v for k, v in tgt.items() if k != "object_verts"})
    assert criteria.MHEntLoss().chamfer_select is False and criteria.MHEntLoss(None, True).chamfer_select is False
    on = criteria.MHEntChamferLoss(None, True)
    assert isinstance(on, criteria.MHEntLoss) and on.chamfer_select is True and on.aligned is True and not criteria.MHEntChamferLoss().aligned
    for q in (0, N + 1, 1.0):
        with pytest.raises(ValueError, match="Q="):
            criteria.chamfer_select(out, tgt, Q=q)
    with pytest.raises(ValueError, match="points="):
        criteria.chamfer_select(out, tgt, points="uv")
    with pytest.raises(ValueError, match="verts"):
        criteria.chamfer_select(out, tgt, points="verts")
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        criteria.chamfer_select(out, tgt, Q=1)
