"""CPU: the hand mesh evaluation's host side - the f64 restatement the GPU tests compare with (tests/mesh_eval_ref.py) against a plain torch.cdist
composition, the C entry (csrc/mesh_eval.hip) declared, exported, bound and refusing bad arguments before any launch, and the Python error paths of
criteria.mesh_eval / criteria.mesh_select, which are all raised on CPU tensors before the device is needed."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_eval_ref
from conftest import ROOT
from mhentropy_amd import _lib, criteria, ops


@pytest.mark.parametrize("seed,N,B,V,T", [(1, 3, 2, 65, 2), (2, 1, 1, 1, 1), (3, 2, 3, 257, 4), (4, 2, 1, 778, 3)])
def test_restatement_matches_a_cdist_composition(seed, N, B, V, T):
    case = mesh_eval_ref.make_case(seed, N, B, V, T)
    ref = mesh_eval_ref.mesh_eval64(case["pred"], case["target"], case["scale"], case["thr"], case["unit"])
    assert ref["gap"] >= mesh_eval_ref.GAP
    t64 = lambda a: torch.as_tensor(np.array(a, np.float64))          # (a copy: the case arrays are read-only)
    su = t64(case["scale"]) * case["unit"]
    P = t64(case["pred"]) * su[None, :, None, None]
    G = (t64(case["target"]) * su[:, None, None])[None].expand(N, B, V, 3)
    D = torch.cdist(P.reshape(N * B, V, 3), G.reshape(N * B, V, 3), compute_mode="donot_use_mm_for_euclid_dist")
    d1, d2 = D.min(2).values.view(N, B, V), D.min(1).values.view(N, B, V)
    assert np.abs(d1.numpy() - ref["d1"]).max() <= 1e-12 * ref["d1"].max() and np.abs(d2.numpy() - ref["d2"]).max() <= 1e-12 * ref["d2"].max()
    assert np.abs((P - G).norm(dim=-1).mean(-1).numpy() - ref["err"]).max() <= 1e-12 * ref["err"].max()
    for t, th in enumerate(case["thr"].tolist()):
        p, r = (d1 < th).double().mean(-1), (d2 < th).double().mean(-1)
        f = torch.where(p + r > 0, 2 * p * r / (p + r).clamp_min(1e-300), torch.zeros_like(p))
        assert np.array_equal(np.rint(p.numpy() * V), ref["count_p"][t]) and np.array_equal(np.rint(r.numpy() * V), ref["count_r"][t])
        assert np.abs(f.numpy() - ref["f"][t]).max() <= 1e-12
    assert ((ref["count_p"] > 0) & (ref["count_p"] < V)).any() or V < 3          # the thresholds cut through the distances: the counts say something


def test_symbol_declared_and_bound_from_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhe.h")).read(), flags=re.S)
    m = re.search(r"\bmhe_mesh_eval_f32\s*\(([^)]*)\)\s*;", src)
    assert m, "mhe_mesh_eval_f32 is not declared in include/mhe.h"
    L = _lib.lib()
    assert "mhe_mesh_eval_f32" in _lib.SIGNATURES and hasattr(L, "mhe_mesh_eval_f32")
    res, args = _lib.SIGNATURES["mhe_mesh_eval_f32"]
    assert res is _lib.C.c_int and len(args) == len(m.group(1).split(",")) == 12
    assert args[:6] == [_lib.C.c_void_p] * 6 and args[6:10] == [_lib.C.c_int] * 4 and args[10] is _lib.C.c_float and args[11] is _lib.C.c_void_p
    assert re.search(r"#define\s+MHE_MESH_EVAL_MAX_THRESHOLDS\s+4\b", src) and ops.MESH_EVAL_MAX_THRESHOLDS == 4 and ops.MESH_EVAL_MAX_VERTS == 778
    assert "mesh_eval.hip" in __import__("mhentropy_amd.build", fromlist=["SOURCES"]).SOURCES
    assert callable(ops.mesh_eval) and callable(criteria.mesh_eval) and callable(criteria.mesh_select)


def test_entry_refuses_bad_arguments_before_any_launch():
    L, Z = _lib.lib(), None
    N, B, V, T = 3, 2, 37, 2
    f = lambda *s: torch.zeros(*s)
    A = lambda t: _lib.C.c_void_p(t.data_ptr())          # host addresses: every call below must return before a kernel could read them
    pred, tgt, sc, thr, err, prf = f(N, B, V, 3), f(B, V, 3), f(B), torch.tensor([5.0, 15.0, 1.0, 2.0, 3.0]), f(N, B), f(3, 5, N, B)

    def call(pred=pred, target=tgt, scale=sc, th=thr, e=err, p=prf, n=N, b=B, v=V, t=T, unit=1000.0):
        return L.mhe_mesh_eval_f32(*(Z if x is None else A(x) for x in (pred, target, scale, th, e, p)), n, b, v, t, unit, Z)
    bad = {"null pred": dict(pred=None), "null target": dict(target=None), "null scale": dict(scale=None), "null thr": dict(th=None),
           "null err": dict(e=None), "null prf": dict(p=None), "V = 0": dict(v=0), "V = 779": dict(v=779), "T = 0": dict(t=0), "T = 5": dict(t=5),
           "N = 0": dict(n=0), "N B = 2^31": dict(n=1 << 16, b=1 << 15), "err overlaps pred": dict(e=pred), "prf overlaps target": dict(p=tgt),
           "err overlaps prf": dict(e=prf), "NaN threshold": dict(th=torch.tensor([5.0, float("nan")])), "NaN unit": dict(unit=float("nan"))}
    for what, kw in bad.items():
        assert call(**kw) == 1 and b"mhe_mesh_eval_f32" in L.mhe_last_error(), what          # MHE_ERR_ARG
    assert call(v=779) == 1 and b"V in 1..778" in L.mhe_last_error()
    assert call(t=5) == 1 and b"T in 1..4" in L.mhe_last_error()
    assert call(e=prf) == 1 and b"overlap" in L.mhe_last_error()


def _cpu_case(N=3, B=2, V=5):
    g = torch.Generator().manual_seed(0)
    out = {"verts": torch.randn(N, B, V * 3, generator=g), "xyz": torch.randn(N, B, 63, generator=g), "faces": torch.zeros(4, 3)}
    tgt = {"verts": torch.randn(B, V * 3, generator=g), "scale": torch.rand(B, generator=g) + 0.5}
    return out, tgt


def test_mesh_eval_error_paths_on_cpu_tensors():
    out, tgt = _cpu_case()
    N, B, V = 3, 2, 5
    drop = lambda d, k: {q: v for q, v in d.items() if q != k}
    with pytest.raises(ValueError, match="output has no 'verts'"):
        criteria.mesh_eval(drop(out, "verts"), tgt)
    with pytest.raises(ValueError, match="target has no 'verts'"):
        criteria.mesh_eval(out, drop(tgt, "verts"))
    with pytest.raises(ValueError, match="target has no 'scale'"):
        criteria.mesh_eval(out, drop(tgt, "scale"))
    with pytest.raises(ValueError, match=r"B=2 images, target\['verts'\] 3"):
        criteria.mesh_eval(out, dict(tgt, verts=torch.zeros(3, V * 3)))
    with pytest.raises(ValueError, match=r"V=5 vertices, target\['verts'\] 4"):
        criteria.mesh_eval(out, dict(tgt, verts=torch.zeros(B, 4, 3)))
    with pytest.raises(ValueError, match=r"target\['scale'\]"):
        criteria.mesh_eval(out, dict(tgt, scale=torch.ones(3)))
    for wrong in (torch.zeros(N, B), torch.zeros(N, B, 16), torch.zeros(N, B, V, 2), torch.zeros(N, B, V, 3, 1)):
        with pytest.raises(ValueError, match=r"output\['verts'\] must be"):
            criteria.mesh_eval(dict(out, verts=wrong), tgt)
    for wrong in (torch.zeros(B), torch.zeros(B, 16), torch.zeros(B, V, 2)):
        with pytest.raises(ValueError, match=r"target\['verts'\] must be"):
            criteria.mesh_eval(out, dict(tgt, verts=wrong))
    for v in (0, 779):
        with pytest.raises(ValueError, match=rf"output\['verts'\] has V={v} vertices per hypothesis \(1..778\)"):
            criteria.mesh_eval({"verts": torch.zeros(N, B, v, 3)}, dict(tgt, verts=torch.zeros(B, v, 3)))
    for th in ((), (1.0, 2.0, 3.0, 4.0, 5.0)):
        with pytest.raises(ValueError, match="thresholds holds"):
            criteria.mesh_eval(out, tgt, thresholds=th)
    for th in ((0.0,), (5.0, -1.0), (float("nan"),)):
        with pytest.raises(ValueError, match="thresholds must be positive"):
            criteria.mesh_eval(out, tgt, thresholds=th)
    for ns in ([0], [N + 1], [1, N + 1], [2, 2], [3, 1], [], [1.0]):
        with pytest.raises(ValueError, match="ns must"):
            criteria.mesh_eval(out, tgt, ns=ns)
    # valid arguments pass every check and reach the device check
    for kw in (dict(), dict(aligned=True), dict(ns=[1, N]), dict(thresholds=(5.0,))):
        with pytest.raises(_lib.MheError, match="CUDA/HIP"):
            criteria.mesh_eval(out, tgt, **kw)
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        criteria.mesh_eval(dict(out, verts=out["verts"].view(N, B, V, 3)), dict(tgt, verts=tgt["verts"].view(B, V, 3)))
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        ops.mesh_eval(torch.zeros(N, B, V, 3), torch.zeros(B, V, 3), torch.ones(B), (5.0,))


def test_mesh_select_error_paths_on_cpu_tensors():
    out, tgt = _cpu_case()
    N = 3
    with pytest.raises(ValueError, match="mesh_select: output has no 'verts'"):
        criteria.mesh_select({k: v for k, v in out.items() if k != "verts"}, tgt)
    for q in (0, N + 1, 1.0):
        with pytest.raises(ValueError, match="mesh_select: Q="):
            criteria.mesh_select(out, tgt, Q=q)
    with pytest.raises(ValueError, match="mesh_select: target has no 'verts'"):
        criteria.mesh_select(out, {"scale": tgt["scale"]})
    with pytest.raises(ValueError, match="mesh_select: output\\['verts'\\] has V=5 vertices, target"):
        criteria.mesh_select(out, dict(tgt, verts=torch.zeros(2, 4, 3)))
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        criteria.mesh_select(out, tgt, Q=2, aligned=True)


def test_run_flag_needs_the_metrics_pass():
    from mhentropy_amd import harness, run
    with pytest.raises(SystemExit, match="--mesh-metrics needs --test-samples"):
        run.main(["--mesh-metrics", "--iters", "1"])
    assert harness.MESH_SCALARS[:6] == ("mesh_err", "mesh_err_pa", "f5", "f15", "f5_pa", "f15_pa") and len(harness.MESH_SCALARS) == 12
