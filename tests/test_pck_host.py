"""CPU: the PCK curve's host side - the f64 restatement the GPU tests compare with (tests/pck_ref.py) against an independent per-point loop, its
seeded cases (every seed and shape tests/test_gpu_pck.py uses converges and keeps its gap), the limits of include/mhe.h against the ops
constants, the C entry's refusals on host memory, and the Python error paths of criteria.pck_auc / pck_select and ops.pck_thresholds, all raised
on CPU tensors before the device is needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

import pck_ref
from conftest import ROOT
from mhentropy_amd import _lib, criteria, harness, ops
from pck_ref import edge_cases, other_cases, walk_cases


def test_reference_agrees_with_a_per_point_loop():
    case = pck_ref.make_case(7, 2, 2, 5, 4, valid_share=0.7)
    valid = np.array(case["valid"])
    valid[0, 0], valid[1] = 1, 0          # image 0 keeps a point, image 1 none
    ref = pck_ref.pck64(case["pred"], case["target"], case["scale"], case["thr"], valid, case["unit"])
    thr = [float(t) for t in case["thr"]]
    for n in range(2):
        for b in range(2):
            su = float(case["scale"][b]) * case["unit"]
            hits, total, nv = [0] * 4, 0.0, 0
            for p in range(5):
                if not valid[b, p]:
                    continue
                d = math.sqrt(sum((float(case["pred"][n, b, p, c]) * su - float(case["target"][b, p, c]) * su) ** 2 for c in range(3)))
                nv += 1
                total += d
                for i in range(4):
                    hits[i] += d <= thr[i]
            assert list(ref["hits"][n, b]) == hits and ref["n_valid"][b] == nv
            if nv == 0:
                assert np.isnan(ref["auc"][n, b]) and np.isnan(ref["err"][n, b])
                continue
            area = sum((thr[i + 1] - thr[i]) * (hits[i] + hits[i + 1]) for i in range(3)) / (2.0 * nv * (thr[3] - thr[0]))
            assert abs(ref["auc"][n, b] - area) <= 1e-15 and abs(ref["err"][n, b] - total / nv) <= 1e-12 * total
    assert ref["n_valid"][1] == 0 and ref["n_valid"][0] >= 1
    # inclusive, and exact arithmetic: a 3-4-0 offset is 5 away
    one = pck_ref.pck64(np.array([[[[3.0, 4.0, 0.0]]]], np.float32), np.zeros((1, 1, 3), np.float32), np.ones(1, np.float32),
                        np.array([np.nextafter(np.float32(5), np.float32(0)), 5.0, 6.0], np.float32), None, 1.0)
    assert list(one["hits"][0, 0]) == [0, 1, 1] and one["gap"] == 0.0
    bad = pck_ref.pck64(np.array([[[[np.nan, 0.0, 0.0], [1.0, 0.0, 0.0]]]], np.float32), np.zeros((1, 2, 3), np.float32), np.ones(1, np.float32),
                        np.array([0.0, 2.0], np.float32), None, 1.0)
    assert list(bad["hits"][0, 0]) == [0, 1] and np.isnan(bad["err"][0, 0]) and bad["auc"][0, 0] == 0.25


@pytest.mark.parametrize("cases", (edge_cases, other_cases, walk_cases))
def test_every_gpu_case_converges_and_keeps_its_gap(cases):
    for seed, N, B, P, T, share in cases():
        case = pck_ref.make_case(seed, N, B, P, T, share)
        d = pck_ref.distances64(case["pred"], case["target"], case["scale"], case["unit"])
        gap = np.abs(d[..., None] - case["thr"].astype(np.float64)).min()          # (every point, valid or not)
        assert gap >= 2 * pck_ref.GAP, ((seed, N, B, P, T), gap)
        assert case["thr"].shape == (T,) and case["thr"][0] == 0.0 and case["thr"][-1] == 50.0 and (np.diff(case["thr"]) > 0).all()
        assert 0.0 < d.min() and d.max() < 50.0
        assert (case["valid"] is None) == (share >= 1.0)


def test_header_limits_equal_the_ops_constants():
    src = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert int(re.search(r"#define\s+MHE_PCK_MAX_POINTS\s+(\d+)", src).group(1)) == ops.PCK_MAX_POINTS == 778
    assert int(re.search(r"#define\s+MHE_PCK_MAX_THRESHOLDS\s+(\d+)", src).group(1)) == ops.PCK_MAX_THRESHOLDS == 256
    assert "UNPINNED" in src[src.index("3D PCK curve"):src.index("MHE_PCK_MAX_POINTS")]
    res, args = _lib.SIGNATURES["mhe_pck_curve_f32"]
    V, I, F = _lib.C.c_void_p, _lib.C.c_int, _lib.C.c_float
    assert res is I and args == [V] * 5 + [F] + [V] * 3 + [I] * 4 + [V]
    assert hasattr(_lib.lib(), "mhe_pck_curve_f32")
    assert "pck.hip" in __import__("mhentropy_amd.build", fromlist=["SOURCES"]).SOURCES


def test_entry_refuses_bad_arguments_before_any_launch():
    L, Z = _lib.lib(), None
    N, B, P, T = 3, 2, 37, 5
    f = lambda *s: torch.zeros(*s)
    A = lambda t: _lib.C.c_void_p(t.data_ptr())          # host addresses: every call below must return before a kernel could read them
    pred, tgt, sc, thr, auc, err = f(N, B, P, 3), f(B, P, 3), f(B), torch.arange(5.0), f(N, B), f(N, B)
    hits, valid = torch.zeros(N, B, T, dtype=torch.int32), torch.ones(B, P, dtype=torch.uint8)

    def call(pred=pred, target=tgt, scale=sc, valid=valid, th=thr, h=hits, a=auc, e=err, n=N, b=B, p=P, t=T, unit=1000.0):
        return L.mhe_pck_curve_f32(*(Z if x is None else A(x) for x in (pred, target, scale, valid, th)), unit,
                                   *(Z if x is None else A(x) for x in (h, a, e)), n, b, p, t, Z)
    bad = {"null pred": dict(pred=None), "null target": dict(target=None), "null scale": dict(scale=None), "null thr": dict(th=None),
           "null auc": dict(a=None), "null err": dict(e=None), "P = 0": dict(p=0), "P = 779": dict(p=779), "T = 1": dict(t=1), "T = 257": dict(t=257),
           "N = 0": dict(n=0), "B = 0": dict(b=0), "N B = 2^31": dict(n=1 << 16, b=1 << 15), "NaN unit": dict(unit=float("nan")),
           "thr in host memory": dict()}
    for what, kw in bad.items():
        assert call(**kw) == 1 and b"mhe_pck_curve_f32" in L.mhe_last_error(), what          # MHE_ERR_ARG
    assert call(p=779) == 1 and b"P in 1..778" in L.mhe_last_error()
    assert call(t=257) == 1 and b"T in 2..256" in L.mhe_last_error()
    assert call() == 1 and b"device memory" in L.mhe_last_error()


def _cpu_case(N=3, B=2, V=5):
    g = torch.Generator().manual_seed(0)
    out = {"verts": torch.randn(N, B, V * 3, generator=g), "xyz": torch.randn(N, B, 63, generator=g), "faces": torch.zeros(4, 3)}
    tgt = {"verts": torch.randn(B, V * 3, generator=g), "pose3d": torch.randn(B, 63, generator=g), "scale": torch.rand(B, generator=g) + 0.5}
    return out, tgt


def test_pck_auc_error_paths_on_cpu_tensors():
    out, tgt = _cpu_case()
    N, B, V = 3, 2, 5
    drop = lambda d, k: {q: v for q, v in d.items() if q != k}
    with pytest.raises(ValueError, match="points='uv'"):
        criteria.pck_auc(out, tgt, points="uv")
    with pytest.raises(ValueError, match="output has no 'xyz'"):
        criteria.pck_auc(drop(out, "xyz"), tgt)
    with pytest.raises(ValueError, match="output has no 'verts'"):
        criteria.pck_auc(drop(out, "verts"), tgt, points="verts")
    with pytest.raises(ValueError, match="target has no 'pose3d'"):
        criteria.pck_auc(out, drop(tgt, "pose3d"))
    with pytest.raises(ValueError, match="target has no 'verts'"):
        criteria.pck_auc(out, drop(tgt, "verts"), points="verts")
    with pytest.raises(ValueError, match="target has no 'scale'"):
        criteria.pck_auc(out, drop(tgt, "scale"))
    with pytest.raises(ValueError, match=r"B=2 images, target\['pose3d'\] 3"):
        criteria.pck_auc(out, dict(tgt, pose3d=torch.zeros(3, 63)))
    with pytest.raises(ValueError, match=r"P=5 points, target\['verts'\] 4"):
        criteria.pck_auc(out, dict(tgt, verts=torch.zeros(B, 4, 3)), points="verts")
    with pytest.raises(ValueError, match=r"target\['scale'\]"):
        criteria.pck_auc(out, dict(tgt, scale=torch.ones(3)))
    for wrong in (torch.zeros(N, B), torch.zeros(N, B, 16), torch.zeros(N, B, V, 2)):
        with pytest.raises(ValueError, match=r"output\['verts'\] must be"):
            criteria.pck_auc(dict(out, verts=wrong), tgt, points="verts")
    for p in (0, 779):
        with pytest.raises(ValueError, match=rf"P={p} points per hypothesis \(1..778\)"):
            criteria.pck_auc({"verts": torch.zeros(N, B, p, 3)}, dict(tgt, verts=torch.zeros(B, p, 3)), points="verts")
    for steps in (1, 257, 0, 100.0, True):
        with pytest.raises(ValueError, match="steps="):
            criteria.pck_auc(out, tgt, steps=steps)
    for vmin, vmax in ((0.0, float("inf")), (float("nan"), 50.0), (float("-inf"), 50.0), (5.0, 5.0), (50.0, 0.0), (0.0, "x")):
        with pytest.raises(ValueError, match="vmin="):
            criteria.pck_auc(out, tgt, vmin=vmin, vmax=vmax)
    with pytest.raises(ValueError, match="not strictly ascending in float32"):
        criteria.pck_auc(out, tgt, vmin=1.0, vmax=1.0 + 1e-6, steps=100)
    for ns in ([0], [N + 1], [1, N + 1], [2, 2], [3, 1], [], [1.0]):
        with pytest.raises(ValueError, match="ns must"):
            criteria.pck_auc(out, tgt, ns=ns)
    for valid in (torch.ones(B, 20, dtype=torch.bool), torch.ones(21, dtype=torch.bool), torch.ones(B, 21), torch.ones(B, 21, dtype=torch.int32),
                  np.ones((B, 21), bool)):
        with pytest.raises(ValueError, match="valid must be"):
            criteria.pck_auc(out, tgt, valid=valid)
    # valid arguments pass every check and reach the device check
    for kw in (dict(), dict(aligned=True), dict(ns=[1, N]), dict(points="verts", curve=True), dict(valid=torch.ones(B, 21, dtype=torch.bool)),
               dict(valid=torch.ones(B, 21, dtype=torch.uint8), steps=2), dict(steps=256, vmin=1.0, vmax=20.0)):
        with pytest.raises(_lib.MheError, match="CUDA/HIP"):
            criteria.pck_auc(out, tgt, **kw)
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        ops.pck_curve(torch.zeros(N, B, V, 3), torch.zeros(B, V, 3), torch.ones(B), (0.0, 5.0))


def test_pck_select_and_threshold_table_error_paths():
    out, tgt = _cpu_case()
    N = 3
    with pytest.raises(ValueError, match="pck_select: points="):
        criteria.pck_select(out, tgt, points="uv")
    with pytest.raises(ValueError, match="pck_select: output has no 'xyz'"):
        criteria.pck_select({k: v for k, v in out.items() if k != "xyz"}, tgt)
    for q in (0, N + 1, 1.0):
        with pytest.raises(ValueError, match="pck_select: Q="):
            criteria.pck_select(out, tgt, Q=q)
    with pytest.raises(ValueError, match="pck_select: target has no 'pose3d'"):
        criteria.pck_select(out, {"scale": tgt["scale"]})
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        criteria.pck_select(out, tgt, Q=2, points="verts", aligned=True)
    for thr in ((1.0,), tuple(range(257)), (0.0, 1.0, 1.0), (0.0, 2.0, 1.0), (0.0, float("nan")), (0.0, float("inf")), (1.0, 1.0 + 1e-9), "ab", 5):
        with pytest.raises(_lib.MheError, match="pck_curve.thresholds"):
            ops.pck_thresholds(thr, "cuda:0")
    with pytest.raises(_lib.MheError, match="CUDA/HIP device"):
        ops.pck_thresholds((0.0, 1.0), "cpu")


def test_run_flag_and_scalar_names():
    from mhentropy_amd import run
    with pytest.raises(SystemExit, match="--pck-metrics needs --test-samples"):
        run.main(["--pck-metrics", "--iters", "1"])
    assert harness.PCK_SCALARS == ("auc_j", "auc_j_pa", "auc_v", "auc_v_pa", "auc_j_best", "auc_j_pa_best", "auc_v_best", "auc_v_pa_best")
    with pytest.raises(ValueError, match="nothing was added"):
        harness.PckPool().curve()


def test_pool_refuses_calls_made_with_different_tables():
    hits, n = torch.ones(2, 3, 4, dtype=torch.int32), torch.full((3,), 5, dtype=torch.int32)
    thr = torch.tensor([0.0, 1.0, 2.0, 3.0])
    pool = harness.PckPool()
    pool.add(hits, n, thr)
    pool.add(hits, n, thr.clone())          # another tensor, the same values
    t, h, total = pool.curve()
    assert h.tolist() == [6, 6, 6, 6] and total == 30 and np.array_equal(t, thr.numpy()) and abs(pool.auc() - 0.2) < 1e-15
    with pytest.raises(ValueError, match="3 thresholds, the pool holds 4"):
        pool.add(hits[..., :3], n, thr[:3])
    pool.add(hits, n, thr + 0.5)          # the same length, other values: found where the host reads
    with pytest.raises(ValueError, match="different thresholds"):
        pool.curve()
