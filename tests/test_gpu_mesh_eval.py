"""GPU tests of the hand mesh evaluation: mhe_mesh_eval_f32 (csrc/mesh_eval.hip) through ops.mesh_eval and the C entry itself, criteria.mesh_eval
(aligned, best of n), criteria.mesh_select and `run --mesh-metrics`.  Values against the float64 restatement of tests/mesh_eval_ref.py, computed
once per case and shared.

Bounds.  err: 1e-4 relative, element by element - the worst case of a fixed-order f32 sum of up to 778 non-negative terms, each good to a few
ulp.  Precision and recall: the reference's counts exactly; every case asserts, in f64, that no nearest distance lies within GAP = 1e-3 relative
of a threshold (mesh_eval_ref.make_case builds its cases that way), f32 rounding of a distance being ~1e-6 relative.  F: 1e-6.

Shapes.  V in {1, 2, 63, 64, 65, 255, 256, 257, 778} (the wave, block and tail edges: 1 to 4 vertices per thread, the four-at-a-time scan and its
tail) x (N, B) in {(1, 1), (3, 2), (5, 3)}, T cycling through 1..4.  The entry gives a workgroup more than one hypothesis only once N B passes
2,048 rows, so the hypothesis walk is met at (N, B) = (701, 3): 351 workgroups per image walk two hypotheses, the last one a single one.  At that
size the f64 parity runs for V <= 65; for V in {255, 256, 257, 600, 778} (1, 2, 3, 4 vertices per thread) the f64 reference would take the CPU
tens of seconds, and the walk is checked bit for bit against the same rows evaluated one hypothesis per workgroup ((N, B) = (1, 2103)), the
path the small shapes pin against f64."""
import functools

import numpy as np
import pytest
import torch

import mesh_eval_ref
from mhentropy_amd import _lib, criteria, ops

pytestmark = pytest.mark.gpu
VS = (1, 2, 63, 64, 65, 255, 256, 257, 778)
SMALL = ((1, 1), (3, 2), (5, 3))
WALK = (701, 3)


def _cu(a):
    return torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared case arrays are read-only)


@functools.lru_cache(None)
def _case(seed, N, B, V, T):
    case = mesh_eval_ref.make_case(seed, N, B, V, T)
    ref = mesh_eval_ref.mesh_eval64(case["pred"], case["target"], case["scale"], case["thr"], case["unit"])
    assert ref["gap"] >= mesh_eval_ref.GAP, ((seed, N, B, V, T), ref["gap"])
    return case, ref


def _run(case):
    err, prf = ops.mesh_eval(_cu(case["pred"]), _cu(case["target"]), _cu(case["scale"]), case["thr"].tolist(), case["unit"])
    torch.cuda.synchronize()
    return err.cpu().numpy(), prf.cpu().numpy()


def _check(what, case, ref):
    N, B, V = case["pred"].shape[:3]
    T = len(case["thr"])
    err, prf = _run(case)
    assert err.shape == (N, B) and prf.shape == (3, T, N, B) and err.dtype == prf.dtype == np.float32
    rel = np.abs(err - ref["err"]) / ref["err"]
    print(f"{what}: err rel {rel.max():.2e}; F diff {np.abs(prf[2] - ref['f']).max():.2e}; f64 gap {ref['gap']:.2e}; "
          f"precision {ref['precision'].min():.2f}..{ref['precision'].max():.2f}")
    assert (rel <= 1e-4).all(), (what, rel.max())
    assert np.array_equal(np.rint(prf[0].astype(np.float64) * V), ref["count_p"]), what + ": precision counts"
    assert np.array_equal(np.rint(prf[1].astype(np.float64) * V), ref["count_r"]), what + ": recall counts"
    assert np.abs(prf[0] - ref["precision"]).max() <= 1e-6 and np.abs(prf[1] - ref["recall"]).max() <= 1e-6
    assert np.abs(prf[2] - ref["f"]).max() <= 1e-6, what + ": F"


@pytest.mark.parametrize("V", VS)
def test_parity_at_the_edges(V, gpu_lib):
    for i, (N, B) in enumerate(SMALL):
        T = 1 + (VS.index(V) + i) % 4
        _check(f"V={V} N={N} B={B} T={T}", *_case(1000 + 10 * V + i, N, B, V, T))


@pytest.mark.parametrize("V", (1, 2, 63, 64, 65))
def test_parity_of_the_hypothesis_walk(V, gpu_lib):
    N, B = WALK
    T = 1 + VS.index(V) % 4
    _check(f"walk V={V} T={T}", *_case(2000 + V, N, B, V, T))


@pytest.mark.parametrize("V", (255, 256, 257, 600, 778))
def test_hypothesis_walk_equals_one_hypothesis_per_workgroup(V, gpu_lib):
    N, B = WALK
    g = torch.Generator().manual_seed(3000 + V)
    target = torch.randn(B, V, 3, generator=g)
    pred = (target[None] + 0.15 * torch.randn(N, B, V, 3, generator=g)).cuda()
    target, scale = target.cuda(), (0.025 + 0.015 * torch.rand(B, generator=g)).cuda()
    thr = (5.0, 15.0, 2.5, 10.0)
    err, prf = ops.mesh_eval(pred, target, scale, thr)
    err1, prf1 = ops.mesh_eval(pred.view(1, N * B, V, 3), target.repeat(N, 1, 1), scale.repeat(N), thr)          # row r = n B + b: image r % B
    assert torch.equal(err, err1.view(N, B)) and torch.equal(prf, prf1.view(3, 4, N, B))
    assert 0.05 < float(prf[0].mean()) < 0.95          # the thresholds cut through the distances


# ---- strictness and degenerate cases, in exactly representable numbers -------------------------------------------------------------------------
def _grid(V, step=10.0):
    v = np.arange(V)
    return np.stack([step * (v % 7), step * ((v // 7) % 7), step * (v // 49)], 1).astype(np.float32)          # neighbours `step` apart


def _exact(pred, target, thr):
    """integer coordinates, scale = 1, unit = 1 -> (err, prf) of the kernel and the f64 reference"""
    B = target.shape[0]
    one = np.ones(B, np.float32)
    err, prf = ops.mesh_eval(_cu(pred), _cu(target), _cu(one), list(thr), unit=1.0)
    torch.cuda.synchronize()
    return err.cpu().numpy(), prf.cpu().numpy(), mesh_eval_ref.mesh_eval64(pred, target, one, np.asarray(thr, np.float64), 1.0)


@pytest.mark.parametrize("V", (1, 65, 300, 778))
def test_the_comparison_is_strict(V, gpu_lib):
    thr = 3.0
    target = _grid(V)[None]
    pred = (target + np.array([thr, 0.0, 0.0], np.float32))[None]          # every nearest distance is exactly thr (the neighbours are 10 apart)
    err, prf, ref = _exact(pred, target, (thr, thr + 1.0))
    assert np.array_equal(ref["d1"], np.full((1, 1, V), thr)) and np.array_equal(ref["d2"], np.full((1, 1, V), thr))
    assert np.array_equal(err, np.full((1, 1), thr, np.float32))
    assert np.array_equal(prf[:, 0], np.zeros((3, 1, 1), np.float32)), "distance == thr must not be counted"
    assert np.array_equal(prf[:, 1], np.ones((3, 1, 1), np.float32)), "thr + 1 counts every vertex"


def test_identical_far_and_duplicate_vertices(gpu_lib):
    V = 300
    target = np.stack([_grid(V), _grid(V) + 1.0])          # B = 2
    same = np.broadcast_to(target[None], (2, 2, V, 3)).copy()
    err, prf, _ = _exact(same, target, (2.0, 50.0))
    assert np.array_equal(err, np.zeros((2, 2), np.float32)) and np.array_equal(prf, np.ones((3, 2, 2, 2), np.float32))
    far = same + np.array([0.0, 10000.0, 0.0], np.float32)
    err, prf, _ = _exact(far, target, (2.0, 50.0, 9000.0))          # (the grid spans 60 in y: the nearest vertex of the other set is >= 9940 away)
    assert np.array_equal(err, np.full((2, 2), 10000.0, np.float32))
    assert np.array_equal(prf, np.zeros((3, 3, 2, 2), np.float32)), "all out of range: P = R = 0 and F = 0, not NaN"
    # duplicates: every vertex twice in both sets, and two predicted vertices at one distance of a target vertex - the minima meet ties
    dup = np.concatenate([target[:, :150], target[:, :150]], 1)
    pred = dup[None] + np.array([[[[3.0, 0.0, 0.0]]], [[[0.0, 4.0, 0.0]]], [[[5.0, 5.0, 0.0]]]], np.float32)          # (3, 1, 1, 3) shifts: N = 3
    err, prf, ref = _exact(pred.astype(np.float32), dup, (3.0, 4.0, 5.0, 8.0))
    assert (np.abs(err - ref["err"]) <= 1e-4 * ref["err"]).all()
    assert np.array_equal(np.rint(prf[0].astype(np.float64) * V), ref["count_p"]) and np.array_equal(np.rint(prf[1].astype(np.float64) * V), ref["count_r"])
    assert np.abs(prf[2] - ref["f"]).max() <= 1e-6
    assert ref["count_p"].min() == 0 and ref["count_p"].max() == V          # (3 < 3 is false, 3 < 4 true, ...: both ends are met)


# ---- layout and determinism --------------------------------------------------------------------------------------------------------------------
def test_rows_scale_and_determinism(gpu_lib):
    case, _ = _case(1000 + 10 * 257 + 2, 5, 3, 257, 1 + (VS.index(257) + 2) % 4)
    pred, target, scale, thr = _cu(case["pred"]), _cu(case["target"]), _cu(case["scale"]), case["thr"].tolist()
    err, prf = ops.mesh_eval(pred, target, scale, thr)
    err2, prf2 = ops.mesh_eval(pred, target, scale, thr)
    assert torch.equal(err, err2) and torch.equal(prf, prf2), "two calls must give the same bits"
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    errp, prfp = ops.mesh_eval(pred[perm].contiguous(), target, scale, thr)
    assert torch.equal(errp, err[perm]) and torch.equal(prfp, prf[:, :, perm]), "shuffled hypotheses permute the outputs"
    assert len(set(case["scale"].tolist())) == 3
    for b in range(3):          # one call with three scales = three single-image calls
        e1, p1 = ops.mesh_eval(pred[:, b:b + 1].contiguous(), target[b:b + 1].contiguous(), scale[b:b + 1].contiguous(), thr)
        assert torch.equal(e1[:, 0], err[:, b]) and torch.equal(p1[..., 0], prf[..., b])
    # ... and the scale matters: another scale, other counts
    e3, p3 = ops.mesh_eval(pred, target, scale * 2.0, thr)
    assert torch.allclose(e3, err * 2.0, rtol=1e-6) and not torch.equal(p3, prf)


# ---- argument refusals of the C entry ---------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_with_device_memory(gpu_lib):
    L, Z = gpu_lib, None
    N, B, V, T = 3, 2, 37, 2
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    A = lambda t: _lib.C.c_void_p(t.data_ptr())
    pred, tgt, sc, err, prf = f(N, B, V, 3), f(B, V, 3), f(B), f(N, B), f(3, 5, N, B)
    thr = (_lib.C.c_float * 5)(5.0, 15.0, 1.0, 2.0, 3.0)
    TH = _lib.C.cast(thr, _lib.C.c_void_p)

    def call(pred=pred, target=tgt, scale=sc, th=TH, e=err, p=prf, n=N, b=B, v=V, t=T):
        return L.mhe_mesh_eval_f32(*(Z if x is None else A(x) for x in (pred, target, scale)), th, *(Z if x is None else A(x) for x in (e, p)),
                                   n, b, v, t, 1000.0, _lib.C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = {"V = 0": dict(v=0), "V = 779": dict(v=779), "T = 0": dict(t=0), "T = 5": dict(t=5), "null pred": dict(pred=None),
           "null target": dict(target=None), "null scale": dict(scale=None), "null thr": dict(th=Z), "null err": dict(e=None), "null prf": dict(p=None),
           "err overlaps pred": dict(e=pred), "prf overlaps target": dict(p=tgt), "err overlaps prf": dict(e=prf), "N B = 2^31": dict(n=1 << 16, b=1 << 15)}
    for what, kw in bad.items():
        assert call(**kw) == 1 and b"mhe_mesh_eval_f32" in L.mhe_last_error(), what          # MHE_ERR_ARG
    torch.cuda.synchronize()
    for t in (pred, tgt, sc, err, prf):
        assert bool((t == 7.0).all()), "a refused call must not launch"
    assert call() == 0


# ---- the public interface ---------------------------------------------------------------------------------------------------------------------
def _sample_output(seed=5, N=6, B=3, V=65, T=2):
    case, ref = _case(seed, N, B, V, T)
    pred = _cu(case["pred"])
    pred[2], pred[4] = pred[0], pred[1]          # planted ties between hypotheses (rows 0 = 2, 1 = 4)
    out = {"verts": pred.view(N, B, V * 3), "xyz": torch.randn(N, B, 63, device="cuda"), "log_q": torch.randn(N, B, device="cuda"),
           "faces": torch.zeros(N, B, dtype=torch.int64, device="cuda"), "image": torch.zeros(N, B, 4, device="cuda")}
    tgt = {"verts": _cu(case["target"]).view(B, V * 3), "scale": _cu(case["scale"])}
    return case, out, tgt


def test_criteria_mesh_eval_forms_alignment_and_best_of_n(gpu_lib):
    case, out, tgt = _sample_output()
    N, B, V = 6, 3, 65
    pv, tv = out["verts"].view(N, B, V, 3), tgt["verts"].view(B, V, 3)
    before, ptr = out["verts"].clone(), out["verts"].data_ptr()
    err, prf = ops.mesh_eval(pv.contiguous(), tv.contiguous(), tgt["scale"], (5.0, 15.0))
    for o, t in ((out, tgt), (dict(out, verts=pv), dict(tgt, verts=tv)), (dict(out, verts=pv.requires_grad_(True)), tgt)):
        res = criteria.mesh_eval(o, t)
        assert set(res) == {"mesh_err", "precision", "recall", "f_score"} and not res["mesh_err"].requires_grad
        assert res["mesh_err"].shape == (N, B) and all(res[k].shape == (2, N, B) for k in ("precision", "recall", "f_score"))
        assert torch.equal(res["mesh_err"], err) and torch.equal(res["precision"], prf[0]) and torch.equal(res["recall"], prf[1])
        assert torch.equal(res["f_score"], prf[2])
    one = criteria.mesh_eval(out, tgt, thresholds=[15.0])
    assert one["f_score"].shape == (1, N, B) and torch.equal(one["f_score"][0], prf[2, 1])
    # aligned: the existing Procrustes kernel's output, evaluated; the caller's tensor is neither replaced nor written
    al = ops.procrustes_align(out["verts"].contiguous(), tgt["verts"].contiguous())
    err_a, prf_a = ops.mesh_eval(al.view(N, B, V, 3), tv.contiguous(), tgt["scale"], (5.0, 15.0))
    res = criteria.mesh_eval(out, tgt, aligned=True)
    assert torch.equal(res["mesh_err"], err_a) and torch.equal(res["f_score"], prf_a[2]) and not torch.equal(err_a, err)
    assert out["verts"].data_ptr() == ptr and torch.equal(out["verts"], before)
    # best of the first n: torch.min / torch.max over the first n rows, index ties to the lower n
    ns = [1, 2, 3, 5, 6]
    res = criteria.mesh_eval(out, tgt, ns=ns)
    assert set(res) == {"mesh_err", "precision", "recall", "f_score", "mesh_err_min", "mesh_err_index", "f_score_max"}
    assert res["mesh_err_min"].shape == (5, B) and res["mesh_err_index"].shape == (5, B) and res["mesh_err_index"].dtype == torch.int64
    assert res["f_score_max"].shape == (2, 5, B)
    assert torch.equal(err[2], err[0]) and torch.equal(err[4], err[1])
    for i, n in enumerate(ns):
        assert torch.equal(res["mesh_err_min"][i], err[:n].min(0).values)
        first = (err[:n] == err[:n].min(0).values[None]).float().argmax(0)          # the lowest n attaining the minimum
        assert torch.equal(res["mesh_err_index"][i], first)
        assert torch.equal(res["f_score_max"][:, i], prf[2][:, :n].max(1).values)
    assert bool((res["mesh_err_index"] != 2).all() and (res["mesh_err_index"] != 4).all())          # a planted twin never wins over its original
    assert torch.equal(criteria.mesh_eval(out, tgt, ns=[N])["mesh_err_min"][0], err.min(0).values)


def test_mesh_select_is_a_stable_sort_of_mesh_err(gpu_lib):
    case, out, tgt = _sample_output()
    N, B = 6, 3
    cols = torch.arange(B, device="cuda")
    for aligned in (False, True):
        err = criteria.mesh_eval(out, tgt, aligned=aligned)["mesh_err"]
        val, order = torch.sort(err, dim=0, stable=True)
        for Q in (1, 4, N):
            sel = criteria.mesh_select(out, tgt, Q=Q, aligned=aligned)
            assert set(sel) == set(out) | {"mesh_err", "mesh_err_index"}
            assert torch.equal(sel["mesh_err"], val[:Q]) and torch.equal(sel["mesh_err_index"], order[:Q]) and sel["mesh_err_index"].dtype == torch.int64
            for k in ("verts", "xyz", "log_q"):          # every (N, B, ...) tensor is cut to (Q, B, ...), chamfer_select's convention
                assert sel[k].shape[:2] == (Q, B) and torch.equal(sel[k], out[k][order[:Q], cols])
            assert sel["faces"] is out["faces"] and sel["image"] is out["image"]
    sel = criteria.mesh_select(out, tgt, Q=N)
    pos = {int(n): i for i, n in enumerate(sel["mesh_err_index"][:, 0].tolist())}
    assert pos[0] < pos[2] and pos[1] < pos[4], "ties go to the lower n"


# ---- the trainer shell ------------------------------------------------------------------------------------------------------------------------
def test_run_mesh_metrics(gpu_lib, tmp_path):
    import json
    from mhentropy_amd import harness, run
    common = ["--backbone", "resnet18", "--batch", "4", "--hyps", "4", "--test-samples", "3", "--hidden", "64", "--flow-steps", "2", "--dtype", "f32",
              "--epochs", "1", "--iters", "2", "--image-size", "96"]
    tags = {"metric_it/" + k for k in harness.MESH_SCALARS}
    for flag in (True, False):
        sc = tmp_path / f"scalars_{int(flag)}.jsonl"
        log = run.main(common + ["--scalars", str(sc)] + (["--mesh-metrics"] if flag else []))
        rows = [json.loads(line) for line in open(sc)]
        seen = {r["tag"] for r in rows}
        assert len(log) == 1 and np.isfinite(log[0]["loss"])
        if flag:
            assert tags <= seen and all(np.isfinite(r["value"]) for r in rows if r["tag"] in tags)
            assert sum(r["tag"] == "metric_it/mesh_err" for r in rows) == 2
            assert all(np.isfinite(log[0][k]) for k in harness.MESH_SCALARS)
            assert log[0]["mesh_err_best"] <= log[0]["mesh_err"]
            assert log[0]["f15_best"] >= log[0]["f15"] and 0.0 <= log[0]["f5"] <= 1.0
        else:
            assert not (tags & seen) and not (set(harness.MESH_SCALARS) & set(log[0]))
