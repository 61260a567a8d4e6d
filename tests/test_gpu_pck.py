"""GPU tests of the 3D PCK curve: mhe_pck_curve_f32 (csrc/pck.hip) through ops.pck_curve and the C entry itself, criteria.pck_auc (aligned, best
of n, curve), criteria.pck_select, harness.PckPool and `run --pck-metrics`.  Values against the float64 restatement of tests/pck_ref.py, computed
once per case and shared.

Bounds.  hits: the reference's integers exactly; every case asserts, in f64, that no distance lies within GAP = 1e-3 mm of a threshold
(pck_ref.make_case builds its cases that way), f32 rounding of a distance below 50 mm being ~1e-5 mm.  auc: 2 f32 ulp = 2.4e-7 relative - both
sides evaluate one f64 expression of the same integers and round once; only the order of the f64 sum differs.  err: 1e-4 relative, the bound
tests/test_gpu_mesh_eval.py derives for a fixed-order f32 sum of up to 778 non-negative terms.

Shapes.  P in {1, 2, 21, 63, 64, 65, 255, 256, 257, 778}: the kernel serves a hypothesis with 32 lanes (P <= 32), 64 (<= 64) or the whole
256-thread workgroup (1 to 4 points per thread), x (N, B) in {(1, 1), (3, 2), (5, 3)}, T cycling through {2, 3, 100, 255, 256} (1 to 8 bins per
finishing lane)."""
import functools

import numpy as np
import pytest
import torch

import pck_ref
from mhentropy_amd import _lib, criteria, harness, ops
from pck_ref import PS, SMALL, TS, WALK

pytestmark = pytest.mark.gpu
ULP2 = 2.4e-7


def _cu(a):
    return None if a is None else torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared case arrays are read-only)


@functools.lru_cache(None)
def _case(seed, N, B, P, T, share=1.0):
    case = pck_ref.make_case(seed, N, B, P, T, share)
    ref = pck_ref.pck64(case["pred"], case["target"], case["scale"], case["thr"], case["valid"], case["unit"])
    assert ref["gap"] >= pck_ref.GAP, ((seed, N, B, P, T), ref["gap"])
    return case, ref


def _run(case, valid="case", **kw):
    valid = case["valid"] if isinstance(valid, str) else valid
    hits, auc, err = ops.pck_curve(_cu(case["pred"]), _cu(case["target"]), _cu(case["scale"]), _cu(case["thr"]), _cu(valid), case["unit"], **kw)
    torch.cuda.synchronize()
    return None if hits is None else hits.cpu().numpy(), auc.cpu().numpy(), err.cpu().numpy()


def _compare(what, got, ref):
    hits, auc, err = got
    assert hits.dtype == np.int32 and auc.dtype == err.dtype == np.float32
    assert hits.shape == ref["hits"].shape and auc.shape == err.shape == ref["auc"].shape
    live = np.broadcast_to(ref["n_valid"][None] > 0, auc.shape)
    rel_a = np.abs(auc[live] - ref["auc"][live]) / np.maximum(ref["auc"][live], 1e-30)
    rel_e = np.abs(err[live] - ref["err"][live]) / ref["err"][live]
    print(f"{what}: hits differ at {int((hits != ref['hits']).sum())}; auc rel {rel_a.max(initial=0):.2e}; err rel {rel_e.max(initial=0):.2e}; "
          f"f64 gap {ref['gap']:.2e} mm; auc {np.nanmin(ref['auc']):.3f}..{np.nanmax(ref['auc']):.3f}")
    assert np.array_equal(hits, ref["hits"]), what + ": hits"
    assert (rel_a <= ULP2).all(), (what, "auc", rel_a.max())
    assert (rel_e <= 1e-4).all(), (what, "err", rel_e.max())
    assert np.isnan(auc[~live]).all() and np.isnan(err[~live]).all() and not hits[~live].any(), what + ": an image without a valid point"


def _check(what, case, ref):
    _compare(what, _run(case), ref)


@pytest.mark.parametrize("P", PS)
def test_parity_at_the_edges(P, gpu_lib):
    for i, (N, B) in enumerate(SMALL):
        T = TS[(PS.index(P) + i) % len(TS)]
        _check(f"P={P} N={N} B={B} T={T}", *_case(1000 + 10 * P + i, N, B, P, T))


# ---- the inclusive boundary, in exactly representable numbers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (4, 21, 64, 300))
def test_the_comparison_is_inclusive(P, gpu_lib):
    f = np.float32
    offs = np.array([[0, 0, 0], [3, 4, 0], [5, 12, 0], [9, 12, 0]], f)          # distances exactly 0, 5, 13, 15
    down, up = (lambda x: np.nextafter(f(x), f(-1e9))), (lambda x: np.nextafter(f(x), f(1e9)))
    thr = np.array([0.0, up(0), down(5), 5.0, up(5), down(13), 13.0, up(13), 14.0], f)          # 15 lies above thr[T - 1]
    assert (np.diff(thr) > 0).all()
    target = np.stack([np.arange(P), 7 * np.arange(P) % 11, np.arange(P) % 3], 1).astype(f)[None]          # B = 1, integers
    pred = np.stack([target + offs[(np.arange(P) + s) % 4][None] for s in range(3)])          # N = 3: the offsets rotate over the points
    one = np.ones(1, f)
    ref = pck_ref.pck64(pred, target, one, thr, None, 1.0)
    assert set(np.unique(ref["d"])) == {0.0, 5.0, 13.0, 15.0} and ref["gap"] == 0.0
    hits, auc, err = ops.pck_curve(_cu(pred), _cu(target), _cu(one), _cu(thr), None, 1.0)
    hits, auc, err = hits.cpu().numpy(), auc.cpu().numpy(), err.cpu().numpy()
    assert np.array_equal(hits, ref["hits"]), "the counts must be the reference's to the integer"
    for n in range(3):
        k = [(ref["d"][n, 0] == v).sum() for v in (0.0, 5.0, 13.0, 15.0)]
        assert list(hits[n, 0]) == [k[0], k[0], k[0], k[0] + k[1], k[0] + k[1], k[0] + k[1], k[0] + k[1] + k[2], k[0] + k[1] + k[2], k[0] + k[1] + k[2]]
        assert k[0] > 0 and k[3] > 0 and hits[n, 0, -1] == P - k[3]          # 0 counts at thr[0] = 0; 15 counts nowhere
    assert (np.abs(auc - ref["auc"]) <= ULP2 * ref["auc"]).all() and (np.abs(err - ref["err"]) <= 1e-4 * ref["err"]).all()
    # the same table as a Python sequence: checked, uploaded once and kept
    h2, a2, e2 = ops.pck_curve(_cu(pred), _cu(target), _cu(one), thr.tolist(), None, 1.0)
    assert np.array_equal(h2.cpu().numpy(), hits) and np.array_equal(a2.cpu().numpy(), auc)
    assert ops.pck_thresholds(thr.tolist(), "cuda") is ops.pck_thresholds(tuple(thr.tolist()), torch.device("cuda", torch.cuda.current_device()))


# ---- valid masks and non-finite coordinates ---------------------------------------------------------------------------------------------------
def test_a_random_mask(gpu_lib):
    case, ref = _case(2000, 4, 3, 65, 100, 0.6)
    assert 0 < ref["n_valid"].min() and ref["n_valid"].max() < 65
    _compare("random mask", _run(case), ref)
    as_bool = ops.pck_curve(_cu(case["pred"]), _cu(case["target"]), _cu(case["scale"]), _cu(case["thr"]), _cu(case["valid"]).bool())
    assert np.array_equal(as_bool[0].cpu().numpy(), ref["hits"])


def test_an_image_with_one_valid_point_and_one_with_none(gpu_lib):
    case, full = _case(2001, 3, 3, 300, 100)
    clean = _run(case, valid=None)
    _compare("no mask", clean, full)
    valid = np.ones((3, 300), np.uint8)
    valid[0] = 0
    valid[0, 257] = 1          # image 0: one valid point, one of a thread's second round; image 1: none
    valid[1] = 0
    ref = pck_ref.pck64(case["pred"], case["target"], case["scale"], case["thr"], valid, case["unit"])
    assert list(ref["n_valid"]) == [1, 0, 300]
    got = _run(case, valid=valid)
    _compare("one valid point / none", got, ref)
    assert np.isnan(got[1][:, 1]).all() and np.isnan(got[2][:, 1]).all() and not got[0][:, 1].any()
    assert set(np.unique(got[0][:, 0])) <= {0, 1} and got[0][:, 0, -1].all()
    for a, b in zip(got, clean):          # image 2's rows: the bits of the run without any mask
        assert np.array_equal(a[:, 2], b[:, 2])
    only1 = np.ones((3, 300), np.uint8)
    only1[1] = 0
    got1 = _run(case, valid=only1)
    for a, b in zip(got1, clean):
        assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 2], b[:, 2])


@pytest.mark.parametrize("P", (21, 300))
def test_a_non_finite_coordinate_stays_in_its_row(P, gpu_lib):
    case, ref = _case(2001, 3, 3, 300, 100) if P == 300 else _case(2002, 6, 3, 21, 100)
    clean = _run(case)
    for bad in (np.nan, np.inf):
        pred = np.array(case["pred"])
        pred[1, 2, P - 1, 1] = bad
        got = _run(dict(case, pred=pred))
        r64 = pck_ref.pck64(pred, case["target"], case["scale"], case["thr"], None, case["unit"])
        assert np.array_equal(got[0], r64["hits"]) and np.isnan(got[2][1, 2]) and np.isnan(r64["err"][1, 2])
        assert got[0][1, 2, -1] == P - 1 and clean[0][1, 2, -1] == P          # the point hits nothing, the row's other points count
        assert abs(got[1][1, 2] - r64["auc"][1, 2]) <= ULP2 * r64["auc"][1, 2]
        mask = np.ones(got[1].shape, bool)
        mask[1, 2] = False
        for a, b in zip(got, clean):
            assert np.array_equal(a[mask], b[mask]), "every other row: the bits of the clean run"


# ---- the hypothesis walk ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (21, 65))
def test_parity_of_the_hypothesis_walk(P, gpu_lib):
    """The entry asks for at most 2,048 workgroups: an image's N hypotheses are split over min(N, ceil(2048 / B)) of them, so a workgroup is
    handed more than one hypothesis once N > ceil(2048 / B).  The fewest rows at which that happens are (N, B) = (2049, 1); with more than one
    image, B = 3 needs N = 684 - the shape used here: 342 workgroups per image, two hypotheses each (one after the other at P = 65, side by
    side in one wave at P = 21)."""
    N, B = WALK
    assert N == -(-2048 // B) + 1
    _check(f"walk P={P}", *_case(3000 + P, N, B, P, 100))


def test_hypothesis_walk_equals_one_hypothesis_per_workgroup(gpu_lib):
    """(N, B) = (684, 3) at P = 778 against the same rows as (1, 2052), where every workgroup has one hypothesis - the path the small shapes pin
    against f64 (the f64 reference at this size would take the CPU tens of seconds)."""
    (N, B), P = WALK, 778
    g = torch.Generator().manual_seed(3778)
    target = torch.randn(B, P, 3, generator=g)
    pred = (target[None] + 0.15 * torch.randn(N, B, P, 3, generator=g)).cuda()
    target, scale = target.cuda(), (0.025 + 0.015 * torch.rand(B, generator=g)).cuda()
    valid = (torch.rand(B, P, generator=g) < 0.8).cuda()
    thr = np.linspace(0.0, 50.0, 100).tolist()
    a = ops.pck_curve(pred, target, scale, thr, valid)
    b = ops.pck_curve(pred.view(1, N * B, P, 3), target.repeat(N, 1, 1), scale.repeat(N), thr, valid.repeat(N, 1))          # row r = n B + b: image r % B
    assert torch.equal(a[0], b[0].view(N, B, 100)) and torch.equal(a[1], b[1].view(N, B)) and torch.equal(a[2], b[2].view(N, B))
    assert 0.5 < float(a[1].mean()) < 0.95 and int(a[0].max()) <= int(valid.sum(1).max())


@pytest.mark.parametrize("P", (2, 21, 64))
def test_rounds_of_a_packed_workgroup_equal_one_hypothesis_per_workgroup(P, gpu_lib):
    """At P <= 64 a workgroup serves 8 (P <= 32) or 4 hypotheses side by side, so it walks them in more than one round only once it is handed more
    than that: B = 1, N = 32,770 gives each of 1,928 workgroups 17 hypotheses (3 rounds at P = 2 and 21, 5 at P = 64, the last one partly idle).
    Compared bit for bit with the same hypotheses run 2,048 at a time, one per workgroup."""
    N = 32770
    g = torch.Generator().manual_seed(4000 + P)
    target = torch.randn(1, P, 3, generator=g)
    pred = (target[None] + 0.15 * torch.randn(N, 1, P, 3, generator=g)).cuda()
    target, scale = target.cuda(), torch.tensor([0.03], device="cuda")
    thr = np.linspace(0.0, 50.0, 100).tolist()
    whole = ops.pck_curve(pred, target, scale, thr)
    parts = [ops.pck_curve(pred[i:i + 2048].contiguous(), target, scale, thr) for i in range(0, N, 2048)]
    for k in range(3):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts]))
    assert 0.5 < float(whole[1].mean()) < 0.95


def test_two_launches_give_the_same_bits(gpu_lib):
    for key in ((2001, 3, 3, 300, 100), (2002, 6, 3, 21, 100), (2000, 4, 3, 65, 100, 0.6)):
        case, _ = _case(*key)
        a, b = _run(case), _run(case)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
        none = _run(case, want_hits=False)
        assert none[0] is None and np.array_equal(none[1], a[1]) and np.array_equal(none[2], a[2]), "the values do not depend on want_hits"


# ---- argument refusals of the C entry ---------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_with_device_memory(gpu_lib):
    """R = N B by the entry's signature, so `R % B != 0` cannot be passed; its place is taken by N < 1 and B < 1."""
    L, Z = gpu_lib, None
    N, B, P, T = 3, 2, 37, 5
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    A = lambda t: _lib.C.c_void_p(t.data_ptr())
    pred, tgt, sc, auc, err = f(N, B, P, 3), f(B, P, 3), f(B), f(N, B), f(N, B)
    thr = torch.arange(300.0, device="cuda")
    hits, valid = torch.full((N, B, 300), 7, dtype=torch.int32, device="cuda"), torch.full((B, P), 7, dtype=torch.uint8, device="cuda")
    host_thr = torch.arange(5.0)

    def call(pred=pred, target=tgt, scale=sc, valid=valid, th=thr, h=hits, a=auc, e=err, n=N, b=B, p=P, t=T):
        return L.mhe_pck_curve_f32(*(Z if x is None else A(x) for x in (pred, target, scale, valid, th)), 1000.0,
                                   *(Z if x is None else A(x) for x in (h, a, e)), n, b, p, t,
                                   _lib.C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = {"T = 1": dict(t=1), "T = 257": dict(t=257), "P = 779": dict(p=779), "P = 0": dict(p=0), "N = 0": dict(n=0), "B = 0": dict(b=0),
           "N B = 2^31": dict(n=1 << 16, b=1 << 15), "null pred": dict(pred=None), "null thr": dict(th=None), "null auc": dict(a=None),
           "null err": dict(e=None), "thr in host memory": dict(th=host_thr), "auc overlaps pred": dict(a=pred), "err overlaps target": dict(e=tgt),
           "hits overlaps thr": dict(h=thr), "err overlaps valid": dict(e=valid), "auc overlaps err": dict(a=err), "hits overlaps auc": dict(h=auc)}
    for what, kw in bad.items():
        assert call(**kw) == 1 and b"mhe_pck_curve_f32" in L.mhe_last_error(), what          # MHE_ERR_ARG
    torch.cuda.synchronize()
    for t in (pred, tgt, sc, auc, err, hits, valid):
        assert bool((t == 7).all()), "a refused call must not launch"
    assert call() == 0 and call(h=None, valid=None) == 0
    torch.cuda.synchronize()


# ---- the public interface ---------------------------------------------------------------------------------------------------------------------
def _sample_output():
    cj, _ = _case(2002, 6, 3, 21, 100)
    cv, _ = _case(2003, 6, 3, 65, 100)
    N, B = 6, 3
    xyz, verts = _cu(cj["pred"]), _cu(cv["pred"])
    for t in (xyz, verts):
        t[2], t[4] = t[0], t[1]          # planted ties between hypotheses (rows 0 = 2, 1 = 4)
    out = {"xyz": xyz.view(N, B, 63), "verts": verts.view(N, B, 65 * 3), "log_q": torch.randn(N, B, device="cuda"),
           "faces": torch.zeros(N, B, dtype=torch.int64, device="cuda"), "image": torch.zeros(N, B, 4, device="cuda")}
    tgt = {"pose3d": _cu(cj["target"]).view(B, 63), "verts": _cu(cv["target"]).view(B, 65 * 3), "scale": _cu(cj["scale"])}
    return out, tgt


def test_criteria_pck_auc_forms_alignment_curve_and_best_of_n(gpu_lib):
    out, tgt = _sample_output()
    N, B = 6, 3
    thr = np.linspace(0.0, 50.0, 100).astype(np.float32)
    for points, key, P in (("xyz", "pose3d", 21), ("verts", "verts", 65)):
        pv, tv = out[points].view(N, B, P, 3).contiguous(), tgt[key].view(B, P, 3).contiguous()
        before, ptr = out[points].clone(), out[points].data_ptr()
        hits, auc, err = ops.pck_curve(pv, tv, tgt["scale"], _cu(thr))
        for o, t in ((out, tgt), ({**out, points: pv}, {**tgt, key: tv}), ({**out, points: pv.clone().requires_grad_(True)}, tgt)):
            res = criteria.pck_auc(o, t, points=points)
            assert set(res) == {"auc", "err", "thresholds"} and not res["auc"].requires_grad
            assert torch.equal(res["auc"], auc) and torch.equal(res["err"], err) and np.array_equal(res["thresholds"].cpu().numpy(), thr)
        ref = pck_ref.pck64(pv.cpu().numpy(), tv.cpu().numpy(), tgt["scale"].cpu().numpy(), thr)
        assert np.array_equal(hits.cpu().numpy(), ref["hits"])
        # curve=True: the integer curve and the valid points
        res = criteria.pck_auc(out, tgt, points=points, curve=True)
        assert set(res) == {"auc", "err", "thresholds", "hits", "n_valid"} and res["hits"].dtype == res["n_valid"].dtype == torch.int32
        assert torch.equal(res["hits"], hits) and res["n_valid"].tolist() == [P] * B and bool((res["hits"][..., -1] <= res["n_valid"][None]).all())
        valid = torch.rand(B, P, device="cuda") < 0.5
        valid[:, 0] = True
        res = criteria.pck_auc(out, tgt, points=points, curve=True, valid=valid)
        assert torch.equal(res["n_valid"], valid.sum(1).int()) and bool((res["hits"][..., -1] <= res["n_valid"][None]).all())
        assert torch.equal(res["hits"], ops.pck_curve(pv, tv, tgt["scale"], _cu(thr), valid)[0])
        assert torch.equal(criteria.pck_auc(out, tgt, points=points, curve=True, valid=valid.to(torch.uint8))["hits"], res["hits"])
        # other thresholds
        res = criteria.pck_auc(out, tgt, points=points, vmin=2.0, vmax=30.0, steps=17, curve=True)
        t17 = np.linspace(2.0, 30.0, 17).astype(np.float32)
        assert np.array_equal(res["thresholds"].cpu().numpy(), t17) and torch.equal(res["hits"], ops.pck_curve(pv, tv, tgt["scale"], _cu(t17))[0])
        # aligned: the existing Procrustes kernel's output, evaluated, bit for bit; the caller's tensor is neither replaced nor written
        al = ops.procrustes_align(out[points].contiguous(), tgt[key].contiguous())
        h_a, auc_a, err_a = ops.pck_curve(al.view(N, B, P, 3), tv, tgt["scale"], _cu(thr))
        res = criteria.pck_auc(out, tgt, points=points, aligned=True, curve=True)
        assert torch.equal(res["auc"], auc_a) and torch.equal(res["err"], err_a) and torch.equal(res["hits"], h_a) and not torch.equal(auc_a, auc)
        assert out[points].data_ptr() == ptr and torch.equal(out[points], before)
        # best of the first n against numpy on the returned auc, index ties to the lower n
        ns = [1, 2, 3, 5, 6]
        res = criteria.pck_auc(out, tgt, points=points, ns=ns)
        assert set(res) == {"auc", "err", "thresholds", "auc_max", "auc_index"}
        assert res["auc_max"].shape == (5, B) and res["auc_index"].shape == (5, B) and res["auc_index"].dtype == torch.int64
        a = res["auc"].cpu().numpy()
        assert np.array_equal(a[2], a[0]) and np.array_equal(a[4], a[1])
        for i, n in enumerate(ns):
            assert np.array_equal(res["auc_max"][i].cpu().numpy(), a[:n].max(0))
            assert np.array_equal(res["auc_index"][i].cpu().numpy(), (a[:n] == a[:n].max(0)[None]).argmax(0))          # the lowest n attaining it
        idx = res["auc_index"].cpu().numpy()
        assert (idx != 2).all() and (idx != 4).all()          # a planted twin never wins over its original


def test_pck_select_cuts_every_tensor_consistently(gpu_lib):
    out, tgt = _sample_output()
    N, B = 6, 3
    cols = torch.arange(B, device="cuda")
    for points, aligned in (("xyz", False), ("verts", False), ("xyz", True)):
        auc = criteria.pck_auc(out, tgt, points=points, aligned=aligned)["auc"]
        val, order = torch.sort(auc.neg(), dim=0, stable=True)
        sel = criteria.pck_select(out, tgt, Q=2, points=points, aligned=aligned)
        assert set(sel) == set(out) | {"auc", "auc_index"}
        assert torch.equal(sel["auc"], val[:2].neg()) and torch.equal(sel["auc_index"], order[:2]) and sel["auc_index"].dtype == torch.int64
        assert bool((sel["auc"][0] >= sel["auc"][1]).all()) and torch.equal(sel["auc"][0], auc.max(0).values)
        for k in ("verts", "xyz", "log_q"):
            assert sel[k].shape[:2] == (2, B) and torch.equal(sel[k], out[k][order[:2], cols])
        assert sel["faces"] is out["faces"] and sel["image"] is out["image"]
    sel = criteria.pck_select(out, tgt, Q=N)
    pos = {int(n): i for i, n in enumerate(sel["auc_index"][:, 0].tolist())}
    assert pos[0] < pos[2] and pos[1] < pos[4], "ties go to the lower n"


# ---- the pool and the trainer shell -----------------------------------------------------------------------------------------------------------
def test_pool_over_three_batches_equals_the_concatenated_batch(gpu_lib):
    pool, cases = harness.PckPool(), []
    for k, B in enumerate((2, 5, 3)):
        case, ref = _case(2010 + k, 2, B, 21, 100, 0.7)
        cases.append(case)
        out = {"xyz": _cu(case["pred"]).view(2, B, 63)}
        tgt = {"pose3d": _cu(case["target"]).view(B, 63), "scale": _cu(case["scale"])}
        res = criteria.pck_auc(out, tgt, valid=_cu(case["valid"]), curve=True)
        pool.add(res["hits"], res["n_valid"], res["thresholds"])
    cat = lambda k, ax: np.concatenate([c[k] for c in cases], ax)
    ref = pck_ref.pck64(cat("pred", 1), cat("target", 0), cat("scale", 0), cases[0]["thr"], cat("valid", 0))
    assert ref["gap"] >= pck_ref.GAP
    thr, hits, n = pool.curve()
    assert hits.dtype == np.int64 and np.array_equal(hits, ref["hits"][0].sum(0)) and n == int(ref["n_valid"].sum())
    assert np.array_equal(thr, cases[0]["thr"])
    want = float(pck_ref.auc64(ref["hits"][0].sum(0), ref["n_valid"].sum(), thr))
    assert abs(pool.auc() - want) <= ULP2 * want


def test_run_pck_metrics(gpu_lib, tmp_path, capsys):
    import json
    from mhentropy_amd import run
    sc = tmp_path / "scalars.jsonl"
    log = run.main(["--backbone", "resnet18", "--batch", "4", "--hyps", "4", "--test-samples", "8", "--hidden", "64", "--flow-steps", "2", "--dtype",
                    "f32", "--epochs", "1", "--iters", "2", "--image-size", "96", "--pck-metrics", "--scalars", str(sc)])
    rows = [json.loads(line) for line in open(sc)]
    tags = {"metric_it/" + k for k in harness.PCK_SCALARS}
    assert len(log) == 1 and np.isfinite(log[0]["loss"])
    assert tags <= {r["tag"] for r in rows} and all(np.isfinite(r["value"]) for r in rows if r["tag"] in tags)
    assert sum(r["tag"] == "metric_it/auc_j" for r in rows) == 2
    for k in harness.PCK_SCALARS[:4]:
        assert 0.0 <= log[0][k] <= log[0][k + "_best"] <= 1.0
    pooled = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith('{"pck_pooled_auc"')]
    assert len(pooled) == 1 and set(pooled[0]["pck_pooled_auc"]) == set(harness.PCK_SCALARS[:4])
    assert all(0.0 <= v <= 1.0 for v in pooled[0]["pck_pooled_auc"].values())
    pool = run.main.last_pck_pool["auc_v"]
    assert pool.curve()[2] == 2 * 4 * 778          # two iterations of four images' meshes, hypothesis 0
