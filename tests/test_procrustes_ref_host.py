"""CPU: the Procrustes reference helper tests/procrustes_ref.py before any GPU run - its full-rank result against align_f64, the classes of the
constructed cases of tests/test_gpu_aligned_edges.py, the candidates of the deficient classes, and the derived bounds against the REFERENCE's
own f32 rows (tests/golden/criteria_aligned_*.npz) and a plain numpy restatement of the kernels' f32 arithmetic (procrustes_ref.kernel_f32) on
every GPU case.  Nothing here runs a kernel."""
import functools

import numpy as np
import pytest

import procrustes_ref as pr
from conftest import load_golden
from test_aligned_oracle import align_f64

DEG = pr.degenerate_cases()


def _gpu_cases():
    """every (name, target, pred) the GPU suite aligns against the reference"""
    for (N, P) in pr.SWEEP:
        yield f"sweep N={N} P={P}", lambda N=N, P=P: pr.sweep_case(N, P)
    for (N, P) in pr.FAR:
        yield f"far N={N} P={P}", lambda N=N, P=P: pr.sweep_case(N, P, far=True)
    for name in DEG:
        yield name, lambda name=name: DEG[name][:2]


GPU_CASES = dict(_gpu_cases())


def _ratio(got, ref, bound):
    diff = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(diff == 0, 0.0, diff / bound)


def test_candidates_equal_align_f64_on_random_full_rank_rows():
    rng = np.random.default_rng(3)
    for P in (4, 21, 70):
        tgt, pred = pr.sweep_case(6, P)
        al, R, s = align_f64(tgt, pred)
        S = pr.Solved(tgt, pred)
        assert (S.classes() == "full").all()
        assert np.abs(S.out_candidates()[0] - al).max() <= 1e-13 * np.abs(al).max()
        assert np.abs(S.R_candidates()[0] - R).max() <= 1e-13 and np.abs(S.sigma().sum(-1) - s).max() <= 1e-13
        n, b = int(rng.integers(6)), int(rng.integers(2))
        c = pr.candidates(tgt[b], pred[n, b])
        assert pr.classify(tgt[b], pred[n, b]) == "full" and len(c) == 1
        assert np.abs(c[0]["out"] - al[n, b]).max() <= 1e-13 * np.abs(al).max() and np.abs(c[0]["R"] - R[n, b]).max() <= 1e-13
        assert abs(c[0]["s"] - s[n, b]) <= 1e-13


@pytest.mark.parametrize("name", sorted(DEG))
def test_classify_puts_every_constructed_case_in_its_class(name):
    tgt, pred, cls, kind = DEG[name]
    S = pr.Solved(tgt, pred)
    assert (S.classes() == cls).all(), (name, S.classes())
    assert pr.classify(tgt[0], pred[0, 0]) == cls
    if name.startswith("nearly_planar"):
        rel = S.S[..., 2] / S.S[..., 0]
        assert (rel >= 1e-3).all() and (rel <= 1e-2).all(), rel
    if name.startswith("cube"):
        assert np.abs(S.S / S.S[..., :1] - 1.0).max() <= 1e-6          # repeated singular values
        assert (np.sign(np.linalg.det(S.M)) == (-1.0 if "mirror" in name else 1.0)).all()


def test_sweep_rows_with_few_points_are_deficient_by_construction():
    for (N, P), cls in (((1, 1), "rank0"), ((5, 2), "rank1"), ((3, 3), "rank2"), ((4, 4), "full")):
        assert (pr.Solved(*pr.sweep_case(N, P)).classes() == cls).all()


def test_classify_refuses_an_ill_posed_row():
    """a target 2e-8 of its extent thick (about the plane z = 0, so that f32 holds the thickness): sigma3 / sigma1 = 1e-9 to within a factor
    of 3, neither `full` nor exact"""
    rng = np.random.default_rng(9)
    tgt = (rng.normal(0, 0.03, (21, 3)) * np.array([1.0, 1.0, 2e-8])).astype(np.float32)
    pred = (tgt.astype(np.float64) @ pr.rot(rng).T * 30.0 + rng.normal(0, 0.2, (21, 3))).astype(np.float32)
    a, x = tgt.astype(np.float64), pred.astype(np.float64)
    sv = np.linalg.svd((a - a.mean(0)).T @ (x - x.mean(0)), compute_uv=False)
    assert 1e-9 / 3 < sv[2] / sv[0] < 3e-9, sv[2] / sv[0]
    with pytest.raises(ValueError, match="ill-posed"):
        pr.classify(tgt.reshape(-1), pred.reshape(-1))
    with pytest.raises(ValueError, match="ill-posed"):
        pr.out_bound(tgt.reshape(-1), pred.reshape(-1))


@pytest.mark.parametrize("name", sorted(k for k, v in DEG.items() if v[2] == "rank2"))
def test_rank2_candidates_are_orthogonal_and_agree_on_a_planar_hypothesis(name):
    tgt, pred, cls, kind = DEG[name]
    S = pr.Solved(tgt, pred)
    Rc, oc = S.R_candidates(), S.out_candidates()
    for R in Rc:
        assert np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max() <= 1e-14
    assert np.allclose(np.linalg.det(Rc[0]), -np.linalg.det(Rc[1]), atol=1e-14) and np.allclose(np.abs(np.linalg.det(Rc[0])), 1.0, atol=1e-14)
    assert np.abs(Rc[0] @ S.M.swapaxes(-1, -2) - Rc[1] @ S.M.swapaxes(-1, -2)).max() <= 1e-14          # both are polar factors of M
    gap = np.abs(oc[0] - oc[1]).max() / np.abs(oc).max()
    if kind == "planar_hyp":
        assert gap <= 1e-13, gap
        assert (S.hypothesis_rank() == 2).all()
    else:
        assert gap > 1e-3, gap                                          # a really ambiguous row: the min over the candidates matters
    c = pr.candidates(tgt[0], pred[0, 0])
    assert len(c) == 2 and np.array_equal(c[0]["out"], oc[0, 0, 0]) and np.array_equal(c[1]["R"], Rc[1, 0, 0])


@pytest.mark.parametrize("name", sorted(k for k, v in DEG.items() if v[2] == "rank1"))
def test_rank1_candidates(name):
    tgt, pred, cls, kind = DEG[name]
    S = pr.Solved(tgt, pred)
    c = pr.candidates(tgt[1], pred[2, 1])
    assert len(c) == 1 and abs(c[0]["s"] - S.S[2, 1, 0]) <= 1e-15
    assert np.abs(S.M[2, 1] @ c[0]["v1"] - c[0]["s"] * c[0]["u1"]).max() <= 1e-14
    assert (c[0]["out"] is not None) == (kind == "rank1_collinear_hyp")
    assert ((S.hypothesis_rank() == 1).all()) == (kind == "rank1_collinear_hyp")


def test_rank0_candidates():
    tgt, pred = pr.sweep_case(1, 1)
    c = pr.candidates(tgt[0], pred[0, 0])
    assert c[0]["s"] == 0.0 and np.array_equal(c[0]["out"], tgt[0].astype(np.float64))
    z = pr.candidates(np.zeros(63, np.float32), pr.sweep_case(17, 21)[1][0, 0])
    assert z[0]["s"] == 0.0 and not z[0]["out"].any()


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_bounds_are_finite_and_the_f32_restatement_stays_inside(name):
    """out_bound is finite and positive on every GPU case, and the numpy restatement of the kernels' f32 arithmetic - which the bound was
    derived for, not fitted to - stays inside it: out (every row within the bound of one candidate), R (full rows) and s"""
    tgt, pred = GPU_CASES[name]()
    S = pr.Solved(tgt, pred)
    b = S.bounds()
    assert np.isfinite(b["out"]).all() and (b["out"] > 0).all() and np.isfinite(b["R"]).all() and np.isfinite(b["s"]).all()
    assert (b["out"] <= 1e-4 * np.abs(S.out_candidates()).max()).all()          # a bound that admits 1e-4 would check nothing
    out, R, s = pr.kernel_f32(tgt, pred)
    kind = DEG[name][3] if name in DEG else None
    if kind != "rank1":
        sel, _ = pr.select(out.astype(np.float64), S.out_candidates(), b["out"])
        assert _ratio(out, sel, b["out"]).max() <= 1.0, name
    assert _ratio(s, S.sigma().sum(-1), b["s"]).max() <= 1.0
    R64 = R.astype(np.float64)
    assert np.abs(np.swapaxes(R64, -1, -2) @ R64 - np.eye(3)).max() <= b["R"].min()
    if (S.rank >= 2).all():
        Rsel, _ = pr.select(R64.reshape(S.N, S.B, 9), S.R_candidates().reshape(2, S.N, S.B, 9), b["R"][..., None])
        assert _ratio(R64.reshape(S.N, S.B, 9), Rsel, b["R"][..., None]).max() <= 1.0
    if (S.rank == 1).all():
        v1, u1 = S.Vt[..., 0, :], S.U[..., :, 0]
        assert _ratio((R64 @ v1[..., None])[..., 0], u1, b["R"][..., None]).max() <= 1.0


@pytest.mark.parametrize("name", sorted(k for k in DEG if k.startswith(("planar_", "collinear_"))))
def test_the_deficiency_survives_the_kernels_own_centring(name):
    """the constructed deficient cases are exact in f32: the f32 mean of the kernels' summation order is the f64 mean, bit for bit, and a
    constant coordinate centres to exactly 0"""
    tgt, pred, cls, kind = DEG[name]
    N, B = pred.shape[:2]
    C = pred.reshape(N, B, -1, 3)
    P = C.shape[2]
    t2 = (pr._lane_sum(lambda p: C[:, :, p], P) / np.float32(P)).astype(np.float32)
    assert np.array_equal(t2.astype(np.float64), C.astype(np.float64).mean(2))
    x = C - t2[:, :, None]
    assert np.array_equal(x.astype(np.float64), C.astype(np.float64) - C.astype(np.float64).mean(2, keepdims=True))
    A = tgt.reshape(B, -1, 3).astype(np.float64)
    t1 = A.mean(1).astype(np.float32)
    assert np.array_equal(t1.astype(np.float64), A.mean(1))
    if "planar_target" in name or "planar_both" in name:
        assert not (tgt.reshape(B, -1, 3)[..., 2] - t1[:, None, 2]).any()
    if "planar_hypothesis" in name or "planar_both" in name:
        assert not x[..., 1].any()


@functools.lru_cache(None)
def _golden(tag):
    return load_golden(f"criteria_aligned_{tag}"), load_golden(f"mhent_{tag}")


@pytest.mark.parametrize("tag", ["small", "shipped"])
@pytest.mark.parametrize("case", ["base", "mirror"])
def test_reference_f32_rows_stay_inside_the_bounds_at_their_own_serial_depth(tag, case):
    """NOT the bound the GPU suite holds wave_kernel to (P > 32): the same derivation at the reference's own summation depth.
    The reference's own f32 evaluation (numpy, LAPACK sgesdd) of its fixtures against the same derivation.  Its means and products are
    numpy reductions over the point axis of a (P, 3) array - a serial chain of P additions - so the derivation is evaluated with d = P for
    it (depth_of); every other term is unchanged.  With the wave kernel's own d = ceil(P / 64) + 6 the reference's 778-point rows reach 2.2
    times the bound (its serial f32 mean loses more than the kernel's lane chains and butterfly), the 21-point rows (d = P either way) 0.05.
    Every row is `full`."""
    g, d = _golden(tag)
    worst = {}
    for lbl, src in (("xyz", "sample_xyz"), ("verts", "sample_verts")):
        tgt = g[f"{case}_pose3d"] if lbl == "xyz" else g[f"{case}_verts"]
        S = pr.Solved(tgt, d[src], depth_of=lambda P: P)
        assert (S.classes() == "full").all()
        b = S.bounds()
        worst[lbl] = (_ratio(g[f"{case}_{lbl}_aligned"], S.out_candidates()[0], b["out"]).max(),
                      _ratio(g[f"{case}_R_{lbl}"], S.R_candidates()[0], b["R"][..., None, None]).max(),
                      _ratio(g[f"{case}_s_{lbl}"], S.sigma().sum(-1), b["s"]).max())
    print(f"reference f32 rows {tag} {case}: max |diff| / bound (out, R, s) = {worst}")
    for lbl, w in worst.items():
        assert max(w) <= 1.0, (lbl, w)
