"""GPU: the aligned evaluation's kernels at their edges - csrc/procrustes.hip (target_kernel, rows_kernel, wave_kernel, polar3) against the
float64 reference tests/procrustes_ref.py, which is defined on degenerate rows, and the split form of csrc/metrics.hip against the float64
criterion oracle.  Bounds: derived in procrustes_ref's docstring from the kernels' arithmetic with u = 2^-24 (accumulation depth, centring,
polar sensitivity sqrt2 |dM|_F / (sigma2 + sigma3), final fma); tests/test_procrustes_ref_host.py checks them on the CPU against the
reference's own f32 rows and a numpy restatement.  Every comparison prints max(|diff| / bound) before it asserts (`pytest -s`).

Paths (csrc/procrustes.hip: PSMALL = 32, CH = 256 hypotheses per rows_kernel workgroup, WAVES x HPW = 4 x 4 hypotheses per wave_kernel
workgroup, PMAX = 1024; `vec` = float2 loads and stores, taken when P*3 is even and pred and out are 8-byte aligned).  The (N, P) pairs of
the sweep, pruned from P in {1,2,3,4,21,31,32,33,49,63,64,65,777,778,1023,1024} x N to the pairs that select a distinct path:

  (N, P)      kernel  chunk / workgroup                          vec    what else
  (1, 1)      rows    chunk 0, cn = 1                            -      rank0: M = 0, out = t1
  (5, 2)      rows    chunk 0 ragged                             -      rank1 in the inputs; u2 from a noise-sized remainder
  (3, 3)      rows    chunk 0 ragged                             -      rank2 in the inputs; u3 from a noise-sized remainder
  (4, 4)      rows    chunk 0 ragged                             -      the smallest P of full rank
  (16, 4)     rows    chunk 0 ragged                             -
  (17, 21)    rows    chunk 0 ragged                             -      the joints' P, odd row stride 63
  (255, 21)   rows    chunk 0 ragged, one short of CH            -
  (256, 21)   rows    chunk 0, cn == CH                          -
  (257, 21)   rows    chunk 1 (n0 = 256), ragged cn = 1          -
  (513, 21)   rows    chunks 0, 1 full, chunk 2 ragged           -
  (3, 31)     rows    chunk 0 ragged                             -      P = PSMALL - 1
  (257, 31)   rows    chunk 1                                    -      odd row stride 93
  (1, 32)     rows    chunk 0, cn = 1                            -      P = PSMALL
  (256, 32)   rows    chunk 0, cn == CH                          -      P = PSMALL: the whole 98 704-byte LDS request is written
  (257, 32)   rows    chunk 1                                    -      P = PSMALL
  (513, 32)   rows    three chunks                               -      P = PSMALL
  (1, 33)     wave    workgroup 0, break at h = 1 of wave 0      false  the smallest wave row: 31 lanes hold no point
  (3, 33)     wave    break at h = 3 inside wave 0 (N < HPW)     false
  (17, 33)    wave    N = 16 k + 1: workgroup 1 holds one row    false
  (5, 49)     wave    wave 1 breaks at h = 1                     false
  (16, 63)    wave    one full workgroup, no break               false  one point short of a full wave
  (1, 64)     wave    break at h = 1                             true   one point per lane
  (17, 64)    wave    second workgroup                           true
  (5, 65)     wave    wave 1 breaks at h = 1                     false  lane 0 takes a second point
  (33, 65)    wave    three workgroups                           false
  (3, 777)    wave    break at h = 3                             false
  (17, 777)   wave    second workgroup                           false
  (5, 778)    wave    wave 1 breaks                              true   the mesh
  (16, 778)   wave    one full workgroup                         true
  (1, 1023)   wave    break at h = 1                             false  P = PMAX - 1
  (3, 1023)   wave    break at h = 3                             false
  (1, 1024)   wave    break at h = 1                             true   P = PMAX: the LDS slices at their sized maximum
  (33, 1024)  wave    three workgroups                           true   P = PMAX
  far family (hypotheses 100 extents from the origin; the centring term sqrt3 f k dominates the bound): (257, 21), (17, 32), (5, 65),
  (3, 778), (1, 1024)
  vec false at an EVEN P (pred at a 4-byte offset): test_scalar_path_reproduces_the_vector_path, P = 778 and 64
  metrics.hip, SPLIT: N = 1 (spread := 0), 2, 255 (one ragged chunk), 256 (N == CH: pass 2 reuses the rows pass 1 left in LDS - those of
  coord_sp), 257 and 513 (N > CH: pass 2 reloads coord_sp chunk by chunk)

Measured on an MI355X, the largest |diff| / bound of every test of this file:
  sweep            rows_kernel 0.338 (N=5 P=2, out; full-rank rows 0.326 at N=16 P=4)   wave_kernel 0.353 (N=5 P=49, out)
  far family       rows_kernel 0.092 (N=257 P=21)   wave_kernel 0.138 (N=5 P=65)
  rank2            0.232 (three_points, out)        rank1 0.376 (two_points, out)
  cube, mirrored   0.093 (s); the aligned copy returns to the target within 3.0e-8 m (bound 1e-6)
  nearly planar    0.204 (P=21), 0.161 (P=778)
  split metrics    2.2e-7 of max|ref| over the 14 rows and the six N (bound 1e-4);   pa_mpjpe 1.1e-8 of the extent (bound 1e-5 + 1e-4 max)
No bound was widened and no kernel changed.  The numpy restatement procrustes_ref.kernel_f32 gives the same ratios on the CPU.
One defect surfaced outside these kernels: with this module's allocations earlier in the process, test_gpu_chamfer_train.py's
test_graphed_step_replays_bit_equal_to_eager failed.  train.GraphedStep kept no reference to its static inputs and that test passes a
temporary x.clone(): the graphs read a freed block, which a later allocation (torch.equal's temporaries between two replays) could take.
GraphedStep now keeps (x, y, noise) alive.
Sensitivity (one arithmetic-only change each in a scratch build, each run once through this file and the earlier suites of the same kernels,
test_gpu_aligned.py, test_gpu_body_eval.py and the metrics tests of test_gpu_kernels.py, which all still passed):
  wave_kernel's scalar load stops one element short      17 tests of this file fail (sweep at every odd P > 32, far, row independence,
                                                         scalar against vector path, pa_mpjpe P = 33 and 63)
  polar3's eigenvalue sort without its third comparison  test_rank1_rows_give_what_is_determined[collinear_target_P21 / _P40] fail
  pass 2 of the split metrics reads coord                test_split_metrics_match_the_oracle_on_two_arrays[257] and [513] fail
"""
import numpy as np
import pytest
import torch

import procrustes_ref as pr
from conftest import assert_close
from edge_measure import Measure
from test_aligned_oracle import align_f64
from test_gpu_body_eval import RTOL as RTOL_BODY, _similar
from test_gpu_kernels import RTOL as RTOL_METRICS

pytestmark = pytest.mark.gpu
DEG = pr.degenerate_cases()


def M(kernel):
    return Measure(kernel, suite="aligned-edges")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _align(tgt, pred):
    from mhentropy_amd import ops
    out, R, s = ops.procrustes_align(_dev(pred), _dev(tgt), want_transform=True)
    return out.cpu().numpy(), R.cpu().numpy(), s.cpu().numpy()


def _compare(m, case, tgt, pred, kind=None):
    """one call against the reference: out (every row against the candidate nearest to it in units of the bound - one candidate for `full`),
    s, R (full and rank2 rows: against the nearest candidate; rank1 rows: R v1 = u1), R orthogonal and everything finite"""
    S = pr.Solved(tgt, pred)
    b = S.bounds()
    out, R, s = _align(tgt, pred)
    assert np.isfinite(out).all() and np.isfinite(R).all() and np.isfinite(s).all(), case
    if kind != "rank1":                                                      # (a collinear target leaves the row of a general hypothesis open)
        sel, _ = pr.select(out.astype(np.float64), S.out_candidates(), b["out"])
        m.add(case + " out", out, sel, b["out"])
    m.add(case + " s", s, S.sigma().sum(-1), b["s"])
    R64 = R.astype(np.float64)
    if (S.rank >= 1).all():
        m.add(case + " R^T R", np.swapaxes(R64, -1, -2) @ R64, np.broadcast_to(np.eye(3), R64.shape), b["R"][..., None, None])
    if (S.rank >= 2).all():
        Rsel, _ = pr.select(R64.reshape(S.N, S.B, 9), S.R_candidates().reshape(2, S.N, S.B, 9), b["R"][..., None])
        m.add(case + " R", R64.reshape(S.N, S.B, 9), Rsel, b["R"][..., None])
    elif (S.rank == 1).all():
        m.add(case + " R v1", (R64 @ S.Vt[..., 0, :, None])[..., 0], S.U[..., :, 0], b["R"][..., None])
    return S, out, R, s


# ---- 1. the shape sweep -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", sorted(pr.SWEEP), ids=lambda v: str(v))
def test_sweep_matches_f64(gpu_lib, N, P):
    m = M("rows_kernel" if P <= pr.PSMALL else "wave_kernel")
    tgt, pred = pr.sweep_case(N, P)
    S, out, R, s = _compare(m, f"N={N} P={P} ({pr.SWEEP[(N, P)]})", tgt, pred)
    if P >= 4:                                                              # the unique result is align_f64's
        al, R64, s64 = align_f64(tgt, pred)
        b = S.bounds()
        m.add(f"N={N} P={P} out vs align_f64", out, al, b["out"])
        m.add(f"N={N} P={P} R vs align_f64", R, R64, b["R"][..., None, None])
    if P == 1:
        assert not s.any() and np.array_equal(out, np.broadcast_to(tgt[None], out.shape))          # exactly t1, the one target point
    m.report()


@pytest.mark.parametrize("N,P", sorted(pr.FAR), ids=lambda v: str(v))
def test_sweep_far_from_the_origin_matches_f64(gpu_lib, N, P):
    """hypotheses 100 extents from the origin: the f32 mean and the subtraction c - t2 lose the most; the centring term carries the bound"""
    m = M("rows_kernel (far)" if P <= pr.PSMALL else "wave_kernel (far)")
    tgt, pred = pr.sweep_case(N, P, far=True)
    S, out, R, s = _compare(m, f"far N={N} P={P}", tgt, pred)
    b, k = S.bounds()["out"], S.k()[:, :, 0, 0]
    centring = (pr.SQ3 * (pr.depth(P) + 1) * pr.U32 * S.cmax * k)[..., None]
    assert (centring >= 0.5 * b).mean() > 0.5, "the case does not make the centring term dominate"
    m.report()


# ---- 2. row independence, 3. scalar against vector path: bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,rows", [(257, 21, (5, 255, 256)), (257, 32, (5, 255, 256)), (33, 65, (2, 16, 32))], ids=lambda v: str(v))
def test_a_row_does_not_depend_on_its_position(gpu_lib, N, P, rows):
    """row (n, b) of the N-hypothesis call equals the one-hypothesis call on that row, bit for bit: n from the first chunk (workgroup), the
    second chunk's first row and the last row (N = 257: rows 256 is both; 255 is the first chunk's last)"""
    from mhentropy_amd import ops
    tgt, pred = pr.sweep_case(N, P)
    dp, dt = _dev(pred), _dev(tgt)
    out, R, s = ops.procrustes_align(dp, dt, want_transform=True)
    for n in rows:
        o1, R1, s1 = ops.procrustes_align(dp[n:n + 1].contiguous(), dt, want_transform=True)
        assert torch.equal(o1[0], out[n]) and torch.equal(R1[0], R[n]) and torch.equal(s1[0], s[n]), (N, P, n)


@pytest.mark.parametrize("P", [778, 64])
def test_scalar_path_reproduces_the_vector_path(gpu_lib, P):
    """pred viewed at a 4-byte offset into a larger buffer: contiguous, not 8-byte aligned -> wave_kernel's scalar loads and stores.  The
    arithmetic is the same: the bits of the aligned call"""
    from mhentropy_amd import ops
    N = 5
    tgt, pred = pr.sweep_case(N, P)
    dp, dt = _dev(pred), _dev(tgt)
    big = torch.full((dp.numel() + 3,), float("nan"), device="cuda")
    view = big[1:1 + dp.numel()].view(dp.shape)
    view.copy_(dp)
    assert view.is_contiguous() and dp.data_ptr() % 8 == 0 and view.data_ptr() % 8 == 4
    a = ops.procrustes_align(dp, dt, want_transform=True)
    b = ops.procrustes_align(view, dt, want_transform=True)
    for x, y in zip(a, b):
        assert torch.isfinite(y).all() and torch.equal(x, y)


# ---- 4. constructed degenerate rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(k for k, v in DEG.items() if v[2] == "rank2"))
def test_rank2_rows_land_on_a_candidate(gpu_lib, name):
    """planar target, planar hypothesis, both, P = 3: every row within the bound of one of R+-'s results, R orthogonal within the R bound"""
    tgt, pred, cls, kind = DEG[name]
    m = M("polar3 rank2")
    S, out, R, s = _compare(m, name, tgt, pred, kind)
    assert (S.classes() == "rank2").all()
    # d det = det tr(R^T dR), |tr| <= 3 |dR|_2: |det R| = 1 within 3 R_bound, either sign
    m.add(name + " |det R|", np.abs(np.linalg.det(R.astype(np.float64))), np.ones(s.shape), 3 * S.bounds()["R"])
    m.report()


@pytest.mark.parametrize("name", sorted(k for k, v in DEG.items() if v[2] == "rank1"))
def test_rank1_rows_give_what_is_determined(gpu_lib, name):
    """collinear target: s and R v1 = u1, R orthogonal and finite; collinear hypothesis and P = 2: the full aligned row as well"""
    tgt, pred, cls, kind = DEG[name]
    m = M("polar3 rank1")
    S, out, R, s = _compare(m, name, tgt, pred, kind)
    assert (S.classes() == "rank1").all()
    m.report()


@pytest.mark.parametrize("name", ["cube", "cube_mirror", "nearly_planar_P21", "nearly_planar_P778"])
def test_repeated_singular_values_and_flat_hands_are_unique(gpu_lib, name):
    """the cube's corners against rotated (hypothesis 0: a quarter turn, exact in f32), scaled, shifted copies, and the same mirrored: M is
    a multiple of an orthogonal matrix, the Jacobi loop meets repeated eigenvalues, R is unique all the same and the copy returns to the
    target; a flat open hand (sigma3 / sigma1 of a few 1e-3): the plain comparison, its bound moderate because sigma2 is large"""
    tgt, pred, cls, kind = DEG[name]
    m = M("polar3 " + name)
    S, out, R, s = _compare(m, name, tgt, pred, kind)
    assert (S.classes() == "full").all()
    al, R64, s64 = align_f64(tgt, pred)
    m.add(name + " out vs align_f64", out, al, S.bounds()["out"])
    if name.startswith("cube"):
        det = np.linalg.det(R.astype(np.float64))
        m.add(name + " det R", det, np.full(det.shape, -1.0 if "mirror" in name else 1.0), 3 * S.bounds()["R"])          # (the mirror's sign is kept)
        err = np.abs(out - tgt[None]).max()
        print(f"aligned-edges: {name}: the aligned copy returns to the target within {err:.2e} m")
        assert err < 1e-6                                                    # metres, on a 0.6 m offset (test_rigid_mirrored_and_zero_targets)
    m.report()


# ---- 5. split metrics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 513])
def test_split_metrics_match_the_oracle_on_two_arrays(gpu_lib, N):
    """mhe_metrics_split_f32 on two DIFFERENT arrays against the criterion oracle composed as aligned_metrics_oracle composes it (error rows of
    xyz_err, 3D *_std rows of xyz_spread), image 0 fully visible and image 1 fully invisible; each row reads its own array: the rows equal
    those of the one-array kernel on that array bit for bit, and swapping the arrays changes both kinds of row"""
    from mhentropy_amd import ops, criteria
    from oracle import criteria_ref
    B = 3
    rng = np.random.default_rng(4000 + N)
    y = {"pose3d": rng.normal(0, 1, (B, 63)).astype(np.float32), "scale": rng.uniform(0.5, 1.5, B).astype(np.float32),
         "crop_uv": rng.uniform(-1, 1, (B, 42)).astype(np.float32), "vis": (rng.random((B, 21)) < 0.7).astype(np.float32)}
    y["vis"][0], y["vis"][1] = 1.0, 0.0
    xe = (y["pose3d"][None] + rng.normal(0, 0.3, (N, B, 63))).astype(np.float32)
    xs = (y["pose3d"][None] * 0.5 + rng.normal(0.2, 0.6, (N, B, 63))).astype(np.float32)
    uv = ((y["crop_uv"][None] + 1) * 128 + rng.normal(0, 9, (N, B, 42))).astype(np.float32)
    dy = {k: _dev(v) for k, v in y.items()}
    args = (_dev(uv), dy["pose3d"], dy["scale"], dy["crop_uv"], dy["vis"])
    de, ds = _dev(xe), _dev(xs)
    out = ops.metrics_split(de, ds, *args)
    ty = {k: torch.as_tensor(v) for k, v in y.items()}
    base = {"log_p": torch.zeros(B), "uv": torch.as_tensor(uv)}
    _, _, m_err = criteria_ref.mhent_loss(dict(base, xyz=torch.as_tensor(xe)), ty)
    _, _, m_spr = criteria_ref.mhent_loss(dict(base, xyz=torch.as_tensor(xs)), ty)
    spread = lambda k: k.startswith("eucLoss_3d") and k.endswith("_std")          # noqa: E731
    worst = 0.0
    for i, k in enumerate(criteria.METRIC_KEYS):
        ref = (m_spr if spread(k) else m_err)[k].double().numpy()
        worst = max(worst, float(np.abs(out[i].cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-30)))
    print(f"aligned-edges: metrics_kernel<split> N={N}: max |diff| / max|ref| over the 14 rows = {worst:.2e} (bound {RTOL_METRICS:g})")
    for i, k in enumerate(criteria.METRIC_KEYS):
        assert_close(out[i].cpu(), (m_spr if spread(k) else m_err)[k], RTOL_METRICS, what=f"{k} (N={N})")
    one_e, one_s, swapped = ops.metrics(de, *args), ops.metrics(ds, *args), ops.metrics_split(ds, de, *args)
    for i, k in enumerate(criteria.METRIC_KEYS):
        assert torch.equal(out[i], (one_s if spread(k) else one_e)[i]), k
        if k.startswith("eucLoss_3d") and (N > 1 or not spread(k)):          # (N = 1: the spread is 0 whatever the array)
            assert not torch.equal(out[i], swapped[i]), k
        if k.startswith("eucLoss_2d"):
            assert torch.equal(out[i], swapped[i]), k
    if N == 1:
        assert all(not out[i].any() for i, k in enumerate(criteria.METRIC_KEYS) if k.endswith("_std"))


# ---- 6. PA-MPJPE ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [32, 33, 63])
def test_pa_mpjpe_at_the_kernel_boundary_matches_f64(gpu_lib, P):
    """body.point_errors across rows_kernel's last P and wave_kernel's first: float64 align_f64, then the mean point distance; the bound of
    test_point_errors_match_f64"""
    from mhentropy_amd import body
    B, K = 3, 5
    rng = np.random.default_rng(900 + P)
    tgt = rng.normal(0, 0.3, (B, P, 3)).astype(np.float32)
    ext = float(np.abs(tgt).max())
    pts = _similar(rng, tgt.astype(np.float64), K, 0.01 * ext).astype(np.float32)
    al = align_f64(tgt.reshape(B, -1), np.ascontiguousarray(pts.transpose(1, 0, 2, 3)).reshape(K, B, -1))[0].reshape(K, B, P, 3)
    pa_ref = np.linalg.norm(al - tgt.astype(np.float64)[None], axis=-1).mean(-1).T
    pa = body.point_errors(_dev(pts), _dev(tgt))["pa_mpjpe"].cpu().numpy()
    assert pa.shape == (B, K)
    print(f"aligned-edges: point_errors P={P}: pa_mpjpe max|diff| / extent {np.abs(pa - pa_ref).max() / ext:.2e} (bound 1e-5 + {RTOL_BODY:g} max)")
    assert_close(pa, pa_ref, RTOL_BODY, 1e-5 * ext, what=f"pa_mpjpe P={P}")
