"""The forward pass's small kernels between the convolutions and around the loss, each against a float64 reference at the edges it has: the
BatchNorm apply (csrc/conv.hip: bn_act_kernel), the two max pools, the average pool and its fused form, the NCHW -> NHWC conversions, the
BatchNorm finalize over fx::wave_totals (csrc/common.h), the two serial row sums, the ELBO reduction, the stochastic head, the apply form of
the dropout and the top-Q selection (csrc/metrics.hip).  Shapes: channel counts that are no multiple of a workgroup's share, pixel counts
below one pixel group, and one case per grid-stride loop that is larger than the capped grid, so that the second trip of the loop runs.

Operands are rounded to the storage type on the CPU; every expected value is float64 on the CPU from those rounded operands.

Bounds (u32 = 2^-24, ub = 2^-8; none of them is tuned, the measured max(|diff| / bound) is printed before it is asserted, `pytest -s`):
  bn_act            |got - ref| <= 4 u32 (|x s| + |t| + |r rs| + |rt|) per element: one fma per affine, one add, each rounding at most u32 of
                    a partial result that the sum of the magnitudes bounds; bf16 storage adds the final rounding, ub |ref|
  max pool          no affine: bit-equal to F.max_pool2d over the stored values (max is exact).  With the affine:
                    2 u32 max_taps(|x s| + |t|) around relu(max_taps(x s + t)) (one fma per tap; max and relu are 1-Lipschitz); bf16 + ub |ref|
  average pool      (HW / 4 + 4) u32 mean_p |x| per (b, c): four serial sums of at most HW / 4 + 1 terms, three adds, one division
  bn_act_avgpool    bit-equal to avgpool(bn_act(...)); against the f64 mean of the f64 bn_act: the mean over the pixels of the bn_act bound
                    plus the average pool's bound on the mean of |ref|.  bf16 a second time against the mean of the f64 values ROUNDED to bf16,
                    which is what the kernel sums: there the element bound is 4 u32 (...) + 2 ub |ref|, not + ub |ref| - the kernel rounds its
                    f32 value v, the reference rounds ref, and |rnd(v) - rnd(ref)| <= ub |v| + |v - ref| + ub |ref|: where the f32 error
                    carries v across a bf16 tie that ref stays short of, the two roundings part by a whole bf16 step (2 ub |ref| at the bottom of
                    a binade), and at HW = 1 no average dilutes it
  nchw_to_nhwc      f32 bit-equal; bf16 bit-equal to x.to(torch.bfloat16) (NaN stays NaN, whichever NaN); padding channels are +0
  bn_finalize       from the integer words decoded on the CPU (as ops.stat_totals does, in exact integer arithmetic): scale and 1 / std within
                    4 u32 relative (var rounded to f32, + eps, sqrt, division), shift within 4 u32 (|beta| + |mean scale|), the mean within u32
                    relative (one rounding of the f64 quotient), the running buffers within 4 u32 (|old| + |batch statistic|)
  row sums          N u32 sum_n |x_n| (a serial sum of N terms has N - 1 roundings of partial sums that sum_n |x_n| bounds); with
                    `accumulate` the old value is one more term: N u32 (|old| + sum_n |x_n|)
  elbo_reduce       (N / 64 + 8) u32 (sum_n |lp_n| + sum_n |lq_n|) / N for each output: at most N / 64 + 1 serial terms per lane, six butterfly
                    steps, one division, one final add
  reparam           sd within 4 u32 relative of exp(l2 / 2) | sigmoid(l2); z within 4 u32 (|mn| + |sd eps|); deterministic: z == mn to the bit
  dropout_ (apply)  u32 |ref| (one product with the f32 keep scale), bf16 ub |ref|; dropped elements are +0 to the bit
  topk_gather       exact, in the order of a stable descending sort with NaN above every number
"""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import assert_close
from edge_measure import Measure as _Measure

BF, F32 = torch.bfloat16, torch.float32
U32, UB = 2.0 ** -24, 2.0 ** -8
DTYPES = pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
FORMS = ["no-residual", "residual", "residual-affine"]
EW_CAP = 4096 * 256          # vectors one launch of the element-wise grids covers in its first trip (ew_blocks of csrc/conv.hip)


def _dtn(dt):
    return "bfloat16" if dt == BF else "float32"


def _np(t):
    return t.detach().cpu().double().numpy()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ---- references (float64, CPU) -----------------------------------------------------------------------------------------------------------
def bn_act_reference(x, s, t, r, rs, rt, relu):
    """(y, magnitude) in f64: y = relu?(x s + t + (r rs + rt | r)), magnitude = |x s| + |t| + |r rs| + |rt|; x / r [..., C], tables [C]"""
    x, s, t = x.double(), s.double(), t.double()
    y, mag = x * s + t, (x * s).abs() + t.abs()
    if r is not None:
        r = r.double()
        if rs is not None:
            y, mag = y + r * rs.double() + rt.double(), mag + (r * rs.double()).abs() + rt.double().abs()
        else:
            y, mag = y + r, mag + r.abs()
    return (y.clamp_min(0.0) if relu else y), mag


def maxpool_reference(x, s=None, t=None):
    """3x3 stride-2 pad-1 max pool of NHWC x in its own float type (exact) - or, with the affine, (relu(max_taps(x s + t)), max_taps(|x s| + |t|))
    in f64"""
    import torch.nn.functional as F
    pool = lambda v: F.max_pool2d(v.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    if s is None:
        return pool(x)
    x, s, t = x.double(), s.double(), t.double()
    return pool(x * s + t).clamp_min(0.0), pool((x * s).abs() + t.abs())


def topk_reference(score, Q):
    """idx [Q, B] of score [N, B]: a stable descending sort, NaN above every number (torch.topk's order with the ties settled by index)"""
    score = np.asarray(score)
    nan = np.isnan(score)
    clean = np.where(nan, 0.0, score)
    out = []
    for b in range(score.shape[1]):
        order = np.argsort(-clean[:, b], kind="stable")                        # -0.0 and +0.0 compare equal: the index decides
        order = order[np.argsort(~nan[order, b], kind="stable")]               # NaN rows first, in index order
        out.append(order[:Q])
    return np.stack(out, 1).astype(np.int32)


def rank_rule(score):
    """the rank the kernel gives row n of one image (csrc/metrics.hip, topk_gather_kernel), restated: the number of rows m that precede n, where m
    precedes n if it is NaN and n is not, or neither is NaN and score[m] > score[n], or they are level (both NaN, or equal) and m < n"""
    v = np.asarray(score)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        gt, eq = v[:, None] > v[None, :], v[:, None] == v[None, :]             # [m, n]
    above = np.where(nan[:, None], ~nan[None, :], gt)
    level = np.where(nan[:, None], nan[None, :], eq)
    idx = np.arange(len(v))
    return (above | (level & (idx[:, None] < idx[None, :]))).sum(0)


def decode_totals(words):
    """[2, C] float64 totals of a unit of statistic words [2, S, 2, C] (int64, CPU): sum over the shards as exact integers, then
    plane 0 * 2^-16 + plane 1 * 2^-56 rounded once"""
    w = np.array(words.tolist(), dtype=object).sum(axis=1)          # Python integers: no wrap at any shard size
    return np.array([[float(Fraction(int(h) * 2 ** 40 + int(l), 2 ** 56)) for h, l in zip(w[0][k], w[1][k])] for k in range(2)])


# ---- 0. the references and the rank rule (no GPU) ----------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
ADVERSARIAL = [
    [NAN], [NAN, NAN, NAN, NAN, NAN], [1.0, NAN, 1.0, NAN, 0.5], [NAN, 3.0, 3.0, 3.0], [INF, NAN, -INF, INF, NAN, -INF],
    [0.0, -0.0, 0.0, -0.0], [-0.0, NAN, 0.0, INF, -INF, NAN, 0.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0], [5.0], [1.0, 2.0, 3.0, 4.0], [4.0, 3.0, 2.0, 1.0],
]


def _adversarial_rows():
    g = np.random.default_rng(5)
    rows = [np.array(r, np.float32) for r in ADVERSARIAL]
    for N in (64, 65, 200):
        v = g.integers(0, 4, N).astype(np.float32)           # four levels: heavy ties
        v[g.random(N) < 0.3] = NAN
        v[g.random(N) < 0.1] = INF
        v[g.random(N) < 0.1] = -INF
        rows.append(v)
        rows.append(np.full(N, NAN, np.float32))
    return rows


def test_rank_rule_is_a_permutation_and_the_reference_sort_agrees():
    """over all-NaN, some-NaN, tied, +-inf and +-0 rows: the ranks of an image are a permutation of 0 .. N-1 (so every slot r < Q is written exactly
    once), and the numpy reference sort puts row n at position rank[n]"""
    for v in _adversarial_rows():
        rank = rank_rule(v)
        assert sorted(rank.tolist()) == list(range(len(v))), (v, rank)
        order = topk_reference(v[:, None], len(v))[:, 0]
        assert np.array_equal(rank[order], np.arange(len(v))), (v, rank, order)
        # NaN above every number, then descending
        k = int(np.isnan(v).sum())
        assert np.isnan(v[order[:k]]).all() and not np.isnan(v[order[k:]]).any()
        assert (v[order[k + 1:]] <= v[order[k:-1]]).all()


def test_reference_sort_agrees_with_torch_topk_where_torch_defines_the_order():
    """distinct finite scores and NaN: torch.topk (NaN is the largest value) gives the same values in the same order"""
    g = torch.Generator().manual_seed(3)
    s = torch.randn(200, 4, generator=g)
    s[::7, 1] = NAN
    s[:, 3] = NAN
    ref = topk_reference(s.numpy(), 50)
    vals = torch.topk(s, 50, dim=0).values.numpy()
    mine = np.take_along_axis(s.numpy(), ref.astype(np.int64), 0)
    assert np.array_equal(np.isnan(vals), np.isnan(mine)) and np.array_equal(np.nan_to_num(vals), np.nan_to_num(mine))


def test_bn_act_and_pool_references_agree_with_torch_functional():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(9)
    x, r = torch.randn(2, 5, 6, 12, generator=g), torch.randn(2, 5, 6, 12, generator=g)
    s, t, rs, rt = (torch.randn(12, generator=g) for _ in range(4))
    y, mag = bn_act_reference(x, s, t, r, rs, rt, True)
    want = F.relu(x.double() * s.double() + t.double() + r.double() * rs.double() + rt.double())
    assert_close(y.numpy(), want.numpy(), 1e-15, what="bn_act reference")
    assert (mag * (1 + 1e-15) >= y.abs()).all()
    m, _ = maxpool_reference(x, s, t)
    want = F.max_pool2d(F.relu(x.double() * s.double() + t.double()).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(m, want.contiguous())          # relu commutes with max
    assert torch.equal(maxpool_reference(x), F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous())


def test_decode_totals_agrees_with_the_float_encoding():
    """stat_from_float's encoding, restated here so that the test needs no library: the decoded totals are the f64 sums of the shard values, and
    shards near 2^40 do not wrap the integer sum"""
    g = torch.Generator().manual_seed(2)
    t = torch.randn(64, 2, 5, generator=g, dtype=torch.float64) * 100.0
    t[3, 1, 2], t[9, 0, 4] = 2.0 ** 40, -2.0 ** 40
    t[:, 1, 4] = 2.0 ** 40.5
    d = t * 2.0 ** 16
    hi = torch.round(d)
    words = torch.stack([hi.to(torch.int64), torch.round((d - hi) * 2.0 ** 40).to(torch.int64)])
    want = np.array([[float(sum(Fraction(float(v)) for v in t[:, k, c])) for c in range(5)] for k in range(2)])
    assert_close(decode_totals(words), want, 0.0, atol=64 * 2.0 ** -57, what="decoded totals")


# ---- 1. bn_act -------------------------------------------------------------------------------------------------------------------------------
BN_ACT_SHAPES = [(1, 4), (7, 12), (33, 260), (1000, 64)]
BN_ACT_STRIDE = (8200, 512)          # 1,049,600 vectors of 4: 1,024 of them in the second trip of the grid-stride loop


@functools.lru_cache(None)
def _bn_act_operands(P, C, dtname):
    """x, r (storage-rounded, f32 on the CPU) and the four f32 tables of one shape: computed once, never written"""
    dt = getattr(torch, dtname)
    g = torch.Generator().manual_seed(P * 1000 + C + (dt == BF))
    x, r = (torch.randn(P, C, generator=g).to(dt).float() for _ in range(2))
    s, t, rs, rt = (torch.randn(C, generator=g) for _ in range(4))          # about half of the scales are negative
    return x, r, s, t, rs, rt


def _bn_act_forms(r, rs, rt):
    return {"no-residual": (None, None, None), "residual": (r, None, None), "residual-affine": (r, rs, rt)}


def _bn_act_bound(ref, mag, dt):
    return 4 * U32 * mag + (UB * ref.abs() if dt == BF else 0.0)


def _dev(t, dt=None):
    return None if t is None else (t.to(dt) if dt is not None else t).cuda()


@pytest.mark.gpu
@DTYPES
def test_bn_act_against_f64(gpu_lib, dt):
    """every form x relu on / off at ragged (P, C); `out=x` (the in-place use of resnet.py) gives the same bits"""
    from mhentropy_amd import ops
    m = _Measure("bn_act " + _dtn(dt))
    for P, C in BN_ACT_SHAPES:
        x, r, s, t, rs, rt = _bn_act_operands(P, C, _dtn(dt))
        for form, (fr, frs, frt) in _bn_act_forms(r, rs, rt).items():
            for relu in (True, False):
                ref, mag = bn_act_reference(x, s, t, fr, frs, frt, relu)
                xd = _dev(x, dt)
                args = (_dev(s), _dev(t), _dev(fr, dt), _dev(frs), _dev(frt))
                y = ops.bn_act(xd, *args, relu=relu)
                m.add((P, C, form, relu), _np(y), ref.numpy(), _bn_act_bound(ref, mag, dt).numpy())
                assert torch.equal(_bits(xd), _bits(x.to(dt))), "bn_act wrote its input"
                y2 = ops.bn_act(xd, *args, relu=relu, out=xd)
                assert y2.data_ptr() == xd.data_ptr() and torch.equal(_bits(y2), _bits(y)), ("out= aliased to x differs", P, C, form, relu)
    m.report()


@pytest.mark.gpu
@DTYPES
def test_bn_act_grid_stride_second_trip(gpu_lib, dt):
    """(8200, 512): more vectors than the capped grid covers at once; the last 1,024 vectors are written by the loop's second trip"""
    from mhentropy_amd import ops
    P, C = BN_ACT_STRIDE
    assert EW_CAP < P * C // 4 <= EW_CAP + 1024
    x, r, s, t, rs, rt = _bn_act_operands(P, C, _dtn(dt))
    m = _Measure("bn_act grid-stride " + _dtn(dt))
    xd, rd = _dev(x, dt), _dev(r, dt)
    for form, (fr, frs, frt) in _bn_act_forms(r, rs, rt).items():
        ref, mag = bn_act_reference(x, s, t, fr, frs, frt, True)
        y = ops.bn_act(xd, _dev(s), _dev(t), None if fr is None else rd, _dev(frs), _dev(frt), relu=True)
        m.add((P, C, form), _np(y), ref.numpy(), _bn_act_bound(ref, mag, dt).numpy())
    # in place, no relu: a vector the second trip skipped would keep x
    ref, mag = bn_act_reference(x, s, t, None, None, None, False)
    y = ops.bn_act(xd, _dev(s), _dev(t), relu=False, out=xd)
    m.add((P, C, "in place"), _np(y), ref.numpy(), _bn_act_bound(ref, mag, dt).numpy())
    m.report()


# ---- 2. max pool -----------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1, 4), (2, 1, 7, 8), (2, 7, 1, 12), (3, 2, 2, 8), (2, 18, 18, 64), (3, 19, 22, 12), (3, 19, 22, 24)]


@functools.lru_cache(None)
def _pool_operands(shape, dtname):
    dt = getattr(torch, dtname)
    B, H, W, C = shape
    g = torch.Generator().manual_seed(B + 10 * H + 100 * W + 1000 * C + (dt == BF))
    x = torch.randn(B, H, W, C, generator=g).to(dt).float()
    s, t = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    s[::7] *= -1.0          # every seventh scale negative
    return x, s, t


@pytest.mark.gpu
@DTYPES
def test_maxpool_without_the_affine_is_bit_equal(gpu_lib, dt):
    """random and all-negative inputs: the stored values' maximum, to the bit (on bf16: C % 8 == 0 rows on maxpool8_kernel, C % 8 == 4 rows on
    maxpool_kernel<u16>)"""
    from mhentropy_amd import ops
    for shape in POOL_SHAPES:
        x, _, _ = _pool_operands(shape, _dtn(dt))
        for what, v in (("random", x), ("all negative", -x.abs() - 0.125)):
            y = ops.maxpool3x3s2(_dev(v, dt))
            assert torch.equal(_bits(y), _bits(maxpool_reference(v).to(dt))), (shape, what)
    print("forward-edges: maxpool3x3s2 %s without the affine: bit-equal at %d shapes" % (_dtn(dt), len(POOL_SHAPES)))


@pytest.mark.gpu
@DTYPES
def test_maxpool_with_the_affine_against_f64(gpu_lib, dt):
    from mhentropy_amd import ops
    m = _Measure("maxpool3x3s2 affine " + _dtn(dt))
    for shape in POOL_SHAPES:
        x, s, t = _pool_operands(shape, _dtn(dt))
        ref, mag = maxpool_reference(x, s, t)
        y = ops.maxpool3x3s2(_dev(x, dt), _dev(s), _dev(t))
        m.add(shape, _np(y), ref.numpy(), (2 * U32 * mag + (UB * ref.abs() if dt == BF else 0.0)).numpy())
    m.report()


@pytest.mark.gpu
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
def test_maxpool_bf16_four_channel_kernel_agrees_with_the_eight_channel_kernel(gpu_lib, affine):
    """bf16, C % 8 == 4 (maxpool_kernel<u16>: guarded loads) against the same channels twice, C % 8 == 0 (maxpool8_kernel: clamped loads and a
    select): both halves of the wide result are the narrow result to the bit"""
    from mhentropy_amd import ops
    rows = [sh for sh in POOL_SHAPES if sh[3] % 8 == 4]
    assert len(rows) == 3
    for shape in rows:
        x, s, t = _pool_operands(shape, "bfloat16")
        C = shape[3]
        tab = lambda v: (_dev(torch.cat([v, v])) if affine else None)
        narrow = ops.maxpool3x3s2(_dev(x, BF), _dev(s) if affine else None, _dev(t) if affine else None)
        wide = ops.maxpool3x3s2(_dev(torch.cat([x, x], -1), BF), tab(s), tab(t))
        assert torch.equal(_bits(wide[..., :C]), _bits(narrow)) and torch.equal(_bits(wide[..., C:]), _bits(narrow)), shape


# 5 x 5 images (3 x 3 outputs: corner, edge and one interior window), as many as put the output just past the capped grid
POOL_STRIDE = [(F32, 4), (BF, 4), (BF, 8)]          # maxpool_kernel<float>, maxpool_kernel<u16> (C % 8 == 4), maxpool8_kernel


@pytest.mark.gpu
@pytest.mark.parametrize("dt,C", POOL_STRIDE, ids=["f32-4ch", "bf16-4ch", "bf16-8ch"])
def test_maxpool_grid_stride_second_trip(gpu_lib, dt, C):
    """one vector of the kernel's width per output pixel and 1,049,400 output pixels: 824 of them belong to the second trip.  The reference is
    F.max_pool2d in f32 (max is exact)"""
    from mhentropy_amd import ops
    B, H, W = 116600, 5, 5
    assert EW_CAP < B * 3 * 3 <= EW_CAP + 1024
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, H, W, C, generator=g).to(dt)
    y = ops.maxpool3x3s2(x.cuda())
    ref = maxpool_reference(x.float()).to(dt)
    assert torch.equal(_bits(y), _bits(ref))
    assert torch.equal(_bits(y[-100:]), _bits(ref[-100:])), "the second trip's images"


# ---- 3. average pool and its fused form ------------------------------------------------------------------------------------------------------
def _avgpool_bound(absmean, HW):
    return (HW / 4 + 4) * U32 * absmean


@pytest.mark.gpu
@DTYPES
def test_avgpool_against_f64(gpu_lib, dt):
    """HW < 4 leaves pixel groups empty, C = 8 / 72 / 200 leave the last 64-channel workgroup partly idle"""
    from mhentropy_amd import ops
    m = _Measure("avgpool " + _dtn(dt))
    g = torch.Generator().manual_seed(31 + (dt == BF))
    for HW in (1, 3, 4, 5, 49, 257):
        for C in (8, 64, 72, 200):
            for B in (1, 3):
                x = (torch.randn(B, HW, 1, C, generator=g) + 0.25).to(dt).float()
                y = ops.avgpool(_dev(x, dt))
                assert tuple(y.shape) == (B, C)
                xd = x.double().reshape(B, HW, C)
                m.add((B, HW, C), _np(y), xd.mean(1).numpy(), _avgpool_bound(xd.abs().mean(1), HW).numpy())
    m.report()


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("form", FORMS)
def test_bn_act_avgpool_is_the_two_launches_and_close_to_f64(gpu_lib, form, dt):
    """C = 4, 12, 260 leave part of the last 256-channel workgroup idle: bit for bit ops.avgpool(ops.bn_act(...)), and within the sum of the two
    kernels' bounds of f64"""
    from mhentropy_amd import ops
    m = _Measure("bn_act_avgpool %s %s" % (form, _dtn(dt)))
    g = torch.Generator().manual_seed(77 + FORMS.index(form) + 10 * (dt == BF))
    for C in (4, 12, 260, 512):
        s, t, rs, rt = (torch.randn(C, generator=g) for _ in range(4))
        for HW in (1, 3, 49):
            for B in (1, 3):
                x, r = (torch.randn(B, HW, 1, C, generator=g).to(dt).float() for _ in range(2))
                fr, frs, frt = _bn_act_forms(r, rs, rt)[form]
                xd, args = _dev(x, dt), (_dev(s), _dev(t), _dev(fr, dt), _dev(frs), _dev(frt))
                for relu in (True, False):
                    y = ops.bn_act_avgpool(xd, *args, relu=relu)
                    two = ops.avgpool(ops.bn_act(xd, *args, relu=relu))
                    assert torch.equal(_bits(y), _bits(two)), ("not the two launches' bits", C, HW, B, relu)
                    ref, mag = bn_act_reference(x, s, t, fr, frs, frt, relu)
                    pix = lambda v: v.reshape(B, HW, C).mean(1)
                    m.add((C, HW, B, relu), _np(y), pix(ref).numpy(), (pix(_bn_act_bound(ref, mag, dt)) + _avgpool_bound(pix(ref.abs()), HW)).numpy())
                    if dt == BF:
                        stored = ref.float().to(BF).double()          # the kernel sums what bn_act would have stored
                        bound = pix(4 * U32 * mag + 2 * UB * ref.abs()) + _avgpool_bound(pix(stored.abs()), HW)
                        m.add((C, HW, B, relu, "from rounded values"), _np(y), pix(stored).numpy(), bound.numpy())
    m.report()


# ---- 4. NCHW -> NHWC -------------------------------------------------------------------------------------------------------------------------
def _same_or_both_nan(got, want, what):
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(gn, wn), what + ": NaN positions"
    assert torch.equal(_bits(got)[~gn], _bits(want)[~wn]), what + ": bits"


def _special_image(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    flat = x.view(-1)
    special = torch.tensor([0.0, -0.0, INF, -INF, NAN, 3.0e38, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -8])
    flat[torch.arange(len(special)) * 3 % flat.numel()] = special          # zeros, infinities, NaN, bf16 ties
    return x


def _check_layout(y, x, Cp, dt, what):
    B, C, H, W = x.shape
    y = y.cpu()
    assert tuple(y.shape) == (B, H, W, Cp) and y.dtype == dt, what
    want = x.permute(0, 2, 3, 1).contiguous()
    if dt == F32:
        assert torch.equal(_bits(y[..., :C]), _bits(want)), what + ": f32 copy is not bit-equal"          # NaN payload included
    else:
        _same_or_both_nan(y[..., :C], want.to(BF), what)
    assert not _bits(y[..., C:]).any(), what + ": padding channels are not +0"


@pytest.mark.gpu
@DTYPES
def test_nchw_to_nhwc_bits(gpu_lib, dt):
    """C = 1, 3, 5, 8, 9 at 5 x 7 with +-0, +-inf, NaN, a value near the largest and bf16 ties; channels padded to a 16-byte chunk with zeros"""
    from mhentropy_amd import ops
    chunk = 4 if dt == F32 else 8
    for C in (1, 3, 5, 8, 9):
        x = _special_image(2, C, 5, 7, C)
        _check_layout(ops.nchw_to_nhwc(x.cuda(), dt), x, (C + chunk - 1) // chunk * chunk, dt, "nchw_to_nhwc C = %d %s" % (C, _dtn(dt)))


@pytest.mark.gpu
@pytest.mark.parametrize("C,Cp,dt", [(3, 4, BF), (3, 4, F32), (3, 8, BF), (5, 8, BF)], ids=["3to4-bf16", "3to4-f32", "3to8-bf16", "5to8-bf16"])
def test_nchw_to_nhwc_pad_bits(gpu_lib, C, Cp, dt):
    from mhentropy_amd import ops
    x = _special_image(2, C, 5, 7, 10 * C + Cp)
    _check_layout(ops.nchw_to_nhwc(x.cuda(), dt, cpad=Cp), x, Cp, dt, "nchw_to_nhwc_pad %d -> %d %s" % (C, Cp, _dtn(dt)))


@pytest.mark.gpu
@pytest.mark.parametrize("Cp", [4, 8], ids=["3to4-kernel", "generic-kernel"])
def test_nchw_to_nhwc_grid_stride_second_trip(gpu_lib, Cp):
    """1 x 3 x 1025 x 1024 = 1,049,600 pixels, bf16: the last 1,024 pixels belong to the second trip"""
    from mhentropy_amd import ops
    x = _special_image(1, 3, 1025, 1024, Cp)
    assert EW_CAP < 1025 * 1024 <= EW_CAP + 1024
    _check_layout(ops.nchw_to_nhwc(x.cuda(), BF, cpad=Cp), x, Cp, BF, "nchw_to_nhwc_pad 3 -> %d at 1025 x 1024" % Cp)


# ---- 5. bn_finalize over wave_totals ---------------------------------------------------------------------------------------------------------
S2_BIG, S1_BIG = 11, 40          # the channels of the C = 67 unit that hold one shard of 2^40 / -2^40 (shards 5 and 50)
MOMENTUM, EPS = 0.1, 1e-5


@functools.lru_cache(None)
def _stat_unit(C):
    """(shard values [64, 2, C] f64, count, gamma, beta, running mean, running var): shard s covers count / 64 samples of mean mu_s (mixed
    signs) and mean square mu_s^2 + 1 + 40 rand, so that every shard word differs and the variance is at least 1.  C = 67: count = 2^34 (shards
    near 2^28, still summed as integers) - channel 11 gets one s2 shard of 2^40 (64 more variance), channel 40 one s1 shard of -2^40 (mean - 64)
    with s2 shards of (5000 .. 6000) count / 64, which keeps its variance above 900; both take the double-precision path of wave_totals"""
    g = torch.Generator().manual_seed(400 + C)
    count = 2.0 ** 34 if C == 67 else 4096.0
    mu = torch.randn(64, C, generator=g, dtype=torch.float64)
    q = mu ** 2 + 1.0 + 40.0 * torch.rand(64, C, generator=g, dtype=torch.float64)
    t = torch.stack([mu, q], 1) * (count / 64)
    if C == 67:
        t[5, 1, S2_BIG] = 2.0 ** 40
        t[:, 1, S1_BIG] = (5000.0 + 1000.0 * torch.rand(64, generator=g, dtype=torch.float64)) * (count / 64)
        t[50, 0, S1_BIG] = -2.0 ** 40
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    return t, count, gamma, torch.randn(C, generator=g), torch.randn(C, generator=g), torch.rand(C, generator=g) * 3.0 + 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("clear", [False, True], ids=["keep", "clear"])
@pytest.mark.parametrize("want_mi", [False, True], ids=["affine", "affine+mean_invstd"])
@pytest.mark.parametrize("C", [1, 3, 5, 64, 67])
def test_bn_finalize_against_f64_from_the_decoded_words(gpu_lib, C, want_mi, clear):
    from mhentropy_amd import ops
    assert ops.stat_shards() == 64
    t, count, gamma, beta, rmean0, rvar0 = _stat_unit(C)
    words = ops.stat_from_float(t)
    s1, s2 = decode_totals(words)
    if C == 67:
        assert (words[0].abs() >= 2 ** 55).any(1).any(0).nonzero().flatten().tolist() == [S2_BIG, S1_BIG], "only these two channels take the double path"
    mean = s1 / count
    var = s2 / count - mean ** 2
    assert var.min() > 0.9, var.min()
    mom, eps = float(np.float32(MOMENTUM)), float(np.float32(EPS))          # the kernel's own f32 parameters
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma.double().numpy() * invstd
    st, rmean, rvar = words.cuda(), rmean0.clone().cuda(), rvar0.clone().cuda()
    nbt = torch.full((), 41, dtype=torch.int64, device="cuda") if (clear or C == 67) else None
    out = ops.bn_finalize(st, gamma.cuda(), beta.cuda(), rmean, rvar, count, MOMENTUM, EPS, want_mean_invstd=want_mi, clear=clear, num_batches_tracked=nbt)
    m = _Measure("bn_finalize C = %d%s%s" % (C, " + mean_invstd" if want_mi else "", " clear" if clear else ""))
    m.add("scale", _np(out[0]), scale, 4 * U32 * np.abs(scale))
    m.add("shift", _np(out[1]), beta.double().numpy() - mean * scale, 4 * U32 * (beta.double().abs().numpy() + np.abs(mean * scale)))
    if want_mi:
        m.add("mean", _np(out[2][0]), mean, U32 * np.abs(mean))
        m.add("1 / std", _np(out[2][1]), invstd, 4 * U32 * invstd)
    unbiased = var * (count / (count - 1.0))
    m.add("running_mean", _np(rmean), (1 - mom) * rmean0.double().numpy() + mom * mean, 4 * U32 * (rmean0.double().abs().numpy() + np.abs(mean)))
    m.add("running_var", _np(rvar), (1 - mom) * rvar0.double().numpy() + mom * unbiased, 4 * U32 * (rvar0.double().numpy() + unbiased))
    m.report()
    if nbt is not None:
        assert int(nbt) == 42, "num_batches_tracked must rise by exactly 1 (%d workgroups)" % ((C + 3) // 4)
    if clear:
        assert not st.cpu().any(), "clear=True must zero all four planes"
    else:
        assert torch.equal(st.cpu(), words), "clear=False must leave the words untouched"


# ---- 6. serial row sums ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["sum_over_hypotheses", "sum_row_blocks"])
def test_row_sums_against_f64(gpu_lib, kernel):
    """rows [N * B, C] summed over n: sum_over_hypotheses takes row n * B + b, sum_row_blocks row g * N + n.  Dense `out`, and `out` as the
    first C columns of a [B, C + 5] matrix whose other columns must not change; with and without `accumulate`"""
    from mhentropy_amd import ops
    m = _Measure(kernel)
    g = torch.Generator().manual_seed(len(kernel))
    for N in (1, 7, 200):
        for B in (1, 3):
            for C in (1, 61, 513):
                rows = torch.randn(N * B, C, generator=g)
                per = rows.double().view(N, B, C) if kernel == "sum_over_hypotheses" else rows.double().view(B, N, C).transpose(0, 1)
                total, mag = per.sum(0), per.abs().sum(0)
                rd = rows.cuda()
                call = (lambda **kw: ops.sum_over_hypotheses(rd, N, B, **kw)) if kernel == "sum_over_hypotheses" else (lambda **kw: ops.sum_row_blocks(rd, B, N, **kw))
                m.add((N, B, C, "fresh"), _np(call()), total.numpy(), (N * U32 * mag).numpy())
                for accumulate in (False, True):
                    wide = torch.randn(B, C + 5, generator=g)
                    dev = wide.cuda()
                    call(out=dev[:, :C], out_stride=C + 5, accumulate=accumulate)
                    got = dev.cpu()
                    assert torch.equal(_bits(got[:, C:]), _bits(wide[:, C:])), ("columns beside `out` written", N, B, C, accumulate)
                    old = wide[:, :C].double() if accumulate else torch.zeros(B, C, dtype=torch.float64)
                    m.add((N, B, C, "strided", accumulate), got[:, :C].double().numpy(), (old + total).numpy(), (N * U32 * (old.abs() + mag)).numpy())
    m.report()


# ---- 7. elbo_reduce --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_q", [True, False], ids=["log_q", "no-log_q"])
def test_elbo_reduce_against_f64(gpu_lib, with_q):
    """q_log_p = mean_n lp, h = - mean_n lq, log_p = h + q_log_p; N around the 64 lanes, B around the 4 images of a workgroup"""
    from mhentropy_amd import ops
    m = _Measure("elbo_reduce" + ("" if with_q else " without log_q"))
    g = torch.Generator().manual_seed(13 + with_q)
    for N in (1, 63, 64, 65, 200):
        for B in (1, 3, 4, 5):
            lp = torch.randn(N * B, generator=g) * 30.0 - 50.0
            lq = torch.randn(N * B, generator=g) * 5.0 + 2.0
            q, h, p = ops.elbo_reduce(lp.cuda(), lq.cuda() if with_q else None, N, B)
            lp64, lq64 = lp.double().view(N, B), (lq.double().view(N, B) if with_q else torch.zeros(N, B, dtype=torch.float64))
            bound = ((N / 64 + 8) * U32 * (lp64.abs().sum(0) + lq64.abs().sum(0)) / N).numpy()
            m.add((N, B, "q_log_p"), _np(q), lp64.mean(0).numpy(), bound)
            m.add((N, B, "h"), _np(h), -lq64.mean(0).numpy(), bound)
            m.add((N, B, "log_p"), _np(p), (lp64.mean(0) - lq64.mean(0)).numpy(), bound)
            if not with_q:
                assert not _bits(h).any(), "without log_q the entropy term is +0"
    m.report()


# ---- 8. reparam ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sigmoid", [False, True], ids=["exp", "sigmoid"])
@pytest.mark.parametrize("n", [1, 257, 1024 * 256 + 3], ids=["1", "257", "grid-stride"])
def test_reparam_against_f64(gpu_lib, n, sigmoid):
    """sd = exp(l2 / 2) | sigmoid(l2) for l2 in [-20, 20], z = mn + sd eps; 1024 * 256 + 3 elements put three into the loop's second trip"""
    from mhentropy_amd import ops
    g = torch.Generator().manual_seed(n + sigmoid)
    mn, eps = torch.randn(n, generator=g), torch.randn(n, generator=g)
    l2 = torch.rand(n, generator=g) * 40.0 - 20.0
    l2[:2] = torch.tensor([-20.0, 20.0])[:n]
    sd64 = torch.sigmoid(l2.double()) if sigmoid else torch.exp(l2.double() / 2)
    m = _Measure("reparam %s n = %d" % ("sigmoid" if sigmoid else "exp", n))
    sd, z = ops.reparam(mn.cuda(), l2.cuda(), eps.cuda(), sigmoid_act=sigmoid)
    m.add("sd", _np(sd), sd64.numpy(), (4 * U32 * sd64).numpy())
    m.add("z", _np(z), (mn.double() + sd64 * eps.double()).numpy(), (4 * U32 * (mn.double().abs() + (sd64 * eps.double()).abs())).numpy())
    for what, (sd_d, z_d) in (("deterministic", ops.reparam(mn.cuda(), l2.cuda(), eps.cuda(), sigmoid_act=sigmoid, deterministic=True)),
                              ("eps=None", ops.reparam(mn.cuda(), l2.cuda(), None, sigmoid_act=sigmoid))):
        assert torch.equal(_bits(z_d), _bits(mn)), what + ": z must be mn to the bit"
        assert torch.equal(_bits(sd_d), _bits(sd)), what + ": sd differs from the stochastic form's"
    m.report()


# ---- 9. dropout_, apply form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout_apply_form_against_the_mask(gpu_lib, p, dt):
    """given bits, no draw: 8 * (512 * 256 + 5) elements, five mask bytes in the loop's second trip; x * ops.dropout_mask(bits) in f64"""
    from mhentropy_amd import ops
    n = 8 * (512 * 256 + 5)
    g = torch.Generator().manual_seed(int(p * 10) + (dt == BF))
    x = torch.randn(n, generator=g).to(dt).float()
    bits = torch.randint(0, 256, (n // 8,), generator=g, dtype=torch.uint8)
    bits[-5:] = torch.tensor([0x00, 0xFF, 0xA5, 0x5A, 0x01], dtype=torch.uint8)
    mask = ops.dropout_mask(bits, (n,), p)
    keep = mask != 0
    assert 0.45 < keep.float().mean() < 0.55          # whatever p is: the bits given here are uniform bytes, p only sets the scale of the kept
    xd, bd = _dev(x, dt), bits.cuda()
    back = ops.dropout_(xd, p, bits=bd)
    assert back.data_ptr() == bd.data_ptr() and torch.equal(bd.cpu(), bits), "the given bits were changed"
    ref = x.double() * mask.double()
    m = _Measure("dropout_ apply p = %g %s" % (p, _dtn(dt)))
    m.add("kept", _np(xd)[keep.numpy()], ref.numpy()[keep.numpy()], ((UB if dt == BF else U32) * ref.abs()).numpy()[keep.numpy()])
    m.report()
    assert not _bits(xd)[~keep].any(), "dropped elements must be +0"


# ---- 10. topk_gather -------------------------------------------------------------------------------------------------------------------------
def _scores(kind, N, B, g):
    s = torch.randn(N, B, generator=g)
    if kind == "ties":
        s = torch.floor(s.clamp(-1.9, 1.9))          # four levels
    elif kind == "inf-and-zeros":
        pick = torch.randint(0, 6, (N, B), generator=g)
        for k, v in enumerate((INF, -INF, 0.0, -0.0)):
            s[pick == k] = v
    return s


def _check_topk(ops, s, rows, N, B, Q, D, what):
    idx, out = ops.topk_gather(s.reshape(-1).cuda(), rows.cuda(), N, B, Q)
    ref = topk_reference(s.numpy(), Q)
    idx = idx.cpu().numpy()
    assert idx.shape == (Q, B) and np.array_equal(idx, ref), (what, idx, ref)
    want = rows.view(N, B, D)[torch.as_tensor(ref, dtype=torch.int64), torch.arange(B)[None, :]]          # [Q, B, D]
    assert torch.equal(_bits(out), _bits(want.reshape(Q * B, D))), (what, "gathered rows")
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["continuous", "ties", "inf-and-zeros"])
def test_topk_gather_is_a_stable_descending_sort(gpu_lib, kind):
    """idx and the gathered rows are exact; among equal scores (-0.0 == +0.0 included) the lower index comes first"""
    from mhentropy_amd import ops
    g = torch.Generator().manual_seed(len(kind))
    count = 0
    for N in (1, 5, 64, 65, 200):
        for B in (1, 3, 5):
            s = _scores(kind, N, B, g)
            for D in (1, 45, 64, 65):
                rows = torch.randn(N * B, D, generator=g)
                for Q in sorted({1, max(N // 2, 1), N}):
                    _check_topk(ops, s, rows, N, B, Q, D, (kind, N, B, Q, D))
                    count += 1
    print("forward-edges: topk_gather %s: exact at %d (N, B, D, Q)" % (kind, count))


@pytest.mark.gpu
@pytest.mark.parametrize("N,Q", [(5, 3), (65, 65), (200, 100)])
def test_topk_gather_with_nan_scores_writes_every_slot(gpu_lib, N, Q):
    """K = 0, K < Q and K >= Q rows that are not NaN, one image each (and one without NaN): Q distinct indices in [0, N) per image, NaN rows
    first in index order, then the numbers descending; the rows match"""
    from mhentropy_amd import ops
    B, D = 4, 45
    g = torch.Generator().manual_seed(N)
    s = torch.floor(torch.randn(N, B, generator=g) * 2.0)          # ties among the numbers as well
    s[:, 0] = NAN                                                      # K = 0
    s[torch.randperm(N, generator=g)[:N - (Q - 1) // 2], 1] = NAN      # K = (Q - 1) // 2 < Q
    s[torch.randperm(N, generator=g)[:N - Q], 2] = NAN                 # K = Q
    K = (~torch.isnan(s)).sum(0).tolist()
    assert K[0] == 0 and K[1] < Q and K[2] >= Q and K[3] == N, K
    rows = torch.randn(N * B, D, generator=g)
    idx = _check_topk(ops, s, rows, N, B, Q, D, ("NaN scores", N, Q))          # the kernel's idx, already equal to the reference order
    for b in range(B):
        assert len(set(idx[:, b].tolist())) == Q and idx[:, b].min() >= 0 and idx[:, b].max() < N
