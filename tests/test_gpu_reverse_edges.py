"""The reverse pass's small kernels (csrc/trunk_bwd.hip, csrc/flow_bwd.hip), each against the float64 references of tests/reverse_ref.py at the
edges it has: BatchNorm reverse (reduce, finalize, the three apply kernels, mean / invstd), the max pool's winners and its scatter with the
fused BatchNorm forms, average pool and stride-2 reverse, gradient norm, clip + Adam, and the RealNVP coupling reverse with its element-wise
stages.  Shapes: channel counts that leave threads idle, pixel counts below and around one block's share, and one case per grid-stride loop
above its capped grid.

Operands are rounded to the storage type on the CPU; every expected value is float64 on the CPU from those rounded operands.

Bounds (u32 = 2^-24, ub = 2^-8; none of them is tuned, the measured max(|diff| / bound) is printed before it is asserted, `pytest -s`):
  gates, scatters   exact: g [a > 0] with a = +0, -0, a negative value and the smallest subnormal as float64 `a > 0` says; winners, pooled values,
                    xwin and the scattered, gated gradient on dyadic inputs (every f32 partial result exact), bf16 copies, padding columns +0
  bn_bwd_reduce     sum g': L u32 sum |g'| + W 2^-56;  sum g' xhat: (L + 3) u32 sum |g' xhat| + W 2^-56.  L = the longest serial f32 chain
                    = ceil(rows per block / row lanes) + row lanes - 1 (the LDS fold), W = contributing workgroups (one fx::add2 quantum each),
                    + 3 for the roundings of every term (subtraction, product with invstd, fma)
  pooled_bn_sums,   the same with L = trips of the grid-stride walk + 256 / (C / E) folded partials
  maxpool_bwd_bn
  bn_bwd_finalize   from the words decoded on the CPU (ops.stat_totals): dbeta, dgamma u32 relative (one rounding of the f64 total); k2 u32;
                    k1 6 u32 (five roundings: k2, two products, the rounded dgamma, the division; + 1 for second order);
                    k0 8 u32 (|k2 dbeta / M| + |k1 mean|) (four roundings on the first term, six on the second, one sum; + 1)
  bn_mean_invstd    mean u32 relative, 1 / std 4 u32 relative (var to f32, + eps, sqrt, division)
  bn_bwd_apply      2 u32 (|k2 g'| + |k1 y| + |k0|) (two fma), bf16 + ub |ref|; all three kernels and maxpool_bwd_bn's apply form
  avgpool_bwd       2 u32 |ref| (1 / HW, the product), bf16 + ub |ref|
  upsample2         without base value-equal (a -0.0 gradient comes out as +0.0: 0 + -0); with base u32 (|base| + |g|), bf16 + ub |ref|
  sqnorm            (L + 22) u32 sum g^2, L = 4 ceil((n / 4) / 262144) (+ 1 with a tail) the longest per-thread fma chain; two calls bit-equal
  adam_step         reverse_ref.clip_adam's per-element bounds on m, v, p from the operation count; powf as below
  mask_pad          u32 |ref|, bf16 + ub |ref|;  cond_lrelu 2 u32 (|pre| + |cond|) (sum, slope product), bf16 + ub |ref|;
  lrelu_bwd         u32 |ref|, bf16 + ub |ref|;  add u32 (|a| + |b|);  couple_accum 3 u32 (|g_part| + |m| (|GXs| + |GXt|))
  couple_bwd        reverse_ref.couple_bwd's model: every operation u32 of its result, tanhf / expf one ulp of theirs, 1 - s^2 the absolute
                    error 2 |s| ulp(s) + u32; db_s / db_t against the f64 column sums of the written rows: (19 + workgroups) u32 (|old| + sum |row|)
  transcendentals   the model times max(1, ceil(2 r)), r = the error of a plain float32 torch evaluation of the same formula on the CPU against
                    float64, in units of the model bound, over the test's own inputs (computed by the test, never from the kernel).  Measured:
                    couple_bwd r = 0.66 -> factor 2; adam_step r = 1.00 (p at step 100000) -> factor 2

Max pool and NaN (observed, not asserted): maxpool_idx_kernel keeps a NaN only if it is the first tap of its window inside the image (v > m is
false either way); torch propagates every NaN.
"""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

import reverse_ref as rr
from edge_measure import Measure

BF, F32 = torch.bfloat16, torch.float32
U32, UB = 2.0 ** -24, 2.0 ** -8
DTYPES = pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
EW_CAP, FLOW_CAP = 8192 * 256, 16384 * 256          # lanes one launch covers in its first trip: ewg of trunk_bwd.hip, ew_grid of flow_bwd.hip
SLOPE = float(np.float32(0.01))                       # the kernels' own f32 constant


def M(kernel):
    return Measure(kernel, "reverse-edges")


def _dtn(dt):
    return "bf16" if dt == BF else "f32"


def _np(t):
    return t.detach().cpu().double().numpy()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _dev(t, dt=None):
    return None if t is None else (t.to(dt) if dt is not None else t).cuda()


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _ub(ref, dt):
    return UB * ref.abs() if dt == BF else 0.0


def _plant_gate(a, dt):
    """+0, -0, a negative value and the smallest positive subnormal of dt at the front of a gate tensor"""
    flat = a.view(-1)
    vals = torch.tensor([0.0, -0.0, -1.0, 2.0 ** -149 if dt == F32 else 2.0 ** -133])[:flat.numel()]
    flat[:len(vals)] = vals
    return a


def _ewg(n, cap=8192):
    return min(max(-(-n // 256), 1), cap)


# ---- 1. BatchNorm reverse: reduce, finalize, mean / invstd ----------------------------------------------------------------------------------
REDUCE_SHAPES = [(P, C) for P in (1, 5, 63, 64, 65, 257, 4161) for C in (4, 12, 20, 400)] + [(7, 1028), (4161, 64), (131073 + 5, 4)]


def _reduce_geometry(P, C):
    """(workgroups, L) of mhe_bn_bwd_reduce_nhwc's launch: L = rows per row lane + the LDS fold"""
    blocks = min(max(P // 64, 1), 2048)
    rpb = -(-P // blocks)
    blocks = -(-P // rpb)
    rl_n = 256 // min(C // 4, 256)
    return blocks, -(-rpb // rl_n) + rl_n - 1


@functools.lru_cache(None)
def _bn_operands(P, C, dtname):
    dt = BF if dtname == "bf16" else F32
    g = _gen(P, C, dtname)
    gr, y = torch.randn(P, C, generator=g).to(dt).float(), (torch.randn(P, C, generator=g) * 2 + 0.5).to(dt).float()
    a = _plant_gate(torch.relu(torch.randn(P, C, generator=g)).to(dt).float(), dt)
    mean, invstd = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    return gr, a, y, mean, invstd, gamma


def _sum_bounds(mag1, mag2, L, W):
    return L * U32 * mag1 + W * 2.0 ** -56, (L + 3) * U32 * mag2 + W * 2.0 ** -56


def _check_finalize(m, case, ops, st, tot, gamma, mean, invstd, count, skip=None):
    C = gamma.numel()
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    coef = ops.bn_bwd_coef(st, gamma.cuda(), torch.stack([mean, invstd]).cuda(), dg, db, count)
    c = rr.bn_bwd_coef(tot[0], tot[1], gamma, mean, invstd, count)
    keep = np.ones(C, bool) if skip is None else ~skip
    for name, got, k, mag in (("dbeta", db, 1, c["dbeta"].abs()), ("dgamma", dg, 1, c["dgamma"].abs()), ("k2", coef[0], 1, c["k2"].abs()),
                              ("k1", coef[1], 6, c["k1"].abs()), ("k0", coef[2], 8, c["k0mag"])):
        m.add(case + (name,), _np(got)[keep], c[name].numpy()[keep], (k * U32 * mag).numpy()[keep])
    return dg, db


@pytest.mark.gpu
@DTYPES
def test_bn_bwd_reduce_and_finalize_against_f64(gpu_lib, dt):
    """every (P, C) with the gate and without: idle row lanes (C = 12, 20, 400), a ragged second quad trip (1028), P below one row group, the
    unrolled loop's remainder, a short last block, more than 64 blocks and the 2048-block cap"""
    from mhentropy_amd import ops
    m, mf = M("bn_bwd_reduce " + _dtn(dt)), M("bn_bwd_finalize " + _dtn(dt))
    for P, C in REDUCE_SHAPES:
        gr, a, y, mean, invstd, gamma = _bn_operands(P, C, _dtn(dt))
        W, L = _reduce_geometry(P, C)
        mi = torch.stack([mean, invstd]).cuda()
        for gate in (a, None):
            st = ops.stat_unit(C, "cuda")
            ops.launch("mhe_bn_bwd_reduce_nhwc", _dev(gr, dt), _dev(gate, dt), _dev(y, dt), mi, st, P, C, ops.dtype_code(dt))
            tot = ops.stat_totals(st.cpu())
            s1, s2, mag1, mag2 = rr.bn_bwd_sums(gr, gate, y, mean, invstd)
            b1, b2 = _sum_bounds(mag1, mag2, L, W)
            case = (P, C, "gate" if gate is not None else "no gate")
            m.add(case + ("sum g'",), tot[0].numpy(), s1.numpy(), b1.numpy())
            m.add(case + ("sum g' xhat",), tot[1].numpy(), s2.numpy(), b2.numpy())
            _check_finalize(mf, case, ops, st, tot, gamma, mean, invstd, P)
    m.report()
    mf.report()


@pytest.mark.gpu
def test_bn_bwd_reduce_accumulates_and_marks_a_non_finite_partial(gpu_lib):
    from mhentropy_amd import ops
    P, C = 257, 12
    gr, a, y, mean, invstd, gamma = _bn_operands(P, C, "f32")
    W, L = _reduce_geometry(P, C)
    mi = torch.stack([mean, invstd]).cuda()
    m = M("bn_bwd_reduce into a unit that holds sums")
    old = ops.stat_from_float(torch.randn(64, 2, C, generator=_gen(3), dtype=torch.float64) * 10)
    st = old.cuda()
    ops.launch("mhe_bn_bwd_reduce_nhwc", gr.cuda(), a.cuda(), y.cuda(), mi, st, P, C, ops.F32)
    added = ops.stat_totals(st.cpu()) - ops.stat_totals(old)
    s1, s2, mag1, mag2 = rr.bn_bwd_sums(gr, a, y, mean, invstd)
    b1, b2 = _sum_bounds(mag1, mag2, L, W)
    m.add("sum g'", added[0].numpy(), s1.numpy(), b1.numpy())
    m.add("sum g' xhat", added[1].numpy(), s2.numpy(), b2.numpy())
    m.report()
    # one inf in channel 3: its partial plants the marker, finalize turns it into NaN; every other channel is untouched by it
    bad = gr.clone()
    bad[100, 3] = float("inf")
    st = ops.stat_unit(C, "cuda")
    ops.launch("mhe_bn_bwd_reduce_nhwc", bad.cuda(), None, y.cuda(), mi, st, P, C, ops.F32)
    tot = ops.stat_totals(st.cpu())
    skip = np.arange(C) == 3
    fin = torch.where(torch.isinf(bad), torch.zeros(()), bad)
    s1, s2, mag1, mag2 = rr.bn_bwd_sums(fin, None, y, mean, invstd)
    b1, b2 = _sum_bounds(mag1, mag2, L, W)
    m = M("bn_bwd_reduce beside a channel with an inf")
    m.add("sum g'", tot[0].numpy()[~skip], s1.numpy()[~skip], b1.numpy()[~skip])
    m.add("sum g' xhat", tot[1].numpy()[~skip], s2.numpy()[~skip], b2.numpy()[~skip])
    dg, db = _check_finalize(m, ("inf",), ops, st, tot, gamma, mean, invstd, P, skip=skip)
    m.report()
    assert math.isnan(float(dg[3])) and math.isnan(float(db[3])), "the channel with the inf must finalize to NaN"


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 5, 64, 67])
def test_bn_mean_invstd_against_f64_from_the_decoded_words(gpu_lib, C):
    from mhentropy_amd import ops
    g = _gen(C, "mi")
    count, eps = 4096.0, float(np.float32(1e-5))
    mu = torch.randn(64, C, generator=g, dtype=torch.float64)
    q = mu ** 2 + 1.0 + 40.0 * torch.rand(64, C, generator=g, dtype=torch.float64)
    words = ops.stat_from_float(torch.stack([mu, q], 1) * (count / 64))
    tot = ops.stat_totals(words)
    mean, invstd = rr.mean_invstd(tot[0], tot[1], count, eps)
    mi = ops.bn_mean_invstd(words.cuda(), count, 1e-5)
    m = M("bn_mean_invstd C = %d" % C)
    m.add("mean", _np(mi[0]), mean.numpy(), (U32 * mean.abs()).numpy())
    m.add("1 / std", _np(mi[1]), invstd.numpy(), (4 * U32 * invstd).numpy())
    m.report()


# ---- 2. bn_bwd_apply: narrow, wide U = 4, wide U = 1 ----------------------------------------------------------------------------------------
def _apply_kernel(P, C, dt, aligned=True):
    """the kernel mhe_bn_bwd_apply_nhwc launches, from its own shape arithmetic"""
    E = 4 if dt == F32 else 8
    nl = P * C // E
    deep = nl * 16 <= (80 << 20)
    wblocks = _ewg((nl + 3) // 4 if deep else nl)
    if C % E == 0 and (wblocks * 256) % (C // E) == 0 and aligned:
        return "wide U=4" if deep else "wide U=1"
    return "narrow"


APPLY_CASES = [
    # (dt, P, C, element offset of every tensor, the kernel it reaches)
    (F32, 100, 12, 0, "narrow"),          # 75 lane groups -> 1 block, 256 % 3 != 0
    (F32, 400, 12, 0, "narrow"),          # 2 blocks
    (BF, 100, 12, 0, "narrow"),           # C % 8 != 0
    (BF, 257, 64, 4, "narrow"),           # views 8 bytes into their allocations: 8- but not 16-byte aligned
    (F32, 1000, 64, 0, "wide U=4"), (BF, 1000, 64, 0, "wide U=4"), (F32, 336, 2048, 0, "wide U=4"),
    (F32, 700, 12, 0, "wide U=4"),        # 3 blocks, 768 % 3 == 0; 2100 lanes over a stride of 768: the U loop's last piece is ragged
    (F32, 350, 24, 0, "wide U=4"), (BF, 700, 24, 0, "wide U=4"),
    (F32, 1, 4, 0, "wide U=4"), (F32, 5, 4, 0, "wide U=4"), (F32, 255, 4, 0, "wide U=4"), (F32, 257, 4, 0, "wide U=4"),          # one block, nl = P
    (BF, 1, 8, 0, "wide U=4"), (BF, 257, 8, 0, "wide U=4"),
]


def _offset_dev(t, dt, off):
    """t on the device as a view `off` elements into its allocation"""
    if t is None:
        return None
    buf = torch.zeros(t.numel() + 8, dtype=dt, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t.to(dt))
    return v


def _check_apply(m, ops, dt, P, C, off, forms):
    gr, a, y, _, _, _ = (_bn_operands if P * C < (1 << 22) else _bn_operands.__wrapped__)(P, C, _dtn(dt))
    coef = torch.randn(3, C, generator=_gen(P, C, "coef"))
    for gate, masked in forms:
        ga = a if gate else None
        ref, mag, gp = rr.bn_bwd_apply(gr, ga, y, *coef)
        gy = _offset_dev(torch.zeros(P, C), dt, off)
        gm = _offset_dev(torch.zeros(P, C), dt, off) if masked else None
        ops.launch("mhe_bn_bwd_apply_nhwc", _offset_dev(gr, dt, off), _offset_dev(ga, dt, off), _offset_dev(y, dt, off), coef.cuda(), gy, gm, P, C,
                   ops.dtype_code(dt))
        m.add((_dtn(dt), P, C, off, gate, masked), _np(gy), ref.numpy(), (2 * U32 * mag + _ub(ref, dt)).numpy())
        if masked:
            assert np.array_equal(_np(gm), gp.numpy()), ("g [a > 0] is not exact", _dtn(dt), P, C, gate)


@pytest.mark.gpu
def test_bn_bwd_apply_every_kernel_against_f64(gpu_lib):
    from mhentropy_amd import ops
    by_kernel = {}
    for dt, P, C, off, kernel in APPLY_CASES:
        assert _apply_kernel(P, C, dt, aligned=off % 8 == 0 if dt == BF else off % 4 == 0) == kernel, (P, C, off)
        _check_apply(by_kernel.setdefault(kernel, M("bn_bwd_apply " + kernel)), ops, dt, P, C, off, [(g, w) for g in (True, False) for w in (True, False)])
    assert set(by_kernel) == {"narrow", "wide U=4"}
    for m in by_kernel.values():
        m.report()


@pytest.mark.gpu
def test_bn_bwd_apply_wide_single_piece_kernel_above_80_mb(gpu_lib):
    """f32 (327681, 64): 5,242,896 lanes of 16 bytes, just above 80 MB per tensor -> wide U = 1 with the grid capped at 8192 blocks: three trips
    of the grid-stride loop, the last one ragged"""
    from mhentropy_amd import ops
    P, C = 327681, 64
    assert _apply_kernel(P, C, F32) == "wide U=1" and (P * C // 4) * 16 > (80 << 20) >= ((P - 1) * C // 4) * 16
    m = M("bn_bwd_apply wide U=1")
    _check_apply(m, ops, F32, P, C, 0, [(True, True)])
    m.report()


# ---- 3. max pool: winners, scatter, the fused BatchNorm forms -------------------------------------------------------------------------------
POOL_HW = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (8, 8), (9, 7), (16, 8)]


@functools.lru_cache(None)
def _pool_operands(B, H, W, C, dtname):
    """dyadic operands, so that every f32 partial result of the kernels is exact and bf16 rounding is the only rounding: x = (8 a + b) / 64 in
    clusters one bf16 step apart (they tie after the affine and the rounding), scales in {+-0.5, +-1, +-2}, shifts in sixteenths, gradients in
    sixteenths; half of relu(x s + t) is zero"""
    g = _gen(B, H, W, C, dtname)
    x = (torch.randint(-31, 32, (B, H, W, C), generator=g) * 8 + torch.randint(0, 2, (B, H, W, C), generator=g)).float() / 64
    scale = torch.tensor([1.0, -1.0, 0.5, -2.0, 2.0, -0.5])[torch.arange(C) % 6]
    shift = torch.randint(-32, 33, (C,), generator=g).float() / 16
    Ho, Wo = rr.pooled_size(H, W)
    gy = torch.randint(-64, 65, (B, Ho, Wo, C), generator=g).float() / 16
    mean, invstd = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
    return x, scale, shift, gy, mean, invstd, torch.randn(3, C, generator=g)


def _walk_bounds(mag1, mag2, lanes, blocks, cpp):
    """sums of a grid-stride walk: a thread's trips, then 256 / cpp partials folded serially"""
    L = -(-lanes // (blocks * 256)) + 256 // cpp
    return _sum_bounds(mag1, mag2, L, blocks)


def _check_plain_pool(ops, x, gy, dt, what):
    B, H, W, C = x.shape
    pooled, tap = rr.maxpool_winners(x.to(dt))
    y, idx = ops.maxpool3x3s2_idx(_dev(x, dt))
    assert torch.equal(_bits(y), _bits(pooled)), (what, "pooled values")
    assert torch.equal(idx.cpu(), tap), (what, "winner taps")
    gx = ops.maxpool3x3s2_bwd(_dev(gy, dt), idx, H, W)
    want = rr.stored(rr.maxpool_bwd(gy, tap, H, W), dt)
    assert np.array_equal(_np(gx), want.numpy()), (what, "scattered gradient")
    return tap


@pytest.mark.gpu
@DTYPES
def test_maxpool_winners_and_scatter_are_exact(gpu_lib, dt):
    """plain forms: the clustered image (negative values, bf16 ties) and its ReLU (ties at zero); C = 4 and 12 as well in f32"""
    from mhentropy_amd import ops
    n = 0
    for H, W in POOL_HW:
        for B in (1, 3):
            for C in (8, 64) + ((4, 12) if dt == F32 else ()):
                x, _, _, gy, _, _, _ = _pool_operands(B, H, W, C, _dtn(dt))
                _check_plain_pool(ops, x, gy, dt, (B, H, W, C, "clustered"))
                _check_plain_pool(ops, torch.relu(x), gy, dt, (B, H, W, C, "relu"))
                n += 2
    print("reverse-edges: maxpool3x3s2_idx / _bwd %s: exact at %d cases" % (_dtn(dt), n))


@pytest.mark.gpu
@DTYPES
def test_maxpool_window_of_minus_infinity_or_below_the_old_sentinel(gpu_lib, dt):
    """found by this test: maxpool_idx_kernel started from -3.0e38 with winner tap 0, so such a window pooled to -3.0e38, its winner could name a
    pixel outside the image and maxpool_bwd_kernel dropped the gradient; it now starts from the first tap inside the image, as torch does"""
    from mhentropy_amd import ops
    g = _gen("sentinel")
    for H, W in ((1, 1), (3, 5), (8, 8)):
        gy = torch.randint(-64, 65, (2, *rr.pooled_size(H, W), 4), generator=g).float() / 16
        low = torch.where(torch.rand(2, H, W, 4, generator=g) < 0.5, -3.2e38, -3.3e38)
        for what, x in (("-inf", torch.full((2, H, W, 4), -float("inf"))), ("below -3.0e38", low)):
            tap = _check_plain_pool(ops, x, gy, dt, (H, W, what))
            hi, wi = rr.window_pixels(tap, H, W)
            assert (hi >= 0).all() and (hi < H).all() and (wi >= 0).all() and (wi < W).all()
    x = torch.zeros(1, 3, 3, 4)
    x[0, 2, 2, :], x[0, 0, 0, 0] = float("nan"), float("nan")
    y, idx = ops.maxpool3x3s2_idx(_dev(x, dt))
    print("reverse-edges: maxpool3x3s2_idx %s with NaN at (0,0) ch 0 and (2,2): pooled ch 0 %s taps %s; ch 1 %s taps %s" % (
        _dtn(dt), y[0, :, :, 0].flatten().tolist(), idx[0, :, :, 0].flatten().tolist(), y[0, :, :, 1].flatten().tolist(), idx[0, :, :, 1].flatten().tolist()))


def _check_fused_pool(ms, ops, B, H, W, C, dt, kernels=("idx", "win", "bwd", "pooled")):
    """the fused forms at one shape; ms = (sums, apply) measures"""
    x, scale, shift, gy, mean, invstd, coef = _pool_operands(B, H, W, C, _dtn(dt))
    E = 4 if dt == F32 else 8
    cpp, case = C // E, (B, H, W, C)
    act = rr.affine_relu(x, scale, shift, dt)
    pooled, tap = rr.maxpool_winners(act.float())          # (exact: the stored values are f32 values)
    pooled, xw = pooled.double(), rr.gather_winners(x, tap)
    xd, sc, sh, gyd = _dev(x, dt), scale.cuda(), shift.cuda(), _dev(gy, dt)
    mi = torch.stack([mean, invstd]).cuda()
    if "idx" in kernels:
        y, idx = ops.maxpool3x3s2_idx(xd, sc, sh)
        assert np.array_equal(_np(y), pooled.numpy()) and torch.equal(idx.cpu(), tap), (case, "affine pool")
    if "win" in kernels:
        y, idx, xwin = ops.maxpool3x3s2_idx_win(xd, sc, sh)
        assert np.array_equal(_np(y), pooled.numpy()) and torch.equal(idx.cpu(), tap), (case, "affine pool with winners' inputs")
        assert np.array_equal(_np(xwin), xw.double().numpy()), (case, "xwin")
    idx = tap.cuda()
    if "bwd" in kernels:
        gx_ref = torch.where(act > 0, rr.stored(rr.maxpool_bwd(gy, tap, H, W), dt), torch.zeros((), dtype=torch.float64))
        s1, s2, mag1, mag2 = rr.bn_bwd_sums(gx_ref, None, x, mean, invstd)
        lanes = B * H * W * cpp
        b1, b2 = _walk_bounds(mag1, mag2, lanes, _ewg(lanes), cpp)
        for want_gx in (True, False):
            st = ops.stat_unit(C, "cuda")
            gx = ops.maxpool3x3s2_bwd_bn(gyd, idx, xd, sc, sh, mi, st, want_gx=want_gx)
            if want_gx:
                assert np.array_equal(_np(gx), gx_ref.numpy()), (case, "scattered, gated gradient")
            tot = ops.stat_totals(st.cpu())
            ms[0].add(case + ("bwd_bn", want_gx, "sum g'"), tot[0].numpy(), s1.numpy(), b1.numpy())
            ms[0].add(case + ("bwd_bn", want_gx, "sum g' xhat"), tot[1].numpy(), s2.numpy(), b2.numpy())
        ref, mag, _ = rr.bn_bwd_apply(gx_ref, None, x, *coef)
        out = ops.maxpool3x3s2_bwd_bn_apply(gyd, idx, xd, sc, sh, mi, coef.cuda())
        ms[1].add(case, _np(out), ref.numpy(), (2 * U32 * mag + _ub(ref, dt)).numpy())
    if "pooled" in kernels:
        s1, s2, mag1, mag2 = rr.bn_bwd_sums(gy, pooled, xw, mean, invstd)
        nl = pooled.numel() // E
        blocks = min(_ewg((nl + 1) // 2), 2048)
        b1, b2 = _walk_bounds(mag1, mag2, nl, blocks, cpp)
        st = ops.stat_unit(C, "cuda")
        ops.pooled_bn_sums(gyd, _dev(pooled.float(), dt), _dev(xw, dt), mi, st)
        tot = ops.stat_totals(st.cpu())
        ms[0].add(case + ("pooled_bn_sums", "sum g'"), tot[0].numpy(), s1.numpy(), b1.numpy())
        ms[0].add(case + ("pooled_bn_sums", "sum g' xhat"), tot[1].numpy(), s2.numpy(), b2.numpy())


@pytest.mark.gpu
@DTYPES
def test_fused_pool_forms_against_f64(gpu_lib, dt):
    """winners, pooled values, xwin and the gated scatter exact; the sums of all three walks and the apply form within their bounds; (8, 8) and
    (16, 8) at C = 64 take maxpool_bwd_bn_kernel's shift path, everything else its division path; negative scales on a third of the channels"""
    from mhentropy_amd import ops
    ms = (M("maxpool_bwd_bn / pooled_bn_sums sums " + _dtn(dt)), M("maxpool_bwd_bn apply " + _dtn(dt)))
    for H, W in POOL_HW:
        for B in (1, 3):
            for C in (8, 64):
                _check_fused_pool(ms, ops, B, H, W, C, dt)
    ms[0].report()
    ms[1].report()


@pytest.mark.gpu
def test_pool_kernels_above_the_grid_cap(gpu_lib):
    """f32, C = 8, 3 x 5 images: 174,800 of them put every pooled-size walk (plain and affine winners, pooled_bn_sums) past 8192 blocks,
    70,000 every full-size walk (scatter and the three maxpool_bwd_bn forms)"""
    from mhentropy_amd import ops
    ms = (M("pool sums above the cap"), M("maxpool_bwd_bn apply above the cap"))
    Bp, Bf = 174800, 70000
    assert Bp * 6 * 2 > EW_CAP and Bf * 15 * 2 > EW_CAP > Bf * 6 * 2
    _check_fused_pool(ms, ops, Bp, 3, 5, 8, F32, kernels=("idx", "win", "pooled"))
    x, _, _, gy, _, _, _ = _pool_operands(Bp, 3, 5, 8, "f32")
    pooled, tap = rr.maxpool_winners(x)
    y, idx = ops.maxpool3x3s2_idx(x.cuda())
    assert torch.equal(y.cpu(), pooled) and torch.equal(idx.cpu(), tap)
    _check_fused_pool(ms, ops, Bf, 3, 5, 8, F32, kernels=("bwd",))
    x, _, _, gy, _, _, _ = _pool_operands(Bf, 3, 5, 8, "f32")
    _check_plain_pool(ops, x, gy, F32, "plain scatter above the cap")
    _pool_operands.cache_clear()
    ms[0].report()
    ms[1].report()


# ---- 4. average pool and stride-2 reverse ---------------------------------------------------------------------------------------------------
def _check_avgpool_bwd(m, ops, B, HW, C, dt, masked):
    g = _gen(B, HW, C, _dtn(dt), masked)
    gf = torch.randn(B, C, generator=g)
    mask = _plant_gate(torch.relu(torch.randn(B, HW, C, generator=g)).to(dt).float(), dt) if masked else None
    ref = rr.avgpool_bwd(gf, HW, mask)
    gx = ops.avgpool_bwd(gf.cuda(), HW, dt, mask=_dev(mask, dt))
    m.add((B, HW, C, masked), _np(gx), ref.numpy(), (2 * U32 * ref.abs() + _ub(ref, dt)).numpy())
    if masked:
        assert not _np(gx)[(mask <= 0).numpy()].any(), "closed gates must give 0"


@pytest.mark.gpu
@DTYPES
def test_avgpool_bwd_against_f64(gpu_lib, dt):
    from mhentropy_amd import ops
    m = M("avgpool_bwd " + _dtn(dt))
    for HW in (1, 49, 64):
        for C in (4, 12, 2048):
            for B in (1, 3):
                for masked in (False, True):
                    _check_avgpool_bwd(m, ops, B, HW, C, dt, masked)
    if dt == F32:
        assert 65 * 64 * 2048 // 4 > EW_CAP          # one case above the 8192-block cap
        _check_avgpool_bwd(m, ops, 65, 64, 2048, dt, True)
    m.report()


@pytest.mark.gpu
@DTYPES
def test_upsample2_against_f64(gpu_lib, dt):
    """without base: value-equal (the kernel forms 0 + g, so a -0.0 gradient comes out as +0.0); with base one rounded sum"""
    from mhentropy_amd import ops
    m = M("upsample2 with base " + _dtn(dt))
    for H, W in ((1, 1), (2, 2), (3, 3), (5, 4), (8, 8)):
        for C in (4, 12):
            g = _gen(H, W, C, _dtn(dt))
            gs = torch.randn(2, (H + 1) // 2, (W + 1) // 2, C, generator=g).to(dt).float()
            gs.view(-1)[0] = -0.0
            base = torch.randn(2, H, W, C, generator=g).to(dt).float()
            out = ops.upsample2(_dev(gs, dt), H, W)
            assert np.array_equal(_np(out), rr.upsample2(gs, H, W)[0].numpy()), (H, W, C)
            ref, mag = rr.upsample2(gs, H, W, base)
            m.add((H, W, C), _np(ops.upsample2(_dev(gs, dt), H, W, base=_dev(base, dt))), ref.numpy(), (U32 * mag + _ub(ref, dt)).numpy())
    m.report()


# ---- 5. gradient norm, clip + Adam ----------------------------------------------------------------------------------------------------------
SQ_S = 262144          # float4 lanes of one sqnorm_partial_kernel trip (1024 blocks x 256)


@pytest.mark.gpu
def test_sqnorm_against_f64_and_bit_reproducible(gpu_lib):
    """n < 4 and n % 4 != 0 (the tail of block 0), the second in-flight load present and absent, the second trip"""
    from mhentropy_amd import ops
    m = M("sqnorm")
    for n in (1, 2, 3, 4, 5, 7, 1023, SQ_S * 4 - 1, SQ_S * 4 + 4, 2 * SQ_S * 4 + 5):
        gr = torch.randn(n, generator=_gen(n, "sq"))
        L = 4 * -(-(n // 4) // SQ_S) + (1 if n % 4 else 0)
        o1, o2 = torch.zeros(1, device="cuda"), torch.full((1,), 7.0, device="cuda")
        gd = gr.cuda()
        ops.sqnorm(gd, o1)
        ops.sqnorm(gd, o2)
        assert torch.equal(_bits(o1), _bits(o2)), (n, "two calls differ")
        ref = rr.sqnorm(gr)
        m.add(n, _np(o1), np.array([ref]), (L + 22) * U32 * ref)
    m.report()


def _adam_f32(p, g, m, v, t, sq, lr, b1, b2, eps, max_norm, gs):
    """the kernel's formula in plain float32 torch on the CPU (for the transcendental margin only)"""
    f = lambda x: torch.tensor(x, dtype=F32)
    tt = f(float(t))
    bc1, bc2s = 1 - torch.pow(f(b1), tt), torch.sqrt(1 - torch.pow(f(b2), tt))
    coef = f(gs)
    if max_norm > 0:
        cc = f(max_norm) / (torch.sqrt(f(sq)) * f(gs) + f(1e-6))
        coef = coef * torch.minimum(cc, f(1.0))
    gg = g * coef
    mm = f(b1) * m + (1 - f(b1)) * gg
    vv = f(b2) * v + (1 - f(b2)) * gg * gg
    return p - (f(lr) / bc1) * mm / (torch.sqrt(vv) / bc2s + f(eps)), mm, vv


ADAM = dict(lr=float(np.float32(2e-4)), b1=float(np.float32(0.9)), b2=float(np.float32(0.999)), eps=float(np.float32(1e-8)))
ADAM_CASES = [(n, mode) for n in (1, 255, 257) for mode in ("clip", "no-clip-needed", "max_norm=0", "grad_scale", "step-100000")] + \
             [(EW_CAP + 3, "clip"), (EW_CAP + 3, "step-100000")]


@pytest.mark.gpu
def test_train_tick_and_adam_step_against_f64(gpu_lib):
    """three steps advanced by train_tick (and one from a counter preset so that the tick makes it 100000, where b^t underflows); each step's reference starts from the
    state the kernel left, so every step is checked against its own one-step bound.  Element 0 has g = m = v = 0: p[0] keeps its bits"""
    from mhentropy_amd import ops
    m, ratios, rows = M("adam_step"), [], []
    for n, mode in ADAM_CASES:
        g = _gen(n, mode)
        scale = 1e-4 if mode == "no-clip-needed" else 3.0
        max_norm, gs = (0.0 if mode == "max_norm=0" else 1.0), (0.5 if mode == "grad_scale" else 1.0)
        p0 = torch.randn(n, generator=g)
        P, Mo, V = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        step, sq = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((1,), 5.0, device="cuda")
        if mode == "step-100000":
            step.fill_(100000 - 1)
            Mo, V = (torch.randn(n, generator=g) * 0.1).cuda(), (torch.rand(n, generator=g) * 0.1).cuda()
            Mo[0], V[0] = 0.0, 0.0
        for k in range(1 if mode == "step-100000" or n > 1000 else 3):
            gr = torch.randn(n, generator=g) * scale
            gr[0] = 0.0
            before = (P.cpu(), Mo.cpu(), V.cpu())
            ops.train_tick(step, sq)
            assert float(sq) == 0.0, "train_tick must clear the squared norm"
            G = gr.cuda()
            ops.sqnorm(G, sq)
            t = int(step)
            assert t == (100000 if mode == "step-100000" else k + 1)
            ops.adam_step(P, G, Mo, V, sq if max_norm > 0 else None, step, 2e-4, max_norm=max_norm, grad_scale=gs)
            sqv = float(sq) if max_norm > 0 else None
            if mode == "clip":
                assert sqv ** 0.5 * gs > 1.0 or n == 1
            rows.append(((n, mode, t), before, gr, t, sqv, max_norm, gs, (P.cpu(), Mo.cpu(), V.cpu())))
            assert torch.equal(_bits(P[:1]), _bits(p0[:1])), (n, mode, "g = m = v = 0 must leave p unchanged")
    # the transcendental margin: float32 torch on the CPU against the f64 reference, in units of the model bound
    for case, (p, mo, v), gr, t, sqv, max_norm, gs, _ in rows:
        r = rr.clip_adam(p, gr, mo, v, t, sqv, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], max_norm, gs, tiny=float(np.float32(1e-6)))
        for got, key, b in zip(_adam_f32(p, gr, mo, v, t, sqv, 2e-4, 0.9, 0.999, 1e-8, max_norm, gs), ("p", "m", "v"), ("bp", "bm", "bv")):
            diff = (got.double() - r[key]).abs()
            ratios.append(float(torch.where(diff == 0, torch.zeros(()).double(), diff / r[b]).max()))
    factor = max(1, math.ceil(2 * max(ratios)))
    print("reverse-edges: adam_step: float32 torch on the CPU is within %.3f of the model bound -> factor %d" % (max(ratios), factor))
    for case, (p, mo, v), gr, t, sqv, max_norm, gs, (p2, m2, v2) in rows:
        r = rr.clip_adam(p, gr, mo, v, t, sqv, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], max_norm, gs, tiny=float(np.float32(1e-6)))
        m.add(case + ("m",), _np(m2), r["m"].numpy(), r["bm"].numpy())
        m.add(case + ("v",), _np(v2), r["v"].numpy(), r["bv"].numpy())
        m.add(case + ("p",), _np(p2), r["p"].numpy(), factor * r["bp"].numpy())
    m.report()


# ---- 6. RealNVP element-wise stages ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_flow_mask_pad_against_f64(gpu_lib):
    from mhentropy_amd import ops
    m = M("mask_pad")
    for R in (1, 3, 65):
        for dim in (1, 45, 64):
            g = _gen(R, dim, "mp")
            x, mask = torch.randn(R, dim, generator=g), torch.where(torch.arange(dim) % 2 == 0, torch.rand(dim, generator=g) + 0.5, torch.zeros(()))
            ref = rr.mask_pad(x, mask)
            xd, md = x.cuda(), mask.cuda()
            outs = {"f32 entry": (ops.flow_mask_pad(xd, md, torch.full((R, 64), 9.0, device="cuda")), None)}
            for form in ("f32", "bf16", "both"):
                of = torch.full((R, 64), 9.0, device="cuda") if form != "bf16" else None
                ob = torch.full((R, 64), 9.0, device="cuda", dtype=BF) if form != "f32" else None
                ops.flow_mask_pad_mixed(xd, md, out_f32=of, out_bf16=ob)
                outs[form] = (of, ob)
            for form, (of, ob) in outs.items():
                for o, dt in ((of, F32), (ob, BF)):
                    if o is not None:
                        m.add((R, dim, form, _dtn(dt)), _np(o), ref.numpy(), (U32 * ref.abs() + _ub(ref, dt)).numpy())
                        assert not _bits(o[:, dim:]).any(), "padding columns must be +0"
    m.report()


def _cond_operands(N, B, H, dt, seed):
    g = _gen(N, B, H, seed)
    pre = torch.randn(N * B, H, generator=g).to(dt).float()
    wide = torch.randn(B, H + 8, generator=g)
    return pre, wide


@pytest.mark.gpu
def test_flow_cond_lrelu_against_f64(gpu_lib):
    """in place and the mixed forms; the conditioning rows are a column slice of a wider matrix (cond_stride = H + 8 > H)"""
    from mhentropy_amd import ops
    m = M("cond_lrelu")
    for N, B in ((1, 1), (4, 3), (5, 2)):
        for H in (4, 64, 512):
            for dt in (F32, BF):
                pre, wide = _cond_operands(N, B, H, dt, "cl")
                ref, mag = rr.cond_lrelu(pre, wide[:, 4:4 + H], B, SLOPE)
                wd = wide.cuda()
                cond = wd[:, 4:4 + H]
                bound = lambda o: (2 * U32 * mag + _ub(ref, o)).numpy()
                if dt == F32:
                    Pd = pre.cuda()
                    ops.flow_cond_lrelu(Pd, cond, H + 8, B)
                    m.add((N, B, H, "in place"), _np(Pd), ref.numpy(), bound(F32))
                for form in ("f32", "bf16", "both"):
                    of = torch.zeros(N * B, H, device="cuda") if form != "bf16" else None
                    ob = torch.zeros(N * B, H, device="cuda", dtype=BF) if form != "f32" else None
                    ops.flow_cond_lrelu_mixed(_dev(pre, dt), cond, H + 8, B, out_f32=of, out_bf16=ob)
                    for o, odt in ((of, F32), (ob, BF)):
                        if o is not None:
                            m.add((N, B, H, "from " + _dtn(dt), form, _dtn(odt)), _np(o), ref.numpy(), bound(odt))
                assert torch.equal(wd.cpu(), wide), "the conditioning matrix was written"
    m.report()


@pytest.mark.gpu
@pytest.mark.parametrize("slope", [0.01, 0.0])
def test_flow_lrelu_bwd_against_f64(gpu_lib, slope):
    from mhentropy_amd import ops
    m = M("lrelu_bwd slope %g" % slope)
    s64 = float(np.float32(slope))
    for n in (4, 260, 3 * 512):
        for gdt in (F32, BF):
            for hdt in (F32, BF):
                g = _gen(n, _dtn(gdt), _dtn(hdt))
                gr = torch.randn(n, generator=g).to(gdt).float()
                h = _plant_gate(torch.randn(n, generator=g).to(hdt).float(), hdt)
                ref = rr.lrelu_bwd(gr, h, s64)
                of, ob = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda", dtype=BF)
                ops.flow_lrelu_bwd_mixed(_dev(gr, gdt), _dev(h, hdt), out_f32=of, out_bf16=ob, slope=slope)
                m.add((n, _dtn(gdt), _dtn(hdt), "f32"), _np(of), ref.numpy(), (U32 * ref.abs()).numpy())
                m.add((n, _dtn(gdt), _dtn(hdt), "bf16"), _np(ob), ref.numpy(), (U32 * ref.abs() + UB * ref.abs()).numpy())
                assert np.array_equal(_np(of)[(h > 0).numpy()], gr.double().numpy()[(h > 0).numpy()]), "open gates pass g unchanged"
                if gdt == F32 and hdt == F32:
                    G = gr.cuda()
                    ops.flow_lrelu_bwd(G, h.cuda(), slope=slope)
                    m.add((n, "in place"), _np(G), ref.numpy(), (U32 * ref.abs()).numpy())
    m.report()


@pytest.mark.gpu
def test_flow_elementwise_kernels_above_the_grid_cap(gpu_lib):
    """R = 4 x 8193 rows of 512: 4,194,816 vectors of 4, past the 16384-block cap; cond_lrelu in place, lrelu_bwd_mixed bf16 x bf16 -> bf16"""
    from mhentropy_amd import ops
    N, B, H = 4, 8193, 512
    assert N * B * H // 4 > FLOW_CAP
    pre, wide = _cond_operands(N, B, H, F32, "cap")
    ref, mag = rr.cond_lrelu(pre, wide[:, 4:4 + H], B, SLOPE)
    Pd = pre.cuda()
    ops.flow_cond_lrelu(Pd, wide.cuda()[:, 4:4 + H], H + 8, B)
    m = M("cond_lrelu / lrelu_bwd above the cap")
    m.add("cond_lrelu", _np(Pd), ref.numpy(), (2 * U32 * mag).numpy())
    gr, h = pre.to(BF).float(), wide[:, :H].repeat(N, 1).to(BF).float()
    ref = rr.lrelu_bwd(gr, h, SLOPE)
    ob = torch.zeros(N * B, H, device="cuda", dtype=BF)
    ops.flow_lrelu_bwd_mixed(_dev(gr, BF), _dev(h, BF), out_bf16=ob, slope=0.01)
    m.add("lrelu_bwd_mixed", _np(ob), ref.numpy(), ((U32 + UB) * ref.abs()).numpy())
    m.report()


@pytest.mark.gpu
def test_add_against_f64(gpu_lib):
    from mhentropy_amd import ops
    m = M("add")
    for n in (1, 257, 100003):
        g = _gen(n, "add")
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        out = ops.add(a.cuda(), b.cuda(), out=torch.zeros(n, device="cuda"))
        m.add(n, _np(out), (a.double() + b.double()).numpy(), (U32 * (a.double().abs() + b.double().abs())).numpy())
    m.report()


# ---- 7. the coupling's reverse --------------------------------------------------------------------------------------------------------------
COUPLE_RB = [(1, 1), (3, 3), (63, 9), (64, 16), (65, 5), (130, 13)]
COUPLE_FORMS = [(False, False, False), (True, False, False), (True, True, True), (False, True, True)]          # g_logp, bf16 copies, db_s / db_t
QW = -0.75


@functools.lru_cache(None)
def _couple_operands(R, B, dim):
    g = _gen(R, B, dim, "cp")
    mask = (torch.arange(dim) % 2).float() if dim > 1 else torch.zeros(1)
    Os = torch.rand(R, 64, generator=g) * 8 - 4          # |Os| <= 4: 1 - tanh^2 >= 1.3e-3, e^s in [1 / e, e]
    Os.view(-1)[:3] = torch.tensor([4.0, -4.0, 0.0])
    return (torch.randn(R, dim, generator=g), Os, torch.randn(R, 64, generator=g), mask, torch.randn(R, dim, generator=g), torch.randn(B, generator=g),
            torch.randn(64, generator=g), torch.randn(64, generator=g))


def _couple_f32(x_out, Os, Ot, mask, g_out, g_logp, B):
    """the kernel's formula in plain float32 torch on the CPU (for the transcendental margin only)"""
    R, dim = x_out.shape
    s, t = torch.tanh(Os[:, :dim]), Ot[:, :dim]
    es = torch.exp(s)
    xi = (x_out - t) / es
    a_q = torch.zeros(R, 1) if g_logp is None else (g_logp[torch.arange(R) % B] * torch.tensor(QW))[:, None]
    on = (mask == 0).expand(R, dim)
    gos = (g_out * xi * es - a_q) * (1 - s * s)
    return {"x_in": torch.where(on, xi, x_out), "GOs": torch.where(on, gos, torch.zeros(())), "g_part": torch.where(on, g_out * es, g_out)}


@pytest.mark.gpu
def test_flow_couple_bwd_against_f64(gpu_lib):
    """R around the 64 rows of a workgroup (the `r >= R` break ahead of the LDS fold), dim < 64 padding columns, with and without the adjoint
    of log q, the bf16 copies and the bias-gradient accumulators (preset, to show they accumulate)"""
    from mhentropy_amd import ops
    cases = [(R, B, dim) + f for R, B in COUPLE_RB for dim in (45, 64, 1) for f in COUPLE_FORMS]
    ratios = []
    for R, B, dim, lp, _, _ in cases:
        x_out, Os, Ot, mask, g_out, g_logp, _, _ = _couple_operands(R, B, dim)
        r = rr.couple_bwd(x_out, Os, Ot, mask, g_out, g_logp if lp else None, QW, B)
        f = _couple_f32(x_out, Os, Ot, mask, g_out, g_logp if lp else None, B)
        for k in ("x_in", "GOs", "g_part"):
            diff, ref = f[k].double(), r[k][:, :dim]
            diff = (diff - ref).abs()
            ratios.append(float(torch.where(diff == 0, torch.zeros(()).double(), diff / r["b_" + k][:, :dim]).max()))
    factor = max(1, math.ceil(2 * max(ratios)))
    print("reverse-edges: couple_bwd: float32 torch on the CPU is within %.3f of the model bound -> factor %d" % (max(ratios), factor))
    m, md = M("couple_bwd"), M("couple_bwd db_s / db_t")
    for R, B, dim, lp, bf, db in cases:
        x_out, Os, Ot, mask, g_out, g_logp, db_s0, db_t0 = _couple_operands(R, B, dim)
        r = rr.couple_bwd(x_out, Os, Ot, mask, g_out, g_logp if lp else None, QW, B)
        new = lambda *s, dt=F32: torch.full(s, 9.0, device="cuda", dtype=dt)
        x_in, GOs, GOt, g_part = new(R, dim), new(R, 64), new(R, 64), new(R, dim)
        GOs_b, GOt_b = (new(R, 64, dt=BF), new(R, 64, dt=BF)) if bf else (None, None)
        db_s, db_t = (db_s0.cuda(), db_t0.cuda()) if db else (None, None)
        args = (x_out.cuda(), Os.cuda(), Ot.cuda(), mask.cuda(), g_out.cuda(), g_logp.cuda() if lp else None, QW)
        if not bf and not db:
            ops.launch("mhe_flow_couple_bwd_f32", *args, x_in, GOs, GOt, g_part, R, B, dim)
        elif R <= 64:
            ops.flow_couple_bwd(*args, B, x_in, GOs, GOt, g_part, GOs_b, GOt_b, db_s, db_t)
        else:          # (the wrapper takes the column sums of more than one workgroup in a fixed order instead: the kernel's own atomics here)
            ops.launch("mhe_flow_couple_bwd_mixed", *args, x_in, GOs, GOt, g_part, GOs_b, GOt_b, db_s, db_t, R, B, dim)
        case = (R, B, dim, lp, bf, db)
        m.add(case + ("x_in",), _np(x_in), r["x_in"].numpy(), factor * r["b_x_in"].numpy())
        m.add(case + ("GOs",), _np(GOs), r["GOs"].numpy(), factor * r["b_GOs"].numpy())
        m.add(case + ("g_part",), _np(g_part), r["g_part"].numpy(), factor * r["b_g_part"].numpy())
        assert np.array_equal(_np(GOt), r["GOt"].numpy()), (case, "GOt is a masked copy")
        assert not _bits(GOs[:, dim:]).any() and not _bits(GOt[:, dim:]).any(), (case, "padding columns must be +0")
        if bf:
            assert torch.equal(_bits(GOs_b), _bits(GOs.to(BF))) and torch.equal(_bits(GOt_b), _bits(GOt.to(BF))), (case, "bf16 copies")
        if db:
            chain = 19 + (R + 63) // 64          # 16 rows per thread, 3 adds of the fold, one atomic add per workgroup
            for got, old, rows in ((db_s, db_s0, GOs), (db_t, db_t0, GOt)):
                rows = rows.cpu().double()
                md.add(case, _np(got), (old.double() + rows.sum(0)).numpy(), (chain * U32 * (old.double().abs() + rows.abs().sum(0))).numpy())
    m.report()
    md.report()


@pytest.mark.gpu
def test_flow_couple_accum_against_f64(gpu_lib):
    from mhentropy_amd import ops
    m = M("couple_accum")
    for R, _ in COUPLE_RB:
        for dim in (45, 64, 1):
            g = _gen(R, dim, "ca")
            gp, GXs, GXt = torch.randn(R, dim, generator=g), torch.randn(R, 64, generator=g), torch.randn(R, 64, generator=g)
            mask = (torch.arange(dim) % 2).float() * (torch.rand(dim, generator=g) + 0.5)
            ref, mag = rr.couple_accum(gp, GXs, GXt, mask)
            out = ops.flow_couple_accum(gp.cuda(), GXs.cuda(), GXt.cuda(), mask.cuda(), torch.zeros(R, dim, device="cuda"))
            m.add((R, dim), _np(out), ref.numpy(), (3 * U32 * mag).numpy())
    m.report()
