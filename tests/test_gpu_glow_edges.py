"""The conditional Glow's staged kernels (csrc/glow.hip) and the dense layer they run on (mhe_linear_f32 and its skinny forms, csrc/conv.hip),
each against the float64 references of tests/glow_stage_ref.py at the edges it has: grid-stride loops above their 16384-block cap, the image
index (r / row_div) % n_img with gate / image tables that are column-offset views of a wider table, the one-wave-per-row kernels at every
pitch boundary with T below its maximum and rows behind R, image_rows_bwd_kernel from C = 4 (512 row lanes) to C = 2048 (one, no fold), and
all three row-tile instantiations of skinny_linear_kernel with the row-split grid and the 128 x 128 fallback.

Operands are rounded to the storage type on the CPU; every expected value is float64 on the CPU from those rounded operands.  Every output
is pre-filled with NaN (an unwritten cell fails) and followed by two guard rows that must keep their bits; padding columns of the inputs hold
NaN (the kernels must not use them), padding columns of the outputs must be +0.

Bounds (u32 = 2^-24, ub = 2^-8; none is tuned, the measured max(|diff| / bound) is printed before it is asserted, `pytest -s`).  They are
the first-order error of a float32 evaluation in the kernel's operation order, carried along by glow_stage_ref.V: every operation u32 of its
result (+ 2^-126: a result below the smallest normal may come out as zero), expf / logf 2 u32 of theirs:
  add_image_rows    u32 |H + img|
  relu_copy         exact (the sign of a zero is not defined: fmaxf(-0, +0)); bf16 = the rounding of the exact value
  glu_residual      H + T / (1 + expf(-g)): expf, sum, division, sum
  glu_bwd           s = 1 / (1 + expf(-g)); g_t3 = g_h s (bf16: + ub |ref|); g_gate = ((g_h t3) s) (1 - s)
  relu_bwd_add      exact on dyadic inputs; the gate [h > 0] at +0, -0, -1 and the smallest subnormal as float64 says
  coupling          scale = 1 / (1 + expf(-(us + 2))) + 1e-3f; y = u scale + shift or (u - shift) / scale; logdet: logf per feature, a chain of
                    ld / 64 + 6 additions (a lane's columns, the wave's butterfly), one sum onto the seed; identity columns bit-exact,
                    padding +0; inverse(forward(u)) against u with the forward's bound carried through the inverse's
  coupling_inv_bwd, g_v = g_y / scale; g_us = ((-g_v (v - shift) / scale + a_q / scale) sig) (1 - sig), a_q = g_log_p[r % B] q_weight one product
  _wide, _fwd_bwd   (narrow) or given per row; fwd: g_v = g_y scale, g_us = ((g_y v + a_p / scale) sig) (1 - sig); identity columns and d shift of
                    the forward form exact, padding and the columns from 2 T on +0
  base_density_bwd  g_z - a_p z: product, sum
  pad64             exact
  finish            |z|^2: (ld / 64 + 6) u32 sum z^2; the constant: one sum per part; then product, sums; v_out bit-exact; finish_f32 bit-equal
                    to finish_dev with one part p and the host constant sign p (the kernel forms 0 + sign p)
  glu_bwd_sum       g_t3 as glu_bwd (bf16); sums: L u32 sum |term|, L = 4 trips + nl (four rows in flight per trip of a row lane, nl lanes
                    folded serially), then s (1 - s) or s; two calls bit-equal
  mask_scale_sum    g' = bf16(g scale [t2 > 0]): u32 |ref| + ub |ref|; bsum = the sum of the values as stored: L u32 sum |stored|
  linear            (K / 4 + 6) u32 (sum |x w| + |b|): per wave K / 16 instructions of four products, three LDS adds, the bias, slack; the
                    skinny entry bit-equal to mhe_linear_f32 where it dispatches there; the bf16 copy = the rounding of the f32 output
  transcendentals   the model times max(1, ceil(2 r)), r = the error of a plain float32 torch evaluation of the same formula on the CPU
                    (glow_stage_ref.plain_float32) against float64, in units of the model bound, over the test's own inputs.

Tried once against deliberately edited kernels, each of which fails here: `% n_img` dropped from glu_residual_kernel (the (3, 12) one-image
case: 1.3e7 bounds), `j <= T` for `j < T` in coupling_kernel (NaN: the guard column reads the parameters' padding), the LDS fold of
image_rows_bwd_kernel started at l = 2 (gct / bsum of glu_bwd_sum, bsum of mask_scale_sum).  Clamping m to M instead of M - 1 in
skinny_linear_kernel changes no output: the lanes past M only feed result columns that are never stored, so no value test can see it.

Measured on an MI355X (r -> factor; max(|diff| / bound), each over all cases of its kernel):
  add_image_rows 1.000 (a half-ulp tie), above the cap 1.000;  relu_copy, relu_bwd_add, pad64, v_out, the bf16 copy: exact
  glu_residual T f32 r = 0.940 -> 2, 0.470;  T bf16 r = 0.963 -> 2, 0.482;  above the cap r = 0.997 -> 2, 0.498
  glu_bwd f32 r = 0.683 -> 2, 0.342;  bf16 r = 0.740 -> 2, 0.986 (the bf16 store);  above the cap r = 0.461 -> 1, 0.996
  coupling r = 0.880 -> 2, 0.436;  inverse(forward(u)) 0.434
  coupling_inv_bwd r = 0.655 -> 2, 0.328;  _wide r = 0.717 -> 2, 0.358;  coupling_fwd_bwd r = 0.711 -> 2, 0.355
  base_density_bwd 0.952;  finish 0.313
  glu_bwd_sum g_t3 r = 0.762 -> 2, 0.996 (the bf16 store);  gct / bsum r = 0.679 -> 2, 0.340
  mask_scale_sum g' 0.000 (bit-equal to the reference's two roundings), bsum 0.005
  linear skinny<4> 0.102, <8> 0.104, <16> 0.105, <4> rows split 0.073, tiled 0.116;  linear_f32_bf16copy 0.041, rows split 0.080
"""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch

import glow_stage_ref as gr
from edge_measure import Measure

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U32, UB = 2.0 ** -24, 2.0 ** -8
NAN, SENT = float("nan"), 7.25
CAP = 16384 * 256                                      # quads one launch covers in its first trip: gg() of glow.hip
CAP_R = CAP + 3                                        # rows of C = 4 above it: one quad per row, three in the ragged second trip
GATES = [0.0, 1.0, -1.0, 30.0, -30.0, 104.0, -104.0]   # expf(104) = inf in float32
US = [-120.0, -2.0, 0.0, 40.0]                         # scale -> 1e-3, sig = 1 / 2, ..., sig = 1
DTYPES = pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])


def _dtn(dt):
    return "bf16" if dt == BF else "f32"


def _np(t):
    return t.detach().cpu().double().numpy()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _rn(g, *shape, dt=F32):
    """normal values as the storage type dt holds them, as float32"""
    return torch.randn(*shape, generator=g).to(dt).float()


def _dev(t, dt=F32):
    return None if t is None else t.to(dt).cuda()


def _plant(a, vals, roll=0):
    flat = a.view(-1)
    vals = (vals[roll % len(vals):] + vals[:roll % len(vals)])[:flat.numel()]
    flat[:len(vals)] = torch.tensor(vals)
    return a


def _plant_h(a, dt):
    """+0, -0, a negative value and the smallest positive subnormal of dt at the front"""
    return _plant(a, [0.0, -0.0, -1.0, 2.0 ** -149 if dt == F32 else 2.0 ** -133])


class Out:
    """a device tensor of `shape` pre-filled with `fill` (NaN, or the values of an in-place operand), followed by two guard rows"""

    def __init__(self, shape, dt=F32, fill=NAN):
        self.rows = shape[0]
        self.buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), SENT, dtype=dt, device="cuda")
        self.t = self.buf[:shape[0]]
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.to(dt))
        else:
            self.t.fill_(fill)

    def check(self, what):
        assert torch.equal(_bits(self.buf[self.rows:]), _bits(torch.full_like(self.buf[self.rows:], SENT).cpu())), (what, "rows behind R were written")
        return self.t


class Table:
    """[n, C] values as a column-offset view (stride 3 C + 8, offset C + 4) of a wider table; the other columns hold a sentinel that must stay"""

    def __init__(self, n, Cc, values=None, around=NAN):
        self.stride, self.off, self.C, self.around = 3 * Cc + 8, Cc + 4, Cc, around
        self.wide = torch.full((n, self.stride), around, device="cuda")
        self.inner = self.wide[:, self.off:self.off + Cc]
        self.inner.copy_(values) if values is not None else self.inner.fill_(NAN)
        self.view = self.wide[:, self.off:]          # what a caller passes: ctab[:, slot * H:]

    def check(self, what):
        w = self.wide.clone()
        w[:, self.off:self.off + self.C] = self.around
        assert torch.equal(_bits(w), _bits(torch.full_like(w, self.around))), (what, "columns beside the view were written")
        return self.inner


class Rows:
    """the cases of one kernel: the margin for expf / logf from the plain float32 evaluations, then Measure"""

    def __init__(self, kernel):
        self.kernel, self.rows, self.r = kernel, [], None

    def add(self, case, got, ref, f32=None, extra=0.0):
        v, e = ref.v.numpy(), ref.e.numpy()
        if f32 is not None:
            diff = np.abs(f32.v.double().numpy() - v)
            with np.errstate(divide="ignore", invalid="ignore"):
                self.r = max(self.r or 0.0, float(np.where(diff == 0, 0.0, diff / e).max()) if diff.size else 0.0)
        self.rows.append((case, _np(got), v, e, extra))

    def report(self):
        factor = 1 if self.r is None else max(1, math.ceil(2 * self.r))
        if self.r is not None:
            print("glow-edges: %s: float32 torch on the CPU is within %.3f of the model bound -> factor %d" % (self.kernel, self.r, factor))
        m = Measure(self.kernel, "glow-edges")
        for case, got, v, e, extra in self.rows:
            m.add(case, got, v, factor * e + extra)
        m.report()


def _ub(ref, dt):
    return UB * np.abs(ref.v.numpy()) if dt == BF else 0.0


# ---- 1. element-wise stages -----------------------------------------------------------------------------------------------------------------
EW_RC = [(1, 4), (1, 12), (3, 12), (5, 512), (64, 4), (257, 4)]


def _layouts(R):
    """(row_div, n_img): sample-major with one and three images; batch-major R = n_img N with N = 1 and 5"""
    return [(1, 1), (1, 3)] + [(N, R // N) for N in (1, 5) if R % N == 0]


EW_CASES = [(R, Cc, rd, ni) for R, Cc in EW_RC for rd, ni in _layouts(R)] + [(15, Cc, 5, 3) for Cc in (4, 12, 512)]
CAP_CASE = (CAP_R, 4, 1, 3)


def _ew_cases(big):
    return [CAP_CASE] if big else EW_CASES


def _tail(t):
    """the quads of the ragged second trip (C = 4: the last three rows)"""
    return gr.V(t.v[-3:], t.e[-3:]) if isinstance(t, gr.V) else t[-3:]


def _run_add_image_rows(rows, ops, case):
    R, Cc, rd, ni = case
    g = _gen("air", case)
    H, img = _rn(g, R, Cc), _rn(g, ni, Cc)
    ref = gr.add_image_rows(H, img, rd, ni)
    out, tab = Out((R, Cc), fill=H), Table(ni, Cc, img.cuda())
    ops.launch("mhe_glow_add_image_rows_f32", out.t, tab.view, tab.stride, R, Cc, rd, ni)
    got = out.check(case)
    rows.add(case, got, ref)
    if R == CAP_R:
        rows.add(case + ("tail",), got[-3:], _tail(ref))


def _run_relu_copy(rows, ops, case, dt):
    R, Cc = case[:2]
    x = _plant_h(_rn(_gen("rc", case), R, Cc), F32)
    ref = gr.stored(gr.relu_copy(x), dt)
    out = Out((R, Cc), dt)
    ops.launch("mhe_relu_copy_f32", x.cuda(), out.t, R * Cc, ops.dtype_code(dt))
    got = _np(out.check(case))
    assert np.array_equal(got, ref.numpy()), (case, _dtn(dt), "relu_copy is exact")
    assert np.array_equal(got[-3:], ref.numpy()[-3:]), (case, "tail")
    rows.append(case)


def _run_glu_residual(rows, ops, case, dt):
    R, Cc, rd, ni = case
    g = _gen("gr", case, _dtn(dt))
    H, T, gate = _rn(g, R, Cc), _rn(g, R, Cc, dt=dt), _plant(_rn(g, ni, Cc) * 2, GATES, roll=R + Cc)
    ref = gr.glu_residual(H, T, gate, rd, ni)
    with gr.plain_float32():
        f32 = gr.glu_residual(H, T, gate, rd, ni)
    out, tab = Out((R, Cc), fill=H), Table(ni, Cc, gate.cuda())
    ops.launch("mhe_glow_glu_residual_f32", out.t, _dev(T, dt), ops.dtype_code(dt), tab.view, tab.stride, R, Cc, rd, ni)
    got = out.check(case)
    rows.add(case + (_dtn(dt),), got, ref, f32)
    if R == CAP_R:
        rows.add(case + ("tail",), got[-3:], _tail(ref))


def _run_glu_bwd(rows, ops, case, dt):
    R, Cc, rd, ni = case
    g = _gen("gb", case, _dtn(dt))
    g_h, t3, gate = _rn(g, R, Cc), _rn(g, R, Cc, dt=dt), _plant(_rn(g, ni, Cc) * 2, GATES, roll=R + Cc)
    ref = gr.glu_bwd(g_h, t3, gate, rd, ni)
    with gr.plain_float32():
        f32 = gr.glu_bwd(g_h, t3, gate, rd, ni)
    g_t3, g_gate, tab = Out((R, Cc), dt), Out((R, Cc)), Table(ni, Cc, gate.cuda())
    ops.launch("mhe_glow_glu_bwd_f32", g_h.cuda(), _dev(t3, dt), tab.view, tab.stride, g_t3.t, g_gate.t, R, Cc, rd, ni, ops.dtype_code(dt))
    for name, o, rf, ff, d_o in (("g_t3", g_t3, ref[0], f32[0], dt), ("g_gate", g_gate, ref[1], f32[1], F32)):
        got = o.check(case)
        rows.add(case + (_dtn(dt), name), got, rf, ff, extra=_ub(rf, d_o))
        if R == CAP_R:
            rows.add(case + (name, "tail"), got[-3:], _tail(rf), extra=_ub(_tail(rf), d_o))


def _run_relu_bwd_add(rows, ops, case, gdt, hdt, entry):
    """dyadic operands (sixteenths, |.| <= 4): acc + g is exact in float32"""
    R, Cc = case[:2]
    g = _gen("rba", case, _dtn(gdt), _dtn(hdt))
    acc, gg = (torch.randint(-64, 65, (2, R, Cc), generator=g).float() / 16).unbind(0)
    h = _plant_h(_rn(g, R, Cc, dt=hdt), hdt)
    ref = gr.relu_bwd_add(acc, gg, h).v
    out = Out((R, Cc), fill=acc)
    if entry == "f32":
        ops.launch("mhe_relu_bwd_add_f32", out.t, _dev(gg, gdt), h.cuda(), R * Cc, ops.dtype_code(gdt))
    else:
        ops.launch("mhe_relu_bwd_add_mixed", out.t, _dev(gg, gdt), _dev(h, hdt), R * Cc, ops.dtype_code(gdt), ops.dtype_code(hdt))
    got = _np(out.check(case))
    assert np.array_equal(got, ref.numpy()), (case, _dtn(gdt), _dtn(hdt), entry, "acc + g [h > 0] is exact on dyadic inputs")
    assert np.array_equal(got.reshape(-1)[:4], (acc.view(-1)[:4] + torch.tensor([0.0, 0.0, 0.0, 1.0])[:R * Cc] * gg.view(-1)[:4]).double().numpy()), "only the subnormal opens the gate"
    assert np.array_equal(got[-3:], ref.numpy()[-3:]), (case, "tail")
    rows.append(case)


@pytest.mark.gpu
def test_add_image_rows_against_f64(gpu_lib):
    from mhentropy_amd import ops
    rows = Rows("add_image_rows")
    for case in EW_CASES:
        _run_add_image_rows(rows, ops, case)
    rows.report()


@pytest.mark.gpu
@DTYPES
def test_relu_copy_is_exact(gpu_lib, dt):
    from mhentropy_amd import ops
    rows = []
    for case in EW_CASES:
        _run_relu_copy(rows, ops, case, dt)
    print("glow-edges: relu_copy -> %s: max(|diff| / bound) = 0.000 (exact) over %d cases" % (_dtn(dt), len(rows)))


@pytest.mark.gpu
@DTYPES
def test_glu_residual_against_f64(gpu_lib, dt):
    """gates planted at 0, +-1, +-30, +-104 (rolled from case to case, so that the one-image C = 4 tables reach them all)"""
    from mhentropy_amd import ops
    rows = Rows("glu_residual T " + _dtn(dt))
    for case in EW_CASES:
        _run_glu_residual(rows, ops, case, dt)
    rows.report()


@pytest.mark.gpu
@DTYPES
def test_glu_bwd_against_f64(gpu_lib, dt):
    from mhentropy_amd import ops
    rows = Rows("glu_bwd " + _dtn(dt))
    for case in EW_CASES:
        _run_glu_bwd(rows, ops, case, dt)
    rows.report()


RBA_FORMS = [(F32, F32, "f32"), (BF, F32, "f32"), (F32, BF, "mixed"), (BF, BF, "mixed"), (BF, F32, "mixed")]


@pytest.mark.gpu
def test_relu_bwd_add_is_exact_on_dyadic_inputs(gpu_lib):
    """mhe_relu_bwd_add_f32 with g in f32 / bf16, mhe_relu_bwd_add_mixed with h in bf16 and g in f32 / bf16 (and its hand-over to the f32 form)"""
    from mhentropy_amd import ops
    rows = []
    for gdt, hdt, entry in RBA_FORMS:
        for case in EW_CASES:
            _run_relu_bwd_add(rows, ops, case, gdt, hdt, entry)
    print("glow-edges: relu_bwd_add: max(|diff| / bound) = 0.000 (exact) over %d cases" % len(rows))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["add_image_rows", "relu_copy", "glu_residual", "glu_bwd", "relu_bwd_add"])
def test_elementwise_stage_above_the_grid_cap(gpu_lib, kernel):
    """16384 x 256 + 3 quads (C = 4, three images, 67 MB per tensor): the second trip of the grid-stride loop, ragged; every value depends on
    its index (random), the three tail quads are also compared on their own"""
    from mhentropy_amd import ops
    assert CAP_R * 4 // 4 == CAP + 3
    with torch.no_grad():
        if kernel == "add_image_rows":
            rows = Rows("add_image_rows above the cap")
            _run_add_image_rows(rows, ops, CAP_CASE)
        elif kernel == "relu_copy":
            rows = []
            _run_relu_copy(rows, ops, CAP_CASE, BF)
            _run_relu_copy(rows, ops, CAP_CASE, F32)
        elif kernel == "glu_residual":
            rows = Rows("glu_residual above the cap")
            _run_glu_residual(rows, ops, CAP_CASE, BF)
        elif kernel == "glu_bwd":
            rows = Rows("glu_bwd above the cap")
            _run_glu_bwd(rows, ops, CAP_CASE, BF)
        else:
            rows = []
            _run_relu_bwd_add(rows, ops, CAP_CASE, BF, BF, "mixed")
            _run_relu_bwd_add(rows, ops, CAP_CASE, F32, F32, "f32")
    if isinstance(rows, Rows):
        rows.report()
    else:
        print("glow-edges: %s above the cap: max(|diff| / bound) = 0.000 (exact) over %d cases" % (kernel, len(rows)))


# ---- 2. one wave per row, four rows per workgroup -------------------------------------------------------------------------------------------
ROWS_R = [1, 3, 4, 5, 9]
NARROW, WIDE = [2, 45, 63, 64], [65, 144, 192, 256]


def _row_cases(dims):
    out = []
    for dim in dims:
        for first in (0, 1):
            for T in sorted({1, gr.t_max(dim, first)}):
                out += [(R, dim, first, T) for R in ROWS_R]
    return out


def _nanpad(t, cols):
    """t [R, n] in a [R, cols] tensor whose other columns are NaN"""
    out = torch.full((t.shape[0], cols), NAN)
    out[:, :t.shape[1]] = t
    return out


def _coupling_operands(R, dim, first, T, ldp):
    g = _gen("cpl", R, dim, first, T)
    prm = torch.cat([_rn(g, R, T), _plant(_rn(g, R, T) * 2, US, roll=R)], 1)
    return _nanpad(_rn(g, R, dim), gr.pad_cols(dim)), _nanpad(prm, ldp), _nanpad(_rn(g, R, dim), gr.pad_cols(dim)), _rn(g, R)


def _zero_bits(t):
    return not _bits(t).any()


@pytest.mark.gpu
def test_coupling_both_directions_against_f64(gpu_lib):
    """every pitch boundary (dim 64: no padding column and 2 T = ldp), T = 1 (the j < T guard with transform-parity columns behind it), R % 4 != 0,
    logdet accumulated onto a non-zero seed, us planted at -120, -2, 0, 40; forward then inverse returns the input"""
    from mhentropy_amd import ops
    rows, trip = Rows("coupling"), Rows("coupling inverse(forward(u))")
    for R, dim, first, T in _row_cases(NARROW + WIDE):
        ld, ldp = gr.pad_cols(dim), gr.pad_cols(2 * T)
        u, prm, _, seed = _coupling_operands(R, dim, first, T, ldp)
        ud, pd, fwd_y = u.cuda(), prm.cuda(), None
        for inverse in (0, 1):
            case = (R, dim, first, T, "inverse" if inverse else "forward")
            ref = gr.coupling(u, prm, dim, first, T, inverse, seed)
            with gr.plain_float32():
                f32 = gr.coupling(u, prm, dim, first, T, inverse, seed)
            y, ldet = Out((R, ld)), Out((R,), fill=seed)
            ops.launch("mhe_glow_coupling_f32", ud, pd, y.t, ldet.t, R, dim, first, T, inverse)
            got = y.check(case)
            rows.add(case + ("y",), got, ref[0], f32[0])
            rows.add(case + ("logdet",), ldet.check(case), ref[1], f32[1])
            assert _zero_bits(got[:, dim:]), (case, "padding columns must be +0")
            if not inverse:
                fwd_y, fwd_l, fwd_ref = got.clone(), ldet.t.clone(), ref
        back, ldet = Out((R, ld)), Out((R,), fill=fwd_l)
        ops.launch("mhe_glow_coupling_f32", fwd_y, pd, back.t, ldet.t, R, dim, first, T, 1)
        ref = gr.coupling(fwd_ref[0], prm, dim, first, T, 1, fwd_ref[1].v)
        want = gr.V(gr.pad64(u[:, :dim], ld), ref[0].e)
        trip.add((R, dim, first, T, "u"), back.check("trip"), want)
        trip.add((R, dim, first, T, "logdet"), ldet.check("trip"), gr.V(seed, ref[1].e + fwd_ref[1].e))
    rows.report()
    trip.r = rows.r          # the same expf / logf evaluations: the same margin
    trip.report()


def _check_coupling_bwd(rows, case, g_v, g_prm, ref, f32, dim, T):
    gv, gp = g_v.check(case), g_prm.check(case)
    rows.add(case + ("g_v",), gv, ref[0], f32[0])
    rows.add(case + ("g_prm",), gp, ref[1], f32[1])
    assert _zero_bits(gv[:, dim:]) and _zero_bits(gp[:, 2 * T:]), (case, "padding columns must be +0")


@pytest.mark.gpu
def test_coupling_inv_bwd_narrow_against_f64(gpu_lib):
    """64-pitch rows; g_log_p NULL and given per image with B = 1 and 3 (rows r = n B + b), q_weight = -1 / N"""
    from mhentropy_amd import ops
    rows = Rows("coupling_inv_bwd")
    for R, dim, first, T in _row_cases(NARROW):
        v, prm, g_y, _ = _coupling_operands(R, dim, first, T, 64)
        for B in (1, 3):
            if R % B:
                continue
            qw = float(np.float32(-1.0 / (R // B)))
            g_logp = _rn(_gen("glp", R, B), B)
            for given in (False, True):
                case = (R, dim, first, T, B, given)
                a_q = lambda: gr.mul(gr.d(g_logp)[torch.arange(R) % B], qw) if given else None
                ref = gr.coupling_inv_bwd(v, prm, g_y, dim, first, T, a_q(), ldp=64)
                with gr.plain_float32():
                    f32 = gr.coupling_inv_bwd(v, prm, g_y, dim, first, T, a_q(), ldp=64)
                g_v, g_prm = Out((R, 64)), Out((R, 64))
                ops.launch("mhe_glow_coupling_inv_bwd_f32", v.cuda(), prm.cuda(), g_y.cuda(), g_logp.cuda() if given else None, qw, g_v.t, g_prm.t,
                           R, B, dim, first, T)
                _check_coupling_bwd(rows, case, g_v, g_prm, ref, f32, dim, T)
    rows.report()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["inv_bwd_wide", "fwd_bwd"])
def test_coupling_reverse_at_every_pitch_against_f64(gpu_lib, form):
    """pitches ld = ceil64(dim), ldp = ceil64(2 T_max) (so T = 1 leaves up to 254 columns to zero, T_max at dim 64, 192, 256 none); the
    adjoint of the log-density per row, NULL and given; the ops wrapper gives the same bits"""
    from mhentropy_amd import ops
    rows = Rows("coupling_" + form)
    entry, fn, wrap = {"inv_bwd_wide": ("mhe_glow_coupling_inv_bwd_wide_f32", gr.coupling_inv_bwd, ops.glow_coupling_inv_bwd_wide),
                       "fwd_bwd": ("mhe_glow_coupling_fwd_bwd_f32", gr.coupling_fwd_bwd, ops.glow_coupling_fwd_bwd)}[form]
    for R, dim, first, T in _row_cases(NARROW + WIDE):
        ld, ldp = gr.pad_cols(dim), gr.pad_cols(2 * gr.t_max(dim, first))
        v, prm, g_y, g_log = _coupling_operands(R, dim, first, T, ldp)
        for given in (False, True):
            case = (R, dim, first, T, given)
            a = (gr.V(g_log) if form == "inv_bwd_wide" else g_log) if given else None
            ref = fn(v, prm, g_y, dim, first, T, a, ldp=ldp)
            with gr.plain_float32():
                f32 = fn(v, prm, g_y, dim, first, T, (gr.V(g_log) if form == "inv_bwd_wide" else g_log) if given else None, ldp=ldp)
            g_v, g_prm = Out((R, ld)), Out((R, ldp))
            args = (v.cuda(), prm.cuda(), g_y.cuda(), g_log.cuda() if given else None)
            ops.launch(entry, *args, g_v.t, g_prm.t, R, dim, first, T, ld, ldp)
            _check_coupling_bwd(rows, case, g_v, g_prm, ref, f32, dim, T)
            if R == 5:
                w_v, w_prm = wrap(*args, dim, first, T)
                assert torch.equal(_bits(w_v), _bits(g_v.t)) and torch.equal(_bits(w_prm), _bits(g_prm.t)), (case, "the wrapper's result differs")
    rows.report()


@pytest.mark.gpu
def test_base_density_bwd_and_pad64_against_f64(gpu_lib):
    from mhentropy_amd import ops
    rows, n = Rows("base_density_bwd"), 0
    for dim in NARROW + WIDE:
        ld = gr.pad_cols(dim)
        for R in ROWS_R:
            g = _gen("bd", R, dim)
            x, g_z, g_logp = _rn(g, R, dim), _rn(g, R, dim), _rn(g, R)
            xp = Out((R, ld))
            ops.launch("mhe_pad64_f32", x.cuda(), xp.t, R, dim)
            assert torch.equal(_bits(xp.check((R, dim))), _bits(gr.pad64(x).float())), (R, dim, "pad64 is exact, padding +0")
            n += 1
            zp = _nanpad(x, ld).cuda()
            for gz in (None, g_z):
                for gl in (None, g_logp):
                    case = (R, dim, gz is not None, gl is not None)
                    g_y = Out((R, ld))
                    ops.launch("mhe_glow_base_density_bwd_f32", zp, _dev(gz), _dev(gl), g_y.t, R, dim, ld)
                    got = g_y.check(case)
                    rows.add(case, got, gr.base_density_bwd(_nanpad(x, ld), gz, gl, dim))
                    assert _zero_bits(got[:, dim:]), (case, "padding columns must be +0")
                    if R == 5 and gz is not None and gl is not None:
                        assert torch.equal(_bits(ops.glow_base_density_bwd(zp, gz.cuda(), gl.cuda(), dim)), _bits(got)), (case, "the wrapper's result differs")
    rows.report()
    print("glow-edges: pad64: max(|diff| / bound) = 0.000 (exact) over %d cases" % n)


@pytest.mark.gpu
def test_finish_against_f64(gpu_lib):
    """n_parts 1 and 64, sign +-1, v_out NULL and given; mhe_glow_finish_f32 (raw handle: no Python caller) bit for bit"""
    from mhentropy_amd import ops
    L, rows = gpu_lib, Rows("finish")
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    for dim in NARROW + WIDE:
        ld = gr.pad_cols(dim)
        for R in ROWS_R:
            g = _gen("fin", R, dim)
            z, v, logdet = _nanpad(_rn(g, R, dim), ld), _nanpad(_rn(g, R, dim), ld), _rn(g, R) * 3
            zd, vd, ldd = z.cuda(), v.cuda(), logdet.cuda()
            for n_parts in (1, 64):
                parts = _rn(g, n_parts)
                for sign in (1.0, -1.0):
                    for want_v in (False, True):
                        case = (R, dim, n_parts, sign, want_v)
                        v_out, logp = (Out((R, dim)) if want_v else None), Out((R,))
                        ops.launch("mhe_glow_finish_dev_f32", zd, vd if want_v else None, ldd, v_out.t if want_v else None, logp.t, R, dim, sign, parts.cuda(), n_parts)
                        rows.add(case, logp.check(case), gr.finish(z, logdet, dim, sign, parts))
                        if want_v:
                            assert torch.equal(_bits(v_out.check(case)), _bits(v[:, :dim])), (case, "v_out is a copy")
                        if n_parts == 1:
                            v2, lp2 = (Out((R, dim)) if want_v else None), Out((R,))
                            st = L.mhe_glow_finish_f32(p(zd), p(vd if want_v else None), p(ldd), p(v2.t if want_v else None), p(lp2.t), R, dim, sign, sign * float(parts[0]),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
                            assert st == 0, L.mhe_last_error()
                            assert torch.equal(_bits(lp2.check(case)), _bits(logp.t)), (case, "finish_f32 differs from finish_dev")
                            assert not want_v or torch.equal(_bits(v2.check(case)), _bits(v_out.t))
            out, lp = ops.glow_finish(zd, vd, ldd, R, dim, True, parts.cuda())
            assert torch.equal(_bits(lp), _bits(logp.t)) and torch.equal(_bits(out), _bits(v_out.t)), "the wrapper's result differs"
    rows.report()


# ---- 3. the per-image reverse stages ---------------------------------------------------------------------------------------------------------
CN = [(4, 1), (4, 513), (4, 2049), (8, 257), (512, 1), (512, 3), (512, 15), (512, 16), (512, 17), (512, 200), (2048, 1), (2048, 4), (2048, 5)]


@pytest.mark.gpu
def test_glu_bwd_sum_against_f64(gpu_lib):
    """C = 4 (512 row lanes, N below, around and above them) to C = 2048 (one lane, no fold), N around 4 nl; gct / bsum rows of a wider table"""
    from mhentropy_amd import ops
    rows, sums = Rows("glu_bwd_sum g_t3"), Rows("glu_bwd_sum gct / bsum")
    for Cc, N in CN:
        for B in (1, 3):
            case = (Cc, N, B)
            g = _gen("gbs", case)
            g_h, t3, gate = _rn(g, N * B, Cc), _rn(g, N * B, Cc, dt=BF), _plant(_rn(g, B, Cc) * 2, GATES, roll=N + Cc)
            ref = gr.glu_bwd_sum(g_h, t3, gate, N, B)
            with gr.plain_float32():
                f32 = gr.glu_bwd_sum(g_h, t3, gate, N, B)
            tab, got = Table(B, Cc, gate.cuda()), []
            for call in range(2):
                g_t3, gct, bsum = Out((N * B, Cc), BF), Table(B, Cc, around=SENT), Table(B, Cc, around=SENT)
                ops.launch("mhe_glow_glu_bwd_sum", g_h.cuda(), _dev(t3, BF), tab.view, tab.stride, g_t3.t, gct.view, gct.stride, bsum.view, bsum.stride, N, B, Cc)
                got.append((g_t3.check(case), gct.check(case), bsum.check(case)))
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*got)), (case, "two calls differ")
            rows.add(case, got[0][0], ref[0], f32[0], extra=_ub(ref[0], BF))
            sums.add(case + ("gct",), got[0][1], ref[1], f32[1])
            sums.add(case + ("bsum",), got[0][2], ref[2], f32[2])
    rows.report()
    sums.report()


@pytest.mark.gpu
def test_mask_scale_sum_against_f64(gpu_lib):
    """t2 with zeros and -0 planted; g' in place as bf16; the bias sum is the sum of the STORED values"""
    from mhentropy_amd import ops
    rows, sums = Rows("mask_scale_sum g'"), Rows("mask_scale_sum bsum")
    scale = float(np.float32(1.0 / (1.0 - 0.2)))
    for Cc, N in CN:
        for B in (1, 3):
            case = (Cc, N, B)
            g = _gen("mss", case)
            gg = _rn(g, N * B, Cc, dt=BF)
            t2 = _plant(torch.relu(_rn(g, N * B, Cc, dt=BF)), [0.0, -0.0, 1.0, 0.0], roll=N)
            st, bs = gr.mask_scale_sum(gg, t2, scale, N, B)
            got = []
            for call in range(2):
                io, bsum = Out((N * B, Cc), BF, fill=gg), Table(B, Cc, around=SENT)
                ops.launch("mhe_glow_mask_scale_sum", io.t, _dev(t2, BF), scale, bsum.view, bsum.stride, N, B, Cc)
                got.append((io.check(case), bsum.check(case)))
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*got)), (case, "two calls differ")
            rows.add(case, got[0][0], gr.V(st, (U32 + UB) * st.abs()))
            assert not _np(got[0][0])[(t2 <= 0).numpy()].any(), (case, "closed gates must give 0")
            sums.add(case, got[0][1], bs)
    rows.report()
    sums.report()


# ---- 4. the dense layer ---------------------------------------------------------------------------------------------------------------------
MNK = [(1, 4, 64), (16, 16, 64), (17, 20, 64), (64, 8180, 64), (65, 8192, 64), (128, 8192, 64), (129, 8192, 128), (256, 8180, 64), (65, 512, 64),
       (200, 36, 192), (257, 8, 64), (5, 8, 32), (300, 64, 96)]


def _linear_kernel(M, N, K):
    """the kernel mhe_linear_f32 reaches, from its own shape arithmetic (skinny_launch of conv.hip)"""
    if M > 256 or K % 64:
        return "tiled"
    if M > 64 and (N + 15) // 16 < 512:
        return "skinny<4> rows split"
    return "skinny<%d>" % (4 if M <= 64 else 8 if M <= 128 else 16)


@pytest.mark.gpu
def test_linear_every_kernel_against_f64(gpu_lib):
    """all three row-tile instantiations (<8> and <16> need N >= 8180), M one above each row tile, the row-split grid with a ragged last
    slice, N % 16 = 4 and 8 (the clamped weight row and the nb < N guard), and the tiled fallback for M > 256 and K % 64 != 0; with and without
    bias and ReLU.  mhe_linear_skinny_f32 is called through the raw handle (no Python caller)"""
    from mhentropy_amd import ops
    L, by_kernel = gpu_lib, {}
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    for Mr, N, K in MNK:
        g = _gen("lin", Mr, N, K)
        x, w, b = _rn(g, Mr, K), _rn(g, N, K) * K ** -0.5, _rn(g, N)
        xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
        kernel = _linear_kernel(Mr, N, K)
        m = by_kernel.setdefault(kernel, Measure("linear " + kernel, "glow-edges"))
        for bias in (None, b):
            for relu in (False, True):
                case = (Mr, N, K, bias is not None, relu)
                ref, mag = gr.linear(x, w, bias, relu)
                y = Out((Mr, N))
                ops.linear(xd, wd, bd if bias is not None else None, relu=relu, out=y.t)
                got = y.check(case)
                m.add(case, _np(got), ref.numpy(), gr.linear_bound(mag, K).numpy())
                if kernel != "tiled":
                    y2 = Out((Mr, N))
                    st = L.mhe_linear_skinny_f32(p(xd), p(wd), p(bd if bias is not None else None), p(y2.t), Mr, N, K, int(relu), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                    assert st == 0, L.mhe_last_error()
                    assert torch.equal(_bits(y2.check(case)), _bits(got)), (case, "mhe_linear_skinny_f32 differs from mhe_linear_f32")
    assert set(by_kernel) == {"tiled", "skinny<4>", "skinny<8>", "skinny<16>", "skinny<4> rows split"}
    for m in by_kernel.values():
        m.report()


@pytest.mark.gpu
@pytest.mark.parametrize("Mr,N,K", [(16, 16, 64), (65, 512, 64)])
def test_linear_bf16copy_is_the_rounding_of_its_f32_output(gpu_lib, Mr, N, K):
    from mhentropy_amd import ops
    g = _gen("linb", Mr, N, K)
    x, w, b = _rn(g, Mr, K), _rn(g, N, K) * K ** -0.5, _rn(g, N)
    m = Measure("linear_f32_bf16copy " + _linear_kernel(Mr, N, K), "glow-edges")
    for relu in (0, 1):
        ref, mag = gr.linear(x, w, b, bool(relu))
        y, yb = Out((Mr, N)), Out((Mr, N), BF)
        ops.launch("mhe_linear_f32_bf16copy", x.cuda(), w.cuda(), b.cuda(), y.t, yb.t, Mr, N, K, relu)
        got = y.check((Mr, N, K))
        m.add((Mr, N, K, relu), _np(got), ref.numpy(), gr.linear_bound(mag, K).numpy())
        assert torch.equal(_bits(yb.check((Mr, N, K))), _bits(got.cpu().to(BF))), "the bf16 copy is not the rounding of the f32 output"
        y1 = ops.linear(x.cuda(), w.cuda(), b.cuda(), relu=bool(relu))
        assert torch.equal(_bits(y1), _bits(got)), "the f32 output differs from mhe_linear_f32's"
    m.report()
