"""The weight-gradient kernels of csrc/wgrad.hip at the edges their launcher (plan_wgrad) and their zero-fill paths have: ragged output tiles
(Cout, KH*KW*Cin no multiple of the tile), pixel counts that fill the last stage / the last slice only partly, Ho != Wo with neither a power
of two (the multiply-high reciprocals of the LDS-DMA kernel), ldw > KH*KW*Cin, the XCD-aware grid order with empty slices, the grouped and the
multi-problem launch, the dense form, and the fixed-order column sums.  Every expected value is float64 on the CPU from the storage-rounded
operands (einsum over F.unfold); a CPU-only self-check holds that reference against f64 autograd.

Bounds: 2e-5 of max|dW| for both storage types (the project's bound for this kernel family: bf16 products are exact in f32, the f32
accumulation over at most ~5,000 pixels stays well inside it); 1e-6 of max|sum| for the column sums (sums of at most 5,000 values in f32,
cut into slabs).  Every test prints the error it measured before it asserts (pytest -s)."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import assert_close

BF, F32 = torch.bfloat16, torch.float32
RTOL = 2e-5

# (Cin, Cout, k, stride, pad, B, H, W): the variant mhe_conv_wgrad_variant must name for bf16 / f32 storage, what the row is there for
ROWS = [
    ((24, 72, 3, 1, 1, 3, 7, 5), 1128128, 128128),      # N = 216, Cout = 72 ragged against 128; P = 105 = 3 stages + 9 pixels; Ho = 7 != Wo = 5
    ((40, 56, 1, 1, 0, 5, 9, 11), 1064064, 64128),      # the `plain` address path; P = 495
    ((48, 200, 1, 2, 0, 2, 13, 10), 1128064, 128128),   # strided 1x1 (not plain); Ho = 7, Wo = 5; Cout ragged in the second row tile
    ((72, 40, 3, 2, 1, 4, 14, 9), 1064128, 64128),      # stride-2 3x3, odd Wo
    ((264, 256, 3, 1, 1, 3, 7, 5), 1256256, 128128),    # the 256 x 256 tile at N = 2376: last column tile ragged
    ((72, 136, 1, 1, 0, 6, 27, 29), 1128128, 128128),   # P = 4698: ten slices of 512 in XCD order (grid.z = 16, six empty), last slice 90 pixels
    ((8, 72, 9, 1, 4, 2, 11, 6), 2128128, 128128),      # 81 taps > 64: the register-staged bf16 kernel without an environment switch
    ((12, 68, 3, 1, 1, 3, 7, 5), 128128, 128128),       # Cin % 8 != 0: the generic kernel on bf16 storage
    ((4, 36, 3, 1, 1, 3, 7, 5), 64128, 64128),          # the generic kernel, small tile
]
XCD_ROW = 5
IDS = ["%dto%d_k%ds%dp%d_b%d_%dx%d" % r[0] for r in ROWS]


def _geom(case):
    Cin, Cout, k, stride, pad, B, H, W = case
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def dw_reference(x, gy, k, stride, pad):
    """dW [Cout, k*k*Cin] (tap-major, channel-minor) in float64 from NHWC operands: dW[o, t, c] = sum_{b, l} gy[b, l, o] * patches[b, c, t, l]"""
    import torch.nn.functional as F
    B, H, W, Cin = x.shape
    Cout = gy.shape[-1]
    cols = F.unfold(x.double().permute(0, 3, 1, 2), k, padding=pad, stride=stride).view(B, Cin, k * k, -1)
    return torch.einsum("blo,bctl->otc", gy.double().reshape(B, -1, Cout), cols).reshape(Cout, k * k * Cin).numpy()


@functools.lru_cache(None)
def _problem(row, dtname):
    """operands (storage-rounded, NHWC, on the CPU as f32) and the f64 gradient of one table row: computed once, shared, never written"""
    case = ROWS[row][0]
    Cin, Cout, k, stride, pad, B, H, W = case
    dt = getattr(torch, dtname)
    Ho, Wo = _geom(case)
    g = torch.Generator().manual_seed(1000 + 10 * row + (dt == BF))
    x = torch.randn(B, H, W, Cin, generator=g).to(dt).float()
    gy = torch.randn(B, Ho, Wo, Cout, generator=g).to(dt).float()
    return x, gy, dw_reference(x, gy, k, stride, pad)


def _dtn(dt):
    return "bfloat16" if dt == BF else "float32"


def _desc(case, dt, from_ops):
    Cin, Cout, k, stride, pad, B, H, W = case
    return from_ops.ConvDesc(B, H, W, Cin, Cout, k, k, stride, pad, from_ops.dtype_code(dt), 0, 0)


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    print("wgrad-edges: %s: max|diff| / max|ref| = %.3e" % (what, np.abs(got - ref).max() / np.abs(ref).max()))
    assert_close(got, ref, RTOL, what=what)


# ---- 0. the reference itself (no GPU) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [2, 3])
def test_einsum_reference_agrees_with_f64_autograd(row):
    import torch.nn.functional as F
    Cin, Cout, k, stride, pad, B, H, W = ROWS[row][0]
    x, gy, ref = _problem(row, "bfloat16")
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, stride=stride, padding=pad).backward(gy.double().permute(0, 3, 1, 2))
    assert_close(ref, w.grad.permute(0, 2, 3, 1).reshape(Cout, -1).numpy(), 1e-13, what="einsum reference vs f64 autograd")


# ---- 1. ragged single-problem launches --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("slabs", [True, False], ids=["partial-slabs", "atomics"])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("row", range(len(ROWS)), ids=IDS)
def test_ragged_weight_gradient_against_f64(gpu_lib, row, dt, slabs, monkeypatch):
    """ops.conv_wgrad at one table row: the instantiation is the one the row is there for, dW += (the ones survive) equals the f64 gradient to
    2e-5 of its largest element, and where the pixel range goes through slabs two launches give the same bits"""
    import ctypes as C
    from mhentropy_amd import ops
    monkeypatch.setattr(ops, "WGRAD_SLABS", slabs)
    case, v_bf16, v_f32 = ROWS[row]
    Cin, Cout, k, stride, pad, B, H, W = case
    d = _desc(case, dt, ops)
    variant = gpu_lib.mhe_conv_wgrad_variant(C.byref(d), 0, 0, 1)
    assert variant == (v_bf16 if dt == BF else v_f32), (case, variant)
    ws_floats = gpu_lib.mhe_conv_wgrad_workspace_floats(C.byref(d))
    if dt == F32:
        assert ws_floats > 0, "the f32 split (64-pixel slices) must take slabs at every row"
    if dt == BF and row == XCD_ROW:
        gz = ws_floats // (256 * 128)          # padded tile area: two 128-row tiles x one 128-column tile
        assert ws_floats % (256 * 128) == 0 and gz == 10, (ws_floats, gz)          # >= 8 slices: XCD order, grid.z rounded up to 16
    x, gy, ref = _problem(row, _dtn(dt))
    xd, gyd = x.to(dt).cuda(), gy.to(dt).cuda()
    dw = ops.conv_wgrad(xd, gyd, k, k, stride, pad, torch.ones(Cout, k * k * Cin, device="cuda"))
    _close(dw.cpu().numpy() - 1.0, ref, "variant %d %s %s %s" % (variant, IDS[row], _dtn(dt), "slabs" if slabs and ws_floats else "atomics"))
    if slabs and ws_floats:
        dw2 = ops.conv_wgrad(xd, gyd, k, k, stride, pad, torch.ones(Cout, k * k * Cin, device="cuda"))
        assert torch.equal(dw, dw2), "two slab launches differ: the summation order is not fixed"


@pytest.mark.gpu
@pytest.mark.parametrize("slabs", [True, False], ids=["partial-slabs", "atomics"])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("row", [0, XCD_ROW], ids=[IDS[0], IDS[XCD_ROW]])
def test_row_pitch_wider_than_the_gradient(gpu_lib, row, dt, slabs, monkeypatch):
    """ldw = KH*KW*Cin + 12: the gradient lands at that pitch and the twelve pad floats of every row come back bit-unchanged"""
    from mhentropy_amd import ops
    monkeypatch.setattr(ops, "WGRAD_SLABS", slabs)
    Cin, Cout, k, stride, pad, B, H, W = ROWS[row][0]
    N = k * k * Cin
    x, gy, ref = _problem(row, _dtn(dt))
    buf = torch.full((Cout, N + 12), -123.0)
    buf[:, :N] = 1.0
    dev = buf.cuda()
    ops.conv_wgrad(x.to(dt).cuda(), gy.to(dt).cuda(), k, k, stride, pad, dev, ldw=N + 12)
    out = dev.cpu()
    assert torch.equal(out[:, N:], buf[:, N:]), "pad columns of dW written"
    _close(out[:, :N].numpy() - 1.0, ref, "ldw = N + 12, %s %s" % (IDS[row], _dtn(dt)))


# ---- 2. MHE_WGRAD_DMA=0 / MHE_WGRAD_W16=0: read once per process, hence one fresh child each -------------------------------------------------------
ENV_RUNS = [("MHE_WGRAD_DMA", [0, 1, 2, 3], [2128128, 2064064, 2128064, 2064128], "wgrad_bf16_kernel"),
            ("MHE_WGRAD_W16", [4], [1256256], "wgrad_dma_kernel<256, 256, 4, 2>")]


def _env_child(out_path):
    """runs in the child: the rows of the switch that is set, bf16, through ops.conv_wgrad; dW (+ 1), variant codes and kernel names to out_path"""
    import ctypes as C
    from mhentropy_amd import _lib, ops
    (rows,) = [r for name, r, _, _ in ENV_RUNS if os.environ.get(name) == "0"]
    res = {}
    for row in rows:
        Cin, Cout, k, stride, pad, B, H, W = ROWS[row][0]
        x, gy, _ = _problem(row, "bfloat16")
        d = _desc(ROWS[row][0], BF, ops)
        res["variant%d" % row] = np.int64(_lib.lib().mhe_conv_wgrad_variant(C.byref(d), 0, 0, 1))
        res["kernel%d" % row] = np.array(ops._wgrad_kernel_name(d))
        dw = ops.conv_wgrad(x.to(BF).cuda(), gy.to(BF).cuda(), k, k, stride, pad, torch.ones(Cout, k * k * Cin, device="cuda"))
        res["dw%d" % row] = dw.cpu().numpy()
    np.savez(out_path, **res)


@pytest.mark.gpu
def test_register_staged_and_eight_wave_kernels_in_fresh_processes(gpu_lib):
    """MHE_WGRAD_DMA=0: the first four rows on the four register-staged bf16 tiles; MHE_WGRAD_W16=0: the 256 x 256 tile on eight waves.  One child
    per switch, one after the other; a child that fails ends the test before the next one starts"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {here!r}); import test_gpu_wgrad_edges as T; T._env_child(sys.argv[1])"
    with tempfile.TemporaryDirectory() as tmp:
        for name, rows, variants, kernel in ENV_RUNS:
            out = os.path.join(tmp, name + ".npz")
            env = {k: v for k, v in os.environ.items() if k not in ("MHE_WGRAD_DMA", "MHE_WGRAD_W16")}
            p = subprocess.run([sys.executable, "-c", code, out], env={**env, name: "0"}, timeout=300, capture_output=True, text=True)
            assert p.returncode == 0, (name, p.returncode, p.stderr[-2000:])
            got = np.load(out)
            for row, variant in zip(rows, variants):
                assert int(got["variant%d" % row]) == variant, (name, row, int(got["variant%d" % row]))
                assert kernel in str(got["kernel%d" % row]), (name, row, str(got["kernel%d" % row]))
                _close(got["dw%d" % row] - 1.0, _problem(row, "bfloat16")[2], "%s=0 variant %d %s" % (name, variant, IDS[row]))


# ---- 3. grouped, multi-problem and dense forms ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _grouped(nbatch, R, K, N):
    g = torch.Generator().manual_seed(R + K + N)
    xs = torch.randn(nbatch, R, K, generator=g).to(BF).float()
    gys = torch.randn(nbatch, R, N, generator=g).to(BF).float()
    refs = torch.einsum("brn,brk->bnk", gys.double(), xs.double()).numpy()
    shared = torch.einsum("brn,rk->bnk", gys.double(), xs[0].double()).numpy()          # every problem reads problem 0's x
    return xs, gys, refs, shared


@pytest.mark.gpu
@pytest.mark.parametrize("slabs", [True, False], ids=["partial-slabs", "atomics"])
@pytest.mark.parametrize("nbatch,R,K,N,variant", [(5, 1100, 72, 136, 1128128), (3, 300, 1032, 256, 1256256)], ids=["5x1100x72x136", "3x300x1032x256"])
def test_grouped_launch_dense_and_strided(gpu_lib, nbatch, R, K, N, variant, slabs, monkeypatch):
    """ops.conv_wgrad_batched with its default strides and as the train step lays the operands out: one shared x (stride 0), gy at twice the
    dense stride inside a larger buffer, the gradients dw_batch_stride > N*K apart in an arena whose other floats must not change.
    (K = 1032: the 256 x 256 tile asks for KH*KW*Cin % 256 == 0 or >= 1024, and 1032 leaves its last column tile ragged)"""
    import ctypes as C
    from mhentropy_amd import ops
    monkeypatch.setattr(ops, "WGRAD_SLABS", slabs)
    d = ops.ConvDesc(R, 1, 1, K, N, 1, 1, 1, 0, ops.BF16, 0, 0)
    assert gpu_lib.mhe_conv_wgrad_variant(C.byref(d), 0, 0, nbatch) == variant
    took_slabs = slabs and gpu_lib.mhe_conv_wgrad_batched_workspace_floats(C.byref(d), nbatch) > 0
    xs, gys, refs, shared = _grouped(nbatch, R, K, N)
    # default strides
    runs = []
    for _ in range(2 if took_slabs else 1):
        dw = torch.ones(nbatch, N, K, device="cuda")
        ops.conv_wgrad_batched(xs.to(BF).cuda(), gys.to(BF).cuda(), dw, N * K, nbatch)
        runs.append(dw)
    for b in range(nbatch):
        _close(runs[0][b].cpu().numpy() - 1.0, refs[b], "grouped variant %d, dense strides, problem %d" % (variant, b))
    assert len(runs) == 1 or torch.equal(runs[0], runs[1]), "two grouped slab launches differ"
    # the train step's layout
    dws = N * K + 52
    gbuf = torch.zeros(nbatch, 2, R, N)
    gbuf[:, 0] = gys
    gbuf[:, 1] = 77.0          # the floats between two problems' gy: never read
    arena = torch.full((nbatch * dws,), -123.0)
    for b in range(nbatch):
        arena[b * dws:b * dws + N * K] = 1.0
    runs = []
    for _ in range(2 if took_slabs else 1):
        dev = arena.cuda()
        ops.conv_wgrad_batched(xs[0].to(BF).cuda(), gbuf.to(BF).cuda(), dev, dws, nbatch, x_batch_stride=0, gy_batch_stride=2 * R * N)
        runs.append(dev.cpu())
    out = runs[0].view(nbatch, dws)
    assert torch.equal(out[:, N * K:], arena.view(nbatch, dws)[:, N * K:]), "floats between the problems' gradients written"
    for b in range(nbatch):
        _close(out[b, :N * K].view(N, K).numpy() - 1.0, shared[b], "grouped variant %d, shared x / strided gy / arena, problem %d" % (variant, b))
    assert len(runs) == 1 or torch.equal(runs[0], runs[1]), "two grouped slab launches differ"


@pytest.mark.gpu
def test_multi_problem_launch_at_ragged_shapes(gpu_lib):
    """ops.conv_wgrad_multi over the first six bf16 rows (rows 0 and 5 share the 128 x 128 class and one launch: one unsplit problem with plain
    stores next to one in ten slices) and an f32 row: against f64, against ops.conv_wgrad per problem, and two calls give the same bits"""
    from mhentropy_amd import ops
    todo = [(row, BF) for row in range(6)] + [(0, F32)]
    items, singles = [], []
    for row, dt in todo:
        Cin, Cout, k, stride, pad, B, H, W = ROWS[row][0]
        x, gy, _ = _problem(row, _dtn(dt))
        xd, gyd = x.to(dt).cuda(), gy.to(dt).cuda()
        items.append((xd, gyd, k, k, stride, pad, torch.ones(Cout, k * k * Cin, device="cuda")))
        singles.append(ops.conv_wgrad(xd, gyd, k, k, stride, pad, torch.ones(Cout, k * k * Cin, device="cuda")).cpu().numpy())
    ops.conv_wgrad_multi(items)
    first = [it[6].clone() for it in items]
    for (row, dt), it, one in zip(todo, items, singles):
        _close(it[6].cpu().numpy() - 1.0, _problem(row, _dtn(dt))[2], "multi-problem %s %s" % (IDS[row], _dtn(dt)))
        assert_close(it[6].cpu().numpy() - 1.0, one - 1.0, RTOL, what="multi-problem vs its own launch %s %s" % (IDS[row], _dtn(dt)))
    for it in items:
        it[6].fill_(1.0)
    ops.conv_wgrad_multi(items)
    assert all(torch.equal(it[6], f) for it, f in zip(items, first)), "two multi-problem calls differ: the summation order is not fixed"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("R", [1, 33, 1000])
def test_dense_layer_weight_gradient(gpu_lib, R, dt):
    """ops.linear_wgrad: dW [12, 20] += gy [R, 12]^T x [R, 20]"""
    from mhentropy_amd import ops
    K, N = 20, 12
    g = torch.Generator().manual_seed(R)
    x = torch.randn(R, K, generator=g).to(dt).float()
    gy = torch.randn(R, N, generator=g).to(dt).float()
    dw = ops.linear_wgrad(x.to(dt).cuda(), gy.to(dt).cuda(), torch.ones(N, K, device="cuda"))
    _close(dw.cpu().numpy() - 1.0, (gy.double().T @ x.double()).numpy(), "linear_wgrad R = %d %s" % (R, _dtn(dt)))


@pytest.mark.gpu
def test_workspace_one_float_short_is_an_error(gpu_lib):
    """mhe_conv_wgrad_ws_nhwc with a workspace one float short of mhe_conv_wgrad_workspace_floats on a launch that takes slabs: an error code, a
    message, and dW untouched (no fall-back to order-dependent atomics)"""
    import ctypes as C
    from mhentropy_amd import ops
    case = ROWS[XCD_ROW][0]
    Cin, Cout, k, stride, pad, B, H, W = case
    d = _desc(case, BF, ops)
    need = gpu_lib.mhe_conv_wgrad_workspace_floats(C.byref(d))
    assert need > 0
    x, gy, ref = _problem(XCD_ROW, "bfloat16")
    xd, gyd = x.to(BF).cuda(), gy.to(BF).cuda()
    ws = torch.empty(need, device="cuda")
    dw = torch.full((Cout, k * k * Cin), 5.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = gpu_lib.mhe_conv_wgrad_ws_nhwc(C.byref(d), xd.data_ptr(), gyd.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), need - 1, stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"workspace" in gpu_lib.mhe_last_error()
    assert torch.equal(dw.cpu(), torch.full((Cout, k * k * Cin), 5.0)), "a refused launch wrote dW"
    rc = gpu_lib.mhe_conv_wgrad_ws_nhwc(C.byref(d), xd.data_ptr(), gyd.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), need, stream)
    assert rc == 0
    _close(dw.cpu().numpy() - 5.0, ref, "workspace of exactly the queried size")


# ---- 4. column sums ---------------------------------------------------------------------------------------------------------------------------
COLSUM_R = [1, 16, 17, 1000, 4096, 5000]          # <= 16 rows: one launch; more: row slabs into the workspace + a second launch
COLSUM_RTOL = 1e-6


@functools.lru_cache(None)
def _rows(R, Cc, dtname):
    g = torch.Generator().manual_seed(R * 7 + Cc)
    rows = torch.randn(R, Cc, generator=g).to(getattr(torch, dtname)).float()
    return rows, rows.double().sum(0).numpy()


def _colsum_close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    print("wgrad-edges: %s: max|diff| / max|ref| = %.3e" % (what, np.abs(got - ref).max() / np.abs(ref).max()))
    assert_close(got, ref, COLSUM_RTOL, what=what)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", [8, 64, 256, 320, 1032])
def test_column_sums_against_f64(gpu_lib, Cc, dt):
    """ops.colsum: out += column sums in a fixed order, for both launch forms and (C = 320, 1032) a ragged last column group"""
    from mhentropy_amd import ops
    for R in COLSUM_R:
        assert (gpu_lib.mhe_colsum_workspace_floats(R, Cc) > 0) == (R > 16)
        rows, ref = _rows(R, Cc, _dtn(dt))
        dev = rows.to(dt).cuda()
        out = ops.colsum(dev, torch.ones(Cc, device="cuda"))
        _colsum_close(out.cpu().numpy() - 1.0, ref, "colsum R = %d C = %d %s" % (R, Cc, _dtn(dt)))
        assert torch.equal(out, ops.colsum(dev, torch.ones(Cc, device="cuda"))), "two column sums differ (R = %d)" % R


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("R", [16, 1000])
def test_column_sums_into_strided_groups(gpu_lib, R, dt):
    """group_width = 64, group_stride = 100: column c is added to out[(c // 64) * 100 + c % 64], the 36 floats between two groups stay"""
    from mhentropy_amd import ops
    Cc, gw, gs = 320, 64, 100
    rows, ref = _rows(R, Cc, _dtn(dt))
    buf = torch.full((Cc // gw, gs), -123.0)
    buf[:, :gw] = 1.0
    dev = buf.cuda()
    ops.colsum(rows.to(dt).cuda(), dev, group_width=gw, group_stride=gs)
    out = dev.cpu()
    assert torch.equal(out[:, gw:], buf[:, gw:]), "gaps between the output groups written"
    _colsum_close(out[:, :gw].reshape(-1).numpy() - 1.0, ref, "grouped colsum R = %d %s" % (R, _dtn(dt)))


@pytest.mark.gpu
def test_column_sums_refuse_what_they_cannot_do(gpu_lib):
    """C = 24 neither divides 256 nor reaches it; 5,000 rows without a workspace have no fixed-order form: an error each, and `out` untouched"""
    from mhentropy_amd import _lib, ops
    out = torch.full((24,), 5.0, device="cuda")
    with pytest.raises(_lib.MheError, match="C=24"):
        ops.colsum(torch.ones(40, 24, device="cuda"), out)
    big = torch.ones(5000, 64, device="cuda")
    out64 = torch.full((64,), 5.0, device="cuda")
    rc = gpu_lib.mhe_colsum_f32(big.data_ptr(), out64.data_ptr(), 5000, 64, ops.F32, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"workspace" in gpu_lib.mhe_last_error()
    assert torch.equal(out.cpu(), torch.full((24,), 5.0)) and torch.equal(out64.cpu(), torch.full((64,), 5.0)), "a refused call wrote `out`"
