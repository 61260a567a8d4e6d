"""Two convolution entries that the suite reached only through a whole train step, each against float64 at the smallest shape it accepts:
mhe_conv1x1_cat_bias_nhwc (ops.conv2d_nhwc xcat= without mask=: one product over two operand tensors, + a per-channel constant, + a residual)
and mhe_conv2d_f32out_nhwc (ops.linear_bf16_f32out: f32 result of a bf16 product).  Operands are storage-rounded bf16; the reference is
float64 on the CPU.

Bounds: the f32 accumulation of exact bf16 products carries tests/test_gpu_wgrad_edges.py's 2e-5 of max|ref| (here over at most 192 terms,
far fewer than its ~5,000).  The f32 result has nothing else.  The cat form stores bf16, and the forward epilogue (conv_shared.h) rounds
twice by design: the product goes to LDS as the bf16 value a plain launch would store, then product + constant + residual is rounded to
storage.  Round to nearest on bf16's 8 significand bits is at most 2^-8 of the value, so the two roundings add at most
2^-8 (max|product| + max|ref|) (1 + 2e-5).  Each test prints what it measured before it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

from conftest import assert_close

RTOL_ACC = 2e-5
U_BF16 = 2.0 ** -8            # unit roundoff of bf16 storage
B, H, W = 2, 16, 16          # 512 pixels: four 128-row tiles


def _bf16(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def _report(what, got, ref):
    print("conv-forms: %s: max|diff| / max|ref| = %.3e" % (what, np.abs(got - ref).max() / np.abs(ref).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("Cout,tile", [(128, 0), (64, 0), (128, 1)], ids=["128x128", "128x64", "forced-128x64"])
@pytest.mark.parametrize("with_residual", [False, True], ids=["bias", "bias+residual"])
def test_two_operand_product_with_bias_against_f64(gpu_lib, Cout, tile, with_residual):
    from mhentropy_amd import ops
    Cin, cin2 = 64, 128                                   # unequal, so a swapped operand pair cannot pass
    x, xc = _bf16((B, H, W, Cin), 1), _bf16((B, H, W, cin2), 2)
    w = _bf16((Cout, Cin + cin2), 3, (Cin + cin2) ** -0.5)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(4))
    res = _bf16((B, H, W, Cout), 5) if with_residual else None
    prod = torch.cat([x, xc], -1).double().reshape(-1, Cin + cin2) @ w.double().t()
    ref = prod + bias.double()
    if with_residual:
        ref = ref + res.double().reshape(-1, Cout)
    y = ops.conv2d_nhwc(x.cuda(), w.cuda(), 1, 1, 1, 0, xcat=xc.cuda(), out_shift=bias.cuda(), residual=res.cuda() if with_residual else None,
                        tile=tile)
    torch.cuda.synchronize()
    got = y.float().cpu().double().reshape(-1, Cout).numpy()
    _report("cat_bias Cout=%d tile=%d residual=%d" % (Cout, tile, with_residual), got, ref.numpy())
    two_roundings = U_BF16 * (prod.abs().max().item() + ref.abs().max().item()) * (1 + RTOL_ACC)
    print("conv-forms: bound %.3e of max|ref|" % (RTOL_ACC + two_roundings / ref.abs().max().item()))
    assert_close(got, ref.numpy(), RTOL_ACC, atol=two_roundings, what="mhe_conv1x1_cat_bias_nhwc")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [128, 72], ids=["128", "ragged-72"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
def test_f32_result_of_a_bf16_product_against_f64(gpu_lib, N, with_bias):
    from mhentropy_amd import ops
    R, K = 300, 128                                       # three row tiles, the last ragged
    x, w = _bf16((R, K), 11), _bf16((N, K), 12, K ** -0.5)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(13)) if with_bias else None
    ref = x.double() @ w.double().t()
    if with_bias:
        ref = ref + bias.double()
    out = torch.full((R, N), 7.0, device="cuda")
    y = ops.linear_bf16_f32out(x.cuda(), w.cuda(), bias.cuda() if with_bias else None, out=out)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32
    got = y.cpu().double().numpy()
    _report("f32out N=%d bias=%d" % (N, with_bias), got, ref.numpy())
    assert_close(got, ref.numpy(), RTOL_ACC, what="mhe_conv2d_f32out_nhwc")
