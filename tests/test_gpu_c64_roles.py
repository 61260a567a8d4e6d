"""The row-streaming 3x3 kernel's forward forms (csrc/conv_stream.hip, 64 -> 64 channels on 64-pixel-wide maps) run three roles per
workgroup: multiply waves, load waves (global rows -> BatchNorm + ReLU -> LDS ring) and store waves (staging -> batch statistics -> global
stores).  The roles meet only at the tick barrier, so the cases below are the ones where a ring slot or a staging parity could be read or
written a tick early or late: the smallest image (H = 16, 9 pairs), an odd height (the last pair holds one real row: the store waves'
`nrows` guard, the load waves' zero row) and a grid capped at 256 workgroups with 258 images (two workgroups walk two images: ring slot
and staging parity carried across the image boundary, whose first pair is an idle tick).  The operand carries a channel with a negative
BatchNorm scale and one that is below zero everywhere after the affine (ReLU: exact zeros).

Per case, with BatchNorm on load + ReLU + statistics and in the plain form (which is handed the transformed operand, so that one float64
reference serves both):
  values      against F.conv2d in float64 on the bf16-rounded transformed input, TOL of tests/test_gpu_conv_tiles.py (bf16 output rounding);
              against the tiled kernel to the 8e-3 that test_row_streaming_3x3_kernel allows for another summation order;
  bits        on-load form == in-place bn_act pass + plain form, outputs and statistics words: the equality that
              tests/test_gpu_modules.py::test_row_streamed_3x3_bn_on_load_equals_in_place_pass asserts through the whole trunk
              (resnet.bn_apply_3x3 = "auto" against "pass"), here on the one launch;
  statistics  the words against the float64 mean / mean square of the kernel's own stored output (1e-5, as test_row_streaming_3x3_kernel),
              the finalized scale / shift against float64 from the words (4 ulp, as test_bn_finalize_against_f64_from_the_decoded_words);
              two launches give identical words and outputs."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu
TOL = 6e-3                       # tests/test_gpu_conv_tiles.py: bf16 output rounding (2^-9) relative to the tensor's scale
U32 = 2.0 ** -24
W, C = 64, 64
NEG, DEAD = 3, 5                 # input channels: negative BatchNorm scale; below zero everywhere after the affine
CASES = [(128, 16), (128, 17), (258, 16)]


@functools.lru_cache(None)
def _case(B, H):
    """(x, w, scale, shift, transformed input as the kernel forms it, float64 reference) - computed once per geometry, never modified"""
    g = torch.Generator().manual_seed(B + H)
    x = torch.randn(B, C, H, W, generator=g).bfloat16().float()
    w = (torch.randn(C, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5).bfloat16().float()
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    sc[NEG] = -sc[NEG]
    sh[DEAD] = -100.0            # |x| < 7 at these sizes, scale <= 1.5
    # fmaf(x, scale, shift) -> ReLU -> bf16: the product of two f32 is exact in f64
    xin = torch.relu(x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float().bfloat16().float()
    assert not xin[:, DEAD].any() and (xin[:, NEG] > 0).any()
    ref = F.conv2d(xin.double(), w.double(), None, 1, 1)
    return x, w, sc, sh, xin, ref


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()


def _finalized_from_words(stats, gamma, beta, count, eps=1e-5):
    from mhentropy_amd import ops
    tot = ops.stat_totals(stats).cpu().numpy()
    mean = tot[0] / count
    var = tot[1] / count - mean ** 2
    scale = gamma.double().numpy() / np.sqrt(var + float(np.float32(eps)))
    return scale, beta.double().numpy() - mean * scale, mean


@pytest.mark.parametrize("B,H", CASES)
def test_three_role_forward_forms(gpu_lib, B, H):
    from mhentropy_amd import ops, resnet
    x, w, sc, sh, xin, ref = _case(B, H)
    for mode in (0, 1):
        assert ops.conv_tile_choice(B, H, W, C, C, 3, 1, 1, torch.bfloat16, mode) == 9, "the launcher takes the row-streaming kernel here"
    xd = _nhwc(x)
    wd = resnet.pack_conv_weight(w, torch.bfloat16).cuda()
    scd, shd = sc.cuda(), sh.cuda()
    a = ops.bn_act(xd, scd, shd)                                      # the in-place pass of the library's other path
    flips = (a.float().cpu().permute(0, 3, 1, 2) != xin).float().mean().item()
    print(f"B={B} H={H}: bn_act pass vs the f64-formed operand: {flips:.2e} of the elements differ")
    assert flips == 0.0
    g = torch.Generator().manual_seed(7)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    n = float(B * H * W)
    got = {}
    for form, operand, kw in (("bn-on-load", xd, dict(in_scale=scd, in_shift=shd, relu_in=True)), ("plain", a, {})):
        runs = []
        for _ in range(2):
            stats = ops.stat_unit(C, "cuda")
            y = ops.conv2d_nhwc(operand, wd, 3, 3, 1, 1, stats=stats, **kw)
            runs.append((y, stats))
        (y, stats), (y2, stats2) = runs
        assert torch.equal(y, y2) and torch.equal(stats, stats2), f"{form}: two launches differ"
        yc = y.float().cpu().permute(0, 3, 1, 2)
        err = (yc.double() - ref).abs().max().item() / ref.abs().max().item()
        print(f"B={B} H={H} {form}: max|y - ref| / max|ref| = {err:.2e} (bound {TOL:.1e})")
        assert_close(yc, ref, TOL, what=form + ": values vs float64")
        ys = y.double().cpu().permute(0, 3, 1, 2)
        stt = ops.stat_totals(stats).cpu()
        assert_close(stt[0] / n, ys.mean((0, 2, 3)), 1e-5, 1e-5, what=form + ": batch mean")
        assert_close(stt[1] / n, (ys ** 2).mean((0, 2, 3)), 1e-5, what=form + ": batch E[x^2]")
        scale, shift, mean = _finalized_from_words(stats, gamma, beta, n)
        fs, fh = ops.bn_finalize(stats.clone(), gamma.cuda(), beta.cuda(), None, None, n)
        es = np.abs(fs.cpu().double().numpy() - scale) / (4 * U32 * np.abs(scale))
        eh = np.abs(fh.cpu().double().numpy() - shift) / (4 * U32 * (beta.double().abs().numpy() + np.abs(mean * scale)))
        print(f"B={B} H={H} {form}: finalized scale / shift error in units of the bound: {es.max():.2f} / {eh.max():.2f}")
        assert es.max() <= 1.0 and eh.max() <= 1.0
        got[form] = (y, stats)
    assert torch.equal(got["bn-on-load"][0], got["plain"][0]), "BatchNorm on the row load vs in-place pass + plain form: outputs"
    assert torch.equal(got["bn-on-load"][1], got["plain"][1]), "BatchNorm on the row load vs in-place pass + plain form: statistics words"
    forced = ops.conv2d_nhwc(xd, wd, 3, 3, 1, 1, tile=1, in_scale=scd, in_shift=shd, relu_in=True)
    same = torch.equal(forced, got["bn-on-load"][0])
    print(f"B={B} H={H}: tiled kernel (on-load form) bit-identical: {same}")
    assert_close(got["bn-on-load"][0].float().cpu(), forced.float().cpu(), 8e-3, what="vs the tiled kernel")
