"""GPU: the timing bracket (ops.TIMING / ops.KERNEL_TIMES, bench.py's live roofline pass and tools/train_lines.py): one record per
timed launch, under the name the launcher's kernel choice gives, with the algorithmic work in closed form and both events recorded."""
import pytest
import torch

from mhentropy_amd import _lib, ops, resnet

pytestmark = pytest.mark.gpu

B, H, W, Cin, Cout = 2, 8, 8, 64, 64
BF = torch.bfloat16


def _conv3x3():
    x = torch.randn(B, H, W, Cin, device="cuda").to(BF)
    w = resnet.pack_conv_weight(torch.randn(Cout, Cin, 3, 3), BF).cuda()
    d = _lib.ConvDesc(B, H, W, Cin, Cout, 3, 3, 1, 1, ops.BF16, 0, 0, 0, 0)
    y = torch.empty(B, H, W, Cout, device="cuda", dtype=BF)
    return (lambda: ops.conv2d_nhwc(x, w, 3, 3, 1, 1, out=y),
            lambda: (ops._conv_kernel_name(d, BF, 0), 2.0 * B * H * W * Cout * 3 * 3 * Cin, 2 * (x.numel() + y.numel() + w.numel())))


def _stem():
    x = torch.randn(2, 3, 32, 32, device="cuda")
    w = resnet.pack_stem_weight(torch.randn(64, 3, 7, 7), BF).cuda()
    return (lambda: ops.stem_conv7x7s2(x, w, BF),
            lambda: ("mhe::conv::stem_kernel<unsigned short>", 2.0 * 2 * 16 * 16 * 64 * 147, 4 * x.numel() + 2 * (2 * 16 * 16 * 64)))


def _wgrad1x1():
    x = torch.randn(B, H, W, Cin, device="cuda").to(BF)
    gy = torch.randn(B, H, W, Cout, device="cuda").to(BF)
    dw = torch.zeros(Cout, Cin, device="cuda")
    d = _lib.ConvDesc(B, H, W, Cin, Cout, 1, 1, 1, 0, ops.BF16, 0, 0)
    return (lambda: ops.conv_wgrad(x, gy, 1, 1, 1, 0, dw),
            lambda: (ops._wgrad_kernel_name(d), 2.0 * B * H * W * Cout * Cin, 2 * (x.numel() + gy.numel()) + 4 * Cout * Cin))


def _bn_act():
    x = torch.randn(B, H, W, Cout, device="cuda").to(BF)
    scale, shift = torch.rand(Cout, device="cuda") + 0.5, torch.randn(Cout, device="cuda")
    return (lambda: ops.bn_act(x, scale, shift),
            lambda: ("mhe::conv::bn_act_kernel<unsigned short>", 0.0, 2 * x.numel() * 2))


@pytest.mark.parametrize("case", [_conv3x3, _stem, _wgrad1x1, _bn_act], ids=["conv2d_3x3", "stem_conv7x7s2", "conv_wgrad_1x1", "bn_act"])
def test_one_record_per_timed_launch(gpu_lib, case):
    torch.manual_seed(0)
    run, expected = case()
    saved = ops.TIMING, ops.TIMING_DG, list(ops.KERNEL_TIMES)
    try:
        ops.TIMING = ops.TIMING_DG = False
        ops.KERNEL_TIMES.clear()
        run()
        assert ops.KERNEL_TIMES == []                       # off: nothing is logged
        ops.TIMING = True
        run()
        torch.cuda.synchronize()
        assert len(ops.KERNEL_TIMES) == 1
        name, flops, ev0, ev1, nbytes = ops.KERNEL_TIMES[0]
        print(name, flops, nbytes)
        assert (name, flops, nbytes) == expected()
        assert ev0.elapsed_time(ev1) >= 0                   # both events were recorded (elapsed_time raises otherwise)
    finally:
        ops.TIMING, ops.TIMING_DG = saved[0], saved[1]
        ops.KERNEL_TIMES[:] = saved[2]
