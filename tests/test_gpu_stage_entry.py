"""GPU: the stage entries of the forward-only ResNet-50 path (layer1 -> 2, 2 -> 3, 3 -> 4).

The fused tail kernels (csrc/conv_fuse.hip, csrc/conv_tail.hip forward form) can write the block output at even rows and even columns only,
compact - all that the next block's stride-2 1x1 shortcut reads - and a downsample block's bn3 and shortcut BatchNorm are finalized by one
launch (mhe_bn_finalize_pair_step).  Everything here is an exact comparison: the compact output is a subset of the same stored values,
conv1's output and statistics do not change, the merged finalize runs the same arithmetic per unit.

Geometry minima read from the launchers: bottleneck_tail needs Cb 64 / 128, Cout 64 / 128, pixels % 128 == 0; conv_tail needs
Cin % 64 == 0, Cin >= 128, Cout % 256 == 0, pixels % 128 == 0.  Both run at most 256 persistent workgroups, so 300 / 320 tiles give a
workgroup a second tile and leave the last round partial.  Pixels % 128 == 0 admits an odd map only with a batch that is a multiple of
128: B = 128 at 3 x 3 (9 tiles, ceil(3 / 2) = 2) is that case - the launchers do not reject odd maps as such."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 0x7FC1            # bf16 bit pattern no kernel output has (a NaN with a payload): the sentinel around the compact tensor
PAD = 4096


def _guarded(shape):
    """a tensor of `shape` inside a larger sentinel-filled buffer -> (view, whole buffer as int16 bits)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), SENT, dtype=torch.int16, device="cuda")
    return buf[PAD:PAD + n].view(torch.bfloat16).view(shape), buf


def _assert_guards(buf, what):
    assert bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all()), what + ": written outside the compact tensor"
    assert not bool((buf[PAD:-PAD] == SENT).any()), what + ": part of the compact tensor was not written"


def _bits(t):
    return t.contiguous().view(torch.int16)


# (B, H, W, Cb, N2): minimum; every workgroup a second tile, last round partial (300 tiles); odd map (9 tiles); the wider instantiations
FUSE_GEOMS = [(2, 8, 8, 64, 64), (2, 120, 160, 64, 64), (128, 3, 3, 64, 128), (2, 16, 16, 128, 64), (2, 16, 24, 128, 128)]


@pytest.mark.parametrize("affine2", [False, True], ids=["identity", "downsample-bn"])
@pytest.mark.parametrize("geom", FUSE_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_bottleneck_tail_quarter_output(gpu_lib, geom, affine2):
    """mhe_bottleneck_tail_quarter_nhwc against mhe_bottleneck_tail_nhwc: a_quarter == a[:, ::2, ::2], y1 and its statistics words equal"""
    from mhentropy_amd import ops, resnet
    B, H, W, Cb, N2 = geom
    C4 = 4 * Cb
    g = torch.Generator().manual_seed(B + H + Cb + N2)
    y2 = torch.randn(B, H, W, Cb, generator=g).bfloat16().cuda()
    idt = torch.randn(B, H, W, C4, generator=g).bfloat16().cuda()
    w3 = resnet.pack_conv_weight(torch.randn(C4, Cb, 1, 1, generator=g) * (2.0 / Cb) ** 0.5, torch.bfloat16).cuda()
    w1 = resnet.pack_conv_weight(torch.randn(N2, C4, 1, 1, generator=g) * (2.0 / C4) ** 0.5, torch.bfloat16).cuda()
    aff = lambda c: ((torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.3).cuda())
    bn2, bn3 = aff(Cb), aff(C4)
    ida = aff(C4) if affine2 else None
    assert ops.bottleneck_tail_supported(B, H, W, Cb, N2)
    st_f, st_q = ops.stat_unit(N2, "cuda"), ops.stat_unit(N2, "cuda")
    a_full, y1_full = ops.bottleneck_tail(y2, bn2, w3, bn3, idt, ida, w1, stats=st_f)
    aq, buf = _guarded((B, (H + 1) // 2, (W + 1) // 2, C4))
    a_q, y1_q = ops.bottleneck_tail(y2, bn2, w3, bn3, idt, ida, w1, stats=st_q, quarter=True, a_out=aq)
    torch.cuda.synchronize()
    _assert_guards(buf, "bottleneck_tail quarter")
    assert torch.equal(_bits(a_q), _bits(a_full[:, ::2, ::2, :])), "compact block output"
    assert torch.equal(_bits(y1_q), _bits(y1_full)), "conv1 output"
    assert torch.equal(st_q, st_f) and bool((st_f != 0).any()), "conv1 statistics words"


# (B, H, W, Cin, Cout): minimum; 300 tiles in one column; 2 x 160 tiles in the XCD-aware order (only column tile 0 writes the operand); odd map
TAIL_GEOMS = [(2, 8, 8, 128, 256), (2, 120, 160, 128, 256), (2, 80, 128, 128, 512), (128, 3, 3, 192, 256)]


@pytest.mark.parametrize("affine2", [False, True], ids=["identity", "downsample-bn"])
@pytest.mark.parametrize("geom", TAIL_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_conv_tail_quarter_output(gpu_lib, geom, affine2):
    """mhe_conv1x1_residual_in_quarter_nhwc against mhe_conv1x1_residual_in_nhwc on the residual-tail kernel (variant 10)"""
    from mhentropy_amd import ops, resnet
    B, H, W, Cin, Cout = geom
    g = torch.Generator().manual_seed(B + H + Cin + Cout)
    x = torch.randn(B, H, W, Cin, generator=g).bfloat16().cuda()
    x2 = torch.randn(B, H, W, Cin, generator=g).bfloat16().cuda()
    w = resnet.pack_conv_weight(torch.randn(Cout, Cin, 1, 1, generator=g) * (2.0 / Cin) ** 0.5, torch.bfloat16).cuda()
    aff = lambda: ((torch.rand(Cin, generator=g) + 0.5).cuda(), (torch.randn(Cin, generator=g) * 0.3).cuda())
    (sc, sh), (s2, h2) = aff(), (aff() if affine2 else (None, None))
    assert ops.conv_tile_choice(B, H, W, Cin, Cout, 1, 1, 0, torch.bfloat16, 2) == 10
    st_f, st_q = ops.stat_unit(Cout, "cuda"), ops.stat_unit(Cout, "cuda")
    a_full = torch.empty_like(x)
    y_full = ops.conv1x1_residual_in(x, x2, w, sc, sh, s2, h2, a_out=a_full, stats=st_f)
    aq, buf = _guarded((B, (H + 1) // 2, (W + 1) // 2, Cin))
    y_q = ops.conv1x1_residual_in(x, x2, w, sc, sh, s2, h2, a_out=aq, stats=st_q, quarter=True)
    torch.cuda.synchronize()
    _assert_guards(buf, "conv_tail quarter")
    assert torch.equal(_bits(aq), _bits(a_full[:, ::2, ::2, :])), "compact operand"
    assert torch.equal(_bits(y_q), _bits(y_full)), "conv1 output"
    assert torch.equal(st_q, st_f) and bool((st_f != 0).any()), "conv1 statistics words"


def test_quarter_output_is_refused_off_the_tail_kernel(gpu_lib):
    """a geometry the residual-tail kernel does not take (32 pixels) must be an error, never a launch of a kernel that knows the full layout only"""
    from mhentropy_amd import _lib, ops
    x = torch.zeros(2, 4, 4, 128, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(256, 128, dtype=torch.bfloat16, device="cuda")
    one = torch.ones(128, device="cuda")
    aq, buf = _guarded((2, 2, 2, 128))
    with pytest.raises(_lib.MheError):
        ops.conv1x1_residual_in(x, x, w, one, one, a_out=aq, quarter=True)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


def _unit(C, seed, n=4096.0):
    g = torch.Generator().manual_seed(seed)
    S = 64
    s1 = torch.randn(S, C, generator=g) * 3.0
    s2 = s1 ** 2 / (n / S) + torch.rand(S, C, generator=g) * 40.0 + 1.0
    from mhentropy_amd import ops
    return ops.stat_from_float(torch.stack([s1, s2], 1)).cuda(), (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()


@pytest.mark.parametrize("marked", [None, 0, 1], ids=["clean", "nan-unit0", "nan-unit1"])
def test_pair_finalize_equals_two_launches(gpu_lib, marked):
    """mhe_bn_finalize_pair_step against two mhe_bn_finalize_step launches: different C (30 is no multiple of the 4 channels a workgroup owns),
    different counts, bit-equal affine / running buffers / counters, accumulators cleared; the accumulators' non-finite marker in one unit
    gives NaN in that unit and leaves the other alone"""
    from mhentropy_amd import ops
    out = []
    for pair in (False, True):
        units = []
        for k, (C, n) in enumerate(((64, 4096.0), (30, 1024.0))):
            st, gamma, beta = _unit(C, 11 + k, n)
            if marked == k:
                st[0, 5, 1, 3] = 1 << 62
            units.append((st, gamma, beta, torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), n, torch.full((), 7, dtype=torch.int64, device="cuda")))
        if pair:
            affs = ops.bn_finalize_pair(units[0], units[1], 0.1, 1e-5, clear=True)
        else:
            affs = [ops.bn_finalize(u[0], u[1], u[2], u[3], u[4], u[5], 0.1, 1e-5, clear=True, num_batches_tracked=u[6]) for u in units]
        torch.cuda.synchronize()
        out.append([(a[0], a[1], u[3], u[4], u[6], u[0]) for a, u in zip(affs, units)])
    for k in range(2):
        for name, t0, t1 in zip(("scale", "shift", "running_mean", "running_var", "num_batches_tracked", "stats"), out[0][k], out[1][k]):
            assert torch.equal(t0.view(torch.int32) if t0.dtype == torch.float32 else t0, t1.view(torch.int32) if t1.dtype == torch.float32 else t1), (k, name)
        scale, shift, rmean, rvar, nbt, st = out[1][k]
        assert int(nbt) == 8 and not bool(st.any())
        if marked == k:
            assert bool(torch.isnan(scale[3])) and bool(torch.isnan(rvar[3])) and int(torch.isnan(scale).sum()) == 1
        else:
            assert bool(torch.isfinite(scale).all() and torch.isfinite(shift).all() and torch.isfinite(rmean).all() and torch.isfinite(rvar).all())


def test_trunk_with_stage_entries_equals_the_full_form(gpu_lib):
    """ResNet-50, bf16, train mode, B = 2 at 128 x 128 - the smallest input at which all three stage boundaries run through the fused
    kernels (layer3's 8 x 8 maps are the 128 pixels the residual-tail kernel needs).  MHE_STAGE_ENTRY on against off: feature and every
    BatchNorm buffer bit-equal, the statistics arena all zero after the pass (the merged finalize cleared both of its units)."""
    from mhentropy_amd import ops, resnet
    torch.manual_seed(3)
    trunk = resnet.resnet50(compute_dtype=torch.bfloat16).cuda().train()
    B, S = 2, 128
    # the stage boundaries do run the kernels with the compact output at this size
    assert ops.bottleneck_tail_supported(B, S // 4, S // 4, 64, 128)
    assert ops.conv_tile_choice(B, S // 8, S // 8, 512, 256, 1, 1, 0, torch.bfloat16, 2) == 10
    assert ops.conv_tile_choice(B, S // 16, S // 16, 1024, 512, 1, 1, 0, torch.bfloat16, 2) == 10
    assert trunk.stage_entry and trunk.fuse_tail and trunk.fuse_recompute
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(4)).cuda()
    state0 = {k: v.clone() for k, v in trunk.state_dict().items()}
    res = {}
    for on in (True, False):
        trunk.load_state_dict(state0)
        trunk.stage_entry = on
        with torch.no_grad():
            f = trunk(x).clone()
        torch.cuda.synchronize()
        bufs = {k: v.clone() for k, v in trunk.state_dict().items() if "running_" in k or "num_batches_tracked" in k}
        assert not bool(trunk._pool.buf.any()), "statistics arena not cleared"
        res[on] = (f, bufs)
    assert torch.isfinite(res[True][0]).all()
    assert torch.equal(res[True][0].view(torch.int32), res[False][0].view(torch.int32)), "feature"
    assert len(res[True][1]) == 3 * 53
    for k, v in res[True][1].items():
        assert torch.equal(v, res[False][1][k]), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(state0[k]) + 1, k
