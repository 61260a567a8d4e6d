"""GPU parity of the train step's reverse kernels against torch autograd
run on the CPU oracle (the reference differentiates the same arithmetic with autograd,
hand/CrossModalHand.py:455-470).  fp32 tolerance 1e-4 relative to the tensor's scale."""
import numpy as np
import pytest
import torch

from conftest import load_golden, assert_close
from mhentropy_amd import synth, mano_pack

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _tables(seed=0):
    t = synth.mano_tables(seed)
    blob = _dev(mano_pack.pack_tables(t["shapedirs"], t["posedirs"], t["v_template"], t["J_regressor"], t["weights"],
                                      t["hands_components"][:45], t["hands_mean"]))
    from oracle import mano_ref
    return blob, mano_ref.tables_from_numpy(t)


@pytest.mark.parametrize("B,N,scale", [(3, 4, 0.3), (2, 5, 1.5)])
def test_mano_likelihood_backward_matches_autograd(gpu_lib, B, N, scale):
    """d sum_b g_b log_p_b / d (th45, det) with log_p_b the mean over the image's N hypotheses;
    scale=1.5 pushes th45/beta/th3 outside the soft priors' boxes so their gradients are exercised."""
    from mhentropy_amd import ops
    from oracle import network_ref
    blob, tb = _tables()
    rng = np.random.default_rng(5)
    R = N * B
    th45 = torch.as_tensor(rng.normal(0, scale, (R, 45)).astype(np.float32))
    det = torch.as_tensor(rng.normal(0, 1.0, (B, 16)).astype(np.float32))
    det[:, 3:13] *= 0.02 * scale
    det[:, 0:3] *= 2.0 * scale
    det[:, 13:] *= 0.2
    _, yn = synth.batch(3, B, with_image=False)
    y = {k: torch.as_tensor(v) for k, v in yn.items()}
    g = torch.as_tensor(rng.normal(0, 1, (B,)).astype(np.float32))
    th45_r, det_r = th45.clone().requires_grad_(True), det.clone().requires_grad_(True)
    z = network_ref.combine_z(det_r.repeat(N, 1), th45_r)
    lp = network_ref.forward_log_p(tb, z, y, N)["log_p"].reshape(N, B).mean(0)
    (lp * g).sum().backward()
    g45, gdet = ops.mano_joints_bwd(_dev(th45), _dev(det), blob, _dev(yn["crop_uv"]), _dev(yn["vis"]), _dev(g), N)
    assert_close(g45.cpu(), th45_r.grad, RTOL, what="d/d th45")
    assert_close(gdet.cpu(), det_r.grad, RTOL, what="d/d det")


def _model_and_state(backbone, h, steps, seed=0, dtype=torch.float32):
    from mhentropy_amd import harness
    tables = synth.mano_tables(0)
    model = harness.build_mhent(backbone=backbone, h_dims=(h, h), num_steps=steps, tables=tables, compute_dtype=dtype)
    sd = {}
    sd.update({"feat_extractor.res." + k: v for k, v in synth.resnet_state(seed, backbone).items()})
    sd.update({k: v for k, v in synth.head_state(seed + 1, 512 if backbone == "resnet18" else 2048).items()})
    sd.update({"q_z_giv_i." + k: v for k, v in synth.flow_state(seed + 2, 45, 512, (h, h), steps).items()})
    missing, unexpected = model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith("mano_dec") for k in missing), missing
    return model.cuda().train(), {k: torch.as_tensor(v) for k, v in sd.items()}


def _grad_report(ts, model, ref_grads):
    """per parameter: (max-abs error / max-abs reference, relative L2 error, name)"""
    rows = []
    for name, p in model.named_parameters():
        if name not in ref_grads:
            continue
        got, want = ts.grad_of(p).cpu().double(), ref_grads[name].double()
        if want.abs().max().item() < 1e-12:
            assert got.abs().max().item() < 1e-9, name
            continue
        rows.append(((got - want).abs().max().item() / want.abs().max().item(), ((got - want).norm() / want.norm()).item(), name))
    rows.sort(reverse=True)
    return rows


@pytest.mark.parametrize("backbone,h,steps,B,N", [("resnet18", 64, 2, 2, 4), ("resnet50", 512, 6, 3, 4)])
def test_train_step_gradients_match_autograd(gpu_lib, backbone, h, steps, B, N):
    """every parameter gradient of total = mean(-log_p) against torch autograd on the CPU oracle"""
    from mhentropy_amd.train import TrainStep
    from oracle import train_ref, mano_ref
    model, sd = _model_and_state(backbone, h, steps)
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0))
    xn, yn = synth.batch(7, B, image_size=64 if backbone == "resnet50" else 96)
    z0 = synth.noise(7, N * B)
    x, y = torch.as_tensor(xn), {k: torch.as_tensor(v) for k, v in yn.items()}
    out_ref, total_ref, grads, _ = train_ref.loss_and_grads(sd, tb, x, y, torch.as_tensor(z0), N, arch=backbone)
    ts = TrainStep(model)
    out = ts.forward_backward(x.cuda(), {k: v.cuda() for k, v in y.items()}, noise=torch.as_tensor(z0).cuda(), N=N)
    assert_close(out["log_p"].cpu(), out_ref["log_p"].detach(), 2e-4, what="log_p")
    assert_close(ts.z0_recovered.cpu(), z0, 1e-4, what="flow input recovered by the reverse pass")
    rows = _grad_report(ts, model, grads)
    print("worst relative gradient errors:", rows[:5])
    if backbone == "resnet18":
        bad = [r for r in rows if r[0] > 2e-3]
        assert not bad, f"{len(bad)} of {len(rows)} parameter gradients off (max-abs rel, L2 rel, name): {bad[:8]}"
    else:
        # 50 layers of train-mode BatchNorm over 3 x (2 x 2) samples: individual gradient ELEMENTS are ill-conditioned
        # (a ReLU / leaky-ReLU / max-pool decision that flips under fp32 round-off changes them by O(1)).  Yardstick,
        # measured with this oracle on the same inputs: its own fp32 and fp64 runs differ by up to 0.28 max-abs-relative
        # and 2.2e-2 in relative L2, 173 of 407 tensors beyond 2e-3.  Hence a norm-wise bound here, element-wise
        # bounds on ResNet-18 above, and element-wise tests of every reverse kernel at ResNet-50's shapes.
        assert max(r[1] for r in rows) < 6e-2, sorted(rows, key=lambda r: -r[1])[:5]
        assert sorted(r[1] for r in rows)[len(rows) // 2] < 5e-3
        heads = [r for r in rows if not r[2].startswith("feat_extractor.res.") and not r[2].startswith("q_z_giv_i")]
        assert all(r[0] < 1e-2 for r in heads), heads           # (they see the trunk's output, hence a little of its noise)


def _nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


CONV_CASES = [(64, 64, 3, 1, 1, 16, 4), (128, 128, 3, 2, 1, 16, 3), (1024, 2048, 1, 1, 0, 4, 4), (256, 512, 1, 2, 0, 8, 2),
              (2048, 512, 1, 1, 0, 4, 4), (512, 512, 3, 1, 1, 8, 2), (64, 256, 1, 1, 0, 16, 2)]


@pytest.mark.parametrize("slabs", [True, False], ids=["partial-slabs", "atomics"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Cin,Cout,k,stride,pad,H,B", CONV_CASES)
def test_conv_weight_and_data_gradients(gpu_lib, Cin, Cout, k, stride, pad, H, B, dt, slabs, monkeypatch):
    """mhe_conv_wgrad_nhwc and the data gradient (forward kernel on flipped / transposed weights) vs autograd of
    F.conv2d on the same (storage-rounded) operands"""
    from mhentropy_amd import ops, train
    import torch.nn.functional as F
    monkeypatch.setattr(ops, "WGRAD_SLABS", slabs)       # pixel-range partials through workspace slabs + reducer, or f32 atomics
    g = torch.Generator().manual_seed(Cin + Cout + k)
    x = torch.randn(B, Cin, H, H, generator=g).to(dt).float().requires_grad_(True)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(dt).float().requires_grad_(True)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    gy = torch.randn(y.shape, generator=g).to(dt).float()
    y.backward(gy)
    dw = torch.ones(Cout, k * k * Cin, device="cuda")              # dW += : the ones must survive
    ops.conv_wgrad(_nhwc(x.detach(), dt), _nhwc(gy, dt), k, k, stride, pad, dw)
    want_dw = w.grad.permute(0, 2, 3, 1).reshape(Cout, -1)
    assert_close(dw.cpu() - 1.0, want_dw, 2e-5 if dt == torch.float32 else 2e-5, what="dW")     # bf16 operands, f32 accumulate: exact products
    bke = 32 if dt == torch.float32 else 64
    idx = torch.arange(w.numel()).view(w.shape)
    di = train.dgrad_operand_index(idx)
    wd = torch.zeros(Cin, (di.shape[1] + bke - 1) // bke * bke)
    wd[:, :di.shape[1]] = w.detach().reshape(-1)[di]
    res = torch.randn(B, Cin, H, H, generator=g).to(dt).float()
    gx = train.conv_dgrad(_nhwc(gy, dt), wd.to(dt).cuda().contiguous(), k, stride, pad, H, H, residual=_nhwc(res, dt))
    want = (x.grad + res).permute(0, 2, 3, 1)
    assert_close(gx.float().cpu(), want, 1e-4 if dt == torch.float32 else 1.5e-2, what="dX + residual")
    if k == 3 and stride == 2:          # the parity-split form (no zero-dilated copy of gy): same result
        w_s2 = []
        for tb in train.dgrad_s2_operand_indices(idx):
            f2 = torch.zeros(Cin, (tb.shape[1] + bke - 1) // bke * bke)
            f2[:, :tb.shape[1]] = w.detach().reshape(-1)[tb]
            w_s2.append(f2.to(dt).cuda().contiguous())
        gx2 = train.conv_dgrad(_nhwc(gy, dt), None, k, stride, pad, H, H, residual=_nhwc(res, dt), w_s2=w_s2)
        assert_close(gx2.float().cpu(), want, 1e-4 if dt == torch.float32 else 1.5e-2, what="dX + residual, parity classes")


@pytest.mark.parametrize("tile", [0, 2, 3, 8])
def test_stride2_dgrad_parity_classes_gate_and_bn_sums(gpu_lib, tile):
    """mhe_conv3x3s2_dgrad_nhwc with the ReLU gate, residual and BatchNorm-reverse sums of the data-gradient epilogue, every output
    written at its strided position: against the zero-dilated form through the same epilogue (train.conv_dgrad's old path) and
    against autograd; tile forces the 128x128 / 256x256 register-staged kernels and the phase-pipelined one (partial tiles)"""
    from mhentropy_amd import ops, train
    import torch.nn.functional as F
    dt, B, Cin, Cout, H = torch.bfloat16, 3, 128, 256, 24
    g = torch.Generator().manual_seed(11)
    x = torch.relu(torch.randn(B, Cin, H, H, generator=g)).to(dt).float().requires_grad_(True)        # post-ReLU input = the gate
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).to(dt).float()
    y = F.conv2d(x, w, stride=2, padding=1)
    gy = torch.randn(y.shape, generator=g).to(dt).float()
    y.backward(gy)
    res = torch.randn(B, Cin, H, H, generator=g).to(dt).float()
    idx = torch.arange(w.numel()).view(w.shape)
    pack = lambda tb: torch.nn.functional.pad(w.reshape(-1)[tb], (0, (-tb.shape[1]) % 64)).to(dt).cuda().contiguous()
    w_s2 = [pack(tb) for tb in train.dgrad_s2_operand_indices(idx)]
    wd = pack(train.dgrad_operand_index(idx))
    bn_y = torch.randn(B, H, H, Cin, generator=g).to(dt).cuda()
    mi = torch.stack([torch.randn(Cin, generator=g) * 0.1, torch.rand(Cin, generator=g) + 0.5]).cuda().contiguous()
    st_new, st_old = (ops.stat_unit(Cin, "cuda") for _ in range(2))
    mask = _nhwc(x.detach(), dt)
    new = ops.conv3x3s2_dgrad(_nhwc(gy, dt), w_s2, residual=_nhwc(res, dt), mask=mask, bn=[(bn_y, mi, st_new)], tile=tile)
    old = ops.conv2d_nhwc(ops.upsample2(_nhwc(gy, dt), H, H), wd, 3, 3, 1, 1, residual=_nhwc(res, dt), mask=mask, bn=[(bn_y, mi, st_old)])
    want = ((x.grad + res) * (x.detach() > 0)).permute(0, 2, 3, 1)
    assert_close(new.float().cpu(), want, 1.5e-2, what="gated dX + residual")
    assert_close(new.float().cpu(), old.float().cpu(), 8e-3, what="parity classes vs zero-dilated form")      # both round to bf16 once
    sn, so = ops.stat_totals(st_new).cpu(), ops.stat_totals(st_old).cpu()
    gf = new.float().cpu().reshape(-1, Cin)
    xh = (bn_y.float().cpu().reshape(-1, Cin) - mi[0].cpu()) * mi[1].cpu()
    bound = lambda t: 5 * 2.0 ** -9 * t.pow(2).sum(0).sqrt() + 1e-4        # the kernel sums the values before their bf16 rounding
    assert ((sn[0] - gf.sum(0)).abs() <= bound(gf)).all() and ((sn[1] - (gf * xh).sum(0)).abs() <= bound(gf * xh)).all()
    assert ((sn - so).abs() <= 2 * torch.stack([bound(gf), bound(gf * xh)])).all()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,P", [(64, 4096), (256, 1000), (512, 640), (1024, 300), (2048, 200)])
def test_batchnorm_relu_backward(gpu_lib, C, P, dt):
    from mhentropy_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(C)
    y = (torch.randn(P, C, generator=g) * 2 + 0.5).to(dt).float().requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.3).requires_grad_(True)
    idt = torch.randn(P, C, generator=g).to(dt).float()
    z = F.batch_norm(y, None, None, gamma, beta, training=True, eps=1e-5)
    a = F.relu(z + idt)
    go = torch.randn(P, C, generator=g).to(dt).float()
    a.backward(go)
    mean, var = y.detach().mean(0), y.detach().var(0, unbiased=False)
    mi = torch.stack([mean, 1 / torch.sqrt(var + 1e-5)]).cuda().contiguous()
    st = ops.stat_unit(C, "cuda")
    dga, dbe = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    yy = y.detach().to(dt).cuda().view(1, 1, P, C)
    gy, gm = ops.bn_backward(go.to(dt).cuda().view(1, 1, P, C), a.detach().to(dt).cuda().view(1, 1, P, C), yy, mi, gamma.detach().cuda(), st,
                             dga, dbe, want_masked=True)
    tol = 1e-4 if dt == torch.float32 else 1e-2
    assert_close(dga.cpu(), gamma.grad, tol, what="dgamma"); assert_close(dbe.cpu(), beta.grad, tol, what="dbeta")
    assert_close(gy.float().cpu().view(P, C), y.grad, tol, what="dy")
    assert_close(gm.float().cpu().view(P, C), go * (a.detach() > 0), 1e-6, what="masked g")


@pytest.mark.parametrize("B,S", [(2, 32), (3, 40)])
def test_stem_weight_gradient_over_pixel_pairs(gpu_lib, B, S):
    """mhe_conv_wgrad_rect_nhwc as the bf16 train step uses it: the 7x7 / stride-2 / pad-3 stem read as a 7 x 4 / stride (2, 1) / pad (3, 2)
    convolution over pixel pairs (two neighbours x 3 channels padded to 4); un-mapped through dW[co][c][kh][2 kw' + par - 1] it must equal
    torch's weight gradient of the stem on the same (bf16-rounded) operands, and the generic kernel's result on the 8-channel copy"""
    from mhentropy_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(B * S)
    bf = torch.bfloat16
    x = torch.randn(B, 3, S, S, generator=g)
    xr = x.to(bf).float()
    gy = torch.randn(B, 64, S // 2, S // 2, generator=g).to(bf).float()
    w = torch.zeros(64, 3, 7, 7, requires_grad=True)
    F.conv2d(xr, w, stride=2, padding=3).backward(gy)
    xd = x.cuda()
    xp = ops.nchw_to_nhwc(xd, bf, cpad=4)
    assert torch.equal(xp[..., :3].float().cpu(), xr.permute(0, 2, 3, 1)) and not xp[..., 3].any()
    gyd = gy.permute(0, 2, 3, 1).contiguous().to(bf).cuda()
    dw = torch.zeros(64, 7 * 4 * 8, device="cuda")
    ops.conv_wgrad_rect(xp.view(B, S, S // 2, 8), gyd, 7, 4, 2, 1, 3, 2, dw)
    d5 = dw.view(64, 7, 4, 2, 4).cpu()                      # [co][kh][kw'][parity][c]
    got = torch.zeros(64, 3, 7, 7)
    for kw in range(7):
        got[:, :, :, kw] = d5[:, :, (kw + 1) // 2, (kw + 1) % 2, :3].permute(0, 2, 1)
    assert_close(got, w.grad, 2e-5, what="stem weight gradient over pixel pairs")
    # the columns that correspond to no tap (kw = -1) or to the padding channel: whatever the padding pixels / zero channel contribute
    assert not d5[..., 3].any()
    dw8 = torch.zeros(64, 7 * 7 * 8, device="cuda")
    ops.conv_wgrad(ops.nchw_to_nhwc(xd, bf), gyd, 7, 7, 2, 3, dw8)
    assert_close(got, dw8.view(64, 7, 7, 8)[..., :3].permute(0, 3, 1, 2).cpu(), 2e-5, what="vs the generic kernel on 8 padded channels")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(18, 18), (19, 22)])
def test_stem_pool_with_batchnorm_folded_in(gpu_lib, dt, H, W):
    """mhe_maxpool3x3s2_idx_affine_nhwc / mhe_maxpool3x3s2_bwd_bn_nhwc against the separate passes they replace in the train step
    (BatchNorm apply, pool with winners; pool scatter, BatchNorm-reverse reduction with the ReLU gate): pooled values, winning taps and the
    gated gradient to the bit, the per-channel sums to summation order; and against torch autograd through relu(bn) -> max_pool2d."""
    from mhentropy_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(11)
    B, C = 3, 64
    y0 = torch.randn(B, C, H, W, generator=g).to(dt).float()
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    scale[::7] *= -1.0                                                  # negative BatchNorm weights: relu(bn) is decreasing in the raw output
    mean, invstd = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    y0d, sc, sh = _nhwc(y0, dt), scale.cuda(), shift.cuda()
    r0 = ops.bn_act(y0d, sc, sh, relu=True)
    a_ref, idx_ref = ops.maxpool3x3s2_idx(r0)
    a, idx = ops.maxpool3x3s2_idx(y0d, sc, sh)
    assert torch.equal(a, a_ref) and torch.equal(idx, idx_ref)
    gy = torch.randn(a.shape, generator=g).to(dt).cuda()
    mi = torch.stack([mean, invstd]).cuda().contiguous()
    st = ops.stat_unit(C, "cuda")
    gx = ops.maxpool3x3s2_bwd_bn(gy, idx, y0d, sc, sh, mi, st)
    g_sep = ops.maxpool3x3s2_bwd(gy, idx_ref, H, W)
    assert torch.equal(gx, torch.where(r0 > 0, g_sep, torch.zeros_like(g_sep)))
    st_ref = torch.zeros_like(st)
    from mhentropy_amd import _lib
    ops.check(_lib.lib().mhe_bn_bwd_reduce_nhwc(ops._ptr(g_sep), ops._ptr(r0), ops._ptr(y0d), ops._ptr(mi), ops._ptr(st_ref), B * H * W, C,
                                                ops.dtype_code(dt), ops._stream()), "mhe_bn_bwd_reduce_nhwc")
    assert_close(ops.stat_totals(st).cpu(), ops.stat_totals(st_ref).cpu(), 1e-5, what="BatchNorm-reverse sums")
    # the two-walk form of the train step: sums without the scattered gradient, then the BatchNorm reverse applied where it is formed -
    # to the bit what the apply pass makes of the stored gradient
    st2 = torch.zeros_like(st)
    assert ops.maxpool3x3s2_bwd_bn(gy, idx, y0d, sc, sh, mi, st2, want_gx=False) is None
    assert_close(ops.stat_totals(st2).cpu(), ops.stat_totals(st).cpu(), 1e-6, what="sums of the walk that stores nothing")
    # round 4: the same sums from the POOLED tensors alone (the gradient is non-zero at the winners only): the pool also keeps the raw
    # input at every winner.  f32: equal to summation order; bf16: where two windows picked one pixel the walk rounds the sum of their
    # gradients to bf16 first (as the apply walk stores it), here the terms enter exactly - a last-bit difference on those pixels
    a3, idx3, win = ops.maxpool3x3s2_idx_win(y0d, sc, sh)
    assert torch.equal(a3, a) and torch.equal(idx3, idx)
    ho, wo = torch.meshgrid(torch.arange(a.shape[1]), torch.arange(a.shape[2]), indexing="ij")
    hi = (2 * ho.view(1, -1, a.shape[2], 1) - 1 + idx.cpu().long() // 3).clamp(0, H - 1)
    wi = (2 * wo.view(1, a.shape[1], -1, 1) - 1 + idx.cpu().long() % 3).clamp(0, W - 1)
    bi = torch.arange(B).view(-1, 1, 1, 1).expand_as(hi)
    ci = torch.arange(C).view(1, 1, 1, -1).expand_as(hi)
    assert torch.equal(win.cpu(), y0d.cpu()[bi, hi, wi, ci])
    st3 = torch.zeros_like(st)
    ops.pooled_bn_sums(gy, a, win, mi, st3)
    t3, t1 = ops.stat_totals(st3).cpu(), ops.stat_totals(st).cpu()
    assert_close(t3, t1, 1e-5 if dt == torch.float32 else 2e-3, what="sums from the pooled tensors")
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    coef = ops.bn_bwd_coef(st, gamma, mi, dg, db, B * H * W)
    dg1, db1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    gy_ref = ops.bn_backward(gx, None, y0d, mi, gamma, st, dg1, db1, reduced=True)
    gy_two = ops.maxpool3x3s2_bwd_bn_apply(gy, idx, y0d, sc, sh, mi, coef)
    assert torch.equal(gy_two, gy_ref) and torch.equal(dg, dg1) and torch.equal(db, db1)
    # torch autograd through the same composition (f32): values up to the storage rounding of dt
    yt = y0.clone().requires_grad_(True)
    rt = torch.relu(yt * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    pt = F.max_pool2d(rt.detach().to(dt).float() + (rt - rt.detach()), 3, 2, 1)  # pool over the values as stored, gradient through relu(bn)
    assert_close(a.float().cpu(), pt.detach().permute(0, 2, 3, 1), 1e-6 if dt == torch.float32 else 8e-3, what="pooled activation")   # torch: mul + add, here fma
    (pt * gy.float().cpu().permute(0, 3, 1, 2)).sum().backward()
    want = yt.grad / scale.view(1, -1, 1, 1)                            # d/d(relu(bn) input): the gated pool gradient
    assert_close(gx.float().cpu(), want.permute(0, 2, 3, 1), 1e-6 if dt == torch.float32 else 1e-2, what="gated pool gradient")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_pool_backward(gpu_lib, dt):
    from mhentropy_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(2, 64, 18, 18, generator=g)).to(dt).float().requires_grad_(True)     # ties at zero, as after ReLU
    y = F.max_pool2d(x, 3, 2, 1)
    gy = torch.randn(y.shape, generator=g).to(dt).float()
    y.backward(gy)
    yy, idx = ops.maxpool3x3s2_idx(_nhwc(x.detach(), dt))
    assert_close(yy.float().cpu(), y.detach().permute(0, 2, 3, 1), 0, what="maxpool")
    gx = ops.maxpool3x3s2_bwd(_nhwc(gy, dt), idx, 18, 18)
    assert_close(gx.float().cpu(), x.grad.permute(0, 2, 3, 1), 1e-6 if dt == torch.float32 else 1e-2, what="maxpool backward")
    gf = torch.randn(3, 128, generator=g)
    ga = ops.avgpool_bwd(gf.cuda(), 16, dt)
    assert_close(ga.float().cpu(), (gf / 16)[:, None, :].expand(3, 16, 128), 1e-6 if dt == torch.float32 else 4e-3, what="avgpool backward")


def test_clip_adam_matches_torch(gpu_lib):
    from mhentropy_amd import ops
    g = torch.Generator().manual_seed(0)
    n = 100003
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) * s for s in (0.001, 3.0, 0.5)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=2e-4)
    P, M, V = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    step, sq = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    for gr in grads:
        ref.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_([ref], 1.0)
        opt.step()
        G = gr.clone().cuda()
        ops.train_tick(step, sq); ops.sqnorm(G, sq)
        ops.adam_step(P, G, M, V, sq, step, 2e-4, max_norm=1.0)
        assert abs(sq.item() ** 0.5 - gr.norm().item()) < 1e-3 * gr.norm().item()
    assert_close(P.cpu(), ref.detach(), 1e-6, what="parameters after 3 clipped Adam steps")
    assert (P.cpu() - p0).abs().max() > 1e-4


def test_full_step_matches_oracle_clip_adam(gpu_lib):
    """TrainStep.step (forward, reverse, clip_grad_norm_(1.0), Adam lr 2e-4) against the oracle's train step
    (hand/CrossModalHand.py:455-470).  Adam's first update is lr * g / (|g| + eps): elements whose gradient is
    ~0 may take either sign, so the bound is on the bulk of the elements."""
    from mhentropy_amd.train import TrainStep
    from oracle import train_ref, mano_ref
    B, N = 2, 4
    model, sd = _model_and_state("resnet18", 64, 2)
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0))
    xn, yn = synth.batch(7, B, image_size=96)
    z0 = torch.as_tensor(synth.noise(7, N * B))
    x, y = torch.as_tensor(xn), {k: torch.as_tensor(v) for k, v in yn.items()}
    _, _, grads, buffers = train_ref.loss_and_grads(sd, tb, x, y, z0, N, arch="resnet18")
    params = {k: v for k, v in sd.items() if k in grads}
    new, norm = train_ref.clip_and_adam(params, grads, {})
    ts = TrainStep(model)
    ts.step(x.cuda(), {k: v.cuda() for k, v in y.items()}, noise=z0.cuda(), N=N)
    assert abs(ts.sq.item() ** 0.5 - norm.item()) < 2e-3 * norm.item(), (ts.sq.item() ** 0.5, norm.item())
    tot = off = 0
    for name, p in model.named_parameters():
        if name in new and grads[name].abs().max() > 0:
            d = (p.detach().cpu() - new[name]).abs()
            sig = grads[name].abs() > 1e-4 * grads[name].abs().max()         # elements with a meaningful gradient
            tot += int(sig.sum()); off += int((d[sig] > 2e-5).sum())
            assert (p.detach().cpu() - sd[name]).abs().max() > 1e-5, name + " did not move"
    assert off < 2e-3 * tot, (off, tot)
    # BatchNorm running statistics advanced (their values are pinned by test_gpu_modules' trunk tests)
    for k in ("feat_extractor.res.bn1.running_mean", "feat_extractor.res.layer4.1.bn2.running_var"):
        assert (dict(model.named_buffers())[k].cpu() - sd[k]).abs().max() > 1e-6, k
    assert int(model.feat_extractor.res.bn1.num_batches_tracked) == 1
    # dead head: no gradient, no movement
    assert (model.feat_extractor.l2[0].weight.detach().cpu() == sd["feat_extractor.l2.0.weight"]).all()


def test_bf16_flow_reverse_close_to_fp32_autograd(gpu_lib):
    """performance mode of the flow (bf16 operands on the hidden x hidden products, forward kernel and reverse pass):
    gradients stay within bf16 rounding of the fp32 autograd reference (norm-wise; f32 trunk so that only the flow differs)"""
    from mhentropy_amd.train import TrainStep
    from oracle import train_ref, mano_ref
    B, N, h, steps = 4, 8, 128, 2
    model, sd = _model_and_state("resnet18", h, steps)
    model.q_z_giv_i.compute_dtype = torch.bfloat16
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0))
    xn, yn = synth.batch(11, B, image_size=96)
    z0 = torch.as_tensor(synth.noise(11, N * B))
    x, y = torch.as_tensor(xn), {k: torch.as_tensor(v) for k, v in yn.items()}
    out_ref, _, grads, _ = train_ref.loss_and_grads(sd, tb, x, y, z0, N, arch="resnet18")
    ts = TrainStep(model)
    assert ts.flow_bf16
    out = ts.forward_backward(x.cuda(), {k: v.cuda() for k, v in y.items()}, noise=z0.cuda(), N=N)
    assert_close(out["log_p"].cpu(), out_ref["log_p"].detach(), 2e-2, what="log_p (bf16 flow)")
    rows = _grad_report(ts, model, grads)
    flow = [r for r in rows if r[2].startswith("q_z_giv_i")]
    assert len(flow) == 2 * steps * 2 * 10
    assert max(r[1] for r in flow) < 0.15, sorted(flow, key=lambda r: -r[1])[:5]
    # (with only N*B = 32 rows the bf16 roundings do not average out: the median sits at ~3e-2 since round 2, when the 45-wide
    # products' operands went to bf16 as well - like the forward kernel's; every product accumulates in f32)
    assert sorted(r[1] for r in flow)[len(flow) // 2] < 4e-2, sorted(r[1] for r in flow)[len(flow) // 2]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_repeated_steps_minimise_the_loss(gpu_lib, dt):
    """40 train steps on one fixed batch: mean(-log_p) must fall well below its starting value in both the fp32 parity
    mode and the bf16 performance mode (Adam's first step moves every weight by lr, so the loss is allowed to rise
    first - the reference's optimizer does the same)."""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(0)
    model = harness.build_mhent(backbone="resnet18", h_dims=(128, 128), num_steps=2, tables=synth.mano_tables(0), compute_dtype=dt).cuda().train()
    xn, yn = synth.batch(3, 16, image_size=128)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    z0 = torch.as_tensor(synth.noise(3, 8 * 16)).cuda()
    ts = TrainStep(model)
    losses = [float(ts.step(x, y, noise=z0, N=8)["total"]) for _ in range(40)]
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < 0.35 * losses[0], (losses[0], losses[-1])
    # the flat buffers stay consistent with the module's parameters (views) and the packed caches were dropped
    p = model.det_head[0].weight
    assert p.data_ptr() == ts.P[ts.off[id(p)]:].data_ptr()
    # the reference's per-iteration metrics pass rides on the same forward (hand/CrossModalHand.py:357-361)
    o = ts.step(x, y, noise=z0, N=8, test_samples=5)
    assert o["xyz"].shape == (5, 16, 63) and o["verts"].shape == (5, 16, 2334) and o["uv"].shape == (5, 16, 42)
    # module forward paths read the trainer's device-resident packs: same loss from the module API as from the trainer
    again = model.get_loss(x, y, mods=["uv"], N=8, noise=z0)
    probe = ts.forward_backward(x, y, noise=z0, N=8)
    assert_close(again["log_p"].cpu(), probe["log_p"].cpu(), 5e-3 if dt == torch.float32 else 5e-2, what="module forward after training")
    model.eval()
    with torch.no_grad():
        s = model.sample(x, N=[4, 4], temp=0.8, y=y)
    assert torch.isfinite(s["uv"]).all()


@pytest.mark.parametrize("tag", ["small", "shipped"])
def test_reverse_pass_matches_the_references_own_gradients(gpu_lib, tag):
    """the gradients torch autograd produced on the REFERENCE's MHEnt (captured by oracle/gen_golden.py from
    /root/reference/hand/network.py with N=10, loss = mean(-log_p), criteria.py:55,173): det_head.2.weight, the first s-net's
    input layer, the last t-net's output layer and the conditioning feature - from the trunk feature on"""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    g = load_golden(f"mhent_{tag}")
    seed, h, steps, B, N = int(g["seed"]), int(g["h"]), int(g["steps"]), int(g["B"]), int(g["N_loss"])
    model = harness.build_mhent(backbone="resnet50", h_dims=(h, h), num_steps=steps, tables=synth.mano_tables(0))
    sd = {"q_z_giv_i." + k: torch.as_tensor(v) for k, v in synth.flow_state(seed, 45, 512, (h, h), steps).items()}
    sd.update({k: torch.as_tensor(v) for k, v in synth.head_state(seed, 2048, 512, 16).items()})
    assert not model.load_state_dict(sd, strict=False)[1]
    ts = TrainStep(model.cuda().train())
    y = {k[2:]: torch.as_tensor(v).cuda() for k, v in g.items() if k.startswith("y_")}
    out = ts.forward_backward(None, y, noise=torch.as_tensor(g["z0_loss"]).cuda(), N=N, trunk_out=torch.as_tensor(g["trunk"]).cuda())
    for k in ("log_p", "q_log_p_z_giv_y", "h_q_z_giv_i"):
        assert_close(out[k].cpu(), g["loss_" + k], RTOL, what=k)
    params = dict(model.named_parameters())
    for name in ("det_head.2.weight", "q_z_giv_i.s.0.l.0.weight", f"q_z_giv_i.t.{2 * steps - 1}.l.2.weight"):
        assert_close(ts.grad_of(params[name]).cpu(), g["grad_" + name], 2e-4, what="d loss / d " + name)
    assert_close(ts.tape["g_feat"].cpu(), g["grad_feat"], 2e-4, what="d loss / d feat")


def test_autograd_bridge_runs_the_references_loop_unchanged(gpu_lib):
    """hand/CrossModalHand.py:452-470 verbatim: get_loss -> criterion -> zero_grad -> total_loss.backward() ->
    clip_grad_norm_ -> torch.optim.Adam.step(), with a TrainStep attached: .grad equals the explicit reverse pass and the
    parameters move exactly like the fused step's."""
    from mhentropy_amd import harness
    from mhentropy_amd.criteria import MHEntLoss
    from mhentropy_amd.train import TrainStep
    xn, yn = synth.batch(3, 4, image_size=96)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    z0 = torch.as_tensor(synth.noise(3, 6 * 4)).cuda()
    models = []
    for _ in range(2):
        m, _sd = _model_and_state("resnet18", 64, 2)
        models.append(m)
    fused = TrainStep(models[0])
    bridge = TrainStep(models[1]).attach()
    opt = torch.optim.Adam(models[1].parameters(), lr=2e-4)
    crit = MHEntLoss()
    for it in range(3):
        ref = fused.step(x, y, noise=z0, N=6)
        out = models[1].get_loss(x, y, mods=["uv"], N=6, noise=z0)
        assert out["log_p"].requires_grad and not out["th_norm"].requires_grad
        total, losses, _ = crit(dict(out), y)
        opt.zero_grad()
        total.backward()
        if it == 0:
            for (n, p), (_, q) in zip(models[1].named_parameters(), models[0].named_parameters()):
                if p.grad is None:
                    continue
                # two separate runs of the same arithmetic (rounds 1-3: the f32 atomics' order differed), and a ReLU / max-pool decision that
                # flips under that round-off moves single elements by O(1 %) (tools/debug_bridge.py: 6e-7 when the launch
                # histories match, up to 2e-4 .. 1e-2 otherwise) - so a norm-wise bound
                a, b = p.grad.double().cpu(), fused.grad_of(q).double().cpu()
                assert ((a - b).norm() / (b.norm() + 1e-30)).item() < 2e-2, n
        torch.nn.utils.clip_grad_norm_(models[1].parameters(), 1.0)
        opt.step()
        assert_close(total.detach().cpu(), ref["total"].cpu(), 2e-2 if it else 1e-6, what=f"loss at step {it}")
        if it == 0:
            # after the first update the two replicas agree except where a ~0 gradient's sign decided Adam's +-lr step
            tot = off = 0
            for p, q in zip(models[1].parameters(), models[0].parameters()):
                d = (p.detach() - q.detach()).abs()
                tot += d.numel(); off += int((d > 2e-5).sum())
            assert off < 5e-3 * tot, (off, tot)


def test_module_paths_follow_parameters_written_outside_the_trainer(gpu_lib):
    """after torch's optimizer.step() on the attach() bridge (hand/CrossModalHand.py:470) and after load_state_dict, the
    modules' own paths (eval-mode sample, no-grad get_loss) must run on the NEW weights: compared with a fresh model built
    from the state_dict, which packs its operands from scratch"""
    from mhentropy_amd.criteria import MHEntLoss
    from mhentropy_amd.train import TrainStep
    xn, yn = synth.batch(5, 4, image_size=96)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    z0 = torch.as_tensor(synth.noise(5, 6 * 4)).cuda()
    model, _ = _model_and_state("resnet18", 64, 2)
    TrainStep(model).attach()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)       # a step large enough that stale packs would be visible
    total, _, _ = MHEntLoss()(dict(model.get_loss(x, y, mods=["uv"], N=6, noise=z0)), y)
    opt.zero_grad(); total.backward(); opt.step()

    def outputs(m):
        m.eval()
        with torch.no_grad():
            o = m.sample(x, N=[3, 3], temp=0.8, mods={"uv", "xyz"}, y=y, noise=z0[:12])
            l = m.get_loss(x, y, mods=["uv"], N=6, noise=z0)
        return o["uv"].float().cpu(), l["log_p"].float().cpu()

    fresh, _ = _model_and_state("resnet18", 64, 2)
    fresh.load_state_dict(model.state_dict())
    for got, want, what in zip(outputs(model), outputs(fresh), ("sample uv", "log_p")):
        assert_close(got, want, 1e-5, what=what + " right after optimizer.step()")
    # ... and a checkpoint load into the trainer-owned model
    other, _ = _model_and_state("resnet18", 64, 2)
    with torch.no_grad():
        for p_ in other.parameters():
            p_.mul_(1.05)
    model.load_state_dict(other.state_dict())
    fresh.load_state_dict(other.state_dict())
    for got, want, what in zip(outputs(model), outputs(fresh), ("sample uv", "log_p")):
        assert_close(got, want, 1e-5, what=what + " right after load_state_dict")


@pytest.mark.parametrize("backbone,dt,names,tol", [
    ("resnet18", torch.float32, ("bn1", "layer1.0.bn2", "layer3.0.downsample.1", "layer4.1.bn1"), 1e-5),
    # the bf16 ResNet-50 step: conv3 of layer1 / layer2 is never written (Gram statistics, csrc/conv_fold.hip) - those units have no
    # output tensor to count pixels on (round 5: second_bn_update raised there, found by bench.py's iteration_with_metrics leg)
    ("resnet50", torch.bfloat16, ("bn1", "layer1.0.bn3", "layer1.0.downsample.1", "layer2.1.bn3", "layer3.2.bn2", "layer4.1.bn1"), 1e-5)])
def test_metrics_pass_advances_batchnorm_buffers_twice(gpu_lib, backbone, dt, names, tol):
    """the reference runs the encoder twice per iteration in train mode (get_loss, then sample: hand/CrossModalHand.py:355-361),
    so running_mean / running_var take two momentum updates and num_batches_tracked += 2; step(test_samples=) reuses the
    feature and applies the second update to the buffers"""
    from mhentropy_amd.train import TrainStep
    xn, yn = synth.batch(6, 4, image_size=96 if backbone == "resnet18" else 128)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    z0 = torch.as_tensor(synth.noise(6, 4 * 4)).cuda()
    model, _ = _model_and_state(backbone, 64, 2, dtype=dt)
    r0 = {n: (m.running_mean.clone(), m.running_var.clone()) for n, m in model.feat_extractor.res.named_modules() if n in names}
    if dt == torch.float32:
        ref, _ = _model_and_state(backbone, 64, 2, dtype=dt)
        ref.train()
        with torch.no_grad():                        # two train-mode encoder passes over the same batch
            ref.feat_extractor.res(x); ref.feat_extractor.res(x)
        want = {n: (ref.feat_extractor.res.get_submodule(n).running_mean, ref.feat_extractor.res.get_submodule(n).running_var) for n in names}
    else:
        # bf16: the module's forward-only path and the train step's tape path round at different points (4 images: a 4x4 map in layer4,
        # 2e-2 apart there), so the yardstick is the train step itself, deterministic bit for bit: ONE update r1 = (1-m) r0 + m s from a
        # twin model, and two updates with the same statistic s are r2 = (1-m) r1 + m s = (2-m) r1 - (1-m) r0
        twin, _ = _model_and_state(backbone, 64, 2, dtype=dt)
        TrainStep(twin, lr=0.0).step(x, y, noise=z0, N=4)
        m_ = 0.1
        want = {n: tuple((2 - m_) * r1 - (1 - m_) * r0_ for r1, r0_ in zip((twin.feat_extractor.res.get_submodule(n).running_mean,
                                                                          twin.feat_extractor.res.get_submodule(n).running_var), r0[n])) for n in names}
        assert int(twin.feat_extractor.res.bn1.num_batches_tracked) == 1
    ts = TrainStep(model, lr=0.0)
    ts.step(x, y, noise=z0, N=4, test_samples=2)
    for name in names:
        a = model.feat_extractor.res.get_submodule(name)
        assert_close(a.running_mean.cpu(), want[name][0].cpu(), tol, 1e-7, what=name + ".running_mean")
        assert_close(a.running_var.cpu(), want[name][1].cpu(), tol, what=name + ".running_var")
        assert int(a.num_batches_tracked) == 2
    ts.step(x, y, noise=z0, N=4, test_samples=2, double_bn_update=False)
    assert int(model.feat_extractor.res.bn1.num_batches_tracked) == 3


def test_run_entry_point(gpu_lib, tmp_path, monkeypatch):
    """`python -m mhentropy_amd.run` (shape of the reference's run.py / CrossModalHand.train): two short epochs on synthetic
    batches with the per-iteration metrics pass, MultiStepLR and a checkpoint in the reference's container"""
    from mhentropy_amd import run, harness
    ck = tmp_path / "ck.pth"
    log = run.main(["--backbone", "resnet18", "--batch", "8", "--hyps", "6", "--test-samples", "5", "--hidden", "64", "--flow-steps", "2",
                    "--dtype", "f32", "--epochs", "2", "--iters", "4", "--image-size", "96", "--milestones", "1", "--save", str(ck)])
    assert len(log) == 2 and all(np.isfinite(r["loss"]) and r["epe3d"] > 0 and r["epe2d"] > 0 for r in log)
    assert log[0]["lr"] == 2e-4 and abs(log[1]["lr"] - 2e-5) < 1e-12
    sd = torch.load(ck)
    assert set(sd) == {"decoderPose", "encoderRGB", "mhe_rng_state"} and "q_z_giv_i.s.0.l.0.weight" in sd["encoderRGB"]
    # the device generator's words travel with the checkpoint: 8 iterations drew the loss noise + the metrics pass's noise each
    assert sd["mhe_rng_state"].dtype == torch.int64 and int(sd["mhe_rng_state"][0]) == 0 and int(sd["mhe_rng_state"][1]) > 0
    fresh = harness.build_mhent(backbone="resnet18", h_dims=(64, 64), num_steps=2, tables=synth.mano_tables(0))
    harness.load_model(ck, fresh)
    assert torch.equal(fresh.det_head[0].weight, sd["encoderRGB"]["det_head.0.weight"])
    # ... and driven by a YAML file in the reference's schema, resumed from that checkpoint, with the TensorBoard scalars' tags
    cfg = tmp_path / "tiny.yaml"
    cfg.write_text("dataset:\n  dataset_name: ho3d\nnetwork:\n  enc_type: MHEnt\n  input: image\n  num_latent: 512\n  backbone: resnet18\n"
                   "  h_dims: [64, 64]\n  num_steps: 2\n  regressor: realnvp\n  rot_prior: null\n  w_reg_th: 50\n  w_prior_2d: 0\n  w_reg_ds: 0\n"
                   "  b_2d: 0.03\n  entropy: true\n  mode: false\ntraining:\n  batch_size: 8\n  lr: 0.0002\n  milestones: [150, 250]\n  test_samples: 5\n")
    sc = tmp_path / "scalars.jsonl"
    seen, orig_load = {}, harness.load_model

    def spy(path, model, **kw):                    # resumed, not re-initialised: the model holds the checkpoint's weights before the first step
        r = orig_load(path, model, **kw)
        seen["w"] = model.det_head[0].weight.detach().cpu().clone()
        return r
    monkeypatch.setattr(harness, "load_model", spy)
    log2 = run.main(["--cfg", str(cfg), "--load", str(ck), "--hyps", "6", "--dtype", "f32", "--epochs", "1", "--iters", "2", "--image-size", "96",
                     "--scalars", str(sc)])
    assert len(log2) == 1 and np.isfinite(log2[0]["loss"])
    assert torch.equal(seen["w"], sd["encoderRGB"]["det_head.0.weight"].cpu())
    # resumed, not re-initialised - on the loss this time: the FIRST resumed iteration's total is the checkpointed model's loss on
    # that batch (batch 0, the run's own noise draw), i.e. the model the config path built + TrainStep's operand packs ARE the saved
    # model.  (Round 2 compared the resumed epoch's mean with the untrained model's: 6,175 vs 3,133 "failed" - tools/resume_diag.py
    # shows why that was the wrong expectation: after 8 steps on 8-image batches of random targets the checkpointed model scores 674 on
    # the batch it saw last and 3,700 / 9,005 on batches 0 / 1, which the resumed run replays; both construction paths and the packs
    # agree to 1e-6.  Adam's moments restart on resume as in the reference, hand/CrossModalHand.py:191-203,589-602.)
    from mhentropy_amd import ops
    # run.main restores the checkpoint's generator words (the resumed run CONTINUES the base-noise stream); its first draw is the loss noise
    ops.rng_set_state(torch.device("cuda", torch.cuda.current_device()), sd["mhe_rng_state"])
    noise0 = ops.randn(6 * 8, 45, torch.device("cuda", torch.cuda.current_device()))
    xn, yn = synth.batch(0, 8, image_size=96)
    fresh = fresh.cuda().train()
    with torch.no_grad():
        want = float(-fresh.get_loss(_dev(xn), {k: _dev(v) for k, v in yn.items()}, mods=["uv"], N=6, noise=noise0)["log_p"].mean())
    got = log2[0]["it_losses"][0]
    assert abs(got - want) <= 1e-3 * abs(want), (got, want)
    # ... and fed from decoded samples through the GPU input pipeline (row f4)
    log3 = run.main(["--backbone", "resnet18", "--batch", "4", "--hyps", "4", "--test-samples", "3", "--hidden", "64", "--flow-steps", "2",
                     "--dtype", "f32", "--epochs", "1", "--iters", "2", "--input-pipeline"])
    assert len(log3) == 1 and np.isfinite(log3[0]["loss"]) and log3[0]["epe2d"] > 0
    # ... and replayed from HIP graphs (re-captured when the learning rate steps)
    log4 = run.main(["--backbone", "resnet18", "--batch", "4", "--hyps", "4", "--hidden", "64", "--flow-steps", "2", "--dtype", "f32", "--epochs", "2",
                     "--iters", "3", "--image-size", "96", "--milestones", "1", "--graph", "1"])
    assert len(log4) == 2 and all(np.isfinite(r["loss"]) for r in log4) and abs(log4[1]["lr"] - 2e-5) < 1e-12
    # one optimizer step per iteration, capture iterations included (the warm-up pass of GraphedStep IS the iteration)
    assert int(run.main.last_trainer.step_t.item()) == 6
    assert int(run.main.last_trainer.model.feat_extractor.res.bn1.num_batches_tracked) == 6
    tags = {__import__("json").loads(l)["tag"] for l in open(sc)}
    assert {"loss_it/neg_log_p", "loss_avg/loss_total", "metric_train/eval_3d_rgb", "param/theta_norm", "param/beta_norm"} <= tags


def test_graphed_loop_equals_eager_loop(gpu_lib):
    """--graph 1 == --graph 0: a loop that takes GraphedStep's warm-up result for the capture iteration and replays the rest applies
    exactly one optimizer step per batch - same step count, BatchNorm buffers and PARAMETERS, bit for bit, as the eager loop on the same
    batches and noise (hand/CrossModalHand.py:455-470: one step per iteration).  Round 4: every cross-workgroup sum of the step is
    order-independent (fixed-point statistics, weight gradients through slabs + a fixed-order reducer, fixed-order column sums), so
    the comparison is exact; up to round 3 the f32 atomics only allowed a statistical bound."""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep, GraphedStep
    B, N, iters = 4, 4, 4
    batches = []
    for i in range(iters):
        xn, yn = synth.batch(40 + i, B, image_size=96)
        batches.append((_dev(xn), {k: _dev(yn[k]) for k in ("crop_uv", "vis")}, _dev(synth.noise(40 + i, N * B))))

    def fresh():
        torch.manual_seed(3)
        m = harness.build_mhent(backbone="resnet18", h_dims=(64, 64), num_steps=2, tables=synth.mano_tables(0)).cuda().train()
        return m, TrainStep(m, lr=2e-4)
    m0, ts0 = fresh()
    eager = [float(ts0.step(x, y, noise=z, N=N)["total"]) for x, y, z in batches]
    m1, ts1 = fresh()
    sx, sy, sz = batches[0][0].clone(), {k: v.clone() for k, v in batches[0][1].items()}, batches[0][2].clone()
    g = GraphedStep(ts1, sx, sy, noise=sz, N=N)
    graphed = [float(-g.warm_out["log_p"].mean())]
    for x, y, z in batches[1:]:
        sx.copy_(x); sz.copy_(z)
        for k in sy:
            sy[k].copy_(y[k])
        graphed.append(float(-g.replay()["log_p"].mean()))
    assert int(ts0.step_t.item()) == int(ts1.step_t.item()) == iters
    assert int(m0.feat_extractor.res.bn1.num_batches_tracked) == int(m1.feat_extractor.res.bn1.num_batches_tracked) == iters
    assert graphed == eager, (graphed, eager)          # same kernels, same inputs, order-independent sums: the same losses ...
    assert torch.equal(ts1.P, ts0.P), float((ts1.P - ts0.P).abs().max())          # ... and the same parameters after four Adam steps
    assert torch.equal(ts1.M, ts0.M) and torch.equal(ts1.V, ts0.V)          # Adam's moments too
    assert torch.equal(m1.feat_extractor.res.bn1.running_var, m0.feat_extractor.res.bn1.running_var)


def test_full_size_train_step_is_deterministic(gpu_lib):
    """BASELINE.json configs[2] shape (B=256, K=64, ResNet-50, h=512, bf16): two reverse passes from the same state give the SAME flat
    gradient, bit for bit, and two optimizer steps from the same state the same parameters (the reference's CPU step is deterministic,
    hand/CrossModalHand.py:455-470; the f32 atomics of rounds 1-3 were not)"""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(1)
    model = harness.build_mhent(backbone="resnet50", tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
    xn, yn = synth.batch(2, 256, image_size=256)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    z0 = torch.as_tensor(synth.noise(2, 64 * 256)).cuda()
    ts = TrainStep(model, lr=0.0)                      # lr 0: the parameters stay put; the BatchNorm buffers are restored by hand
    bufs = {n: b.clone() for n, b in model.named_buffers()}

    def run():
        for n, b in model.named_buffers():
            b.copy_(bufs[n])
        out = ts.forward_backward(x, y, noise=z0, N=64)
        return out["log_p"].clone(), ts.G.clone()
    lp1, g1 = run()
    lp2, g2 = run()
    assert torch.isfinite(g1).all() and g1.abs().max() > 0
    assert torch.equal(lp1, lp2), float((lp1 - lp2).abs().max())
    bad = (g1 != g2)
    assert not bad.any(), (int(bad.sum()), float((g1 - g2).abs().max()), [n for n, p in model.named_parameters() if (ts.grad_of(p) != g2[ts.off[id(p)]:ts.off[id(p)] + p.numel()].view(p.shape)).any()][:8])


def test_full_size_train_step_properties(gpu_lib):
    """BASELINE.json configs[2] shape (B=256, K=64, ResNet-50, h=512, bf16): properties that do not need the oracle at this size -
    finite loss and gradients, every parameter except the dead l2 head receives a gradient, BatchNorm bias gradients equal the
    channel sums of the raw-output gradients (sum over pixels of dL/dy = 0 for train-mode BN, so conv biases would be dead),
    the clip coefficient caps the update, the loss falls over a few steps"""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(1)
    model = harness.build_mhent(backbone="resnet50", tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
    xn, yn = synth.batch(2, 256, image_size=256)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    z0 = torch.as_tensor(synth.noise(2, 64 * 256)).cuda()
    ts = TrainStep(model)
    out = ts.forward_backward(x, y, noise=z0, N=64)
    assert torch.isfinite(out["log_p"]).all() and torch.isfinite(ts.G).all()
    dead = []
    for n, p in model.named_parameters():
        g = ts.grad_of(p)
        if n.startswith("feat_extractor.l2."):
            assert not g.any(), n
        elif not g.any():
            dead.append(n)
    assert not dead, dead
    p0 = ts.P.clone()
    losses = [float(out["total"])] + [float(ts.step(x, y, noise=z0, N=64)["total"]) for _ in range(6)]
    upd = (ts.P - p0).abs().max().item()
    assert 0 < upd <= 6 * 2e-4 * 1.5, upd                            # Adam moves a weight by about lr per step at most
    assert np.isfinite(losses).all() and min(losses[3:]) < losses[0], losses


def test_grouped_flow_weight_gradients_equal_the_per_net_launches(gpu_lib, monkeypatch):
    """RealNVP reverse pass at the shipped width (h = 512, bf16 mode, forward activations kept): the three weight-gradient products of all
    coupling nets as grouped launches after the chain (ops.conv_wgrad_batched) against one launch per net inside the chain - the same
    products over the same operands, so every flow gradient agrees to f32 summation order"""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(2)
    model = harness.build_mhent(backbone="resnet18", h_dims=(512, 512), num_steps=2, tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
    B, N = 8, 32
    xn, yn = synth.batch(5, B, image_size=96)
    x, y = _dev(xn), {k: _dev(v) for k, v in yn.items()}
    z0 = _dev(synth.noise(5, N * B))
    ts = TrainStep(model)
    assert ts.flow_bf16
    grads = {}
    monkeypatch.setenv("MHE_FLOW_REV_FUSED", "0")
    for mode in ("1", "0"):
        monkeypatch.setenv("MHE_FLOW_WGRAD_GROUPED", mode)
        ts.forward_backward(x, y, noise=z0, N=N)
        assert ts._flow_kept is not None
        grads[mode] = {n: ts.grad_of(p).clone() for n, p in model.named_parameters() if n.startswith("q_z_giv_i")}
    assert len(grads["1"]) == 4 * 2 * 10
    for n, g1 in grads["1"].items():
        g0 = grads["0"][n]
        assert g0.abs().max() > 0, n
        assert_close(g1.cpu(), g0.cpu(), 2e-5, what="grouped vs per-net " + n)


def test_fused_reverse_chain_of_the_flow_equals_the_coupling_by_coupling_pass(gpu_lib, monkeypatch):
    """csrc/flow_rev.hip (bf16 mode, h = 512, 64 hypotheses per image): the data-gradient chain of all couplings in one launch against
    the 13-launches-per-coupling pass - the same operands and products; the fused kernel applies the leaky-ReLU reverse to the f32
    accumulator where the launch-by-launch pass first rounds the product to bf16, so the two agree to bf16 rounding of the 512-wide
    gradients (norm-wise, like test_bf16_flow_reverse_close_to_fp32_autograd), the recovered base sample and everything f32 to 1e-5"""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(4)
    model = harness.build_mhent(backbone="resnet18", h_dims=(512, 512), num_steps=2, tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
    B, N = 6, 64
    xn, yn = synth.batch(6, B, image_size=96)
    x, y = _dev(xn), {k: _dev(v) for k, v in yn.items()}
    z0 = _dev(synth.noise(6, N * B))
    ts = TrainStep(model)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MHE_FLOW_REV_FUSED", mode)
        out = ts.forward_backward(x, y, noise=z0, N=N)
        res[mode] = ({n: ts.grad_of(p).clone() for n, p in model.named_parameters()}, ts.z0_recovered.clone(), ts.tape["g_feat"].clone(), float(out["total"]))
    (g0, z_0, gf0, l0), (g1, z_1, gf1, l1) = res["0"], res["1"]
    assert l0 == l1
    assert_close(z_1.cpu(), z_0.cpu(), 1e-5, what="recovered base sample")
    assert_close(z_1.cpu(), z0.cpu(), 2e-2, what="recovered base sample vs the noise that went in (bf16 nets)")
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-30))
    assert rel(gf1, gf0) < 1e-2, rel(gf1, gf0)
    worst = max((rel(g1[n], g0[n]), n) for n in g0 if g0[n].abs().max() > 0)
    assert worst[0] < 5e-2, worst
    flow = [rel(g1[n], g0[n]) for n in g0 if n.startswith("q_z_giv_i") and g0[n].abs().max() > 0]
    assert len(flow) == 4 * 2 * 10 and sorted(flow)[len(flow) // 2] < 5e-3, sorted(flow)[len(flow) // 2]


def test_conv3_reverse_on_gram_statistics_equals_the_pass_that_reads_y3(gpu_lib):
    """layer1 / layer2 bottlenecks of ResNet-50 in the bf16 train step: conv3's raw output y3 is never written by the forward pass (bn3's
    statistics from the Gram matrix of its input, the next block's tail kernel evaluates it on the fly).  Two reverse passes over ONE forward
    pass's tape (a second forward would differ in the last bit of the Gram sums' atomics, and 53 train-mode BatchNorm layers on a small
    batch amplify that to tens of per cent in the first layers' gradients):
      B  y3 evaluated once more, its BatchNorm reverse on the operand load of its data gradient, gy3 written for the weight gradient,
      C  conv3 + bn3 reversed on the Gram statistics (csrc/conv_fold.hip): y3 / gy3 exist nowhere.
    C replaces B's bf16-rounded gy3 by f32 / f64 algebra: every trunk gradient agrees norm-wise to 1e-2 (bf16 rounding of one operand of
    each product downstream), the tensors the fold itself writes (conv3 weights, bn3 weight / bias of the folded blocks) to 5e-3."""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(3)
    model = harness.build_mhent(backbone="resnet50", h_dims=(64, 64), num_steps=1, tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
    B, N = 8, 4
    xn, yn = synth.batch(9, B, image_size=128)
    x, y = _dev(xn), {k: _dev(v) for k, v in yn.items()}
    z0 = _dev(synth.noise(9, N * B))
    ts = TrainStep(model)
    ts.train_recompute, ts.conv3_fold = True, True
    ts.shortcut_fold = False        # (layer1's shortcut on Gram statistics has a test of its own below; its run-to-run spread reaches the stem undamped)
    ts.forward(x, y, noise=z0, N=N)
    res = {}
    for mode, fold in (("B", False), ("C", True), ("C2", True)):
        ts.conv3_fold = fold
        ts.backward()
        res[mode] = ({n: ts.grad_of(p).clone() for n, p in model.named_parameters()}, ts.n_fold)
    assert res["B"][1] == 0 and res["C"][1] == 7, [r[1] for r in res.values()]      # 3 + 4 blocks (layer2's last keeps its y3 for the forward's tail only)
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-30))
    gB, gC, gC2 = res["B"][0], res["C"][0], res["C2"][0]
    trunk = [n for n in gB if n.startswith("feat_extractor.res.") and gB[n].abs().max() > 0]
    assert all(torch.isfinite(gC[n]).all() for n in trunk)
    pre = "feat_extractor.res."
    # nothing upstream of the first folded block (layer2.3) changes at all
    for n in ("layer4.0.conv1.weight", "layer3.1.conv2.weight", "layer3.0.conv2.weight", "layer3.0.bn1.weight"):
        assert torch.equal(gC[pre + n], gB[pre + n]), n
    # the first folded block: what the fold writes, and what its data gradient feeds - bf16 rounding of gy3 (B) against exact algebra (C)
    for n, tol in (("layer2.3.bn3.bias", 1e-6), ("layer2.3.conv3.weight", 5e-3), ("layer2.3.bn3.weight", 8e-3), ("layer2.3.conv2.weight", 1.5e-2),
                   ("layer2.3.conv1.weight", 2e-2)):
        assert rel(gC[pre + n], gB[pre + n]) <= tol, (n, rel(gC[pre + n], gB[pre + n]))
    # through the six further folds the difference stays at the bf16 level in the residual layers (it grows by ~1.5e-3 per block here), and
    # so did the run-to-run spread of C itself up to round 3 (f32 atomics of D's split-K; C2 == C exactly since round 4); the stem's
    # own few parameters sit behind the max pool's reverse and see up to 1e-1 (the band of the other whole-trunk comparisons: 2e-1)
    layers = [n for n in trunk if ".layer" in n]
    worst = max((rel(gC[n], gB[n]), n) for n in layers)
    assert worst[0] < 8e-2, worst           # (seven folds: 4.4e-2 seen at layer1.1's first BatchNorm, run to run)
    again = max((rel(gC2[n], gC[n]), n) for n in layers)
    assert again[0] < 8e-2, again
    assert max(rel(gC[n], gB[n]) for n in trunk) < 2e-1
    assert rel(gC2[pre + "layer2.3.conv3.weight"], gC[pre + "layer2.3.conv3.weight"]) < 1e-5          # the fold's accumulator cleans itself


def test_shortcut_reverse_on_gram_statistics_equals_the_pass_over_its_output(gpu_lib):
    """layer1's shortcut (1x1, 64 -> 256, stride 1) in the bf16 train step: its BatchNorm's batch statistics come from the Gram matrix of the
    block's input, and the reverse pass runs conv + BatchNorm on those statistics (csrc/conv_fold.hip) - no apply pass over the gradient,
    the shortcut's raw output and the result, one ungated data-gradient launch on [g | a].  Two reverse passes over ONE forward tape, the
    second with the fold switched off for that unit (its raw output exists: the forward's tail reads it)."""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(5)
    model = harness.build_mhent(backbone="resnet50", h_dims=(64, 64), num_steps=1, tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
    B, N = 8, 4
    xn, yn = synth.batch(11, B, image_size=128)
    x, y = _dev(xn), {k: _dev(v) for k, v in yn.items()}
    z0 = _dev(synth.noise(11, N * B))
    ts = TrainStep(model)
    assert ts.shortcut_fold
    ts.forward(x, y, noise=z0, N=N)
    ud = ts.blocks[0].ud
    assert ud.fold_rev and ud.y is not None
    res = {}
    for mode, fold in (("pass", False), ("fold", True), ("fold again", True)):
        ud.fold_rev = fold
        ts.backward()
        res[mode] = ({n: ts.grad_of(p).clone() for n, p in model.named_parameters()}, ts.n_fold_ds)
    assert [res[m][1] for m in ("pass", "fold", "fold again")] == [0, 1, 1]
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-30))
    gP, gF, gF2 = res["pass"][0], res["fold"][0], res["fold again"][0]
    pre = "feat_extractor.res."
    # upstream of the shortcut nothing changes (up to round 3: nothing but the run-to-run spread of the reverse pass itself - f32 atomics of the
    # small weight gradients, amplified by the train-mode BatchNorm layers in between; measured below as fold against fold: 0 now)
    for n in ("layer2.0.downsample.0.weight", "layer1.1.conv1.weight", "layer1.0.conv3.weight"):
        spread = rel(gF2[pre + n], gF[pre + n])
        print(f"upstream {n}: fold vs pass {rel(gF[pre + n], gP[pre + n]):.2e}, fold vs fold {spread:.2e}")
        assert spread == 0.0 and rel(gF[pre + n], gP[pre + n]) == 0.0, (n, rel(gF[pre + n], gP[pre + n]), spread)      # round 4: bit for bit
    for n, tol in (("layer1.0.downsample.1.bias", 1e-3), ("layer1.0.downsample.0.weight", 5e-3), ("layer1.0.downsample.1.weight", 8e-3)):
        spread = rel(gF2[pre + n], gF[pre + n])
        print(f"shortcut {n}: fold vs pass {rel(gF[pre + n], gP[pre + n]):.2e}, fold vs fold {spread:.2e}")
        assert rel(gF[pre + n], gP[pre + n]) <= tol + 3 * spread, (n, rel(gF[pre + n], gP[pre + n]), spread)
    # behind it: the stem (through the max pool's reverse).  The reverse pass is deterministic since round 4 (fold against fold: 0), so
    # what is left is the fold's own arithmetic: its weights [(k2 W)^T | S] and the per-channel constant c0 are rounded to bf16, i.e. the
    # shortcut's input gradient carries a ~1e-3 relative error that is COHERENT over a channel's pixels.  conv1's weight gradient does
    # not see a per-channel constant (bn1's reverse removes it): measured 3.4e-3; bn1's own sums over 32k pixels add the coherent part
    # up: dgamma 5.9e-2, and dbeta = sum_p g - pure cancellation, |sum g| << sum |g| - 0.5.  Bounds = about twice the measured figures.
    for n, tol in (("conv1.weight", 8e-3), ("bn1.weight", 1.2e-1), ("bn1.bias", 1.0)):
        spread = rel(gF2[pre + n], gF[pre + n])
        print(f"stem {n}: fold vs pass {rel(gF[pre + n], gP[pre + n]):.2e}, fold vs fold {spread:.2e}")
        assert spread == 0.0 and rel(gF[pre + n], gP[pre + n]) < tol, (n, rel(gF[pre + n], gP[pre + n]), spread)


def test_resident_tile_3x3_kernel_in_the_train_step_equals_the_im2col_kernels(gpu_lib):
    """layer2 / layer3's stride-1 3x3 units in the bf16 train step run on the resident-tile kernel (csrc/conv_halo.hip): forward with the
    producer's BatchNorm + ReLU on its load (the normalised tensor written on the way for the weight gradient), data gradient in the
    same kernel.  Against the im2col kernels + separate BatchNorm pass (conv_halo / conv_halo_dg = False) on the same inputs:
      forward  whole steps of two trainers: the launch counts prove which path ran; the loss agrees to 5e-3 (1.7e-3 seen: the two forms sum a
               tap's products in different orders and round y2 to bf16 from different f32 sums; B = 4 under 53 train-mode BatchNorms).  The
               GRADIENTS of two different forwards are not comparable at this batch size (ReLU gates flip: 0.7 norm-wise in layer1) - the
               forward kernel itself is compared layer by layer in test_gpu_modules.py;
      reverse  two reverse passes over ONE forward tape, data gradients on the resident-tile kernel / on the im2col kernels: nothing
               upstream of the first such unit changes at all, everything else at the bf16 level norm-wise."""
    from mhentropy_amd import harness, ops
    from mhentropy_amd.train import TrainStep
    B, N = 4, 4
    xn, yn = synth.batch(21, B, image_size=256)                     # layer2 at 32 x 32, layer3 at 16 x 16: the two widths the kernel takes
    x, y = _dev(xn), {k: _dev(v) for k, v in yn.items()}
    z0 = _dev(synth.noise(21, N * B))
    calls = {"fwd": 0, "dg": 0}
    f0 = ops.conv3x3_halo
    def spy(*a, **k):                                                # (the data gradient is the same entry with the ReLU gate's tensor as mask=)
        calls["dg" if k.get("mask") is not None else "fwd"] += 1
        return f0(*a, **k)
    ops.conv3x3_halo = spy
    try:
        res = {}
        for mode, on in (("halo", True), ("im2col", False), ("halo again", True)):
            torch.manual_seed(5)
            model = harness.build_mhent(backbone="resnet50", h_dims=(64, 64), num_steps=1, tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
            ts = TrainStep(model, lr=0.0)
            ts.conv_halo = ts.conv_halo_dg = on
            calls["fwd"] = calls["dg"] = 0
            out = ts.forward_backward(x, y, noise=z0, N=N)
            res[mode] = (float(out["total"]), {n: ts.grad_of(p).clone() for n, p in model.named_parameters()}, dict(calls))
        # 3 + 5 stride-1 units of layer2 / layer3 (the first block of a stage has the stride-2 unit)
        assert res["halo"][2] == {"fwd": 8, "dg": 8} and res["im2col"][2] == {"fwd": 0, "dg": 0}, (res["halo"][2], res["im2col"][2])
        assert res["halo again"][0] == res["halo"][0] and all(torch.equal(res["halo again"][1][n], g) for n, g in res["halo"][1].items())
        assert abs(res["halo"][0] - res["im2col"][0]) <= 5e-3 * abs(res["im2col"][0]), (res["halo"][0], res["im2col"][0])
        # ---- reverse: one tape (the last trainer's: resident-tile forward), two reverse passes
        ts.forward(x, y, noise=z0, N=N)
        rev = {}
        for mode, on in (("halo", True), ("im2col", False)):
            ts.conv_halo_dg = on
            calls["dg"] = 0
            ts.backward()
            rev[mode] = ({n: ts.grad_of(p).clone() for n, p in model.named_parameters()}, calls["dg"])
    finally:
        ops.conv3x3_halo = f0
    assert rev["halo"][1] == 8 and rev["im2col"][1] == 0, (rev["halo"][1], rev["im2col"][1])
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-30))
    gH, gI = rev["halo"][0], rev["im2col"][0]
    pre = "feat_extractor.res."
    for n in ("layer4.0.conv1.weight", "layer4.2.conv3.weight", "layer3.5.conv3.weight", "layer3.5.bn3.weight", "layer3.5.conv2.weight"):
        assert torch.equal(gH[pre + n], gI[pre + n]), n              # upstream of (and at: its weight gradient reads the same gy) the first such unit
    names = [n for n in gI if n.startswith(pre) and gI[n].abs().max() > 0]
    errs = sorted((rel(gH[n], gI[n]), n) for n in names)
    layers = [e for e in errs if ".layer" in e[1]]
    assert layers[-1][0] < 8e-2 and layers[len(layers) // 2][0] < 2e-2, (layers[-3:], layers[len(layers) // 2])
    # the stem's BatchNorm sits behind the max pool's reverse: its bias gradient is a nearly cancelling sum of 4 M gated elements (0.5 seen, the
    # same figure as in the shortcut test above), its weight gradient 6.5e-2
    stem = [e for e in errs if ".layer" not in e[1]]
    assert all(e[0] < (1.0 if e[1].endswith("res.bn1.bias") else 1.5e-1) for e in stem), stem


def test_fallback_operand_layouts_are_refreshed_when_a_fallback_path_runs(gpu_lib):
    """The flow's plain operand layouts (the second-generation coupling kernel's stream, the coupling-by-coupling reverse pass's matrices)
    are not re-gathered after every optimizer step while only the one-launch kernels run (hidden 512, 64 hypotheses per image): a path
    that reads them - here the modules' own `sample` with 3 hypotheses per image, and a train step with 16 hypotheses per image - must
    find them at the CURRENT parameters, after eager steps and after HIP-graph replays alike (compared with a fresh model built from
    the state_dict, which packs its operands from scratch)."""
    from mhentropy_amd.train import TrainStep, GraphedStep
    B = 2
    xn, yn = synth.batch(7, B, image_size=96)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    z64, z3 = torch.as_tensor(synth.noise(7, 64 * B)).cuda(), torch.as_tensor(synth.noise(8, 3 * B)).cuda()
    z16 = torch.as_tensor(synth.noise(9, 16 * B)).cuda()

    def sample_of(m):
        m.eval()
        with torch.no_grad():
            o = m.sample(x, N=[3, 3], temp=0.8, mods={"uv"}, y=y, noise=z3)
        m.train()
        assert torch.isfinite(o["uv"]).all()
        return o["uv"].float().cpu()

    def fresh_like(model):
        f, _ = _model_and_state("resnet18", 512, 2, dtype=torch.bfloat16)
        f.load_state_dict(model.state_dict())
        return f

    model, _ = _model_and_state("resnet18", 512, 2, dtype=torch.bfloat16)
    ts = TrainStep(model, lr=1e-3)                          # steps large enough that stale layouts would be visible (1e-2 diverges in two steps)
    ts.arena.poison_stale = True                                 # ... and a reader that skipped need_fallback() would meet NaN (MHE_POISON_STALE_TABLES)
    assert ts.flow_fused_tables and not ts.arena.fb_keep
    for _ in range(2):
        ts.step(x, y, noise=z64, N=64)                      # the one-launch kernels only: the fallback layouts are left behind
    assert ts.arena.fb_stale and not ts.arena.fb_keep
    assert_close(sample_of(model), sample_of(fresh_like(model)), 1e-5, what="sample after eager steps on the one-launch kernels")
    assert ts.arena.fb_keep and not ts.arena.fb_stale                 # ... refreshed on demand, and kept fresh from now on
    ts.step(x, y, noise=z64, N=64)
    assert not ts.arena.fb_stale
    assert_close(sample_of(model), sample_of(fresh_like(model)), 1e-5, what="sample after a further step")
    # graph replays: the captured repack of a trainer that never needed the layouts does not refresh them
    model2, _ = _model_and_state("resnet18", 512, 2, dtype=torch.bfloat16)
    ts2 = TrainStep(model2, lr=1e-3)
    ts2.arena.poison_stale = True
    gs = GraphedStep(ts2, x, y, noise=z64, N=64)
    assert not gs._fb_in_graph
    gs.replay(); gs.replay()
    torch.cuda.synchronize()
    assert ts2.arena.fb_stale
    assert_close(sample_of(model2), sample_of(fresh_like(model2)), 1e-5, what="sample after graph replays")
    gs.replay()
    torch.cuda.synchronize()
    assert ts2.arena.fb_stale                                    # (the replay cannot refresh them: stale again, refreshed again on demand)
    assert_close(sample_of(model2), sample_of(fresh_like(model2)), 1e-5, what="sample after a further replay")
    # a train step that takes the coupling-by-coupling passes itself (16 hypotheses per image) equals the same step of a fresh trainer
    out = ts2.forward_backward(x, y, noise=z16, N=16)
    ts3 = TrainStep(fresh_like(model2), lr=1e-3)
    ref = ts3.forward_backward(x, y, noise=z16, N=16)
    assert torch.equal(out["log_p"], ref["log_p"]) and torch.equal(ts2.G, ts3.G)


def test_multi_problem_weight_gradient_launch(gpu_lib):
    """mhe_conv_wgrad_multi_nhwc (round 5): the weight gradients of several layers in one call - problems of one tile shape share a launch, the
    pixel range of each is cut only as far as a common slice length asks (fewer partial slabs), unsplit problems add their tiles with plain
    stores.  Against one launch per layer (same bf16 products, f32 sums in another order) and against torch autograd; `dW +=` semantics;
    two calls give the same bits (fixed summation order).  Shapes: layer3's three convolutions (256 x 256 and 128 x 128 tile classes, split),
    layer1's 64-channel shapes (64 x 128 / 128 x 64 classes), a stride-2 3x3, an f32 problem (its own launch), and a batch with more tiles
    than the chip takes (unsplit: the plain-store form)."""
    from mhentropy_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(11)
    bf = torch.bfloat16
    # (Cin, Cout, k, stride, pad, H, B, dtype)
    cases = [(256, 256, 3, 1, 1, 16, 24, bf), (256, 1024, 1, 1, 0, 16, 24, bf), (1024, 256, 1, 1, 0, 16, 24, bf), (512, 256, 1, 1, 0, 16, 24, bf),
             (64, 64, 3, 1, 1, 32, 6, bf), (64, 256, 1, 1, 0, 32, 6, bf), (256, 64, 1, 1, 0, 32, 6, bf), (128, 128, 3, 2, 1, 32, 6, bf),
             (64, 128, 1, 1, 0, 16, 4, torch.float32),
             (1152, 1024, 1, 1, 0, 8, 8, bf), (1024, 1152, 1, 1, 0, 8, 8, bf), (1152, 1152, 1, 1, 0, 8, 8, bf), (1024, 1024, 3, 1, 1, 8, 8, bf)]
    items, refs, singles = [], [], []
    for (Cin, Cout, k, stride, pad, H, B, dt) in cases:
        x = torch.randn(B, Cin, H, H, generator=g).to(dt).float().requires_grad_(False)
        w = torch.zeros(Cout, Cin, k, k, requires_grad=True)
        y = F.conv2d(x, w, stride=stride, padding=pad)
        gy = torch.randn(y.shape, generator=g).to(dt).float()
        y.backward(gy)
        refs.append(w.grad.permute(0, 2, 3, 1).reshape(Cout, -1))
        xd, gyd = _nhwc(x, dt), _nhwc(gy, dt)
        dw = torch.ones(Cout, k * k * Cin, device="cuda")
        items.append((xd, gyd, k, k, stride, pad, dw))
        singles.append(ops.conv_wgrad(xd, gyd, k, k, stride, pad, torch.ones(Cout, k * k * Cin, device="cuda")))
    ops.conv_wgrad_multi(items)
    torch.cuda.synchronize()
    first = [it[6].clone() for it in items]
    for it, ref, one, c in zip(items, refs, singles, cases):
        assert_close(it[6].cpu() - 1.0, ref, 2e-5, what=f"multi-problem dW vs autograd {c}")            # dW += : the ones survive
        assert_close(it[6].cpu(), one.cpu(), 2e-5, what=f"multi-problem dW vs its own launch {c}")
    for it in items:
        it[6].fill_(1.0)
    ops.conv_wgrad_multi(items)
    torch.cuda.synchronize()
    assert all(torch.equal(it[6], f) for it, f in zip(items, first)), "two multi-problem calls differ: the summation order is not fixed"


def test_operand_repack_from_affine_groups_equals_the_indexed_repack(gpu_lib):
    """TrainStep.repack (round 5): the bf16 operand layouts (convolution weights in every tile order, the flow's fragment-major and fallback
    layouts) come from (base, stride, validity) per eight elements.  Every group of the ResNet-50 + RealNVP arena is affine, and the
    operands are the bits the one-index-per-element gather produces."""
    from mhentropy_amd import harness, ops
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(2)
    model = harness.build_mhent(backbone="resnet50", tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
    ts = TrainStep(model)
    a = ts.arena.main[torch.bfloat16]
    assert a.aff is not None and a.idx.numel() > 5e7, "the bf16 arena is expected to be affine in groups of eight"
    segs = a.aff[2]
    assert sum(hi - lo for kind, lo, hi in segs if kind == "idx") < 1e-3 * a.idx.numel() / 8, segs      # (the stem's taps stay on indices)
    with torch.no_grad():
        ts.P.add_(torch.randn_like(ts.P) * 1e-3)          # operands of other parameters than the ones packed at construction
    ts.repack()
    got = a.view.clone()
    ops.gather(ts.P, a.idx, a.view, a.idx2)
    assert torch.equal(got, a.view)
    # (the fallback layouts - gathered only when a fallback path runs - go through the same choice: affine where every range qualifies)
    ts.arena.repack_fallback()
    fb = ts.arena.fallback[torch.bfloat16]
    if fb.idx.numel():
        got = fb.view.clone()
        ops.gather(ts.P, fb.idx, fb.view, fb.idx2)
        assert torch.equal(got, fb.view)


def test_queued_multi_problem_weight_gradients_equal_one_launch_per_layer(gpu_lib):
    """TrainStep queues the trunk's weight gradients per gradient bucket and launches them together (MHE_WGRAD_MULTI, ops.conv_wgrad_multi).
    Two reverse passes over ONE forward pass's tape - queued vs one launch per layer: the same bf16 operands and products, f32 sums in another
    order, so every parameter gradient agrees to 2e-5 of its scale; the queued form twice: equal bit for bit (fixed summation order).
    ResNet-50 in the bf16 mode at 128 x 128 (all four tile classes, split and unsplit problems)."""
    from mhentropy_amd import harness
    from mhentropy_amd.train import TrainStep
    torch.manual_seed(6)
    model = harness.build_mhent(backbone="resnet50", h_dims=(64, 64), num_steps=1, tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
    B, N = 16, 4
    xn, yn = synth.batch(10, B, image_size=128)
    x, y = _dev(xn), {k: _dev(v) for k, v in yn.items()}
    z0 = _dev(synth.noise(10, N * B))
    ts = TrainStep(model)
    assert ts.wgrad_multi
    ts.forward(x, y, noise=z0, N=N)
    grads = {}
    for mode in (True, False, True):
        ts.wgrad_multi = mode
        ts.backward()
        g = {n: ts.grad_of(p).clone() for n, p in model.named_parameters()}
        if mode and True in grads:
            bad = [n for n in g if not torch.equal(g[n], grads[True][n])]
            assert not bad, bad[:6]
        grads[mode] = g
    worst = (0.0, "")
    for n, a in grads[True].items():
        b_ = grads[False][n]
        if b_.abs().max() == 0:
            assert a.abs().max() == 0, n
            continue
        e = float((a - b_).abs().max() / b_.abs().max())
        worst = max(worst, (e, n))
    print("queued vs per-layer weight gradients, worst max-abs relative difference:", worst)
    assert worst[0] < 2e-5, worst
