"""The float64 references of tests/reverse_ref.py against float64 torch autograd of the operations they claim to differentiate (no GPU, no
library): agreement to float64 rounding, 1e-12 of the tensor's scale; the winner reference equal to torch's return_indices."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import reverse_ref as rr
from conftest import assert_close

F64, BF = torch.float64, torch.bfloat16
TOL = 1e-12


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("form", ["plain", "relu", "relu-residual"])
def test_bn_backward_reference_is_autograd_of_batch_norm(form):
    g = _gen(1)
    P, C, eps = 37, 12, 1e-5
    y = (torch.randn(P, C, generator=g, dtype=F64) * 2 + 0.5).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    gamma.requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    res = torch.randn(P, C, generator=g, dtype=F64)
    z = F.batch_norm(y, None, None, gamma, beta, training=True, eps=eps)
    a = {"plain": z, "relu": F.relu(z), "relu-residual": F.relu(z + res)}[form]
    go = torch.randn(P, C, generator=g, dtype=F64)
    a.backward(go)
    gy, dgamma, dbeta = rr.bn_backward(go, None if form == "plain" else a.detach(), y.detach(), gamma.detach(), eps)
    assert_close(gy.numpy(), y.grad.numpy(), TOL, what="dy")
    assert_close(dgamma.numpy(), gamma.grad.numpy(), TOL, what="dgamma")
    assert_close(dbeta.numpy(), beta.grad.numpy(), TOL, what="dbeta")


def test_gate_is_a_greater_than_zero():
    """+0, -0, a negative value and the smallest positive subnormals are gated as float64 `a > 0` says, which is torch's ReLU backward"""
    for dt, tiny in ((torch.float32, 2.0 ** -149), (BF, 2.0 ** -133)):
        a = torch.tensor([0.0, -0.0, -1.0, tiny, 1.0], dtype=dt)
        assert float(a[3]) == tiny
        x = a.double().requires_grad_(True)
        F.relu(x).backward(torch.ones(5, dtype=F64))
        assert torch.equal(rr.gated(torch.ones(5), a), x.grad) and x.grad.tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]


def test_mean_invstd_reference_is_batch_norm_statistics():
    g = _gen(2)
    y = torch.randn(50, 7, generator=g, dtype=F64) * 3 + 1
    mean, istd = rr.mean_invstd(y.sum(0), (y * y).sum(0), 50, 1e-5)
    assert_close(mean.numpy(), y.mean(0).numpy(), TOL)
    assert_close(istd.numpy(), (1 / torch.sqrt(y.var(0, unbiased=False) + 1e-5)).numpy(), 1e-11)


def _tied_image(B, H, W, C, dt, seed):
    """few levels (ties everywhere), post-ReLU zeros, and for bf16 values that differ only below its precision before rounding"""
    g = _gen(seed)
    x = torch.randint(-3, 4, (B, H, W, C), generator=g).float() / 2 + torch.randint(0, 3, (B, H, W, C), generator=g).float() * 2.0 ** -10
    return torch.relu(x).to(dt)


@pytest.mark.parametrize("dt", [torch.float32, BF, F64], ids=["f32", "bf16", "f64"])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (8, 8), (9, 7)])
def test_winner_reference_is_torch_return_indices(H, W, dt):
    x = _tied_image(2, H, W, 4, dt, H * 10 + W)
    pooled, tap = rr.maxpool_winners(x)
    xt = x.float() if dt == BF else x
    want, flat = F.max_pool2d(xt.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    Ho, Wo = rr.pooled_size(H, W)
    hi, wi = flat // W, flat % W                                  # [B, C, Ho, Wo] input pixel of the winner
    dh = hi - (2 * torch.arange(Ho)[:, None] - 1)
    dw = wi - (2 * torch.arange(Wo)[None, :] - 1)
    assert torch.equal(pooled.permute(0, 3, 1, 2).to(xt.dtype), want)
    assert torch.equal(tap.permute(0, 3, 1, 2).long(), dh * 3 + dw)
    assert (tap.float().var() > 0) or H * W == 1


def test_winner_reference_on_windows_of_minus_infinity_and_nan():
    x = torch.full((1, 3, 3, 1), -float("inf"))
    pooled, tap = rr.maxpool_winners(x)
    want, flat = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    assert torch.equal(pooled.permute(0, 3, 1, 2), want)
    assert tap.flatten().tolist() == [4, 3, 1, 0] and flat.flatten().tolist() == [0, 1, 3, 4]
    x[0, 2, 2, 0] = float("nan")
    pooled, tap = rr.maxpool_winners(x)
    assert torch.isnan(pooled[0, 1, 1, 0]) and int(tap[0, 1, 1, 0]) == 4 and not torch.isnan(pooled.flatten()[:3]).any()


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (9, 7), (16, 8)])
def test_pool_reverse_reference_is_autograd_of_max_pool(H, W):
    x = _tied_image(2, H, W, 4, F64, H + W).requires_grad_(True)
    y = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1)
    gy = torch.randn(y.shape, generator=_gen(3), dtype=F64)
    y.backward(gy)
    _, tap = rr.maxpool_winners(x.detach())
    gx = rr.maxpool_bwd(gy.permute(0, 2, 3, 1), tap, H, W)
    assert_close(gx.numpy(), x.grad.numpy(), TOL, what="max pool reverse")
    assert torch.equal(rr.gather_winners(x.detach(), tap), y.detach().permute(0, 2, 3, 1))


def test_fused_pool_reference_is_autograd_through_relu_of_the_affine():
    """relu(y scale + shift) -> max pool, negative scales included: the gated scatter is d / d(relu's input), the winners' raw inputs
    reproduce the pooled values"""
    g = _gen(5)
    B, H, W, C = 2, 9, 7, 8
    y = (torch.randint(-8, 9, (B, H, W, C), generator=g).double() / 4).requires_grad_(True)
    scale = torch.tensor([1.0, -1.0, 0.5, -2.0] * 2, dtype=F64)
    shift = torch.randint(-4, 5, (C,), generator=g).double() / 4
    pre = y * scale + shift
    pre.retain_grad()
    pooled = F.max_pool2d(F.relu(pre).permute(0, 3, 1, 2), 3, 2, 1)
    gy = torch.randn(pooled.shape, generator=g, dtype=F64)
    pooled.backward(gy)
    act = rr.affine_relu(y.detach(), scale, shift, F64)
    m, tap = rr.maxpool_winners(act)
    assert torch.equal(m, pooled.detach().permute(0, 2, 3, 1))
    gx = torch.where(act > 0, rr.maxpool_bwd(gy.permute(0, 2, 3, 1), tap, H, W), torch.zeros((), dtype=F64))
    assert_close(gx.numpy(), pre.grad.numpy(), TOL, what="gated scatter")
    xwin = rr.gather_winners(y.detach(), tap)
    assert torch.equal((xwin * scale + shift).clamp_min(0.0), m)


@pytest.mark.parametrize("masked", [False, True])
def test_avgpool_and_stride2_references_are_autograd(masked):
    g = _gen(7)
    B, HW, C = 3, 49, 12
    x = torch.randn(B, HW, C, generator=g, dtype=F64).requires_grad_(True)
    a = F.relu(x) if masked else x
    gf = torch.randn(B, C, generator=g, dtype=F64)
    a.mean(1).backward(gf)
    assert_close(rr.avgpool_bwd(gf, HW, a.detach() if masked else None).numpy(), x.grad.numpy(), TOL, what="average pool reverse")
    for H, W in ((1, 1), (2, 2), (3, 3), (5, 4), (8, 8)):
        x = torch.randn(2, H, W, 4, generator=g, dtype=F64).requires_grad_(True)
        base = torch.randn(2, H, W, 4, generator=g, dtype=F64)
        gs = torch.randn(2, (H + 1) // 2, (W + 1) // 2, 4, generator=g, dtype=F64)
        ((x[:, ::2, ::2] * gs).sum() + (x * base).sum()).backward()
        out, mag = rr.upsample2(gs, H, W, base)
        assert_close(out.numpy(), x.grad.numpy(), TOL, what="stride-2 slice reverse")
        assert (mag >= out.abs() - 1e-15).all()
        assert torch.equal(rr.upsample2(gs, H, W)[0] + base, out)


@pytest.mark.parametrize("max_norm,scale", [(1.0, 3.0), (1.0, 1e-4), (0.0, 3.0)], ids=["clip-active", "clip-inactive", "no-clip"])
def test_clip_adam_reference_is_clip_grad_norm_and_torch_adam(max_norm, scale):
    g = _gen(11)
    n, lr = 257, 2e-4
    p0 = torch.randn(n, generator=g, dtype=F64)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=lr)
    p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for t in range(1, 6):
        gr = torch.randn(n, generator=g, dtype=F64) * scale
        ref.grad = gr.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        out = rr.clip_adam(p, gr, m, v, t, rr.sqnorm(gr) if max_norm > 0 else None, lr, 0.9, 0.999, 1e-8, max_norm, 1.0)
        p, m, v = out["p"], out["m"], out["v"]
        assert (out["bp"] >= 0).all() and (out["bm"] >= 0).all() and (out["bv"] >= 0).all()
    assert_close(p.numpy(), ref.detach().numpy(), TOL, what="parameters after 5 steps")
    assert_close(m.numpy(), opt.state[ref]["exp_avg"].numpy(), TOL, what="m")
    assert_close(v.numpy(), opt.state[ref]["exp_avg_sq"].numpy(), TOL, what="v")
    # grad_scale: the gradient buffer holds grad / grad_scale
    half = rr.clip_adam(p0, gr * 2.0, m, v, 6, rr.sqnorm(gr * 2.0) if max_norm > 0 else None, lr, 0.9, 0.999, 1e-8, max_norm, 0.5)
    full = rr.clip_adam(p0, gr, m, v, 6, rr.sqnorm(gr) if max_norm > 0 else None, lr, 0.9, 0.999, 1e-8, max_norm, 1.0)
    assert_close(half["p"].numpy(), full["p"].numpy(), TOL, what="grad_scale = 0.5")


@pytest.mark.parametrize("with_logp", [False, True])
@pytest.mark.parametrize("R,B,dim", [(6, 3, 45), (4, 2, 64), (5, 5, 1)])
def test_coupling_reference_is_autograd_of_the_forward_formula(R, B, dim, with_logp):
    """x_out = m x + (1 - m)(x e^s + t), s = tanh(Os)(1 - m), log q -= sum s; loss = <g_out, x_out> + sum_r a_q[r] log q[r]"""
    g = _gen(R * dim)
    mask = (torch.arange(dim) % 2).double() if dim > 1 else torch.zeros(1, dtype=F64)
    x = torch.randn(R, dim, generator=g, dtype=F64).requires_grad_(True)
    Os = (torch.rand(R, dim, generator=g, dtype=F64) * 8 - 4).requires_grad_(True)
    Ot = torch.randn(R, dim, generator=g, dtype=F64).requires_grad_(True)
    g_out = torch.randn(R, dim, generator=g, dtype=F64)
    g_logp = torch.randn(B, generator=g, dtype=F64) if with_logp else None
    qw = -0.7
    x_out, dlogq = rr.coupling_forward(x, Os, Ot, mask)
    loss = (g_out * x_out).sum()
    if with_logp:
        loss = loss + (g_logp[torch.arange(R) % B] * qw * dlogq).sum()
    loss.backward()
    pad = lambda t: torch.cat([t.detach(), torch.randn(R, 64 - dim, generator=g, dtype=F64)], 1)          # the padding columns are not read
    out = rr.couple_bwd(x_out.detach(), pad(Os), pad(Ot), mask, g_out, g_logp, qw, B)
    assert_close(out["x_in"].numpy(), x.detach().numpy(), TOL, what="x_in")
    assert_close(out["GOs"][:, :dim].numpy(), Os.grad.numpy(), TOL, what="GOs")
    assert_close(out["GOt"][:, :dim].numpy(), Ot.grad.numpy(), TOL, what="GOt")
    assert_close(out["g_part"].numpy(), x.grad.numpy(), TOL, what="g_part")
    assert not out["GOs"][:, dim:].any() and not out["GOt"][:, dim:].any()
    for k in ("b_x_in", "b_GOs", "b_g_part"):
        assert (out[k] >= 0).all() and torch.isfinite(out[k]).all()


def test_flow_stage_references_are_autograd():
    g = _gen(13)
    N, B, H = 4, 3, 8
    pre = torch.randn(N * B, H, generator=g, dtype=F64).requires_grad_(True)
    cond = torch.randn(B, H, generator=g, dtype=F64)
    out, mag = rr.cond_lrelu(pre.detach(), cond, B, 0.01)
    want = F.leaky_relu(pre.view(N, B, H) + cond, 0.01).view(N * B, H)
    assert_close(out.numpy(), want.detach().numpy(), TOL)
    gr = torch.randn(N * B, H, generator=g, dtype=F64)
    want.backward(gr)
    assert_close(rr.lrelu_bwd(gr, out, 0.01).numpy(), pre.grad.numpy(), TOL, what="leaky relu reverse")
    assert torch.equal(rr.lrelu_bwd(gr, out, 0.0), gr * (out > 0))
    # the nets see m x: mask_pad is that product, couple_accum adds its adjoint m (GXs + GXt) to the direct part
    x = torch.randn(5, 45, generator=g, dtype=F64).requires_grad_(True)
    mask = (torch.arange(45) % 2).double()
    GXs, GXt, gp = torch.randn(5, 64, generator=g, dtype=F64), torch.randn(5, 64, generator=g, dtype=F64), torch.randn(5, 45, generator=g, dtype=F64)
    xp = F.pad(x * mask, (0, 19))
    assert torch.equal(rr.mask_pad(x.detach(), mask), xp.detach())
    ((xp * (GXs + GXt)).sum() + (x * gp).sum()).backward()
    assert_close(rr.couple_accum(gp, GXs, GXt, mask)[0].numpy(), x.grad.numpy(), TOL, what="couple_accum")
