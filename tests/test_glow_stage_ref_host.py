"""The float64 references of tests/glow_stage_ref.py, checked on the CPU: every backward reference against float64 torch autograd of the
forward reference it reverses, the forward coupling / finish references against oracle/glow_ref.py at dim 45 and 144, and the error model's
own arithmetic on a case worked by hand."""
import math
import zlib

import numpy as np
import pytest
import torch

import glow_stage_ref as gr
from oracle import glow_ref

F64 = torch.float64
DIMS = [(2, 0), (2, 1), (45, 0), (45, 1), (64, 0), (64, 1), (65, 1), (144, 0), (144, 1), (256, 0)]


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _close(a, b, what, tol=1e-12):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol * (1.0 + float(b.abs().max())), (what, err)


def test_error_model_on_a_case_worked_by_hand():
    u = gr.U32
    p = gr.mul(3.0, 0.5)                                     # one rounding of 1.5
    assert float(p.v) == 1.5 and abs(float(p.e) - (1.5 * u + gr.TINY)) < 1e-20
    s = gr.add(p, 2.0)                                       # carries the product's error, adds one rounding of 3.5
    assert float(s.v) == 3.5 and abs(float(s.e) - (1.5 * u + 3.5 * u + 2 * gr.TINY)) < 1e-20
    q = gr.div(s, 7.0)                                       # (error of the numerator) / 7 + one rounding of 0.5
    assert float(q.v) == 0.5 and abs(float(q.e) - (5.0 * u / 7 + 0.5 * u + gr.TINY * (2 / 7 + 1))) < 1e-20
    t = gr.vsum(gr.V(torch.tensor([1.0, -2.0, 4.0])), 0, 5)
    assert float(t.v) == 3.0 and abs(float(t.e) - (5 * u * 7.0 + gr.TINY)) < 1e-20
    sg = gr.sigmoid(torch.tensor([0.0, -104.0, 104.0], dtype=F64))
    assert float(sg.v[0]) == 0.5 and 0 < float(sg.v[1]) < 1e-45 < gr.TINY <= float(sg.e[1]) and float(sg.v[2]) == 1.0


@pytest.mark.parametrize("row_div,n_img,R", [(1, 1, 5), (1, 3, 7), (5, 3, 15), (1, 4, 4)])
def test_elementwise_forward_references(row_div, n_img, R):
    g = _gen(row_div, n_img, R)
    C = 12
    H, T, img = _rn(g, R, C), _rn(g, R, C), _rn(g, n_img, C)
    rows = torch.tensor([(r // row_div) % n_img for r in range(R)])
    _close(gr.add_image_rows(H, img, row_div, n_img).v, H + img[rows], "add_image_rows")
    _close(gr.glu_residual(H, T, img, row_div, n_img).v, H + T * torch.sigmoid(img[rows]), "glu_residual")
    _close(gr.glu_residual(H, T, img, row_div, n_img).v, H + torch.nn.functional.glu(torch.cat([T, img[rows]], 1), 1), "F.glu")
    _close(gr.relu_copy(H), torch.relu(H), "relu_copy")
    x = _rn(g, R, 45)
    p = gr.pad64(x)
    assert p.shape == (R, 64) and torch.equal(p[:, :45], x) and not p[:, 45:].any()


@pytest.mark.parametrize("row_div,n_img,R", [(1, 1, 5), (1, 3, 7), (5, 3, 15)])
def test_glu_bwd_against_autograd(row_div, n_img, R):
    g = _gen("glu", row_div, n_img, R)
    C = 8
    H, T, gate, g_h = _rn(g, R, C), _rn(g, R, C).requires_grad_(), _rn(g, n_img, C).requires_grad_(), _rn(g, R, C)
    (gr.glu_residual(H, T, gate, row_div, n_img).v * g_h).sum().backward()
    g_t3, g_rows = gr.glu_bwd(g_h, T.detach(), gate.detach(), row_div, n_img)
    _close(g_t3.v, T.grad, "g_t3")
    per_image = torch.zeros(n_img, C, dtype=F64).index_add(0, gr.image_of(R, row_div, n_img), g_rows.v)
    _close(per_image, gate.grad, "g_gate rows summed per image")
    assert (g_t3.e > 0).all() and (g_rows.e > 0).all()


def test_relu_bwd_add_against_autograd():
    g = _gen("relu")
    h, gg, acc = _rn(g, 40).requires_grad_(), _rn(g, 40), _rn(g, 40)
    with torch.no_grad():
        h[:3] = torch.tensor([0.0, -0.0, 2.0 ** -149])
    (torch.relu(h) * gg).sum().backward()
    _close(gr.relu_bwd_add(acc, gg, h.detach()).v, acc + h.grad, "relu_bwd_add")
    assert gr.relu_bwd_add(acc, gg, h.detach()).v[2] == acc[2] + gg[2], "the smallest subnormal opens the gate"


def _coupling_operands(dim, first, T, R=5):
    g = _gen("cp", dim, first, T)
    ldp = gr.pad_cols(2 * T)
    prm = _rn(g, R, ldp)
    prm[0, T:T + 4][:T] = torch.tensor([-120.0, -2.0, 0.0, 40.0], dtype=F64)[:T]
    return _rn(g, R, gr.pad_cols(dim)), prm, _rn(g, R, gr.pad_cols(dim)), _rn(g, R)


@pytest.mark.parametrize("dim,first", DIMS)
@pytest.mark.parametrize("full", [True, False])
def test_coupling_reverse_references_against_autograd(dim, first, full):
    T = gr.t_max(dim, first) if full else 1
    v0, prm0, g_y, a = _coupling_operands(dim, first, T)
    ld = v0.shape[1]
    for inverse, bwd in ((1, gr.coupling_inv_bwd), (0, gr.coupling_fwd_bwd)):
        v, prm = v0.clone().requires_grad_(), prm0.clone().requires_grad_()
        y, logdet = gr.coupling(v, prm, dim, first, T, inverse)
        assert y.v.shape == (5, ld) and not y.v[:, dim:].any()
        # the sampling direction's log q gains + sum log scale = - (the inverse's log|det|); the density direction's log p gains log|det|
        ((y.v[:, :dim] * g_y[:, :dim]).sum() + (a * (-logdet.v if inverse else logdet.v)).sum()).backward()
        g_v, g_prm = bwd(v0, prm0, g_y, dim, first, T, gr.V(a) if inverse else a)
        _close(g_v.v[:, :dim], v.grad[:, :dim], ("g_v", inverse))
        _close(g_prm.v[:, :2 * T], prm.grad[:, :2 * T], ("g_prm", inverse), tol=1e-11)
        assert not g_v.v[:, dim:].any() and not g_prm.v[:, 2 * T:].any()
        g_v0, _ = bwd(v0, prm0, g_y, dim, first, T, None)
        _close(g_v0.v, g_v.v, "g_v does not depend on the adjoint of the log-density")


@pytest.mark.parametrize("dim", [2, 45, 64, 144])
def test_base_density_bwd_against_autograd_of_finish(dim):
    g = _gen("bd", dim)
    R, ld = 4, gr.pad_cols(dim)
    z = _rn(g, R, ld).requires_grad_()
    g_z, g_logp, logdet = _rn(g, R, dim), _rn(g, R), _rn(g, R)
    lp = gr.finish(z, logdet, dim, 1.0, torch.tensor([0.25, -1.5]))
    ((z[:, :dim] * g_z).sum() + (lp.v * g_logp).sum()).backward()
    _close(gr.base_density_bwd(z.detach(), g_z, g_logp, dim).v, z.grad, "g_z and g_logp")
    assert not z.grad[:, dim:].any()
    for gz, gl in ((None, g_logp), (g_z, None), (None, None)):
        want = (0 if gz is None else gr.pad64(gz, ld)) - (0 if gl is None else gl[:, None] * gr.pad64(z.detach()[:, :dim], ld))
        _close(gr.base_density_bwd(z.detach(), gz, gl, dim).v, want + torch.zeros(R, ld, dtype=F64), "an absent operand is a zero")


@pytest.mark.parametrize("C,N,B", [(4, 1, 1), (8, 7, 3), (512, 5, 2)])
def test_per_image_reverse_stages_against_autograd(C, N, B):
    g = _gen("rows", C, N, B)
    H, T, gate, g_h = _rn(g, N * B, C), _rn(g, N * B, C).requires_grad_(), _rn(g, B, C).requires_grad_(), _rn(g, N * B, C)
    (gr.glu_residual(H, T, gate, 1, B).v * g_h).sum().backward()            # rows r = n B + b: image r % B
    g_t3, gct, bsum = gr.glu_bwd_sum(g_h, T.detach(), gate.detach(), N, B)
    _close(g_t3.v, T.grad, "g_t3")
    _close(gct.v, gate.grad, "gct")
    _close(bsum.v, T.grad.view(N, B, C).sum(0), "bsum = the column sums of g_t3 per image")
    # mask_scale_sum: t2 = dropout(relu(h)) = relu(h) keep scale; the gradient of h is g scale [t2 > 0], here as the bf16 values stored
    h = _rn(g, N * B, C).requires_grad_()
    keep = (torch.rand(N * B, C, generator=g) < 0.8).to(F64)
    gg = _rn(g, N * B, C).to(torch.bfloat16).to(F64)
    t2 = torch.relu(h) * keep * 1.25
    (t2 * gg).sum().backward()
    st, bs = gr.mask_scale_sum(gg, t2.detach(), 1.25, N, B)
    assert float((st - h.grad).abs().max()) <= gr.UB * float(h.grad.abs().max())
    assert torch.equal(st, st.to(torch.bfloat16).to(F64)) and torch.equal(bs.v, st.view(N, B, C).sum(0))
    assert gr.rows_chain(200, 512) == 4 * 13 + 4 and gr.rows_chain(5, 2048) == 4 * 2 + 1 and gr.rows_chain(1, 4) == 4 + 512


@pytest.mark.parametrize("dim", [45, 144])
def test_coupling_and_finish_against_the_oracle(dim):
    g = _gen("oracle", dim)
    R = 6
    for l, (idf, trf) in enumerate(glow_ref.masks(dim, 2)):
        first, T = int(trf[0]), trf.numel()
        assert first == 1 - l and T == gr.t_max(dim, first)
        x, params, seed = _rn(g, R, dim), _rn(g, R, 2 * T), _rn(g, R)
        scale, shift = glow_ref._scale_shift(params, T)
        prm = gr.pad64(params, gr.pad_cols(2 * T))
        y = x.clone()
        y[:, trf] = x[:, trf] * scale + shift
        got, logdet = gr.coupling(gr.pad64(x), prm, dim, first, T, 0, seed)
        _close(got.v, gr.pad64(y), "forward", tol=1e-9)          # (the oracle's 1e-3 is the float64 constant, the kernels' the float32 one)
        _close(logdet.v, seed + torch.log(scale).sum(1), "forward logdet", tol=1e-9)
        back, logdet2 = gr.coupling(got.v, prm, dim, first, T, 1, logdet.v)
        _close(back.v, gr.pad64(x), "inverse of forward", tol=1e-9)
        _close(logdet2.v, seed, "logdet returns to its seed")
        yi = x.clone()
        yi[:, trf] = (x[:, trf] - shift) / scale
        _close(gr.coupling(gr.pad64(x), prm, dim, first, T, 1)[0].v, gr.pad64(yi), "inverse", tol=1e-9)
        parts = _rn(g, 3)
        for sign in (1.0, -1.0):
            lp = gr.finish(gr.pad64(x), seed, dim, sign, parts)
            _close(lp.v, glow_ref.std_normal_log_prob(x) + sign * seed + parts.sum(), "finish", tol=1e-7)      # (log(2 pi) as float32)
        _close(gr.finish(gr.pad64(x), seed, dim, -1.0, parts[:0], host_const=0.75).v, glow_ref.std_normal_log_prob(x) - (seed + 0.75), "finish, host constant", tol=1e-7)


def test_linear_reference():
    g = _gen("lin")
    x, w, b = _rn(g, 5, 32), _rn(g, 8, 32), _rn(g, 8)
    y, mag = gr.linear(x, w, b, relu=True)
    _close(y, torch.relu(torch.nn.functional.linear(x, w, b)), "linear")
    assert (mag >= y.abs() - 1e-12).all() and gr.linear_bound(mag, 64).shape == mag.shape
    assert math.isclose(float(gr.linear_bound(torch.tensor(1.0), 64)), 22 * 2.0 ** -24)
    assert np.float32(gr.C1E3) == np.float32(1e-3) and gr.C1E3 != 1e-3
