"""GPU tests of the DENSITY direction's reverse pass - ConditionalGlow.log_prob / BodyFlowHead.log_prob under grad, the maximum-likelihood loss of
the reference's README.md:32-34: the new kernels (forward-coupling reverse and base-density gradient in csrc/glow.hip, the float64 ActNorm / LU
reverse of that direction in csrc/glow_affine.hip and csrc/glow_affine_wide.hip) and the whole flow, each against torch autograd in float64 on the
CPU over the unmodified oracle (oracle/glow_ref.log_prob)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mhentropy_amd import synth

pytestmark = pytest.mark.gpu


def _f64(t):
    return torch.as_tensor(np.asarray(t, np.float64))


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _glow(D, H, L, NB, Fc, seed, p=0.0):
    from mhentropy_amd.glow import ConditionalGlow
    g = ConditionalGlow(D, H, L, NB, context_features=Fc, dropout_probability=p)
    sd = synth.glow_state(seed, D, H, L, NB, Fc)
    g.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    return g.cuda().eval(), sd


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [45, 144])
@pytest.mark.parametrize("first", [0, 1])
def test_forward_coupling_reverse_vs_f64(gpu_lib, D, first):
    """pitch 64 (D = 45) and 192 (D = 144), with and without dL/dlog p: max error <= 1e-5 of the reference tensor's max, padding exactly zero"""
    from mhentropy_amd import ops
    R, Dp = 50, (D + 63) // 64 * 64
    cols = torch.arange(first, D, 2)
    T = cols.numel()
    Pp = (2 * T + 63) // 64 * 64
    rng = np.random.default_rng(10 * D + first)
    v = torch.zeros(R, Dp); v[:, :D] = torch.as_tensor(rng.normal(0, 1, (R, D)).astype(np.float32))
    prm = torch.as_tensor(rng.normal(0, 0.7, (R, Pp)).astype(np.float32)); prm[:, 2 * T:] = 0
    gy = torch.zeros(R, Dp); gy[:, :D] = torch.as_tensor(rng.normal(0, 1, (R, D)).astype(np.float32))
    gq = torch.as_tensor(rng.normal(0, 1, R).astype(np.float32))
    for with_lp in (True, False):
        gv, gp = ops.glow_coupling_fwd_bwd(v.cuda(), prm.cuda(), gy.cuda(), gq.cuda() if with_lp else None, D, first, T)
        v64, p64 = v[:, :D].double().requires_grad_(), prm[:, :2 * T].double().requires_grad_()
        scale = torch.sigmoid(p64[:, T:] + 2.0) + 1e-3
        y = v64.clone()
        y[:, cols] = v64[:, cols] * scale + p64[:, :T]
        loss = (gy[:, :D].double() * y).sum()
        if with_lp:
            loss = loss + (gq.double() * torch.log(scale).sum(1)).sum()
        loss.backward()
        for name, got, ref in (("g_v", gv[:, :D], v64.grad), ("g_params", gp[:, :2 * T], p64.grad)):
            err = float((got.cpu().double() - ref).abs().max())
            assert err <= 1e-5 * float(ref.abs().max()), (name, with_lp, err)
        assert gv.shape == (R, Dp) and gp.shape == (R, Pp)
        assert (Dp == D or float(gv[:, D:].abs().max()) == 0.0) and (Pp == 2 * T or float(gp[:, 2 * T:].abs().max()) == 0.0)


def test_base_density_gradient(gpu_lib):
    """g_y = g_z - g_lp z on padded rows: one f32 multiply-add per element, compared with the same expression in f64 (1e-6 of the max: f32
    rounding of one product and one sum); padding exactly zero; either gradient may be absent"""
    from mhentropy_amd import ops
    R, D, Dp = 37, 144, 192
    rng = np.random.default_rng(3)
    z = torch.zeros(R, Dp); z[:, :D] = torch.as_tensor(rng.normal(0, 1, (R, D)).astype(np.float32))
    gz = torch.as_tensor(rng.normal(0, 1, (R, D)).astype(np.float32))
    gq = torch.as_tensor(rng.normal(0, 1, R).astype(np.float32))
    for a, b in ((gz, gq), (None, gq), (gz, None)):
        got = ops.glow_base_density_bwd(z.cuda(), None if a is None else a.cuda(), None if b is None else b.cuda(), D).cpu()
        ref = (0 if a is None else a.double()) - (0 if b is None else b.double()[:, None]) * z[:, :D].double()
        assert float((got[:, :D].double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
        assert float(got[:, D:].abs().max()) == 0.0


@pytest.mark.parametrize("D", [45, 144])
def test_density_affine_reverse_vs_f64(gpu_lib, D):
    """narrow (D = 45, csrc/glow_affine.hip) and wide (D = 144, csrc/glow_affine_wide.hip), 4 layers, random dA, dc, 37 dL/dlog p rows: every
    parameter gradient within 1e-9 (relative to the tensor's max) of f64 autograd; two runs bit-identical; host pointers refused"""
    from mhentropy_amd import ops, _lib
    from oracle import glow_ref
    L, Dp = 4, (D + 63) // 64 * 64
    g, sd = _glow(D, 64, L, 1, 64, 11)
    ptab = g.small_param_table()
    aff = (ops.glow_affine if D <= 64 else ops.glow_affine_wide)(ptab, L, D, 1e-3)
    rng = np.random.default_rng(5)
    gA = torch.zeros(L, Dp, Dp); gA[:, :D, :D] = torch.as_tensor(rng.normal(0, 1, (L, D, D)).astype(np.float32))
    gc = torch.zeros(L, Dp); gc[:, :D] = torch.as_tensor(rng.normal(0, 1, (L, D)).astype(np.float32))
    gq = torch.as_tensor(rng.normal(0, 1, 37).astype(np.float32))
    gr = ops.glow_affine_density_bwd(gA.cuda(), gc.cuda(), gq.cuda(), L, D, aff["ws"]).cpu()
    gr2 = ops.glow_affine_density_bwd(gA.cuda(), gc.cuda(), gq.cuda(), L, D, aff["ws"]).cpu()
    assert gr.dtype == torch.float64 and torch.equal(gr, gr2)
    lib = _lib.lib()
    entry = lib.mhe_glow_affine_density_bwd_f64 if D <= 64 else lib.mhe_glow_affine_wide_density_bwd_f64
    host, out = np.zeros(L * Dp * Dp, np.float32), torch.empty_like(gr).cuda()
    with pytest.raises(_lib.MheError, match="device memory"):
        _lib.check(entry(C.c_void_p(host.ctypes.data), ops._ptr(gc.cuda()), None, 0, L, D, ops._ptr(aff["ws"]), ops._ptr(out), ops._stream()), "density_bwd")
    n = D * (D - 1) // 2
    names = ("log_scale", "shift", "lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")
    S = float(gq.double().sum())
    for l in range(L):
        p0, p1 = glow_ref.layer_prefix(l, 0), glow_ref.layer_prefix(l, 1)
        leaf = {k: _f64(sd[(p0 if k in ("log_scale", "shift") else p1) + k]).requires_grad_() for k in names}
        W, diag = glow_ref.lu_weight({p1 + k: leaf[k] for k in names[2:]}, p1)
        A = W * torch.exp(leaf["log_scale"])[None, :]
        c = W @ leaf["shift"] + leaf["bias"]
        const = leaf["log_scale"].sum() + torch.log(diag).sum()
        ((gA[l, :D, :D].double() * A).sum() + (gc[l, :D].double() * c).sum() + S * const).backward()
        r = gr[l]
        parts = {"log_scale": r[:D], "shift": r[D:2 * D], "lower_entries": r[2 * D:2 * D + n], "upper_entries": r[2 * D + n:2 * D + 2 * n],
                 "unconstrained_upper_diag": r[2 * D + 2 * n:3 * D + 2 * n], "bias": r[3 * D + 2 * n:]}
        for k in names:
            ref = leaf[k].grad.numpy()
            err = float(np.abs(parts[k].numpy() - ref).max())
            assert err <= 1e-9 * float(np.abs(ref).max()), (k, l, err, float(np.abs(ref).max()))


# ---- the whole flow -------------------------------------------------------------------------------------------------------------------
def _loss(lp, z, w):
    return -(w * lp).sum() + 0.01 * z.square().mean()


def _check_flow(D, H, L, NB, Fc, R, Bc, bound, p=0.0):
    """per-tensor rel-L2 of every parameter gradient, dL/dinputs and dL/dcontext against the f64 oracle; Bc context rows (Bc < R: sample-major
    inputs, row r uses context[r % Bc]); p > 0: train mode, the device-drawn dropout masks handed to the oracle"""
    from mhentropy_amd import ops
    from oracle import glow_ref
    g, sd = _glow(D, H, L, NB, Fc, 7, p)
    rng = np.random.default_rng(13)
    x = rng.normal(0, 0.8, (R, D)).astype(np.float32)
    ctx = rng.normal(0, 0.5, (Bc, Fc)).astype(np.float32)
    w = (0.2 + rng.random(R)).astype(np.float32)
    masks = None
    if p > 0:
        g.train()
        g.record_masks, g.last_masks = True, []
        ops.rng_state(torch.device("cuda", torch.cuda.current_device()), seed=21)        # the same masks in every run of the test
    xg, cg = torch.as_tensor(x).cuda().requires_grad_(), torch.as_tensor(ctx).cuda().requires_grad_()
    lp, z = g.log_prob(xg, context=cg)
    assert lp.shape == (R,) and z.shape == (R, D) and lp.requires_grad and z.requires_grad
    _loss(lp, z, torch.as_tensor(w).cuda()).backward()
    if p > 0:
        g.record_masks = False
        assert len(g.last_masks) == L * NB
        masks = [ops.dropout_mask(b, (R, H), g.p_drop).cpu().double() for b in g.last_masks]
    sd64 = {k: _f64(v).requires_grad_() for k, v in sd.items()}
    x64, c64 = _f64(x).requires_grad_(), _f64(ctx).requires_grad_()
    lp64, z64 = glow_ref.log_prob(sd64, x64, c64.repeat(R // Bc, 1), L, NB, masks=masks)
    _loss(lp64, z64, _f64(w)).backward()
    assert _rel_l2(lp.detach().cpu(), lp64.detach()) <= 1e-4 and _rel_l2(z.detach().cpu(), z64.detach()) <= 1e-4
    errs = {"inputs": _rel_l2(xg.grad.cpu(), x64.grad), "context": _rel_l2(cg.grad.cpu(), c64.grad)}
    for name, prm in g.named_parameters():
        assert prm.grad is not None and sd64[name].grad is not None, name
        errs[name] = _rel_l2(prm.grad.cpu(), sd64[name].grad)
    assert len(errs) == len(list(g.parameters())) + 2 and len(errs) == L * (10 + 6 * NB) + 2          # (no tensor skipped)
    worst = max(errs, key=errs.get)
    print(f"D={D} hidden={H} {L}x{NB} ctx={Fc} R={R} Bc={Bc} p={p}: worst per-tensor rel-L2 {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= bound, (worst, errs[worst])


@pytest.mark.parametrize("D, Fc", [(144, 256), (45, 128)])
def test_log_prob_gradients_small_geometry(gpu_lib, D, Fc):
    """hidden 128, 2 layers x 1 block, R = 6.  Bound 1e-4.  Measured on an MI355X: worst per-tensor rel-L2 3.6e-7 (D = 144, context 256; a block
    weight), 2.6e-7 (D = 45, context 128; dL/dcontext)"""
    _check_flow(D, 128, 2, 1, Fc, 6, 6, 1e-4)


@pytest.mark.parametrize("Bc", [12, 3])
def test_log_prob_gradients_hand_geometry(gpu_lib, Bc):
    """the hand flow as the reference builds it (45, 512, 4, 2, context 512), R = 12: R context rows, and B = 3 context rows with sample-major
    inputs.  Bound 1e-3.  Measured on an MI355X: worst per-tensor rel-L2 9.3e-7 (R context rows), 9.8e-7 (B = 3), both dL/dcontext"""
    _check_flow(45, 512, 4, 2, 512, 12, Bc, 1e-3)


def test_log_prob_gradients_prohmr_geometry(gpu_lib):
    """(144, 1024, 4, 2, context 2048), R = 8.  Bound 1e-3.  Measured on an MI355X: worst per-tensor rel-L2 1.3e-6 (dL/dcontext)"""
    _check_flow(144, 1024, 4, 2, 2048, 8, 8, 1e-3)


def test_log_prob_gradients_with_dropout(gpu_lib):
    """hand geometry, train mode, p = 0.2: the mask bits drawn on the device are on the tape and handed to the oracle.  Bound 1e-3.
    Measured on an MI355X: worst per-tensor rel-L2 9.6e-7 (dL/dcontext)"""
    _check_flow(45, 512, 4, 2, 512, 12, 12, 1e-3, p=0.2)


def test_wide_flow_refuses_train_mode_dropout(gpu_lib):
    g, _ = _glow(144, 128, 2, 1, 256, 7, p=0.2)
    g.train()
    x, ctx = torch.zeros(4, 144, device="cuda"), torch.zeros(4, 256, device="cuda")
    with pytest.raises(NotImplementedError, match="dropout"):
        g.log_prob(x, context=ctx)


@pytest.mark.parametrize("D, Fc", [(144, 256), (45, 128)])
def test_grad_values_equal_the_inference_pass(gpu_lib, D, Fc):
    g, _ = _glow(D, 128, 2, 1, Fc, 7)
    rng = np.random.default_rng(2)
    x = torch.as_tensor(rng.normal(0, 0.8, (12, D)).astype(np.float32)).cuda()
    for Bc in (12, 3):
        ctx = torch.as_tensor(rng.normal(0, 0.5, (Bc, Fc)).astype(np.float32)).cuda()
        g.eval()
        plain = g.log_prob(x, context=ctx)
        assert not plain[0].requires_grad and not plain[1].requires_grad and plain[0].grad_fn is None
        with torch.no_grad():
            ref = g.log_prob(x, context=ctx)
        g.train()                                       # (dropout p = 0: train mode changes nothing but switches the grad path on)
        lp, z = g.log_prob(x, context=ctx)
        assert lp.requires_grad and z.requires_grad
        assert torch.equal(lp.detach(), ref[0]) and torch.equal(z.detach(), ref[1]) and torch.equal(plain[0], ref[0])
        g.eval()
        lp, z = g.log_prob(x.clone().requires_grad_(), context=ctx)
        assert lp.requires_grad and torch.equal(lp.detach(), ref[0]) and torch.equal(z.detach(), ref[1])


def test_bf16_refused_under_grad(gpu_lib):
    g, _ = _glow(144, 128, 2, 1, 256, 7)
    g.train()
    g.compute_dtype = torch.bfloat16
    x, ctx = torch.randn(4, 144, device="cuda") * 0.5, torch.randn(4, 256, device="cuda") * 0.5
    with pytest.raises(NotImplementedError, match="float32"):
        g.log_prob(x, context=ctx)
    with torch.no_grad():
        assert torch.isfinite(g.log_prob(x, context=ctx)[0]).all()       # (the no-grad path still takes bf16)


# ---- the body head ----------------------------------------------------------------------------------------------------------------------
def _head(Fc, H, L, NB, seed=5):
    from mhentropy_amd import body
    head = body.BodyFlowHead(body.synthetic_body_tables(2, NV=700), context_features=Fc, hidden=H, num_layers=L, num_blocks=NB)
    sd = synth.glow_state(seed, 144, H, L, NB, Fc)
    head.flow.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    return head.cuda().eval(), sd


def test_head_log_prob_call_forms(gpu_lib):
    from mhentropy_amd import body
    from oracle import rot6d_ref
    head, _ = _head(256, 128, 2, 1)
    rng = np.random.default_rng(8)
    M = rot6d_ref.rotation_from_ortho6d(torch.as_tensor(rng.normal(0, 1, (5 * 24, 6)))).float().view(5, 24, 3, 3).cuda()
    feats = torch.as_tensor(rng.normal(0, 0.5, (5, 256)).astype(np.float32)).cuda()
    p6 = body.rotmat_to_rot6d(M)
    assert p6.shape == (5, 24, 6)
    back = body.rot6d_to_rotmat(p6.contiguous())
    assert float((back - M).abs().max()) <= 1e-6
    a = head.log_prob(feats, rotmats=M)
    b = head.flow.log_prob(p6.reshape(-1, 144), feats)
    c = head.log_prob(feats, pose6d=p6.reshape(-1, 144))
    assert a[0].shape == (5,) and a[1].shape == (5, 144)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0])
    with pytest.raises(ValueError):
        head.log_prob(feats)
    with pytest.raises(ValueError):
        head.log_prob(feats, pose6d=p6.reshape(-1, 144), rotmats=M)


def test_nll_and_entropy_in_one_step(gpu_lib):
    """small geometry, B = 2, K = 6: the NLL node and the sampling node in one loss, one backward; every parameter gradient and dL/dfeats against
    the oracle's sum of the two terms.  Bound 1e-4.  Measured on an MI355X: worst per-tensor rel-L2 4.0e-7 (a context-layer bias)"""
    from oracle import glow_ref
    Fc, H, L, NB, B, K = 256, 128, 2, 1, 2, 6
    head, sd = _head(Fc, H, L, NB)
    rng = np.random.default_rng(17)
    feats = rng.normal(0, 0.5, (B, Fc)).astype(np.float32)
    pose = rng.normal(0, 0.8, (B, 144)).astype(np.float32)
    noise = rng.normal(0, 1, (B, K, 144)).astype(np.float32)
    noise[:, 0] = 0.0
    f = torch.as_tensor(feats).cuda().requires_grad_()
    loss = -head.log_prob(f, pose6d=torch.as_tensor(pose).cuda())[0].mean() \
        + head(f, K, noise=torch.as_tensor(noise).cuda(), want_verts=False)["log_prob"][:, 1:].mean()
    loss.backward()
    sd64 = {k: _f64(v).requires_grad_() for k, v in sd.items()}
    f64 = _f64(feats).requires_grad_()
    ref = -glow_ref.log_prob(sd64, _f64(pose), f64, L, NB)[0].mean() + glow_ref.sample_and_log_prob(sd64, _f64(noise), f64, L, NB)[1][:, 1:].mean()
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-4 * abs(float(ref.detach()))
    errs = {"feats": _rel_l2(f.grad.cpu(), f64.grad)}
    for name, prm in head.flow.named_parameters():
        assert prm.grad is not None, name
        errs[name] = _rel_l2(prm.grad.cpu(), sd64[name].grad)
    worst = max(errs, key=errs.get)
    print(f"NLL + entropy: worst per-tensor rel-L2 {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= 1e-4, (worst, errs[worst])


def test_adam_on_the_nll_reduces_it(gpu_lib):
    head, _ = _head(256, 128, 2, 1)
    head.train()
    rng = np.random.default_rng(4)
    feats = torch.as_tensor(rng.normal(0, 0.5, (16, 256)).astype(np.float32)).cuda()
    pose = torch.as_tensor(rng.normal(0, 0.8, (16, 144)).astype(np.float32)).cuda()
    opt = torch.optim.Adam(head.flow.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = -head.log_prob(feats, pose6d=pose)[0].mean()
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in head.flow.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    print("nll", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and all(torch.isfinite(p).all() for p in head.flow.parameters())
    assert losses[-1] < losses[0] - 30.0, losses                     # (measured on an MI355X: 203.3 -> 127.2)
