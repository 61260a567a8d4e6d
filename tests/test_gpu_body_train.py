"""GPU tests of the body flow head's reverse pass (BodyFlowHead under grad: body._flow_backward over glow.ConditionalGlow._reverse): the new kernels - the wide float64 affine
map and its reverse (csrc/glow_affine_wide.hip), the wide coupling reverse (csrc/glow.hip), the joint reverse (csrc/body.hip) - and the whole head,
each against torch autograd in float64 on CPU over the oracle chain (oracle/glow_ref.py -> oracle/rot6d_ref.py -> oracle/body_ref.py)."""
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


def _glow(D, H, L, NB, Fc, seed):
    from mhentropy_amd.glow import ConditionalGlow
    g = ConditionalGlow(D, H, L, NB, context_features=Fc, dropout_probability=0.0)
    sd = synth.glow_state(seed, D, H, L, NB, Fc)
    g.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    return g.cuda().eval(), sd


def test_wide_affine_forward_and_reverse_vs_f64(gpu_lib):
    """D = 144, 4 layers: A, c, A^-1, c^-1, constants within 2 f32 ulp of f64 torch.linalg.inv; reverse within rel 1e-9 of f64 autograd;
    two runs bit-identical"""
    from mhentropy_amd import ops
    from oracle import glow_ref
    D, L, Dp = 144, 4, 192
    g, sd = _glow(D, 64, L, 1, 64, 11)
    ptab = g.small_param_table()
    out = ops.glow_affine_wide(ptab, L, D, 1e-3)
    again = ops.glow_affine_wide(ptab, L, D, 1e-3)
    with pytest.raises(Exception, match="device memory"):          # host pointers are refused
        ops.glow_affine_wide(ptab.cpu(), L, D, 1e-3)
    for k in ("A", "c", "Ainv", "AinvT", "cinv", "const_parts"):
        assert torch.equal(out[k], again[k]), k
    rng = np.random.default_rng(5)
    gA = torch.zeros(L, Dp, Dp); gA[:, :D, :D] = torch.as_tensor(rng.normal(0, 1, (L, D, D)).astype(np.float32))
    gc = torch.zeros(L, Dp); gc[:, :D] = torch.as_tensor(rng.normal(0, 1, (L, D)).astype(np.float32))
    gq = torch.as_tensor(rng.normal(0, 1, 37).astype(np.float32))
    gr = ops.glow_affine_wide_bwd(gA.cuda(), gc.cuda(), gq.cuda(), L, D, out["ws"]).cpu()
    gr2 = ops.glow_affine_wide_bwd(gA.cuda(), gc.cuda(), gq.cuda(), L, D, again["ws"]).cpu()
    assert torch.equal(gr, gr2)
    n = D * (D - 1) // 2
    names = ("log_scale", "shift", "lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")
    S = float(gq.double().sum())
    for l in range(L):
        p0, p1 = glow_ref.layer_prefix(l, 0), glow_ref.layer_prefix(l, 1)
        leaf = {k: _f64(sd[(p0 if k in ("log_scale", "shift") else p1) + k]).requires_grad_() for k in names}
        s64 = {p1 + k: leaf[k] for k in names[2:]}
        W, diag = glow_ref.lu_weight(s64, p1)
        A = W * torch.exp(leaf["log_scale"])[None, :]
        c = W @ leaf["shift"] + leaf["bias"]
        Ainv = torch.linalg.inv(A)
        cinv = -(Ainv @ c)
        const = leaf["log_scale"].sum() + torch.log(diag).sum()
        for name, got, ref in (("A", out["A"][l, :D, :D], A), ("c", out["c"][l, :D], c), ("Ainv", out["Ainv"][l, :D, :D], Ainv),
                               ("AinvT", out["AinvT"][l, :D, :D], Ainv.t()), ("cinv", out["cinv"][l, :D], cinv), ("const", out["const_parts"][l:l + 1], const.view(1))):
            r = ref.detach().numpy()
            ulp = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
            err = np.abs(got.cpu().numpy().astype(np.float64) - r)
            assert (err <= 2 * ulp).all(), (name, l, float((err / ulp).max()))
        assert float(out["A"][l, D:].abs().max()) == 0.0 and float(out["Ainv"][l, :, D:].abs().max()) == 0.0
        loss = (gA[l, :D, :D].double() * Ainv).sum() + (gc[l, :D].double() * cinv).sum() + S * const
        loss.backward()
        r = gr[l]
        parts = {"log_scale": r[:D], "shift": r[D:2 * D], "lower_entries": r[2 * D:2 * D + n], "upper_entries": r[2 * D + n:2 * D + 2 * n],
                 "unconstrained_upper_diag": r[2 * D + 2 * n:3 * D + 2 * n], "bias": r[3 * D + 2 * n:]}
        for k in names:
            ref = leaf[k].grad.numpy()
            err = float(np.abs(parts[k].numpy() - ref).max())
            assert err <= 1e-9 * float(np.abs(ref).max()), (k, l, err, float(np.abs(ref).max()))


@pytest.mark.parametrize("first", [0, 1])
def test_wide_coupling_reverse_vs_f64(gpu_lib, first):
    from mhentropy_amd import ops
    R, D, Dp, T = 50, 144, 192, 72
    rng = np.random.default_rng(first)
    v = torch.zeros(R, Dp); v[:, :D] = torch.as_tensor(rng.normal(0, 1, (R, D)).astype(np.float32))
    prm = torch.as_tensor(rng.normal(0, 0.7, (R, Dp)).astype(np.float32)); prm[:, 2 * T:] = 0
    gy = torch.zeros(R, Dp); gy[:, :D] = torch.as_tensor(rng.normal(0, 1, (R, D)).astype(np.float32))
    gq = torch.as_tensor(rng.normal(0, 1, R).astype(np.float32))
    gv, gp = ops.glow_coupling_inv_bwd_wide(v.cuda(), prm.cuda(), gy.cuda(), gq.cuda(), D, first, T)
    v64, p64 = v[:, :D].double().requires_grad_(), prm[:, :2 * T].double().requires_grad_()
    cols = torch.arange(first, D, 2)
    scale = torch.sigmoid(p64[:, T:] + 2.0) + 1e-3
    y = v64.clone()
    y[:, cols] = (v64[:, cols] - p64[:, :T]) / scale
    loss = (gy[:, :D].double() * y).sum() + (gq.double() * torch.log(scale).sum(1)).sum()
    loss.backward()
    for name, got, ref in (("g_v", gv[:, :D], v64.grad), ("g_params", gp[:, :2 * T], p64.grad)):
        err = float((got.cpu().double() - ref).abs().max())
        assert err <= 1e-5 * float(ref.abs().max()), (name, err)
    assert float(gv[:, D:].abs().max()) == 0.0 and float(gp[:, 2 * T:].abs().max()) == 0.0


def _joint_reverse_case(tables, R, seed):
    from mhentropy_amd import body
    from oracle import body_ref, rot6d_ref
    layer = body.BodyLayer(tables).cuda()
    J, nb = layer.J, layer.nb
    rng = np.random.default_rng(seed)
    rm = rot6d_ref.rotation_from_ortho6d(torch.as_tensor(rng.normal(0, 1, (R, J, 6))))
    bt = torch.as_tensor(rng.normal(0, 1, (R, nb)))
    w = torch.as_tensor(rng.normal(0, 1, (R, J, 3)).astype(np.float32))
    g_rot, g_bt = body.lbs_pose_bwd(layer, rm.float().cuda().contiguous(), bt.float().cuda().contiguous(), w.cuda())
    tb = {k: (_f64(v) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v)) for k, v in tables.items()}
    rm64, bt64 = rm.float().double().requires_grad_(), bt.float().double().requires_grad_()
    _, joints = body_ref.lbs(tb, rm64, bt64)
    (joints * w.double()).sum().backward()
    for name, got, ref in (("g_rotmats", g_rot, rm64.grad), ("g_betas", g_bt, bt64.grad)):
        err = float((got.cpu().double() - ref).abs().max())
        assert err <= 1e-5 * float(ref.abs().max()), (name, err, float(ref.abs().max()))


def test_joint_reverse_smpl_size(gpu_lib):
    from mhentropy_amd import body
    _joint_reverse_case(body.synthetic_body_tables(3, NV=700), 64, 1)


def test_joint_reverse_mano_tree(gpu_lib):
    from oracle import mano_ref
    t = synth.mano_tables(0)
    _joint_reverse_case({"v_template": t["v_template"], "shapedirs": t["shapedirs"], "posedirs": t["posedirs"], "J_regressor": t["J_regressor"],
                         "weights": t["weights"], "parents": np.asarray(mano_ref.PARENTS)}, 40, 2)


# ---- the whole head -------------------------------------------------------------------------------------------------------------------
def _head(Fc, H, L, NB, seed=5, table_seed=2):
    from mhentropy_amd import body
    tables = body.synthetic_body_tables(table_seed)
    head = body.BodyFlowHead(tables, context_features=Fc, hidden=H, num_layers=L, num_blocks=NB)
    sd = synth.glow_state(seed, 144, H, L, NB, Fc)
    head.flow.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    return head.cuda().eval(), sd, tables


def _inputs(B, K, Fc, seed=3):
    rng = np.random.default_rng(seed)
    feats = rng.normal(0, 0.5, (B, Fc)).astype(np.float32)
    noise = rng.normal(0, 1, (B, K, 144)).astype(np.float32)
    noise[:, 0] = 0.0                                   # row 0: the mode sample (ProHMR)
    betas = rng.normal(0, 1, (B, 10)).astype(np.float32)
    return feats, noise, betas


def _loss(out, target, w, lp_from=1):
    return out["log_prob"][:, lp_from:].mean() + (w * (out["joints"] - target).abs()).sum() + 0.1 * out["pose6d"].square().mean()


def _check_head(Fc, H, L, NB, B, K, hyp_slice, bound, lp_from=1):
    from oracle import glow_ref, rot6d_ref, body_ref
    head, sd, tables = _head(Fc, H, L, NB)
    feats, noise, betas = _inputs(B, K, Fc)
    lo, hi = hyp_slice or (0, K)
    rng = np.random.default_rng(9)
    target = rng.normal(0, 0.3, (B, hi - lo, 24, 3)).astype(np.float32)
    w = rng.random((B, hi - lo, 24, 1)).astype(np.float32) / (B * (hi - lo))
    f, b = torch.as_tensor(feats).cuda().requires_grad_(), torch.as_tensor(betas).cuda().requires_grad_()
    out = head(f, K, betas=b, noise=torch.as_tensor(noise).cuda(), hyp_slice=hyp_slice, want_verts=False)
    _loss(out, torch.as_tensor(target).cuda(), torch.as_tensor(w).cuda(), lp_from).backward()
    # f64 oracle chain
    sd64 = {k: _f64(v).requires_grad_() for k, v in sd.items()}
    f64, b64 = _f64(feats).requires_grad_(), _f64(betas).requires_grad_()
    x, lp, _ = glow_ref.sample_and_log_prob(sd64, _f64(noise), f64, L, NB)
    p = x[:, lo:hi].reshape(-1, 24, 6)
    rm = rot6d_ref.rotation_from_ortho6d(p)
    tb = {k: (_f64(v) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v)) for k, v in tables.items()}
    _, joints = body_ref.lbs(tb, rm, b64.repeat_interleave(hi - lo, 0))
    _loss({"log_prob": lp, "joints": joints.view(B, hi - lo, 24, 3), "pose6d": x}, _f64(target), _f64(w), lp_from).backward()
    errs = {"feats": _rel_l2(f.grad.cpu(), f64.grad), "betas": _rel_l2(b.grad.cpu(), b64.grad)}
    for name, prm in head.flow.named_parameters():
        assert prm.grad is not None, name
        errs[name] = _rel_l2(prm.grad.cpu(), sd64[name].grad)
    worst = max(errs, key=errs.get)
    print(f"B={B} K={K} hidden={H} {L}x{NB} ctx={Fc} slice={hyp_slice}: worst per-tensor rel-L2 {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= bound, (worst, errs[worst])
    return head


@pytest.mark.parametrize("hyp_slice", [None, (2, 5)])
def test_head_gradients_small_geometry(gpu_lib, hyp_slice):
    _check_head(256, 128, 2, 1, 2, 6, hyp_slice, 1e-4)


def test_head_gradients_prohmr_geometry(gpu_lib):
    """hidden 1024, 4 layers x 2 blocks, context 2048, B = 4, K = 8.  Measured on an MI355X: worst per-tensor rel-L2 2.9e-6 (bound 1e-3)."""
    _check_head(2048, 1024, 4, 2, 4, 8, None, 1e-3)


@pytest.mark.parametrize("Fc, H, L, NB", [(256, 128, 2, 1), (2048, 1024, 4, 2)])
def test_head_gradients_one_sample(gpu_lib, Fc, H, L, NB):
    """K = 1 (ProHMR's mode sample, ConditionalGlow.forward's default): one row per image, with the log-probability itself in the loss"""
    _check_head(Fc, H, L, NB, 2, 1, None, 1e-4 if H == 128 else 1e-3, lp_from=0)


def test_grad_forward_equals_eval_forward(gpu_lib):
    head, _, _ = _head(256, 128, 2, 1)
    head.train()                                        # (dropout p = 0: train mode changes nothing but switches the grad path on)
    feats, noise, betas = (torch.as_tensor(a).cuda() for a in _inputs(2, 6, 256))
    with torch.no_grad():
        ref = head(feats, 6, betas=betas, noise=noise)
    out = head(feats, 6, betas=betas, noise=noise)
    assert out["log_prob"].requires_grad
    for k in ("pose6d", "log_prob", "joints", "vertices"):
        assert torch.equal(out[k].detach(), ref[k]), k
    with torch.no_grad():
        ref = head(feats, 6, betas=betas, noise=noise, hyp_slice=(1, 4))
    out = head(feats, 6, betas=betas, noise=noise, hyp_slice=(1, 4))
    for k in ("pose6d", "log_prob", "joints", "vertices"):
        assert torch.equal(out[k].detach(), ref[k]), k


def test_adam_training_reduces_loss(gpu_lib):
    head, _, _ = _head(256, 128, 2, 1)
    head.train()
    feats, noise, betas = (torch.as_tensor(a).cuda() for a in _inputs(2, 6, 256))
    target = torch.as_tensor(np.random.default_rng(4).normal(0, 0.3, (2, 6, 24, 3)).astype(np.float32)).cuda()
    opt = torch.optim.Adam(head.flow.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        out = head(feats, 6, betas=betas, noise=noise, want_verts=False)
        loss = out["log_prob"][:, 1:].mean() * 1e-3 + (out["joints"] - target).abs().mean()
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in head.flow.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    print("loss", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and all(torch.isfinite(p).all() for p in head.flow.parameters())
    assert losses[-1] < losses[0] - 0.1, losses                      # (measured on an MI355X: 0.020 -> -0.974)


def test_refusals(gpu_lib):
    head, _, _ = _head(256, 128, 2, 1)
    head.train()
    feats, noise, betas = (torch.as_tensor(a).cuda() for a in _inputs(2, 6, 256))
    out = head(feats, 6, betas=betas, noise=noise)
    with pytest.raises(NotImplementedError, match="vertex"):
        out["vertices"].sum().backward()
    head.flow.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match="float32"):
        head(feats, 6, betas=betas, noise=noise)
    with torch.no_grad():
        assert torch.isfinite(head(feats, 6, betas=betas, noise=noise)["log_prob"]).all()       # (the no-grad path still takes bf16)
    head.flow.compute_dtype = torch.float32
    head.flow.p_drop = 0.2
    with pytest.raises(NotImplementedError, match="dropout"):
        head(feats, 6, betas=betas, noise=noise)
