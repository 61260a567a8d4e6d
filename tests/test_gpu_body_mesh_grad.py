"""GPU tests of the body flow head's reverse pass through its mesh: the skinning reverse (csrc/lbs_skin_bwd.hip: mhe_lbs_bwd_tables_f32,
mhe_lbs_skin_bwd_f32), the pose chain's reverse from the skinning transforms (csrc/body.hip: mhe_lbs_transforms_bwd_f32), body.lbs_bwd and
BodyFlowHead(verts_grad=True), each against torch autograd in float64 on CPU over the oracle chain (oracle/glow_ref.py -> oracle/rot6d_ref.py ->
oracle/body_ref.py)."""
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


def _mano_tables():
    from oracle import mano_ref
    t = synth.mano_tables(0)
    return {"v_template": t["v_template"], "shapedirs": t["shapedirs"], "posedirs": t["posedirs"], "J_regressor": t["J_regressor"],
            "weights": t["weights"], "parents": np.asarray(mano_ref.PARENTS)}


_TABLES = {}


def _tables(name):
    from mhentropy_amd import body
    if name not in _TABLES:
        _TABLES[name] = _mano_tables() if name == "mano" else body.synthetic_body_tables(4)
    return _TABLES[name]


@pytest.mark.parametrize("with_joints", [False, True])
@pytest.mark.parametrize("model", ["mano", "smpl"])
def test_lbs_bwd_vs_f64(gpu_lib, model, with_joints):
    """body.lbs_bwd against f64 autograd of body_ref.lbs (scale 0.7; R = 1, 5, 33, 70: rows past a multiple of 32 included).
    Measured on an MI355X: worst per-tensor rel-L2 4.8e-7 (MANO), 1.9e-6 (SMPL size) (bound 1e-4)."""
    from mhentropy_amd import body
    from oracle import body_ref, rot6d_ref
    tables = _tables(model)
    layer = body.BodyLayer(tables).cuda()
    J, nb, NV, scale = layer.J, layer.nb, layer.NV, 0.7
    tb = {k: (_f64(v) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v)) for k, v in tables.items()}
    worst = 0.0
    for R in (1, 5, 33, 70):
        rng = np.random.default_rng(R + 100 * with_joints)
        rm = rot6d_ref.rotation_from_ortho6d(torch.as_tensor(rng.normal(0, 1, (R, J, 6)))).float()
        bt = torch.as_tensor(rng.normal(0, 1, (R, nb)).astype(np.float32))
        gv = torch.as_tensor(rng.normal(0, 1, (R, NV, 3)).astype(np.float32))
        gj = torch.as_tensor(rng.normal(0, 1, (R, J, 3)).astype(np.float32)) if with_joints else None
        g_rot, g_bt = body.lbs_bwd(layer, rm.cuda().contiguous(), bt.cuda().contiguous(), gv.cuda(), None if gj is None else gj.cuda(), scale=scale)
        g_rot2, g_bt2 = body.lbs_bwd(layer, rm.cuda().contiguous(), bt.cuda().contiguous(), gv.cuda(), None if gj is None else gj.cuda(), scale=scale)
        assert torch.equal(g_rot, g_rot2) and torch.equal(g_bt, g_bt2), "two calls differ"
        rm64, bt64 = rm.double().requires_grad_(), bt.double().requires_grad_()
        verts, joints = body_ref.lbs(tb, rm64, bt64)
        loss = (verts * scale * gv.double()).sum() + ((joints * gj.double()).sum() if gj is not None else 0.0)
        loss.backward()
        for name, got, ref in (("g_rotmats", g_rot, rm64.grad), ("g_betas", g_bt, bt64.grad)):
            err = _rel_l2(got.cpu(), ref)
            worst = max(worst, err)
            assert err <= 1e-4, (model, R, name, err)
    print(f"{model} joints={with_joints}: worst rel-L2 {worst:.2e}")


def test_transforms_bwd_reduces_to_pose_bwd(gpu_lib):
    """with zero transform and pose-map gradients the chain reverse is the joints-only reverse"""
    from mhentropy_amd import body, ops, _lib
    from oracle import rot6d_ref
    layer = body.BodyLayer(_tables("smpl")).cuda()
    R, J, nb = 37, layer.J, layer.nb
    rng = np.random.default_rng(7)
    rm = rot6d_ref.rotation_from_ortho6d(torch.as_tensor(rng.normal(0, 1, (R, J, 6)))).float().cuda().contiguous()
    bt = torch.as_tensor(rng.normal(0, 1, (R, nb)).astype(np.float32)).cuda()
    gj = torch.as_tensor(rng.normal(0, 1, (R, J, 3)).astype(np.float32)).cuda()
    ref_rot, ref_bt = body.lbs_pose_bwd(layer, rm, bt, gj)
    g_rot, g_bt = torch.empty_like(rm), torch.empty_like(bt)
    ops.check(_lib.lib().mhe_lbs_transforms_bwd_f32(ops._ptr(rm), ops._ptr(bt), ops._ptr(layer._jt), ops._ptr(layer._jsd), ops._ptr(layer.parents),
                                                    ops._ptr(gj), ops._ptr(torch.zeros(R, J, 12, device="cuda")),
                                                    ops._ptr(torch.zeros(R, 9 * (J - 1), device="cuda")), None, ops._ptr(g_rot), ops._ptr(g_bt), R, J,
                                                    nb, ops._stream()), "mhe_lbs_transforms_bwd_f32")
    assert torch.allclose(g_rot, ref_rot, rtol=1e-6, atol=1e-6) and torch.allclose(g_bt, ref_bt, rtol=1e-6, atol=1e-6)


def test_c_entries_refuse_bad_arguments(gpu_lib):
    from mhentropy_amd import body, ops, _lib
    L = _lib.lib()
    layer = body.BodyLayer(_tables("mano")).cuda()
    J, nb, NV, VP, R = layer.J, layer.nb, layer.NV, layer.VP, 3
    d = lambda *s: torch.zeros(*s, device="cuda")
    ws, tab = d(L.mhe_lbs_workspace_floats(R, J, nb)), layer._bwd_tables(torch.device("cuda"))
    gv, gtf, gpm, gbt = d(R, NV, 3), d(R, J, 12), d(R, 9 * (J - 1)), d(R, nb)
    P = ops._ptr
    skin = lambda ws_, J_: L.mhe_lbs_skin_bwd_f32(P(ws_), P(layer._vt), P(layer._vsd), P(layer._vpd), P(layer._vw), P(tab), P(gv), P(gtf), P(gpm),
                                                 P(gbt), R, J_, nb, NV, VP, 1.0, ops._stream())
    assert skin(ws, J) == 0
    assert skin(None, J) != 0 and b"null" in L.mhe_last_error()
    assert skin(ws, 33) != 0 and b"J=33" in L.mhe_last_error()
    assert L.mhe_lbs_skin_bwd_f32(P(ws), P(layer._vt), P(layer._vsd), P(layer._vpd), P(layer._vw), P(tab), P(gv), P(gtf), P(gpm), P(gbt), R, J, nb, NV,
                                  VP + 16, 1.0, ops._stream()) != 0
    assert L.mhe_lbs_bwd_tables_f32(P(layer._vsd), None, P(layer._vw), P(tab), J, nb, NV, VP, ops._stream()) != 0 and b"null" in L.mhe_last_error()
    assert L.mhe_lbs_bwd_tables_f32(P(layer._vsd), P(layer._vpd), P(layer._vw), P(tab), 33, nb, NV, VP, ops._stream()) != 0
    assert L.mhe_lbs_bwd_tables_floats(33, nb, VP) == 0 and L.mhe_lbs_bwd_tables_floats(J, nb, VP + 16) == 0
    rm, bt, grot = d(R, J, 3, 3), d(R, nb), d(R, J, 3, 3)
    chain = lambda tf_, J_: L.mhe_lbs_transforms_bwd_f32(P(rm), P(bt), P(layer._jt), P(layer._jsd), P(layer.parents), None, P(tf_), P(gpm), None,
                                                       P(grot), P(gbt), R, J_, nb, ops._stream())
    assert chain(gtf, J) == 0
    assert chain(None, J) != 0 and b"null" in L.mhe_last_error()
    assert chain(gtf, 33) != 0 and b"J=33" in L.mhe_last_error()
    torch.cuda.synchronize()


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
    noise[:, 0] = 0.0
    betas = rng.normal(0, 1, (B, 10)).astype(np.float32)
    return feats, noise, betas


def _extra_regressor(NV, E=9, seed=11):
    """sparse synthetic (E, NV) regressor: 'extra joints' as ProHMR's out-of-tree keypoint set builds them from the posed vertices"""
    rng = np.random.default_rng(seed)
    reg = rng.random((E, NV)) * (rng.random((E, NV)) < 0.003)
    reg[:, 0] += 1e-3
    return (reg / reg.sum(1, keepdims=True)).astype(np.float32)


def _loss(out, tj, tv, te, reg, w):
    extra = torch.einsum("ev,bkvc->bkec", reg, out["vertices"])
    return (out["log_prob"][:, 1:].mean() + (w * (out["joints"] - tj).abs()).sum() + (out["vertices"] - tv).abs().mean()
            + (extra - te).abs().mean())


def _targets(B, n, NV, E, seed=9):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.3, (B, n, 24, 3)).astype(np.float32), rng.normal(0, 0.3, (B, n, NV, 3)).astype(np.float32),
            rng.normal(0, 0.3, (B, n, E, 3)).astype(np.float32), (rng.random((B, n, 24, 1)) / (B * n)).astype(np.float32))


def _check_head(Fc, H, L, NB, B, K, hyp_slice, bound):
    from oracle import glow_ref, rot6d_ref, body_ref
    head, sd, tables = _head(Fc, H, L, NB)
    NV = head.body.NV
    feats, noise, betas = _inputs(B, K, Fc)
    lo, hi = hyp_slice or (0, K)
    reg = _extra_regressor(NV)
    tj, tv, te, w = _targets(B, hi - lo, NV, reg.shape[0])
    cu = lambda a: torch.as_tensor(a).cuda()
    f, b = cu(feats).requires_grad_(), cu(betas).requires_grad_()
    out = head(f, K, betas=b, noise=cu(noise), hyp_slice=hyp_slice, verts_grad=True)
    _loss(out, cu(tj), cu(tv), cu(te), cu(reg), cu(w)).backward()
    sd64 = {k: _f64(v).requires_grad_() for k, v in sd.items()}
    f64, b64 = _f64(feats).requires_grad_(), _f64(betas).requires_grad_()
    x, lp, _ = glow_ref.sample_and_log_prob(sd64, _f64(noise), f64, L, NB)
    rm = rot6d_ref.rotation_from_ortho6d(x[:, lo:hi].reshape(-1, 24, 6))
    tb = {k: (_f64(v) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v)) for k, v in tables.items()}
    verts, joints = body_ref.lbs(tb, rm, b64.repeat_interleave(hi - lo, 0))
    ref = {"log_prob": lp, "joints": joints.view(B, hi - lo, 24, 3), "vertices": verts.view(B, hi - lo, NV, 3)}
    _loss(ref, _f64(tj), _f64(tv), _f64(te), _f64(reg), _f64(w)).backward()
    errs = {"feats": _rel_l2(f.grad.cpu(), f64.grad), "betas": _rel_l2(b.grad.cpu(), b64.grad)}
    for name, prm in head.flow.named_parameters():
        assert prm.grad is not None, name
        errs[name] = _rel_l2(prm.grad.cpu(), sd64[name].grad)
    worst = max(errs, key=errs.get)
    print(f"B={B} K={K} hidden={H} {L}x{NB} ctx={Fc} slice={hyp_slice}: worst per-tensor rel-L2 {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= bound, (worst, errs[worst])


@pytest.mark.parametrize("hyp_slice", [None, (2, 5)])
def test_head_mesh_gradients_small_geometry(gpu_lib, hyp_slice):
    """Measured on an MI355X: worst per-tensor rel-L2 1.2e-6 (no slice), 1.9e-6 (slice (2, 5)) (bound 1e-4)."""
    _check_head(256, 128, 2, 1, 2, 6, hyp_slice, 1e-4)


def test_head_mesh_gradients_prohmr_geometry(gpu_lib):
    """hidden 1024, 4 layers x 2 blocks, context 2048, B = 4, K = 8.  Measured on an MI355X: worst per-tensor rel-L2 3.0e-6 (bound 1e-3)."""
    _check_head(2048, 1024, 4, 2, 4, 8, None, 1e-3)


def _grads(head, fn):
    head.zero_grad(set_to_none=True)
    fn()
    return [p.grad.clone() for p in head.flow.parameters()]


def test_invariants(gpu_lib):
    head, _, _ = _head(256, 128, 2, 1)
    head.train()
    feats, noise, betas = (torch.as_tensor(a).cuda() for a in _inputs(2, 6, 256))
    ref = head(feats, 6, betas=betas, noise=noise)
    out = head(feats, 6, betas=betas, noise=noise, verts_grad=True)
    for k in ("pose6d", "log_prob", "joints", "vertices"):                     # the forward is the default's, bit for bit
        assert torch.equal(out[k].detach(), ref[k].detach()), k
    tgt = torch.as_tensor(np.random.default_rng(4).normal(0, 0.3, (2, 6, 24, 3)).astype(np.float32)).cuda()
    joint_loss = lambda vg: (lambda: (lambda o: (o["log_prob"][:, 1:].mean() + (o["joints"] - tgt).abs().mean()).backward())(
        head(feats, 6, betas=betas, noise=noise, verts_grad=vg)))
    for a, b in zip(_grads(head, joint_loss(False)), _grads(head, joint_loss(True))):      # no vertex gradient: the joints-only route
        assert torch.equal(a, b)
    tv = torch.as_tensor(np.random.default_rng(5).normal(0, 0.3, (2, 6, head.body.NV, 3)).astype(np.float32)).cuda()
    vert_loss = lambda: (lambda o: ((o["vertices"] - tv).abs().mean() + o["log_prob"].mean()).backward())(
        head(feats, 6, betas=betas, noise=noise, verts_grad=True))
    g1, g2 = _grads(head, vert_loss), _grads(head, vert_loss)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)), "two backward passes differ"
    out = head(feats, 6, betas=betas, noise=noise, hyp_slice=(1, 4), verts_grad=True)
    out["vertices"].sum().backward()                                          # an expanded (stride-0) incoming gradient
    assert all(torch.isfinite(p.grad).all() for p in head.flow.parameters())
    with pytest.raises(NotImplementedError, match="vertex"):                 # the default still refuses
        head(feats, 6, betas=betas, noise=noise)["vertices"].sum().backward()
    with pytest.raises(ValueError):
        head(feats, 6, betas=betas, noise=noise, want_verts=False, verts_grad=True)
    with torch.no_grad():
        a = head(feats, 6, betas=betas, noise=noise)
        b = head(feats, 6, betas=betas, noise=noise, verts_grad=True)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_adam_training_on_vertices(gpu_lib):
    head, _, _ = _head(256, 128, 2, 1)
    head.train()
    feats, noise, betas = (torch.as_tensor(a).cuda() for a in _inputs(2, 6, 256))
    betas.requires_grad_()
    tv = torch.as_tensor(np.random.default_rng(6).normal(0, 0.3, (2, 6, head.body.NV, 3)).astype(np.float32)).cuda()
    opt = torch.optim.Adam(list(head.flow.parameters()) + [betas], lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        out = head(feats, 6, betas=betas, noise=noise, verts_grad=True)
        loss = (out["vertices"] - tv).abs().mean()
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in head.flow.parameters()) and torch.isfinite(betas.grad).all()
        opt.step()
        losses.append(float(loss.detach()))
    print("vertex L1", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and losses[-1] < losses[0] * 0.98, losses           # (measured on an MI355X: 0.286 -> 0.267)
