"""GPU tests of the body head's mesh-regressed keypoints and 2D keypoint likelihood: keypoints = keypoint_regressor x vertices accumulated inside
the skinning kernels (csrc/lbs_skin.hip: mhe_lbs_skin_kp_mfma_f32; csrc/body.hip: mhe_lbs_skin_kp_f32), their reverse (csrc/body_kp.hip:
mhe_lbs_keypoints_bwd_f32 into body.lbs_bwd), body.keypoint_log_prob (mhe_kp_log_prob_f32 / _bwd_f32) and BodyFlowHead(want_keypoints=True).
Reference-pinned: the hand-size keypoints against the joints the reference's own ManoLayer.xyz_from_vertice produced (tests/golden/mano.npz), the
likelihood against oracle.network_ref.laplace_log_prob (pinned by tests/test_oracle_golden.py).  Everything else against float64 on the CPU over
the oracle chain (oracle/glow_ref.py -> oracle/rot6d_ref.py -> oracle/body_ref.py -> regressor -> projection -> Laplace)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, assert_close
from mhentropy_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # tests/test_gpu_kernels.py: the bound test_loss_rows_match_reference_vectors puts on the same Laplace term of the hand path


def _f64(t):
    return torch.as_tensor(np.asarray(t, np.float64))


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _cu(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _mano_tables():
    """MANO's tables with the reference wrapper's 21-keypoint regressor (hand/ManoLayer.py:108-148 through oracle/mano_ref.py's constants): 16
    J_regressor rows in the wrapper's order, 5 one-hot rows at the tip vertices, then the RHD reorder"""
    from oracle import mano_ref
    t = synth.mano_tables(0)
    reg = np.zeros((21, 778), np.float32)
    for src, dst in mano_ref.WRAPPER_JOINT_MAP.items():
        reg[dst] = t["J_regressor"][src]
    for dst, vid in mano_ref.WRAPPER_TIP_VERTS.items():
        reg[dst, vid] = 1.0
    reg = reg[list(mano_ref.FREIHAND2RHD)]
    return {"v_template": t["v_template"], "shapedirs": t["shapedirs"], "posedirs": t["posedirs"], "J_regressor": t["J_regressor"],
            "weights": t["weights"], "parents": np.asarray(mano_ref.PARENTS), "keypoint_regressor": reg}


_TABLES = {}


def _tables(name):
    from mhentropy_amd import body
    if name not in _TABLES:
        _TABLES[name] = _mano_tables() if name == "mano" else body.synthetic_body_tables(int(name.split("kp_")[1]), keypoints=int(name.split("kp_")[0]))
    return _TABLES[name]


def _tb(tables, dtype):
    return {k: (torch.as_tensor(np.asarray(v, dtype)) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v)) for k, v in tables.items()}


def _oracle_kp(tables, rm, betas, dtype):
    from oracle import body_ref
    tb = _tb(tables, dtype)
    verts, joints = body_ref.lbs(tb, rm.to(tb["v_template"].dtype), betas.to(tb["v_template"].dtype))
    return torch.einsum("kv,rvc->rkc", tb["keypoint_regressor"], verts), verts, joints


def _laplace64(kp, cam, uv, vis, b=0.03):
    """the restated likelihood in the tensors' own dtype: batch_orth_proj (inv_norm=False) + _Laplace.log_prob, const b"""
    B, K = kp.shape[:2]
    cam = cam if cam.dim() == 3 else cam[:, None, :].expand(B, K, 3)
    proj = cam[..., None, :1] * kp[..., :2] + cam[..., None, 1:]
    d = (uv[:, None] - proj).abs()
    return ((vis[:, None, :, None] == 1.0) * (-(torch.relu(d - 1e-4) + 1e-4) / b - np.log(2 * b))).flatten(2).sum(2), proj


# ---- 1. reference-pinned: hand-size keypoints -----------------------------------------------------------------------------------------
def test_hand_size_keypoints_match_reference_joints(gpu_lib):
    """BodyLayer on MANO's tables + the wrapper's regressor == `joints` of tests/golden/mano.npz (the reference's xyz_from_vertice on its centred
    mm mesh): keypoints are linear in the vertices, so 1000 * (kp - rowsum * centre) is the same quantity"""
    from mhentropy_amd import body
    from oracle import mano_ref
    g = load_golden("mano")
    assert int(g["table_seed"]) == 0
    t = _tables("mano")
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0))
    theta, beta = torch.as_tensor(g["theta"]), torch.as_tensor(g["beta"])
    full_pose = torch.cat([theta[:, :3], tb["th_hands_mean"] + theta[:, 3:48].mm(tb["th_selected_comps"])], 1)
    rots = mano_ref.rodrigues(full_pose.reshape(-1, 3)).view(-1, 16, 3, 3)
    layer = body.BodyLayer(t).cuda()
    out = layer(beta.cuda(), rotmats=rots.cuda(), want_keypoints=True)
    centre = out["joints"][:, mano_ref.JOINT_REORDER[9]].unsqueeze(1)
    rowsum = torch.as_tensor(t["keypoint_regressor"].sum(1)).cuda().view(1, 21, 1)
    assert_close((1000 * (out["keypoints"] - rowsum * centre)).cpu(), g["joints"], 1e-4, what="wrapper joints (mm, centred on joint 9)")
    only = layer(beta.cuda(), rotmats=rots.cuda(), want_verts=False, want_keypoints=True)
    assert "vertices" not in only and torch.equal(only["keypoints"], out["keypoints"])


# ---- 2. reference-pinned: the likelihood ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_hyp", [True, False])
@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("NK", [1, 17, 21, 64])
def test_likelihood_matches_reference_laplace(gpu_lib, NK, K, per_hyp):
    from mhentropy_amd import body
    from oracle import network_ref
    B = 4
    rng = np.random.default_rng(1000 * NK + 10 * K + per_hyp)
    kp = rng.normal(0, 0.3, (B, K, NK, 3)).astype(np.float32)
    cam = np.concatenate([rng.uniform(0.5, 1.5, (B, K, 1)), rng.normal(0, 0.1, (B, K, 2))], -1).astype(np.float32)
    cam = cam if per_hyp else np.ascontiguousarray(cam[:, 0])
    uv = rng.normal(0, 0.4, (B, NK, 2)).astype(np.float32)
    vis = (rng.random((B, NK)) < 0.7).astype(np.float32)
    vis[0], vis[1] = 0.0, 1.0
    got = body.keypoint_log_prob(_cu(kp), _cu(cam), _cu(uv), _cu(vis))
    assert got.shape == (B, K)
    c = torch.as_tensor(cam if per_hyp else np.repeat(cam[:, None], K, 1))
    mu = (c[..., None, :1] * torch.as_tensor(kp)[..., :2] + c[..., None, 1:]).reshape(B * K, NK, 2)
    x = torch.as_tensor(uv).repeat_interleave(K, 0)
    w = torch.as_tensor(vis).repeat_interleave(K, 0)[..., None].expand(B * K, NK, 2)
    ref = network_ref.laplace_log_prob(x, mu, w).view(B, K)
    assert network_ref.LAPLACE_B == 0.03
    assert_close(got.cpu(), ref, RTOL, 1e-6, what="log p(uv | keypoints) (network.py:233-258)")
    assert bool((got[0] == 0).all()), "an image without visible keypoints has log-likelihood exactly 0"


# ---- 3. forward accuracy against the f64 oracle, both kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mfma", ["1", "0"])
@pytest.mark.parametrize("NK", [17, 64])
@pytest.mark.parametrize("R", [1, 5, 19, 70])
def test_keypoints_at_smpl_size_match_oracle(gpu_lib, monkeypatch, R, NK, mfma):
    from mhentropy_amd import body, ops, _lib
    from oracle import rot6d_ref
    monkeypatch.setenv("MHE_LBS_MFMA", mfma)
    t = _tables(f"{NK}kp_1")
    layer = body.BodyLayer(t).cuda()
    rng = np.random.default_rng(R)
    p6 = torch.as_tensor(rng.normal(0, 1, (R, 144)).astype(np.float32))
    betas = torch.as_tensor(rng.normal(0, 1, (R, 10)).astype(np.float32))
    rm = rot6d_ref.rotation_from_ortho6d(p6.view(R, 24, 6))
    both = layer(betas.cuda(), pose6d=p6.cuda(), want_keypoints=True)
    only = layer(betas.cuda(), pose6d=p6.cuda(), want_verts=False, want_keypoints=True)
    plain = layer(betas.cuda(), pose6d=p6.cuda())
    assert both["keypoints"].shape == (R, NK, 3) and "vertices" not in only
    assert torch.equal(only["keypoints"], both["keypoints"]) and torch.equal(both["vertices"], plain["vertices"])
    k64, _, _ = _oracle_kp(t, rm.double(), betas.double(), np.float64)
    k32, _, _ = _oracle_kp(t, rm, betas, np.float32)
    ext = float(k64.abs().max())
    e_gpu, e_f32 = float((only["keypoints"].cpu().double() - k64).abs().max()) / ext, float((k32.double() - k64).abs().max()) / ext
    print(f"SMPL-size keypoints R={R} NK={NK} MHE_LBS_MFMA={mfma}: max error / extent  HIP {e_gpu:.2e}   f32 oracle {e_f32:.2e}")
    assert e_gpu <= max(3 * e_f32, 2e-6), (e_gpu, e_f32)
    # rows past R of an oversized output are not stored
    L, P = _lib.lib(), ops._ptr
    big = torch.full((R + 40, NK, 3), -7.0, device="cuda")
    ws = torch.empty(L.mhe_lbs_workspace_floats(R, 24, 10), device="cuda")
    rmd, bd = both["rotmats"].contiguous(), betas.cuda().contiguous()
    ops.check(L.mhe_lbs_pose_f32(P(rmd), P(bd), P(layer._jt), P(layer._jsd), P(layer.parents), P(ws), None, R, 24, 10, ops._stream()), "pose")
    dev = torch.device("cuda", 0)
    if mfma == "1":
        assert L.mhe_lbs_skin_kp_supported(R, 24, 10, 6890, layer.VP, NK, 0)
        ops.check(L.mhe_lbs_skin_kp_mfma_f32(P(ws), P(layer._split_tables(dev)), P(layer._kp_split(dev)), None, P(big), R, 24, 10, 6890, layer.VP, NK,
                                             1.0, ops._stream()), "skin")
    else:
        ops.check(L.mhe_lbs_skin_kp_f32(P(ws), P(layer._vt), P(layer._vsd), P(layer._vpd), P(layer._vw), P(layer.keypoint_regressor), None, P(big), R, 24,
                                        10, 6890, layer.VP, NK, 1.0, ops._stream()), "skin")
    assert torch.equal(big[:R], only["keypoints"]) and bool((big[R:] == -7.0).all())
    # scale != 1: the keypoints are regressed from the scaled vertices
    sc = layer(betas.cuda(), pose6d=p6.cuda(), scale=0.7, want_keypoints=True)
    sc_only = layer(betas.cuda(), pose6d=p6.cuda(), scale=0.7, want_verts=False, want_keypoints=True)
    assert torch.equal(sc["keypoints"], sc_only["keypoints"]) and torch.equal(sc["vertices"], layer(betas.cuda(), pose6d=p6.cuda(), scale=0.7)["vertices"])
    e_sc = float((sc["keypoints"].cpu().double() - 0.7 * k64).abs().max()) / (0.7 * ext)
    print(f"  scale=0.7: max error / extent  HIP {e_sc:.2e}")
    assert e_sc <= max(3 * e_f32, 2e-6), (e_sc, e_f32)


# ---- 4. no vertex tensor --------------------------------------------------------------------------------------------------------------------
def test_keypoints_without_a_vertex_tensor(gpu_lib):
    from mhentropy_amd import body
    R, NK = 4096, 17
    layer = body.BodyLayer(_tables("17kp_1")).cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    p6 = torch.randn(R, 144, device="cuda", generator=gen)
    betas = torch.randn(R, 10, device="cuda", generator=gen)
    rm = body.rot6d_to_rotmat(p6.view(R, 24, 6))
    layer(betas[:8].contiguous(), rotmats=rm[:8].contiguous(), want_verts=False, want_keypoints=True)          # the per-model pieces are made here
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    only = layer(betas, rotmats=rm, want_verts=False, want_keypoints=True)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"R={R}: peak allocation growth of the keypoints-only call {growth / 1e6:.1f} MB (a vertex tensor is {R * 6890 * 12 / 1e6:.0f} MB)")
    assert growth < R * 6890 * 3 * 4
    again = layer(betas, rotmats=rm, want_verts=False, want_keypoints=True)
    both = layer(betas, rotmats=rm, want_keypoints=True)
    plain = layer(betas, rotmats=rm)
    assert torch.equal(only["keypoints"], again["keypoints"]), "two calls differ"
    assert torch.equal(only["keypoints"], both["keypoints"]) and torch.equal(both["vertices"], plain["vertices"])
    assert torch.isfinite(only["keypoints"]).all()


def test_c4_per_gpu_size_keypoints(gpu_lib):
    """R = 16,384 hypotheses (config C4 per GPU), keypoints only: finite, and a row slice decodes to exactly the rows of the full decode"""
    from mhentropy_amd import body
    R = 16384
    layer = body.BodyLayer(_tables("17kp_1")).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    p6, betas = torch.randn(R, 144, device="cuda", generator=gen), torch.randn(R, 10, device="cuda", generator=gen)
    full = layer(betas, pose6d=p6, want_verts=False, want_keypoints=True)["keypoints"]
    part = layer(betas[4100:6150].contiguous(), pose6d=p6[4100:6150].contiguous(), want_verts=False, want_keypoints=True)["keypoints"]
    assert full.shape == (R, 17, 3) and torch.isfinite(full).all() and torch.equal(part, full[4100:6150])


# ---- 5. gradients ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_others", [False, True])
@pytest.mark.parametrize("model", ["mano", "17kp_4"])
def test_lbs_bwd_keypoints_vs_f64(gpu_lib, model, with_others):
    """body.lbs_bwd(g_keypoints=...) against f64 autograd of body_ref.lbs + regressor (scale 0.7), alone and added to simultaneous vertex and joint
    gradients; test_lbs_bwd_vs_f64's bound.  Measured on an MI355X: see the printed figures."""
    from mhentropy_amd import body
    from oracle import body_ref, rot6d_ref
    tables = _tables(model)
    layer = body.BodyLayer(tables).cuda()
    J, nb, NV, NK, scale = layer.J, layer.nb, layer.NV, layer.NK, 0.7
    tb = _tb(tables, np.float64)
    worst = 0.0
    for R in (1, 33, 70):
        rng = np.random.default_rng(R + 100 * with_others)
        rm = rot6d_ref.rotation_from_ortho6d(torch.as_tensor(rng.normal(0, 1, (R, J, 6)))).float()
        bt = torch.as_tensor(rng.normal(0, 1, (R, nb)).astype(np.float32))
        gk = torch.as_tensor(rng.normal(0, 1, (R, NK, 3)).astype(np.float32))
        gv = torch.as_tensor(rng.normal(0, 0.1, (R, NV, 3)).astype(np.float32)) if with_others else None
        gj = torch.as_tensor(rng.normal(0, 1, (R, J, 3)).astype(np.float32)) if with_others else None
        dv = lambda a: None if a is None else a.cuda()
        run = lambda: body.lbs_bwd(layer, rm.cuda().contiguous(), bt.cuda().contiguous(), dv(gv), dv(gj), scale=scale, g_keypoints=gk.cuda())
        (g_rot, g_bt), (g_rot2, g_bt2) = run(), run()
        assert torch.equal(g_rot, g_rot2) and torch.equal(g_bt, g_bt2), "two calls differ"
        rm64, bt64 = rm.double().requires_grad_(), bt.double().requires_grad_()
        verts, joints = body_ref.lbs(tb, rm64, bt64)
        kp = torch.einsum("kv,rvc->rkc", tb["keypoint_regressor"], verts * scale)
        loss = (kp * gk.double()).sum()
        if with_others:
            loss = loss + (verts * scale * gv.double()).sum() + (joints * gj.double()).sum()
        loss.backward()
        for name, got, ref in (("g_rotmats", g_rot, rm64.grad), ("g_betas", g_bt, bt64.grad)):
            err = _rel_l2(got.cpu(), ref)
            worst = max(worst, err)
            assert err <= 1e-4, (model, R, name, err)
    print(f"{model} with vertex + joint gradients={with_others}: worst rel-L2 {worst:.2e}")


def test_lbs_bwd_walks_rows_in_chunks(gpu_lib, monkeypatch):
    """the keypoints-only route bounds its vertex-gradient buffer by walking KP_BWD_ROWS rows at a time: the same bits as one pass"""
    from mhentropy_amd import body
    layer = body.BodyLayer(_tables("mano")).cuda()
    R = 70
    gen = torch.Generator(device="cuda").manual_seed(2)
    rm = body.rot6d_to_rotmat(torch.randn(R, 16, 6, device="cuda", generator=gen))
    bt, gk = torch.randn(R, 10, device="cuda", generator=gen), torch.randn(R, 21, 3, device="cuda", generator=gen)
    one = body.lbs_bwd(layer, rm, bt, None, g_keypoints=gk)
    monkeypatch.setattr(body, "KP_BWD_ROWS", 32)
    many = body.lbs_bwd(layer, rm, bt, None, g_keypoints=gk)
    assert torch.equal(one[0], many[0]) and torch.equal(one[1], many[1])


@pytest.mark.parametrize("per_hyp", [True, False])
@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("NK", [17, 64])
def test_likelihood_gradients_vs_f64(gpu_lib, NK, K, per_hyp):
    """g_keypoints and g_cam of mhe_kp_log_prob_bwd_f32 against f64 autograd, 1e-5 of each tensor's max, no element left out; uv is drawn at
    least 1.1e-3 from every projection so that nothing lies within 1e-3 of the 1e-4 kink (asserted on the inputs)"""
    from mhentropy_amd import body
    B = 4
    rng = np.random.default_rng(77 * NK + 7 * K + per_hyp)
    kp = rng.normal(0, 0.3, (B, K, NK, 3)).astype(np.float32)
    cam = np.concatenate([rng.uniform(0.5, 1.5, (B, K, 1)), rng.normal(0, 0.1, (B, K, 2))], -1).astype(np.float32)
    cam = cam if per_hyp else np.ascontiguousarray(cam[:, 0])
    vis = (rng.random((B, NK)) < 0.7).astype(np.float32)
    vis[0], vis[1] = 0.0, 1.0
    uv = rng.normal(0, 0.4, (B, NK, 2)).astype(np.float32)
    kp64, cam64 = _f64(kp).requires_grad_(), _f64(cam).requires_grad_()
    for _ in range(50):                                             # redraw the few targets that fall next to a kink
        _, proj = _laplace64(kp64.detach(), cam64.detach(), _f64(uv), _f64(vis))
        near = (((_f64(uv)[:, None] - proj).abs() - 1e-4).abs() <= 1.1e-3).any(1).numpy()
        if not near.any():
            break
        uv[near] = rng.normal(0, 0.4, int(near.sum())).astype(np.float32)
    ref, proj = _laplace64(kp64, cam64, _f64(uv), _f64(vis))
    assert float(((_f64(uv)[:, None] - proj.detach()).abs() - 1e-4).abs().min()) > 1e-3, "a target within 1e-3 of the kink"
    g = rng.normal(0, 1, (B, K)).astype(np.float32)
    (ref * _f64(g)).sum().backward()
    kpd, camd = _cu(kp).requires_grad_(), _cu(cam).requires_grad_()
    got = body.keypoint_log_prob(kpd, camd, _cu(uv), _cu(vis))
    (got * _cu(g)).sum().backward()
    assert_close(got.detach().cpu(), ref.detach(), 1e-5, what="value")
    for name, a, b in (("g_keypoints", kpd.grad, kp64.grad), ("g_cam", camd.grad, cam64.grad)):
        err = float((a.cpu().double() - b).abs().max() / b.abs().max())
        print(f"NK={NK} K={K} per-hypothesis cam={per_hyp}: {name} max error / max {err:.2e}")
        assert err <= 1e-5, (name, err)
    assert bool((kpd.grad[..., 2] == 0).all()) and bool((kpd.grad[0] == 0).all()) and bool((camd.grad[0] == 0).all())


def _head(Fc=256, H=128, L=2, NB=1, seed=5):
    from mhentropy_amd import body
    tables = _tables("17kp_2")
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
    cam = np.concatenate([rng.uniform(0.5, 1.5, (B, 1)), rng.normal(0, 0.1, (B, 2))], -1).astype(np.float32)
    vis = (rng.random((B, 17)) < 0.7).astype(np.float32)
    return feats, noise, betas, cam, vis


def _head_oracle(sd, tables, feats, noise, betas, lo, hi, L, NB):
    from oracle import glow_ref, rot6d_ref, body_ref
    B = feats.shape[0]
    x, lp, _ = glow_ref.sample_and_log_prob(sd, noise, feats, L, NB)
    rm = rot6d_ref.rotation_from_ortho6d(x[:, lo:hi].reshape(-1, 24, 6))
    tb = _tb(tables, np.float64)
    verts, _ = body_ref.lbs(tb, rm, betas.repeat_interleave(hi - lo, 0))
    return lp, torch.einsum("kv,rvc->rkc", tb["keypoint_regressor"], verts).view(B, hi - lo, -1, 3)


@pytest.mark.parametrize("hyp_slice", [None, (2, 5)])
def test_head_keypoint_loss_gradients_small_geometry(gpu_lib, hyp_slice):
    """loss = log_prob[:, 1:].mean() - keypoint_log_prob(keypoints, cam, uv, vis).mean() in one backward call, without verts_grad and without a
    vertex tensor, against f64 autograd of the restated path; test_head_mesh_gradients_small_geometry's bound"""
    from mhentropy_amd import body
    Fc, H, L, NB, B, K = 256, 128, 2, 1, 2, 6
    head, sd, tables = _head(Fc, H, L, NB)
    feats, noise, betas, cam, vis = _inputs(B, K, Fc)
    lo, hi = hyp_slice or (0, K)
    sd64 = {k: _f64(v).requires_grad_() for k, v in sd.items()}
    f64, b64, c64 = _f64(feats).requires_grad_(), _f64(betas).requires_grad_(), _f64(cam).requires_grad_()
    lp, kp64 = _head_oracle(sd64, tables, f64, _f64(noise), b64, lo, hi, L, NB)
    rng = np.random.default_rng(8)                      # targets 0.05 .. 0.3 from the nearest hypothesis' projection: none next to a kink
    proj0 = (c64[:, None, None, :1] * kp64[..., :2] + c64[:, None, None, 1:]).detach()
    draw = lambda: (proj0[:, 0] + _f64(rng.uniform(0.05, 0.3, (B, 17, 2)) * rng.choice([-1.0, 1.0], (B, 17, 2)))).float().double()
    uv = draw()
    for _ in range(50):                                 # (another hypothesis' projection may land next to a target: redraw those)
        near = (((uv[:, None] - proj0).abs() - 1e-4).abs() <= 1.1e-3).any(1)
        if not bool(near.any()):
            break
        uv = torch.where(near, draw(), uv)
    ll, proj = _laplace64(kp64, c64, uv, _f64(vis))
    assert float(((uv[:, None] - proj.detach()).abs() - 1e-4).abs().min()) > 1e-3, "a target within 1e-3 of the kink"
    (lp[:, 1:].mean() - ll.mean()).backward()
    f, b, c = _cu(feats).requires_grad_(), _cu(betas).requires_grad_(), _cu(cam).requires_grad_()
    out = head(f, K, betas=b, noise=_cu(noise), hyp_slice=hyp_slice, want_verts=False, want_keypoints=True)
    assert out["keypoints"].shape == (B, hi - lo, 17, 3) and "vertices" not in out
    (out["log_prob"][:, 1:].mean() - body.keypoint_log_prob(out["keypoints"], c, uv.float().contiguous().cuda(), _cu(vis)).mean()).backward()
    errs = {"feats": _rel_l2(f.grad.cpu(), f64.grad), "betas": _rel_l2(b.grad.cpu(), b64.grad), "cam": _rel_l2(c.grad.cpu(), c64.grad)}
    for name, prm in head.flow.named_parameters():
        assert prm.grad is not None, name
        errs[name] = _rel_l2(prm.grad.cpu(), sd64[name].grad)
    worst = max(errs, key=errs.get)
    print(f"slice={hyp_slice}: worst per-tensor rel-L2 {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= 1e-4, (worst, errs[worst])


# ---- 6. invariants ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mfma", ["1", "0"])
def test_layer_invariants(gpu_lib, monkeypatch, mfma):
    from mhentropy_amd import body
    monkeypatch.setenv("MHE_LBS_MFMA", mfma)
    t = _tables("17kp_1")
    layer = body.BodyLayer(t).cuda()
    eye6 = torch.tensor([1., 0, 0, 0, 1, 0], device="cuda").repeat(24)
    rest = layer(torch.zeros(3, 10, device="cuda"), pose6d=eye6.repeat(3, 1).contiguous(), want_keypoints=True)
    tpl = torch.as_tensor(t["keypoint_regressor"].astype(np.float64) @ t["v_template"].astype(np.float64))
    assert_close(rest["keypoints"].cpu(), tpl[None].expand(3, 17, 3), 1e-5, what="identity pose, zero betas = regressor x template")
    # A one-hot row is a picked vertex.  The pieces of the vertex (three bf16 that sum to the f32 exactly) meet a regressor piece of exactly 1.0,
    # every product and every partial sum is representable, so the value is the stored vertex; the order in which the matrix core adds the sixteen
    # k terms of one instruction is not specified, hence the stated bound is 1 ulp (the scalar kernel's fmaf(1, v, 0) chain is exact).
    rng = np.random.default_rng(6)
    out = layer(_cu(rng.normal(0, 1, (19, 10)).astype(np.float32)), pose6d=_cu(rng.normal(0, 1, (19, 144)).astype(np.float32)), want_keypoints=True)
    reg = t["keypoint_regressor"]
    rows = [k for k in range(17) if (reg[k] == 1.0).sum() == 1 and (reg[k] != 0).sum() == 1]
    assert len(rows) >= 3
    for k in rows:
        a, b = out["keypoints"][:, k].cpu().numpy(), out["vertices"][:, int(reg[k].argmax())].cpu().numpy()
        assert (np.abs(a - b) <= np.spacing(np.abs(b))).all(), k
        print(f"MHE_LBS_MFMA={mfma} one-hot row {k}: bit-equal to its vertex = {bool((a == b).all())}")


def test_head_invariants(gpu_lib):
    from mhentropy_amd import body
    head, _, _ = _head()
    feats, noise, betas, cam, vis = (_cu(a) for a in _inputs(2, 6, 256))
    with torch.no_grad():
        full = head(feats, 6, betas=betas, noise=noise, want_keypoints=True)
        part = head(feats, 6, betas=betas, noise=noise, hyp_slice=(2, 5), want_verts=False, want_keypoints=True)
        plain = head(feats, 6, betas=betas, noise=noise)
    assert torch.equal(part["keypoints"], full["keypoints"][:, 2:5]) and torch.equal(part["joints"], full["joints"][:, 2:5])
    assert all(torch.equal(plain[k], full[k]) for k in plain)
    head.train()                                        # grad-mode forward equals the eval forward bit for bit
    out = head(feats, 6, betas=betas, noise=noise, want_keypoints=True)
    assert out["keypoints"].requires_grad
    for k in ("pose6d", "log_prob", "joints", "vertices", "keypoints"):
        assert torch.equal(out[k].detach(), full[k]), k
    out = head(feats, 6, betas=betas, noise=noise, hyp_slice=(2, 5), want_verts=False, want_keypoints=True)
    assert torch.equal(out["keypoints"].detach(), part["keypoints"])
    # vis = 0 everywhere: value 0 and all-zero gradients
    cam.requires_grad_()
    uv = torch.zeros(2, 17, 2, device="cuda")
    head.zero_grad(set_to_none=True)
    ll = body.keypoint_log_prob(out["keypoints"], cam, uv, torch.zeros(2, 17, device="cuda"))
    assert bool((ll == 0).all())
    ll.sum().backward()
    assert bool((cam.grad == 0).all()) and all(p.grad is None or bool((p.grad == 0).all()) for p in head.flow.parameters())
    # the existing refusal stays: a vertex gradient without verts_grad=True, with or without keypoints next to it
    out = head(feats, 6, betas=betas, noise=noise, want_keypoints=True)
    with pytest.raises(NotImplementedError, match="vertex"):
        (out["vertices"].sum() + out["keypoints"].sum()).backward()


def test_regressor_written_in_place_refreshes_the_pieces(gpu_lib):
    """load_state_dict copies a new regressor into the persistent buffer without moving it: the matrix-core path must not keep its old bf16 pieces"""
    from mhentropy_amd import body
    t = _tables("17kp_1")
    layer = body.BodyLayer(t).cuda()
    gen = torch.Generator(device="cuda").manual_seed(9)
    p6, betas = torch.randn(5, 144, device="cuda", generator=gen), torch.randn(5, 10, device="cuda", generator=gen)
    first = layer(betas, pose6d=p6, want_verts=False, want_keypoints=True)["keypoints"]
    sd = layer.state_dict()
    sd["keypoint_regressor"] = sd["keypoint_regressor"].flip(0).contiguous()
    layer.load_state_dict(sd)
    second = layer(betas, pose6d=p6, want_verts=False, want_keypoints=True)["keypoints"]
    assert torch.equal(second, first.flip(1)) and not torch.equal(second, first)


# ---- 7. it trains -------------------------------------------------------------------------------------------------------------------------------------
def test_adam_training_on_2d_keypoints(gpu_lib):
    """30 Adam steps on the paper's loss (entropy term + expected 2D keypoint log-likelihood), fixed batch and noise, 2D targets only"""
    from mhentropy_amd import body
    head, _, _ = _head()
    head.train()
    feats, noise, betas, cam, vis = (_cu(a) for a in _inputs(2, 6, 256))
    uv = _cu(np.random.default_rng(4).normal(0, 0.3, (2, 17, 2)).astype(np.float32))
    opt = torch.optim.Adam(head.flow.parameters(), lr=1e-3)
    losses, terms = [], []
    for _ in range(30):
        opt.zero_grad()
        out = head(feats, 6, betas=betas, noise=noise, want_verts=False, want_keypoints=True)
        ll = body.keypoint_log_prob(out["keypoints"], cam, uv, vis).mean()
        loss = out["log_prob"].mean() - ll
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in head.flow.parameters())
        opt.step()
        losses.append(float(loss.detach())); terms.append(float(ll.detach()))
    print("loss", losses[0], "->", losses[-1], "| keypoint log-likelihood", terms[0], "->", terms[-1])
    assert np.isfinite(losses).all() and all(torch.isfinite(p).all() for p in head.flow.parameters())
    assert losses[-1] < losses[0] and terms[-1] > terms[0], (losses, terms)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_lib):
    from mhentropy_amd import body, _lib, ops
    L, P = _lib.lib(), ops._ptr
    d = lambda *s: torch.zeros(*s, device="cuda")
    kp, cam, uv, vis = d(2, 3, 5, 3), d(2, 3, 3), d(2, 5, 2), torch.ones(2, 5, device="cuda")
    assert body.keypoint_log_prob(kp, cam, uv, vis).shape == (2, 3)
    for bad in ((kp.double(), cam, uv, vis), (kp, cam.half(), uv, vis), (kp, cam, uv.double(), vis), (kp, cam, uv, vis.bool()),
                (kp, cam, uv.cpu(), vis), (kp, cam, d(2, 4, 2), vis), (kp, cam, d(3, 5, 2), vis), (kp, cam, uv, d(2, 6)), (kp, d(2, 4, 3), uv, vis),
                (d(2, 3, 65, 3), cam, d(2, 65, 2), d(2, 65))):
        with pytest.raises((ValueError, _lib.MheError), match="keypoint_log_prob"):
            body.keypoint_log_prob(*bad)
    plain = body.BodyFlowHead(body.synthetic_body_tables(2), context_features=256, hidden=128, num_layers=2, num_blocks=1).cuda().eval()
    with pytest.raises(ValueError, match="keypoint_regressor"):
        plain(d(2, 256), 3, want_keypoints=True)
    with pytest.raises(ValueError, match="keypoint_regressor"):
        plain.body(d(2, 10), pose6d=d(2, 144), want_keypoints=True)
    layer = body.BodyLayer(_tables("mano")).cuda()
    with pytest.raises(_lib.MheError, match="lbs_bwd.g_keypoints"):
        body.lbs_bwd(layer, d(2, 16, 3, 3), d(2, 10), None, g_keypoints=d(2, 20, 3))
    with pytest.raises(ValueError, match="lbs_bwd"):
        body.lbs_bwd(layer, d(2, 16, 3, 3), d(2, 10), None)
    # the C entries with device buffers: MHE_ERR_ARG and the entry's name, never a launch
    ws, kpo = d(L.mhe_lbs_workspace_floats(2, 16, 10)), d(2, 21, 3)
    dev = torch.device("cuda", 0)
    sp, ks = layer._split_tables(dev), layer._kp_split(dev)
    call = lambda R, NK, ks_: L.mhe_lbs_skin_kp_mfma_f32(P(ws), P(sp), P(ks_), None, P(kpo), R, 16, 10, 778, layer.VP, NK, 1.0, ops._stream())
    for R, NK, ks_ in ((2, 0, ks), (2, 65, ks), (0, 21, ks), (2, 21, None)):
        assert call(R, NK, ks_) == 1 and b"mhe_lbs_skin_kp_mfma_f32" in L.mhe_last_error()
    call = lambda R, NK, reg: L.mhe_lbs_skin_kp_f32(P(ws), P(layer._vt), P(layer._vsd), P(layer._vpd), P(layer._vw), P(reg), None, P(kpo), R, 16, 10, 778,
                                                    layer.VP, NK, 1.0, ops._stream())
    for R, NK, reg in ((2, 0, layer.keypoint_regressor), (2, 65, layer.keypoint_regressor), (0, 21, layer.keypoint_regressor), (2, 21, None)):
        assert call(R, NK, reg) == 1 and b"mhe_lbs_skin_kp_f32" in L.mhe_last_error()
    assert L.mhe_lbs_keypoints_bwd_f32(P(layer.keypoint_regressor), P(kpo), P(d(2, 778, 3)), 0, 21, 778, 0, ops._stream()) == 1
    assert b"mhe_lbs_keypoints_bwd_f32" in L.mhe_last_error()
    torch.cuda.synchronize()
