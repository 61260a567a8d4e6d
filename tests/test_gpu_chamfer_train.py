"""GPU: training with the hand-object Chamfer term, get_loss(chamfer_w=...) (the reference's switched-off branch hand/network.py:821-826,
defined for N hypotheses as every other term of _reverse_kld is averaged) through every layer - the two new kernels entries
mhe_mano_joints_chamfer_f32 / mhe_mano_joints_chamfer_bwd_f32 against the f64 restatement tests/chamfer_ref.py on the oracle-decoded
joints, the module, the train step, the autograd bridge, graph replay, the Glow branch, hypothesis sharding and run.py.
Tolerances: 1e-4 values and kernel gradients, 2e-4 parameter gradients through TrainStep (those of tests/test_gpu_xyz.py)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chamfer_ref
from conftest import ROOT, free_port, assert_close
from mhentropy_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # BASELINE.json north_star: 1e-4 relative, fp32
B, N = 3, 3          # R = 9 rows: no multiple of the 4 waves of a workgroup, and r % B matters
W = 10.0             # the reference's w_chamfer


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _tables():
    from test_gpu_train import _tables as t
    return t()


@functools.lru_cache(None)
def _tables64():
    from oracle import mano_ref
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0))
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in tb.items()}


@functools.lru_cache(None)
def _hand(seed):
    """th45 [R,45], det [B,16] (f32 values) and the oracle's f64 normalised joints xyz64 (N,B,21,3) of their R = N B hypotheses"""
    from oracle import network_ref
    rng = np.random.default_rng(seed)
    th45 = torch.as_tensor(rng.normal(0, 0.8, (N * B, 45)).astype(np.float32))
    det = torch.as_tensor(rng.normal(0, 1.0, (B, 16)).astype(np.float32))
    det[:, 3:13] *= 0.03
    det[:, 13:] *= 0.2
    with torch.no_grad():
        z = network_ref.combine_z(det.double().repeat(N, 1), th45.double())
        xyz = network_ref.decode(_tables64(), z)["xyz"].reshape(N, B, 21, 3).numpy()
    return th45, det, xyz


@functools.lru_cache(None)
def _case(seed, VO, counted, plant, determined=False):
    """_hand(seed) + object targets in the units of the data (tests/chamfer_ref.make_case's): scale 0.025..0.04 m, root and vertices in mm,
    the vertices within 90 mm of the root.  counted: per-image counts, the padded vertices planted ON joints of hypothesis 0 (+1e-3 mm) -
    closer than any valid vertex, so a kernel that reads past V_b fails.  plant: duplicated vertices (exact ties), one vertex exactly on the
    root (= joint 12, whose normalised coordinates are exactly 0: a zero distance in the kernel's arithmetic too) and one on the f64
    position of joint 5 of hypothesis 0.  determined: duplicated vertices only, and - as chamfer_ref.make_case does - the vertices of a
    close call are drawn again from the same seeded generator until every minimum of the f64 case has its runner-up 2 GAP away."""
    th45, det, xyz = _hand(seed)
    rng = np.random.default_rng(seed + 77)
    scale = rng.uniform(0.025, 0.04, B).astype(np.float32)
    root = (rng.uniform(-80.0, 80.0, (B, 3)) + np.array([0.0, 0.0, 500.0])).astype(np.float32)
    obj = (root[:, None, :] + rng.uniform(-90.0, 90.0, (B, VO, 3))).astype(np.float32)
    a0 = xyz[0] * (scale.astype(np.float64) * chamfer_ref.UNIT)[:, None, None] + root[:, None, :]          # (B,21,3) f64
    count = None
    if counted:
        count = np.asarray([max(VO - 7, 1), VO, max(VO // 2, 1)], np.int32)
    if plant and VO >= 16:
        obj[:, 5], obj[:, 9] = obj[:, 2], obj[:, 3]
        obj[:, 1] = root
        obj[:, 4] = a0[:, 5].astype(np.float32)
    if determined:
        for _ in range(400):
            obj[:, 5], obj[:, 9] = obj[:, 2], obj[:, 3]
            bad_p, bad_o = chamfer_ref._close_calls(xyz, scale, root, obj, count)
            if not bad_p.any() and not bad_o.any():
                break
            idx_p = chamfer_ref.chamfer64(xyz, scale, root, obj, count)["idx_p"]
            for b in range(B):          # the vertices with a close call of their own, and the nearest vertex of a joint with one
                redo = np.union1d(np.nonzero(bad_o[b])[0], idx_p[:, b][bad_p[:, b]])
                obj[b, redo] = (root[b] + rng.uniform(-90.0, 90.0, (redo.size, 3))).astype(np.float32)
        else:
            raise AssertionError("_case: no draw with every minimum determined")
    if count is not None:
        for b in range(B):
            pad = VO - int(count[b])
            obj[b, int(count[b]):] = (a0[b][np.arange(pad) % 21] + 1e-3).astype(np.float32)
    c = {"th45": th45, "det": det, "xyz64": xyz, "scale": scale, "root": root, "obj": obj, "count": count}
    c["ref"] = chamfer_ref.chamfer64(xyz, scale, root, obj, count)
    return c


def _cham(c):
    return (_dev(c["scale"]), _dev(c["root"]), _dev(c["obj"]), None if c["count"] is None else _dev(c["count"]))


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("VO", [1, 63, 64, 65, 130])
def test_forward_rows_match_chamfer64_on_the_oracle_joints(gpu_lib, VO, counted):
    """dist [R] of mhe_mano_joints_chamfer_f32 against the f64 Chamfer distance of the oracle-decoded joints, and against ops.chamfer on
    the kernel's own xyz; log_p and the other outputs are those of the call without the term, bit for bit"""
    from mhentropy_amd import ops
    c = _case(11, VO, counted, True)
    blob, _ = _tables()
    _, yn = synth.batch(3, B, with_image=False)
    cu, vis, p3 = _dev(yn["crop_uv"]), _dev(yn["vis"]), _dev(yn["pose3d"])
    th45, det, cham = _dev(c["th45"]), _dev(c["det"]), _cham(c)
    want = ("xyz", "terms", "log_p", "norms")
    for mods in (["uv"], ["xyz", "uv"]):
        o = ops.mano_joints(th45, det, blob, cu, vis, 0.03, 50.0, want=want, pose3d=p3, mods=mods, chamfer=cham)
        off = ops.mano_joints(th45, det, blob, cu, vis, 0.03, 50.0, want=want, pose3d=p3, mods=mods)
        print(f"VO={VO} counted={counted} {mods}: max rel err {np.abs(o['chamfer'].cpu().numpy() - c['ref']['dist'].reshape(-1)).max() / c['ref']['dist'].max():.3e}")
        assert_close(o["chamfer"].cpu(), c["ref"]["dist"].reshape(-1), RTOL, what=f"VO={VO} dist")
        for k in want:
            assert torch.equal(o[k], off[k]), k
        own, _ = ops.chamfer(o["xyz"].view(N, B, 21, 3), *cham)
        assert_close(o["chamfer"].cpu(), own.reshape(-1).cpu(), RTOL, what=f"VO={VO} dist vs ops.chamfer")
    again = ops.mano_joints(th45, det, blob, cu, vis, 0.03, 50.0, want=want, pose3d=p3, mods=mods, chamfer=cham)
    assert torch.equal(again["chamfer"], o["chamfer"])
    if VO >= 16:
        assert (c["ref"]["dist"] > 1.0).all()


@pytest.mark.parametrize("VO", [65, 130])
@pytest.mark.parametrize("mods", [["uv"], ["xyz", "uv"], ["xyz"]])
def test_reverse_matches_f64_autograd(gpu_lib, mods, VO):
    """d sum_b g_b (log_p_b - w chamfer_b) / d (th45, det) of mhe_mano_joints_chamfer_bwd_f32 against f64 autograd on the oracle decode,
    per-image counts with the padding planted on the joints, duplicated vertices kept (they do not change the gradient)"""
    from mhentropy_amd import ops
    from oracle import network_ref
    c = _case(11, VO, True, False, True)                         # (duplicated vertices 5 = 2, 9 = 3 inside every image's count)
    assert c["ref"]["gap"] >= chamfer_ref.GAP, c["ref"]["gap"]            # every minimum of the reference case is determined
    blob, _ = _tables()
    tb64 = _tables64()
    rng = np.random.default_rng(5)
    _, yn = synth.batch(3, B, with_image=False)
    y = {k: torch.as_tensor(v).double() for k, v in yn.items()}
    g = torch.as_tensor(rng.normal(0, 1, (B,)))
    th45_r, det_r = c["th45"].double().requires_grad_(True), c["det"].double().requires_grad_(True)
    z = network_ref.combine_z(det_r.repeat(N, 1), th45_r)
    lp = network_ref.forward_log_p(tb64, z, y, N)
    xyz = network_ref.decode(tb64, z)["xyz"]
    w3 = y["vis"][..., None].repeat(N, 1, 3).flatten(-2)
    lx = network_ref.laplace_log_prob(y["pose3d"].repeat(N, 1), xyz.flatten(-2), w3, b=0.03)
    lik = {"uv": lp["log_p_uv_giv_z"], "xyz": lx, "xyz_uv": lp["log_p_uv_giv_z"] + lx}["_".join(mods)]
    rows = lik + lp["log_p_th3"] + lp["log_p_th45"] + lp["log_p_bt"]
    s64, r64, o64 = (torch.as_tensor(np.asarray(c[k], np.float64)) for k in ("scale", "root", "obj"))
    pts = xyz.reshape(N, B, 21, 3)
    dist = []
    for b in range(B):
        d = chamfer_ref._pair_dist(pts, s64, r64, o64, b, int(c["count"][b]))
        dist.append(d.min(-1)[0].mean(-1) + d.min(-2)[0].mean(-1))
    dist = torch.stack(dist, 1)                                   # (N, B)
    assert_close(dist.detach(), c["ref"]["dist"], 1e-12, what="the autograd restatement is chamfer64")
    ((rows.reshape(N, B).mean(0) - W * dist.mean(0)) * g).sum().backward()
    cu = _dev(yn["crop_uv"]) if "uv" in mods else None
    p3 = _dev(yn["pose3d"]) if "xyz" in mods else None
    args = (_dev(c["th45"]), _dev(c["det"]), blob, cu, _dev(yn["vis"]), _dev(g.float()), N)
    g45, gdet = ops.mano_joints_bwd(*args, pose3d=p3, mods=mods, laplace_b_3d=0.03, chamfer=_cham(c), chamfer_w=W)
    off45, offdet = ops.mano_joints_bwd(*args, pose3d=p3, mods=mods, laplace_b_3d=0.03)
    print(f"{mods} VO={VO}: d/d th45 {(g45.cpu() - th45_r.grad).abs().max() / th45_r.grad.abs().max():.3e}  "
          f"d/d det {(gdet.cpu() - det_r.grad).abs().max() / det_r.grad.abs().max():.3e}  "
          f"(term's share of d/d th45: {(g45 - off45).abs().max() / g45.abs().max():.2f})")
    assert (g45 - off45).abs().max() > 1e-2 * g45.abs().max()          # the term is a visible part of the gradient under test
    assert_close(g45.cpu(), th45_r.grad, RTOL, what="d/d th45")
    assert_close(gdet.cpu(), det_r.grad, RTOL, what="d/d det")
    again = ops.mano_joints_bwd(*args, pose3d=p3, mods=mods, laplace_b_3d=0.03, chamfer=_cham(c), chamfer_w=W)
    assert torch.equal(again[0], g45) and torch.equal(again[1], gdet)
    zero = ops.mano_joints_bwd(*args, pose3d=p3, mods=mods, laplace_b_3d=0.03, chamfer=_cham(c), chamfer_w=0.0)
    assert_close(zero[0].cpu(), off45.cpu(), 1e-6, what="chamfer_w = 0 in the kernel")


def _small_model():
    from test_gpu_train import _model_and_state
    return _model_and_state("resnet18", 64, 2)


def _batch(seed=3, Bn=B, image_size=96, with_count=True, VO=130):
    xn, yn = synth.batch(seed, Bn, image_size=image_size)
    yn.update(synth.object_targets(seed, Bn, VO=VO, with_count=with_count))
    return torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}


def test_term_off_is_bit_equal_and_term_on_touches_log_p_only(gpu_lib):
    """chamfer_w = 0 through the new argument: torch.equal outputs and gradients, no 'chamfer' key.  chamfer_w = 10: q_log_p_z_giv_y,
    h_q_z_giv_i, th_norm and bt_norm torch.equal to the term-off run with the same noise, log_p lower by w chamfer (1e-6 relative),
    chamfer = mean over n of criteria.chamfer_dist of the sampled joints.  Module and train step."""
    from mhentropy_amd import criteria
    from mhentropy_amd.train import TrainStep
    model, _ = _small_model()
    x, y = _batch()
    z0 = torch.as_tensor(synth.noise(3, N * B)).cuda()
    ts = TrainStep(model)
    for mods in (["uv"], ["xyz", "uv"]):
        with torch.no_grad():
            base = model.get_loss(x, y, mods=mods, N=N, noise=z0)
            off = model.get_loss(x, y, mods=mods, N=N, noise=z0, chamfer_w=0.0)
            on = model.get_loss(x, y, mods=mods, N=N, noise=z0, chamfer_w=W)
        assert set(off) == set(base) and "chamfer" not in off and set(on) == set(base) | {"chamfer"}
        for k in base:
            assert torch.equal(base[k], off[k]), k
        for k in ("q_log_p_z_giv_y", "h_q_z_giv_i", "th_norm", "bt_norm"):
            assert torch.equal(base[k], on[k]), k
        assert on["chamfer"].shape == (B,) and (on["chamfer"] > 1.0).all()
        assert_close(on["log_p"].cpu(), (base["log_p"] - W * on["chamfer"]).cpu(), 1e-6, what="log_p")
        with torch.no_grad():
            xyz = model.sample(x, N=N, temp=1.0, noise=z0, mods=["xyz"])["xyz"].view(N, B, 21, 3)
            assert_close(on["chamfer"].cpu(), criteria.chamfer_dist(xyz, y).mean(0).cpu(), RTOL, what="chamfer vs chamfer_dist")
        tb = ts.forward_backward(x, y, noise=z0, N=N, mods=mods)
        Gb = ts.G.clone()
        to = ts.forward_backward(x, y, noise=z0, N=N, mods=mods, chamfer_w=0.0)
        assert "chamfer" not in to and torch.equal(ts.G, Gb)
        for k in tb:
            assert torch.equal(tb[k], to[k]), k
        tn = ts.forward_backward(x, y, noise=z0, N=N, mods=mods, chamfer_w=W)
        assert not torch.equal(ts.G, Gb)
        for k in ("q_log_p_z_giv_y", "h_q_z_giv_i", "th_norm", "bt_norm"):
            assert torch.equal(tb[k], tn[k]), k
        assert_close(tn["log_p"].cpu(), (tb["log_p"] - W * tn["chamfer"]).cpu(), 1e-6, what="train step log_p")
        assert_close(tn["chamfer"].cpu(), on["chamfer"].cpu(), 1e-6, what="train step chamfer")
    # the attribute is the default of the argument
    model.chamfer_w = W
    with torch.no_grad():
        assert torch.equal(model.get_loss(x, y, mods=mods, N=N, noise=z0)["log_p"], on["log_p"])
    model.chamfer_w = 0.0
    with pytest.raises(ValueError, match="object_verts"):
        model.get_loss(x, {k: v for k, v in y.items() if k != "object_verts"}, N=N, noise=z0, chamfer_w=W)


@pytest.mark.parametrize("mods", [["uv"], ["xyz", "uv"]])
def test_train_step_matches_f64_autograd_of_the_oracle(gpu_lib, mods):
    """TrainStep.forward_backward(None, y, trunk_out=..., chamfer_w=10), ResNet-18 heads, h = 64, 2 flow steps: loss values (1e-4) and the
    gradients of det_head.2.weight, a first and a last flow layer and g_feat (2e-4) against f64 autograd of network_ref.reverse_kld plus the
    Chamfer formula of chamfer_ref on the oracle's joints"""
    import torch.nn.functional as F
    from mhentropy_amd.train import TrainStep
    from oracle import network_ref
    model, sd = _small_model()
    steps = 2
    _, y = _batch(seed=8)
    rng = np.random.default_rng(8)
    trunk = rng.normal(0, 0.5, (B, 512)).astype(np.float32)
    z0 = synth.noise(8, N * B)
    names = ("det_head.2.weight", "q_z_giv_i.s.0.l.0.weight", f"q_z_giv_i.t.{2 * steps - 1}.l.2.weight")
    sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    for n in names:
        sd64[n] = sd64[n].clone().requires_grad_(True)
    y64 = {k: (v.cpu().double() if v.dtype == torch.float32 else v.cpu()) for k, v in y.items()}
    feat = F.linear(torch.as_tensor(trunk).double(), sd64["feat_extractor.l1.0.weight"], sd64["feat_extractor.l1.0.bias"]).requires_grad_(True)
    tb64 = _tables64()
    ref = network_ref.reverse_kld(sd64, tb64, feat, y64, torch.as_tensor(z0).double(), N)
    xyz = network_ref.decode(tb64, ref["_z"])["xyz"]
    if "xyz" in mods:
        w3 = y64["vis"][..., None].repeat(N, 1, 3).flatten(-2)
        lx = network_ref.laplace_log_prob(y64["pose3d"].repeat(N, 1), xyz.flatten(-2), w3, b=0.03)
        ref["q_log_p_z_giv_y"] = ref["q_log_p_z_giv_y"] + lx.reshape(N, B).mean(0)
        ref["log_p"] = ref["h_q_z_giv_i"] + ref["q_log_p_z_giv_y"]
    pts = xyz.reshape(N, B, 21, 3)
    obj64 = y64["object_verts"].reshape(B, -1, 3)
    dist = []
    for b in range(B):
        d = chamfer_ref._pair_dist(pts, y64["scale"], y64["original_pose3d"][:, chamfer_ref.ROOT], obj64, b, int(y64["object_count"][b]))
        dist.append(d.min(-1)[0].mean(-1) + d.min(-2)[0].mean(-1))
    cham = torch.stack(dist, 1).mean(0)
    log_p = ref["log_p"] - W * cham
    grads = torch.autograd.grad(-log_p.mean(), [feat] + [sd64[n] for n in names])
    ts = TrainStep(model)
    out = ts.forward_backward(None, y, noise=_dev(z0), N=N, trunk_out=_dev(trunk), mods=mods, chamfer_w=W)
    assert_close(out["chamfer"].cpu(), cham.detach(), RTOL, what="chamfer")
    assert_close(out["log_p"].cpu(), log_p.detach(), RTOL, what="log_p")
    assert_close(out["q_log_p_z_giv_y"].cpu(), ref["q_log_p_z_giv_y"].detach(), RTOL, what="q_log_p_z_giv_y")
    assert_close(out["h_q_z_giv_i"].cpu(), ref["h_q_z_giv_i"].detach(), RTOL, what="h_q_z_giv_i")
    params = dict(model.named_parameters())
    for n, gr in zip(names, grads[1:]):
        print(f"{mods} d loss / d {n}: {(ts.grad_of(params[n]).cpu() - gr).abs().max() / gr.abs().max():.3e}")
        assert_close(ts.grad_of(params[n]).cpu(), gr, 2e-4, what=f"d loss / d {n}")
    assert_close(ts.tape["g_feat"].cpu(), grads[0], 2e-4, what="d loss / d feat")
    # two reverse passes on the same inputs: the same bits
    G = ts.G.clone()
    ts.forward_backward(None, y, noise=_dev(z0), N=N, trunk_out=_dev(trunk), mods=mods, chamfer_w=W)
    assert torch.equal(ts.G, G)


def test_autograd_bridge_equals_the_fused_reverse_pass(gpu_lib):
    """get_loss(chamfer_w=10) -> total_loss.backward() with a TrainStep attached: .grad equals the explicit reverse pass"""
    from mhentropy_amd.train import TrainStep
    model, _ = _small_model()
    x, y = _batch(Bn=4)
    z0 = torch.as_tensor(synth.noise(3, 6 * 4)).cuda()
    ts = TrainStep(model).attach()
    for mods in (["uv"], ["xyz", "uv"]):
        model.zero_grad()
        out = model.get_loss(x, y, mods=mods, N=6, noise=z0, chamfer_w=W)
        assert out["log_p"].requires_grad and not out["chamfer"].requires_grad and out["chamfer"].shape == (4,)
        (-out["log_p"]).mean().backward()
        got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        assert len(got) == len(list(model.parameters()))
        lp = out["log_p"].detach().clone()
        off = model.get_loss(x, y, mods=mods, N=6, noise=z0)
        assert "chamfer" not in off and (off["log_p"].detach() - lp).abs().min() > 1e-3
        ref = ts.forward_backward(x, y, noise=z0, N=6, mods=mods, chamfer_w=W)
        assert_close(lp.cpu(), ref["log_p"].cpu(), 1e-6, what=f"{mods} log_p")
        for n, p in model.named_parameters():
            assert_close(got[n].cpu(), ts.grad_of(p).cpu(), 1e-5, what=f"{mods} d loss / d {n}")


def test_graphed_step_replays_bit_equal_to_eager(gpu_lib):
    """GraphedStep with the term on (ResNet-18, 128x128, B=8, N=4, lr 0): the replay equals the eager step bit for bit, also after a new
    object (vertices and counts) is copied into the captured static batch"""
    from mhentropy_amd.train import TrainStep, GraphedStep
    Bn, Nn, mods = 8, 4, ["xyz", "uv"]
    x, y = _batch(seed=21, Bn=Bn, image_size=128)
    _, y2 = _batch(seed=22, Bn=Bn, image_size=128)
    objs = [{k: t[k] for k in ("object_verts", "object_count")} for t in (y, y2)]
    z0 = torch.as_tensor(synth.noise(21, Nn * Bn)).cuda()
    ts = TrainStep(_small_model()[0], lr=0.0)
    eager = []
    for ob in objs:
        o = ts.step(x, dict(y, **ob), noise=z0, N=Nn, mods=mods, chamfer_w=W)
        eager.append((ts.G.clone(), o["log_p"].clone(), o["total"].clone(), o["chamfer"].clone()))
    assert not torch.equal(eager[0][3], eager[1][3])
    sy = {k: v.clone() for k, v in y.items()}
    gs = GraphedStep(ts, x.clone(), sy, noise=z0, N=Nn, mods=mods, chamfer_w=W)
    for i in (0, 1, 0):
        for k, v in objs[i].items():
            sy[k].copy_(v)
        o = gs.replay()
        torch.cuda.synchronize()
        G, lp, tot, ch = eager[i]
        assert torch.equal(o["chamfer"], ch) and torch.equal(o["log_p"], lp) and torch.equal(o["total"], tot), i
        assert torch.equal(ts.G, G), i


def test_glow_branch_chamfer_is_the_mean_of_its_rows(gpu_lib):
    """Glow branch (parity unpinned): the step runs with the term on and out['chamfer'] is the per-image mean over N of the row distances of
    the same hypotheses; the term-off keys do not move"""
    from mhentropy_amd import harness, ops
    from mhentropy_amd.network import MHEnt
    from mhentropy_amd.train import TrainStep
    special, common = harness.mhent_cfgs(backbone="resnet18", tables=synth.mano_tables(0))
    special["q_z_giv_i_model"] = "glow"
    model = MHEnt(special, **common)
    model.q_z_giv_i.load_state_dict({k: torch.as_tensor(v) for k, v in synth.glow_state(3).items()}, strict=False)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in synth.head_state(4, 512).items()}, strict=False)
    model = model.cuda().train()
    Nn = 5
    _, y = _batch(seed=5)
    f = _dev(np.random.default_rng(6).normal(0, 0.5, (B, 512)).astype(np.float32))
    noise = _dev(np.random.default_rng(7).normal(0, 1, (B, Nn, 45)).astype(np.float32))
    ts = TrainStep(model)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {}
    for key, w in (("off", 0.0), ("on", W)):
        ops.rng_state(dev, seed=12)                      # the same dropout masks -> the same hypotheses in both runs
        res[key] = ts.forward_backward(None, y, noise=noise, N=Nn, trunk_out=f, chamfer_w=w)
        res[key + "_G"] = ts.G.clone()
    th45, det = ts.tape["th45"], ts.tape["det"]
    for k in ("q_log_p_z_giv_y", "h_q_z_giv_i", "th_norm", "bt_norm"):
        assert torch.equal(res["off"][k], res["on"][k]), k
    o = ops.mano_joints(th45, det, model.mano_dec.table_blob(), y["crop_uv"], y["vis"], model.b_2d, model.th45_ref_alpha, want=("log_p",),
                        chamfer=model.chamfer_operands(y, W)[1])
    assert_close(res["on"]["chamfer"].cpu(), o["chamfer"].reshape(Nn, B).mean(0).cpu(), 1e-6, what="chamfer")
    assert_close(res["on"]["log_p"].cpu(), (res["off"]["log_p"] - W * res["on"]["chamfer"]).cpu(), 1e-6, what="log_p")
    assert torch.isfinite(res["on_G"]).all() and not torch.equal(res["on_G"], res["off_G"])


X2_WORKER = r'''
import os, sys, json
sys.path.insert(0, os.environ["MHE_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MHE_ROOT"], "tests"))
import torch
from mhentropy_amd import dist as mdist, synth
from mhentropy_amd.train import TrainStep
from test_gpu_train import _model_and_state
rank, _, world, dist = mdist.init("gloo")
torch.cuda.set_device(0)
B, N = 3, 4
xn, yn = synth.batch(40 + rank, B, image_size=64)
yn.update(synth.object_targets(40 + rank, B, VO=130, with_count=True))
x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
z0 = torch.as_tensor(synth.noise(40 + rank, N * B)).cuda()
res = {}
for name, sharded in (("images", False), ("hypotheses", True)):
    model, _ = _model_and_state("resnet18", 64, 2)
    ts = TrainStep(model, dist=dist, shard_hypotheses=sharded)
    out = ts.forward_backward(x, y, noise=z0, N=N, mods=["xyz", "uv"], chamfer_w=10.0)
    ts.finish_allreduce()
    res[name] = (out["log_p"].clone(), out["q_log_p_z_giv_y"].clone(), ts.G.clone() / world, ts.tape["g_feat"].clone(), out["chamfer"].clone())
off = TrainStep(_model_and_state("resnet18", 64, 2)[0], dist=dist, shard_hypotheses=True).forward(x, y, noise=z0, N=N, mods=["xyz", "uv"])
a, b = res["images"], res["hypotheses"]
rel = lambda u, v: float((u - v).abs().max() / (v.abs().max() + 1e-30))
with open(os.path.join(os.environ["MHE_OUT"], f"x2_rank{rank}.json"), "w") as fh:
    json.dump({"log_p": rel(b[0], a[0]), "q": rel(b[1], a[1]), "grad": rel(b[2], a[2]), "g_feat": rel(b[3], a[3]), "chamfer": rel(b[4], a[4]),
               "off_differs": rel(off["log_p"], b[0])}, fh)
dist.destroy_process_group()
'''


def test_hypothesis_sharded_step_equals_the_image_sharded_one(gpu_lib, tmp_path):
    """TrainStep(shard_hypotheses=True) with the term on, two gloo ranks on one GPU: the gathered object rows give the same loss terms and
    gradients as the image-sharded step (the bounds of tests/test_gpu_xyz.py)"""
    script = tmp_path / "x2_worker.py"
    script.write_text(X2_WORKER)
    env = dict(os.environ, MHE_ROOT=ROOT, MHE_OUT=str(tmp_path), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), str(script)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-3000:]
    for r in range(2):
        rec = json.load(open(tmp_path / f"x2_rank{r}.json"))
        assert rec["log_p"] < 1e-5 and rec["q"] < 1e-5 and rec["chamfer"] < 1e-5, rec
        assert rec["g_feat"] < 2e-3 and rec["grad"] < 2e-3, rec
        assert rec["off_differs"] > 1e-3, rec


def test_run_main_with_chamfer_w(gpu_lib):
    """python -m mhentropy_amd.run --chamfer-w 10: eager, replayed from HIP graphs, and fed by the GPU input pipeline"""
    from mhentropy_amd import run
    common = ["--backbone", "resnet18", "--batch", "4", "--hyps", "4", "--hidden", "64", "--flow-steps", "2", "--dtype", "f32", "--epochs", "1",
              "--chamfer-w", "10"]
    for extra in (["--iters", "3", "--image-size", "96"],
                  ["--iters", "3", "--image-size", "96", "--graph", "1"],
                  ["--iters", "2", "--input-pipeline"]):
        log = run.main(common + extra)
        assert len(log) == 1 and np.isfinite(log[0]["loss"]) and all(np.isfinite(v) for v in log[0]["it_losses"]), (extra, log)
