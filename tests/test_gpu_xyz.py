"""GPU: the 3D-supervised loss get_loss(mods=['xyz', 'uv']) / (mods=['xyz']) (hand/CrossModalHand.py:354, hand/network.py:393,398-400,
620-662) through every layer - the MANO loss-pass kernels and their reverse, the module boundary against the reference-generated
fixtures tests/golden/mhent_xyz_*.npz, the train step, the autograd bridge, graph replay, the Glow branch, hypothesis sharding and run.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, free_port, load_golden, assert_close
from mhentropy_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # BASELINE.json north_star: 1e-4 relative, fp32
MODS = {"xyz_uv": ["xyz", "uv"], "xyz": ["xyz"]}
TARGETS = ("far", "near")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _y(g, tname):
    y = {k[2:]: _dev(v) for k, v in g.items() if k.startswith("y_")}
    y["pose3d"] = _dev(g[f"{tname}_pose3d"])
    return y


def _model_from_golden(g):
    from mhentropy_amd import harness
    seed, h, steps = int(g["seed"]), int(g["h"]), int(g["steps"])
    model = harness.build_mhent(backbone="resnet50", h_dims=(h, h), num_steps=steps, tables=synth.mano_tables(0))
    sd = {"q_z_giv_i." + k: torch.as_tensor(v) for k, v in synth.flow_state(seed, 45, 512, (h, h), steps).items()}
    sd.update({k: torch.as_tensor(v) for k, v in synth.head_state(seed, 2048, 512, 16).items()})
    assert not model.load_state_dict(sd, strict=False)[1]
    return model.cuda()


@pytest.mark.parametrize("tag", ["small", "shipped"])
@pytest.mark.parametrize("fused", [True, False])
def test_get_loss_xyz_matches_reference_vectors(gpu_lib, tag, fused):
    """module boundary: get_loss(x, y, mods=m, noise=z0) against the reference's MHEnt, both mods sets, both targets"""
    g = load_golden(f"mhent_xyz_{tag}")
    model = _model_from_golden(g)
    trunk = _dev(g["trunk"])
    model.feat_extractor.res.forward = lambda x: trunk        # the fixture pins everything after the trunk
    model.fused_entropy = fused
    B = int(g["B"])
    x = torch.zeros(B, 3, 8, 8, device="cuda")
    for tname in TARGETS:
        for mname, mods in MODS.items():
            key = f"{tname}_{mname}"
            out = model.get_loss(x, _y(g, tname), mods=list(reversed(mods)) if tname == "near" else mods, noise=_dev(g["z0_loss"]))
            assert set(out) == {"th_norm", "bt_norm", "log_p", "q_log_p_z_giv_y", "h_q_z_giv_i"}
            for k in out:
                assert_close(out[k].cpu(), g[f"{key}_loss_{k}"], RTOL, what=f"{key} {k}")


def _tables():
    from test_gpu_train import _tables as t
    return t()


def _det_th45(z):
    """the decoder's operands of fixture rows z [R,61] = [th3 th45 bt logs t]: th45 [R,45] and det [B,16] = [th3 bt logs t]"""
    z = torch.as_tensor(z)
    return z[:, 3:48].contiguous(), torch.cat([z[:, :3], z[:, 48:]], 1).contiguous()


@pytest.mark.parametrize("tag", ["small", "shipped"])
def test_mano_kernel_terms_match_reference_vectors(gpu_lib, tag):
    """per-row terms (uv, xyz, th3, th45, bt) and log_p of mhe_mano_joints_mods_f32 on the fixture's hypotheses"""
    from mhentropy_amd import ops
    g = load_golden(f"mhent_xyz_{tag}")
    B = int(g["B"])
    th45, det = _det_th45(g["z_loss"])
    blob, _ = _tables()
    names = ["log_p_uv_giv_z", "log_p_xyz_giv_z", "log_p_th3", "log_p_th45", "log_p_bt"]
    for tname in TARGETS:
        y = _y(g, tname)
        for mname, mods in MODS.items():
            key = f"{tname}_{mname}"
            o = ops.mano_joints(_dev(th45), _dev(det[:B]), blob, y["crop_uv"] if "uv" in mods else None, y["vis"], 0.03, 50.0,
                                want=("terms", "log_p"), pose3d=y["pose3d"], mods=mods, laplace_b_3d=0.03)
            terms = o["terms"].cpu()
            for c, n in enumerate(names):
                if n == "log_p_uv_giv_z" and "uv" not in mods:
                    assert (terms[:, c] == 0).all(), key
                    continue
                assert_close(terms[:, c], g[f"{key}_terms_{n}"], RTOL, what=f"{key} {n}")
            assert_close(o["log_p"].cpu(), g[f"{key}_terms_log_p"], RTOL, what=f"{key} log_p")


def test_uv_only_mods_entry_is_bit_identical_to_the_uv_entry(gpu_lib):
    """mods = uv through the new entry point: the same kernel arithmetic as mhe_mano_joints_f32 (terms[:, 1] is the xyz slot, 0)"""
    from mhentropy_amd import ops
    blob, _ = _tables()
    rng = np.random.default_rng(11)
    B, N = 16, 64
    th45 = _dev(rng.normal(0, 1.2, (N * B, 45)).astype(np.float32))
    det = rng.normal(0, 1, (B, 16)).astype(np.float32)
    det[:, 3:13] *= 0.05
    det = _dev(det)
    _, yn = synth.batch(4, B, with_image=False)
    y = {k: _dev(v) for k, v in yn.items()}
    want = ("z", "xyz", "uv", "terms", "log_p", "norms", "joints_mm")
    a = ops.mano_joints(th45, det, blob, y["crop_uv"], y["vis"], 0.03, 50.0, want=want)
    b = ops.mano_joints(th45, det, blob, y["crop_uv"], y["vis"], 0.03, 50.0, want=want, mods=["uv"])
    assert b["terms"].shape == (N * B, 5) and (b["terms"][:, 1] == 0).all()
    assert torch.equal(a["terms"], b["terms"][:, [0, 2, 3, 4]])
    for k in ("log_p", "norms", "z", "xyz", "uv", "joints_mm"):
        assert torch.equal(a[k], b[k]), k
    g = _dev(rng.normal(0, 1, (B,)).astype(np.float32))
    ga = ops.mano_joints_bwd(th45, det, blob, y["crop_uv"], y["vis"], g, N)
    gb = ops.mano_joints_bwd(th45, det, blob, y["crop_uv"], y["vis"], g, N, mods=["uv"])
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])


@pytest.mark.parametrize("mods", [["xyz", "uv"], ["xyz"]])
@pytest.mark.parametrize("target", ["far", "near"])
def test_mano_reverse_xyz_matches_f64_autograd(gpu_lib, mods, target):
    """d sum_b g_b log_p_b / d (th45, det) with the 3D term against f64 autograd on the oracle decode; invisible joints, a non-zero
    pose3d root (far: its constant term takes no gradient) and a target within 2e-3 ... 2e-2 of every hypothesis' joints (near)"""
    from mhentropy_amd import ops
    from oracle import network_ref
    blob, tb = _tables()
    tb64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in tb.items()}
    rng = np.random.default_rng(5)
    B, N = 3, 4
    th45 = torch.as_tensor(rng.normal(0, 0.8, (N * B, 45)).astype(np.float32))
    det = torch.as_tensor(rng.normal(0, 1.0, (B, 16)).astype(np.float32))
    det[:, 3:13] *= 0.03
    det[:, 13:] *= 0.2
    _, yn = synth.batch(3, B, with_image=False)
    y = {k: torch.as_tensor(v).double() for k, v in yn.items()}
    assert (y["vis"] == 0).any() and (y["vis"][:, network_ref.ROOT_IDX] == 1).any()
    if target == "near":
        # within 2e-3 ... 2e-2 of hypothesis 0's joints (clear of the 1e-4 dead zone), the exactly-zero root left at 0
        with torch.no_grad():
            z0 = network_ref.combine_z(det.double(), th45[:B].double())
            xyz0 = network_ref.decode(tb64, z0)["xyz"].flatten(-2)
        off = rng.uniform(2e-3, 2e-2, (B, 63)) * rng.choice([-1.0, 1.0], (B, 63))
        p3 = (xyz0 + torch.as_tensor(off)).float().double()
        p3[:, 3 * network_ref.ROOT_IDX:3 * network_ref.ROOT_IDX + 3] = 0.0
    else:
        p3 = y["pose3d"]
        assert (p3[:, 3 * network_ref.ROOT_IDX:3 * network_ref.ROOT_IDX + 3].abs() > 1e-2).all()
    g = torch.as_tensor(rng.normal(0, 1, (B,)))
    th45_r, det_r = th45.double().requires_grad_(True), det.double().requires_grad_(True)
    z = network_ref.combine_z(det_r.repeat(N, 1), th45_r)
    lp = network_ref.forward_log_p(tb64, z, y, N)
    w3 = y["vis"][..., None].repeat(N, 1, 3).flatten(-2)
    lx = network_ref.laplace_log_prob(p3.repeat(N, 1), network_ref.decode(tb64, z)["xyz"].flatten(-2), w3, b=0.03)
    rows = (lp["log_p_uv_giv_z"] + lx if "uv" in mods else lx) + lp["log_p_th3"] + lp["log_p_th45"] + lp["log_p_bt"]
    (rows.reshape(N, B).mean(0) * g).sum().backward()
    cu = _dev(yn["crop_uv"]) if "uv" in mods else None
    g45, gdet = ops.mano_joints_bwd(_dev(th45), _dev(det), blob, cu, _dev(yn["vis"]), _dev(g.float()), N, pose3d=_dev(p3.float()),
                                    mods=mods, laplace_b_3d=0.03)
    assert_close(g45.cpu(), th45_r.grad, RTOL, what="d/d th45")
    assert_close(gdet.cpu(), det_r.grad, RTOL, what="d/d det")
    # the root's 3D term is a constant: moving the target's root moves log_p by that constant only, and no gradient
    if target == "far":
        p3b = p3.clone()
        p3b[:, 3 * network_ref.ROOT_IDX:3 * network_ref.ROOT_IDX + 3] += 0.5
        g45b, gdetb = ops.mano_joints_bwd(_dev(th45), _dev(det), blob, cu, _dev(yn["vis"]), _dev(g.float()), N,
                                          pose3d=_dev(p3b.float()), mods=mods, laplace_b_3d=0.03)
        assert torch.equal(g45b, g45) and torch.equal(gdetb, gdet)


def _ts_from_golden(g):
    from mhentropy_amd.train import TrainStep
    return TrainStep(_model_from_golden(g).train())


@pytest.mark.parametrize("tag", ["small", "shipped"])
def test_train_step_xyz_matches_the_references_own_gradients(gpu_lib, tag):
    """TrainStep.forward_backward(None, y, trunk_out=..., mods=m): loss values (1e-4) and the reference's autograd gradients (2e-4)"""
    g = load_golden(f"mhent_xyz_{tag}")
    steps, N = int(g["steps"]), int(g["N_loss"])
    ts = _ts_from_golden(g)
    params = dict(ts.model.named_parameters())
    for tname in TARGETS:
        for mname, mods in MODS.items():
            key = f"{tname}_{mname}"
            out = ts.forward_backward(None, _y(g, tname), noise=_dev(g["z0_loss"]), N=N, trunk_out=_dev(g["trunk"]), mods=mods)
            for k in ("log_p", "q_log_p_z_giv_y", "h_q_z_giv_i"):
                assert_close(out[k].cpu(), g[f"{key}_loss_{k}"], RTOL, what=f"{key} {k}")
            for name in ("det_head.2.weight", "q_z_giv_i.s.0.l.0.weight", f"q_z_giv_i.t.{2 * steps - 1}.l.2.weight"):
                assert_close(ts.grad_of(params[name]).cpu(), g[f"{key}_grad_{name}"], 2e-4, what=f"{key} d loss / d {name}")
            assert_close(ts.tape["g_feat"].cpu(), g[f"{key}_grad_feat"], 2e-4, what=f"{key} d loss / d feat")


def _small_model():
    from test_gpu_train import _model_and_state
    return _model_and_state("resnet18", 64, 2)[0]


def test_autograd_bridge_xyz_equals_the_fused_reverse_pass(gpu_lib):
    """the reference's loop (get_loss -> total_loss.backward()) in 3D-supervised mode: .grad equals the explicit reverse pass of the
    same trainer on the same parameters"""
    from mhentropy_amd.train import TrainStep
    xn, yn = synth.batch(3, 4, image_size=96)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    z0 = torch.as_tensor(synth.noise(3, 6 * 4)).cuda()
    model = _small_model()
    ts = TrainStep(model).attach()
    for mods in (["xyz", "uv"], ["xyz"]):
        model.zero_grad()
        out = model.get_loss(x, y, mods=mods, N=6, noise=z0)
        assert out["log_p"].requires_grad and not out["th_norm"].requires_grad
        (-out["log_p"]).mean().backward()
        got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        assert len(got) == len(list(model.parameters()))
        lp = out["log_p"].detach().clone()
        uv = model.get_loss(x, y, mods=["uv"], N=6, noise=z0)          # a different mode is a different loss
        assert (uv["log_p"].detach() - lp).abs().min() > 1e-3
        ref = ts.forward_backward(x, y, noise=z0, N=6, mods=mods)
        assert_close(lp.cpu(), ref["log_p"].cpu(), 1e-6, what=f"{mods} log_p")
        for n, p in model.named_parameters():
            assert_close(got[n].cpu(), ts.grad_of(p).cpu(), 1e-5, what=f"{mods} d loss / d {n}")


def test_graphed_step_xyz_replays_bit_equal_to_eager(gpu_lib):
    """GraphedStep in 3D-supervised mode (ResNet-18, 128x128, B=8, N=4, lr 0 so every step sees the same parameters): the replay equals
    the eager step bit for bit, also after a new pose3d is copied into the captured static batch"""
    from mhentropy_amd.train import TrainStep, GraphedStep
    B, N, mods = 8, 4, ["xyz", "uv"]
    xn, yn = synth.batch(21, B, image_size=128)
    x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    p3b = torch.as_tensor(synth.batch(22, B, with_image=False)[1]["pose3d"]).cuda()
    z0 = torch.as_tensor(synth.noise(21, N * B)).cuda()
    ts = TrainStep(_small_model(), lr=0.0)
    eager = []
    for p3 in (y["pose3d"], p3b):
        o = ts.step(x, dict(y, pose3d=p3), noise=z0, N=N, mods=mods)
        eager.append((ts.G.clone(), o["log_p"].clone(), o["total"].clone()))
    assert not torch.equal(eager[0][1], eager[1][1])
    sy = {k: v.clone() for k, v in y.items()}
    gs = GraphedStep(ts, x.clone(), sy, noise=z0, N=N, mods=mods)
    for i, p3 in enumerate((y["pose3d"], p3b, y["pose3d"])):
        sy["pose3d"].copy_(p3)
        o = gs.replay()
        torch.cuda.synchronize()
        G, lp, tot = eager[i % 2]
        assert torch.equal(o["log_p"], lp) and torch.equal(o["total"], tot), i
        assert torch.equal(ts.G, G), i


def test_glow_branch_xyz_term_is_the_mean_of_its_rows(gpu_lib):
    """Glow branch (parity unpinned): xyz-mode q_log_p_z_giv_y minus uv-mode equals the per-image mean over N of the xyz row terms
    of the same hypotheses"""
    from mhentropy_amd import harness, ops
    from mhentropy_amd.network import MHEnt
    from mhentropy_amd.train import TrainStep
    special, common = harness.mhent_cfgs(backbone="resnet18", tables=synth.mano_tables(0))
    special["q_z_giv_i_model"] = "glow"
    model = MHEnt(special, **common)
    model.q_z_giv_i.load_state_dict({k: torch.as_tensor(v) for k, v in synth.glow_state(3).items()}, strict=False)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in synth.head_state(4, 512).items()}, strict=False)
    model = model.cuda().train()
    B, N = 3, 5
    _, yn = synth.batch(5, B, with_image=False)
    y = {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
    f = _dev(np.random.default_rng(6).normal(0, 0.5, (B, 512)).astype(np.float32))
    noise = _dev(np.random.default_rng(7).normal(0, 1, (B, N, 45)).astype(np.float32))
    ts = TrainStep(model)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {}
    for key, mods in (("uv", ["uv"]), ("xyz_uv", ["xyz", "uv"])):
        ops.rng_state(dev, seed=12)                      # the same dropout masks -> the same hypotheses in both modes
        res[key] = ts.forward_backward(None, y, noise=noise, N=N, trunk_out=f, mods=mods)
        res[key + "_th45"] = ts.tape["th45"].clone()
        res[key + "_det"] = ts.tape["det"].clone()
    assert torch.equal(res["uv_th45"], res["xyz_uv_th45"])
    assert torch.equal(res["uv"]["h_q_z_giv_i"], res["xyz_uv"]["h_q_z_giv_i"])
    blob = model.mano_dec.table_blob()
    o = ops.mano_joints(res["xyz_uv_th45"], res["xyz_uv_det"], blob, y["crop_uv"], y["vis"], model.b_2d, model.th45_ref_alpha,
                        want=("terms",), pose3d=y["pose3d"], mods=["xyz", "uv"], laplace_b_3d=model.b_3d)
    xyz_mean = o["terms"][:, 1].reshape(N, B).mean(0)
    diff = res["xyz_uv"]["q_log_p_z_giv_y"] - res["uv"]["q_log_p_z_giv_y"]
    scale = res["xyz_uv"]["q_log_p_z_giv_y"].abs().max().item()
    assert (diff - xyz_mean).abs().max().item() <= 1e-5 * scale, (diff, xyz_mean)
    assert xyz_mean.abs().min().item() > 1.0


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
x, y = torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
z0 = torch.as_tensor(synth.noise(40 + rank, N * B)).cuda()
res = {}
for name, sharded in (("images", False), ("hypotheses", True)):
    model, _ = _model_and_state("resnet18", 64, 2)
    ts = TrainStep(model, dist=dist, shard_hypotheses=sharded)
    out = ts.forward_backward(x, y, noise=z0, N=N, mods=["xyz", "uv"])
    ts.finish_allreduce()
    res[name] = (out["log_p"].clone(), out["q_log_p_z_giv_y"].clone(), ts.G.clone() / world, ts.tape["g_feat"].clone())
uv = TrainStep(_model_and_state("resnet18", 64, 2)[0], dist=dist, shard_hypotheses=True).forward(x, y, noise=z0, N=N)
a, b = res["images"], res["hypotheses"]
rel = lambda u, v: float((u - v).abs().max() / (v.abs().max() + 1e-30))
with open(os.path.join(os.environ["MHE_OUT"], f"x2_rank{rank}.json"), "w") as fh:
    json.dump({"log_p": rel(b[0], a[0]), "q": rel(b[1], a[1]), "grad": rel(b[2], a[2]), "g_feat": rel(b[3], a[3]),
               "uv_differs": rel(uv["q_log_p_z_giv_y"], b[1])}, fh)
dist.destroy_process_group()
'''


def test_hypothesis_sharded_xyz_step_equals_the_image_sharded_one(gpu_lib, tmp_path):
    """TrainStep(shard_hypotheses=True) in 3D-supervised mode on two gloo ranks, one GPU: the gathered pose3d rows give the same loss
    terms and gradients as the image-sharded step"""
    script = tmp_path / "x2_worker.py"
    script.write_text(X2_WORKER)
    env = dict(os.environ, MHE_ROOT=ROOT, MHE_OUT=str(tmp_path), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), str(script)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-3000:]
    for r in range(2):
        rec = json.load(open(tmp_path / f"x2_rank{r}.json"))
        assert rec["log_p"] < 1e-5 and rec["q"] < 1e-5, rec
        assert rec["g_feat"] < 2e-3 and rec["grad"] < 2e-3, rec
        assert rec["uv_differs"] > 1e-3, rec


def test_run_main_with_mods_uv_xyz(gpu_lib):
    """python -m mhentropy_amd.run --mods uv,xyz: eager, replayed from HIP graphs, and fed by the GPU input pipeline"""
    from mhentropy_amd import run
    common = ["--backbone", "resnet18", "--batch", "4", "--hyps", "4", "--hidden", "64", "--flow-steps", "2", "--dtype", "f32", "--epochs", "1"]
    for extra in (["--iters", "3", "--image-size", "96", "--mods", "uv,xyz"],
                  ["--iters", "3", "--image-size", "96", "--mods", "xyz", "--graph", "1"],
                  ["--iters", "2", "--mods", "uv,xyz", "--input-pipeline"]):
        log = run.main(common + extra)
        assert len(log) == 1 and np.isfinite(log[0]["loss"]) and all(np.isfinite(v) for v in log[0]["it_losses"]), (extra, log)
    with pytest.raises(NotImplementedError):
        run.main(common + ["--iters", "1", "--mods", "uv,depth"])
