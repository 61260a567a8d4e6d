"""Golden vectors of the reference's 3D-supervised loss, get_loss(mods=['xyz', 'uv']) and get_loss(mods=['xyz'])
(hand/CrossModalHand.py:354, hand/network.py:393,398-400,620-662), for tests/golden/mhent_xyz_{small,shipped}.npz.

Runs where the reference tree exists (like oracle/gen_golden.py, whose helpers it reuses unchanged): drives the
reference's own MHEnt on CPU with the seeds, sizes and trunk features of mhent_{small,shipped}, checks the oracle
composition  network_ref.decode + laplace_log_prob(b=0.03) + flows_ref.log_prob  against it, and stores data only.

Two targets per size:
  far   the synthetic pose3d of synth.batch (every coordinate far from the decoded joints, root included);
  near  the decoded xyz of hypothesis 0 of each image plus offsets of magnitude >= 2e-3 (every element clear of the
        Laplace's 1e-4 dead zone except the exactly-zero root, which is left at 0).
The vis of synth.batch has invisible joints in every image.

    python tools/gen_golden_xyz.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mhentropy_amd import synth  # noqa: E402
from oracle import flows_ref, mano_ref, network_ref  # noqa: E402
from oracle.gen_golden import GOLD, REF, _FixedPrior, _close, _install_placeholders, _mhent, _t  # noqa: E402

B_3D = 0.03                     # hand/network.py:393
MODS = {"xyz_uv": ["xyz", "uv"], "xyz": ["xyz"]}


def oracle_loss(sd, tb, feat, y, z0, N, mods):
    """_reverse_kld (hand/network.py:760-831) with the 3D term, from the conditioning feature on"""
    z = network_ref.sample_q(sd, feat, z0, N)
    lp = network_ref.forward_log_p(tb, z, y, N)
    w3 = y["vis"][..., None].repeat(N, 1, 3).flatten(-2)
    lx = network_ref.laplace_log_prob(y["pose3d"].repeat(N, 1), network_ref.decode(tb, z)["xyz"].flatten(-2), w3, b=B_3D)
    lik = lp["log_p_uv_giv_z"] + lx if "uv" in mods else lx
    rows = lik + lp["log_p_th3"] + lp["log_p_th45"] + lp["log_p_bt"]          # the reference's dict order (network.py:620-662)
    out = {"th_norm": z[:, :48].norm(p=2, dim=1), "bt_norm": z[:, 48:58].norm(p=2, dim=1)}
    out["q_log_p_z_giv_y"] = rows.reshape(N, -1).mean(0)
    log_q = flows_ref.log_prob(network_ref.sub(sd, "q_z_giv_i."), z[:, 3:48], feat.repeat(N, 1))
    out["h_q_z_giv_i"] = (-log_q).reshape(N, -1).mean(0)
    out["log_p"] = out["h_q_z_giv_i"] + out["q_log_p_z_giv_y"]
    out["_z"], out["_xyz_rows"] = z, lx
    return out


def gen(network, tables, tag, seed, h, steps, B):
    print(f"[mhent_xyz_{tag}]")
    model, sdn = _mhent(network, tables, seed, h, steps)
    model.train()
    sd = _t(sdn)
    tb = mano_ref.tables_from_numpy(tables)
    _, yn = synth.batch(seed, B, with_image=False)
    rng = np.random.default_rng(seed + 99)
    trunk = torch.as_tensor(rng.normal(0, 0.5, (B, 2048)).astype(np.float32))      # the trunk feature of mhent_{tag}
    model.feat_extractor.res.fixed = trunk
    x_dummy = torch.zeros(B, 3, 8, 8)
    N = 10                                                                          # network.py:780
    z0 = torch.as_tensor(synth.noise(seed, N * B))
    model.q_z_giv_i.prior = _FixedPrior(model.q_z_giv_i.prior, z0)
    feat = torch.nn.functional.linear(trunk, sd["feat_extractor.l1.0.weight"], sd["feat_extractor.l1.0.bias"])

    # the near target: hypothesis 0's decoded joints (rows 0..B-1 are n = 0) plus offsets of 2e-3 ... 2e-2 with random signs
    with torch.no_grad():
        xyz0 = network_ref.decode(tb, network_ref.sample_q(sd, feat, z0, N))["xyz"][:B].flatten(-2)
    orng = np.random.default_rng(seed + 313)
    off = orng.uniform(2e-3, 2e-2, (B, 63)) * orng.choice([-1.0, 1.0], (B, 63))
    near = (xyz0.double() + torch.as_tensor(off)).float()
    near[:, 3 * network_ref.ROOT_IDX:3 * network_ref.ROOT_IDX + 3] = 0.0
    assert ((near - xyz0).abs()[:, [k for k in range(63) if k // 3 != network_ref.ROOT_IDX]] >= 1.9e-3).all()
    targets = {"far": torch.as_tensor(yn["pose3d"]), "near": near}

    gold = dict(seed=seed, h=h, steps=steps, B=B, N_loss=N, trunk=trunk.numpy(), z0_loss=z0.numpy(), feat=feat.numpy(), b_3d=B_3D)
    gold.update({"y_" + k: v for k, v in yn.items() if k != "pose3d"})
    gnames = ["det_head.2.weight", "q_z_giv_i.s.0.l.0.weight", f"q_z_giv_i.t.{2 * steps - 1}.l.2.weight"]
    pr = dict(model.named_parameters())
    for tname, p3 in targets.items():
        y = _t({k: v for k, v in yn.items() if k != "pose3d"})
        y["pose3d"] = p3
        y["image"] = torch.zeros(B, 1)
        gold[f"{tname}_pose3d"] = p3.numpy()
        for mname, mods in MODS.items():
            key = f"{tname}_{mname}"
            ref = model.get_loss(x_dummy, y, mods=mods)
            feat_req = feat.clone().requires_grad_(True)
            sd_g = dict(sd)
            for n in gnames:
                sd_g[n] = sd[n].clone().requires_grad_(True)
            out = oracle_loss(sd_g, tb, feat_req, y, z0, N, mods)
            for k in ("th_norm", "bt_norm", "q_log_p_z_giv_y", "h_q_z_giv_i", "log_p"):
                _close(f"{key} get_loss.{k}", out[k], ref[k], 5e-5, 5e-4)
            g_ref = torch.autograd.grad((-ref["log_p"]).mean(), [pr[n] for n in gnames] + [pr["feat_extractor.l1.0.bias"]])
            g = torch.autograd.grad((-out["log_p"]).mean(), [sd_g[n] for n in gnames] + [feat_req])
            for n, a, b in zip(gnames, g[:3], g_ref[:3]):
                _close(f"{key} grad {n}", a, b, 2e-4, 1e-6)
            _close(f"{key} grad feat (sum over B == dL/d l1.bias)", g[3].sum(0), g_ref[3], 2e-4, 1e-6)
            with torch.no_grad():
                terms_ref = model._forward_log_p(out["_z"].detach(), y, use_gt=[], mods=mods, feat=feat)
                # the issue's composition, to the bit: laplace_log_prob(pose3d.repeat(N,1), decode(tb, z)['xyz'], vis repeated, b=0.03)
                lx = network_ref.laplace_log_prob(p3.repeat(N, 1), network_ref.decode(tb, out["_z"].detach())["xyz"].flatten(-2),
                                                  y["vis"][..., None].repeat(N, 1, 3).flatten(-2), b=B_3D)
            assert torch.equal(lx, terms_ref["log_p_xyz_giv_z"]), key + ": log_p_xyz_giv_z is not the oracle's to the bit"
            tkeys = ["log_p_xyz_giv_z", "log_p_th3", "log_p_th45", "log_p_bt", "log_p"] + (["log_p_uv_giv_z"] if "uv" in mods else [])
            gold.update({f"{key}_loss_{k}": ref[k].detach().numpy() for k in ("th_norm", "bt_norm", "q_log_p_z_giv_y", "h_q_z_giv_i", "log_p")})
            gold.update({f"{key}_terms_{k}": terms_ref[k].numpy() for k in tkeys})
            gold.update({f"{key}_grad_{n}": a.numpy() for n, a in zip(gnames, g_ref[:3])})
            gold[f"{key}_grad_feat"] = g[3].detach().numpy()
        if tname == "far":
            gold["z_loss"] = out["_z"].detach().numpy()
    np.savez_compressed(os.path.join(GOLD, f"mhent_xyz_{tag}.npz"), **gold)


def main():
    tables = synth.mano_tables(0)
    _install_placeholders(tables)
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir("/tmp")
    import network        # noqa: E402  (reference module)
    os.chdir(cwd)
    torch.manual_seed(0)
    gen(network, tables, "small", 21, 64, 2, 2)          # the sizes of oracle/gen_golden.py's mhent_small / mhent_shipped
    gen(network, tables, "shipped", 22, 512, 6, 3)
    print("golden fixtures written to", GOLD)


if __name__ == "__main__":
    main()
