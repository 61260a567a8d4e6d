"""CPU: the 3D-supervised loss (get_loss(mods=['xyz', 'uv']), hand/CrossModalHand.py:354, hand/network.py:620-662) - the
reference-generated fixtures tests/golden/mhent_xyz_*.npz (tools/gen_golden_xyz.py) against the oracle composition, and the
C ABI / Python argument checks of the new mode that run before any device work."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, assert_close
from mhentropy_amd import _lib, ops, synth
from oracle import flows_ref, mano_ref, network_ref

MODS = {"xyz_uv": ["xyz", "uv"], "xyz": ["xyz"]}
TARGETS = ("far", "near")


def oracle_loss(sd, tb, feat, y, z0, N, mods, b_3d=0.03):
    """network_ref.decode + laplace_log_prob(b = 0.03) + flows_ref.log_prob: _reverse_kld with the 3D term"""
    z = network_ref.sample_q(sd, feat, z0, N)
    lp = network_ref.forward_log_p(tb, z, y, N)
    w3 = y["vis"][..., None].repeat(N, 1, 3).flatten(-2)
    lx = network_ref.laplace_log_prob(y["pose3d"].repeat(N, 1), network_ref.decode(tb, z)["xyz"].flatten(-2), w3, b=b_3d)
    lik = lp["log_p_uv_giv_z"] + lx if "uv" in mods else lx
    rows = lik + lp["log_p_th3"] + lp["log_p_th45"] + lp["log_p_bt"]
    out = {"th_norm": z[:, :48].norm(p=2, dim=1), "bt_norm": z[:, 48:58].norm(p=2, dim=1)}
    out["q_log_p_z_giv_y"] = rows.reshape(N, -1).mean(0)
    log_q = flows_ref.log_prob(network_ref.sub(sd, "q_z_giv_i."), z[:, 3:48], feat.repeat(N, 1))
    out["h_q_z_giv_i"] = (-log_q).reshape(N, -1).mean(0)
    out["log_p"] = out["h_q_z_giv_i"] + out["q_log_p_z_giv_y"]
    terms = {"log_p_xyz_giv_z": lx, "log_p_th3": lp["log_p_th3"], "log_p_th45": lp["log_p_th45"], "log_p_bt": lp["log_p_bt"],
             "log_p": rows}
    if "uv" in mods:
        terms["log_p_uv_giv_z"] = lp["log_p_uv_giv_z"]
    return out, terms, z


@pytest.mark.parametrize("tag", ["small", "shipped"])
def test_xyz_fixtures_are_the_oracle_composition(tag):
    g = load_golden(f"mhent_xyz_{tag}")
    seed, h, steps, B, N = int(g["seed"]), int(g["h"]), int(g["steps"]), int(g["B"]), int(g["N_loss"])
    assert float(g["b_3d"]) == 0.03
    sdn = {"q_z_giv_i." + k: v for k, v in synth.flow_state(seed, 45, 512, (h, h), steps).items()}
    sdn.update(synth.head_state(seed, 2048, 512, 16))
    sd = {k: torch.as_tensor(v) for k, v in sdn.items()}
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0))
    feat = torch.nn.functional.linear(torch.as_tensor(g["trunk"]), sd["feat_extractor.l1.0.weight"], sd["feat_extractor.l1.0.bias"])
    assert_close(feat, g["feat"], 1e-6, what="feat")
    # the same inputs as mhent_{tag}: the uv-only fixture's trunk and noise
    base = load_golden(f"mhent_{tag}")
    assert np.array_equal(base["trunk"], g["trunk"]) and np.array_equal(base["z0_loss"], g["z0_loss"])
    for tname in TARGETS:
        y = {k[2:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("y_")}
        y["pose3d"] = torch.as_tensor(g[f"{tname}_pose3d"])
        assert (y["vis"] == 0).any(), "the fixtures must exercise invisible joints"
        for mname, mods in MODS.items():
            key = f"{tname}_{mname}"
            with torch.no_grad():
                out, terms, z = oracle_loss(sd, tb, feat, y, torch.as_tensor(g["z0_loss"]), N, mods)
            assert_close(z, g["z_loss"], 1e-6, what=key + " z")
            for k in ("th_norm", "bt_norm", "q_log_p_z_giv_y", "h_q_z_giv_i", "log_p"):
                assert_close(out[k], g[f"{key}_loss_{k}"], 1e-5, what=f"{key} {k}")
            for k, v in terms.items():
                assert_close(v, g[f"{key}_terms_{k}"], 1e-5, what=f"{key} terms {k}")


def test_near_target_clears_the_dead_zone_except_at_the_root():
    """the 'near' pose3d lies within 2e-2 of hypothesis 0's joints but >= 2e-3 from them (the Laplace's 1e-4 dead zone is never
    straddled), with the root left at the exactly-zero normalised root"""
    g = load_golden("mhent_xyz_small")
    B = int(g["B"])
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0))
    with torch.no_grad():
        xyz0 = network_ref.decode(tb, torch.as_tensor(g["z_loss"][:B]))["xyz"].flatten(-2).numpy()
    d = np.abs(g["near_pose3d"] - xyz0)
    root = np.zeros(63, bool)
    root[3 * network_ref.ROOT_IDX:3 * network_ref.ROOT_IDX + 3] = True
    assert (d[:, ~root] >= 1.9e-3).all() and (d[:, ~root] <= 2.1e-2).all()
    assert (g["near_pose3d"][:, root] == 0).all() and (xyz0[:, root] == 0).all()
    assert (np.abs(g["far_pose3d"][:, root]) > 1e-2).all()              # the far target's root is not 0: its term is a constant


def test_new_entry_points_are_declared_and_bound():
    L = _lib.lib()
    for name in ("mhe_mano_joints_mods_f32", "mhe_mano_joints_mods_bwd_f32"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.mhe_abi_version() == 4
    assert (ops.MODS_UV, ops.MODS_XYZ) == (1, 2)
    hdr = open(os.path.join(ROOT, "include", "mhe.h")).read()
    assert "MHE_MODS_UV = 1, MHE_MODS_XYZ = 2" in hdr


def _fake(n):
    """a host buffer: validation must refuse before any pointer is used"""
    return C.cast(C.create_string_buffer(4 * n), C.c_void_p)


@pytest.mark.parametrize("case", ["mods0", "mods_unknown", "xyz_no_pose3d", "uv_no_crop_uv", "b3d_zero"])
def test_mods_entry_points_validate_before_any_device_work(case):
    L = _lib.lib()
    R, B = 4, 2
    th45, det, cu, vis, p3, tb = _fake(R * 45), _fake(B * 16), _fake(B * 42), _fake(B * 21), _fake(B * 63), _fake(16)
    terms, logp, g, g45, grows = _fake(R * 5), _fake(R), _fake(B), _fake(R * 45), _fake(R * 16)
    mods, b3 = 3, 0.03
    if case == "mods0":
        mods = 0
    elif case == "mods_unknown":
        mods = 4
    elif case == "xyz_no_pose3d":
        p3 = None
    elif case == "uv_no_crop_uv":
        cu = None
    else:
        b3 = 0.0
    rc = L.mhe_mano_joints_mods_f32(th45, det, cu, vis, p3, tb, None, None, None, terms, logp, None, None, R, B, mods, 0.03, b3, 50.0,
                                    0, 256.0, None)
    assert rc == 1, rc                                                              # MHE_ERR_ARG
    assert L.mhe_last_error().decode().startswith("mhe_mano_joints_mods_f32")
    rc = L.mhe_mano_joints_mods_bwd_f32(th45, det, cu, vis, p3, tb, g, g45, grows, R, B, mods, 0.03, b3, 50.0, 0.25, None)
    assert rc == 1, rc
    assert L.mhe_last_error().decode().startswith("mhe_mano_joints_mods_bwd_f32")


def test_mods_names():
    assert ops.mods_bits(None) == ops.MODS_UV
    assert ops.mods_bits(["uv"]) == ops.MODS_UV and ops.mods_bits(["xyz"]) == ops.MODS_XYZ
    assert ops.mods_bits(["xyz", "uv"]) == ops.mods_bits(["uv", "xyz"]) == 3
    for bad in (["m"], ["depth"], ["uv", "m"], [], ["uv", "uv"]):
        with pytest.raises(NotImplementedError):
            ops.mods_bits(bad)


def test_get_loss_mode_errors_before_any_device_work():
    """'xyz' without y['pose3d'] names the key; an unbuilt mod raises NotImplementedError as before"""
    from mhentropy_amd import harness
    model = harness.build_mhent(backbone="resnet18", h_dims=(64, 64), num_steps=2, tables=synth.mano_tables(0))
    assert model.b_3d == 0.03
    _, yn = synth.batch(0, 2, with_image=False)
    y = {k: torch.as_tensor(v) for k, v in yn.items() if k != "pose3d"}
    x = torch.zeros(2, 3, 8, 8)
    for mods in (["xyz", "uv"], ["xyz"]):
        with pytest.raises(ValueError, match="pose3d"):
            model.get_loss(x, y, mods=mods)
    for mods in (["m"], ["depth"], ["uv", "m"]):
        with pytest.raises(NotImplementedError):
            model.get_loss(x, y, mods=mods)
