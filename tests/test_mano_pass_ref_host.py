"""CPU: anchors of tests/mano_pass_ref.py, the float64 reference of tests/test_gpu_mano_edges.py - against the vectors the original project's own
_forward_log_p returned (tests/golden/mhent_small.npz, priors_outside.npz, mhent_xyz_small.npz, at the tolerances those fixtures' own oracle tests
use), against itself in float32, and its autograd gradient against a central difference."""
import numpy as np
import pytest
import torch

import mano_pass_ref as mr
from conftest import load_golden, assert_close


def _operands(z, B):
    """fixture rows z [R,61] = [th3 th45 bt logs t] -> th45 [R,45], det [B,16] = [th3 bt logs t]"""
    return np.ascontiguousarray(z[:, 3:48]), np.concatenate([z[:B, :3], z[:B, 48:61]], 1)


@pytest.mark.parametrize("name,zkey", [("mhent_small", "z_loss"), ("priors_outside", "z")])
def test_reference_matches_the_original_projects_uv_vectors(name, zkey):
    """z, the four terms and log_p (1e-6 of the tensor's scale, as tests/test_oracle_golden.py)"""
    g = load_golden(name)
    z = g[zkey]
    B = int(g["B"]) if name == "mhent_small" else z.shape[0] // int(g["N"])          # priors_outside records its hypotheses per image, N
    th45, det = _operands(z, B)
    assert np.array_equal(np.tile(det, (z.shape[0] // B, 1)), np.concatenate([z[:, :3], z[:, 48:61]], 1))          # rows are n * B + b
    o = mr.mano_pass(th45, det, g["y_crop_uv"], g["y_vis"])
    assert_close(o["z"], z, 0.0, what="z")
    for i, k in enumerate(("log_p_uv_giv_z", "log_p_th3", "log_p_th45", "log_p_bt")):
        assert_close(o["terms4"][:, i], g["terms_" + k], 1e-6, 1e-12, what=k)
    if name == "mhent_small":          # this fixture keeps log_p as its mean over the N hypotheses of an image
        assert_close(o["log_p"].reshape(-1, B).mean(0), g["loss_q_log_p_z_giv_y"], 1e-6, what="log_p, mean over n")
    else:
        assert_close(o["log_p"], g["terms_log_p"], 1e-6, what="log_p")
    if name == "priors_outside":
        assert (o["terms4"][:, 1:].min(0) < -10).all()          # the fixture drives all three priors


def test_reference_matches_the_original_projects_xyz_vectors():
    """the 5-wide terms of mhent_xyz_small.npz, both targets, mods = xyz | uv and xyz (1e-5, as tests/test_xyz_oracle.py)"""
    g = load_golden("mhent_xyz_small")
    B = int(g["B"])
    th45, det = _operands(g["z_loss"], B)
    names = ("log_p_uv_giv_z", "log_p_xyz_giv_z", "log_p_th3", "log_p_th45", "log_p_bt")
    for tname in ("far", "near"):
        for mname, mods in (("xyz_uv", 3), ("xyz", 2)):
            key = f"{tname}_{mname}"
            o = mr.mano_pass(th45, det, g["y_crop_uv"], g["y_vis"], g[f"{tname}_pose3d"], mods=mods, laplace_b_3d=float(g["b_3d"]))
            for c, n in enumerate(names):
                if c == 0 and not mods & 1:
                    assert (o["terms5"][:, 0] == 0).all()
                    continue
                assert_close(o["terms5"][:, c], g[f"{key}_terms_{n}"], 1e-5, what=f"{key} {n}")
            assert_close(o["log_p"], g[f"{key}_terms_log_p"], 1e-5, what=f"{key} log_p")


def _random_case(R=6, B=3, seed=3):
    from mhentropy_amd import synth
    rng = np.random.default_rng(seed)
    th45 = rng.normal(0, 0.8, (R, 45)).astype(np.float32)
    det = (rng.normal(0, 1.0, (B, 16)) * np.array([1.0] * 3 + [0.03] * 10 + [0.2] * 3)).astype(np.float32)
    _, y = synth.batch(seed, B, with_image=False)
    scale = rng.uniform(0.025, 0.04, B).astype(np.float32)
    root = (rng.uniform(-80, 80, (B, 3)) + np.array([0, 0, 500.0])).astype(np.float32)
    obj = (root[:, None] + rng.uniform(-90, 90, (B, 12, 3))).astype(np.float32)
    return th45, det, y, (scale, root, obj, np.array([0, 5, 40], np.int32)), rng.normal(0, 1, B).astype(np.float32)


def test_float32_and_float64_calls_agree_to_float32_accuracy():
    th45, det, y, cham, g = _random_case()
    kw = dict(mods=3, chamfer=cham, chamfer_w=10.0, grad=True, g_log_p=g, row_w=0.5)
    a = mr.mano_pass(th45, det, y["crop_uv"], y["vis"], y["pose3d"], **kw)
    b = mr.mano_pass(th45, det, y["crop_uv"], y["vis"], y["pose3d"], dtype=torch.float32, **kw)
    assert a["gap"] > mr.CH_GAP          # every Chamfer minimum of the case is determined in float32 too
    for k in ("z", "xyz", "uv", "uv_inv", "terms5", "log_p", "norms", "joints_mm", "dist", "g_th45", "g_det"):
        assert a[k].dtype == np.float64 and np.isfinite(a[k]).all(), k
        assert_close(b[k], a[k], 0.0 if k == "z" else 2e-5, what=k)
        assert mr.bound(a, b, k) <= 6e-5 * np.abs(a[k]).max(), k
    # the clamp of obj_count: 0 acts as 1, 40 as VO = 12
    c = mr.mano_pass(th45, det, chamfer=(cham[0], cham[1], cham[2], np.array([1, 5, 12], np.int32)))
    assert np.array_equal(c["dist"], a["dist"])
    # inv_norm only maps uv (and with it the uv likelihood)
    d = mr.mano_pass(th45, det, y["crop_uv"], y["vis"], inv_norm=True, image_size=224.0)
    assert_close(d["uv"], (a["uv"] + 1.0) / 2.0 * 224.0, 1e-14, what="uv, inv_norm")
    assert np.array_equal(d["uv"], d["uv_inv"]) and np.array_equal(d["xyz"], a["xyz"])


def test_rows_are_independent():
    """a subset of the rows with their image index gives the same values: what the GPU suite's R = 8199 test relies on"""
    th45, det, y, cham, g = _random_case()
    kw = dict(mods=3, chamfer=cham, chamfer_w=10.0, grad=True, g_log_p=g, row_w=0.5)
    a = mr.mano_pass(th45, det, y["crop_uv"], y["vis"], y["pose3d"], **kw)
    rows = np.array([4, 1])
    b = mr.mano_pass(th45[rows], det, y["crop_uv"], y["vis"], y["pose3d"], img=rows % 3, **kw)
    for k in ("xyz", "uv", "terms5", "log_p", "norms", "joints_mm", "dist", "g_th45", "g_det"):
        assert_close(b[k], a[k][rows], 1e-13, what=k)


def test_autograd_gradient_agrees_with_a_central_difference():
    th45, det, y, cham, g = _random_case(R=3, B=3)
    kw = dict(mods=3, chamfer=cham, chamfer_w=10.0)

    def loss(t, d):
        o = mr.mano_pass(t, d, y["crop_uv"], y["vis"], y["pose3d"], **kw)
        return float((g.astype(np.float64) * (o["log_p"] - 10.0 * o["dist"])).sum())

    a = mr.mano_pass(th45, det, y["crop_uv"], y["vis"], y["pose3d"], grad=True, g_log_p=g, **kw)
    h = 1e-6
    th, dt = th45.astype(np.float64), det.astype(np.float64)
    for r, c in ((0, 0), (1, 17), (2, 44)):
        e = np.zeros_like(th)
        e[r, c] = h
        fd = (loss(th + e, dt) - loss(th - e, dt)) / (2 * h)
        assert abs(fd - a["g_th45"][r, c]) <= 1e-6 * np.abs(a["g_th45"]).max(), (r, c, fd, a["g_th45"][r, c])
    for r, c in ((0, 1), (1, 7), (2, 13), (0, 15)):          # th3, beta, log s, t (R = B: row r is image r)
        e = np.zeros_like(dt)
        e[r, c] = h
        fd = (loss(th, dt + e) - loss(th, dt - e)) / (2 * h)
        assert abs(fd - a["g_det"][r, c]) <= 1e-6 * np.abs(a["g_det"][:, c]).max(), (r, c, fd, a["g_det"][r, c])


def test_zero_pose_is_finite_in_value_and_gradient():
    """hands_mean = 0, th45 = 0, th3 = 0: all 16 axis-angles exactly zero - Rodrigues at its + 1e-8 epsilon gives the identity and a finite,
    non-zero gradient, in float64 and in float32"""
    from mhentropy_amd import synth
    _, y = synth.batch(5, 2, with_image=False)
    th45, det = np.zeros((2, 45), np.float32), np.zeros((2, 16), np.float32)
    det[1, 3:13] = 0.01
    g = np.array([1.0, -2.0], np.float32)
    out = {}
    for dt in (torch.float64, torch.float32):
        o = mr.mano_pass(th45, det, y["crop_uv"], y["vis"], y["pose3d"], mods=3, zero_mean=True, dtype=dt, grad=True, g_log_p=g)
        for k, v in o.items():
            assert np.isfinite(v).all(), (dt, k)
        assert np.abs(o["g_th45"]).max() > 1.0 and np.abs(o["g_det"][:, :3]).max() > 1.0
        assert (o["terms5"][:, 2:] == 0).all() and (o["norms"][0] == 0).all()
        out[dt] = o
    for k in ("xyz", "uv", "log_p", "g_th45", "g_det"):
        assert_close(out[torch.float32][k], out[torch.float64][k], 2e-5, what=k)
