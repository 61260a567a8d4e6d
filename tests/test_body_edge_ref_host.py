"""CPU checks of tests/body_edge_ref.py, the reference and case table of tests/test_gpu_body_edges.py: the exact-arithmetic cases are exact, the
builder's tables are valid, the case table holds every size class the launchers distinguish (by the launchers' formulas, restated there), and the
reference is the pinned one (oracle/mano_ref.py through oracle/body_ref.py at the MANO sizes)."""
import numpy as np
import pytest
import torch

import body_edge_ref as br
from conftest import assert_close, load_golden
from mhentropy_amd import synth
from oracle import body_ref, mano_ref

ALL = br.CASES + br.ERR_CASES


@pytest.mark.parametrize("c", br.CASES, ids=lambda c: c["name"])
def test_dyadic_cases_are_exact(c):
    """every output of the forward pass of the dyadic model is the same number in float32 and in float64, for the scales 0.5 and 4: a case that is
    not is malformed (the GPU test asserts bit-equality against it)"""
    t = br.tables(c["seed"], c["NV"], c["J"], c["nb"], c["NK"], True)
    rot, betas = br.inputs(c["seed"], c["R"], c["J"], c["nb"], True)
    for scale in (0.5, 4.0):
        a, b = br.forward(t, rot, betas, scale, torch.float64), br.forward(t, rot, betas, scale, torch.float32)
        for k in a:
            assert np.array_equal(a[k], b[k]), (c["name"], k)
            assert np.array_equal(a[k].astype(np.float32).astype(np.float64), a[k]), (c["name"], k, "not representable in f32")
            assert (not a[k].size or np.abs(a[k]).max() < 2.0 ** 20) and np.array_equal(a[k] * 32, np.round(a[k] * 32)), (c["name"], k)
        pm, A, joints = br.pose_parts(br.tb_torch(t, torch.float32), torch.as_tensor(np.array(rot)), torch.as_tensor(np.array(betas)))
        v = br.skin_parts(br.tb_torch(t, torch.float32), pm, torch.as_tensor(np.array(betas)), A) * scale
        assert np.array_equal(v.double().numpy(), a["verts"]) and np.array_equal(joints.double().numpy(), a["joints"])


@pytest.mark.parametrize("dyadic", [False, True])
def test_tables_are_valid(dyadic):
    for c in ALL:
        t = br.tables(c["seed"], c["NV"], c["J"], c["nb"], c["NK"], dyadic)
        J, NV, nb = c["J"], c["NV"], c["nb"]
        assert t["v_template"].shape == (NV, 3) and t["shapedirs"].shape == (NV, 3, nb) and t["posedirs"].shape == (NV, 3, 9 * (J - 1))
        assert t["weights"].shape == (NV, J) and t["J_regressor"].shape == (J, NV)
        assert_close(t["weights"].astype(np.float64).sum(1), np.ones(NV), 1e-6, what="weights rows")
        assert_close(t["J_regressor"].astype(np.float64).sum(1), np.ones(J), 1e-6, what="regressor rows")
        assert (t["weights"] >= 0).all() and (t["J_regressor"] >= 0).all()
        p = t["parents"]
        assert p[0] == -1 and (p[1:] >= 0).all() and (p[1:] < np.arange(1, J)).all() and tuple(p[:24]) == br.SMPL_PARENTS[:J]
        if c["NK"]:
            kr = t["keypoint_regressor"]
            assert kr.shape == (c["NK"], NV)
            assert_close(kr.astype(np.float64).sum(1), np.ones(c["NK"]), 1e-6, what="keypoint rows")
            assert kr[0, NV - 1] == 1.0 and (kr[0] != 0).sum() == 1          # a one-hot row on the last live vertex
        if dyadic:
            for k in ("weights", "J_regressor") + (("keypoint_regressor",) if c["NK"] else ()):
                assert ((t[k] == 0) | (t[k] == 1)).all() and (t[k].sum(1) == 1).all(), k
            for k in ("v_template", "shapedirs", "posedirs"):
                assert np.array_equal(t[k] * 16, np.round(t[k] * 16)) and (not t[k].size or np.abs(t[k]).max() <= 0.5), k
        L = br.layouts(t, c["VP"], 1e3)
        assert L["vt"].shape == (3, c["VP"]) and L["vsd"].shape == (nb, 3, c["VP"]) and L["vpd"].shape == (9 * (J - 1), 3, c["VP"])
        assert L["vw"].shape == (J, c["VP"]) and (L["vw"][:, NV:] == 1e3).all() and np.array_equal(L["vw"][:, :NV], t["weights"].T)
        assert np.array_equal(L["vsd"][:, :, :NV], t["shapedirs"].transpose(2, 1, 0)) and (L["vt"][:, NV:] == 1e3).all()


def test_case_table_holds_every_size_class():
    cs = br.CASES
    models = {(c["J"], c["nb"]) for c in cs}
    assert models == set(br.MODELS) and len(br.MODELS) == 19
    for m in br.MODELS:
        assert len({(c["NV"], c["VP"]) for c in cs if (c["J"], c["nb"]) == m}) >= 2, m
    for v in br.VERTS:
        assert {br.js(c["J"]) for c in cs if (c["NV"], c["VP"]) == v} == {1, 2}, v
    assert {c["R"] for c in cs} == set(br.ROWS) and {c["scale"] for c in cs} == set(br.SCALES) and {c["NK"] for c in cs} == set(br.NKS)
    rev = [c for c in cs if c["J"] >= 2]
    assert {br.nt(c["J"], c["nb"]) for c in rev} == set(range(1, 12))                        # every launch_coef<NT>
    nt_of = {m: br.nt(*m) for m in br.MODELS if m[0] >= 2}
    assert [nt_of[m] for m in [(4, 10), (8, 10), (12, 10), (16, 10), (20, 10), (24, 10), (28, 10)]] == [2, 3, 4, 5, 6, 7, 8]
    assert (nt_of[(2, 1)], nt_of[(3, 14)], nt_of[(3, 15)], nt_of[(28, 13)]) == (1, 1, 2, 8) and 9 * 2 + 14 == 32 and 9 * 27 + 13 == 256
    assert (nt_of[(32, 1)], nt_of[(32, 33)], nt_of[(32, 64)]) == (9, 10, 11)
    assert any(c["J"] % 2 for c in rev) and any((9 * (c["J"] - 1) + c["nb"]) % 2 for c in rev)      # sbw_lds_g / sbw_lds_a round an odd count up
    # the template's two K slots: across the operand halves (7 | 8), across a k-step (15 | 16); K filling its k-steps and one past them
    slot = lambda J, nb: 9 * (J - 1) + nb
    assert slot(1, 7) == 7 and slot(2, 6) == 15 and slot(2, 1) + 2 == 12 and slot(3, 12) + 2 == 32 and br.ks(3, 12) == 2
    assert slot(3, 13) + 2 == 33 and (33 + 15) // 16 == 3 and br.ks(3, 13) == 4 and slot(3, 13) == 31
    # the joint k-steps: one joint, eight and all sixteen in the second
    assert {c["J"] - 16 for c in cs if br.js(c["J"]) == 2} >= {1, 8, 16} and {c["J"] for c in cs if br.js(c["J"]) == 1} >= {1, 16}
    # vertex tiling: fewer tiles than waves, NV <= 32, NV a multiple of 32, pitches 32 and 96, a pitch more than one tile beyond NV
    vs = {(c["NV"], c["VP"]) for c in cs}
    assert vs == set(br.VERTS)
    assert any(nv < 128 for nv, _ in vs) and any(nv <= 32 for nv, _ in vs) and any(nv % 32 == 0 for nv, _ in vs)
    assert {32, 96} <= {vp for _, vp in vs} and any(vp - nv > 32 for nv, vp in vs) and all(vp % 32 == 0 and vp >= nv for nv, vp in vs)
    assert all(c["NV"] <= 300 and c["R"] <= 70 for c in cs)
    # keypoints on the matrix cores: everything but (32, 64), whose pieces, store tiles and staging tiles are 165,888 bytes
    assert br.kp_lds(32, 64, 1) == 165888 > br.LDS_LIMIT
    assert all(br.kp_lds(J, nb, 64) <= br.LDS_LIMIT for J, nb in br.MODELS if (J, nb) != (32, 64))
    assert all(br.skin_lds(J, nb) <= br.LDS_LIMIT for J, nb in br.MODELS)
    # the error variant's image classes
    e = {(c["R"], c["R"] // c["B"]) for c in br.ERR_CASES}
    assert e == {(64, 32), (96, 16), (96, 48)} and {br.js(c["J"]) for c in br.ERR_CASES} == {1, 2}
    assert br.R_BIG == 8192 + 7 and len(br.ROWS_BIG) == 39 and br.ROWS_BIG[-1] == br.R_BIG - 1 and set(br.BIG_MODELS) <= models


def test_parts_restate_the_oracle():
    """pose_parts + skin_parts (the halves the workspace row and the skinning reverse's intermediates are taken from) are body_ref.lbs"""
    for c in br.CASES[::3]:
        t = br.tables(c["seed"], c["NV"], c["J"], c["nb"], c["NK"])
        rot, betas = br.inputs(c["seed"], c["R"], c["J"], c["nb"])
        tb = br.tb_torch(t, torch.float64)
        rt, bt = torch.as_tensor(np.array(rot)).double(), torch.as_tensor(np.array(betas)).double()
        verts, joints = body_ref.lbs(tb, rt, bt)
        pm, A, tj = br.pose_parts(tb, rt, bt)
        assert_close(tj, joints, 1e-13, what=c["name"] + " joints")
        assert_close(br.skin_parts(tb, pm, bt, A), verts, 1e-13, what=c["name"] + " verts")
        assert_close(torch.linalg.det(rt), np.ones((c["R"], c["J"])), 1e-6, what="rotations")


def test_reverse_totals_are_the_chain_of_the_parts():
    """g_rot / g_betas through body_ref.lbs = the skinning reverse's intermediates pushed through the pose chain's reverse: the two autograd routes
    the GPU test compares the kernels with agree"""
    c = br.CASES[16]
    t = br.tables(c["seed"], c["NV"], c["J"], c["nb"], c["NK"])
    rot, betas = br.inputs(c["seed"], c["R"], c["J"], c["nb"])
    rng = np.random.default_rng(3)
    gv, gj, gk = rng.normal(0, 1, (c["R"], c["NV"], 3)), rng.normal(0, 1, (c["R"], c["J"], 3)), rng.normal(0, 1, (c["R"], c["NK"], 3))
    a = br.reverse(t, rot, betas, c["scale"], gv, gj, gk)
    b = br.transforms_reverse(t, rot, betas, a["g_tf"], a["g_pm"], gj, a["g_bt"])
    assert_close(b["g_rot"], a["g_rot"], 1e-12, what="g_rot")
    assert_close(b["g_betas"], a["g_betas"], 1e-12, what="g_betas")


def test_reference_at_mano_size_is_the_pinned_hand_forward():
    """the helper's forward() at the MANO sizes against the reference's own vectors, as test_body_lbs_oracle_at_mano_size_is_the_pinned_hand_forward
    pins oracle/body_ref.py"""
    g = load_golden("mano")
    tn = synth.mano_tables(int(g["table_seed"]))
    tb = mano_ref.tables_from_numpy(tn)
    theta, beta = torch.as_tensor(g["theta"]), torch.as_tensor(g["beta"])
    full_pose = torch.cat([theta[:, :3], tb["th_hands_mean"] + theta[:, 3:48].mm(tb["th_selected_comps"])], 1)
    rots = mano_ref.rodrigues(full_pose.reshape(-1, 3)).view(-1, 16, 3, 3)
    t = {"v_template": tn["v_template"], "shapedirs": tn["shapedirs"], "posedirs": tn["posedirs"], "J_regressor": tn["J_regressor"],
         "weights": tn["weights"], "parents": np.asarray(mano_ref.PARENTS)}
    out = br.forward(t, rots.numpy(), beta.numpy(), 1.0, torch.float64)
    centre = out["joints"][:, mano_ref.JOINT_REORDER[9]][:, None]
    assert_close((out["verts"] - centre) * 1000, g["mesh"], 1e-6, what="mesh")
    assert br.ws_stride(16, 10) == 400 and out["ws"].shape[1] == 9 * 15 + 10 + 15 * 16
