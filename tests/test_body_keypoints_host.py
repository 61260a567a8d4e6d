"""CPU: the body-keypoint entry points refuse bad arguments before any launch (MHE_ERR_ARG with mhe_last_error() naming the entry), their size
queries agree with the documented layouts, and the Python surface (BodyLayer's keypoint_regressor, synthetic_body_tables(keypoints=NK),
keypoint_log_prob's checks) behaves as documented without a device."""
import numpy as np
import pytest
import torch

from mhentropy_amd import _lib, body

MHE_ERR_ARG = 1


def _small_tables(keypoints=0, seed=3):
    return body.synthetic_body_tables(seed, NV=200, J=5, nb=4, parents=(-1, 0, 1, 1, 2), keypoints=keypoints)


def test_size_queries_and_support():
    L = _lib.lib()
    VP = 6912                                                     # SMPL's 6,890 vertices padded to a multiple of 64
    # [VP / 32 vertex tiles][2 k-steps][NKT keypoint tiles][3 pieces][64 lanes x 8] bf16, in floats
    assert L.mhe_lbs_kp_split_floats(17, VP) == VP // 32 * 2 * 1 * 3 * 512 // 2
    assert L.mhe_lbs_kp_split_floats(32, VP) == L.mhe_lbs_kp_split_floats(1, VP)
    assert L.mhe_lbs_kp_split_floats(64, VP) == 2 * L.mhe_lbs_kp_split_floats(17, VP) == L.mhe_lbs_kp_split_floats(33, VP)
    for nk in (0, -1, 65):
        assert L.mhe_lbs_kp_split_floats(nk, VP) == 0
        assert L.mhe_lbs_skin_kp_supported(128, 24, 10, 6890, VP, nk, 1) == 0
    assert L.mhe_lbs_kp_split_floats(17, VP + 8) == 0
    # SMPL's sizes fit (hypotheses' pieces + four staging tiles within the 160 KiB of LDS); R <= 0 and J > 32 do not
    assert L.mhe_lbs_skin_kp_supported(16384, 24, 10, 6890, VP, 17, 1) == 1 and L.mhe_lbs_skin_kp_supported(16384, 24, 10, 6890, VP, 64, 0) == 1
    assert L.mhe_lbs_skin_kp_supported(0, 24, 10, 6890, VP, 17, 1) == 0 and L.mhe_lbs_skin_kp_supported(8, 33, 10, 6890, VP, 17, 1) == 0
    # the vertex output's 4 GiB limit applies only when vertices are written
    assert L.mhe_lbs_skin_kp_supported(60000, 24, 10, 6890, VP, 17, 1) == 0 and L.mhe_lbs_skin_kp_supported(60000, 24, 10, 6890, VP, 17, 0) == 1


def test_c_entries_refuse_before_launching():
    L = _lib.lib()
    Z = None
    cases = {
        "mhe_lbs_kp_split_tables_f32": [lambda: L.mhe_lbs_kp_split_tables_f32(Z, Z, 17, 6890, 6912, Z)],
        "mhe_lbs_skin_kp_mfma_f32": [lambda nk=nk: L.mhe_lbs_skin_kp_mfma_f32(Z, Z, Z, Z, Z, 8, 24, 10, 6890, 6912, nk, 1.0, Z) for nk in (0, 65, 17)],
        "mhe_lbs_skin_kp_f32": [lambda nk=nk: L.mhe_lbs_skin_kp_f32(Z, Z, Z, Z, Z, Z, Z, Z, 8, 24, 10, 6890, 6912, nk, 1.0, Z) for nk in (0, 65, 17)],
        "mhe_lbs_keypoints_bwd_f32": [lambda nk=nk: L.mhe_lbs_keypoints_bwd_f32(Z, Z, Z, 8, nk, 6890, 0, Z) for nk in (0, 65, 17)],
        "mhe_kp_log_prob_f32": [lambda nk=nk: L.mhe_kp_log_prob_f32(Z, Z, Z, Z, Z, 2, 3, nk, 1, 0.03, Z) for nk in (0, 65, 17)],
        "mhe_kp_log_prob_bwd_f32": [lambda nk=nk: L.mhe_kp_log_prob_bwd_f32(Z, Z, Z, Z, Z, Z, Z, 2, 3, nk, 0, 0.03, Z) for nk in (0, 65, 17)],
    }
    for name, calls in cases.items():
        for call in calls:
            assert call() == MHE_ERR_ARG, name
            assert name.encode() in L.mhe_last_error(), (name, L.mhe_last_error())


def test_synthetic_regressor_leaves_the_other_tables_alone():
    a, b = body.synthetic_body_tables(5, NV=2000), body.synthetic_body_tables(5, NV=2000, keypoints=19)
    assert sorted(b) == sorted(list(a) + ["keypoint_regressor"])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    kr = b["keypoint_regressor"]
    assert kr.shape == (19, 2000) and kr.dtype == np.float32 and (kr >= 0).all()
    np.testing.assert_allclose(kr.sum(1), 1.0, rtol=1e-6)
    onehot = [(kr[k] == 1.0).sum() == 1 and (kr[k] != 0).sum() == 1 for k in range(19)]
    assert [k for k in range(19) if onehot[k]] == [2, 6, 10, 14, 18]


def test_layer_surface_without_a_device():
    plain, with_kp = body.BodyLayer(_small_tables()), body.BodyLayer(_small_tables(keypoints=7))
    assert plain.NK == 0 and "keypoint_regressor" not in plain.state_dict()
    assert sorted(with_kp.state_dict()) == sorted(list(plain.state_dict()) + ["keypoint_regressor"])          # (kernel-side layouts are non-persistent)
    assert with_kp.NK == 7 and tuple(with_kp.keypoint_regressor.shape) == (7, 200)
    t = _small_tables(keypoints=7)
    for bad in (np.zeros((0, 200), np.float32), np.zeros((65, 200), np.float32), np.zeros((7, 199), np.float32), np.zeros(200, np.float32)):
        with pytest.raises(ValueError, match="keypoint_regressor"):
            body.BodyLayer({**t, "keypoint_regressor": bad})
    with pytest.raises(ValueError, match="keypoint_regressor"):
        plain(torch.zeros(2, 4), rotmats=torch.zeros(2, 5, 3, 3), want_keypoints=True)
    with pytest.raises(ValueError, match="keypoint_regressor"):
        body.lbs_bwd(plain, torch.zeros(2, 5, 3, 3), torch.zeros(2, 4), None, g_keypoints=torch.zeros(2, 7, 3))


def test_keypoint_log_prob_checks_its_arguments():
    kp, cam, uv, vis = torch.zeros(2, 3, 5, 3), torch.zeros(2, 3, 3), torch.zeros(2, 5, 2), torch.ones(2, 5)
    with pytest.raises(_lib.MheError, match="keypoint_log_prob.keypoints"):                  # host tensors: the hot path has no CPU fallback
        body.keypoint_log_prob(kp, cam, uv, vis)
    for bad_kp in (torch.zeros(2, 3, 5, 2), torch.zeros(2, 3, 0, 3), torch.zeros(2, 3, 65, 3), torch.zeros(6, 5, 3)):
        with pytest.raises(ValueError, match="keypoint_log_prob"):
            body.keypoint_log_prob(bad_kp, cam, uv, vis)
    for bad_cam in (torch.zeros(2, 4, 3), torch.zeros(3, 3), torch.zeros(2, 3, 2)):
        with pytest.raises(ValueError, match="cam"):
            body.keypoint_log_prob(kp, bad_cam, uv, vis)
    with pytest.raises(ValueError, match="positive"):
        body.keypoint_log_prob(kp, cam, uv, vis, b=0.0)
