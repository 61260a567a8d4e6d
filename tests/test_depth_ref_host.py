"""CPU: the depth distance's host side - the f64 restatement the GPU tests compare with (tests/depth_ref.py) against a hand-computed triangle,
against central finite differences of its own dist in both offset modes and against the identity sum g(p) = 0 of the fitted offset; the choice
of seeds (the exact cases have no ambiguous and no fragile sample, the MANO-sized one stays under CAP); ops.depth_obs's sampling rule against
numpy; the two C entries declared with the arity the bindings use; and the Python error paths of criteria.depth_dist / depth_select, raised on
CPU tensors before any device use."""
import numpy as np
import pytest
import torch

import depth_ref as dr
from mhentropy_amd import _lib, criteria, ops


def test_single_triangle_by_hand():
    """S = 4, log s = 0, t = 0: X = 2 v_x + 1.5.  The triangle a = (-0.5, -0.5), b = (3, -0.5), c = (-0.5, 3) in sample units covers the six
    samples with x + y <= 2 (its hypotenuse is x + y = 2.5); v_z = (0, 1, 0) and zscale 0.1 give R = 0.1 (x + 0.5) / 3.5.  obs = 0.5 on all 16
    samples, root_z = 0.5: e = R > 0; at x = 2 it is 0.0714 > trunc = 0.05.  So
        dist = (3 * 0.1 * 0.5 / 3.5 + 2 * 0.1 * 1.5 / 3.5 + 0.05 + 10 * 0.05) / 16
    and with g = 1/16 on the five inliers (x, y) = (0, 0..2), (1, 0..1): sum lam_b = (3 * 0.5 + 2 * 1.5) / 3.5, sum lam_c = 6.5 / 3.5."""
    to_v = lambda X: (X + 0.5) / 2 - 1
    verts = np.array([[to_v(-0.5), to_v(-0.5), 0.0], [to_v(3.0), to_v(-0.5), 1.0], [to_v(-0.5), to_v(3.0), 0.0]])[None, None]
    ref = dr.depth_dist64(verts, [[0, 1, 2]], np.zeros((1, 1, 3)), [0.1], np.full((1, 4, 4), 0.5), [0.5], 0.05)
    covered = {(y, x) for y in range(4) for x in range(4) if x + y <= 2}
    assert {tuple(p) for p in np.argwhere(ref["face_img"][0, 0] == 0)} == covered and (ref["face_img"][0, 0] >= 0).sum() == 6
    assert abs(ref["dist"][0, 0] - (3 * 0.1 * 0.5 / 3.5 + 2 * 0.1 * 1.5 / 3.5 + 0.05 + 10 * 0.05) / 16) < 1e-15
    assert np.allclose(ref["parts"][0, 0], [6 / 16, 0.5, 5 / 6], rtol=0, atol=1e-15)
    sb, sc = (3 * 0.5 + 2 * 1.5) / 3.5, 6.5 / 3.5
    assert np.allclose(ref["g_verts"][0, 0, :, 2], np.array([5 - sb - sc, sb, sc]) * 0.1 / 16, rtol=0, atol=1e-15)
    # dR/dX_k = -gx lam_k with gx = 0.1 / 3.5 per sample, dX/dv_x = 2; gy = 0
    assert np.allclose(ref["g_verts"][0, 0, :, 0], -np.array([5 - sb - sc, sb, sc]) * (0.1 / 3.5) * 2 / 16, rtol=0, atol=1e-15)
    assert np.allclose(ref["g_verts"][0, 0, :, 1], 0, atol=1e-15)
    # the weights of a sample sum to 1: d/dt_x = -gx * S/2 per inlier; d/dlog s = sum_k dX_k v_x S/2
    assert abs(ref["g_logs_t"][0, 0, 1] + 5 * (0.1 / 3.5) * 2 / 16) < 1e-15 and abs(ref["g_logs_t"][0, 0, 2]) < 1e-15
    assert abs(ref["g_logs_t"][0, 0, 0] - (ref["g_verts"][0, 0, :, 0] * verts[0, 0, :, 0]).sum()) < 1e-15


def _fd_configuration(seed=13):
    """two triangles that overlap, S = 8, one row; seed 13 is the first whose samples all keep 0.05 spacings from every edge in both modes"""
    rng = np.random.default_rng(seed)
    verts = np.concatenate([rng.uniform(-0.8, 0.8, (1, 1, 6, 2)), rng.uniform(-0.4, 0.4, (1, 1, 6, 1))], -1)
    logs_t = np.concatenate([rng.uniform(-0.1, 0.1, (1, 1, 1)), rng.uniform(-0.05, 0.05, (1, 1, 2))], -1)
    obs = 0.5 + rng.uniform(-0.07, 0.07, (1, 8, 8))
    obs[rng.uniform(0, 1, obs.shape) < 0.1] = 0
    return verts, np.array([[0, 1, 2], [3, 4, 5]]), logs_t, np.array([0.1]), obs, np.array([0.52])


@pytest.mark.parametrize("root", [False, True])
def test_gradient_against_central_differences_of_the_restatement(root):
    v, faces, lt, zs, obs, root_z = _fd_configuration()
    rz = root_z if root else None
    ref = dr.depth_dist64(v, faces, lt, zs, obs, rz, dr.TRUNC)
    # the piecewise-constant parts do not move: no sample within 0.05 spacings of an edge, no |e| within 1e-4 of trunc (or of 0)
    assert ref["edge_min"].min() > 0.05 and not ref["ambiguous"].any(), ref["edge_min"].min()
    e = ref["resid_img"][np.isfinite(ref["resid_img"])]
    assert e.size >= 12 and np.abs(np.abs(e) - dr.TRUNC).min() > 1e-4 and np.abs(e).min() > 1e-4
    assert (np.abs(e) < dr.TRUNC).sum() >= 4 and (np.abs(e) > dr.TRUNC).sum() >= 2          # both branches of the truncation
    assert len(set(ref["face_img"][ref["face_img"] >= 0])) == 2                            # both faces win samples
    f = lambda vv, ll: dr.depth_dist64(vv, faces, ll, zs, obs, rz, dr.TRUNC)["dist"]
    rng = np.random.default_rng(3)
    h = 1e-6
    for _ in range(6):
        dv, dl = rng.normal(0, 1, v.shape), rng.normal(0, 1, lt.shape)
        fd = (f(v + h * dv, lt + h * dl) - f(v - h * dv, lt - h * dl)) / (2 * h)
        an = (ref["g_verts"] * dv).sum((2, 3)) + (ref["g_logs_t"] * dl).sum(2)
        assert np.abs(an).max() > 1e-4 and np.abs(fd - an).max() <= 1e-7 * np.abs(an).max(), (fd, an)


def test_weights_of_the_fitted_offset_sum_to_zero():
    """sum_p g(p) = 0 because the offset moves with the mesh: the z gradients, each g(p) w_k zscale with the w_k of a sample summing to 1, cancel"""
    for name in ("mix_16_h64", "random_16_h64"):
        op, ref = dr.case(name, False)
        total = ref["g_verts"][..., 2].sum(-1) / op["zscale"][None]
        assert np.abs(ref["g_verts"][..., 2]).sum() > 1e-3 and np.abs(total).max() < 1e-15, total
        _, given = dr.case(name, True)
        assert np.abs(given["g_verts"][..., 2].sum(-1)).max() > 1e-5          # (not so with a given offset)


def test_seeds_of_the_cases():
    for name in dr.EXACT:
        for root in (False, True):
            _, ref = dr.case(name, root)
            assert not ref["ambiguous"].any() and ref["fragile"].sum() == 0, (name, root, int(ref["ambiguous"].sum()), int(ref["fragile"].sum()))
    _, ref = dr.case("mano_64", False)
    assert 0 < ref["ambiguous"].mean() <= dr.CAP
    _, edges = dr.case("edges_8", True)
    assert (edges["n_obs"][:, 1] == 0).all() and (edges["dist"][:, 1] == 0).all()          # O empty
    assert edges["dist"][1, 0] == dr.TRUNC and edges["parts"][1, 0, 0] == 0                   # P empty: the mesh beside the mask
    assert np.isnan(edges["dist"][2, 0]) and np.isfinite(edges["dist"][2, 1])
    _, far = dr.case("far_8", True)
    assert np.abs(far["dist"] - dr.TRUNC).max() < 1e-15 and (far["parts"][..., 2] == 0).all() and (far["parts"][..., 0] > 0).all()
    assert np.abs(far["g_verts"]).max() == 0


@pytest.mark.parametrize("S,k", [(8, 1), (8, 4), (5, 3), (16, 2)])
def test_depth_obs_sampling_rule(S, k):
    rng = np.random.default_rng(S * 10 + k)
    H = S * k
    depth = rng.uniform(0.2, 1.0, (3, H, H)).astype(np.float32)
    depth[rng.uniform(0, 1, depth.shape) < 0.2] = 0.0
    depth[0, k // 2, k // 2], depth[1, k // 2, k // 2], depth[2, k // 2, k // 2] = np.nan, np.inf, -0.3
    mask = rng.uniform(0, 1, (3, H, H)) < 0.5
    mask[:, :k, :k] = True
    want = dr.depth_obs64(depth, mask, S)
    assert want[0, 0, 0] == 0 and want[1, 0, 0] == 0 and want[2, 0, 0] == 0 and (want > 0).any() and (want == 0).any()
    for m in (torch.as_tensor(mask), torch.as_tensor(mask.astype(np.uint8)), torch.as_tensor(mask.astype(np.float32))):
        got = ops.depth_obs(torch.as_tensor(depth), m, S)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, S, S)
        assert np.array_equal(got.numpy(), want.astype(np.float32))
    # one sample, not a mean: the block's centre element
    assert want.max() in depth[:, k // 2::k, k // 2::k]


def test_entries_are_declared_with_the_arity_the_bindings_use():
    assert len(_lib.SIGNATURES["mhe_depth_dist_f32"][1]) == 17 and len(_lib.SIGNATURES["mhe_depth_dist_bwd_f32"][1]) == 18
    assert (ops.DEPTH_MAX_SIZE, ops.DEPTH_MAX_VERTS, ops.DEPTH_MAX_FACES) == (64, 1024, 2048)
    with open(_lib.HEADER_PATH) as f:
        h = f.read()
    for name, val in (("SIZE", 64), ("VERTS", 1024), ("FACES", 2048)):
        assert f"#define MHE_DEPTH_MAX_{name} {val}\n" in h


def test_face_adjacency_on_the_host():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3], [3, 9, 0], [1, 1, 4]], dtype=torch.int32)
    start, lst = ops.face_adjacency(faces, 5)
    assert start.tolist() == [0, 1, 5, 7, 8, 9]
    # (face << 2) | corner, ascending per vertex; face 2 has an index outside [0, 5): no entry
    assert lst.tolist() == [0, 1, 5, 12, 13, 2, 4, 6, 14, -1, -1, -1]
    assert ops.face_adjacency(faces, 5)[0] is start          # kept on the tensor


def _good(N=2, B=2, V=3, H=8):
    return dict(verts=torch.zeros(N, B, V, 3), logs_t=torch.zeros(N, B, 3), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32),
                depth=torch.ones(B, H, H), hand_mask=torch.ones(B, H, H, dtype=torch.bool), scale=torch.ones(B))


@pytest.mark.parametrize("change,match", [
    (dict(verts=torch.zeros(2, 2, 4)), "verts must be"),
    (dict(verts=torch.zeros(2, 2, 1025, 3)), "V=1025"),
    (dict(logs_t=torch.zeros(2, 2, 2)), "logs_t must be"),
    (dict(faces=torch.zeros(2049, 3, dtype=torch.int32)), "faces must be"),
    (dict(faces=torch.zeros(1, 3)), "faces must be"),
    (dict(depth=torch.ones(2, 8, 7)), "depth must be"),
    (dict(hand_mask=torch.ones(2, 16, 16)), "hand_mask is"),
    (dict(hand_mask=torch.ones(3, 8, 8)), "hand_mask must be"),
    (dict(scale=torch.ones(3)), "scale must be"),
    (dict(root_z=torch.ones(2, 3)), "root_z must be"),
    (dict(size=3), "not a multiple"),
    (dict(size=128), "size=128"),
    (dict(trunc=0.0), "trunc="),
    (dict(trunc=float("nan")), "trunc="),
])
def test_depth_dist_refuses_bad_operands_before_any_device_use(change, match):
    kw = dict(_good(), size=8)
    kw.update(change)
    with pytest.raises(ValueError, match=match):
        criteria.depth_dist(**kw)


def test_depth_select_refuses_bad_operands_before_any_device_use():
    g = _good()
    output = {"verts": g["verts"], "logs_t": g["logs_t"], "faces": g["faces"]}
    target = {"depth": g["depth"], "hand_mask": g["hand_mask"], "scale": g["scale"]}
    for k in output:
        with pytest.raises(ValueError, match=f"output has no '{k}'"):
            criteria.depth_select({a: b for a, b in output.items() if a != k}, target, size=8)
    for k in target:
        with pytest.raises(ValueError, match=f"target has no '{k}'"):
            criteria.depth_select(output, {a: b for a, b in target.items() if a != k}, size=8)
    with pytest.raises(ValueError, match="target has no 'pose3d_root'"):
        criteria.depth_select(output, target, size=8, root=True)
    with pytest.raises(ValueError, match="pose3d_root'] must be"):
        criteria.depth_select(output, dict(target, pose3d_root=torch.zeros(2, 2)), size=8, root=True)
    for Q in (0, 3, 1.0):
        with pytest.raises(ValueError, match="Q="):
            criteria.depth_select(output, target, Q=Q, size=8)
    with pytest.raises(_lib.MheError):          # well-formed CPU tensors: refused, there is no CPU path
        criteria.depth_select(output, target, size=8)
