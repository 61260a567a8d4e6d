"""Host (no GPU): the designed HO3D edge cases of tests/ho3d_edge_ref.py reach every edge they are named after, are deterministic
and exactly projectable, run through the oracle, and the oracle reproduces what the reference's own `__getitem__` recorded for
eight of them (tests/golden/ho3d_edge_*.npz, written by oracle/gen_golden.py:gen_ho3d_edges)."""
import math

import numpy as np
import pytest

import ho3d_edge_ref as edge
from conftest import assert_close, load_golden
from oracle import ho3d_ref


@pytest.fixture(scope="module")
def hits():
    return {n: edge.hits(n, b) for b in edge.BATCHES for n in b}


def test_every_case_is_in_exactly_one_batch():
    names = [n for b in edge.BATCHES for n in b]
    assert sorted(names) == sorted(edge.CASES) and max(len(b) for b in edge.BATCHES) <= 16


@pytest.mark.parametrize("key", edge.REQUIRED)
def test_every_key_is_hit_by_the_case_named_after_it(hits, key):
    """a condition, not a measurement: without the designed case (or with one that drifted off its edge) this fails"""
    case = key.split("/")[0]
    assert case in edge.CASES, f"no designed case {case}"
    assert key in hits[case], f"{case} does not reach {key}: it reaches {sorted(hits[case])}"


def test_unreachable_edges_are_unreachable(hits):
    """the crop width is always even and the resize clamp never binds (ho3d_edge_ref's docstring has the argument): over the
    designed cases, and over a sweep of integer centres and float32 sizes that includes every .5 and .25 step"""
    for n, h in hits.items():
        assert not {n + "/resize_odd", n + "/resize_clamp_taken"} & h, n
    for c in (0, 1, 150, 151, 479):
        for size in np.arange(0.5, 330, 0.25, dtype=np.float32):
            x1, _, x2, _ = ho3d_ref.crop_window((c, c), size)
            cw = x2 - x1
            assert cw % 2 == 0, (c, size)
            if cw:
                assert math.floor(255 * (cw / 256)) <= cw - 1 and int(np.floor(np.arange(256) * (cw / 256)).max()) <= cw - 1, (c, size)


def test_builders_are_deterministic():
    for n in edge.CASES:
        (a, pa), (b, pb) = edge.build(n), edge.build(n)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a), n
        assert (pa is None and pb is None) or np.array_equal(pa, pb), n


@pytest.mark.parametrize("name", [n for n in edge.CASES if "near_pi" not in n])
def test_projection_is_exact(name):
    """float32 and float64 evaluation of xyz2uvd give the same bits, for the joints and (zero rotation) for the object"""
    s, _ = edge.build(name)
    J32 = ho3d_ref.xyz2uvd(s["joints3d"] * np.float32(1000.0), s["cam"])
    J64 = ho3d_ref.xyz2uvd(s["joints3d"].astype(np.float64) * 1000.0, s["cam"].astype(np.float64))
    assert J32.dtype == np.float32 and np.array_equal(J32.astype(np.float64), J64.astype(np.float64))
    o = s["obj_verts"] + s["obj_trans"]
    assert np.array_equal(ho3d_ref.xyz2uvd(o * np.float32(1000.0), s["cam"]).astype(np.float64),
                          ho3d_ref.xyz2uvd(o.astype(np.float64) * 1000.0, s["cam"].astype(np.float64)).astype(np.float64))
    uv = J64[:, :2].astype(np.float64) * 1024
    assert np.array_equal(uv, np.rint(uv)), "joints sit on the 1/1024 pixel lattice"


def test_oracle_runs_on_every_case_and_sees_the_designed_visibilities():
    for n in edge.CASES:
        s, a = edge.build(n)
        for prm in ([None] if a is None else [None, edge.aug_dict(a)]):
            img, t = ho3d_ref.getitem(s, prm)
            assert img.shape == (3, 256, 256) and np.isfinite(img).all(), n
            for k, v in t.items():
                assert np.isfinite(np.asarray(v, np.float64)).all(), (n, k)
            if n == "vis1":
                assert np.array_equal(t["vis"], np.asarray(edge.VIS1_EXPECT, np.float32)[ho3d_ref.HO3D2RHD]), t["vis"]
            if n == "vis1_right":
                assert t["vis"][0] == 1 and t["vis"].sum() == 1
            if n == "vis2_low":          # joints 0..3 at -4, just below, (y) -4, just below; 6, 7 one pixel inside the limit
                assert [t["vis"][ho3d_ref.HO3D2RHD.index(j)] for j in (0, 1, 2, 3, 6, 7)] == [1, 0, 1, 0, 1, 1]
            if n == "vis2_high":         # 259, just above, 258, 255
                assert [t["vis"][ho3d_ref.HO3D2RHD.index(j)] for j in (0, 1, 2, 3)] == [1, 0, 1, 1]
    s, _ = edge.build("fuse_both_x_clamps_f64_size")
    scale = edge.intermediates(s)[5]
    assert type(scale) is float and scale == 480.0


@pytest.mark.parametrize("name,augmented", edge.GOLDEN)
def test_oracle_matches_the_reference_on_designed_cases(name, augmented):
    """the existing suite's rule: vis and crop_center exact, the rest to 2e-6 of the tensor's scale (+1e-7)"""
    g = load_golden("ho3d_edge_" + name)
    assert int(g["aug"]) == int(augmented)
    s, a = edge.build(name)
    _, t = ho3d_ref.getitem(s, edge.aug_dict(a) if augmented else None)
    assert np.array_equal(t["vis"], g["vis"]) and np.array_equal(t["crop_center"], g["crop_center"])
    for k in ("crop_uv", "crop_size", "st", "scale", "pose3d"):
        assert_close(t[k].reshape(g[k].shape), g[k], 2e-6, 1e-7, what=f"{name}: {k}")
