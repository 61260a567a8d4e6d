"""GPU tests of the hand-object Chamfer distance: mhe_chamfer_f32 / mhe_chamfer_bwd_f32 (csrc/chamfer.hip) through ops.chamfer,
criteria.chamfer_dist (a torch.autograd.Function), criteria.MHEntChamferLoss (MHEntLoss with chamfer_select on) and criteria.chamfer_select.  Everything against the float64
restatement of tests/chamfer_ref.py (and, at its size, the reference's own output in tests/golden/chamfer_small.npz), computed once per case
and shared.

Bounds: RTOL = 1e-4 of the reference's largest value, the project's bound for f32 kernels against f64 (tests/test_gpu_body_eval.py); indices
are compared exactly.  Every index-exact case asserts, in f64, that the best and second-best candidate of each minimum differ by more than
chamfer_ref.GAP = 1e-3 relative (f32 rounding of a distance is ~1e-6 relative), so ties exist only where test_ties plants them.

Shapes (N, B, P, VO): the fixture's (3, 2, 21, 37); one vertex; the reference's VO = 1000 (one LDS tile, not full); P = 778 mesh points with
VO = 1031 (past the 1024-vertex tile, odd; P above the reverse's 256 hand points per round; 7 hand points per thread); per-image counts with the
padding planted on the hand."""
import functools

import numpy as np
import pytest
import torch

import chamfer_ref
from conftest import assert_close, load_golden
from mhentropy_amd import criteria, ops

pytestmark = pytest.mark.gpu
RTOL = 1e-4
CASES = {"golden_3x2": (101, 3, 2, 21, 37, None), "one_vertex": (102, 1, 1, 21, 1, None), "reference_size": (103, 5, 3, 21, 1000, None),
         "mesh_1031": (104, 2, 2, 778, 1031, None), "ragged": (105, 4, 3, 21, 64, (37, 5, 64))}
# planted cases (chamfer_ref.PLANTS): exact ties; a hand point ON a vertex, the other vertices far enough out that it is nobody else's nearest
CASES.update(ties=(110, 3, 2, 21, 37, None, "ties"), coincident=(109, 3, 2, 21, 37, None, "coincident", 270.0))
FORWARD = ("golden_3x2", "one_vertex", "reference_size", "mesh_1031", "ragged")


def _cu(a):
    return torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared case arrays are read-only)


@functools.lru_cache(None)
def _case(name):
    case = chamfer_ref.make_case(*CASES[name])
    ref = chamfer_ref.chamfer64(case["points"], case["scale"], case["root"], case["obj"], case.get("count"))
    assert ref["gap"] > chamfer_ref.GAP, (name, ref["gap"])
    return case, ref


def _g_dist(name, shape):
    rng = np.random.default_rng(len(name) + 7)
    return (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


@functools.lru_cache(None)
def _grad(name):
    case, ref = _case(name)
    g = _g_dist(name, ref["dist"].shape)
    return g, chamfer_ref.grad64(case["points"], case["scale"], case["root"], case["obj"], g, case.get("count"))


def _forward(case, want_idx=True):
    cnt = _cu(case["count"]) if "count" in case else None
    out = ops.chamfer(_cu(case["points"]), _cu(case["scale"]), _cu(case["root"]), _cu(case["obj"]), cnt, want_idx=want_idx)
    torch.cuda.synchronize()
    return out


def _check_forward(name):
    case, ref = _case(name)
    dist, parts, idx_p, idx_o = (t.cpu().numpy() for t in _forward(case))
    print(f"{name}: dist err {np.abs(dist - ref['dist']).max():.3e} of {np.abs(ref['dist']).max():.3e}; f64 gap of the minima {ref['gap']:.2e}")
    assert_close(dist, ref["dist"], RTOL, what=name + " dist")
    assert_close(parts, ref["parts"], RTOL, what=name + " parts")
    assert np.array_equal(idx_p, ref["idx_p"]), name + " idx_p"
    assert np.array_equal(idx_o, ref["idx_o"]), name + " idx_o"
    return case, ref, dist


@pytest.mark.parametrize("name", FORWARD)
def test_forward_parity(name, gpu_lib):
    case, ref, dist = _check_forward(name)
    if name == "golden_3x2":
        g = load_golden("chamfer_small")
        assert np.array_equal(case["points"], g["points"]) and np.array_equal(case["obj"], g["obj"])
        assert_close(dist, g["dist"], RTOL, what="dist against the reference's output")
    if name == "ragged":
        # the padding would win every minimum it took part in: the distance over all VO vertices is far smaller
        full = chamfer_ref.chamfer64(case["points"], case["scale"], case["root"], case["obj"])
        assert (full["dist"][0, :2] < 0.5 * ref["dist"][0, :2]).all() and (ref["idx_o"][:, 0, 37:] == -1).all() and (ref["idx_o"][:, 1, 5:] == -1).all()


def test_chamfer_dist_forms(gpu_lib):
    """criteria.chamfer_dist: (N, B, K, 3) -> (N, B) and (B, K, 3) -> (B,), object_verts flat as the pipeline emits it or (B, VO, 3), object_count"""
    case, ref = _case("golden_3x2")
    g = load_golden("chamfer_small")
    for flat in (True, False):
        tgt = {k: _cu(v) for k, v in chamfer_ref.target_of(case, flat).items()}
        d4 = criteria.chamfer_dist(_cu(case["points"]), tgt)
        d3 = criteria.chamfer_dist(_cu(case["points"][1]), tgt)
        assert d4.shape == (3, 2) and d3.shape == (2,) and not d4.requires_grad
        assert_close(d4.cpu().numpy(), g["dist"], RTOL, what="4-D form")
        assert_close(d3.cpu().numpy(), g["dist_3d"], RTOL, what="3-D form")
        assert torch.equal(d3, d4[1])
    case, ref = _case("ragged")
    tgt = {k: _cu(v) for k, v in chamfer_ref.target_of(case).items()}
    assert_close(criteria.chamfer_dist(_cu(case["points"]), tgt).cpu().numpy(), ref["dist"], RTOL, what="object_count")
    with pytest.raises(ValueError, match="outside 1..VO=64"):
        criteria.chamfer_dist(_cu(case["points"]), dict(tgt, object_count=_cu(np.array([37, 65, 64], np.int32))))


def test_ties_go_to_the_lowest_index(gpu_lib):
    case, ref, _ = _check_forward("ties")
    assert not (ref["idx_p"] == 5).any() and not (ref["idx_p"] == 30).any() and not (ref["idx_o"] == 7).any() and not (ref["idx_o"] == 20).any()
    assert all((ref["idx_p"] == v).any() for v in (2, 11)) and all((ref["idx_o"] == j).any() for j in (3, 0))          # every planted tie is met


def _autograd(case, g):
    pts = _cu(case["points"]).requires_grad_(True)
    tgt = {k: _cu(v) for k, v in chamfer_ref.target_of(case).items()}
    dist = criteria.chamfer_dist(pts, tgt)
    assert dist.requires_grad
    (gp,) = torch.autograd.grad(dist, pts, _cu(g))
    torch.cuda.synchronize()
    return dist.detach(), gp


@pytest.mark.parametrize("name", ["golden_3x2", "mesh_1031", "ragged", "coincident"])
def test_reverse_parity(name, gpu_lib):
    case, ref = _case(name)
    g, want = _grad(name)
    dist, gp = _autograd(case, g)
    gp = gp.cpu().numpy()
    print(f"{name}: grad err {np.abs(gp - want).max():.3e} of {np.abs(want).max():.3e}")
    assert_close(dist.cpu().numpy(), ref["dist"], RTOL, what=name + " dist")
    assert np.isfinite(gp).all()
    assert_close(gp, want, RTOL, what=name + " d dist / d points")
    valid = ref["idx_o"][ref["idx_o"] >= 0]
    assert np.bincount(valid).max() >= 2          # several vertices share a nearest hand point: the reverse's gather adds more than one term
    if name == "coincident":
        assert (ref["idx_p"][:, :, 4] == 9).all() and (ref["idx_o"][:, :, 9] == 4).all() and ((ref["idx_o"] == 4).sum(-1) == 1).all()
        assert (want[:, :, 4] == 0).all() and (gp[:, :, 4] == 0).all()          # u(0) = 0 in both directions, no NaN
        assert np.abs(want).max() > 0


@pytest.mark.parametrize("name", ["reference_size", "mesh_1031"])
def test_two_runs_give_the_same_bits(name, gpu_lib):
    case, ref = _case(name)
    g = _g_dist(name, ref["dist"].shape)
    a, b = _autograd(case, g), _autograd(case, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    fa, fb = _forward(case), _forward(case)
    assert all(torch.equal(x, y) for x, y in zip(fa, fb))
    plain = _forward(case, want_idx=False)
    assert torch.equal(plain[0], fa[0]) and torch.equal(plain[1], fa[1])          # the values do not depend on whether the indices are asked for


def _ranked(dist64):
    order = np.argsort(dist64, axis=0, kind="stable")
    val = np.take_along_axis(dist64, order, 0)
    assert ((val[1:] - val[:-1]) > 1e-3 * val[1:]).all()          # the f32 ranking is determined
    return val, order


@functools.lru_cache(None)
def _sample():
    """a sample() output dict and its target from seeded tensors (no encoder): N = 5 hypotheses of B = 3 images, 64 object vertices"""
    N, B = 5, 3
    cj, cv = chamfer_ref.make_case(107, N, B, 21, 64), chamfer_ref.make_case(108, N, B, 778, 64)
    rng = np.random.default_rng(17)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    out = {"th_bt": f(N, B, 58), "logs_t": f(N, B, 3), "verts": cv["points"].reshape(N, B, -1), "xyz": cj["points"].reshape(N, B, -1),
           "uv": (128 + 30 * f(N, B, 42)).astype(np.float32), "log_p": f(B), "faces": rng.integers(0, 778, (1538, 3)), "image": f(B, 3, 8, 8)}
    tgt = chamfer_ref.target_of(cj)
    tgt.update(pose3d=f(B, 63), crop_uv=rng.uniform(-1, 1, (B, 42)).astype(np.float32), vis=(rng.uniform(0, 1, (B, 21)) < 0.7).astype(np.float32))
    d64 = {"xyz": chamfer_ref.chamfer64(cj["points"], cj["scale"], cj["root"], cj["obj"])["dist"],
           "verts": chamfer_ref.chamfer64(cv["points"], cj["scale"], cj["root"], cj["obj"])["dist"]}
    return out, tgt, d64


def test_criterion_chamfer_metrics(gpu_lib):
    out, tgt, d64 = _sample()
    o = {k: _cu(v) for k, v in out.items() if k in ("log_p", "xyz", "uv", "verts")}
    y = {k: _cu(v) for k, v in tgt.items()}
    tot0, _, m0 = criteria.MHEntLoss()(dict(o), y)
    tot1, _, m1 = criteria.MHEntChamferLoss()(dict(o), y)
    assert tuple(m0) == criteria.METRIC_KEYS and len(m0) == 14          # the flag off: exactly the existing keys
    assert set(m1) == set(m0) | {"chamfer_rgb_sample", "chamfer_rgb_sample_mean", "chamfer_rgb_select"}
    assert torch.equal(tot0, tot1) and all(torch.equal(m0[k], m1[k]) for k in m0)
    val, order = _ranked(d64["xyz"])
    assert_close(m1["chamfer_rgb_sample"].cpu().numpy(), val[0], RTOL, what="chamfer_rgb_sample")
    assert_close(m1["chamfer_rgb_sample_mean"].cpu().numpy(), d64["xyz"].mean(0), RTOL, what="chamfer_rgb_sample_mean")
    assert m1["chamfer_rgb_select"].dtype == torch.int64 and np.array_equal(m1["chamfer_rgb_select"].cpu().numpy(), order[0])
    # with the aligned evaluation the distance is still taken of the unaligned joints
    _, _, m2 = criteria.MHEntChamferLoss(aligned=True)(dict(o), y)
    assert all(torch.equal(m1[k], m2[k]) for k in ("chamfer_rgb_sample", "chamfer_rgb_sample_mean", "chamfer_rgb_select"))
    with pytest.raises(ValueError, match="object_verts"):
        criteria.MHEntChamferLoss()(dict(o), {k: v for k, v in y.items() if k != "object_verts"})


@pytest.mark.parametrize("Q,points", [(1, "xyz"), (3, "xyz"), (3, "verts")])
def test_chamfer_select(Q, points, gpu_lib):
    out, tgt, d64 = _sample()
    o = {k: (_cu(v) if k != "faces" else v) for k, v in out.items() if k != "log_p"}
    y = {k: _cu(v) for k, v in tgt.items()}
    sel = criteria.chamfer_select(o, y, Q=Q, points=points)
    val, order = _ranked(d64[points])
    assert set(sel) == set(o) | {"chamfer", "chamfer_index"}
    assert sel["faces"] is o["faces"] and sel["image"] is o["image"]
    assert sel["chamfer_index"].dtype == torch.int64 and np.array_equal(sel["chamfer_index"].cpu().numpy(), order[:Q])
    ch = sel["chamfer"].cpu().numpy()
    assert ch.shape == (Q, 3) and (np.diff(ch, axis=0) >= 0).all()
    assert_close(ch, val[:Q], RTOL, what="chamfer")
    for k in ("th_bt", "logs_t", "verts", "xyz", "uv"):
        assert np.array_equal(sel[k].cpu().numpy(), out[k][order[:Q], np.arange(3)]), k
