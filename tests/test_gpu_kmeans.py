"""GPU: the k-means quantisation of a hypothesis set (csrc/kmeans.hip) through ops.kmeans_select, criteria.kmeans_select and
MHEnt.sample(N=[M, n], quant='kmeans'), against the float64 restatement tests/kmeans_ref.py.

Where equality of the decisions (index, count, assign, converged) is demanded, the test first asserts from the reference alone that its
smallest decision margin is at least 1e-3 - three orders above the D * 2^-24 (4e-6 at D = 63) relative rounding of an f32 sum of D squares -
or the data are small integers with power-of-two cluster sizes, so that every f32 distance and mean is exact and the ties are real.  The
seeds of the planted cases were chosen on the CPU for that margin.  Random Gaussian data has margins below f32 rounding: there the properties
of a k-means fixed point are asserted instead, each recomputed in f64 from the kernel's outputs."""
import numpy as np
import pytest
import torch

import kmeans_ref
from mhentropy_amd import criteria, harness, ops, synth

pytestmark = pytest.mark.gpu
MARGIN = 1e-3
U = 2.0 ** -24          # unit roundoff of f32


def _run(pts, Q, score=None, iters=10):
    r = ops.kmeans_select(torch.as_tensor(pts).cuda(), Q, score=None if score is None else torch.as_tensor(score).cuda(), iters=iters)
    torch.cuda.synchronize()
    assert r["index"].dtype == torch.int64 and all(r[k].dtype == torch.int32 for k in ("count", "assign", "converged")) and r["centre"].dtype == torch.float32
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same_decisions(got, ref, what):
    for k in ("index", "count", "assign", "converged"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k, got[k].T.tolist(), ref[k].T.tolist())


def _planted_case(seed, N, B, D, Q, iters=10, min_sep=10.0):
    """a planted case whose reference margin is asserted first; the centres then agree with the f64 means to the rounding of a serial f32
    sum of at most N terms of the image's scale (N <= D in the issue's case: its D * 2^-24 bound)"""
    pts, score, centres = kmeans_ref.planted(seed, N, B, D, Q)
    sep = min(np.linalg.norm(centres[i, b] - centres[j, b]) for b in range(B) for i in range(Q) for j in range(i))
    assert sep >= min_sep, sep                                                # unit sigma: the planted centres lie at least 10 sigma apart
    ref = kmeans_ref.kmeans(pts, Q, score, iters)
    assert ref["margin"] >= MARGIN, ref["margin"]
    got = _run(pts, Q, score, iters)
    _same_decisions(got, ref, (seed, N, B, D, Q))
    tol = max(N, D) * U * np.abs(pts.astype(np.float64)).max((0, 2))          # [B]
    err = np.abs(got["centre"].astype(np.float64) - ref["centre"]).max((0, 2))
    print("kmeans planted N=%d B=%d D=%d Q=%d: margin %.3g, centre err %.3g (tol %.3g)" % (N, B, D, Q, ref["margin"], err.max(), tol.min()))
    assert (err <= tol).all(), (err, tol)
    return got, ref


def test_planted_clusters_match_the_reference_exactly(gpu_lib):
    got, ref = _planted_case(SEEDS[(37, 3, 63, 4)], 37, 3, 63, 4)
    assert (ref["converged"] == 1).all() and (ref["count"].sum(0) == 37).all()


# ---- exact arithmetic: small integers, power-of-two cluster sizes, real ties -----------------------------------------------------------
# The two empty-cluster cases have a cluster that is empty from the first assignment on (a seed drawn twice among duplicate rows): count 0,
# the centre kept, the nearest of all rows reported, last in the order.  A cluster that HAD members and loses them all in a later round was
# not found: after farthest-point seeding none of 600,000 random small-integer inputs emptied one in the reference (kmeans_ref's `emptied`).
EXACT = {
    # name: (rows [N][D], Q, score or None, iters)
    "duplicate rows": ([[0, 0], [0, 0], [4, 0], [4, 0], [0, 8], [0, 8], [0, 8], [0, 8]], 3, None, 10),
    "all rows equal: one seed twice, an empty cluster": ([[3, 3]] * 4, 2, None, 10),
    "a point equidistant from two centres": ([[0], [8], [4], [4], [0]], 2, None, 10),
    "two points equidistant from two centres": ([[0, 0], [8, 0], [4, 3], [4, -3], [0, 0], [8, 0]], 2, None, 10),
    "an empty cluster beside two live ones": ([[0, 0], [0, 0], [4, 0], [4, 0]], 3, None, 10),
    "two clusters of equal count": ([[10], [0], [2], [12]], 2, None, 10),
    "Q = 1": ([[1, 2], [3, 6], [5, 2], [7, 6]], 1, None, 10),
    "Q = N": ([[1, 2], [3, 6], [5, 2], [7, 6]], 4, None, 10),
    "N = 1": ([[5, 1, 7]], 1, None, 10),
    "iters = 0": ([[0], [8], [4], [4], [0]], 2, None, 0),
    "iters = 1": ([[0], [8], [4], [4], [0]], 2, None, 1),
    "iters = 2": ([[0], [8], [4], [4], [0]], 2, None, 2),
    "score given": ([[4], [0], [8], [8], [8]], 2, [0.0, 1.0, 5.0, 2.0, 2.0], 10),
    "a tie in score": ([[4], [0], [8]], 2, [1.0, 3.0, 3.0], 10),
    "score absent": ([[4], [0], [8]], 2, None, 10),
}


TIES = {"duplicate rows", "all rows equal: one seed twice, an empty cluster", "a point equidistant from two centres",
        "two points equidistant from two centres", "a tie in score", "an empty cluster beside two live ones"}


def _exact_reference(rows, Q, score, iters):
    pts = np.array(rows, np.float32)[:, None, :]
    sc = None if score is None else np.array(score, np.float32)[:, None]
    ref = kmeans_ref.kmeans(pts, Q, sc, iters)
    assert all(c & (c - 1) == 0 for c in ref["update_counts"]), ref["update_counts"]       # every mean is exact in f32 as well
    assert np.array_equal(ref["centre"].astype(np.float32).astype(np.float64), ref["centre"])
    return pts, sc, ref


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_arithmetic_and_tie_rules(gpu_lib, name):
    rows, Q, score, iters = EXACT[name]
    pts, sc, ref = _exact_reference(rows, Q, score, iters)
    got = _run(pts, Q, sc, iters)
    _same_decisions(got, ref, name)
    assert np.array_equal(got["centre"].astype(np.float64), ref["centre"]), (name, got["centre"].tolist(), ref["centre"].tolist())
    if name.startswith("iters = "):
        assert got["converged"][0] == (1 if iters >= 2 else 0)
    if name in TIES:
        assert ref["margin"] == 0.0
    if "empty" in name:
        assert ref["count"][-1, 0] == 0 and ref["index"][-1, 0] == 0


def test_two_images_of_one_batch_do_not_mix(gpu_lib):
    """two exact cases of one shape as the two images of a batch, with a tied score: each column is its own case's result"""
    a, b = np.array(EXACT["a point equidistant from two centres"][0], np.float32), np.array([[8], [0], [4], [4], [8]], np.float32)
    pts = np.stack([a, b], 1)
    sc = np.zeros((5, 2), np.float32)
    ref = kmeans_ref.kmeans(pts, 2, sc, 10)
    got = _run(pts, 2, sc, 10)
    _same_decisions(got, ref, "batch")
    assert np.array_equal(got["centre"].astype(np.float64), ref["centre"])


# ---- shapes -------------------------------------------------------------------------------------------------------------------------------
SEEDS = {(37, 3, 63, 4): 22, (50, 2, 1, 5): 26, (40, 2, 72, 4): 18, (12, 2, 2334, 3): 10, (200, 2, 63, 10): 24, (626, 1, 63, 3): 8}


@pytest.mark.parametrize("shape", [(50, 2, 1, 5), (40, 2, 72, 4), (200, 2, 63, 10)])
def test_shapes_match_the_reference(gpu_lib, shape):
    _planted_case(SEEDS[shape], *shape, min_sep=10.0 if shape[2] > 1 else 0.0)          # (on a line the clusters overlap: the margin is the guard)


def test_mesh_sized_rows_through_criteria(gpu_lib):
    """D = 2334 at small N, through criteria.kmeans_select(points='verts'): every (N, B, ...) tensor is cut at the representatives"""
    N, B, D, Q = 12, 2, 2334, 3
    pts, score, _ = kmeans_ref.planted(SEEDS[(N, B, D, Q)], N, B, D, Q)
    ref = kmeans_ref.kmeans(pts, Q, score, 10)
    assert ref["margin"] >= MARGIN, ref["margin"]
    verts = torch.as_tensor(pts).cuda()
    out = {"verts": verts.view(N, B, 778, 3), "log_q": torch.as_tensor(score).cuda().reshape(-1), "tag": torch.arange(N * B).view(N, B).cuda(),
           "faces": torch.zeros(5, 3), "image": torch.zeros(B, 3, 4, 4), "per_image": torch.zeros(B, 7)}
    sel = criteria.kmeans_select(out, Q, points="verts", score="log_q")
    assert set(sel) == set(out) | {"kmeans_index", "kmeans_count", "kmeans_assign", "kmeans_converged"}
    assert sel["kmeans_index"].dtype == sel["kmeans_count"].dtype == torch.int64
    assert np.array_equal(sel["kmeans_index"].cpu().numpy(), ref["index"]) and np.array_equal(sel["kmeans_count"].cpu().numpy(), ref["count"])
    assert np.array_equal(sel["kmeans_assign"].cpu().numpy(), ref["assign"]) and np.array_equal(sel["kmeans_converged"].cpu().numpy(), ref["converged"])
    cols = np.arange(B)
    assert tuple(sel["verts"].shape) == (Q, B, 778, 3) and np.array_equal(sel["verts"].cpu().numpy().reshape(Q, B, D), pts[ref["index"], cols])
    assert np.array_equal(sel["tag"].cpu().numpy(), ref["index"] * B + cols) and tuple(sel["log_q"].shape) == (N * B,)
    assert sel["faces"] is out["faces"] and sel["image"] is out["image"] and sel["per_image"] is out["per_image"]
    same = criteria.kmeans_select(out, Q, points="verts", score=out["log_q"].view(N, B))
    assert torch.equal(same["kmeans_index"], sel["kmeans_index"])


def _largest_n(Q, D):
    limit, n = 160 * 1024, 1
    while ops.kmeans_lds_bytes(n + 1, Q, D) <= limit:
        n += 1
    return n


def test_largest_shape_the_lds_admits_runs_and_one_above_is_refused(gpu_lib):
    Q, D = 3, 63
    N = _largest_n(Q, D)
    assert N == 626 and ops.kmeans_lds_bytes(N, Q, D) <= 160 * 1024 < ops.kmeans_lds_bytes(N + 1, Q, D)
    _planted_case(SEEDS[(N, 1, D, Q)], N, 1, D, Q)
    with pytest.raises(ValueError, match="LDS"):
        ops.kmeans_select(torch.zeros(N + 1, 1, D, device="cuda"), Q)



# ---- random Gaussian data: the properties of a fixed point ------------------------------------------------------------------------------
def test_random_gaussian_data_reaches_a_fixed_point(gpu_lib):
    N, B, D, Q = 200, 4, 63, 10
    rng = np.random.RandomState(5)
    pts = rng.randn(N, B, D).astype(np.float32)
    score = rng.randn(N, B).astype(np.float32)
    got = _run(pts, Q, score, iters=100)
    again = _run(pts, Q, score, iters=100)
    for k in got:
        assert np.array_equal(got[k].view(np.int32) if got[k].dtype == np.float32 else got[k], again[k].view(np.int32) if again[k].dtype == np.float32 else again[k]), k
    p64 = pts.astype(np.float64)
    for b in range(B):
        assert got["converged"][b] == 1
        c, a, idx, cnt = got["centre"][:, b].astype(np.float64), got["assign"][:, b], got["index"][:, b], got["count"][:, b]
        d = ((p64[:, b, None, :] - c[None]) ** 2).sum(-1)                       # [N, Q]
        own = d[np.arange(N), a]
        assert (own <= d.min(1) * (1 + 1e-5)).all()                             # every point sits with (one of) its nearest centre(s)
        assert cnt.sum() == N and (np.diff(cnt) <= 0).all() and len(set(idx.tolist())) == Q
        for q in range(Q):
            members = np.nonzero(a == q)[0]
            assert len(members) == cnt[q] > 0
            # a serial f32 sum of m terms is off by at most (m - 1) u sum|x|, the division adds one more u
            tol = (len(members) + 1) * U * np.abs(p64[members, b]).max()
            assert np.abs(c[q] - p64[members, b].mean(0)).max() <= tol
            assert idx[q] in members and own[idx[q]] <= own[members].min() * (1 + 1e-5)


# ---- through the model --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(gpu_lib):
    B, h, steps = 2, 64, 2          # the C0 configuration of smoke()
    sd = {"q_z_giv_i." + k: v for k, v in synth.flow_state(7, 45, 512, (h, h), steps).items()}
    sd.update(synth.head_state(7, 512, 512, 16))
    sd.update({"feat_extractor.res." + k: v for k, v in synth.resnet_state(7, "resnet18").items()})
    m = harness.build_mhent(backbone="resnet18", h_dims=(h, h), num_steps=steps, tables=synth.mano_tables(0))
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    x, yn = synth.batch(7, B, image_size=128)
    return m.cuda().eval(), torch.as_tensor(x).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}, B


def test_sample_quant_kmeans_is_kmeans_select_of_the_full_sample(model):
    m, x, y, B = model
    M, n, temp = 24, 4, 0.5
    noise = torch.as_tensor(synth.noise(11, M * B)).cuda()
    with torch.no_grad():
        feat = m.feat_extractor(x)[1]
        full = m.sample(x, N=M, temp=temp, noise=noise, feat=feat)
        _, log_q = m.q_z_giv_i.sample_with_log_prob(m._noise(M * B, temp, noise, feat.device), feat)
        want = criteria.kmeans_select(full, n, score=log_q.view(M, B))
        got = m.sample(x, N=[M, n], temp=temp, noise=noise, feat=feat, quant="kmeans")
        topk = m.sample(x, N=[M, n], temp=temp, noise=noise, feat=feat)
    assert set(got) == set(full) | {"quant_index", "quant_count"}
    assert set(topk) == set(full) == {"th_bt", "logs_t", "verts", "faces", "xyz", "uv"}            # without quant: the keys it always returned
    assert torch.equal(got["quant_index"], want["kmeans_index"]) and torch.equal(got["quant_count"], want["kmeans_count"])
    assert got["quant_index"].dtype == got["quant_count"].dtype == torch.int64 and tuple(got["quant_index"].shape) == (n, B)
    assert int(got["quant_count"].sum()) == M * B
    assert torch.equal(got["th_bt"], want["th_bt"]) and torch.equal(got["logs_t"], want["logs_t"])
    for k in ("xyz", "uv", "verts"):
        assert got[k].shape == want[k].shape
        a, b = got[k].double(), want[k].double()
        print("sample(quant='kmeans') %s: bit-identical %s, max rel diff %.3g" % (k, torch.equal(got[k], want[k]), float((a - b).abs().max() / b.abs().max())))
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), k
    assert not torch.equal(got["th_bt"], topk["th_bt"])                                             # (the modes are not the n most likely rows)
    same = m.sample(x, N=[M, M], temp=temp, noise=noise, feat=feat, quant="kmeans")                 # n == M: quant is ignored, as N_quant is
    assert set(same) == set(full) and torch.equal(same["th_bt"], full["th_bt"])


def test_criterion_on_the_cut_output_is_quantised_best_of_m(model):
    m, x, y, B = model
    M, n = 24, 4
    noise = torch.as_tensor(synth.noise(12, M * B)).cuda()
    with torch.no_grad():
        out = m.sample(x, N=[M, n], temp=0.8, noise=noise, quant="kmeans")
        full = m.sample(x, N=M, temp=0.8, noise=noise)
        crit = criteria.MHEntLoss()
        _, _, mq = crit(dict(out, log_p=torch.zeros(B, device="cuda")), y)
        _, _, mf = crit(dict(full, log_p=torch.zeros(B, device="cuda")), y)
    assert set(mq) == set(criteria.METRIC_KEYS) and len(mq) == 14
    for k, v in mq.items():
        assert tuple(v.shape) == (B,) and bool(torch.isfinite(v).all()), k
    # the n kept hypotheses are among the M: their best error cannot beat the best of all M
    assert bool((mq["eucLoss_3d_rgb_sample"] >= mf["eucLoss_3d_rgb_sample"] * (1 - 1e-6)).all())
