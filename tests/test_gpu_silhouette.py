"""GPU tests of the silhouette distance: mhe_silhouette_pixels / mhe_silhouette_dist_f32 / mhe_silhouette_dist_bwd_f32 (csrc/silhouette.hip)
through ops.silhouette_*, criteria.silhouette_dist (a torch.autograd.Function) and criteria.silhouette_select.  Everything against the float64
restatement of tests/silhouette_ref.py, computed once per case and shared.

Bounds (silhouette_ref.FWD_RTOL / REV_RTOL, relative to the reference's largest value): four times what the restatement evaluated in f32 on the
CPU deviates from f64 on these very inputs - measured, not chosen; the figures are in silhouette_ref.py and DESIGN.md, and
tests/test_silhouette_host.py re-measures them.  The pixel list is compared bit for bit.  Indices: every index the kernel returns must attain
the f64 minimum up to FWD_RTOL, and at most 1 % of the entries may differ from the f64 argmin.

Shapes (silhouette_ref.CASES): S in {8, 64}; V in {1, 5, 64, 65, 778} (one thread slot, a wave, a wave and one, all four slots of the 256
threads); N B in {1, 3, 35}; 4,096 kept pixels (the full mask: four rounds of the cover direction, the whole LDS list); vertices partly outside
the image, all inside the mask; a NaN vertex beside clean rows; an image with an empty mask beside others."""
import functools

import numpy as np
import pytest
import torch

import silhouette_ref as sr
from mhentropy_amd import criteria, ops

pytestmark = pytest.mark.gpu


def _cu(a):
    return torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared case arrays are read-only)


# ---- pixel list -------------------------------------------------------------------------------------------------------------------------------
KINDS = ("blob", "empty", "corner", "full", "borders")


@pytest.mark.parametrize("S,k,as_float", [(8, 1, False), (8, 2, True), (64, 1, True), (64, 2, False), (5, 2, False), (64, 4, False)])
def test_pixel_list_equals_the_restatement_bit_for_bit(S, k, as_float, gpu_lib):
    rng = np.random.default_rng(S * 10 + k)
    H = S * k
    batch = np.concatenate([sr.blob_mask(rng, 1, H, kind, k) for kind in KINDS])          # B = 5: one image of every kind
    noisy = rng.uniform(0, 1, (1, H, H)) < 0.5                                           # B = 1: box means on both sides of 0.5, many at it
    for mask in (batch, noisy):
        if as_float:
            mask = (mask * rng.choice([0.25, 0.5, 0.75, 1.0], mask.shape)).astype(np.float32)          # exact box sums
        want_p, want_c = sr.pixel_list(mask, S)
        pixels, count = ops.silhouette_pixels(_cu(mask), S)
        assert pixels.dtype == torch.int32 and count.dtype == torch.int32 and tuple(pixels.shape) == (mask.shape[0], S * S)
        assert np.array_equal(count.cpu().numpy(), want_c), (count.cpu().numpy(), want_c)
        assert np.array_equal(pixels.cpu().numpy(), want_p)
        if mask.shape[0] == 5 and not as_float:
            assert want_c[1] == 0 and want_c[3] == S * S and want_c[2] == 1 and want_p[2, 0] == S - 1          # empty, full, the corner (0, S-1)
            i, j = want_p[4, :want_c[4]] >> 16, want_p[4, :want_c[4]] & 0xffff
            assert i.min() == 0 and j.min() == 0 and i.max() == S - 1 and j.max() == S - 1          # all four borders
    if not as_float:
        as_u8, _ = ops.silhouette_pixels(_cu(batch.astype(np.uint8) * 255), S)          # a byte other than 0 counts as 1
        assert np.array_equal(as_u8.cpu().numpy(), sr.pixel_list(batch, S)[0])


# ---- forward ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _forward(name):
    case, ref = sr.reference(name)
    S = sr.CASES[name]["S"]
    pixels, count = ops.silhouette_pixels(_cu(case["mask"]), S)
    out = ops.silhouette_dist(_cu(case["verts"]), _cu(case["logs_t"]), pixels, count, want_idx=True)
    torch.cuda.synchronize()
    return (pixels, count) + tuple(out)


def _check_forward(name):
    case, ref = sr.reference(name)
    pixels, count, dist, parts, idx_v, idx_m = (t.cpu().numpy() for t in _forward(name))
    assert np.array_equal(pixels, ref["pixels"]) and np.array_equal(count, ref["count"])
    devs = [sr.rel_dev(a, ref[k]) for a, k in ((dist, "dist"), (parts[..., 0], "inside"), (parts[..., 1], "cover"))]
    share, excess = sr.index_report(name, idx_v, idx_m)
    print(f"{name}: dist / inside / cover deviation {devs[0]:.3e} {devs[1]:.3e} {devs[2]:.3e} (bound {sr.FWD_RTOL:.3e}); indices: {share:.5f} differ, "
          f"excess {excess:.3e}")
    assert max(devs) <= sr.FWD_RTOL, (name, devs)
    assert excess <= sr.FWD_RTOL and share <= sr.MISMATCH_CAP, (name, share, excess)
    for b in range(count.shape[0]):          # the list's tail and the empty image
        assert (idx_m[:, b, count[b]:] == -1).all()
        if count[b] == 0:
            assert (dist[:, b] == 0).all() and (parts[:, b] == 0).all() and (idx_v[:, b] == -1).all()
    return case, ref, dist, idx_v, idx_m


@pytest.mark.parametrize("name", list(sr.CASES))
def test_forward_parity(name, gpu_lib):
    case, ref, dist, _, _ = _check_forward(name)
    nan_row = sr.CASES[name].get("nan_row")
    if nan_row is not None:
        assert np.isnan(dist[nan_row]) and np.isnan(dist).sum() == 1          # that row, and no other
    if sr.CASES[name].get("inside_only"):
        assert (ref["inside"] == 0).all()


def test_ties_go_to_the_lowest_index(gpu_lib):
    """exact ties from coordinates that are multiples of 1/8 under the camera s = 1, t = 0: every distance is exact in f32 and in f64"""
    S = 8
    mask = np.zeros((1, S, S), bool)
    mask[0, 2, 2] = mask[0, 2, 5] = True          # centres (-0.375, -0.375) and (0.375, -0.375)
    one = np.array([[0, -0.375, 0], [0, 0.5, 1], [-0.375, -0.125, 2], [-0.375, -0.625, 3], [-0.375, -0.125, 4], [0.375, -0.375, 5]], np.float32)
    verts = np.stack([one, one[::-1]])[:, None]          # (2, 1, 6, 3): the second hypothesis lists the vertices in reverse
    logs_t = np.zeros((2, 1, 3), np.float32)
    ref = sr.silhouette(verts, logs_t, mask, S)
    assert ref["idx_v"][0, 0].tolist() == [0, 0, 0, 0, 0, 1] and ref["idx_m"][0, 0, :2].tolist() == [2, 5]          # vertices 0, 1: midway between the two squares
    assert ref["idx_v"][1, 0].tolist() == [1, 0, 0, 0, 0, 0] and ref["idx_m"][1, 0, :2].tolist() == [1, 0]          # pixel 0: vertices 1, 2, 3 at 0.25
    assert ref["d_v"][0, 0, 0] == 0.25 and ref["d_m"][0, 0, 0] == 0.25 and ref["d_m"][0, 0, 1] == 0
    pixels, count = ops.silhouette_pixels(_cu(mask), S)
    dist, parts, idx_v, idx_m = ops.silhouette_dist(_cu(verts), _cu(logs_t), pixels, count, want_idx=True)
    assert np.array_equal(idx_v.cpu().numpy(), ref["idx_v"]) and np.array_equal(idx_m.cpu().numpy(), ref["idx_m"])
    assert sr.rel_dev(dist.cpu().numpy(), ref["dist"]) <= sr.FWD_RTOL
    # the reverse at the ties: finite, the vertex ON a centre takes no direction from it, and the restatement's gradient at these indices
    g = np.array([[1.0], [-0.5]], np.float32)
    gv, gl = ops.silhouette_dist_bwd(_cu(verts), _cu(logs_t), pixels, count, idx_v, idx_m, _cu(g))
    want_v, want_l = sr.grad(verts, logs_t, mask, S, g, (ref["idx_v"], ref["idx_m"]))
    assert torch.isfinite(gv).all() and torch.isfinite(gl).all() and (gv[0, 0, 5] == 0).all() and (want_v[0, 0, 5] == 0).all()
    assert sr.rel_dev(gv.cpu().numpy(), want_v) <= sr.FWD_RTOL and sr.rel_dev(gl.cpu().numpy(), want_l) <= sr.FWD_RTOL


# ---- reverse ----------------------------------------------------------------------------------------------------------------------------------
def _autograd(name, parts=False):
    case, ref = sr.reference(name)
    v, lt = _cu(case["verts"]).requires_grad_(True), _cu(case["logs_t"]).requires_grad_(True)
    out = criteria.silhouette_dist(v, lt, _cu(case["mask"]), size=sr.CASES[name]["S"], parts=parts)
    dist = out[0] if parts else out
    assert dist.requires_grad
    gv, gl = torch.autograd.grad(dist, (v, lt), _cu(sr.g_dist_of(name, ref["dist"].shape)))
    torch.cuda.synchronize()
    return out, gv, gl


@pytest.mark.parametrize("name", list(sr.CASES))
def test_reverse_parity(name, gpu_lib):
    case, ref, dist, idx_v, idx_m = _check_forward(name)          # the kernel's own indices, verified
    out, gv, gl = _autograd(name, parts=True)
    assert np.array_equal(out[0].detach().cpu().numpy(), dist, equal_nan=True)          # with and without parts, through autograd: the same bits
    assert not out[1].requires_grad and not out[2].requires_grad and tuple(out[0].shape) == ref["dist"].shape
    g = sr.g_dist_of(name, ref["dist"].shape)
    want_v, want_l = sr.grad(case["verts"], case["logs_t"], case["mask"], sr.CASES[name]["S"], g, (np.maximum(idx_v, 0), np.maximum(idx_m, 0)))
    gv, gl = gv.cpu().numpy().reshape(want_v.shape), gl.cpu().numpy()
    dv, dl = sr.rel_dev(gv, want_v), sr.rel_dev(gl, want_l)
    print(f"{name}: g_verts deviation {dv:.3e} of {np.abs(want_v).max():.3e}, g_logs_t {dl:.3e} of {np.abs(want_l).max():.3e} (bound {sr.REV_RTOL[name]:.3e})")
    assert np.isfinite(gv).all() and np.isfinite(gl).all() and (gv[..., 2] == 0).all()
    assert max(dv, dl) <= sr.REV_RTOL[name]
    assert np.abs(want_v).max() > 0 and np.abs(want_l).max() > 0
    nan_row, empty = sr.CASES[name].get("nan_row"), sr.CASES[name].get("empty_image")
    if nan_row is not None:
        assert (gv[nan_row] == 0).all() and (gl[nan_row] == 0).all()
    if empty is not None:
        assert (gv[:, empty] == 0).all() and (gl[:, empty] == 0).all()
    valid = idx_m[idx_m >= 0]
    if sr.CASES[name]["V"] > 1 and sr.CASES[name]["S"] == 64:
        assert np.bincount(valid).max() >= 2          # several pixels share a nearest vertex: the reverse's gather adds more than one term


@pytest.mark.parametrize("name", ["v65_s8_35_rows", "v778_s64_35_rows"])
def test_two_runs_give_the_same_bits(name, gpu_lib):
    (a, ga, la), (b, gb, lb) = _autograd(name), _autograd(name)
    assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()) and torch.equal(ga, gb) and torch.equal(la, lb)
    case, ref = sr.reference(name)
    first = _forward(name)
    pixels, count = ops.silhouette_pixels(_cu(case["mask"]), sr.CASES[name]["S"])
    again = ops.silhouette_dist(_cu(case["verts"]), _cu(case["logs_t"]), pixels, count, want_idx=True)
    plain = ops.silhouette_dist(_cu(case["verts"]), _cu(case["logs_t"]), pixels, count)
    for x, y in zip(first, (pixels, count) + tuple(again)):
        assert torch.equal(x.nan_to_num(), y.nan_to_num()) if x.is_floating_point() else torch.equal(x, y)
    # the values do not depend on whether the indices are asked for
    assert torch.equal(plain[0].nan_to_num(), again[0].nan_to_num()) and torch.equal(plain[1].nan_to_num(), again[1].nan_to_num())


def test_runs_inside_a_captured_hip_graph(gpu_lib):
    """pixel list, forward and reverse captured into one HIP graph: nothing on the host reads the count.  The replay equals eager bit for bit,
    also after the static mask was overwritten with another one (other counts)"""
    name = "v65_s8_35_rows"
    case, ref = sr.reference(name)
    S = sr.CASES[name]["S"]
    v, lt, g = _cu(case["verts"]), _cu(case["logs_t"]), _cu(sr.g_dist_of(name, ref["dist"].shape))
    mask = _cu(case["mask"])
    other = torch.roll(mask, 2, 0) | torch.roll(mask, 1, 2)          # image 3 is no longer empty

    def run():
        pixels, count = ops.silhouette_pixels(mask, S)
        dist, parts, idx_v, idx_m = ops.silhouette_dist(v, lt, pixels, count, want_idx=True)
        gv, gl = ops.silhouette_dist_bwd(v, lt, pixels, count, idx_v, idx_m, g)
        return count, dist, parts, idx_v, idx_m, gv, gl, criteria.silhouette_dist(v, lt, mask, size=S)
    eager = [t.clone() for t in run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    same = lambda x, y: torch.equal(x.nan_to_num(), y.nan_to_num()) if x.is_floating_point() else torch.equal(x, y)
    graph.replay()
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(static, eager))
    assert same(static[1], static[7])
    mask.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in static]
    eager = run()
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(replayed, eager))
    assert not torch.equal(replayed[0].cpu(), torch.as_tensor(ref["count"])) and int(replayed[0][3]) > 0


# ---- the public surface -----------------------------------------------------------------------------------------------------------------------
def test_fitting_the_camera_to_a_rendered_mask_lowers_the_distance(gpu_lib):
    """the use the gradient is for: the mask is ManoLayer.render's of a mesh under a camera; from a perturbed camera, Adam on logs_t alone,
    through criteria.silhouette_dist, brings the distance down"""
    from mhentropy_amd import synth
    from mhentropy_amd.ManoLayer import ManoLayer
    layer = ManoLayer(skeidx="RHD", use_pca=True, ncomps=45, mask_sz=64, tables=synth.mano_tables(0)).cuda()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        mesh = layer(beta=torch.zeros(1, 10).cuda(), theta=(0.1 * torch.randn(1, 48, generator=gen)).cuda())["mesh"].reshape(1, 778, 3)
        mesh = mesh - mesh.mean(1, keepdim=True)
        verts = (0.5 * mesh / mesh[..., :2].abs().max()).contiguous()          # normalised: within +-0.5 around the origin
        true = torch.tensor([[[0.3, 0.1, -0.05]]]).cuda()
        mask = layer.render(true[0, :, :1].exp(), true[0, :, 1:], vertex=verts, norm=torch.ones(1).cuda())["mask"]          # (1, 64, 64) in [0, 1]
    assert int((mask >= 0.5).sum()) >= 50, "the rendered mask is too small to fit anything to"
    at_truth = float(criteria.silhouette_dist(verts[None], true, mask))
    logs_t = (true + torch.tensor([0.25, 0.15, -0.12]).cuda()).requires_grad_(True)
    opt = torch.optim.Adam([logs_t], lr=0.01)
    trace = []
    for _ in range(60):
        opt.zero_grad()
        d = criteria.silhouette_dist(verts[None], logs_t, mask).sum()
        d.backward()
        opt.step()
        trace.append(float(d.detach()))
    print(f"distance at the true camera {at_truth:.4f}; from the perturbed one {trace[0]:.4f} -> {trace[-1]:.4f} in {len(trace)} steps")
    # 60 steps of at most ~0.01 each can undo the perturbation (0.25, 0.15, 0.12); in f64 on the CPU, with an elliptic point cloud, the same
    # loop goes 0.076 -> 0.017, the true camera's own distance
    assert trace[0] > at_truth and trace[-1] < 0.7 * trace[0]


@functools.lru_cache(None)
def _sample():
    """a sample() output dict and its target from seeded tensors (no encoder): N = 5 hypotheses of B = 3 images"""
    case = sr.make_case(seed=231, N=5, B=3, V=65, S=8, k=2)
    N, B = 5, 3
    rng = np.random.default_rng(23)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    out = {"th_bt": f(N, B, 58), "logs_t": np.array(case["logs_t"]), "verts": case["verts"].reshape(N, B, -1), "xyz": f(N, B, 63), "uv": f(N, B, 42),
           "faces": rng.integers(0, 65, (20, 3)), "image": f(B, 3, 8, 8)}
    d64 = sr.silhouette(case["verts"], case["logs_t"], case["mask"], 8)["dist"]
    return out, {"hand_mask": np.array(case["mask"])}, d64


@pytest.mark.parametrize("Q", [1, 5])
def test_silhouette_select(Q, gpu_lib):
    out, tgt, d64 = _sample()
    order = np.argsort(d64, axis=0, kind="stable")
    val = np.take_along_axis(d64, order, 0)
    assert ((val[1:] - val[:-1]) > 1e-4 * val[1:]).all()          # the f32 ranking is determined
    o = {k: (_cu(v) if k != "faces" else v) for k, v in out.items()}
    y = {k: _cu(v) for k, v in tgt.items()}
    sel = criteria.silhouette_select(o, y, Q=Q, size=8)
    assert set(sel) == set(o) | {"silhouette", "silhouette_index"}
    assert sel["faces"] is o["faces"] and sel["image"] is o["image"]
    assert sel["silhouette_index"].dtype == torch.int64 and np.array_equal(sel["silhouette_index"].cpu().numpy(), order[:Q])
    got = sel["silhouette"].cpu().numpy()
    assert got.shape == (Q, 3) and (np.diff(got, axis=0) >= 0).all() and sr.rel_dev(got, val[:Q]) <= sr.FWD_RTOL
    for k in ("th_bt", "logs_t", "verts", "xyz", "uv"):
        assert np.array_equal(sel[k].cpu().numpy(), out[k][order[:Q], np.arange(3)]), k
    # the selection it shares its cutting code with is untouched by it
    assert "chamfer" not in sel and "chamfer_index" not in sel
