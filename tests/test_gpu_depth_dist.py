"""GPU tests of the depth distance: mhe_depth_dist_f32 / mhe_depth_dist_bwd_f32 (csrc/depth_dist.hip) through ops.depth_dist / depth_dist_bwd,
criteria.depth_dist (a torch.autograd.Function) and criteria.depth_select.  Everything against the float64 restatement of tests/depth_ref.py,
computed once per (case, offset mode) and shared.

Cases (depth_ref.CASES): V = 3, F = 1 at S = 8; one face above render.hip's workgroup-list threshold with eight small ones at S = 64 (H = S) and
S = 16 (H = 4 S), (N, B) = (3, 2), rows partly off the image; a random mesh of V = 30, F = 50 with a face whose index lies outside [0, V) and a
zero-area face at S = 16 (H = 64) and S = 8; an image without observation, a mesh beside the mask and a NaN vertex row beside clean rows; every
residual beyond trunc; and one MANO-sized mesh (V = 778, F = 1,538) at S = 64, (N, B) = (2, 2).  Both offset modes everywhere.

Bounds are not fixed numbers: depth_ref derives them per element from the arithmetic (its docstring has the derivation) - one f32 rounding of
the projected coordinates, DELTA = 6e-5 sample units, carried through the plane slopes to R(p) and through |grad lam_k| to the barycentric
weights, plus U = 2^-24 per f32 rounding on the way (the kernel's sums are f64, so the S^2-term accumulation adds no more than the final
rounding).  Every comparison goes through edge_measure.Measure, which prints the largest |diff| / bound; no element is left out."""
import functools

import numpy as np
import pytest
import torch

import depth_ref as dr
from edge_measure import Measure
from mhentropy_amd import criteria, ops

pytestmark = pytest.mark.gpu
U = dr.U


def _cu(a):
    return torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared case arrays are read-only)


def _operands(op, root):
    return (_cu(op["verts"]), _cu(op["faces"]), _cu(op["logs_t"]), _cu(op["zscale"]), _cu(op["obs"]), _cu(op["root_z"]) if root else None)


@functools.lru_cache(None)
def _run(name, root):
    """the kernel's outputs for a case, as numpy: dist, parts, face_img, resid_img, g_verts, g_logs_t"""
    op, _ = dr.case(name, root)
    v, f, lt, zs, obs, rz = _operands(op, root)
    dist, parts, face_img, resid_img = ops.depth_dist(v, f, lt, zs, obs, rz, dr.TRUNC, want_images=True)
    plain, plain_parts = ops.depth_dist(v, f, lt, zs, obs, rz, dr.TRUNC)
    assert torch.equal(plain.view(torch.int32), dist.view(torch.int32)) and torch.equal(plain_parts.view(torch.int32), parts.view(torch.int32))
    g_verts, g_logs_t = ops.depth_dist_bwd(v, f, lt, zs, obs, rz, dr.TRUNC, _cu(op["g_dist"]))
    return {k: t.cpu().numpy() for k, t in (("dist", dist), ("parts", parts), ("face_img", face_img), ("resid_img", resid_img),
                                            ("g_verts", g_verts), ("g_logs_t", g_logs_t))}


def _images(m, tag, got, ref, skip=None, resid=True):
    """the two per-sample images against the reference; NaN patterns must agree (a NaN row, samples outside P).  skip [N,B,S,S]: samples that
    are not compared (the MANO-sized case's ambiguous ones); resid=False: the face image alone"""
    keep = np.ones(ref["face_img"].shape, bool) if skip is None else ~skip
    assert np.array_equal(got["face_img"][keep], ref["face_img"][keep]), (tag, int((got["face_img"] != ref["face_img"])[keep].sum()))
    if not resid:
        return
    nan = np.isnan(ref["resid_img"])
    assert np.array_equal(np.isnan(got["resid_img"])[keep], nan[keep]), tag
    ok = keep & ~nan
    m.add(tag + " resid", got["resid_img"][ok], ref["resid_img"][ok], ref["b_resid"][ok])


def _scalars(m, tag, got, ref):
    """dist, parts and the two gradients under their derived bounds; a NaN row is NaN in dist and parts and zero in the gradients"""
    bad = np.isnan(ref["dist"])
    assert np.array_equal(np.isnan(got["dist"]), bad) and np.array_equal(np.isnan(got["parts"]), np.isnan(ref["parts"])), tag
    z = lambda a: np.where(np.isnan(a), 0.0, a)
    m.add(tag + " dist", z(got["dist"]), z(ref["dist"]), ref["b_dist"] + 2 * U * dr.TRUNC)
    m.add(tag + " parts", z(got["parts"]), z(ref["parts"]), np.stack([np.full(bad.shape, 2 * U), ref["b_offset"], np.full(bad.shape, 2 * U)], -1))
    m.add(tag + " g_verts", got["g_verts"], ref["g_verts"], ref["b_g_verts"])
    m.add(tag + " g_logs_t", got["g_logs_t"], ref["g_logs_t"], ref["b_g_logs_t"])
    assert (z(got["dist"]) >= 0).all() and (z(got["dist"]) <= dr.TRUNC * (1 + 2 * U)).all()
    assert (got["g_verts"][bad] == 0).all() and (got["g_logs_t"][bad] == 0).all()


@pytest.mark.parametrize("root", [False, True], ids=["fitted", "given"])
@pytest.mark.parametrize("name", dr.EXACT)
def test_exact_parity_with_the_f64_restatement(name, root, gpu_lib):
    """the reference has ZERO ambiguous and zero fragile samples here (asserted on the reference alone), so the face image must be equal and
    every value lies within the bound depth_ref derives for it: b_resid = 2 DELTA (|gx| + |gy|) + 4 U max|D| of the winning face (+ the mean
    of the same over P when the offset is fitted, + the f32 rounding of e), b_dist = sum_P b_resid / |O| (min(|e|, trunc) is 1-Lipschitz),
    b_offset, and the gradient bounds accumulated term by term as depth_ref's docstring derives them.  The largest observed ratio is recorded
    in DESIGN.md."""
    op, ref = dr.case(name, root)
    assert not ref["ambiguous"].any() and ref["fragile"].sum() == 0
    got = _run(name, root)
    m = Measure("depth_dist", "depth-parity")
    _images(m, name, got, ref)
    _scalars(m, name, got, ref)
    m.report()
    if name == "edges_8":
        assert (got["dist"][:, 1] == 0).all() and (got["g_verts"][:, 1] == 0).all() and (got["parts"][:, 1, 0] == 0).all()          # O empty
        assert got["parts"][1, 0, 0] == 0 and (got["g_verts"][1, 0] == 0).all() and abs(got["dist"][1, 0] - dr.TRUNC) < 1e-8          # P empty
        assert np.isnan(got["dist"][2, 0]) and (got["face_img"][2, 0] == -1).all() and np.isfinite(got["dist"][2, 1])               # the NaN row alone
    if name == "far_8" and root:
        assert (got["parts"][..., 2] == 0).all() and (got["g_verts"] == 0).all() and (got["g_logs_t"] == 0).all()
    if name in ("mix_64", "mix_16_h64"):
        assert (ref["face_img"] == 0).sum() >= 64 * ref["face_img"].shape[0]          # the big face went through the workgroup's list
    if name.startswith("random"):
        assert not (ref["face_img"] == 7).any() and not (ref["face_img"] == 19).any()          # the out-of-range and the zero-area face


@pytest.mark.parametrize("root", [False, True], ids=["fitted", "given"])
def test_mano_sized_case(root, gpu_lib):
    """V = 778, F = 1,538 at S = 64, (N, B) = (2, 2): the tables' full loops (four faces and two vertices per thread).  Ambiguous samples are
    allowed up to CAP (asserted on the reference alone); the per-sample images are compared outside them; dist within (ambiguous count x trunc)
    / |O| plus the rounding bound; the GRADIENT (and with it the parts, and dist once more under the rounding bound alone) is compared against
    the reference evaluated WITH THE KERNEL'S FACE IMAGE AT THE AMBIGUOUS SAMPLES ONLY - everywhere else the reference keeps its own faces."""
    op, ref = dr.case("mano_64", root)
    assert ref["ambiguous"].mean() <= dr.CAP
    got = _run("mano_64", root)
    m = Measure("depth_dist", "depth-parity-mano")
    # (with the fitted offset every residual moves with the faces chosen at the ambiguous samples: those residuals are compared below)
    _images(m, "mano_64", got, ref, skip=ref["ambiguous"], resid=root)
    slack = ref["ambiguous"].sum((2, 3)) * dr.TRUNC / np.maximum(ref["n_obs"], 1)
    m.add("mano_64 dist (own faces)", got["dist"], ref["dist"], ref["b_dist"] + slack + 2 * U * dr.TRUNC)
    ref2 = dr.depth_dist64(op["verts"], op["faces"], op["logs_t"], op["zscale"], op["obs"], op["root_z"] if root else None, dr.TRUNC, op["g_dist"],
                           face_override=got["face_img"])
    assert np.array_equal(ref2["face_img"], got["face_img"])
    assert ref2["fragile"].sum() == 0, "a residual of the MANO-sized case lies within its bound of 0 or trunc: choose another seed"
    _images(m, "mano_64 (kernel's faces at the ambiguous samples)", got, ref2)
    _scalars(m, "mano_64 (kernel's faces at the ambiguous samples)", got, ref2)
    m.report()
    assert np.abs(got["g_verts"]).max() > 0 and (ref["parts"][..., 0] > 0.1).all()


def test_forward_and_reverse_are_bit_reproducible(gpu_lib):
    """two calls give equal bits, and the reverse's bits of a row do not depend on where the row stands in the batch"""
    for name, root in (("mix_64", False), ("mano_64", True)):
        op, _ = dr.case(name, root)
        v, f, lt, zs, obs, rz = _operands(op, root)
        g = _cu(op["g_dist"])
        bits = lambda t: t.view(torch.int32)
        a, b = ops.depth_dist(v, f, lt, zs, obs, rz, dr.TRUNC), ops.depth_dist(v, f, lt, zs, obs, rz, dr.TRUNC)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
        ga, gb = ops.depth_dist_bwd(v, f, lt, zs, obs, rz, dr.TRUNC, g), ops.depth_dist_bwd(v, f, lt, zs, obs, rz, dr.TRUNC, g)
        assert torch.equal(bits(ga[0]), bits(gb[0])) and torch.equal(bits(ga[1]), bits(gb[1]))
        perm = torch.arange(v.shape[0] - 1, -1, -1).cuda()          # the hypotheses reversed: every row moves to another workgroup
        gp = ops.depth_dist_bwd(v[perm].contiguous(), f, lt[perm].contiguous(), zs, obs, rz, dr.TRUNC, g[perm].contiguous())
        assert torch.equal(bits(gp[0]), bits(ga[0][perm])) and torch.equal(bits(gp[1]), bits(ga[1][perm]))
        dp = ops.depth_dist(v[perm].contiguous(), f, lt[perm].contiguous(), zs, obs, rz, dr.TRUNC)[0]
        assert torch.equal(bits(dp), bits(a[0][perm]))


@pytest.mark.parametrize("root", [False, True], ids=["fitted", "given"])
def test_autograd_equals_the_reverse_entry(root, gpu_lib):
    op, ref = dr.case("mix_16_h64", root)
    got = _run("mix_16_h64", root)
    v, f, lt, zs, obs, rz = _operands(op, root)
    v.requires_grad_(True); lt.requires_grad_(True)
    depth, mask = _cu(op["depth"]), _cu(op["hand_mask"])
    assert torch.equal(ops.depth_obs(depth, mask, 16), obs)          # H = 64 -> S = 16 on the device, the numpy rule's bits
    dist, overlap, offset, inliers = criteria.depth_dist(v, lt, f.long(), depth, mask, zs, root_z=rz, size=16, trunc=dr.TRUNC, parts=True)
    assert np.array_equal(dist.detach().cpu().numpy(), got["dist"]) and not overlap.requires_grad and not offset.requires_grad
    assert np.array_equal(torch.stack([overlap, offset, inliers], -1).cpu().numpy(), got["parts"])
    (dist * _cu(op["g_dist"])).sum().backward()
    assert np.array_equal(v.grad.cpu().numpy(), got["g_verts"]) and np.array_equal(lt.grad.cpu().numpy(), got["g_logs_t"])
    assert depth.grad is None and zs.grad is None


def test_gradient_reaches_z_through_the_mano_layer(gpu_lib):
    from mhentropy_amd import synth
    from mhentropy_amd.ManoLayer import ManoLayer
    layer = ManoLayer(skeidx="RHD", flat_hand_mean=False, ncomps=45, use_pca=True, tables=synth.mano_tables(0)).cuda()
    gen = torch.Generator().manual_seed(11)
    z = (0.2 * torch.randn(2, 61, generator=gen)).cuda().requires_grad_(True)
    verts = layer.verts(z)                                        # (2, 778, 3), normalised
    lt = torch.tensor([[[-1.0, 0.0, 0.0]], [[-1.1, 0.05, 0.0]]]).cuda()          # (N, B) = (2, 1)
    depth = torch.full((1, 64, 64), 0.5).cuda()
    mask = torch.ones(1, 64, 64, dtype=torch.bool).cuda()
    dist, overlap, _, _ = criteria.depth_dist(verts.view(2, 1, 778, 3), lt, layer.mano_layer.faces_i32, depth, mask, torch.full((1,), 0.1).cuda(), parts=True)
    assert (overlap > 0.01).all(), overlap
    dist.sum().backward()
    assert z.grad is not None and torch.isfinite(z.grad).all() and float(z.grad[:, :58].abs().max()) > 0 and float(z.grad[:, 58:].abs().max()) == 0


@functools.lru_cache(None)
def _sample():
    """a sample() output dict and its target built from seeded tensors (no encoder): N = 5 hypotheses of B = 2 images; hypothesis 3 is the mesh
    the depth image was rendered from"""
    rng = np.random.default_rng(41)
    v1, faces = dr._big_and_small(np.random.default_rng(5))
    N, B, S = 5, 2, 16
    verts = (v1[None, None] + rng.normal(0, 0.05, (N, B) + v1.shape)).astype(np.float32)
    logs_t = np.concatenate([rng.uniform(-0.1, 0.1, (N, B, 1)), rng.uniform(-0.05, 0.05, (N, B, 2))], 2).astype(np.float32)
    scale, root = np.array([0.09, 0.08], np.float32), np.array([[0.0, 0.0, 0.55], [0.0, 0.0, 0.6]], np.float32)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    out = {"th_bt": f(N, B, 58), "logs_t": logs_t, "verts": verts.reshape(N, B, -1), "xyz": f(N, B, 63), "faces": faces.astype(np.int64), "image": f(B, 3, 8, 8)}
    return out, scale, root, S


def _target_of(out, scale, root, S, n_true=3):
    """depth and mask of hypothesis n_true's own mesh: ops.render_mesh's depth (zscale in its mm convention) plus the root depth"""
    N, B = out["logs_t"].shape[:2]
    lt = _cu(out["logs_t"][n_true])
    r = ops.render_mesh(_cu(out["verts"][n_true].reshape(B, -1, 3)), _cu(out["faces"].astype(np.int32)), lt[:, 0].exp().contiguous(), lt[:, 1:].contiguous(),
                        zscale=_cu(scale * 1000.0), size=S, anti_aliasing=False, far=0.0, want=("mask", "depth"))
    mask = r["mask"] > 0
    return {"depth": torch.where(mask, r["depth"] + _cu(root[:, 2])[:, None, None], torch.zeros_like(r["depth"])), "hand_mask": mask,
            "scale": _cu(scale), "pose3d_root": _cu(root)}


@pytest.mark.parametrize("root", [False, True], ids=["fitted", "given"])
@pytest.mark.parametrize("Q", [1, 5])
def test_depth_select(Q, root, gpu_lib):
    out, scale, rt, S = _sample()
    o = {k: _cu(v) for k, v in out.items()}
    y = _target_of(out, scale, rt, S)
    sel = criteria.depth_select(o, y, Q=Q, size=S, trunc=dr.TRUNC, root=root)
    assert set(sel) == set(o) | {"depth_dist", "depth_index"} and sel["faces"] is o["faces"] and sel["image"] is o["image"]
    # ordering and tie rule against numpy on the kernel's own distances
    d = criteria.depth_dist(o["verts"], o["logs_t"], o["faces"], y["depth"], y["hand_mask"], y["scale"], root_z=y["pose3d_root"][:, 2] if root else None,
                            size=S, trunc=dr.TRUNC).cpu().numpy()
    order = np.argsort(d, axis=0, kind="stable")
    assert sel["depth_index"].dtype == torch.int64 and np.array_equal(sel["depth_index"].cpu().numpy(), order[:Q])
    assert np.array_equal(sel["depth_dist"].cpu().numpy(), np.take_along_axis(d, order, 0)[:Q])
    for k in ("th_bt", "logs_t", "verts", "xyz"):
        assert np.array_equal(sel[k].cpu().numpy(), out[k][order[:Q], np.arange(2)]), k
    # the hypothesis that IS the target mesh comes first, far ahead of the others (its own distance is rounding, and at most the cost of an
    # edge sample that the two rasterisers' scale arithmetic - exp in f32 there, in f64 here - decides differently)
    assert (order[0] == 3).all() and (d[3] < 0.25 * np.delete(d, 3, 0).min(0)).all(), d


def test_ties_go_to_the_lower_hypothesis(gpu_lib):
    out, scale, rt, S = _sample()
    o = {k: _cu(v) for k, v in out.items()}
    for k in ("verts", "logs_t"):
        o[k][4] = o[k][1]                                        # hypotheses 1 and 4 are the same mesh: equal bits, 1 first
    sel = criteria.depth_select(o, _target_of(out, scale, rt, S), Q=5, size=S)
    idx = sel["depth_index"].cpu().numpy()
    for b in range(2):
        i1, i4 = int(np.nonzero(idx[:, b] == 1)[0][0]), int(np.nonzero(idx[:, b] == 4)[0][0])
        assert i4 == i1 + 1 and float(sel["depth_dist"][i1, b]) == float(sel["depth_dist"][i4, b])


def test_graph_capture_replays_the_eager_bits(gpu_lib):
    op, _ = dr.case("mix_16_h64", False)
    got = _run("mix_16_h64", False)
    v, f, lt, zs, obs, _ = _operands(op, False)
    depth, mask, g = _cu(op["depth"]), _cu(op["hand_mask"]), _cu(op["g_dist"])
    ops.face_adjacency(f, v.shape[2])                             # the one host read, before the capture
    v.requires_grad_(True); lt.requires_grad_(True)

    def step():
        dist = criteria.depth_dist(v, lt, f, depth, mask, zs, size=16, trunc=dr.TRUNC)
        gv, gl = torch.autograd.grad((dist * g).sum(), (v, lt))
        return dist.detach(), gv, gl

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    for t in res:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(res[0].cpu().numpy(), got["dist"]) and np.array_equal(res[1].cpu().numpy(), got["g_verts"])
    assert np.array_equal(res[2].cpu().numpy(), got["g_logs_t"])


def test_entries_refuse_bad_arguments_before_any_launch(gpu_lib):
    from mhentropy_amd._lib import MheError
    op, _ = dr.case("tri_8", False)
    v, f, lt, zs, obs, _ = _operands(op, False)
    dist = torch.empty(1, 1, device="cuda")
    for bad in (dict(trunc=0.0), dict(trunc=float("inf")), dict(S=65), dict(V=1025), dict(F=2049), dict(N=0), dict(dist=None), dict(obs=None),
                dict(dist=lt)):
        a = dict(verts=v, faces=f, logs_t=lt, zscale=zs, obs=obs, root_z=None, trunc=0.05, dist=dist, parts=None, face_img=None, resid_img=None,
                 N=1, B=1, V=3, F=1, S=8)
        a.update(bad)
        with pytest.raises(MheError, match="mhe_depth_dist_f32"):
            ops.launch("mhe_depth_dist_f32", *a.values())
    start, lst = ops.face_adjacency(f, 3)
    gv, gl = torch.empty_like(v), torch.empty_like(lt)
    for bad in (dict(vf_start=None), dict(g_dist=None), dict(g_verts=v), dict(g_logs_t=None)):
        a = dict(verts=v, faces=f, logs_t=lt, zscale=zs, obs=obs, root_z=None, trunc=0.05, vf_start=start, vf_list=lst, g_dist=dist, g_verts=gv,
                 g_logs_t=gl, N=1, B=1, V=3, F=1, S=8)
        a.update(bad)
        with pytest.raises(MheError, match="mhe_depth_dist_bwd_f32"):
            ops.launch("mhe_depth_dist_bwd_f32", *a.values())
