"""GPU tests of the silhouette and depth renderer: mhe_render_mesh_f32 (csrc/render.hip) through ops.render_mesh, ManoLayer.render,
MHEnt.sample(mods=[..., 'm', 'depth']) and criteria.silhouette_iou, against the float64 rasteriser of tests/render_ref.py (computed once per case
and shared; its known-answer checks and the ambiguity cap of every case run on the CPU, tests/test_render_host.py).

Bounds.  Parity is checked on every pixel none of whose samples lies within render_ref.EDGE = 1e-3 sample spacings of a projected edge (the
contract lets a sample on an edge go either way; the derivation of EDGE is in render_ref's docstring): mask exactly (multiples of 1/A^2),
`far` pixels exactly, depth to RTOL = 1e-4 of the largest |d|, the project's bound for f32 kernels against f64.  iou_sums: each ambiguous
sample can move either sum by at most 1/A^2, so the bound of row r is n_ambiguous(r) / A^2 + RTOL ref.  Every parity test prints the smallest edge
distance among the samples it skipped.

Shapes: render_ref.CASES - S = 16 / 64 / 256 anti-aliased (256: 16 row bands, faces straddle them), S = 64 without anti-aliasing on long
overlapping faces (the workgroup's big-face list), F = 1, and V = 6,890 / F = 13,776 (vertices not staged in LDS).  R is 2..6 everywhere."""
import numpy as np
import pytest
import torch

import render_ref
from mhentropy_amd import criteria, harness, ops, synth

pytestmark = pytest.mark.gpu
RTOL = 1e-4
ALL = ("mask", "depth", "iou_sums")


def _cu(a):
    return None if a is None else torch.as_tensor(np.array(a)).cuda()          # (a copy: the shared case arrays are read-only)


def _render(o, want=ALL, **over):
    o = dict(o, **over)
    target = o.get("target") if "iou_sums" in want else None
    out = ops.render_mesh(_cu(o["verts"]), _cu(o["faces"]), _cu(o["scale"]), _cu(o["trans"]), _cu(o.get("zscale")), size=o["size"],
                          anti_aliasing=o["anti_aliasing"], far=100.0, want=want, target=_cu(target))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_images(name, got, ref):
    ok = ~ref["ambiguous"]
    hit = ok & (ref["mask"] > 0)
    scale = np.abs(ref["depth"][ref["mask"] > 0]).max()
    derr = np.abs(got["depth"][hit] - ref["depth"][hit]).max() if hit.any() else 0.0
    print(f"{name}: {(~ok).sum()} of {ok.size} pixels skipped, nearest skipped sample {render_ref.skipped_edge_distance(ref):.2e} from an edge; "
          f"mask mismatches {(got['mask'][ok] != ref['mask'][ok]).sum()}, depth err {derr:.3e} of {scale:.3e}")
    assert np.array_equal(got["mask"][ok], ref["mask"][ok].astype(np.float32)), name + " mask"
    empty = ok & (ref["mask"] == 0)
    assert (got["depth"][empty] == np.float32(100.0)).all(), name + " far pixels"
    assert derr <= RTOL * scale, f"{name} depth: {derr:.3e} > {RTOL * scale:.3e}"


def _check_sums(name, got, ref):
    bound = ref["n_ambiguous"][:, None] / ref["A"] ** 2 + RTOL * ref["iou_sums"]
    err = np.abs(got["iou_sums"] - ref["iou_sums"])
    print(f"{name}: iou_sums err {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}")
    assert (err <= bound).all(), (name, err, bound)


@pytest.mark.parametrize("name", sorted(render_ref.CASES))
def test_parity_with_the_f64_rasteriser(name, gpu_lib):
    o, ref = render_ref.case(name)
    got = _render(o)
    _check_images(name, got, ref)
    _check_sums(name, got, ref)
    # the sums are those of the kernel's OWN mask
    m, t = torch.as_tensor(got["mask"]).double(), torch.as_tensor(np.array(o["target"])).double()
    t = t[torch.arange(m.shape[0]) % t.shape[0]]
    own = torch.stack([torch.minimum(m, t).sum((1, 2)), torch.maximum(m, t).sum((1, 2))], 1).numpy()
    assert (np.abs(got["iou_sums"] - own) <= 1e-5 * own).all(), (got["iou_sums"], own)
    # score only: no image is written, the same bits; and a second call gives the same bits in all three outputs
    assert np.array_equal(_render(o, want=("iou_sums",))["iou_sums"], got["iou_sums"])
    again = _render(o)
    assert all(np.array_equal(again[k], got[k]) for k in ALL)


def test_image_only_call_takes_the_band_grid_and_agrees(gpu_lib):
    """without a score every band of the S = 256 image has its own workgroup: the same images as the one-workgroup-per-row form"""
    o, ref = render_ref.case("sheet_256aa")
    both, img = _render(o), _render(o, want=("mask", "depth"))
    assert np.array_equal(img["mask"], both["mask"]) and np.array_equal(img["depth"], both["depth"])
    only = _render(o, want=("depth",))
    assert np.array_equal(only["depth"], both["depth"])


def _shifted_case():
    v, f = render_ref.sheet(21, 12, 12, extent=0.5)
    R = 3
    verts = np.repeat(v[None], R, 0)
    scale, zscale = np.array([1.0, 1.0, 1.0], np.float32), np.array([100.0, 100.0, 100.0], np.float32)
    trans = np.array([[0.0, 0.0], [0.8, -0.7], [3.0, 0.1]], np.float32)          # on screen; partly off; all off
    return dict(verts=verts, faces=f, scale=scale, trans=trans, zscale=zscale, size=32, anti_aliasing=True)


def test_mesh_partly_and_wholly_off_screen(gpu_lib):
    o = _shifted_case()
    ref = render_ref.render64(o["verts"], o["faces"], o["scale"], o["trans"], o["zscale"], 32, True)
    got = _render(o, want=("mask", "depth"))
    _check_images("shifted", got, ref)
    assert 0 < ref["mask"][1].sum() < 0.6 * ref["mask"][0].sum()
    assert (got["mask"][2] == 0).all() and (got["depth"][2] == np.float32(100.0)).all()


def test_one_face_covering_the_whole_image(gpu_lib):
    v = np.array([[[-3.0, -3.0, 0.5], [5.0, -3.0, 0.5], [-3.0, 5.0, 0.5]]] * 2, np.float32)
    for S, aa in ((64, True), (256, True), (9, False)):
        got = _render(dict(verts=v, faces=np.array([[0, 1, 2]], np.int32), scale=np.ones(2, np.float32), trans=np.zeros((2, 2), np.float32), size=S,
                           anti_aliasing=aa), want=("mask", "depth"))
        assert (got["mask"] == 1).all() and (got["depth"] == np.float32(0.5)).all(), S


def test_degenerate_and_out_of_range_faces_are_ignored(gpu_lib):
    o, _ = render_ref.case("sheet_16aa")
    verts = np.array(o["verts"])
    verts[:, 5, 0] = verts[:, 4, 0]; verts[:, 6, 0] = verts[:, 4, 0]          # vertices 4, 5, 6 share their x: a face of exactly zero projected area
    V = verts.shape[1]
    planted = np.concatenate([o["faces"][:700], [[10, 10, 300], [4, 5, 6]], o["faces"][700:], [[3, 2, V]], [[-1, 7, 8]], [[1, 2 ** 30, 3]]]).astype(np.int32)
    a = dict(o, verts=verts)
    clean = _render(a)
    t = {k: _cu(a[k]) for k in ("verts", "scale", "trans", "zscale", "target")}
    R, S = verts.shape[0], o["size"]
    mask, depth, sums = torch.empty(R, S, S, device="cuda"), torch.empty(R, S, S, device="cuda"), torch.empty(R, 2, device="cuda")
    # the C entry directly: ops.render_mesh refuses an index outside [0, V) before it launches
    ops.launch("mhe_render_mesh_f32", t["verts"], _cu(planted), t["scale"], t["trans"], t["zscale"], t["target"], mask, depth, sums, R, t["target"].shape[0], V,
               len(planted), S, 1, 100.0)
    torch.cuda.synchronize()
    assert np.array_equal(mask.cpu().numpy(), clean["mask"]) and np.array_equal(depth.cpu().numpy(), clean["depth"])
    assert np.array_equal(sums.cpu().numpy(), clean["iou_sums"])
    with pytest.raises(ValueError, match="outside the V="):
        _render(dict(a, faces=planted))


def test_negative_scale_and_optional_zscale(gpu_lib):
    o, _ = render_ref.case("sheet_16aa")
    a, b = _render(o), _render(o, scale=-np.array(o["scale"]))
    assert all(np.array_equal(a[k], b[k]) for k in ALL)
    plain = _render(o, want=("mask", "depth"), zscale=None)
    milli = _render(o, want=("mask", "depth"), zscale=np.full(len(o["scale"]), 1000.0, np.float32))          # z * 1000 / 1000
    assert np.array_equal(plain["mask"], a["mask"]) and np.array_equal(plain["mask"], milli["mask"])
    hit = plain["mask"] > 0
    assert np.abs(plain["depth"] - milli["depth"]).max() <= 1e-6 * np.abs(plain["depth"][hit]).max()
    ref = render_ref.render64(o["verts"], o["faces"], o["scale"], o["trans"], None, o["size"], o["anti_aliasing"])
    _check_images("no zscale", plain, ref)


def test_row_r_is_scored_against_image_r_mod_B(gpu_lib):
    o, _ = render_ref.case("sheet_16aa")
    N, B, S = 3, 2, o["size"]
    verts = np.concatenate([o["verts"], o["verts"]])          # R = 6 sample-major rows
    rep = lambda a: np.concatenate([a, a])
    rng = np.random.default_rng(5)
    target = rng.uniform(0, 1, (B, S, S)).astype(np.float32)
    target[1, : S // 2] = 0
    a = dict(o, verts=verts, scale=rep(o["scale"]), trans=rep(o["trans"]), zscale=rep(o["zscale"]), target=target)
    got = _render(a)
    m = got["mask"].astype(np.float64)
    for r in range(N * B):
        t = target[r % B].astype(np.float64)
        want = np.array([np.minimum(m[r], t).sum(), np.maximum(m[r], t).sum()])
        assert (np.abs(got["iou_sums"][r] - want) <= 1e-5 * want).all(), r
    other = np.array([np.minimum(m[0], target[1]).sum(), np.maximum(m[0], target[1]).sum()])
    assert (np.abs(got["iou_sums"][0] - other) > 1e-2 * other).any()          # ... and the two targets tell rows apart


# ---- the public surface -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(gpu_lib):
    B, N, h, steps = 2, 4, 64, 2          # the C0 configuration of smoke()
    sd = {"q_z_giv_i." + k: v for k, v in synth.flow_state(7, 45, 512, (h, h), steps).items()}
    sd.update(synth.head_state(7, 512, 512, 16))
    sd.update({"feat_extractor.res." + k: v for k, v in synth.resnet_state(7, "resnet18").items()})
    m = harness.build_mhent(backbone="resnet18", h_dims=(h, h), num_steps=steps, tables=synth.mano_tables(0))
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    x, _ = synth.batch(7, B, image_size=128)
    return m.cuda().eval(), torch.as_tensor(x).cuda(), torch.as_tensor(synth.noise(7, N * B)).cuda(), N, B


def test_mano_layer_render_is_render_mesh_with_the_references_keys(model):
    m = model[0]
    R = 3
    g = torch.Generator().manual_seed(3)
    vertex = (torch.rand(R, 778, 3, generator=g) * 1.6 - 0.8).cuda()
    s, t, norm = (torch.rand(R, 1, generator=g) + 0.5).cuda(), (torch.rand(R, 2, generator=g) * 0.2 - 0.1).cuda(), (torch.rand(R, generator=g) * 50 + 60).cuda()
    out = m.mano_dec.render(-s, t, vertex=vertex, norm=norm, render=["mask", "depth"])
    assert set(out) == {"mask", "depth"} and all(tuple(v.shape) == (R, 64, 64) for v in out.values()) and m.mano_dec.mask_sz == 64
    mine = ops.render_mesh(vertex, m.mano_dec.mano_layer.faces_i32, s.view(R), t, norm, size=64, anti_aliasing=True, want=("mask", "depth"))
    assert torch.equal(out["mask"], mine["mask"]) and torch.equal(out["depth"], mine["depth"])
    assert set(m.mano_dec.render(s, t, vertex=vertex, norm=norm)) == {"mask"}
    assert m.mano_dec.render(s, t) == {}


def test_sample_adds_mask_and_depth(model):
    m, x, noise, N, B = model
    with torch.no_grad():
        feat = m.feat_extractor(x)[1]
        plain = m.sample(x, N=N, noise=noise, feat=feat)
        assert set(plain) == {"th_bt", "logs_t", "verts", "faces", "xyz", "uv"}
        out = m.sample(x, N=N, noise=noise, feat=feat, mods=["verts", "uv", "m", "depth"])
        assert set(out) == {"th_bt", "logs_t", "verts", "faces", "uv", "mask", "depth"}
        assert tuple(out["mask"].shape) == tuple(out["depth"].shape) == (N, B, 64, 64)
        assert 0 <= float(out["mask"].min()) and float(out["mask"].max()) <= 1 and torch.equal(out["verts"], plain["verts"])
        assert set(m.sample(x, N=N, noise=noise, feat=feat, mods=["m"])) == {"th_bt", "logs_t", "mask"}
        # by hand: the joint pass on the same operands, then the renderer on its mesh
        R = N * B
        o = ops.mano_joints(out["th_bt"][..., 3:48].reshape(R, 45).contiguous(), m._det(feat), m.mano_dec.table_blob(), inv_norm=True,
                            image_size=float(m.image_size), want=("z", "verts", "joints_mm"))
        assert torch.equal(o["verts"].view(N, B, -1), out["verts"]) and torch.equal(o["z"][:, -3:].reshape(N, B, 3), out["logs_t"])
        J, lt = o["joints_mm"].view(R, 21, 3), out["logs_t"].reshape(R, 3)
        mine = ops.render_mesh(out["verts"].reshape(R, 778, 3), m.mano_dec.mano_layer.faces_i32, lt[:, 0].exp().contiguous(), lt[:, 1:].contiguous(),
                               (J[:, 11] - J[:, 12]).norm(dim=-1), size=64, anti_aliasing=True, want=("mask", "depth"))
    assert torch.equal(mine["mask"].view(N, B, 64, 64), out["mask"]) and torch.equal(mine["depth"].view(N, B, 64, 64), out["depth"])


def _iou_case():
    o, _ = render_ref.case("crossing_64aa")
    N, B = 3, 2
    v = np.concatenate([o["verts"], o["verts"][::-1]]).reshape(N, B, -1)          # (N, B, V*3)
    logs_t = np.stack([np.log(np.abs(np.concatenate([o["scale"], o["scale"][::-1]]))), *np.concatenate([o["trans"], o["trans"][::-1]]).T], 1)
    logs_t = logs_t.astype(np.float32).reshape(N, B, 3)
    logs_t[1, 1, 1] = 5.0                                                          # hypothesis (1, 1) is off the screen
    rng = np.random.default_rng(9)
    hand = np.zeros((B, 256, 256), bool)
    hand[0, 40:200, 60:220] = rng.uniform(0, 1, (160, 160)) < 0.8
    return o, N, B, v, logs_t, hand                                               # image 1's mask is empty: with hypothesis (1, 1) a union of 0


def test_silhouette_iou_against_the_f64_reference(gpu_lib):
    o, N, B, v, logs_t, hand = _iou_case()
    iou = criteria.silhouette_iou(_cu(v), _cu(logs_t), _cu(o["faces"]), _cu(hand), size=64)
    assert tuple(iou.shape) == (N, B) and iou.dtype == torch.float32
    iou = iou.cpu().numpy()
    lt = logs_t.reshape(N * B, 3)
    target = hand.astype(np.float64).reshape(B, 64, 4, 64, 4).mean((2, 4))
    ref = render_ref.render64(v.reshape(N * B, -1, 3), o["faces"], np.exp(lt[:, 0].astype(np.float64)), lt[:, 1:], None, 64, True, target=target)
    assert ref["n_ambiguous"].sum() <= render_ref.CAP * N * B * 128 * 128
    inter, union = ref["iou_sums"][:, 0], ref["iou_sums"][:, 1]
    slack = ref["n_ambiguous"] / 4 + RTOL * union          # of either sum
    lo = np.where(union > 0, np.maximum(inter - slack, 0) / np.maximum(union + slack, 1e-300), 0.0)
    hi = np.where(union > 0, (inter + slack) / np.maximum(union - slack, 1e-300), 0.0)
    print("iou", iou.reshape(-1), "reference", np.where(union > 0, inter / np.maximum(union, 1e-300), 0).reshape(-1), "slack", slack)
    assert (iou.reshape(-1) >= lo - 1e-6).all() and (iou.reshape(-1) <= hi + 1e-6).all()
    assert union[1 * B + 1] == 0 and iou[1, 1] == 0          # an empty union scores 0
    assert (iou[:, 0] > 0.1).all()
    fl = criteria.silhouette_iou(_cu(v).view(N, B, -1, 3), _cu(logs_t), _cu(o["faces"]).long(), _cu(hand).float(), size=64)
    assert np.array_equal(fl.cpu().numpy(), iou)


def test_a_hypothesis_wins_against_its_own_silhouette(gpu_lib):
    o, N, B, v, logs_t, _ = _iou_case()
    logs_t = np.array(logs_t)
    logs_t[1, 1, 1] = 0.0
    logs_t[:, :, 1] += np.array([0.0, 0.25, -0.3])[:, None]          # the three hypotheses of an image lie apart
    winner = np.array([2, 0])
    rows = winner * B + np.arange(B)
    lt = logs_t.reshape(N * B, 3)[rows]
    own = ops.render_mesh(_cu(v.reshape(N * B, -1, 3)[rows]), _cu(o["faces"]), _cu(lt[:, 0]).exp(), _cu(lt[:, 1:]), size=64)["mask"]
    hand = own.repeat_interleave(4, 1).repeat_interleave(4, 2)          # (B, 256, 256): box-averaged back to the silhouette itself
    iou = criteria.silhouette_iou(_cu(v), _cu(logs_t), _cu(o["faces"]), hand)
    assert iou.argmax(0).cpu().tolist() == winner.tolist()
    best = iou.max(0).values.cpu().numpy()
    assert (best == 1.0).all() and (np.sort(iou.cpu().numpy(), 0)[-2] < 0.9).all()
