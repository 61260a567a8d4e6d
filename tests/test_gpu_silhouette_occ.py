"""GPU tests of the occlusion-aware silhouette distance: mhe_silhouette_pixels_occ / mhe_silhouette_dist_occ_f32 / _dist_bwd_occ_f32 /
_dist_grad_occ_f32 (csrc/silhouette.hip) through ops.silhouette_*(count_all=...), criteria.silhouette_dist(occluder=...),
criteria.silhouette_select(occluder=...) and the training term get_loss(sil_w=..., sil_occluder=True) under autograd, TrainStep and GraphedStep.
Everything against the float64 restatement of tests/silhouette_occ_ref.py, computed once per case and shared.

Bounds (silhouette_occ_ref.FWD_RTOL / REV_RTOL, relative to the reference's largest value): four times what the restatement evaluated in f32
on the CPU deviates from f64 on these very inputs, the margin of tests/test_gpu_silhouette.py.  Measured f32 deviations, forward / reverse:
v1_s4 6.8e-8 / 5.7e-8, v5_s4 1.18e-7 / 1.04e-7, v257_s4 1.36e-7 / 6.2e-7, v778_s4 1.59e-7 / 3.4e-7, v1_s8 3.3e-8 / 9.6e-8, v5_s8 1.27e-7 /
1.34e-7, v257_s8 1.41e-7 / 2.9e-6, v778_s8 2.24e-7 / 1.17e-6, v257_s64_two_rounds 6.2e-8 / 7.7e-7 (tests/test_silhouette_occ_host.py
re-measures them).  The pixel list and both index tensors are compared bit for bit: the seeds are those for which the f32 restatement attains
the f64 indices everywhere."""
import functools

import numpy as np
import pytest
import torch

import silhouette_occ_ref as so
import silhouette_ref as sr
from conftest import assert_close
from mhentropy_amd import criteria, ops, synth

pytestmark = pytest.mark.gpu


def _cu(a):
    return torch.as_tensor(np.array(a)).cuda()


def _same(a, b):
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


# ---- pixel list -------------------------------------------------------------------------------------------------------------------------------
def _list_batch(S, k, rng):
    """B = 6 images (H = S k): a blob hand with an overlapping box; an empty hand under an occluder; a hand without occluder; a hand whose
    occluder is everything else (count_all = S^2); both masks full (the occluder section is empty); noise on both, box means at 0.5 included"""
    H = S * k
    hand = np.concatenate([sr.blob_mask(rng, 1, H, "blob") for _ in range(4)] + [np.ones((1, H, H), bool), rng.uniform(0, 1, (1, H, H)) < 0.5])
    occ = np.zeros_like(hand)
    occ[0, H // 4:H // 4 + H // 2, H // 3:] = True
    hand[1] = False
    occ[1, :H // 2] = True
    occ[3] = ~hand[3]
    occ[4] = True
    occ[5] = rng.uniform(0, 1, (H, H)) < 0.5
    return hand, occ


@pytest.mark.parametrize("S,k", [(4, 1), (4, 2), (8, 1), (8, 2)])
@pytest.mark.parametrize("hand_as,occ_as", [("bool", "bool"), ("u8", "f32"), ("f32", "u8"), ("f32", "f32")])
def test_two_section_pixel_list_equals_the_restatement_bit_for_bit(S, k, hand_as, occ_as, gpu_lib):
    rng = np.random.default_rng(S * 10 + k)
    hand, occ = _list_batch(S, k, rng)
    conv = {"bool": lambda m: m, "u8": lambda m: m.astype(np.uint8) * 255,
            "f32": lambda m: (m * rng.choice([0.25, 0.5, 0.75, 1.0], m.shape)).astype(np.float32)}          # exact box sums, means at 0.5
    hand, occ = conv[hand_as](hand), conv[occ_as](occ)
    want_p, want_c, want_a = so.pixel_list(hand, occ, S)
    pixels, count, count_all = ops.silhouette_pixels(_cu(hand), S, _cu(occ))
    assert pixels.dtype == count.dtype == count_all.dtype == torch.int32 and tuple(pixels.shape) == (6, S * S)
    assert np.array_equal(count.cpu().numpy(), want_c) and np.array_equal(count_all.cpu().numpy(), want_a), (count, count_all, want_c, want_a)
    assert np.array_equal(pixels.cpu().numpy(), want_p)
    if hand_as == "bool" and occ_as == "bool":
        assert want_c[1] == 0 and want_a[1] == S * S // 2 and want_a[2] == want_c[2] and want_a[3] == S * S > want_c[3] > 0
        assert want_c[4] == want_a[4] == S * S and 0 < want_c[0] < want_a[0]
        assert len(set(want_p[0, :want_a[0]].tolist())) == want_a[0]          # the overlap is listed once
    # the hand section and its count are those of the one-mask entry
    p1, c1 = ops.silhouette_pixels(_cu(hand), S)
    assert torch.equal(c1, count)
    for b in range(6):
        assert torch.equal(p1[b, :want_c[b]], pixels[b, :want_c[b]])
    if k == 2 and hand_as == "f32":          # a box mean of exactly 0.5 is kept, in either mask
        m = np.zeros((1, 2 * S, 2 * S), np.float32)
        o = np.zeros_like(m)
        m[0, 0:2, 0:2] = 0.5
        o[0, 2:4, 2:4] = [[1, 1], [0, 0]]
        o[0, 0:2, 2:4] = [[1, 0], [0, 0.75]]          # 0.4375: not kept
        p, c, a = ops.silhouette_pixels(_cu(m), S, _cu(o))
        assert c.tolist() == [1] and a.tolist() == [2] and p[0, :3].tolist() == [0, (1 << 16) | 1, -1]


# ---- distance and indices ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _forward(name):
    case, ref = so.reference(name)
    S = so.CASES[name]["S"]
    pixels, count, count_all = ops.silhouette_pixels(_cu(case["mask"]), S, _cu(case["occluder"]))
    v, lt = _cu(case["verts"]), _cu(case["logs_t"])
    out = ops.silhouette_dist(v, lt, pixels, count, want_idx=True, count_all=count_all)
    torch.cuda.synchronize()
    return (v, lt, pixels, count, count_all) + tuple(out)


@pytest.mark.parametrize("name", list(so.CASES))
def test_forward_parity_and_exact_indices(name, gpu_lib):
    case, ref = so.reference(name)
    v, lt, pixels, count, count_all, dist, parts, idx_v, idx_m = _forward(name)
    assert np.array_equal(pixels.cpu().numpy(), ref["pixels"]) and np.array_equal(count.cpu().numpy(), ref["count"])
    assert np.array_equal(count_all.cpu().numpy(), ref["count_all"])
    dist, parts = dist.cpu().numpy(), parts.cpu().numpy()
    devs = [sr.rel_dev(a, ref[k]) for a, k in ((dist, "dist"), (parts[..., 0], "inside"), (parts[..., 1], "cover"))]
    print(f"{name}: dist / inside / cover deviation {devs[0]:.3e} {devs[1]:.3e} {devs[2]:.3e} (bound {so.FWD_RTOL:.3e})")
    assert max(devs) <= so.FWD_RTOL, (name, devs)
    assert np.array_equal(idx_v.cpu().numpy(), ref["idx_v"]) and np.array_equal(idx_m.cpu().numpy(), ref["idx_m"])
    assert (ref["idx_v"] >= ref["count"][None, :, None]).any() or name == "v1_s4"          # vertices that chose an occluder pixel
    plain = ops.silhouette_dist(v, lt, pixels, count, count_all=count_all)          # the values do not depend on the indices being asked for
    assert _same(plain[0].cpu(), torch.as_tensor(dist)) and _same(plain[1].cpu(), torch.as_tensor(parts))
    if name == "v1_s4":          # image 0: no hand under a 4-pixel occluder
        assert ref["count"][0] == 0 and ref["count_all"][0] > 0 and (dist[:, 0] == 0).all() and (parts[:, 0] == 0).all()
        assert (idx_v[:, 0] == -1).all() and (idx_m[:, 0] == -1).all()


@pytest.mark.parametrize("name", list(so.CASES))
def test_both_reverse_paths_agree_bit_for_bit_and_with_the_reference(name, gpu_lib):
    case, ref = so.reference(name)
    v, lt, pixels, count, count_all, dist, parts, idx_v, idx_m = _forward(name)
    g = _cu(so.g_dist_of(name, ref["dist"].shape))
    gv, gl = ops.silhouette_dist_bwd(v, lt, pixels, count, idx_v, idx_m, g, count_all=count_all)
    d2, gv2, gl2 = ops.silhouette_dist_grad(v, lt, pixels, count, g, want_dist=True, count_all=count_all)
    assert _same(d2, dist) and torch.equal(gv2, gv) and torch.equal(gl2, gl)
    gv3, gl3 = ops.silhouette_dist_grad(v, lt, pixels, count, g, count_all=count_all)          # two launches, dist = NULL: the same bits
    assert torch.equal(gv3, gv) and torch.equal(gl3, gl)
    want_v, want_l = so.reference_grad(name)
    dv, dl = sr.rel_dev(gv.cpu().numpy(), want_v), sr.rel_dev(gl.cpu().numpy(), want_l)
    print(f"{name}: g_verts deviation {dv:.3e} of {np.abs(want_v).max():.3e}, g_logs_t {dl:.3e} of {np.abs(want_l).max():.3e} (bound {so.REV_RTOL[name]:.3e})")
    assert torch.isfinite(gv).all() and torch.isfinite(gl).all() and (gv[..., 2] == 0).all()
    assert max(dv, dl) <= so.REV_RTOL[name]
    assert np.abs(want_v).max() > 0
    if name == "v1_s4":
        assert not gv[:, 0].any() and not gl[:, 0].any()          # the image without a hand
    # through criteria's autograd node (the index path, count_all saved next to count): the same bits
    va, la = v.clone().requires_grad_(True), lt.clone().requires_grad_(True)
    out = criteria.silhouette_dist(va, la, _cu(case["mask"]), size=so.CASES[name]["S"], parts=True, occluder=_cu(case["occluder"]))
    ga, gla = torch.autograd.grad(out[0], (va, la), g)
    assert _same(out[0].detach(), dist) and _same(out[1], parts[..., 0]) and _same(out[2], parts[..., 1])
    assert torch.equal(ga, gv) and torch.equal(gla, gl)


# ---- edge rows --------------------------------------------------------------------------------------------------------------------------------
def test_edge_rows_empty_hand_nan_vertex_occluder_interior_and_the_tie(gpu_lib):
    """S = 8, camera s = 1, t = 0 and coordinates that are multiples of 1/8: every distance is exact in f32.  Image 0: hand pixel (2, 2), occluder
    pixel (2, 5) - centres (-0.375, -0.375) and (0.375, -0.375); image 1: no hand, the same occluder"""
    S = 8
    mask, occ = np.zeros((2, S, S), bool), np.zeros((2, S, S), bool)
    mask[0, 2, 2] = True
    occ[:, 2, 5] = True
    # vertex 0: midway between the two squares (a tie: the hand pixel, position 0); 1: inside the occluder pixel; 2: right of it; 3: on the hand
    one = np.array([[0, -0.375, 0], [0.4375, -0.4375, 1], [0.75, -0.375, 2], [-0.375, -0.375, 3]], np.float32)
    verts = np.stack([one, one, one])[:, None].repeat(2, 1)          # (3, 2, 4, 3)
    verts[2, 0, 2, 0] = np.nan                                          # row (2, 0)
    logs_t = np.zeros((3, 2, 3), np.float32)
    ref = so.silhouette(verts, logs_t, mask, occ, S)
    assert ref["idx_v"][0, 0].tolist() == [0, 1, 1, 0] and ref["d_v"][0, 0].tolist() == [0.25, 0.0, 0.25, 0.0]
    v, lt = _cu(verts), _cu(logs_t)
    pixels, count, count_all = ops.silhouette_pixels(_cu(mask), S, _cu(occ))
    assert count.tolist() == [1, 0] and count_all.tolist() == [2, 1]
    dist, parts, idx_v, idx_m = ops.silhouette_dist(v, lt, pixels, count, want_idx=True, count_all=count_all)
    g = _cu(np.array([[1.0, 1.0], [-0.5, 2.0], [1.5, 1.0]], np.float32))
    gv, gl = ops.silhouette_dist_bwd(v, lt, pixels, count, idx_v, idx_m, g, count_all=count_all)
    gv2, gl2 = ops.silhouette_dist_grad(v, lt, pixels, count, g, count_all=count_all)
    assert torch.equal(gv, gv2) and torch.equal(gl, gl2)
    # the image without a hand: 0, a zero gradient, idx_v = -1 - whatever the occluder holds
    assert (dist[:, 1] == 0).all() and (parts[:, 1] == 0).all() and (idx_v[:, 1] == -1).all() and (idx_m[:, 1] == -1).all()
    assert not gv[:, 1].any() and not gl[:, 1].any()
    # the NaN row, and no other
    assert torch.isnan(dist[2, 0]) and torch.isnan(parts[2, 0]).all() and int(torch.isnan(dist).sum()) == 1
    assert not gv[2, 0].any() and not gl[2, 0].any() and torch.isfinite(gv).all() and torch.isfinite(gl).all()
    # the clean rows of image 0: the tie goes to the hand pixel; the vertex inside the occluder costs exactly 0 and gets no inside gradient
    for n in (0, 1):
        assert idx_v[n, 0].tolist() == [0, 1, 1, 0] and idx_m[n, 0, :2].tolist() == [3, -1]
        assert float(parts[n, 0, 0]) == 0.125 and float(parts[n, 0, 1]) == 0.0          # (0.25 + 0 + 0.25 + 0) / 4; the hand centre has vertex 3 on it
        assert not gv[n, 0, 1].any() and not gv[n, 0, 3].any()
        gd = float(g[n, 0])
        assert gv[n, 0, 0].tolist() == [0.25 * gd, 0.0, 0.0] and gv[n, 0, 2].tolist() == [0.25 * gd, 0.0, 0.0]          # away from the pixel it chose
    want_v, want_l = so.grad(verts, logs_t, mask, occ, S, g.cpu().numpy(), (np.maximum(ref["idx_v"], 0), np.maximum(ref["idx_m"], 0)))
    assert sr.rel_dev(gv.cpu().numpy(), want_v) <= so.FWD_RTOL and sr.rel_dev(gl.cpu().numpy(), want_l) <= so.FWD_RTOL
    # without the occluder vertices 1 and 2 are pulled toward the hand
    d0 = criteria.silhouette_dist(v, lt, _cu(mask), size=S)
    d1 = criteria.silhouette_dist(v, lt, _cu(mask), size=S, occluder=_cu(occ))
    assert float(d0[0, 0]) > float(d1[0, 0]) == 0.125


# ---- the same bits as without the argument ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v65_s8_35_rows", "v778_s64_35_rows", "v5_s8_float_mask_2x"])
def test_an_empty_occluder_section_gives_the_bits_of_the_old_entries(name, gpu_lib):
    case, ref = sr.reference(name)
    S = sr.CASES[name]["S"]
    v, lt, mask = _cu(case["verts"]), _cu(case["logs_t"]), _cu(case["mask"])
    g = _cu(sr.g_dist_of(name, ref["dist"].shape))
    pixels, count = ops.silhouette_pixels(mask, S)
    for zero in (torch.zeros_like(mask), torch.zeros(mask.shape, device="cuda", dtype=torch.uint8), torch.zeros(mask.shape, device="cuda")):
        p2, c2, a2 = ops.silhouette_pixels(mask, S, zero)
        assert torch.equal(p2, pixels) and torch.equal(c2, count) and torch.equal(a2, count)
    old = ops.silhouette_dist(v, lt, pixels, count, want_idx=True)
    new = ops.silhouette_dist(v, lt, pixels, count, want_idx=True, count_all=count.clone())
    again = ops.silhouette_dist(v, lt, pixels, count, want_idx=True, count_all=count.clone())
    for a, b, c in zip(old, new, again):
        assert _same(a, b) and _same(b, c)
    for a, b in zip(ops.silhouette_dist_bwd(v, lt, pixels, count, old[2], old[3], g),
                    ops.silhouette_dist_bwd(v, lt, pixels, count, old[2], old[3], g, count_all=count.clone())):
        assert torch.equal(a, b)
    for a, b in zip(ops.silhouette_dist_grad(v, lt, pixels, count, g, want_dist=True),
                    ops.silhouette_dist_grad(v, lt, pixels, count, g, want_dist=True, count_all=count.clone())):
        assert _same(a, b)
    # the public function: occluder = zeros and occluder = None, values and both gradients
    res = []
    for occ in (None, torch.zeros_like(mask)):
        va, la = v.clone().requires_grad_(True), lt.clone().requires_grad_(True)
        out = criteria.silhouette_dist(va, la, mask, size=S, parts=True, occluder=occ)
        res.append(tuple(o.detach() for o in out) + torch.autograd.grad(out[0], (va, la), g))
    for a, b in zip(*res):
        assert _same(a, b)
    # a count_all below count or above S^2 is clamped to count .. S^2 on the device
    low = ops.silhouette_dist(v, lt, pixels, count, want_idx=True, count_all=torch.full_like(count, -5))
    for a, b in zip(old, low):
        assert _same(a, b)


def test_count_all_beyond_the_grid_is_clamped(gpu_lib):
    name = "v5_s8"
    v, lt, pixels, count, count_all, dist, parts, idx_v, idx_m = _forward(name)
    full = pixels.clone()
    for b in range(3):          # fill the -1 tail with the remaining grid pixels, so that S^2 entries are valid
        have = set(full[b, :int(count_all[b])].tolist())
        rest = [(i << 16) | j for i in range(8) for j in range(8) if ((i << 16) | j) not in have]
        full[b, int(count_all[b]):] = torch.tensor(rest, dtype=torch.int32)
    a = ops.silhouette_dist(v, lt, full, count, want_idx=True, count_all=torch.full_like(count, 1 << 20))
    b = ops.silhouette_dist(v, lt, full, count, want_idx=True, count_all=torch.full_like(count, 64))
    for x, y in zip(a, b):
        assert _same(x, y)
    assert int(a[2].max()) < 64 and (a[1][..., 0] <= parts[..., 0]).all()


def test_refusals(gpu_lib):
    import ctypes as C
    from mhentropy_amd import _lib
    name = "v5_s8"
    v, lt, pixels, count, count_all, dist, parts, idx_v, idx_m = _forward(name)
    g = torch.ones_like(dist)
    gv, gl = torch.empty_like(v), torch.empty_like(lt)
    L = _lib.lib()
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    assert L.mhe_silhouette_dist_occ_f32(p(v), p(lt), p(pixels), p(count), p(None), p(dist), p(parts), p(None), p(None), 2, 3, 5, 8, None) == 1
    assert b"count_all" in L.mhe_last_error()
    assert L.mhe_silhouette_dist_bwd_occ_f32(p(v), p(lt), p(pixels), p(count), p(None), p(idx_v), p(idx_m), p(g), p(gv), p(gl), 2, 3, 5, 8, None) == 1
    assert L.mhe_silhouette_dist_grad_occ_f32(p(v), p(lt), p(pixels), p(count), p(None), p(g), p(None), p(gv), p(gl), 2, 3, 5, 8, None) == 1
    assert L.mhe_silhouette_dist_grad_occ_f32(p(v), p(lt), p(pixels), p(count), p(count_all), p(g), p(None), p(gv), p(count_all), 2, 3, 5, 8, None) == 1
    m = torch.zeros(3, 8, 8, dtype=torch.bool, device="cuda")
    for args in ((p(m), 0, p(None), 0, p(pixels), p(count), p(count_all), 3, 8, 8), (p(m), 0, p(m), 2, p(pixels), p(count), p(count_all), 3, 8, 8),
                 (p(m), 0, p(m), 0, p(pixels), p(count), p(count), 3, 8, 8), (p(m), 0, p(m), 0, p(pixels), p(count), p(count_all), 3, 8, 3)):
        assert L.mhe_silhouette_pixels_occ(*args, None) == 1
    with pytest.raises(_lib.MheError):
        ops.silhouette_pixels(m, 8, m.cpu())
    with pytest.raises(_lib.MheError):
        ops.silhouette_pixels(m, 8, m[:2])


# ---- the training term ------------------------------------------------------------------------------------------------------------------------
B, N, W = 2, 4, 10.0


def _small_model():
    from test_gpu_train import _model_and_state
    return _model_and_state("resnet18", 64, 2)          # ResNet-18 and the small flow of config C0


def _batch(seed=3, Bn=B, image_size=96, H=64):
    xn, yn = synth.batch(seed, Bn, image_size=image_size)
    yn["hand_mask"], yn["object_mask"] = synth.object_masks(seed, synth.hand_masks(seed, Bn, H=H, crop_uv=yn["crop_uv"]))
    return torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}


def test_training_term_autograd_train_step_and_graph_agree(gpu_lib):
    """get_loss(sil_w, sil_occluder=True) under autograd (the bridge), TrainStep and GraphedStep: the same 'silhouette' and parameter
    gradients, to the agreement tests/test_gpu_sil_train.py holds the three paths to without an occluder (bridge vs step: 1e-6 values, 1e-5
    gradients; replay vs eager step: bit for bit).  The list is rebuilt inside the graph; an all-zero occluder is sil_occluder=False"""
    from mhentropy_amd.train import TrainStep, GraphedStep
    model, _ = _small_model()
    x, y = _batch()
    z0 = torch.as_tensor(synth.noise(3, N * B)).cuda()
    ts = TrainStep(model, lr=0.0)
    # the module against criteria.silhouette_dist on the sampled meshes, with and without the occluder
    with torch.no_grad():
        on = model.get_loss(x, y, N=N, noise=z0, sil_w=W, sil_occluder=True)
        off = model.get_loss(x, y, N=N, noise=z0, sil_w=W)
        zero = model.get_loss(x, dict(y, object_mask=torch.zeros_like(y["object_mask"])), N=N, noise=z0, sil_w=W, sil_occluder=True)
        s = model.sample(x, N=N, temp=1.0, noise=z0, mods=["verts"])
        want = criteria.silhouette_dist(s["verts"], s["logs_t"], y["hand_mask"], 64, occluder=y["object_mask"]).mean(0)
    assert_close(on["silhouette"].cpu(), want.cpu(), 1e-4, what="silhouette vs silhouette_dist(occluder)")
    assert (on["silhouette"] < off["silhouette"]).all()          # the occluder only removes cost
    for k in off:
        assert torch.equal(off[k], zero[k]), k
    with pytest.raises(ValueError, match="object_mask"):
        model.get_loss(x, {k: v for k, v in y.items() if k != "object_mask"}, N=N, noise=z0, sil_w=W, sil_occluder=True)
    # the explicit reverse pass
    ref = ts.forward_backward(x, y, noise=z0, N=N, sil_w=W, sil_occluder=True)
    G = ts.G.clone()
    assert_close(ref["silhouette"].cpu(), on["silhouette"].cpu(), 1e-6, what="train step silhouette")
    ts.forward_backward(x, y, noise=z0, N=N, sil_w=W)
    G_off = ts.G.clone()
    ts.forward_backward(x, dict(y, object_mask=torch.zeros_like(y["object_mask"])), noise=z0, N=N, sil_w=W, sil_occluder=True)
    assert not torch.equal(G, G_off) and torch.equal(ts.G, G_off) and torch.isfinite(G).all()
    # the autograd bridge
    ts.attach()
    model.zero_grad()
    out = model.get_loss(x, y, N=N, noise=z0, sil_w=W, sil_occluder=True)
    assert out["log_p"].requires_grad and list(out)[-1] == "silhouette"
    (-out["log_p"]).mean().backward()
    assert_close(out["silhouette"].detach().cpu(), ref["silhouette"].cpu(), 1e-6, what="bridge silhouette")
    assert_close(out["log_p"].detach().cpu(), ref["log_p"].cpu(), 1e-6, what="bridge log_p")
    got = {n: p.grad.clone() for n, p in model.named_parameters()}          # (.grad is a view of the buffer the next reverse pass fills)
    ts.forward_backward(x, y, noise=z0, N=N, sil_w=W, sil_occluder=True)
    for n, p in model.named_parameters():
        assert_close(got[n].cpu(), ts.grad_of(p).cpu(), 1e-5, what=f"d loss / d {n}")
    model._trainer = None
    # graph replay: the occluder is a static input, the two-section list is rebuilt on every replay
    occs = [y["object_mask"], torch.roll(y["object_mask"], 9, 2) & ~y["hand_mask"]]
    eager = []
    for o in occs:
        e = ts.step(x, dict(y, object_mask=o), noise=z0, N=N, sil_w=W, sil_occluder=True)
        eager.append((ts.G.clone(), e["log_p"].clone(), e["silhouette"].clone()))
    assert not torch.equal(eager[0][2], eager[1][2])
    sy = {k: v.clone() for k, v in y.items()}
    gs = GraphedStep(ts, x.clone(), sy, noise=z0, N=N, sil_w=W, sil_occluder=True)
    for i in (0, 1, 0):
        sy["object_mask"].copy_(occs[i])
        o = gs.replay()
        torch.cuda.synchronize()
        assert torch.equal(o["silhouette"], eager[i][2]) and torch.equal(o["log_p"], eager[i][1]) and torch.equal(ts.G, eager[i][0]), i
    assert_close(eager[0][2].cpu(), ref["silhouette"].cpu(), 1e-6, what="step silhouette")


def test_run_main_with_the_occluder(gpu_lib):
    from mhentropy_amd import run
    common = ["--backbone", "resnet18", "--batch", "4", "--hyps", "4", "--hidden", "64", "--flow-steps", "2", "--dtype", "f32", "--epochs", "1",
              "--sil-w", "1", "--sil-occluder"]
    for extra in (["--iters", "3", "--image-size", "96", "--graph", "1"], ["--iters", "2", "--input-pipeline"]):
        log = run.main(common + extra)
        assert len(log) == 1 and np.isfinite(log[0]["loss"]) and all(np.isfinite(v) for v in log[0]["it_losses"]), (extra, log)
    with pytest.raises(SystemExit):
        run.main(["--sil-occluder"])


# ---- selection --------------------------------------------------------------------------------------------------------------------------------
def test_selection_prefers_the_fingers_behind_the_object_only_with_the_occluder(gpu_lib):
    """3 images at S = 16: the visible hand is a palm block of 4 x 4 pixels, the object a block above it.  Hypothesis A covers the palm with 16
    vertices and puts two fingers (8 vertices each) on the object; hypothesis B flattens the hand into the visible blob: the same mesh shrunk
    to half its size around the palm's centre, the fingers folded into it.  Without the occluder A's fingers lie far outside the mask and B
    wins; with it they cost nothing and B pays for the palm pixels it no longer covers.  The order is checked against the reference's
    distances: plain (A, B) about (0.26, 0.09), occlusion-aware about (0.016, 0.09)"""
    S, Bn = 16, 3
    mask, occ = np.zeros((Bn, S, S), bool), np.zeros((Bn, S, S), bool)
    rng = np.random.default_rng(5)
    verts = np.zeros((2, Bn, 32, 3), np.float32)
    for b in range(Bn):
        mask[b, 9:13, 5 + b:9 + b] = True          # the palm: 4 x 4 pixels
        occ[b, 1:9, 4 + b:11 + b] = True           # the object above it
        cx = lambda j: (2 * j + 1) / S - 1
        palm = np.array([[cx(j), cx(i)] for i in range(9, 13) for j in range(5 + b, 9 + b)])
        jit = rng.uniform(-0.3, 0.3, (16, 2)) / S          # off the centres: no exact ties
        fingers = np.array([[cx(5 + b + f), cx(i) + 0.01] for f in (1, 3) for i in range(1, 9)])          # two columns, up over the object
        folded = palm[rng.integers(0, 16, 16)] + rng.uniform(-0.4, 0.4, (16, 2)) / S
        centre = palm.mean(0)
        verts[0, b, :16, :2], verts[0, b, 16:, :2] = palm + jit, fingers
        verts[1, b, :16, :2], verts[1, b, 16:, :2] = centre + 0.5 * (palm + jit - centre), centre + 0.5 * (folded - centre)
    logs_t = np.zeros((2, Bn, 3), np.float32)
    d_off = so.silhouette(verts, logs_t, mask, np.zeros_like(occ), S)["dist"]
    d_on = so.silhouette(verts, logs_t, mask, occ, S)["dist"]
    assert (d_off[1] < 0.9 * d_off[0]).all() and (d_on[0] < 0.9 * d_on[1]).all()          # B without the occluder, A with it - by a margin f32 keeps
    out = {"verts": _cu(verts.reshape(2, Bn, -1)), "logs_t": _cu(logs_t)}
    y = {"hand_mask": _cu(mask), "object_mask": _cu(occ)}
    plain = criteria.silhouette_select(out, y, Q=1, size=S)
    aware = criteria.silhouette_select(out, y, Q=1, size=S, occluder=True)
    given = criteria.silhouette_select(out, y, Q=2, size=S, occluder=y["object_mask"])
    assert plain["silhouette_index"].tolist() == [[1, 1, 1]] and aware["silhouette_index"].tolist() == [[0, 0, 0]]
    assert given["silhouette_index"].tolist() == [[0, 0, 0], [1, 1, 1]]
    assert sr.rel_dev(plain["silhouette"].cpu().numpy(), d_off[1:2]) <= so.FWD_RTOL
    assert sr.rel_dev(given["silhouette"].cpu().numpy(), d_on) <= so.FWD_RTOL
    assert torch.equal(aware["verts"], out["verts"][0:1]) and torch.equal(plain["verts"], out["verts"][1:2])
