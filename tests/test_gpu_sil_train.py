"""GPU: training with the silhouette term, get_loss(sil_w=...), through every layer - mhe_silhouette_dist_grad_f32 (forward and reverse of a
row in one launch, the argmins in registers and LDS) against the two-launch path it replaces, bit for bit; mhe_mano_z_grad_add_f32 against
torch slicing; the module, the train step against f64 autograd of the oracle + tests/mano_bwd_ref.py + tests/silhouette_ref.py, the autograd
bridge, graph replay, the Glow branch, run.py and the refusal under hypothesis sharding.
Tolerances: 1e-4 values, 2e-4 parameter gradients through TrainStep (those of tests/test_gpu_chamfer_train.py, BASELINE.json's north star)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mano_bwd_ref
import silhouette_ref as sr
from conftest import assert_close
from mhentropy_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # BASELINE.json north_star: 1e-4 relative, fp32
B, N = 2, 3
W = 10.0         # the term is then a visible part (> 1 %) of the gradients under test
DUP = 2            # the vertex of case v65_s16_duplicate_vertices that most kept pixels choose (checked where the case is made)


def _dev(a):
    return torch.as_tensor(np.array(a)).cuda()


def _same(a, b):
    """torch.equal with NaNs compared by position"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def _count_mask(S, n):
    """(1, S, S) bool with the first n pixels in row-major order"""
    m = np.zeros(S * S, bool)
    m[:n] = True
    return m.reshape(1, S, S)


# name -> (make_case keywords, mask override (B, H, H) | None, count override | None).  V: the ownership boundary v mod 256 / v / 256 and the
# idle slots; S and the counts: the LDS list full (four rounds of 1,024), one pixel, a one-pixel second round; rows of different images side
# by side; a NaN row, an empty image, counts outside 0 .. S^2 (clamped on the device).
EXTRA = {
    "v1_s1": (dict(seed=301, N=1, B=1, V=1, S=1, kind="full"), None, None),
    "v255_s16": (dict(seed=302, N=5, B=2, V=255, S=16), None, None),
    "v256_s16": (dict(seed=303, N=1, B=1, V=256, S=16), None, None),
    "v257_s16_nan_empty": (dict(seed=304, N=7, B=3, V=257, S=16, nan_row=(3, 1), empty_image=2), None, None),
    "v778_s64_full": (dict(seed=305, N=1, B=1, V=778, S=64, kind="full"), None, None),
    "v778_s64_one_pixel": (dict(seed=306, N=1, B=1, V=778, S=64, kind="corner"), None, None),
    "v257_s64_count_1025": (dict(seed=307, N=1, B=1, V=257, S=64), _count_mask(64, 1025), None),
    "v778_s64_5x2": (dict(seed=308, N=5, B=2, V=778, S=64), None, None),
    "v65_s16_count_out_of_range": (dict(seed=309, N=3, B=3, V=65, S=16, kind="full"), None, [1 << 20, -3, 256]),
    "v65_s16_duplicate_vertices": (dict(seed=310, N=3, B=2, V=65, S=16), None, None),          # exact ties: vertices 63 and 64 are vertex DUP
}


@functools.lru_cache(None)
def _operands(name):
    kw = sr.CASES[name] if name in sr.CASES else EXTRA[name][0]
    case = sr.make_case(**kw)
    mask, count_over = (None, None) if name in sr.CASES else EXTRA[name][1:]
    verts = case["verts"]
    if name.endswith("duplicate_vertices"):          # the last two vertices become copies of DUP, the vertex most pixels choose (f64)
        im = sr.silhouette(verts, case["logs_t"], case["mask"], kw["S"])["idx_m"]
        assert np.bincount(im[im >= 0], minlength=63)[:63].argmax() == DUP
        verts = verts.copy()
        verts[:, :, 63] = verts[:, :, 64] = verts[:, :, DUP]
    return kw, verts, case["logs_t"], case["mask"] if mask is None else mask, count_over


def _gpu_operands(name):
    from mhentropy_amd import ops
    kw, verts, logs_t, mask, count_over = _operands(name)
    pixels, count = ops.silhouette_pixels(_dev(mask), kw["S"])
    if count_over is not None:
        count = _dev(np.asarray(count_over, np.int32))
    g = _dev(sr.g_dist_of(name, verts.shape[:2]))
    return kw, _dev(verts), _dev(logs_t), pixels, count, g


@pytest.mark.parametrize("name", list(sr.CASES) + list(EXTRA))
def test_fused_kernel_equals_the_two_launch_path_bit_for_bit(gpu_lib, name):
    """dist, g_verts, g_logs_t of mhe_silhouette_dist_grad_f32 are torch.equal to mhe_silhouette_dist_f32 (with indices) followed by
    mhe_silhouette_dist_bwd_f32; dist = NULL gives the same gradients; two calls give the same bits"""
    from mhentropy_amd import ops
    kw, verts, logs_t, pixels, count, g = _gpu_operands(name)
    dist, _, idx_v, idx_m = ops.silhouette_dist(verts, logs_t, pixels, count, want_idx=True)
    gv, gl = ops.silhouette_dist_bwd(verts, logs_t, pixels, count, idx_v, idx_m, g)
    d2, gv2, gl2 = ops.silhouette_dist_grad(verts, logs_t, pixels, count, g, want_dist=True)
    assert _same(d2, dist), (name, "dist", (d2 - dist).abs().max())
    assert _same(gv2, gv), (name, "g_verts", (gv2 - gv).abs().max())
    assert _same(gl2, gl), (name, "g_logs_t", (gl2 - gl).abs().max())
    assert not torch.isnan(gv2).any() and not torch.isnan(gl2).any() and (gv2[..., 2] == 0).all()
    gv3, gl3 = ops.silhouette_dist_grad(verts, logs_t, pixels, count, g)
    assert torch.equal(gv3, gv2) and torch.equal(gl3, gl2)
    if kw.get("nan_row"):
        n, b = kw["nan_row"]
        assert torch.isnan(d2[n, b]) and torch.isnan(d2).sum() == 1 and not gv2[n, b].any() and not gl2[n, b].any()
    if kw.get("empty_image") is not None:
        e = kw["empty_image"]
        assert not gv2[:, e].any() and not gl2[:, e].any() and (torch.nan_to_num(d2[:, e]) == 0).all()
    if name == "v65_s16_count_out_of_range":          # 2^20 -> 256 = the full list, -3 -> 0 = an empty list
        full = ops.silhouette_dist_grad(verts, logs_t, pixels, torch.full_like(count, 256), g, want_dist=True)
        assert torch.equal(full[0][:, 0], d2[:, 0]) and torch.equal(full[1][:, 0], gv2[:, 0]) and (d2[:, 1] == 0).all() and not gv2[:, 1].any()
    if name in ("v778_s64_full", "v257_s64_count_1025"):
        assert int(count[0]) == (4096 if name == "v778_s64_full" else 1025)
    if name.endswith("duplicate_vertices"):          # the tie rule: the lowest index takes the pixel, its copies get no cover term
        assert (idx_m == DUP).any() and not (idx_m == 63).any() and not (idx_m == 64).any()
        assert not torch.equal(gv2[:, :, DUP], gv2[:, :, 63]) and torch.equal(gv2[:, :, 63], gv2[:, :, 64])
    assert gv2.abs().max() > 0 or name == "v1_s1" or kw.get("inside_only")


def test_fused_kernel_sentinels_graph_and_refusals(gpu_lib):
    """40 rows behind R keep their bits; a captured graph replays the same bits; the argument refusals return MHE_ERR_ARG, outputs untouched"""
    from mhentropy_amd import ops, _lib
    name = "v65_s8_35_rows"
    kw, verts, logs_t, pixels, count, g = _gpu_operands(name)
    Nn, Bn, V, S = kw["N"], kw["B"], kw["V"], kw["S"]
    R = Nn * Bn
    want = ops.silhouette_dist_grad(verts, logs_t, pixels, count, g, want_dist=True)
    outs = [torch.full((R + 40,) + s, -77.25, device="cuda") for s in ((), (V, 3), (3,))]
    ops.launch("mhe_silhouette_dist_grad_f32", verts, logs_t, pixels, count, g, *outs, Nn, Bn, V, S)
    for o, w in zip(outs, want):
        assert _same(o[:R].reshape(w.shape), w) and (o[R:] == -77.25).all()
    # graph replay
    for o in outs:
        o.fill_(3.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.launch("mhe_silhouette_dist_grad_f32", verts, logs_t, pixels, count, g, *outs, Nn, Bn, V, S)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for o in outs:
            o.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            assert _same(o[:R].reshape(w.shape), w) and (o[R:] == 3.0).all()
    # refusals: status 1 (MHE_ERR_ARG), nothing written
    L = _lib.lib()
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    good = [verts, logs_t, pixels, count, g] + outs
    calls = []
    for i in (0, 1, 2, 3, 4, 6, 7):
        a = list(good); a[i] = None
        calls.append((a, (Nn, Bn, V, S)))
    calls += [(good, s) for s in ((0, Bn, V, S), (Nn, 0, V, S), (Nn, Bn, 0, S), (Nn, Bn, 779, S), (Nn, Bn, V, 0), (Nn, Bn, V, 65))]
    for i, j in ((6, 0), (7, 1), (5, 4), (6, 7), (5, 7)):
        a = list(good); a[i] = good[j]
        calls.append((a, (Nn, Bn, V, S)))
    for o in outs:
        o.fill_(5.0)
    before = [t.clone() for t in good]
    for a, s in calls:
        assert L.mhe_silhouette_dist_grad_f32(*[p(t) for t in a], *s, None) == 1, (s, L.mhe_last_error())
    torch.cuda.synchronize()
    for t, b4 in zip(good, before):
        assert _same(t.float(), b4.float())


@pytest.mark.parametrize("R", [1, 63, 64, 65, 257])
def test_z_grad_add_against_torch_slicing(gpu_lib, R):
    from mhentropy_amd import ops
    gen = torch.Generator().manual_seed(R)
    gz, gl, g45, gd = (torch.randn(R + 3, c, generator=gen).cuda() for c in (61, 3, 45, 16))
    for with_l in (True, False):
        a45, ad = g45.clone(), gd.clone()
        ops.mano_z_grad_add(gz[:R], gl[:R] if with_l else None, a45[:R], ad[:R])
        w45, wd = g45.clone(), gd.clone()
        w45[:R] += gz[:R, 3:48]
        wd[:R, 0:3] += gz[:R, 0:3]
        wd[:R, 3:13] += gz[:R, 48:58]
        if with_l:
            wd[:R, 13:16] += gl[:R]
        assert torch.equal(a45, w45) and torch.equal(ad, wd), (R, with_l)          # (rows R .. R+2 are the guard rows)
        if not with_l:
            assert torch.equal(ad[:, 13:], gd[:, 13:])


def _small_model():
    from test_gpu_train import _model_and_state
    return _model_and_state("resnet18", 64, 2)


def _batch(seed=3, Bn=B, image_size=96, H=64):
    xn, yn = synth.batch(seed, Bn, image_size=image_size)
    yn["hand_mask"] = synth.hand_masks(seed, Bn, H=H, crop_uv=yn["crop_uv"])
    return torch.as_tensor(xn).cuda(), {k: torch.as_tensor(v).cuda() for k, v in yn.items()}


@pytest.mark.parametrize("size", [16, 64])
def test_term_off_is_bit_equal_and_term_on_touches_log_p_only(gpu_lib, size):
    """sil_w = 0 through the new argument: torch.equal outputs and gradients, no 'silhouette' key.  sil_w > 0: q_log_p_z_giv_y, h_q_z_giv_i,
    th_norm and bt_norm torch.equal to the term-off run with the same noise, log_p lower by w silhouette (1e-6 relative), silhouette = mean
    over n of criteria.silhouette_dist of the sampled meshes.  Module and train step; both terms on."""
    from mhentropy_amd import criteria
    from mhentropy_amd.train import TrainStep
    model, _ = _small_model()
    model.sil_size = size
    x, y = _batch()
    y.update({k: torch.as_tensor(v).cuda() for k, v in synth.object_targets(3, B, VO=40, with_count=True).items()})
    z0 = torch.as_tensor(synth.noise(3, N * B)).cuda()
    ts = TrainStep(model)
    for mods in (["uv"], ["xyz", "uv"]):
        with torch.no_grad():
            base = model.get_loss(x, y, mods=mods, N=N, noise=z0)
            off = model.get_loss(x, y, mods=mods, N=N, noise=z0, sil_w=0.0)
            on = model.get_loss(x, y, mods=mods, N=N, noise=z0, sil_w=W)
            both = model.get_loss(x, y, mods=mods, N=N, noise=z0, sil_w=W, chamfer_w=10.0)
            cham = model.get_loss(x, y, mods=mods, N=N, noise=z0, chamfer_w=10.0)
        assert set(off) == set(base) and "silhouette" not in off and set(on) == set(base) | {"silhouette"}
        for k in base:
            assert torch.equal(base[k], off[k]), k
        for k in ("q_log_p_z_giv_y", "h_q_z_giv_i", "th_norm", "bt_norm"):
            assert torch.equal(base[k], on[k]) and torch.equal(base[k], both[k]), k
        assert on["silhouette"].shape == (B,) and (on["silhouette"] > 1e-3).all()
        assert_close(on["log_p"].cpu(), (base["log_p"] - W * on["silhouette"]).cpu(), 1e-6, what="log_p")
        assert torch.equal(both["silhouette"], on["silhouette"]) and torch.equal(both["chamfer"], cham["chamfer"])
        assert_close(both["log_p"].cpu(), (base["log_p"] - 10.0 * both["chamfer"] - W * both["silhouette"]).cpu(), 1e-6, what="both terms")
        with torch.no_grad():
            s = model.sample(x, N=N, temp=1.0, noise=z0, mods=["verts"])
            want = criteria.silhouette_dist(s["verts"], s["logs_t"], y["hand_mask"], size).mean(0)
        assert_close(on["silhouette"].cpu(), want.cpu(), RTOL, what="silhouette vs silhouette_dist")
        tb = ts.forward_backward(x, y, noise=z0, N=N, mods=mods)
        Gb = ts.G.clone()
        to = ts.forward_backward(x, y, noise=z0, N=N, mods=mods, sil_w=0.0)
        assert "silhouette" not in to and torch.equal(ts.G, Gb)
        for k in tb:
            assert torch.equal(tb[k], to[k]), k
        tn = ts.forward_backward(x, y, noise=z0, N=N, mods=mods, sil_w=W)
        assert not torch.equal(ts.G, Gb) and torch.isfinite(ts.G).all()
        for k in ("q_log_p_z_giv_y", "h_q_z_giv_i", "th_norm", "bt_norm"):
            assert torch.equal(tb[k], tn[k]), k
        assert_close(tn["log_p"].cpu(), (tb["log_p"] - W * tn["silhouette"]).cpu(), 1e-6, what="train step log_p")
        assert_close(tn["silhouette"].cpu(), on["silhouette"].cpu(), 1e-6, what="train step silhouette")
        t2 = ts.forward_backward(x, y, noise=z0, N=N, mods=mods, sil_w=W, chamfer_w=10.0)
        assert_close(t2["log_p"].cpu(), (tb["log_p"] - 10.0 * t2["chamfer"] - W * t2["silhouette"]).cpu(), 1e-6, what="train step, both terms")
    model.sil_w = W                      # the attribute is the default of the argument
    with torch.no_grad():
        assert torch.equal(model.get_loss(x, y, mods=mods, N=N, noise=z0)["log_p"], on["log_p"])
    model.sil_w = 0.0
    with pytest.raises(ValueError, match="hand_mask"):
        model.get_loss(x, {k: v for k, v in y.items() if k != "hand_mask"}, N=N, noise=z0, sil_w=W)


def _oracle(sd, names, trunk, z0, y, mods, S, dtype, idx):
    """-mean_b log_p with the term on, from the trunk feature on, in `dtype`: network_ref.reverse_kld -> its z -> the mesh of
    tests/mano_bwd_ref.py -> tests/silhouette_ref.py with the minima taken at the indices idx.  -> (values, (d/d feat, d/d named weights))"""
    import torch.nn.functional as F
    from oracle import mano_ref, network_ref
    sdx = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in sd.items()}
    for n in names:
        sdx[n] = sdx[n].clone().requires_grad_(True)
    yx = {k: (v.cpu().to(dtype) if v.dtype == torch.float32 else v.cpu()) for k, v in y.items()}
    feat = F.linear(torch.as_tensor(trunk).to(dtype), sdx["feat_extractor.l1.0.weight"], sdx["feat_extractor.l1.0.bias"]).requires_grad_(True)
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0), dtype=dtype)
    ref = network_ref.reverse_kld(sdx, tb, feat, yx, torch.as_tensor(z0).to(dtype), N)
    z = ref["_z"]
    if "xyz" in mods:
        xyz = network_ref.decode(tb, z)["xyz"]
        w3 = yx["vis"][..., None].repeat(N, 1, 3).flatten(-2)
        lx = network_ref.laplace_log_prob(yx["pose3d"].repeat(N, 1), xyz.flatten(-2), w3, b=0.03)
        ref["q_log_p_z_giv_y"] = ref["q_log_p_z_giv_y"] + lx.reshape(N, B).mean(0)
        ref["log_p"] = ref["h_q_z_giv_i"] + ref["q_log_p_z_giv_y"]
    verts = mano_bwd_ref.mesh_and_joints(z, False, dtype)[0].reshape(N, B, 778, 3)
    lt = z[:, 58:61].reshape(N, B, 3)
    pixels, count = sr.pixel_list(y["hand_mask"].cpu().numpy(), S)
    sil = torch.stack([sr._total(verts, lt, pixels, count, S, torch.eye(B, dtype=dtype)[b].repeat(N, 1) / N, idx) for b in range(B)])
    log_p = ref["log_p"] - W * sil
    grads = torch.autograd.grad(-log_p.mean(), [feat] + [sdx[n] for n in names])
    vals = {"silhouette": sil.detach(), "log_p": log_p.detach(), "q_log_p_z_giv_y": ref["q_log_p_z_giv_y"].detach(),
            "h_q_z_giv_i": ref["h_q_z_giv_i"].detach(), "verts": verts.detach(), "logs_t": lt.detach()}
    return vals, grads


@pytest.mark.parametrize("mods", [["uv"], ["xyz", "uv"]])
def test_train_step_matches_f64_autograd_of_the_oracle(gpu_lib, mods):
    """TrainStep.forward_backward(None, y, trunk_out=..., sil_w=W), ResNet-18 heads, h = 64, 2 flow steps, grid 16: values (1e-4) and the
    gradients of det_head.2.weight, a first and a last flow layer and g_feat (2e-4) against f64 autograd of the oracle, the gradient taken at
    the argmins the kernel attained on the step's own mesh.  Those indices first: at most MISMATCH_CAP of them differ from the f64 argmin on
    the oracle's mesh, each a near-tie - the positions are bound at RTOL of their scale, so an index chosen on them exceeds the f64 minimum
    by at most 2 RTOL of the largest minimum.  The f32 restatement of the whole chain on the CPU must sit within a quarter of every bound."""
    from mhentropy_amd import ops
    from mhentropy_amd.train import TrainStep
    model, sd = _small_model()
    S = model.sil_size = 16
    steps = 2
    _, y = _batch(seed=8)
    rng = np.random.default_rng(8)
    trunk = rng.normal(0, 0.5, (B, 512)).astype(np.float32)
    z0 = synth.noise(8, N * B)
    names = ("det_head.2.weight", "q_z_giv_i.s.0.l.0.weight", f"q_z_giv_i.t.{2 * steps - 1}.l.2.weight")
    ts = TrainStep(model)
    out = ts.forward_backward(None, y, noise=_dev(z0), N=N, trunk_out=_dev(trunk), mods=mods, sil_w=W)
    G = ts.G.clone()
    t = ts.tape
    got = {n: ts.grad_of(dict(model.named_parameters())[n]).cpu().clone() for n in names}
    g_feat = t["g_feat"].cpu().clone()
    verts, logs_t = t["sil_verts"].view(N, B, 778, 3), t["sil_logs_t"].view(N, B, 3)
    _, _, idx_v, idx_m = ops.silhouette_dist(verts, logs_t, *t["sil"], want_idx=True)
    idx = (idx_v.cpu().numpy(), np.maximum(idx_m.cpu().numpy(), 0))
    # the f64 argmins on the oracle's own mesh, and the kernel's indices against them
    free, _ = _oracle(sd, names, trunk, z0, y, mods, S, torch.float64, None)
    f64 = sr.silhouette(free["verts"].numpy(), free["logs_t"].numpy(), y["hand_mask"].cpu().numpy(), S)
    d_v, d_m = sr.attained(free["verts"].numpy(), free["logs_t"].numpy(), f64["pixels"], f64["count"], idx[0], idx[1], S)
    assert (f64["count"] > 0).all()
    share = float(((idx[0] != f64["idx_v"]).sum() + (idx_m.cpu().numpy() != f64["idx_m"]).sum()) / (idx[0].size + idx[1].size))
    scale = max(f64["d_v"].max(), f64["d_m"].max())
    excess = float(max((d_v - f64["d_v"]).max(), (d_m - f64["d_m"]).max()) / scale)
    print(f"{mods}: kernel argmins vs f64: {share:.5f} differ (cap {sr.MISMATCH_CAP}), excess {excess:.3e} (bound {2 * RTOL:.1e})")
    assert share <= sr.MISMATCH_CAP and excess <= 2 * RTOL, (share, excess)
    ref, grads = _oracle(sd, names, trunk, z0, y, mods, S, torch.float64, idx)
    lo, lo_grads = _oracle(sd, names, trunk, z0, y, mods, S, torch.float32, idx)
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
    for k in ("silhouette", "log_p", "q_log_p_z_giv_y", "h_q_z_giv_i"):
        print(f"{mods} {k}: step {rel(out[k].cpu(), ref[k]):.3e}  f32 restatement {rel(lo[k], ref[k]):.3e}  (bound {RTOL:.0e})")
        assert rel(lo[k], ref[k]) <= RTOL / 4, (k, "the inputs are badly conditioned: choose others")
    for n, a, b in zip(("feat",) + names, lo_grads, grads):
        assert rel(a, b) <= 2e-4 / 4, (n, rel(a, b), "the inputs are badly conditioned: choose others")
    for k in ("silhouette", "log_p", "q_log_p_z_giv_y", "h_q_z_giv_i"):
        assert_close(out[k].cpu(), ref[k], RTOL, what=k)
    for n, gr, lg in zip(names, grads[1:], lo_grads[1:]):
        print(f"{mods} d loss / d {n}: step {rel(got[n], gr):.3e}  f32 restatement {rel(lg, gr):.3e}  (bound 2e-4)")
        assert_close(got[n], gr, 2e-4, what=f"d loss / d {n}")
    print(f"{mods} d loss / d feat: step {rel(g_feat, grads[0]):.3e}  f32 restatement {rel(lo_grads[0], grads[0]):.3e}  (bound 2e-4)")
    assert_close(g_feat, grads[0], 2e-4, what="d loss / d feat")
    # the term is a visible part of the gradient under test
    ts.forward_backward(None, y, noise=_dev(z0), N=N, trunk_out=_dev(trunk), mods=mods)
    assert (ts.tape["g_feat"].cpu() - g_feat).abs().max() > 1e-2 * g_feat.abs().max()
    # two reverse passes on the same inputs: the same bits
    ts.forward_backward(None, y, noise=_dev(z0), N=N, trunk_out=_dev(trunk), mods=mods, sil_w=W)
    assert torch.equal(ts.G, G)


def test_autograd_bridge_equals_the_fused_reverse_pass(gpu_lib):
    """get_loss(sil_w=W) -> total_loss.backward() with a TrainStep attached: .grad equals the explicit reverse pass"""
    from mhentropy_amd.train import TrainStep
    model, _ = _small_model()
    x, y = _batch(Bn=4)
    z0 = torch.as_tensor(synth.noise(3, 6 * 4)).cuda()
    ts = TrainStep(model).attach()
    for mods in (["uv"], ["xyz", "uv"]):
        model.zero_grad()
        out = model.get_loss(x, y, mods=mods, N=6, noise=z0, sil_w=W)
        assert out["log_p"].requires_grad and not out["silhouette"].requires_grad and out["silhouette"].shape == (4,)
        assert list(out)[-1] == "silhouette"
        (-out["log_p"]).mean().backward()
        got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        assert len(got) == len(list(model.parameters()))
        lp = out["log_p"].detach().clone()
        off = model.get_loss(x, y, mods=mods, N=6, noise=z0)
        assert "silhouette" not in off and (off["log_p"].detach() - lp).abs().min() > 1e-3
        ref = ts.forward_backward(x, y, noise=z0, N=6, mods=mods, sil_w=W)
        assert_close(lp.cpu(), ref["log_p"].cpu(), 1e-6, what=f"{mods} log_p")
        for n, p in model.named_parameters():
            assert_close(got[n].cpu(), ts.grad_of(p).cpu(), 1e-5, what=f"{mods} d loss / d {n}")


def test_graphed_step_replays_bit_equal_to_eager(gpu_lib):
    """GraphedStep with the term on (ResNet-18, 128x128, B=8, N=4, lr 0): the replay equals the eager step bit for bit, also after a second
    mask is copied into the captured static batch (the kept-pixel list is rebuilt inside the graph)"""
    from mhentropy_amd.train import TrainStep, GraphedStep
    Bn, Nn, mods = 8, 4, ["xyz", "uv"]
    x, y = _batch(seed=21, Bn=Bn, image_size=128)
    _, y2 = _batch(seed=22, Bn=Bn, image_size=128)
    masks = [y["hand_mask"], y2["hand_mask"]]
    z0 = torch.as_tensor(synth.noise(21, Nn * Bn)).cuda()
    ts = TrainStep(_small_model()[0], lr=0.0)
    eager = []
    for m in masks:
        o = ts.step(x, dict(y, hand_mask=m), noise=z0, N=Nn, mods=mods, sil_w=W)
        eager.append((ts.G.clone(), o["log_p"].clone(), o["total"].clone(), o["silhouette"].clone()))
    assert not torch.equal(eager[0][3], eager[1][3])
    sy = {k: v.clone() for k, v in y.items()}
    gs = GraphedStep(ts, x.clone(), sy, noise=z0, N=Nn, mods=mods, sil_w=W)
    for i in (0, 1, 0):
        sy["hand_mask"].copy_(masks[i])
        o = gs.replay()
        torch.cuda.synchronize()
        G, lp, tot, sl = eager[i]
        assert torch.equal(o["silhouette"], sl) and torch.equal(o["log_p"], lp) and torch.equal(o["total"], tot), i
        assert torch.equal(ts.G, G), i


def test_glow_branch_silhouette_is_the_mean_of_its_rows(gpu_lib):
    """Glow branch (parity unpinned): the step runs with the term on and out['silhouette'] is the per-image mean over N of the row distances
    of the same hypotheses; the term-off keys do not move"""
    from mhentropy_amd import harness, ops
    from mhentropy_amd.network import MHEnt
    from mhentropy_amd.train import TrainStep
    special, common = harness.mhent_cfgs(backbone="resnet18", tables=synth.mano_tables(0))
    special["q_z_giv_i_model"] = "glow"
    model = MHEnt(special, **common)
    model.q_z_giv_i.load_state_dict({k: torch.as_tensor(v) for k, v in synth.glow_state(3).items()}, strict=False)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in synth.head_state(4, 512).items()}, strict=False)
    model = model.cuda().train()
    Nn = 5
    _, y = _batch(seed=5)
    f = _dev(np.random.default_rng(6).normal(0, 0.5, (B, 512)).astype(np.float32))
    noise = _dev(np.random.default_rng(7).normal(0, 1, (B, Nn, 45)).astype(np.float32))
    ts = TrainStep(model)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {}
    for key, w in (("off", 0.0), ("on", W)):
        ops.rng_state(dev, seed=12)                      # the same dropout masks -> the same hypotheses in both runs
        res[key] = ts.forward_backward(None, y, noise=noise, N=Nn, trunk_out=f, sil_w=w)
        res[key + "_G"] = ts.G.clone()
    for k in ("q_log_p_z_giv_y", "h_q_z_giv_i", "th_norm", "bt_norm"):
        assert torch.equal(res["off"][k], res["on"][k]), k
    t = ts.tape
    rows, _ = ops.silhouette_dist(ops.mano_verts(t["z"], t["blob"]).view(Nn, B, 778, 3), t["z"][:, 58:61].contiguous().view(Nn, B, 3), *t["sil"])
    assert_close(res["on"]["silhouette"].cpu(), rows.mean(0).cpu(), 1e-6, what="silhouette")
    assert_close(res["on"]["log_p"].cpu(), (res["off"]["log_p"] - W * res["on"]["silhouette"]).cpu(), 1e-6, what="log_p")
    assert torch.isfinite(res["on_G"]).all() and not torch.equal(res["on_G"], res["off_G"])


def test_run_main_with_sil_w(gpu_lib):
    """python -m mhentropy_amd.run --sil-w 1: eager, replayed from HIP graphs, and fed by the GPU input pipeline"""
    from mhentropy_amd import run
    common = ["--backbone", "resnet18", "--batch", "4", "--hyps", "4", "--hidden", "64", "--flow-steps", "2", "--dtype", "f32", "--epochs", "1",
              "--sil-w", "1"]
    for extra in (["--iters", "2", "--image-size", "96"],
                  ["--iters", "3", "--image-size", "96", "--graph", "1"],
                  ["--iters", "2", "--input-pipeline"]):
        log = run.main(common + extra)
        assert len(log) == 1 and np.isfinite(log[0]["loss"]) and all(np.isfinite(v) for v in log[0]["it_losses"]), (extra, log)


def test_hypothesis_sharding_refuses_the_term(gpu_lib):
    """shard_hypotheses + sil_w > 0: NotImplementedError before any launch (the attribute is enough to reach the check: no second process)"""
    from mhentropy_amd.train import TrainStep
    ts = TrainStep(_small_model()[0])
    x, y = _batch()
    ts.shard_hypotheses = True
    with pytest.raises(NotImplementedError, match="sil_w"):
        ts.forward(x, y, N=N, sil_w=W)
    with pytest.raises(NotImplementedError, match="sil_w"):
        ts.forward_backward(x, y, N=N, sil_w=W)
