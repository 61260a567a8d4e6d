"""Float64 restatement of the silhouette distance (mhentropy_amd.criteria.silhouette_dist; the contract at mhe_silhouette_* in include/mhe.h),
its torch autograd gradient, and the seeded inputs of the silhouette tests.  A helper module, not a test.  Written from the definition - dense
(V, S*S) distance matrices and torch.min - independently of the kernel's algorithm:

    p_v = exp(log s) v_xy + t;  pixel (i, j): centre c = ((2j+1)/S - 1, (2i+1)/S - 1), the square of half-width 1/S around it
    M_b = the pixels of the (S, S) box average of hand_mask[b] with a mean >= 0.5, in row-major order
    inside = mean_v min_m sqrt(max(|p_vx - c_mx| - 1/S, 0)^2 + max(|p_vy - c_my| - 1/S, 0)^2),  cover = mean_m min_v |c_m - p_v|
    dist = inside + cover;  0 for an empty M_b;  NaN for a row with a non-finite p_v

Inputs are float32 values (what the GPU reads); `dtype` chooses the precision they are evaluated in: float64 is the yardstick, float32 (the same
expressions on the CPU) measures what f32 arithmetic alone costs - the tests allow the kernel four times that."""
import functools

import numpy as np
import torch


def pixel_list(mask, S):
    """mask (B, H, H) bool or float numpy -> (pixels (B, S*S) int32: (i << 16) | j of the kept pixels in row-major order, then -1; count (B,) int32)"""
    m = torch.as_tensor(np.array(mask)).to(torch.float64)
    B, H = m.shape[:2]
    assert H % S == 0 and m.shape[2] == H
    k = H // S
    keep = (m.view(B, S, k, S, k).mean((2, 4)) >= 0.5).numpy()
    pixels = np.full((B, S * S), -1, np.int32)
    count = np.zeros(B, np.int32)
    for b in range(B):
        i, j = np.nonzero(keep[b])          # row-major
        count[b] = len(i)
        pixels[b, :len(i)] = (i.astype(np.int32) << 16) | j.astype(np.int32)
    return pixels, count


def centres(pixels_b, count_b, S, dtype):
    """(|M_b|, 2) centres (x, y) of one image's kept pixels"""
    p = torch.as_tensor(np.asarray(pixels_b[:int(count_b)], np.int64))
    i, j = p >> 16, p & 0xffff
    return torch.stack([(2 * j + 1).to(dtype) / S - 1, (2 * i + 1).to(dtype) / S - 1], -1)


def _norm(q):
    """sqrt(q) with a zero (not 0/0) derivative at q = 0"""
    pos = q > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q))


def project(verts, logs_t, dtype):
    """verts (..., V, 3), logs_t (..., 3) -> p (..., V, 2)"""
    return torch.exp(logs_t[..., None, 0:1]) * verts[..., :2] + logs_t[..., None, 1:]


def box_matrix(p, c, S):
    """p (..., V, 2), c (M, 2) -> (..., V, M) distances to the pixel squares"""
    a = ((p[..., :, None, :] - c).abs() - 1.0 / S).clamp(min=0)
    return _norm((a * a).sum(-1))


def centre_matrix(p, c):
    """-> (..., V, M) distances to the pixel centres"""
    d = p[..., :, None, :] - c
    return _norm((d * d).sum(-1))


def silhouette(verts, logs_t, mask, S, dtype=torch.float64):
    """verts (N,B,V,3), logs_t (N,B,3), mask (B,H,H) numpy -> dict of numpy arrays: dist / inside / cover (N,B), idx_v (N,B,V) (position in the
    image's pixel list; -1 for an empty list), idx_m (N,B,S*S) (-1 past the count), pixels, count, and d_v (N,B,V) / d_m (N,B,S*S): the minima
    themselves (0 where there is none)"""
    v = torch.as_tensor(np.array(verts)).to(dtype)
    lt = torch.as_tensor(np.array(logs_t)).to(dtype)
    N, B, V = v.shape[:3]
    pixels, count = pixel_list(mask, S)
    out = {k: np.zeros((N, B)) for k in ("dist", "inside", "cover")}
    out.update(idx_v=np.full((N, B, V), -1, np.int32), idx_m=np.full((N, B, S * S), -1, np.int32), d_v=np.zeros((N, B, V)), d_m=np.zeros((N, B, S * S)),
               pixels=pixels, count=count)
    p = project(v, lt, dtype)
    bad = ~torch.isfinite(p).all(-1).all(-1).numpy()          # (N, B)
    for b in range(B):
        M = int(count[b])
        if M:
            c = centres(pixels[b], M, S, dtype)
            dv, iv = box_matrix(p[:, b], c, S).min(-1)          # first occurrence: the lowest index on a tie
            dm, im = centre_matrix(p[:, b], c).min(-2)
            out["inside"][:, b], out["cover"][:, b] = dv.mean(-1).numpy(), dm.mean(-1).numpy()
            out["idx_v"][:, b], out["idx_m"][:, b, :M] = iv.numpy(), im.numpy()
            out["d_v"][:, b], out["d_m"][:, b, :M] = dv.numpy(), dm.numpy()
    for k in ("inside", "cover"):
        out[k][bad] = np.nan
    out["dist"] = out["inside"] + out["cover"]
    return out


def attained(verts, logs_t, pixels, count, idx_v, idx_m, S):
    """the f64 distances at GIVEN indices: (d_v (N,B,V), d_m (N,B,S*S)), 0 where the list is empty / past the count"""
    v = torch.as_tensor(np.asarray(verts, np.float64))
    lt = torch.as_tensor(np.asarray(logs_t, np.float64))
    N, B, V = v.shape[:3]
    p = project(v, lt, torch.float64)
    d_v, d_m = np.zeros((N, B, V)), np.zeros((N, B, S * S))
    for b in range(B):
        M = int(count[b])
        if M:
            c = centres(pixels[b], M, S, torch.float64)
            iv = torch.as_tensor(np.asarray(idx_v[:, b], np.int64))
            im = torch.as_tensor(np.asarray(idx_m[:, b, :M], np.int64))
            assert 0 <= int(iv.min()) and int(iv.max()) < M and 0 <= int(im.min()) and int(im.max()) < V, "index out of range"
            d_v[:, b] = torch.gather(box_matrix(p[:, b], c, S), 2, iv[..., None])[..., 0].numpy()
            d_m[:, b, :M] = torch.gather(centre_matrix(p[:, b], c), 1, im[:, None, :])[:, 0].numpy()
    return d_v, d_m


def _total(v, lt, pixels, count, S, g, idx=None):
    """sum g dist as a differentiable torch scalar; idx = (idx_v, idx_m): the minima are taken at those indices instead of by torch.min.
    Images with an empty list contribute nothing"""
    dtype = v.dtype
    p = project(v, lt, dtype)
    total = torch.zeros((), dtype=dtype)
    for b in range(v.shape[1]):
        M = int(count[b])
        if not M:
            continue
        c = centres(pixels[b], M, S, dtype)
        box, cen = box_matrix(p[:, b], c, S), centre_matrix(p[:, b], c)
        if idx is None:
            dv, dm = box.min(-1)[0], cen.min(-2)[0]
        else:
            dv = torch.gather(box, 2, torch.as_tensor(np.asarray(idx[0][:, b], np.int64))[..., None])[..., 0]
            dm = torch.gather(cen, 1, torch.as_tensor(np.asarray(idx[1][:, b, :M], np.int64))[:, None, :])[:, 0]
        total = total + (g[:, b] * (dv.mean(-1) + dm.mean(-1))).sum()
    return total


def grad(verts, logs_t, mask, S, g_dist, idx=None, dtype=torch.float64):
    """d sum(g_dist * dist) / d (verts, logs_t) by torch autograd -> (g_verts (N,B,V,3), g_logs_t (N,B,3)) numpy; idx as in _total.  A row with
    a non-finite projected vertex gets a zero gradient (it is taken out before autograd sees it: 0 * NaN would be NaN)"""
    v = torch.as_tensor(np.array(verts)).to(dtype)
    lt = torch.as_tensor(np.array(logs_t)).to(dtype)
    g = torch.as_tensor(np.array(g_dist)).to(dtype)
    ok = torch.isfinite(project(v, lt, dtype)).all(-1).all(-1)
    v = torch.where(ok[..., None, None], v, torch.zeros_like(v)).requires_grad_(True)
    lt = torch.where(ok[..., None], lt, torch.zeros_like(lt)).requires_grad_(True)
    pixels, count = pixel_list(mask, S)
    total = _total(v, lt, pixels, count, S, torch.where(ok, g, torch.zeros_like(g)), idx)
    if not total.requires_grad:
        return np.zeros(v.shape), np.zeros(lt.shape)
    gv, gl = torch.autograd.grad(total, (v, lt))
    return gv.numpy(), gl.numpy()


def brute(verts, logs_t, mask, S):
    """the definition once more, as plain Python loops over rows, vertices and pixels in float64 (tiny inputs only) -> (dist, inside, cover,
    idx_v, idx_m) shaped as silhouette()'s"""
    import math
    verts, logs_t, mask = np.asarray(verts, np.float64), np.asarray(logs_t, np.float64), np.asarray(mask, np.float64)
    N, B, V = verts.shape[:3]
    k = mask.shape[1] // S
    dist, inside, cover = np.zeros((N, B)), np.zeros((N, B)), np.zeros((N, B))
    idx_v, idx_m = np.full((N, B, V), -1, np.int32), np.full((N, B, S * S), -1, np.int32)
    for b in range(B):
        kept = [(i, j) for i in range(S) for j in range(S) if mask[b, i * k:(i + 1) * k, j * k:(j + 1) * k].sum() / (k * k) >= 0.5]
        cs = [((2 * j + 1) / S - 1, (2 * i + 1) / S - 1) for i, j in kept]
        for n in range(N):
            s = math.exp(logs_t[n, b, 0])
            ps = [(s * verts[n, b, v, 0] + logs_t[n, b, 1], s * verts[n, b, v, 1] + logs_t[n, b, 2]) for v in range(V)]
            if not all(math.isfinite(x) and math.isfinite(y) for x, y in ps):
                dist[n, b] = inside[n, b] = cover[n, b] = np.nan
                continue
            if not cs:
                continue
            for v, (x, y) in enumerate(ps):
                best = math.inf
                for m, (cx, cy) in enumerate(cs):
                    d = math.hypot(max(abs(x - cx) - 1 / S, 0.0), max(abs(y - cy) - 1 / S, 0.0))
                    if d < best:
                        best, idx_v[n, b, v] = d, m
                inside[n, b] += best / V
            for m, (cx, cy) in enumerate(cs):
                best = math.inf
                for v, (x, y) in enumerate(ps):
                    d = math.hypot(cx - x, cy - y)
                    if d < best:
                        best, idx_m[n, b, m] = d, v
                cover[n, b] += best / len(cs)
            dist[n, b] = inside[n, b] + cover[n, b]
    return dist, inside, cover, idx_v, idx_m


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------
def blob_mask(rng, B, H, kind="blob", k=1):
    """(B, H, H) bool masks: 'blob' = a palm ellipse and three finger bars around a drawn centre (a hand-sized region, touching no border as a
    rule), 'full', 'empty', 'corner' (the k x k box in the corner (0, H-1): one grid pixel at H = S k), 'borders' (a cross that touches all four borders)"""
    yy, xx = np.mgrid[0:H, 0:H]
    x, y = (2 * xx + 1) / H - 1, (2 * yy + 1) / H - 1
    out = np.zeros((B, H, H), bool)
    for b in range(B):
        if kind == "full":
            out[b] = True
        elif kind == "corner":
            out[b, :k, H - k:] = True
        elif kind == "borders":
            out[b] = (np.abs(x - 0.1) < 0.3) | (np.abs(y + 0.2) < 0.26)
        elif kind == "blob":
            cx, cy, a = rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.3), rng.uniform(0.3, 0.45)
            m = ((x - cx) / a) ** 2 + ((y - cy) / (0.8 * a)) ** 2 < 1
            for f in (-0.6, 0.0, 0.6):
                m |= (np.abs(x - cx - f * a) < 0.14 * a) & (y < cy) & (y > cy - 1.9 * a)
            out[b] = m
    return out


@functools.lru_cache(None)
def make_case(seed, N, B, V, S, k=1, kind="blob", spread=0.45, mask_float=False, inside_only=False, nan_row=None, empty_image=None):
    """seeded inputs: masks (B, S k, S k) of `kind` (float: the bool mask times a drawn value in {0.25, 0.5, 0.75, 1} per pixel, exact box
    sums), vertices drawn around the origin with `spread` (at 0.45 and a camera scale near 1.3 part of them lands outside the image),
    cameras (log s, t) near (log 1.3, 0).  inside_only: every projected vertex sits inside a kept pixel square (the mask is then 'full' or
    the vertices are drawn on kept pixels).  nan_row = (n, b): vertex 0 of that row is NaN.  empty_image = b: that image's mask is empty.
    Returns a dict of read-only numpy arrays: verts (N,B,V,3) f32, logs_t (N,B,3) f32, mask (B,H,H)."""
    rng = np.random.default_rng(seed)
    H = S * k
    mask = blob_mask(rng, B, H, kind)
    if empty_image is not None:
        mask[empty_image] = False
    logs_t = np.concatenate([np.log(1.3) + rng.normal(0, 0.15, (N, B, 1)), rng.normal(0, 0.12, (N, B, 2))], -1).astype(np.float32)
    verts = rng.normal(0, spread, (N, B, V, 3)).astype(np.float32)
    if inside_only:
        pixels, count = pixel_list(mask, S)
        for b in range(B):
            c = centres(pixels[b], count[b], S, torch.float64).numpy()
            pick = rng.integers(0, len(c), (N, V))
            p = c[pick] + rng.uniform(-0.9, 0.9, (N, V, 2)) / S
            verts[:, b, :, :2] = ((p - logs_t[:, b, None, 1:].astype(np.float64)) / np.exp(logs_t[:, b, None, 0:1].astype(np.float64))).astype(np.float32)
    if nan_row is not None:
        verts[nan_row[0], nan_row[1], 0, 0] = np.nan
    mask_out = mask
    if mask_float:
        mask_out = (mask * rng.choice([0.25, 0.5, 0.75, 1.0], mask.shape)).astype(np.float32)
    case = {"verts": verts, "logs_t": logs_t, "mask": mask_out}
    for a in case.values():
        a.setflags(write=False)
    return case


# (seed, N, B, V, S) + options of make_case: the shapes of the GPU tests, shared with the CPU test that verifies the choice of seeds
CASES = {
    "v1_s8_one_row": dict(seed=201, N=1, B=1, V=1, S=8),
    "v5_s8_float_mask_2x": dict(seed=202, N=3, B=1, V=5, S=8, k=2, mask_float=True),
    "v65_s8_35_rows": dict(seed=203, N=7, B=5, V=65, S=8, nan_row=(2, 1), empty_image=3),
    "v64_s64_3_rows": dict(seed=204, N=1, B=3, V=64, S=64),
    "v778_s64_35_rows": dict(seed=205, N=7, B=5, V=778, S=64, nan_row=(4, 2)),
    "v778_s64_full_mask_all_inside": dict(seed=206, N=1, B=1, V=778, S=64, kind="full", inside_only=True),
    "v65_s64_all_inside_blob": dict(seed=207, N=3, B=1, V=65, S=64, k=2, inside_only=True),
}
MISMATCH_CAP = 0.01          # share of argmin entries that may differ from the f64 argmin (each of them a near-tie)


def g_dist_of(name, shape):
    rng = np.random.default_rng(len(name) + 11)
    return (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


@functools.lru_cache(None)
def reference(name):
    """(case, f64 silhouette() of it), computed once and shared"""
    kw = CASES[name]
    case = make_case(**kw)
    return case, silhouette(case["verts"], case["logs_t"], case["mask"], kw["S"])


def rel_dev(a, b):
    """max |a - b| relative to max |b| over the finite entries of b; NaN must sit in the same places"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN in different places"
    ok = ~np.isnan(b)
    scale = np.abs(b[ok]).max() if ok.any() else 0.0
    return float(np.abs(a[ok] - b[ok]).max() / scale) if scale > 0 else float(np.abs(a[ok]).max() if ok.any() else 0.0)


def index_report(name, idx_v, idx_m):
    """indices against the f64 restatement: (share of entries that differ from the f64 argmin, the largest excess of the f64 distance at the
    given index over the f64 minimum, relative to the largest minimum of the case).  Rows that are NaN in f64 are left out."""
    case, ref = reference(name)
    S = CASES[name]["S"]
    d_v, d_m = attained(np.nan_to_num(case["verts"]), case["logs_t"], ref["pixels"], ref["count"], idx_v, idx_m, S)
    good = ~np.isnan(ref["dist"])
    scale = max(ref["d_v"][good].max(), ref["d_m"][good].max())
    diff = int((idx_v != ref["idx_v"])[good].sum() + (idx_m != ref["idx_m"])[good].sum())
    excess = max((d_v - ref["d_v"])[good].max(), (d_m - ref["d_m"])[good].max())
    return diff / float(good.sum() * (idx_v.shape[-1] + idx_m.shape[-1])), float(excess / scale) if scale > 0 else float(excess)


@functools.lru_cache(None)
def f32_deviation(name):
    """what f32 arithmetic alone costs on this case: the restatement evaluated in float32 on the CPU against float64 ->
    (forward: the largest rel_dev of dist / inside / cover, reverse: the largest rel_dev of g_verts / g_logs_t with both gradients taken at the
    f64 indices, index mismatch share, index excess)"""
    kw = CASES[name]
    case, ref = reference(name)
    lo = silhouette(case["verts"], case["logs_t"], case["mask"], kw["S"], torch.float32)
    fwd = max(rel_dev(lo[k], ref[k]) for k in ("dist", "inside", "cover"))
    g = g_dist_of(name, ref["dist"].shape)
    idx = (np.maximum(ref["idx_v"], 0), np.maximum(ref["idx_m"], 0))
    hi_g = grad(case["verts"], case["logs_t"], case["mask"], kw["S"], g, idx)
    lo_g = grad(case["verts"], case["logs_t"], case["mask"], kw["S"], g, idx, torch.float32)
    rev = max(rel_dev(a, b) for a, b in zip(lo_g, hi_g))
    share, excess = index_report(name, lo["idx_v"], lo["idx_m"])
    return fwd, rev, share, excess


# Bounds.  f32_deviation() of every case, measured once on a CPU (torch 2.x, float32 against float64; DESIGN.md has the table): forward
# 7.4e-8, 9.0e-8, 1.30e-7, 7.3e-8, 1.36e-7, 1.8e-8, 1.43e-7 in the order of CASES; reverse as below.  The kernel is allowed four times the f32
# restatement's deviation - the margin covers the different summation order.  Forward: four times the LARGEST case's, for every case: one
# case's deviation can be lucky (1.8e-8 is below the half ulp, 3e-8 .. 6e-8, of the f32 number the result is returned as), the largest is what
# f32 evaluation of these expressions costs.  Reverse: four times the case's own (the gradient's conditioning differs by case: a unit vector
# over a distance of a pixel or less amplifies the rounding of p by 1 / distance), but never less than the forward's.
F32_FWD_DEV = 1.44e-7
F32_REV_DEV = {"v1_s8_one_row": 1.03e-7, "v5_s8_float_mask_2x": 5.4e-8, "v65_s8_35_rows": 1.41e-6, "v64_s64_3_rows": 2.64e-7,
               "v778_s64_35_rows": 2.13e-6, "v778_s64_full_mask_all_inside": 2.31e-5, "v65_s64_all_inside_blob": 1.82e-6}
FWD_RTOL = 4 * F32_FWD_DEV
REV_RTOL = {k: 4 * max(v, F32_FWD_DEV) for k, v in F32_REV_DEV.items()}
