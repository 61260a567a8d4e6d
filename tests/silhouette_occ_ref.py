"""Float64 restatement of the occlusion-aware silhouette distance (criteria.silhouette_dist(occluder=...); the contract at the mhe_silhouette_*_occ
entries in include/mhe.h), its torch autograd gradient, and the seeded inputs of its tests.  A helper module, not a test; the pair evaluations,
the projection and the input generators are those of tests/silhouette_ref.py.  Dense matrices and torch.min, independent of the kernel:

    M_b = the kept pixels of hand_mask[b] (box mean >= 0.5), row-major;  O_b = the kept pixels of occluder[b] that are not in M_b, row-major
    list_b = M_b, then O_b, then -1;  count = |M_b|, count_all = |M_b| + |O_b|
    inside = mean_v min_{m in M_b u O_b} box(p_v, c_m)   (ties to the lowest list position: a hand pixel wins over an occluder pixel)
    cover  = mean_{m in M_b} min_v |c_m - p_v|,   dist = inside + cover
    |M_b| = 0: everything 0 whatever O_b holds;  a non-finite p_v: the row is NaN

`dtype` chooses the precision of the evaluation: float64 is the yardstick, float32 (the same expressions on the CPU) measures what f32
arithmetic alone costs - the tests allow the kernel four times that, the margin tests/test_gpu_silhouette.py allows the kernel without occluder."""
import functools

import numpy as np
import torch

import silhouette_ref as sr


def pixel_list(mask, occluder, S):
    """mask, occluder (B, H, H) bool / uint8 / float numpy -> (pixels (B, S*S) int32, count (B,), count_all (B,))"""
    hand, n_hand = sr.pixel_list(np.asarray(mask) != 0 if np.asarray(mask).dtype != np.float32 else mask, S)
    occ, n_occ = sr.pixel_list(np.asarray(occluder) != 0 if np.asarray(occluder).dtype != np.float32 else occluder, S)
    B = hand.shape[0]
    pixels = np.full((B, S * S), -1, np.int32)
    count_all = np.zeros(B, np.int32)
    for b in range(B):
        h = hand[b, :n_hand[b]]
        in_hand = set(h.tolist())
        o = [p for p in occ[b, :n_occ[b]] if p not in in_hand]
        pixels[b, :len(h)] = h
        pixels[b, len(h):len(h) + len(o)] = o
        count_all[b] = len(h) + len(o)
    return pixels, n_hand.astype(np.int32), count_all


def silhouette(verts, logs_t, mask, occluder, S, dtype=torch.float64):
    """sr.silhouette with the occluder: the same dictionary (idx_v is a position in the two-section list) plus count_all"""
    v = torch.as_tensor(np.array(verts)).to(dtype)
    lt = torch.as_tensor(np.array(logs_t)).to(dtype)
    N, B, V = v.shape[:3]
    pixels, count, count_all = pixel_list(mask, occluder, S)
    out = {k: np.zeros((N, B)) for k in ("dist", "inside", "cover")}
    out.update(idx_v=np.full((N, B, V), -1, np.int32), idx_m=np.full((N, B, S * S), -1, np.int32), d_v=np.zeros((N, B, V)), d_m=np.zeros((N, B, S * S)),
               pixels=pixels, count=count, count_all=count_all)
    p = sr.project(v, lt, dtype)
    bad = ~torch.isfinite(p).all(-1).all(-1).numpy()
    for b in range(B):
        M, M2 = int(count[b]), int(count_all[b])
        if M:
            c = sr.centres(pixels[b], M2, S, dtype)
            dv, iv = sr.box_matrix(p[:, b], c, S).min(-1)          # first occurrence: the lowest list position on a tie
            dm, im = sr.centre_matrix(p[:, b], c[:M]).min(-2)
            out["inside"][:, b], out["cover"][:, b] = dv.mean(-1).numpy(), dm.mean(-1).numpy()
            out["idx_v"][:, b], out["idx_m"][:, b, :M] = iv.numpy(), im.numpy()
            out["d_v"][:, b], out["d_m"][:, b, :M] = dv.numpy(), dm.numpy()
    for k in ("inside", "cover"):
        out[k][bad] = np.nan
    out["dist"] = out["inside"] + out["cover"]
    return out


def _total(v, lt, pixels, count, count_all, S, g, idx=None):
    """sum g dist as a differentiable torch scalar; idx = (idx_v, idx_m): the minima are taken at those indices.  An image without a hand
    pixel contributes nothing"""
    dtype = v.dtype
    p = sr.project(v, lt, dtype)
    total = torch.zeros((), dtype=dtype)
    for b in range(v.shape[1]):
        M, M2 = int(count[b]), int(count_all[b])
        if not M:
            continue
        c = sr.centres(pixels[b], M2, S, dtype)
        box, cen = sr.box_matrix(p[:, b], c, S), sr.centre_matrix(p[:, b], c[:M])
        if idx is None:
            dv, dm = box.min(-1)[0], cen.min(-2)[0]
        else:
            dv = torch.gather(box, 2, torch.as_tensor(np.asarray(idx[0][:, b], np.int64))[..., None])[..., 0]
            dm = torch.gather(cen, 1, torch.as_tensor(np.asarray(idx[1][:, b, :M], np.int64))[:, None, :])[:, 0]
        total = total + (g[:, b] * (dv.mean(-1) + dm.mean(-1))).sum()
    return total


def grad(verts, logs_t, mask, occluder, S, g_dist, idx=None, dtype=torch.float64):
    """d sum(g_dist * dist) / d (verts, logs_t) by torch autograd -> (g_verts (N,B,V,3), g_logs_t (N,B,3)) numpy; a row with a non-finite
    projected vertex gets a zero gradient"""
    v = torch.as_tensor(np.array(verts)).to(dtype)
    lt = torch.as_tensor(np.array(logs_t)).to(dtype)
    g = torch.as_tensor(np.array(g_dist)).to(dtype)
    ok = torch.isfinite(sr.project(v, lt, dtype)).all(-1).all(-1)
    v = torch.where(ok[..., None, None], v, torch.zeros_like(v)).requires_grad_(True)
    lt = torch.where(ok[..., None], lt, torch.zeros_like(lt)).requires_grad_(True)
    pixels, count, count_all = pixel_list(mask, occluder, S)
    total = _total(v, lt, pixels, count, count_all, S, torch.where(ok, g, torch.zeros_like(g)), idx)
    if not total.requires_grad:
        return np.zeros(v.shape), np.zeros(lt.shape)
    gv, gl = torch.autograd.grad(total, (v, lt))
    return gv.numpy(), gl.numpy()


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------
def occluder_for(seed, mask, S):
    """(B, H, H) bool: a seeded box per image that covers part of the hand's kept pixels and part of what lies beside them (H = S k: the box
    is made of whole grid pixels).  The hand mask is NOT cut: the overlap is what the list must place once, in the hand section"""
    rng = np.random.default_rng(seed + 900)
    mask = np.asarray(mask) != 0
    B, H = mask.shape[:2]
    k = H // S
    occ = np.zeros((B, H, H), bool)
    for b in range(B):
        i, j = np.nonzero(mask[b])
        ci, cj = (int(i[rng.integers(len(i))]) // k, int(j[rng.integers(len(j))]) // k) if len(i) else (S // 2, S // 2)
        r = max(1, S // 4)
        occ[b, max(ci - r, 0) * k:(ci + r) * k, max(cj - r // 2, 0) * k:(cj + 2 * r) * k] = True
    return occ


def _big_hand(S=64):
    """(1, S, S) bool: 30 x 42 = 1,260 hand pixels - two rounds of the cover direction"""
    m = np.zeros((1, S, S), bool)
    m[0, 10:40, 8:50] = True
    return m


@functools.lru_cache(None)
def make_case(seed, N, B, V, S, big=False):
    """sr.make_case(seed, N, B, V, S) and its occluder -> dict of read-only arrays verts, logs_t, mask, occluder.  big: every image's hand is
    the 1,260-pixel block of _big_hand, the occluder a block to its right and below that overlaps it"""
    base = sr.make_case(seed=seed, N=N, B=B, V=V, S=S)
    mask = np.array(base["mask"])
    if big:
        mask = np.repeat(_big_hand(S), B, 0)
        occ = np.zeros_like(mask)
        occ[:, 30:56, 40:62] = True
    else:
        occ = occluder_for(seed, mask, S)
    case = {"verts": base["verts"], "logs_t": base["logs_t"], "mask": mask, "occluder": occ}
    for a in (mask, occ):
        a.setflags(write=False)
    return case


# N = 2, B = 3; V: one vertex, a few, the first vertex of the second register slot, all four slots; S: 4 and 8; and the two-round hand list.
# The seeds are chosen so that the f32 restatement attains the f64 indices everywhere (tests/test_silhouette_occ_host.py asserts it): the
# kernel's indices are then compared exactly, without a near-tie exemption.
CASES = {
    "v1_s4": dict(seed=401, N=2, B=3, V=1, S=4),
    "v5_s4": dict(seed=402, N=2, B=3, V=5, S=4),
    "v257_s4": dict(seed=403, N=2, B=3, V=257, S=4),
    "v778_s4": dict(seed=404, N=2, B=3, V=778, S=4),
    "v1_s8": dict(seed=405, N=2, B=3, V=1, S=8),
    "v5_s8": dict(seed=406, N=2, B=3, V=5, S=8),
    "v257_s8": dict(seed=407, N=2, B=3, V=257, S=8),
    "v778_s8": dict(seed=808, N=2, B=3, V=778, S=8),
    "v257_s64_two_rounds": dict(seed=409, N=2, B=3, V=257, S=64, big=True),
}


def g_dist_of(name, shape):
    return sr.g_dist_of(name, shape)


@functools.lru_cache(None)
def reference(name):
    """(case, f64 silhouette() of it), computed once and shared"""
    kw = CASES[name]
    case = make_case(**kw)
    return case, silhouette(case["verts"], case["logs_t"], case["mask"], case["occluder"], kw["S"])


@functools.lru_cache(None)
def reference_grad(name):
    """the f64 gradient of the case at the f64 indices, for g_dist_of(name)"""
    case, ref = reference(name)
    g = g_dist_of(name, ref["dist"].shape)
    return grad(case["verts"], case["logs_t"], case["mask"], case["occluder"], CASES[name]["S"], g, (np.maximum(ref["idx_v"], 0), np.maximum(ref["idx_m"], 0)))


@functools.lru_cache(None)
def f32_deviation(name):
    """what f32 arithmetic alone costs on this case -> (forward: the largest sr.rel_dev of dist / inside / cover, reverse: the largest of
    g_verts / g_logs_t at the f64 indices, whether the f32 restatement attains exactly the f64 indices)"""
    kw = CASES[name]
    case, ref = reference(name)
    lo = silhouette(case["verts"], case["logs_t"], case["mask"], case["occluder"], kw["S"], torch.float32)
    fwd = max(sr.rel_dev(lo[k], ref[k]) for k in ("dist", "inside", "cover"))
    g = g_dist_of(name, ref["dist"].shape)
    idx = (np.maximum(ref["idx_v"], 0), np.maximum(ref["idx_m"], 0))
    lo_g = grad(case["verts"], case["logs_t"], case["mask"], case["occluder"], kw["S"], g, idx, torch.float32)
    rev = max(sr.rel_dev(a, b) for a, b in zip(lo_g, reference_grad(name)))
    same = bool(np.array_equal(lo["idx_v"], ref["idx_v"]) and np.array_equal(lo["idx_m"], ref["idx_m"]))
    return fwd, rev, same


# Bounds.  f32_deviation() of every case, measured once on a CPU (float32 against float64), in the order of CASES - forward and reverse as
# recorded below.  The kernel is allowed four times the restatement's deviation, as in tests/silhouette_ref.py and for its reasons: forward
# four times the LARGEST case's for every case, reverse four times the case's own but never less than the forward's.
F32_FWD = {"v1_s4": 6.78e-8, "v5_s4": 1.19e-7, "v257_s4": 1.36e-7, "v778_s4": 1.60e-7, "v1_s8": 3.31e-8, "v5_s8": 1.28e-7, "v257_s8": 1.42e-7,
           "v778_s8": 2.25e-7, "v257_s64_two_rounds": 6.18e-8}
F32_REV = {"v1_s4": 5.73e-8, "v5_s4": 1.04e-7, "v257_s4": 6.24e-7, "v778_s4": 3.45e-7, "v1_s8": 9.63e-8, "v5_s8": 1.35e-7, "v257_s8": 2.90e-6,
           "v778_s8": 1.18e-6, "v257_s64_two_rounds": 7.73e-7}
F32_FWD_DEV = max(F32_FWD.values())
FWD_RTOL = 4 * F32_FWD_DEV
REV_RTOL = {k: 4 * max(v, F32_FWD_DEV) for k, v in F32_REV.items()}
