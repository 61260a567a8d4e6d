"""Float64 restatement of the 3D PCK curve (include/mhe.h, mhe_pck_curve_f32; criteria.pck_auc) in numpy, and the seeded cases the GPU tests run.
With su = scale[b] unit, d_p = |pred[n][b][p] su - target[b][p] su| and the valid points of image b,
    hits[i] = #{valid p: d_p <= thr[i]}  (inclusive, by brute-force comparison),  err = mean over the valid p of d_p,
    auc = sum_i (thr[i+1] - thr[i]) (hits[i] + hits[i+1]) / (2 n_valid (thr[T-1] - thr[0]))
The inputs are the float32 arrays the kernel reads, widened; everything after that is float64.  Besides the results, pck64 reports `gap`, the
smallest |d - thr_i| in the output's unit (mm) over all valid points and thresholds: a count can only differ between f32 and f64 where that is
of the order of the f32 rounding of a distance (1e-5 mm at 50 mm), and the cases are made with gap >= GAP = 1e-3 mm."""
import numpy as np

GAP = 1e-3          # mm, absolute


def distances64(pred, target, scale, unit):
    """-> d (N, B, P) float64"""
    N, B, P = pred.shape[:3]
    su = np.asarray(scale, np.float64) * float(unit)
    p = np.asarray(pred, np.float64).reshape(N, B, P, 3) * su[None, :, None, None]
    g = np.asarray(target, np.float64).reshape(B, P, 3) * su[:, None, None]
    return np.sqrt(((p - g[None]) ** 2).sum(-1))


def auc64(hits, n_valid, thr):
    """hits (..., T) integers, n_valid broadcastable to hits[..., 0], thr (T,) -> the normalised trapezoid area, float64 (NaN where n_valid = 0)"""
    t = np.asarray(thr, np.float64)
    area = (np.diff(t) * (hits[..., :-1] + hits[..., 1:]).astype(np.float64)).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return area / (2.0 * np.asarray(n_valid, np.float64) * (t[-1] - t[0]))


def pck64(pred, target, scale, thr, valid=None, unit=1000.0):
    """pred (N, B, P, 3), target (B, P, 3), scale (B,), thr (T,), valid (B, P) 0/1 or None -> dict: hits (N, B, T) int64, auc (N, B), err (N, B)
    (NaN for an image without a valid point), n_valid (B,), d (N, B, P), gap"""
    N, B, P = pred.shape[:3]
    thr = np.asarray(thr, np.float64).reshape(-1)
    v = np.ones((B, P), bool) if valid is None else np.asarray(valid).astype(bool)
    d = distances64(pred, target, scale, unit)
    with np.errstate(invalid="ignore"):
        hits = ((d[..., None] <= thr) & v[None, :, :, None]).sum(2)
    nv = v.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(v[None], d, 0.0).sum(2) / nv[None]
        err = np.where(np.isfinite(np.where(v[None], d, 0.0)).all(2), err, np.nan)
    dv = d[np.broadcast_to(v[None], d.shape)]
    dv = dv[np.isfinite(dv)]
    gap = float(np.abs(dv[:, None] - thr[None]).min()) if dv.size else float("inf")
    return {"hits": hits, "auc": auc64(hits, nv[None], thr), "err": err, "n_valid": nv, "d": d, "gap": gap}


def make_case(seed, N, B, P, T, valid_share=1.0, unit=1000.0, vmax=50.0):
    """A seeded case whose distances all keep at least 2 GAP (mm) from every threshold: T thresholds np.linspace(0, vmax, T) rounded to f32, target
    points ~ N(0, 1) in normalised units, scale 0.025 .. 0.04, the hypotheses = the target displaced by N(0, 0.15) per coordinate (about 8 mm, so
    the distances lie well inside 0 .. 50 mm).  A point whose distance comes within 2 GAP of a threshold is drawn again from the same generator
    until none is left - a condition on the inputs, met by construction for every seed.  valid_share < 1: a random 0/1 mask of that share."""
    rng = np.random.default_rng(seed)
    thr = np.linspace(0.0, vmax, T).astype(np.float32)
    target = rng.normal(0.0, 1.0, (B, P, 3)).astype(np.float32)
    scale = rng.uniform(0.025, 0.04, (B,)).astype(np.float32)
    pred = (target[None] + rng.normal(0.0, 0.15, (N, B, P, 3))).astype(np.float32)
    valid = None if valid_share >= 1.0 else (rng.uniform(size=(B, P)) < valid_share).astype(np.uint8)
    t64 = thr.astype(np.float64)
    for _ in range(200):
        d = distances64(pred, target, scale, unit)
        bad = (np.abs(d[..., None] - t64) < 2 * GAP).any(-1)
        n, b, p = np.nonzero(bad)
        if not len(n):
            break
        pred[n, b, p] = (target[b, p] + rng.normal(0.0, 0.15, (len(n), 3))).astype(np.float32)
    else:
        raise AssertionError("make_case did not converge")
    for a in (pred, target, scale, thr) + (() if valid is None else (valid,)):
        a.setflags(write=False)
    return {"pred": pred, "target": target, "scale": scale, "thr": thr, "valid": valid, "unit": unit}


# ---- the (seed, N, B, P, T, valid_share) of every seeded case of tests/test_gpu_pck.py; tests/test_pck_host.py makes each of them on the CPU ----
PS = (1, 2, 21, 63, 64, 65, 255, 256, 257, 778)
SMALL = ((1, 1), (3, 2), (5, 3))
TS = (2, 3, 100, 255, 256)
WALK = (684, 3)


def edge_cases():
    for j, P in enumerate(PS):
        for i, (N, B) in enumerate(SMALL):
            yield (1000 + 10 * P + i, N, B, P, TS[(j + i) % len(TS)], 1.0)


def other_cases():
    yield (2000, 4, 3, 65, 100, 0.6)          # the random mask
    yield (2001, 3, 3, 300, 100, 1.0)         # masks planted by the test; determinism
    yield (2002, 6, 3, 21, 100, 1.0)          # the public interface (joints)
    yield (2003, 6, 3, 65, 100, 1.0)          # the public interface (mesh)
    for k, B in enumerate((2, 5, 3)):
        yield (2010 + k, 2, B, 21, 100, 0.7)          # the pool's three batches


def walk_cases():
    for P in (21, 65):
        yield (3000 + P, WALK[0], WALK[1], P, 100, 1.0)
