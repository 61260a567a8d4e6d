"""Float64 restatement of the hand mesh evaluation (include/mhe.h, mhe_mesh_eval_f32; criteria.mesh_eval) in numpy, and the seeded cases the
GPU tests run.  With p_v = pred[n][b][v] scale[b] unit and g_w = target[b][w] scale[b] unit,
    err = mean_v |p_v - g_v|,  d1_v = min_w |p_v - g_w|,  d2_w = min_v |p_v - g_w|,
    precision_t = #{v: d1_v < thr_t} / V,  recall_t = #{w: d2_w < thr_t} / V,  f_t = 2 P R / (P + R)  (0 when P + R = 0)
with the strict < of the FreiHAND / HO3D evaluation code.  The inputs are the float32 arrays the kernel reads, widened; everything after that is
float64.  Besides the results, mesh_eval64 reports `gap`, the smallest relative distance min |d - thr_t| / thr_t of any nearest distance to any
threshold: a count can only differ between f32 and f64 where that is of the order of f32 rounding (1e-6), and the cases are made with gap >= GAP."""
import numpy as np

GAP = 1e-3
ROWS = 16          # rows of one (rows, V, V) block of distances


def nearest64(P, G):
    """P, G (R, V, 3) float64 -> d1 (R, V) = min_w |P_v - G_w|, d2 (R, V) = min_v |P_v - G_w|, a2 (R, V) = the lowest v attaining d2_w"""
    R, V = P.shape[:2]
    d1, d2, a2 = np.empty((R, V)), np.empty((R, V)), np.empty((R, V), np.int64)
    for r0 in range(0, R, ROWS):
        p, g = P[r0:r0 + ROWS], G[r0:r0 + ROWS]
        q = np.zeros((p.shape[0], V, V))
        for c in range(3):
            d = p[:, :, None, c] - g[:, None, :, c]          # [row, v, w]
            d *= d
            q += d
        d1[r0:r0 + ROWS] = np.sqrt(q.min(2))
        a2[r0:r0 + ROWS] = q.argmin(1)
        d2[r0:r0 + ROWS] = np.sqrt(q.min(1))
    return d1, d2, a2


def _scaled(pred, target, scale, unit):
    N, B, V = pred.shape[:3]
    su = np.asarray(scale, np.float64) * float(unit)
    P = np.asarray(pred, np.float64).reshape(N, B, V, 3) * su[None, :, None, None]
    G = np.broadcast_to((np.asarray(target, np.float64).reshape(B, V, 3) * su[:, None, None])[None], (N, B, V, 3))
    return P.reshape(N * B, V, 3), G.reshape(N * B, V, 3)


def mesh_eval64(pred, target, scale, thr, unit=1000.0):
    """pred (N, B, V, 3), target (B, V, 3), scale (B,), thr (T,) -> dict: err (N, B); count_p, count_r (T, N, B) int64, the vertices counted;
    precision, recall, f (T, N, B); d1, d2 (N, B, V); gap, the smallest |d - thr_t| / thr_t over all of them"""
    N, B, V = pred.shape[:3]
    thr = np.asarray(thr, np.float64).reshape(-1)
    P, G = _scaled(pred, target, scale, unit)
    d1, d2, _ = nearest64(P, G)
    err = np.sqrt(((P - G) ** 2).sum(-1)).mean(-1).reshape(N, B)
    cp = (d1[None] < thr[:, None, None]).sum(-1).reshape(-1, N, B)
    cr = (d2[None] < thr[:, None, None]).sum(-1).reshape(-1, N, B)
    prec, rec = cp / V, cr / V
    f = np.where(cp + cr > 0, 2.0 * prec * rec / np.where(cp + cr > 0, prec + rec, 1.0), 0.0)
    both = np.stack([d1, d2])
    gap = min(float((np.abs(both - t) / t).min()) for t in thr)
    return {"err": err, "count_p": cp, "count_r": cr, "precision": prec, "recall": rec, "f": f, "d1": d1.reshape(N, B, V), "d2": d2.reshape(N, B, V),
            "gap": gap}


THRESHOLDS = (5.0, 15.0, 2.5, 10.0)          # mm; a case with T thresholds takes the first T


def make_case(seed, N, B, V, T, unit=1000.0):
    """A seeded case whose nearest distances all keep a relative distance of at least 2 GAP from every threshold: target vertices ~ N(0, 1) in
    normalised units, scale 0.025 .. 0.04 m (a hand of about +-35 mm), the hypotheses = the target displaced by N(0, 0.15) per coordinate (about
    8 mm).  A predicted vertex whose own nearest distance, or the nearest distance of a target vertex it serves, comes within 2 GAP of a threshold
    is drawn again from the same generator, row by row, until none is left - a condition on the inputs, met by construction for every seed."""
    rng = np.random.default_rng(seed)
    thr = np.asarray(THRESHOLDS[:T], np.float64)
    target = rng.normal(0.0, 1.0, (B, V, 3)).astype(np.float32)
    scale = rng.uniform(0.025, 0.04, (B,)).astype(np.float32)
    pred = (target[None] + rng.normal(0.0, 0.15, (N, B, V, 3))).astype(np.float32)
    rows = np.arange(N * B)
    flat = pred.reshape(N * B, V, 3)
    for _ in range(200):
        if not len(rows):
            break
        P, G = _scaled(pred, target, scale, unit)
        d1, d2, a2 = nearest64(P[rows], G[rows])
        near = lambda d: (np.abs(d[None] - thr[:, None, None]) < 2 * GAP * thr[:, None, None]).any(0)
        bad1, bad2 = near(d1), near(d2)
        keep = []
        for i, r in enumerate(rows):
            vs = np.union1d(np.nonzero(bad1[i])[0], a2[i][bad2[i]])
            if len(vs):
                flat[r, vs] = (target[r % B, vs] + rng.normal(0.0, 0.15, (len(vs), 3))).astype(np.float32)
                keep.append(r)
        rows = np.asarray(keep, np.int64)
    else:
        raise AssertionError("make_case did not converge")
    for a in (pred, target, scale):
        a.setflags(write=False)
    return {"pred": pred, "target": target, "scale": scale, "thr": thr.astype(np.float32), "unit": unit}
