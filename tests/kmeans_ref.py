"""float64 restatement of the k-means quantisation (include/mhe.h, mhe_kmeans_select_f32; DESIGN.md "k-means quantisation"), one image at a
time, decision for decision:

    distance        sum over d of (p_d - c_d)^2
    seeds           0: highest score, ties to the lower n (no score: n = 0); k: the point farthest from its nearest earlier seed, ties to the
                    lower n; the initial centres are the seed points
    Lloyd           at most `iters` rounds: assign every point to its nearest centre (ties to the lower k); stop with converged = 1 when no
                    assignment changed (the first round always counts as changed); else every centre becomes the mean of its members, a
                    cluster without members keeps its centre.  Without a fixed point (iters = 0 included) one more assignment follows the
                    last means and converged stays 0
    representative  the member nearest its centre, ties to the lower n; an empty cluster: count 0 and the nearest of all N
    order           count descending, ties to the lower representative, then to the lower seed number; `assign` is in the output order

Besides the five outputs it returns the smallest decision margin it met, (second best - best) / max(|best|, |second best|, tiny) over every
argmin / argmax it took (inf where there was no second candidate): a test that demands equality with an f32 implementation first asserts
that this is far above f32 rounding, a test of the tie rules that it is 0.  update_counts lists the sizes of all clusters that were
averaged (all powers of two: every mean of small integers is exact in f32 too), emptied tells whether a cluster that had members lost
them all in a later round."""
import numpy as np

TINY = 1e-300


def _pick(vals, largest, state):
    """index of the best of vals (first on a tie, as np.argmax / np.argmin), recording the margin to the second best"""
    vals = np.asarray(vals, np.float64)
    i = int(np.argmax(vals) if largest else np.argmin(vals))
    if vals.size > 1:
        rest = np.delete(vals, i)
        second = rest.max() if largest else rest.min()
        state["margin"] = min(state["margin"], abs(second - vals[i]) / max(abs(vals[i]), abs(second), TINY))
    return i


def _sqdist(p, c):
    """p [N, D], c [Q, D] -> [N, Q]"""
    return ((p[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def kmeans_image(points, Q, score=None, iters=10):
    """points [N, D], score [N] or None -> dict(index [Q], count [Q], assign [N], centre [Q, D], converged, margin, update_counts, emptied)"""
    p = np.asarray(points, np.float64)
    N, D = p.shape
    assert 1 <= Q <= N and iters >= 0
    st = {"margin": np.inf}
    seeds = [0 if score is None else _pick(np.asarray(score, np.float64), True, st)]
    mind = _sqdist(p, p[seeds[0]][None])[:, 0]
    for _ in range(1, Q):
        seeds.append(_pick(mind, True, st))
        mind = np.minimum(mind, _sqdist(p, p[seeds[-1]][None])[:, 0])
    c = p[seeds].copy()
    assign = np.full(N, -1)
    converged, update_counts, emptied, had = 0, [], False, np.zeros(Q, bool)

    def assign_all():
        d = _sqdist(p, c)
        a = np.array([_pick(d[n], False, st) for n in range(N)])
        return a, d[np.arange(N), a]

    done = False
    for it in range(iters):
        new, dist = assign_all()
        changed = it == 0 or not np.array_equal(new, assign)
        assign = new
        if not changed:
            converged, done = 1, True
            break
        for k in range(Q):
            m = assign == k
            if m.any():
                c[k] = p[m].sum(0) / m.sum()
                update_counts.append(int(m.sum()))
                had[k] = True
            elif had[k]:
                emptied = True
    if not done:
        assign, dist = assign_all()
    count = np.array([(assign == k).sum() for k in range(Q)])
    emptied = emptied or bool((had & (count == 0)).any())
    rep = np.zeros(Q, np.int64)
    for k in range(Q):
        if count[k]:
            members = np.nonzero(assign == k)[0]
            rep[k] = members[_pick(dist[members], False, st)]
        else:
            rep[k] = _pick(_sqdist(p, c[k][None])[:, 0], False, st)
    order = sorted(range(Q), key=lambda k: (-count[k], rep[k], k))
    slot = np.empty(Q, np.int64)
    slot[order] = np.arange(Q)
    return {"index": rep[order], "count": count[order], "assign": slot[assign], "centre": c[order], "converged": converged,
            "margin": float(st["margin"]), "update_counts": update_counts, "emptied": emptied}


def kmeans(points, Q, score=None, iters=10):
    """points [N, B, D] sample-major, score [N, B] or None -> index [Q, B], count [Q, B], assign [N, B], centre [Q, B, D], converged [B], and
    margin, the smallest over the images; update_counts and emptied are gathered over the images too"""
    points = np.asarray(points)
    N, B, D = points.shape
    per = [kmeans_image(points[:, b], Q, None if score is None else np.asarray(score)[:, b], iters) for b in range(B)]
    out = {k: np.stack([r[k] for r in per], 1) for k in ("index", "count", "assign", "centre")}
    out["converged"] = np.array([r["converged"] for r in per])
    out["margin"] = min(r["margin"] for r in per)
    out["update_counts"] = [c for r in per for c in r["update_counts"]]
    out["emptied"] = any(r["emptied"] for r in per)
    return out


def planted(seed, N, B, D, Q, spread=3.0, with_score=True):
    """Q Gaussian clusters of unit sigma per image around centres drawn with standard deviation `spread` per coordinate, members dealt
    round-robin in a shuffled order -> (points [N, B, D] f32, score [N, B] f32 or None, centres [Q, B, D])"""
    rng = np.random.RandomState(seed)
    centres = rng.randn(Q, B, D) * spread
    which = np.stack([rng.permutation(N) % Q for _ in range(B)], 1)                  # [N, B]
    pts = centres[which, np.arange(B)[None, :]] + rng.randn(N, B, D)
    score = rng.randn(N, B).astype(np.float32) if with_score else None
    return pts.astype(np.float32), score, centres
