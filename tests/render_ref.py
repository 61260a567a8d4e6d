"""A numpy float64 rasteriser of the contract of mhe_render_mesh_f32 (include/mhe.h), written from that contract, and the meshes the render
tests share.  Loop over faces, vectorised over the samples of a face's bounding box.

Besides mask / depth / iou_sums it returns, per sample, the distance in sample spacings to the nearest projected edge SEGMENT of any face
(computed inside every face's bounding box grown by one sample, which is all that matters below 1).  A sample is AMBIGUOUS when that distance
is below EDGE = 1e-3, a pixel when any of its A^2 samples is.  Derivation of EDGE: the kernel rounds a projected coordinate of up to
2 G <= 1,024 sample units to f32, 6e-5 units, and an edge test is a handful of such operations; 1e-3 leaves an order of magnitude.  A
mismatch outside that band is a kernel bug, not rounding.  The contract lets a sample exactly on an edge go either way, so the parity tests
skip the ambiguous pixels - and every case asserts (in f64, on this reference alone) that at most CAP = 1 % of its samples are ambiguous."""
import functools

import numpy as np

EDGE = 1e-3
CAP = 0.01


def _segment_distance(gx, gy, px, py, qx, qy):
    ex, ey = qx - px, qy - py
    L2 = ex * ex + ey * ey
    t = np.clip(((gx - px) * ex + (gy - py) * ey) / L2, 0.0, 1.0) if L2 > 0 else 0.0
    return np.hypot(gx - (px + t * ex), gy - (py + t * ey))


def render64(verts, faces, scale, trans, zscale=None, size=64, anti_aliasing=True, far=100.0, target=None):
    """verts [R,V,3], faces [F,3], scale [R], trans [R,2], zscale [R] or None, target [B,size,size] or None -> dict:
    mask, depth [R,S,S]; edge [R,G,G] (distance to the nearest edge segment, inf where no box reaches); ambiguous [R,S,S] bool;
    n_ambiguous [R] (samples); iou_sums [R,2] when target is given"""
    verts, scale, trans = np.asarray(verts, np.float64), np.asarray(scale, np.float64).reshape(-1), np.asarray(trans, np.float64)
    faces = np.asarray(faces, np.int64)
    R, V = verts.shape[:2]
    S, A = int(size), 2 if anti_aliasing else 1
    G = S * A
    cover, zmin, edge = np.zeros((R, G, G), bool), np.full((R, G, G), np.inf), np.full((R, G, G), np.inf)
    faces = faces[((faces >= 0) & (faces < V)).all(1)]          # an index outside [0, V): the face is skipped
    for r in range(R):
        # sample (row i, col j) sits at x = (2j+1)/G - 1: X = (x + 1) G / 2 - 1/2 puts sample j at X = j
        X = (abs(scale[r]) * verts[r, :, 0] + trans[r, 0] + 1.0) * G / 2 - 0.5
        Y = (abs(scale[r]) * verts[r, :, 1] + trans[r, 1] + 1.0) * G / 2 - 0.5
        D = verts[r, :, 2] * (float(zscale[r]) / 1000.0) if zscale is not None else verts[r, :, 2]
        fx, fy = X[faces], Y[faces]
        x0 = np.maximum(np.ceil(fx.min(1)) - 1, 0).astype(np.int64); x1 = np.minimum(np.floor(fx.max(1)) + 1, G - 1).astype(np.int64)
        y0 = np.maximum(np.ceil(fy.min(1)) - 1, 0).astype(np.int64); y1 = np.minimum(np.floor(fy.max(1)) + 1, G - 1).astype(np.int64)
        for f in np.nonzero((x0 <= x1) & (y0 <= y1))[0]:
            (ax, bx, cx), (ay, by, cy), (da, db, dc) = fx[f], fy[f], D[faces[f]]
            gy, gx = np.meshgrid(np.arange(y0[f], y1[f] + 1, dtype=np.float64), np.arange(x0[f], x1[f] + 1, dtype=np.float64), indexing="ij")
            box = (r, slice(y0[f], y1[f] + 1), slice(x0[f], x1[f] + 1))
            dist = np.minimum(np.minimum(_segment_distance(gx, gy, ax, ay, bx, by), _segment_distance(gx, gy, bx, by, cx, cy)),
                              _segment_distance(gx, gy, cx, cy, ax, ay))
            edge[box] = np.minimum(edge[box], dist)
            area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            if area == 0.0:
                continue
            wc = ((bx - ax) * (gy - ay) - (by - ay) * (gx - ax)) / area          # barycentric weights: the edge opposite a vertex
            wa = ((cx - bx) * (gy - by) - (cy - by) * (gx - bx)) / area
            wb = ((ax - cx) * (gy - cy) - (ay - cy) * (gx - cx)) / area
            inside = (wa >= 0) & (wb >= 0) & (wc >= 0)
            d = np.clip(wa * da + wb * db + wc * dc, min(da, db, dc), max(da, db, dc))
            cover[box] |= inside
            zmin[box] = np.where(inside, np.minimum(zmin[box], d), zmin[box])
    pool = lambda a: a.reshape(R, S, A, S, A)
    dmin = pool(zmin).min((2, 4))
    amb = edge < EDGE
    out = {"mask": pool(cover).mean((2, 4)), "depth": np.where(np.isfinite(dmin), dmin, float(far)), "edge": edge, "ambiguous": pool(amb).any((2, 4)),
           "n_ambiguous": amb.sum((1, 2)), "ambiguous_fraction": float(amb.mean()), "G": G, "A": A}
    if target is not None:
        t = np.asarray(target, np.float64)
        t = t[np.arange(R) % t.shape[0]]
        out["iou_sums"] = np.stack([np.minimum(out["mask"], t).sum((1, 2)), np.maximum(out["mask"], t).sum((1, 2))], 1)
    return out


def skipped_edge_distance(ref):
    """the smallest edge distance among the ambiguous samples (what a parity test had to skip), inf when there are none"""
    e = ref["edge"][ref["edge"] < EDGE]
    return float(e.min()) if e.size else float("inf")


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def grid_faces(rows, cols):
    i, j = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    v = (i * cols + j).reshape(-1)
    return np.concatenate([np.stack([v, v + 1, v + cols], 1), np.stack([v + 1, v + cols + 1, v + cols], 1)]).astype(np.int32)


def sheet(seed, rows=28, cols=28, extent=0.8, fold=False):
    """a jittered rows x cols vertex grid bent into a curved sheet, z a smooth function of x, y.  fold: the sheet is folded along its
    middle column so that its two halves lie over each other and CROSS (z rises with x on one, falls on the other): the nearest surface
    changes inside the image"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.linspace(-1, 1, rows), np.linspace(-1, 1, cols), indexing="ij")
    u = u + rng.uniform(-0.3, 0.3, u.shape) * (2.0 / (cols - 1))
    v = v + rng.uniform(-0.3, 0.3, v.shape) * (2.0 / (rows - 1))
    if fold:
        x, y = extent * (2 * np.abs(u) - 1), extent * v
        z = np.where(u < 0, 0.5 * x + 0.1 * np.sin(3 * y), -0.5 * x + 0.1 * np.cos(2 * y))
    else:
        x, y = extent * u, extent * v
        z = 0.3 * np.sin(2.0 * x) * np.cos(1.5 * y) + 0.2 * x * y
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32), grid_faces(rows, cols)


def random_subset(seed, n=256):
    """n of the synthetic MANO tables' faces (random vertex triples, long edges: deep overlap) over their template's vertices spread to +-0.9"""
    from mhentropy_amd import synth
    t = synth.mano_tables(0)
    rng = np.random.default_rng(seed)
    v = np.asarray(t["v_template"], np.float64).reshape(-1, 3)
    v = v - v.mean(0)
    v = v / np.abs(v[:, :2]).max() * 0.9
    faces = np.asarray(t["faces"])[rng.choice(len(t["faces"]), n, replace=False)]
    return v.astype(np.float32), faces.astype(np.int32)


def smpl_size(seed):
    """V = 6,890 and F = 13,776, SMPL's counts: an 83 x 83 sheet (6,889 vertices, 13,448 faces) plus one vertex and 328 faces that span two
    grid cells each (a closed surface has F = 2V - 4, an open grid fewer: the rest is made up with a second layer)"""
    v, f = sheet(seed, 83, 83)
    rng = np.random.default_rng(seed + 1)
    v = np.concatenate([v, [[0.0, 0.0, -0.5]]]).astype(np.float32)
    i, j = rng.integers(0, 81, 328), rng.integers(0, 81, 328)
    b = i * 83 + j
    extra = np.stack([b, b + 2, b + 2 * 83], 1)
    extra[0, 0] = 6889                                    # the added vertex is used
    return v, np.concatenate([f, extra]).astype(np.int32)


def cameras(seed, R, spread=0.1):
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.85, 1.1, R) * rng.choice([-1.0, 1.0], R)          # the sign is ignored by the contract
    return scale.astype(np.float32), rng.uniform(-spread, spread, (R, 2)).astype(np.float32), rng.uniform(50.0, 150.0, R).astype(np.float32)


# name -> (mesh builder, rows R, size S, anti_aliasing): the parity cases of tests/test_gpu_render.py
CASES = {
    "sheet_16aa": (lambda: sheet(1), 3, 16, True),                   # the smallest image here, many faces per sample
    "crossing_64aa": (lambda: sheet(2, fold=True), 3, 64, True),     # the product size on the one-workgroup path; V = 784, F = 1,458
    "subset_64": (lambda: random_subset(3), 3, 64, False),           # A = 1, long overlapping faces (the workgroup's list of big faces)
    "sheet_256aa": (lambda: sheet(4), 2, 256, True),                 # 16 bands of 32 sample rows; a face is ~19 samples high: faces straddle the bands
    "one_face": (lambda: (np.array([[-0.5, -0.6, 0.1], [0.7, -0.2, 0.4], [0.1, 0.6, -0.3]], np.float32), np.array([[0, 1, 2]], np.int32)), 2, 24, True),
    "smpl_64aa": (lambda: smpl_size(5), 2, 64, True),                # more vertices than the LDS stage holds
}


@functools.lru_cache(None)
def case(name):
    """the case's operands (float32 / int32, as the kernel gets them) and its f64 reference, computed once and shared: read-only"""
    build, R, S, aa = CASES[name]
    verts1, faces = build()
    scale, trans, zscale = cameras(len(name), R)
    rng = np.random.default_rng(len(name) + 100)
    verts = (verts1[None] + rng.normal(0, 0.004, (R,) + verts1.shape)).astype(np.float32)          # every row its own mesh
    target = (rng.uniform(0, 1, (1 if R % 2 else 2, S, S)) * (rng.uniform(0, 1, (1 if R % 2 else 2, S, S)) < 0.6)).astype(np.float32)
    ref = render64(verts, faces, scale, trans, zscale, S, aa, 100.0, target)
    ops = {"verts": verts, "faces": faces, "scale": scale, "trans": trans, "zscale": zscale, "target": target, "size": S, "anti_aliasing": aa}
    for a in list(ops.values()) + [v for v in ref.values() if isinstance(v, np.ndarray)]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ops, ref
