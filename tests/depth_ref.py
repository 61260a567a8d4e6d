"""A numpy float64 restatement of mhe_depth_dist_f32 / mhe_depth_dist_bwd_f32 (include/mhe.h), written from that contract, with the cases
the depth tests share.  A helper module, not a test.  It uses render_ref's edge-segment distance and its EDGE / CAP.

AMBIGUOUS samples.  The kernel rounds projected coordinates once to f32 (DELTA = 6e-5 sample units up to 1,024 units out) and a depth to f32
twice (the vertex depth, then the clamped plane value that becomes the key: U = 2^-24 relative each).  A sample is ambiguous when
  * render_ref's edge distance is below EDGE = 1e-3 sample spacings (coverage may go either way), or
  * the two nearest covering faces differ in depth by less than TIE = b1 + b2, b_f = 2 DELTA (|gx_f| + |gy_f|) + 4 U max|D_f|: moving a face's
    three projected vertices by <= DELTA moves its plane at a sample by <= DELTA (|gx| + |gy|) to first order (the plane through the moved
    vertices differs from the old one by an affine function whose vertex values are -g . delta_k, and the sample's barycentric weights are
    >= 0 and sum to 1), doubled for the second order; each of the <= 4 f32 roundings on the way to the key costs U max|D|.  Within TIE the
    order of the two f32 keys, and with it the winning face, is not decided by the f64 values.
The same b_f bounds the kernel's R(p) against this reference outside the ambiguous samples; it is returned per sample (b_resid adds the
offset's share and the f32 rounding of e).  FRAGILE samples are those of P whose |e| lies within b_resid of 0 or of trunc: there s(p) or
the inlier count may differ; the exact cases assert that there are none.

Gradient bounds (returned next to the gradient, accumulated term by term): with lam'_k the weights of the moved triangle,
(lam'_k - lam_k)(X_j) = -grad lam'_k . delta_j, so |d lam_k| <= DELTA |grad lam_k|_1; the slopes are g = sum_k D_k grad lam_k and the moved
plane differs by the affine function above, so |d gx| <= DELTA (|gx| + |gy|) sum_k |d lam_k / dx| (gy alike) - each doubled for the second
order.  A term g(p) lam_k zs of dz_k is then off by |g| zs (2 DELTA |grad lam_k|_1 + 6 U lam_k) (the weight, the table entry and the slopes are
stored in f32, the sums are f64), a term g(p) gx lam_k of dX_k by |g| (|gx| 2 DELTA |grad lam_k|_1 + lam_k 2 DELTA (|gx|+|gy|) sum_j |dx lam_j|
+ 6 U |gx| lam_k); the chain factors s S/2 and the sums over vertices carry the bounds along, and every f32 output adds U of its value."""
import functools

import numpy as np

from render_ref import CAP, EDGE, _segment_distance  # noqa: F401

DELTA = 6e-5
U = 2.0 ** -24


def _project(verts, logs_t, zs, S):
    s = np.exp(logs_t[0])
    X = (s * verts[:, 0] + logs_t[1] + 1.0) * S / 2 - 0.5
    Y = (s * verts[:, 1] + logs_t[2] + 1.0) * S / 2 - 0.5
    return s, X, Y, verts[:, 2] * zs


def _rasterise(X, Y, D, faces, S):
    """-> face image (nearest covering face, lowest index among equal depths; -1), ambiguous [S,S], edge distance [S,S]"""
    V = X.shape[0]
    z1, z2 = np.full((S, S), np.inf), np.full((S, S), np.inf)
    b1, b2 = np.zeros((S, S)), np.zeros((S, S))
    fimg, edge = np.full((S, S), -1, np.int64), np.full((S, S), np.inf)
    for f, (i0, i1, i2) in enumerate(faces):
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= V:
            continue
        (ax, bx, cx), (ay, by, cy), (da, db, dc) = X[[i0, i1, i2]], Y[[i0, i1, i2]], D[[i0, i1, i2]]
        x0, x1 = int(max(np.ceil(min(ax, bx, cx)) - 1, 0)), int(min(np.floor(max(ax, bx, cx)) + 1, S - 1))
        y0, y1 = int(max(np.ceil(min(ay, by, cy)) - 1, 0)), int(min(np.floor(max(ay, by, cy)) + 1, S - 1))
        if x0 > x1 or y0 > y1:
            continue
        gy_, gx_ = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.float64), np.arange(x0, x1 + 1, dtype=np.float64), indexing="ij")
        box = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        dist = np.minimum(np.minimum(_segment_distance(gx_, gy_, ax, ay, bx, by), _segment_distance(gx_, gy_, bx, by, cx, cy)),
                          _segment_distance(gx_, gy_, cx, cy, ax, ay))
        edge[box] = np.minimum(edge[box], dist)
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area == 0.0:
            continue
        wc = ((bx - ax) * (gy_ - ay) - (by - ay) * (gx_ - ax)) / area
        wa = ((cx - bx) * (gy_ - by) - (cy - by) * (gx_ - bx)) / area
        wb = ((ax - cx) * (gy_ - cy) - (ay - cy) * (gx_ - cx)) / area
        inside = (wa >= 0) & (wb >= 0) & (wc >= 0)
        d = np.clip(wa * da + wb * db + wc * dc, min(da, db, dc), max(da, db, dc))
        sx = ((db - da) * (cy - ay) - (dc - da) * (by - ay)) / area
        sy = ((dc - da) * (bx - ax) - (db - da) * (cx - ax)) / area
        bf = 2 * DELTA * (abs(sx) + abs(sy)) + 4 * U * max(abs(da), abs(db), abs(dc))
        Z1, Z2, B1, B2, FI = z1[box], z2[box], b1[box], b2[box], fimg[box]
        first = inside & (d < Z1)
        second = inside & ~first & (d < Z2)
        Z2[first], B2[first] = Z1[first], B1[first]
        Z1[first], B1[first], FI[first] = d[first], bf, f
        Z2[second], B2[second] = d[second], bf
    with np.errstate(invalid="ignore"):
        tie = np.isfinite(z2) & (z2 - z1 < b1 + b2)
    return fimg, (edge < EDGE) | tie, edge


def _planes(X, Y, D, faces, fimg):
    """per covered sample of a face image: R, the weights of its face's corners, the slopes and the norms the bounds need"""
    S = fimg.shape[0]
    py, px = np.nonzero(fimg >= 0)
    idx = np.asarray(faces, np.int64)[fimg[py, px]]
    ax, bx, cx = X[idx[:, 0]], X[idx[:, 1]], X[idx[:, 2]]
    ay, by, cy = Y[idx[:, 0]], Y[idx[:, 1]], Y[idx[:, 2]]
    da, db, dc = D[idx[:, 0]], D[idx[:, 1]], D[idx[:, 2]]
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    lam = np.stack([((cx - bx) * (py - by) - (cy - by) * (px - bx)) / area, ((ax - cx) * (py - cy) - (ay - cy) * (px - cx)) / area,
                    ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) / area], 1)
    dlx = np.stack([-(cy - by), -(ay - cy), -(by - ay)], 1) / area[:, None]
    dly = np.stack([(cx - bx), (ax - cx), (bx - ax)], 1) / area[:, None]
    dd = np.stack([da, db, dc], 1)
    R = np.clip((lam * dd).sum(1), dd.min(1), dd.max(1))
    gx, gy = (dd * dlx).sum(1), (dd * dly).sum(1)
    bR = 2 * DELTA * (np.abs(gx) + np.abs(gy)) + 4 * U * np.abs(dd).max(1)
    return {"py": py, "px": px, "idx": idx, "lam": lam, "dlx": dlx, "dly": dly, "R": R, "gx": gx, "gy": gy, "bR": bR, "S": S}


def depth_dist64(verts, faces, logs_t, zscale, obs, root_z=None, trunc=0.05, g_dist=None, face_override=None):
    """verts [N,B,V,3], faces [F,3], logs_t [N,B,3], zscale [B], obs [B,S,S], root_z [B] | None, g_dist [N,B] | None (ones) -> dict:
    dist [N,B], parts [N,B,3], face_img [N,B,S,S], resid_img [N,B,S,S] (NaN outside P), g_verts [N,B,V,3], g_logs_t [N,B,3], ambiguous
    [N,B,S,S] bool, fragile [N,B] (count), n_obs [N,B], edge_min [N,B] (the least edge distance of any sample), and the bounds b_resid, b_dist, b_offset, b_g_verts, b_g_logs_t derived above.
    face_override [N,B,S,S]: a face image that replaces this one's AT THE AMBIGUOUS SAMPLES ONLY (the MANO-sized gradient comparison)."""
    verts, logs_t = np.asarray(verts, np.float64), np.asarray(logs_t, np.float64)
    faces, zscale, obs = np.asarray(faces, np.int64), np.asarray(zscale, np.float64), np.asarray(obs, np.float64)
    N, B, V = verts.shape[:3]
    S = obs.shape[1]
    g_dist = np.ones((N, B)) if g_dist is None else np.asarray(g_dist, np.float64)
    o = {"dist": np.zeros((N, B)), "parts": np.zeros((N, B, 3)), "face_img": np.full((N, B, S, S), -1, np.int64),
         "resid_img": np.full((N, B, S, S), np.nan), "g_verts": np.zeros((N, B, V, 3)), "g_logs_t": np.zeros((N, B, 3)),
         "ambiguous": np.zeros((N, B, S, S), bool), "fragile": np.zeros((N, B), np.int64), "n_obs": np.zeros((N, B), np.int64), "edge_min": np.full((N, B), np.inf),
         "b_resid": np.zeros((N, B, S, S)), "b_dist": np.zeros((N, B)), "b_offset": np.zeros((N, B)), "b_g_verts": np.zeros((N, B, V, 3)),
         "b_g_logs_t": np.zeros((N, B, 3))}
    for n in range(N):
        for b in range(B):
            zs = zscale[b]
            s, X, Y, D = _project(verts[n, b], logs_t[n, b], zs, S)
            bad = not (np.isfinite(X).all() and np.isfinite(Y).all() and np.isfinite(D).all() and np.isfinite(zs)) or \
                (root_z is not None and not np.isfinite(root_z[b]))
            if bad:
                o["dist"][n, b], o["parts"][n, b] = np.nan, np.nan
                continue
            fimg, amb, edge = _rasterise(X, Y, D, faces, S)
            o["edge_min"][n, b] = edge.min()
            if face_override is not None:
                fimg = np.where(amb, np.asarray(face_override[n, b], np.int64), fimg)
            o["face_img"][n, b], o["ambiguous"][n, b] = fimg, amb
            ob = obs[b]
            with np.errstate(invalid="ignore"):
                valid = np.isfinite(ob) & (ob > 0)
            nO = int(valid.sum())
            o["n_obs"][n, b] = nO
            off0 = 0.0 if root_z is None else float(root_z[b])
            o["parts"][n, b, 1] = off0
            if nO == 0:
                continue
            pl = _planes(X, Y, D, faces, fimg)
            inP = valid[pl["py"], pl["px"]]
            py, px, R, bR = pl["py"][inP], pl["px"][inP], pl["R"][inP], pl["bR"][inP]
            nP = int(inP.sum())
            if nP == 0:
                o["dist"][n, b] = trunc
                continue
            off = float(np.mean(ob[py, px] - R)) if root_z is None else off0
            b_off = float(np.mean(bR)) if root_z is None else 0.0
            e = R + off - ob[py, px]
            be = bR + b_off + 2 * U * (np.abs(R) + abs(off) + np.abs(ob[py, px]) + np.abs(e))
            inl = np.abs(e) < trunc
            o["resid_img"][n, b, py, px] = e
            o["b_resid"][n, b, py, px] = be
            o["fragile"][n, b] = int(((np.abs(e) < be) | (np.abs(np.abs(e) - trunc) < be)).sum())
            o["dist"][n, b] = (np.minimum(np.abs(e), trunc).sum() + trunc * (nO - nP)) / nO
            o["b_dist"][n, b] = be.sum() / nO + 2 * U * trunc
            o["parts"][n, b] = (nP / nO, off, inl.mean())
            o["b_offset"][n, b] = b_off + 2 * U * abs(off)
            sg = np.sign(e) * inl
            g = (sg - (sg.mean() if root_z is None else 0.0)) / nO * g_dist[n, b]
            lam, dlx, dly, gx, gy, idx = (pl[k][inP] for k in ("lam", "dlx", "dly", "gx", "gy", "idx"))
            G = np.abs(gx) + np.abs(gy)
            dlam = 2 * DELTA * (np.abs(dlx) + np.abs(dly))                                  # [P,3]
            dgx, dgy = 2 * DELTA * G * np.abs(dlx).sum(1), 2 * DELTA * G * np.abs(dly).sum(1)
            acc, bacc = np.zeros((V, 3)), np.zeros((V, 3))
            ag = np.abs(g)[:, None]
            for c, (sl, dsl) in enumerate(((gx, dgx), (gy, dgy))):
                np.add.at(acc[:, c], idx, -(g * sl)[:, None] * lam)
                np.add.at(bacc[:, c], idx, ag * (np.abs(sl)[:, None] * dlam + lam * dsl[:, None] + 6 * U * np.abs(sl)[:, None] * lam))
            np.add.at(acc[:, 2], idx, g[:, None] * lam)
            np.add.at(bacc[:, 2], idx, ag * (dlam + 6 * U * lam))
            cs = s * S / 2
            gv = acc * np.array([cs, cs, zs])
            bgv = bacc * np.abs(np.array([cs, cs, zs])) + 2 * U * np.abs(gv)
            vx, vy = verts[n, b, :, 0], verts[n, b, :, 1]
            gl = np.array([((acc[:, 0] * vx + acc[:, 1] * vy) * cs).sum(), acc[:, 0].sum() * S / 2, acc[:, 1].sum() * S / 2])
            terms = np.array([(np.abs(acc[:, 0] * vx) + np.abs(acc[:, 1] * vy)).sum() * cs, np.abs(acc[:, 0]).sum() * S / 2, np.abs(acc[:, 1]).sum() * S / 2])
            bgl = np.array([((bacc[:, 0] * np.abs(vx) + bacc[:, 1] * np.abs(vy)) * cs).sum(), bacc[:, 0].sum() * S / 2, bacc[:, 1].sum() * S / 2]) + 4 * U * terms
            o["g_verts"][n, b], o["b_g_verts"][n, b], o["g_logs_t"][n, b], o["b_g_logs_t"][n, b] = gv, bgv, gl, bgl
    return o


def depth_obs64(depth, hand_mask, size):
    """ops.depth_obs's sampling rule in numpy: depth, hand_mask [B,H,H] -> obs [B,size,size]"""
    depth, m = np.asarray(depth, np.float64), np.asarray(hand_mask, np.float64)
    B, H = depth.shape[:2]
    k = H // size
    out = np.zeros((B, size, size))
    for b in range(B):
        for i in range(size):
            for j in range(size):
                d = depth[b, i * k + k // 2, j * k + k // 2]
                if m[b, i * k:(i + 1) * k, j * k:(j + 1) * k].mean() >= 0.5 and np.isfinite(d) and d > 0:
                    out[b, i, j] = d
    return out


# ---- the cases the tests share ------------------------------------------------------------------------------------------------------------
def _big_and_small(rng):
    """one face that covers a third of the image (above the kernel's workgroup-list threshold of 64 samples at S >= 16) in front of / behind
    eight small ones"""
    v = [[-0.7, -0.6, 0.1], [0.75, -0.35, 0.3], [-0.1, 0.8, -0.2]]
    f = [[0, 1, 2]]
    for _ in range(8):
        c = rng.uniform(-0.6, 0.6, 2)
        k = len(v)
        for _ in range(3):
            v.append([*(c + rng.uniform(-0.09, 0.09, 2)), rng.uniform(-0.3, 0.4)])
        f.append([k, k + 1, k + 2])
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def _random_mesh(rng, V=30, F=50):
    """random vertices, faces between near neighbours (a crumpled, closed-ish blob: deep overlap), plus a face with an index outside [0, V)
    and a face of zero area (a repeated index)"""
    v = np.concatenate([rng.uniform(-0.7, 0.7, (V, 2)), rng.uniform(-0.5, 0.5, (V, 1))], 1)
    f = []
    for _ in range(F - 2):
        a = rng.integers(V)
        near = np.argsort(((v[:, :2] - v[a, :2]) ** 2).sum(1))[1:8]
        f.append([a, *rng.choice(near, 2, replace=False)])
    f.insert(7, [3, V + 2, 5])
    f.insert(19, [4, 4, 9])
    return v.astype(np.float32), np.asarray(f, np.int32)


def _tri(rng):
    return np.array([[-0.55, -0.6, 0.1], [0.7, -0.2, 0.4], [0.1, 0.65, -0.3]], np.float32), np.array([[0, 1, 2]], np.int32)


def _mano(rng):
    """V = 778, F = 1,538: a posed mesh of tests/golden/mano.npz under the faces of the synthetic tables it was made with (random vertex
    triples with long edges, deep overlap), shrunk to +-0.3 so that the reference's ambiguous share stays under CAP at S = 64"""
    import os
    from mhentropy_amd import synth
    t = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mano.npz"))
    v = np.asarray(t["mesh"][0], np.float64)
    v = v - v.mean(0)
    return (v / np.abs(v[:, :2]).max() * 0.3).astype(np.float32), np.asarray(synth.mano_tables(int(t["table_seed"]))["faces"]).astype(np.int32)


# name -> (mesh, seed, N, B, S, H / S, what): the seeds of the exact cases were chosen on the CPU for ZERO ambiguous and fragile samples
CASES = {
    "tri_8": (_tri, 0, 1, 1, 8, 1, ""),
    "mix_64": (_big_and_small, 3, 3, 2, 64, 1, "off"),                  # the product size; rows partly off the image
    "mix_16_h64": (_big_and_small, 2, 3, 2, 16, 4, ""),
    "random_16_h64": (_random_mesh, 3, 2, 1, 16, 4, ""),
    "random_8": (_random_mesh, 5, 1, 2, 8, 1, "off"),
    "edges_8": (_big_and_small, 0, 3, 2, 8, 1, "edges"),                # image 1 without observation, row n=1 beside the mask, a NaN vertex in row (2, 0)
    "far_8": (_big_and_small, 0, 2, 2, 8, 4, "far"),                    # every residual beyond trunc (given offset) / all truncated but centred (fitted)
    "mano_64": (_mano, 0, 2, 2, 64, 1, ""),                             # V = 778, F = 1,538: ambiguous samples allowed up to CAP
}
EXACT = tuple(k for k in CASES if k != "mano_64")
TRUNC = 0.05


def operands(name, seed=None):
    """the case's operands as the kernel gets them (float32 / int32): verts, faces, logs_t, zscale, depth, hand_mask, root_z, size"""
    build, seed0, N, B, S, k, what = CASES[name]
    rng = np.random.default_rng((seed0 if seed is None else seed) * 1000 + len(name))
    v1, faces = build(rng)
    H = S * k
    verts = (v1[None, None] + rng.normal(0, 0.01, (N, B) + v1.shape)).astype(np.float32)
    logs_t = np.concatenate([rng.uniform(-0.15, 0.1, (N, B, 1)), rng.uniform(-0.08, 0.08, (N, B, 2))], 2).astype(np.float32)
    if what == "off":
        logs_t[-1, :, 1] += 0.7                                         # the last hypothesis hangs over the right edge
    zscale = rng.uniform(0.07, 0.1, B).astype(np.float32)
    root_z = rng.uniform(0.4, 0.7, B).astype(np.float32)
    yy, xx = np.meshgrid((np.arange(H) + 0.5) / H * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1, indexing="ij")
    mask = np.stack([((xx - rng.uniform(-0.1, 0.1)) ** 2 + (yy - rng.uniform(-0.1, 0.1)) ** 2 < rng.uniform(0.5, 0.7) ** 2) for _ in range(B)])
    depth = (root_z[:, None, None] + rng.uniform(-0.08, 0.08, (B, H, H))).astype(np.float32)
    depth[rng.uniform(0, 1, depth.shape) < 0.05] = 0.0                  # holes of the sensor
    if what == "edges":
        mask[1] = False
        mask[0] = xx < -0.2
        logs_t[1, :, 0], logs_t[1, :, 1] = -1.2, 0.6                    # row n=1: a small mesh right of the mask
        verts[2, 0, 1, 0] = np.nan
    if what == "far":
        depth = (depth + 0.5 * (depth > 0)).astype(np.float32)
    return {"verts": verts, "faces": faces, "logs_t": logs_t, "zscale": zscale, "depth": depth, "hand_mask": mask, "root_z": root_z, "size": S}


@functools.lru_cache(None)
def case(name, root, seed=None):
    """(operands, obs, f64 reference) of a case in one offset mode, computed once and shared: read-only"""
    op = operands(name, seed)
    obs = depth_obs64(op["depth"], op["hand_mask"], op["size"]).astype(np.float32)
    rng = np.random.default_rng(7)
    g_dist = rng.uniform(0.5, 1.5, op["verts"].shape[:2]).astype(np.float32)
    ref = depth_dist64(op["verts"], op["faces"], op["logs_t"], op["zscale"], obs, op["root_z"] if root else None, TRUNC, g_dist)
    op = dict(op, obs=obs, g_dist=g_dist)
    for a in list(op.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return op, ref
