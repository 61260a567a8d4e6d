"""Float64 restatement of the hand-object Chamfer distance (reference hand/criteria.py:18-39, with the per-image vertex count of
mhentropy_amd.criteria.chamfer_dist), its torch-f64 autograd gradient, and the seeded inputs of the chamfer tests.  A helper module, not a test.

    a_j = p_j (scale[b] unit) + root[b];  o_v = obj[b][v], v < V_b
    D1 = mean_j min_v |a_j - o_v|,  D2 = mean_v min_j |a_j - o_v|,  dist = D1 + D2

Inputs are float32 values (what the GPU reads) evaluated in float64.  make_case() re-draws, from the same seeded generator, every hand point
and vertex whose best and second-best distances lie within GAP of each other, so that the argmins of an f32 kernel are determined: ties then
exist only where a test plants them."""
import functools

import numpy as np
import torch

UNIT, ROOT = 1000.0, 12
GAP = 1e-3          # least relative distance between the best and the second-best candidate of every minimum in the index-exact cases


def _pair_dist(points, scale, root, obj, b, Vb):
    """(N, P, V_b) f64 torch distances of image b"""
    a = points[:, b] * (scale[b] * UNIT) + root[b]
    return (a[:, :, None, :] - obj[b, :Vb][None, None]).norm(p=2, dim=-1)


def chamfer64(points, scale, root, obj, count=None):
    """points (N,B,P,3), scale (B,), root (B,3), obj (B,VO,3), count (B,) or None -> dict of numpy arrays: dist (N,B), parts (N,B,2),
    idx_p (N,B,P), idx_o (N,B,VO) (-1 past the count; lowest index on exact ties), gap = the least relative difference between the best and
    the nearest strictly larger candidate over all minima"""
    t = [torch.as_tensor(np.asarray(x, np.float64)) for x in (points, scale, root, obj)]
    N, B, P = t[0].shape[:3]
    VO = t[3].shape[1]
    out = {"dist": np.zeros((N, B)), "parts": np.zeros((N, B, 2)), "idx_p": np.zeros((N, B, P), np.int32), "idx_o": np.full((N, B, VO), -1, np.int32)}
    gap = np.inf
    for b in range(B):
        Vb = VO if count is None else int(count[b])
        d = _pair_dist(*t, b, Vb).numpy()
        for axis, key in ((2, "idx_p"), (1, "idx_o")):
            best = d.min(axis, keepdims=True)
            if d.shape[axis] > 1:
                second = np.where(d > best, d, np.inf).min(axis, keepdims=True)
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = np.where(np.isfinite(second), (second - best) / np.maximum(second, 1e-300), np.inf)
                gap = min(gap, float(rel.min()))
            idx = d.argmin(axis)          # first occurrence: the lowest index on a tie
            if key == "idx_p":
                out[key][:, b] = idx
            else:
                out[key][:, b, :Vb] = idx
        out["parts"][:, b, 0] = d.min(2).mean(1)
        out["parts"][:, b, 1] = d.min(1).mean(1)
    out["dist"] = out["parts"].sum(-1)
    out["gap"] = gap
    return out


def grad64(points, scale, root, obj, g_dist, count=None):
    """d sum(g_dist * dist) / d points by torch autograd in float64 -> (N,B,P,3) numpy"""
    p = torch.as_tensor(np.asarray(points, np.float64)).requires_grad_(True)
    s, r, o = (torch.as_tensor(np.asarray(x, np.float64)) for x in (scale, root, obj))
    g = torch.as_tensor(np.asarray(g_dist, np.float64))
    total = 0.0
    for b in range(p.shape[1]):
        d = _pair_dist(p, s, r, o, b, o.shape[1] if count is None else int(count[b]))
        total = total + (g[:, b] * (d.min(-1)[0].mean(-1) + d.min(-2)[0].mean(-1))).sum()
    return torch.autograd.grad(total, p)[0].numpy()


def _draw_points(rng, shape):
    return rng.normal(0.0, 0.7, shape).astype(np.float32)


def _draw_verts(rng, root_b, shape, spread):
    return (root_b + rng.uniform(-spread, spread, shape)).astype(np.float32)


def _close_calls(points, scale, root, obj, count):
    """masks of the hand points (N,B,P) and vertices (B,VO) with a minimum whose nearest strictly larger candidate is within 2 GAP (an exact tie
    is no close call: it is decided by the index)"""
    N, B, P = points.shape[:3]
    bad_p, bad_o = np.zeros((N, B, P), bool), np.zeros(obj.shape[:2], bool)
    t = [torch.as_tensor(np.asarray(x, np.float64)) for x in (points, scale, root, obj)]
    for b in range(B):
        Vb = obj.shape[1] if count is None else int(count[b])
        d = _pair_dist(*t, b, Vb).numpy()
        for axis in (2, 1):
            best = d.min(axis, keepdims=True)
            second = np.where(d > best, d, np.inf).min(axis, keepdims=True)
            close = np.squeeze((second - best) <= 2 * GAP * second, axis) & np.isfinite(np.squeeze(second, axis))
            if axis == 2:
                bad_p[:, b] = close
            else:
                bad_o[b, :Vb] = close.any(0)
    return bad_p, bad_o


def _plant_ties(points, root, obj):
    """duplicated vertices (5 = 2, 30 = 11) and duplicated hand points (7 = 3, 20 = 0): exact ties"""
    obj[:, 5], obj[:, 30] = obj[:, 2], obj[:, 11]
    points[:, :, 7], points[:, :, 20] = points[:, :, 3], points[:, :, 0]


def _plant_coincident(points, root, obj):
    """hand point 4 of every hypothesis sits at the root (p = 0) and vertex 9 of every image IS the root: a zero distance in both directions"""
    points[:, :, 4] = 0.0
    obj[:, 9] = root


PLANTS = {"ties": _plant_ties, "coincident": _plant_coincident}


@functools.lru_cache(None)
def make_case(seed, N, B, P, VO, count=None, plant=None, spread=90.0):
    """seeded inputs in the units of the data: normalised root-relative points, bone scale in m, root and vertices in mm (within `spread` of
    the root).  count: a tuple of valid vertices per image; the vertices past it are then planted ON hand points of hypothesis 0 (closer than
    any valid vertex).  plant: a key of PLANTS, applied before every check so that what it plants survives the re-draws.
    Returns a dict of read-only float32 / int32 numpy arrays."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.025, 0.04, B).astype(np.float32)
    root = (rng.uniform(-80.0, 80.0, (B, 3)) + np.array([0.0, 0.0, 500.0])).astype(np.float32)
    points = _draw_points(rng, (N, B, P, 3))
    obj = np.stack([_draw_verts(rng, root[b], (VO, 3), spread) for b in range(B)])
    cnt = None if count is None else np.asarray(count, np.int32)
    for _ in range(200):
        if plant is not None:
            PLANTS[plant](points, root, obj)
        bad_p, bad_o = _close_calls(points, scale, root, obj, cnt)
        if not bad_p.any() and not bad_o.any():
            break
        points[bad_p] = _draw_points(rng, (int(bad_p.sum()), 3))
        for b in range(B):
            if bad_o[b].any():
                obj[b, bad_o[b]] = _draw_verts(rng, root[b], (int(bad_o[b].sum()), 3), spread)
    else:
        raise AssertionError("make_case: no draw with every minimum determined")
    if cnt is not None:
        for b in range(B):
            pad = VO - int(cnt[b])
            a = points[0, b].astype(np.float64) * (float(scale[b]) * UNIT) + root[b]
            obj[b, int(cnt[b]):] = (a[np.arange(pad) % P] + 1e-3).astype(np.float32)
    case = {"points": points, "scale": scale, "root": root, "obj": obj}
    if cnt is not None:
        case["count"] = cnt
    for v in case.values():
        v.setflags(write=False)
    return case


def target_of(case, flat=True):
    """the target dict of criteria.chamfer_dist as numpy arrays: original_pose3d carries the root in row 12"""
    B = case["scale"].shape[0]
    pose = np.zeros((B, 21, 3), np.float32)
    pose[:, ROOT] = case["root"]
    t = {"scale": case["scale"], "original_pose3d": pose, "object_verts": case["obj"].reshape(B, -1) if flat else case["obj"]}
    if "count" in case:
        t["object_count"] = case["count"]
    return t
