"""MHEntLoss with the reference's call surface (reference hand/criteria.py:42-173):
`MHEntLoss(loss_weights, aligned)(output, target) -> (total, losses, metrics)`; the metrics
block runs in one HIP kernel (csrc/metrics.hip), the Procrustes alignment of the aligned
evaluation in csrc/procrustes.hip.  chamfer_dist (hand/criteria.py:18-39) and the selection
it was written for (chamfer_select) run on csrc/chamfer.hip; silhouette_iou scores the hypotheses' meshes against the image's hand mask
on csrc/render.hip; silhouette_dist, the differentiable distance of the projected mesh to that mask, and silhouette_select run on
csrc/silhouette.hip; kmeans_select, which summarises the hypotheses by the representatives of Q k-means modes, runs on csrc/kmeans.hip;
mesh_eval, the HO3D mesh protocol (vertex error, F-score, best of n) against target['verts'], and mesh_select run on csrc/mesh_eval.hip;
pck_auc, the 3D PCK curve and its area (AUC) of the joints or of the mesh, and pck_select run on csrc/pck.hip."""
import torch
from torch import nn

from . import ops

# row order of mhe_metrics_f32's [14,B] output
METRIC_KEYS = tuple(f"eucLoss_{sup}_rgb_{row}" for sup in ("3d", "2d")
                    for row in ("sample", "sample_std", "vis", "vis_std", "vis_mean", "invis", "invis_std"))
CHAMFER_UNIT = 1000.0          # hand/criteria.py:24 (normalised -> mm)
CHAMFER_ROOT = 12              # hand/criteria.py:25: the row of original_pose3d the joints are relative to


def chamfer_target_operands(target, B=None, who="chamfer_dist"):
    """the target's half of chamfer_dist's checks, shared with the training term (MHEnt.get_loss(chamfer_w=...)): -> (scale [B],
    root [B,3] = original_pose3d[:, 12], obj [B,VO,3], count [B] int32 | None).  B: the images the caller's other operand has."""
    if "object_verts" not in target:
        raise ValueError(f"{who}: target has no 'object_verts'")
    nb = target["scale"].shape[0]
    if B is not None and B != nb:
        raise ValueError(f"{who}: norm_rel_xyz has {B} images, target['scale'] {nb}")
    B = nb
    obj = target["object_verts"]
    if obj.dim() not in (2, 3) or obj.shape[0] != B or obj[0].numel() % 3 or obj[0].numel() == 0 or (obj.dim() == 3 and obj.shape[2] != 3):
        raise ValueError(f"{who}: target['object_verts'] must be (B, VO*3) or (B, VO, 3) with B={B}, got {tuple(obj.shape)}")
    obj = obj.reshape(B, -1, 3)
    count = target.get("object_count")
    if count is not None:
        if tuple(count.shape) != (B,) or count.dtype != torch.int32:
            raise ValueError(f"{who}: target['object_count'] must be a (B,) int32 tensor, got {tuple(count.shape)} {count.dtype}")
        # (one host read; a stream that is being captured cannot take it: the kernel clamps the count to 1..VO there)
        if not (count.is_cuda and torch.cuda.is_current_stream_capturing()) and not (1 <= int(count.min()) and int(count.max()) <= obj.shape[1]):
            raise ValueError(f"{who}: target['object_count'] outside 1..VO={obj.shape[1]}")
    root = target["original_pose3d"]
    if root.dim() != 3 or root.shape[0] != B or root.shape[1] <= CHAMFER_ROOT or root.shape[2] != 3:
        raise ValueError(f"{who}: target['original_pose3d'] must be (B, >={CHAMFER_ROOT + 1}, 3), got {tuple(root.shape)}")
    return target["scale"].contiguous(), root[:, CHAMFER_ROOT].contiguous(), obj.contiguous(), count


def _chamfer_operands(norm_rel_xyz, target):
    """the checks of chamfer_dist that need no device -> (points [N,B,P,3], scale, root, obj [B,VO,3], count or None, input was 3-D)"""
    if "object_verts" not in target:
        raise ValueError("chamfer_dist: target has no 'object_verts'")
    if not isinstance(norm_rel_xyz, torch.Tensor) or norm_rel_xyz.dim() not in (3, 4) or norm_rel_xyz.shape[-1] != 3:
        raise ValueError(f"chamfer_dist: norm_rel_xyz must be (N, B, K, 3) or (B, K, 3), got {tuple(getattr(norm_rel_xyz, 'shape', ()))}")
    single = norm_rel_xyz.dim() == 3
    pts = norm_rel_xyz[None] if single else norm_rel_xyz
    if pts.shape[1] != target["scale"].shape[0]:
        raise ValueError(f"chamfer_dist: norm_rel_xyz has {pts.shape[1]} images, target['scale'] {target['scale'].shape[0]}")
    if not 1 <= pts.shape[2] <= 778:
        raise ValueError(f"chamfer_dist: K={pts.shape[2]} points per hypothesis (1..778)")
    scale, root, obj, count = chamfer_target_operands(target, pts.shape[1])
    return pts.contiguous(), scale, root, obj, count, single


class _Chamfer(torch.autograd.Function):
    """dist [N,B] of ops.chamfer; the gradient reaches the points only.  The argmin buffers are asked for only when the points require grad."""
    @staticmethod
    def forward(ctx, pts, scale, root, obj, count):
        if ctx.needs_input_grad[0]:
            dist, _, idx_p, idx_o = ops.chamfer(pts, scale, root, obj, count, CHAMFER_UNIT, want_idx=True)
            ctx.save_for_backward(pts, scale, root, obj, idx_p, idx_o)
            ctx.count = count
        else:
            dist, _ = ops.chamfer(pts, scale, root, obj, count, CHAMFER_UNIT)
        return dist

    @staticmethod
    def backward(ctx, g_dist):
        pts, scale, root, obj, idx_p, idx_o = ctx.saved_tensors
        return ops.chamfer_bwd(pts, scale, root, obj, ctx.count, idx_p, idx_o, g_dist.contiguous(), CHAMFER_UNIT), None, None, None, None


def chamfer_dist(norm_rel_xyz, target: dict):
    """reference hand/criteria.py:18-39: the symmetric Chamfer distance, in mm, between every hypothesis' points
    `norm_rel_xyz * target['scale'] * 1000 + target['original_pose3d'][:, 12]` and its image's object vertices target['object_verts']
    ((B, VO*3) or (B, VO, 3)): mean over the points of the distance to the nearest vertex plus mean over the vertices of the distance to the
    nearest point.  norm_rel_xyz (N, B, K, 3) -> (N, B); (B, K, 3) -> (B,).  K <= 778.
    Extension: target['object_count'], (B,) int32 in 1..VO - only the first count vertices of an image take part (the zero-padded meshes
    of the input pipeline with object_idx=None and their raw['obj_count']).
    Differentiable with respect to norm_rel_xyz.  HIP tensors only (MheError otherwise); ValueError for a missing 'object_verts', a rank
    other than 3 or 4, shapes that do not agree and a count outside 1..VO."""
    pts, scale, root, obj, count, single = _chamfer_operands(norm_rel_xyz, target)
    dist = _Chamfer.apply(pts, scale, root, obj, count)
    return dist[0] if single else dist


def _rank(dist):
    """dist (N, B) -> (values, n) ascending over N, ties to the lower n"""
    return torch.sort(dist, dim=0, stable=True)


def _select_shape(who, name, src, Q):
    """the checks every selection shares -> (N, B) of src = output[name], an (N, B, ...) tensor"""
    if src.dim() < 3:
        raise ValueError(f"{who}: output[{name!r}] must be (N, B, ...), got {tuple(src.shape)}")
    N, B = src.shape[:2]
    if not isinstance(Q, int) or not 1 <= Q <= N:
        raise ValueError(f"{who}: Q={Q!r} outside 1..N={N}")
    return N, B


def _cut(output, dist, Q, key):
    """rank dist (N, B) and cut every (N, B, ...) tensor of `output` to its Q best hypotheses per image; 'faces' and 'image' pass through.
    Added: `key` (Q, B), the distances, and `key`_index (Q, B) int64, the hypotheses kept."""
    N, B = dist.shape
    val, order = _rank(dist)
    keep, cols = order[:Q], torch.arange(B, device=order.device)
    out = {}
    for k, v in output.items():
        cut = isinstance(v, torch.Tensor) and k not in ("faces", "image") and v.dim() >= 2 and tuple(v.shape[:2]) == (N, B)
        out[k] = v[keep, cols] if cut else v
    out[key], out[key + "_index"] = val[:Q], keep
    return out


def chamfer_select(output, target, Q=1, points="xyz"):
    """Keep, per image, the Q hypotheses of a sample() output that lie closest to the image's object (chamfer_dist of the joints
    output['xyz'], or of the mesh output['verts'] with points='verts'), closest first, ties to the lower n.  Every (N, B, ...) tensor of
    `output` is cut to (Q, B, ...); everything else ('faces', 'image') passes through.  Added: 'chamfer' (Q, B), the distances in mm, and
    'chamfer_index' (Q, B) int64, the hypotheses kept."""
    if points not in ("xyz", "verts"):
        raise ValueError(f"chamfer_select: points={points!r} (xyz or verts)")
    if points not in output:
        raise ValueError(f"chamfer_select: output has no {points!r}")
    src = output[points]
    N, B = _select_shape("chamfer_select", points, src, Q)
    with torch.no_grad():
        dist = chamfer_dist(src.detach().reshape(N, B, -1, 3), target)
    return _cut(output, dist, Q, "chamfer")


MESH_UNIT = 1000.0             # normalised -> mm, as CHAMFER_UNIT


def _mesh_operands(who, output, target, thresholds=(5.0,), ns=None):
    """the checks of mesh_eval that need no device -> (verts (N, B, V, 3) view-shaped, target verts (B, V, 3), scale (B,), thresholds, ns | None)"""
    if "verts" not in output:
        raise ValueError(f"{who}: output has no 'verts'")
    for k in ("verts", "scale"):
        if k not in target:
            raise ValueError(f"{who}: target has no {k!r}")
    pv, tv, scale = output["verts"], target["verts"], target["scale"]
    if not isinstance(pv, torch.Tensor) or pv.dim() not in (3, 4) or (pv.dim() == 4 and pv.shape[-1] != 3) or pv.shape[2:].numel() % 3:
        raise ValueError(f"{who}: output['verts'] must be (N, B, V*3) or (N, B, V, 3), got {tuple(getattr(pv, 'shape', ()))}")
    N, B, V = pv.shape[0], pv.shape[1], pv.shape[2:].numel() // 3
    if not isinstance(tv, torch.Tensor) or tv.dim() not in (2, 3) or (tv.dim() == 3 and tv.shape[-1] != 3) or tv.shape[1:].numel() % 3:
        raise ValueError(f"{who}: target['verts'] must be (B, V*3) or (B, V, 3), got {tuple(getattr(tv, 'shape', ()))}")
    if tv.shape[0] != B:
        raise ValueError(f"{who}: output['verts'] has B={B} images, target['verts'] {tv.shape[0]}")
    if tv.shape[1:].numel() // 3 != V:
        raise ValueError(f"{who}: output['verts'] has V={V} vertices, target['verts'] {tv.shape[1:].numel() // 3}")
    if not 1 <= V <= ops.MESH_EVAL_MAX_VERTS:
        raise ValueError(f"{who}: output['verts'] has V={V} vertices per hypothesis (1..{ops.MESH_EVAL_MAX_VERTS})")
    if not 1 <= N or not 1 <= B:
        raise ValueError(f"{who}: output['verts'] is empty, {tuple(pv.shape)}")
    if not isinstance(scale, torch.Tensor) or tuple(scale.shape) != (B,):
        raise ValueError(f"{who}: target['scale'] must be (B,) = ({B},), got {tuple(getattr(scale, 'shape', ()))}")
    try:
        thr = tuple(float(t) for t in thresholds)
    except TypeError:
        raise ValueError(f"{who}: thresholds must be 1 to {ops.MESH_EVAL_MAX_THRESHOLDS} positive numbers, got {thresholds!r}") from None
    if not 1 <= len(thr) <= ops.MESH_EVAL_MAX_THRESHOLDS:
        raise ValueError(f"{who}: thresholds holds {len(thr)} numbers (1..{ops.MESH_EVAL_MAX_THRESHOLDS})")
    if any(not t > 0 for t in thr):
        raise ValueError(f"{who}: thresholds must be positive, got {thr!r}")
    if ns is not None:
        ns = _check_ns(who, ns, N)
    return pv.detach().reshape(N, B, V, 3), tv.detach().reshape(B, V, 3), scale.detach(), thr, ns


def _min_first_n(err, ns):
    """err (B', N) f32 contiguous -> (values, index), each (B', len(ns)): the least of the first ns[i] entries of a row and the lowest n that
    attains it (mhe_min_of_n_f32)"""
    import ctypes as C
    Bp, N = err.shape
    val = torch.empty(Bp, len(ns), device=err.device, dtype=torch.float32)
    idx = torch.empty(Bp, len(ns), device=err.device, dtype=torch.int32)
    ops.launch("mhe_min_of_n_f32", err, val, idx, Bp, N, C.cast((C.c_int * len(ns))(*ns), C.c_void_p), len(ns))
    return val, idx


def mesh_eval(output, target, thresholds=(5.0, 15.0), aligned=False, ns=None):
    """The HO3D / FreiHAND mesh protocol for every hypothesis of a sample() output: output['verts'] (N, B, V*3) or (N, B, V, 3) against the
    image's ground-truth mesh target['verts'] (B, V*3) or (B, V, 3), both normalised; with p_v = verts * target['scale'] * 1000 (mm) and g_w the
    target's vertices scaled alike,
        mesh_err  (N, B)     mean over v of |p_v - g_v|, the vertex-to-vertex error by correspondence, in mm
        precision (T, N, B)  share of the predicted vertices whose nearest target vertex is closer than thresholds[t] (mm; strictly)
        recall    (T, N, B)  share of the target vertices whose nearest predicted vertex is closer than thresholds[t]
        f_score   (T, N, B)  2 P R / (P + R), 0 when both are 0
    aligned=True: every hypothesis' mesh is first Procrustes-aligned with scale to its target (ops.procrustes_align, the alignment of
    MHEntLoss(aligned=True)) and the aligned mesh is evaluated; output['verts'] is not replaced.
    ns=[n1, ...] (strictly increasing, within 1..N): best of the first n hypotheses - adds mesh_err_min and mesh_err_index (len(ns), B), the
    least mesh_err among hypotheses 0 .. n-1 and the lowest n attaining it (int64), and f_score_max (T, len(ns), B).
    No gradient.  Runs on csrc/mesh_eval.hip (no (N B, V, V) tensor exists); HIP tensors only (MheError otherwise).  ValueError, before
    anything touches the device, for a missing 'verts' on either side, B or V that disagree, V outside 1..778, no thresholds or more than 4,
    a threshold that is not positive, ns outside 1..N."""
    return _mesh_eval("mesh_eval", output, target, thresholds, aligned, ns)


def _mesh_eval(who, output, target, thresholds, aligned, ns):
    pv, tv, scale, thr, ns = _mesh_operands(who, output, target, thresholds, ns)
    with torch.no_grad():
        pv, tv, scale = pv.float().contiguous(), tv.float().contiguous(), scale.float().contiguous()
        if aligned:
            pv = ops.procrustes_align(pv, tv)
        err, prf = ops.mesh_eval(pv, tv, scale, thr, MESH_UNIT)
        res = {"mesh_err": err, "precision": prf[0], "recall": prf[1], "f_score": prf[2]}
        if ns is not None:
            N, B = err.shape
            val, idx = _min_first_n(err.t().contiguous(), ns)
            res["mesh_err_min"], res["mesh_err_index"] = val.t().contiguous(), idx.t().long()
            fmax, _ = _min_first_n(prf[2].permute(0, 2, 1).neg().reshape(-1, N), ns)          # max F = -min(-F)
            res["f_score_max"] = fmax.neg().view(len(thr), B, len(ns)).permute(0, 2, 1).contiguous()
    return res


def mesh_select(output, target, Q=1, aligned=False):
    """chamfer_select with the ground truth: keep, per image, the Q hypotheses of a sample() output whose mesh has the least mesh_err (mesh_eval;
    aligned as there), least first, ties to the lower n - the oracle selection that best-of-n tables are made from.  Every (N, B, ...) tensor of
    `output` is cut to (Q, B, ...); 'faces' and 'image' pass through.  Added: 'mesh_err' (Q, B), in mm, and 'mesh_err_index' (Q, B) int64."""
    if "verts" not in output:
        raise ValueError("mesh_select: output has no 'verts'")
    _select_shape("mesh_select", "verts", output["verts"], Q)
    return _cut(output, _mesh_eval("mesh_select", output, target, (5.0,), aligned, None)["mesh_err"], Q, "mesh_err")


PCK_TARGET = {"xyz": "pose3d", "verts": "verts"}          # the target's key for output[points]


def _check_ns(who, ns, N):
    ns = (ns,) if isinstance(ns, int) else tuple(ns)
    if not 1 <= len(ns) <= 8 or any(not isinstance(n, int) or isinstance(n, bool) for n in ns):
        raise ValueError(f"{who}: ns must hold 1 to 8 integers, got {ns!r}")
    if any(not 1 <= n <= N for n in ns) or any(b <= a for a, b in zip(ns, ns[1:])):
        raise ValueError(f"{who}: ns must be strictly increasing within 1..N={N}, got {ns!r}")
    return ns


def _pck_operands(who, output, target, points, vmin, vmax, steps, ns, valid):
    """the checks of pck_auc that need no device -> (points (N, B, P, 3) view-shaped, target points (B, P, 3), scale (B,), thresholds (T,) f32
    numpy, ns | None, valid (B, P) | None)"""
    import numpy as np
    if points not in PCK_TARGET:
        raise ValueError(f"{who}: points={points!r} (xyz or verts)")
    tkey = PCK_TARGET[points]
    if points not in output:
        raise ValueError(f"{who}: output has no {points!r}")
    for k in (tkey, "scale"):
        if k not in target:
            raise ValueError(f"{who}: target has no {k!r}")
    pv, tv, scale = output[points], target[tkey], target["scale"]
    if not isinstance(pv, torch.Tensor) or pv.dim() not in (3, 4) or (pv.dim() == 4 and pv.shape[-1] != 3) or pv.shape[2:].numel() % 3:
        raise ValueError(f"{who}: output[{points!r}] must be (N, B, P*3) or (N, B, P, 3), got {tuple(getattr(pv, 'shape', ()))}")
    N, B, P = pv.shape[0], pv.shape[1], pv.shape[2:].numel() // 3
    if not isinstance(tv, torch.Tensor) or tv.dim() not in (2, 3) or (tv.dim() == 3 and tv.shape[-1] != 3) or tv.shape[1:].numel() % 3:
        raise ValueError(f"{who}: target[{tkey!r}] must be (B, P*3) or (B, P, 3), got {tuple(getattr(tv, 'shape', ()))}")
    if tv.shape[0] != B:
        raise ValueError(f"{who}: output[{points!r}] has B={B} images, target[{tkey!r}] {tv.shape[0]}")
    if tv.shape[1:].numel() // 3 != P:
        raise ValueError(f"{who}: output[{points!r}] has P={P} points, target[{tkey!r}] {tv.shape[1:].numel() // 3}")
    if not 1 <= P <= ops.PCK_MAX_POINTS:
        raise ValueError(f"{who}: output[{points!r}] has P={P} points per hypothesis (1..{ops.PCK_MAX_POINTS})")
    if not 1 <= N or not 1 <= B:
        raise ValueError(f"{who}: output[{points!r}] is empty, {tuple(pv.shape)}")
    if not isinstance(scale, torch.Tensor) or tuple(scale.shape) != (B,):
        raise ValueError(f"{who}: target['scale'] must be (B,) = ({B},), got {tuple(getattr(scale, 'shape', ()))}")
    if isinstance(steps, bool) or not isinstance(steps, int) or not 2 <= steps <= ops.PCK_MAX_THRESHOLDS:
        raise ValueError(f"{who}: steps={steps!r} (an integer in 2..{ops.PCK_MAX_THRESHOLDS})")
    try:
        vmin, vmax = float(vmin), float(vmax)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: vmin={vmin!r}, vmax={vmax!r} must be numbers") from None
    if not (np.isfinite(vmin) and np.isfinite(vmax)) or not vmax > vmin:
        raise ValueError(f"{who}: vmin={vmin!r}, vmax={vmax!r} must be finite with vmax > vmin")
    thr = np.linspace(vmin, vmax, steps).astype(np.float32)          # f64, rounded once
    if not np.isfinite(thr).all() or not (np.diff(thr) > 0).all():
        raise ValueError(f"{who}: {steps} steps from vmin={vmin!r} to vmax={vmax!r} are not strictly ascending in float32")
    if ns is not None:
        ns = _check_ns(who, ns, N)
    if valid is not None and (not isinstance(valid, torch.Tensor) or tuple(valid.shape) != (B, P) or valid.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"{who}: valid must be a (B, P) = ({B}, {P}) bool or uint8 tensor, got {tuple(getattr(valid, 'shape', ()))} "
                         f"{getattr(valid, 'dtype', type(valid))}")
    return pv.detach().reshape(N, B, P, 3), tv.detach().reshape(B, P, 3), scale.detach(), thr, ns, valid


def pck_auc(output, target, points="xyz", vmin=0.0, vmax=50.0, steps=100, aligned=False, ns=None, valid=None, curve=False):
    """The 3D PCK curve of every hypothesis of a sample() output and the area under it (the AUC of the HO3D / FreiHAND leaderboards):
    points='xyz': the joints output['xyz'] (N, B, 63) against target['pose3d'] (B, 63); points='verts': output['verts'] (N, B, V*3) or
    (N, B, V, 3) against target['verts'].  Both sides are scaled by target['scale'] * 1000 (mm), d_p is the distance of point p to its ground
    truth, and with thresholds = np.linspace(vmin, vmax, steps) (computed in f64, rounded to f32; mm)
        hits (N, B, T) int32   the valid points with d_p <= thresholds[i] (inclusive); PCK = hits / n_valid          (curve=True only)
        auc  (N, B)            trapezoid area under the PCK curve over the trapezoid of the constant 1: in [0, 1]
        err  (N, B)            mean of d_p over the valid points, in mm
        thresholds (T,)        the f32 table, on the device
        n_valid (B,) int32     the valid points of every image                                                     (curve=True only)
    The integer hits and n_valid of several batches can be added into a pooled curve without rounding (harness.PckPool).
    valid (B, P) bool or uint8: the points that count; an image with none gives hits 0 and auc = err = NaN.
    aligned=True: every hypothesis is first Procrustes-aligned with scale to its target (ops.procrustes_align, as mesh_eval); the output's
    tensor is not replaced.  ns=[n1, ...] (strictly increasing, within 1..N): adds auc_max and auc_index (len(ns), B), the largest auc among
    hypotheses 0 .. n-1 and the lowest n attaining it (int64).
    No gradient.  Runs on csrc/pck.hip (no per-point distance is written); HIP tensors only (MheError otherwise).  ValueError, before anything
    touches the device, for a missing key, B or P that disagree, P outside 1..778, steps outside 2..256, vmin or vmax non-finite or
    vmax <= vmin, ns outside 1..N or not increasing, a valid of the wrong shape or dtype."""
    return _pck_auc("pck_auc", output, target, points, vmin, vmax, steps, aligned, ns, valid, curve)


def _pck_auc(who, output, target, points, vmin, vmax, steps, aligned, ns, valid, curve):
    pv, tv, scale, thr, ns, valid = _pck_operands(who, output, target, points, vmin, vmax, steps, ns, valid)
    with torch.no_grad():
        pv, tv, scale = pv.float().contiguous(), tv.float().contiguous(), scale.float().contiguous()
        if not pv.is_cuda:
            raise ops._lib.MheError(f"{who}: expected CUDA/HIP tensors (the hot path has no CPU fallback)")
        if valid is not None:
            valid = valid.contiguous()
        if aligned:
            pv = ops.procrustes_align(pv, tv)
        table = ops.pck_thresholds(thr, pv.device)
        hits, auc, err = ops.pck_curve(pv, tv, scale, table, valid, MESH_UNIT, want_hits=curve)
        res = {"auc": auc, "err": err, "thresholds": table}
        if curve:
            B, P = tv.shape[:2]
            res["hits"] = hits
            res["n_valid"] = torch.full((B,), P, device=pv.device, dtype=torch.int32) if valid is None else (valid != 0).sum(1, dtype=torch.int32)
        if ns is not None:
            val, idx = _min_first_n(auc.neg().t().contiguous(), ns)          # max auc = -min(-auc)
            res["auc_max"], res["auc_index"] = val.neg().t().contiguous(), idx.t().long()
    return res


def pck_select(output, target, Q=1, points="xyz", aligned=False):
    """mesh_select ranked on the AUC: keep, per image, the Q hypotheses of a sample() output of largest auc (pck_auc with its default
    thresholds; points and aligned as there), largest first, ties to the lower n.  Every (N, B, ...) tensor of `output` is cut to (Q, B, ...);
    'faces' and 'image' pass through.  Added: 'auc' (Q, B) and 'auc_index' (Q, B) int64."""
    if points not in PCK_TARGET:
        raise ValueError(f"pck_select: points={points!r} (xyz or verts)")
    if points not in output:
        raise ValueError(f"pck_select: output has no {points!r}")
    _select_shape("pck_select", points, output[points], Q)
    out = _cut(output, _pck_auc("pck_select", output, target, points, 0.0, 50.0, 100, aligned, None, None, False)["auc"].neg(), Q, "auc")
    out["auc"] = out["auc"].neg()
    return out


def silhouette_mask_checks(hand_mask, B, size, who="silhouette_dist"):
    """the mask's half of silhouette_dist's shape checks, shared with the training term (MHEnt.get_loss(sil_w=...)): hand_mask (B, H, H) with
    H a multiple of size, size an int in 1..64.  B None: taken from the mask."""
    if not isinstance(hand_mask, torch.Tensor) or hand_mask.dim() != 3 or (B is not None and hand_mask.shape[0] != B) or \
            hand_mask.shape[1] != hand_mask.shape[2]:
        raise ValueError(f"{who}: hand_mask must be (B, H, H){'' if B is None else f' with B={B}'}, got {tuple(getattr(hand_mask, 'shape', ()))}")
    if not isinstance(size, int) or not 1 <= size <= ops.SILHOUETTE_MAX_SIZE:
        raise ValueError(f"{who}: size={size!r} (1..{ops.SILHOUETTE_MAX_SIZE})")
    H = hand_mask.shape[1]
    if H < size or H % size:
        raise ValueError(f"{who}: hand_mask is {H} x {H}, not a multiple of size={size}")


def silhouette_occluder_checks(occluder, hand_mask, who="silhouette_dist"):
    """the occluder's shape checks, after the mask's: (B, H, H) like hand_mask -> the occluder, contiguous, bool / uint8 / float32 (any other
    type is converted as the mask is)"""
    if not isinstance(occluder, torch.Tensor) or occluder.dim() != 3 or tuple(occluder.shape) != tuple(hand_mask.shape):
        raise ValueError(f"{who}: occluder must be (B, H, H) = {tuple(hand_mask.shape)} like hand_mask, got {tuple(getattr(occluder, 'shape', ()))}")
    if occluder.dtype not in (torch.bool, torch.uint8, torch.float32):
        occluder = occluder.float()
    return occluder.contiguous()


def _silhouette_operands(verts, logs_t, hand_mask, size, occluder=None):
    """the checks of silhouette_dist that need no device -> (verts [N,B,V,3], logs_t [N,B,3], hand_mask [B,H,H], size, occluder [B,H,H] | None)"""
    who = "silhouette_dist"
    if not isinstance(verts, torch.Tensor) or verts.dim() not in (3, 4) or (verts.dim() == 4 and verts.shape[-1] != 3) or verts[0, 0].numel() % 3:
        raise ValueError(f"{who}: verts must be (N, B, V*3) or (N, B, V, 3), got {tuple(getattr(verts, 'shape', ()))}")
    N, B = verts.shape[:2]
    V = verts[0, 0].numel() // 3
    if not 1 <= V <= ops.SILHOUETTE_MAX_VERTS:
        raise ValueError(f"{who}: V={V} vertices per hypothesis (1..{ops.SILHOUETTE_MAX_VERTS})")
    if not isinstance(logs_t, torch.Tensor) or tuple(logs_t.shape) != (N, B, 3):
        raise ValueError(f"{who}: logs_t must be (N, B, 3) = ({N}, {B}, 3), got {tuple(getattr(logs_t, 'shape', ()))}")
    silhouette_mask_checks(hand_mask, B, size, who)
    if occluder is not None:
        occluder = silhouette_occluder_checks(occluder, hand_mask, who)
    if hand_mask.dtype not in (torch.bool, torch.uint8, torch.float32):
        hand_mask = hand_mask.float()
    return verts.reshape(N, B, V, 3).float().contiguous(), logs_t.float().contiguous(), hand_mask.contiguous(), size, occluder


class _Silhouette(torch.autograd.Function):
    """(dist, parts) of ops.silhouette_dist; the gradient of dist reaches verts and logs_t (parts is returned for reading only).  The argmin
    buffers are asked for only when one of them requires grad.  count_all (None: no occluder section) is saved next to count."""
    @staticmethod
    def forward(ctx, verts, logs_t, pixels, count, count_all):
        ctx.occ = count_all is not None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dist, parts, idx_v, idx_m = ops.silhouette_dist(verts, logs_t, pixels, count, want_idx=True, count_all=count_all)
            ctx.save_for_backward(verts, logs_t, pixels, count, idx_v, idx_m, *((count_all,) if ctx.occ else ()))
        else:
            dist, parts = ops.silhouette_dist(verts, logs_t, pixels, count, count_all=count_all)
        ctx.mark_non_differentiable(parts)
        return dist, parts

    @staticmethod
    def backward(ctx, g_dist, _g_parts):
        saved = ctx.saved_tensors
        g_verts, g_logs_t = ops.silhouette_dist_bwd(*saved[:6], g_dist.contiguous(), count_all=saved[6] if ctx.occ else None)
        return g_verts, g_logs_t, None, None, None


def silhouette_dist(verts, logs_t, hand_mask, size=64, parts=False, occluder=None):
    """Distance of every hypothesis' projected mesh to its image's hand mask: verts (N, B, V*3) or (N, B, V, 3) and logs_t (N, B, 3) =
    (log s, tx, ty) of a sample() output, hand_mask (B, H, H) bool or float in [0, 1] (the input pipeline's target['hand_mask']) -> (N, B)
    f32; with parts=True (dist, inside, cover).  In the normalised image coordinates of silhouette_iou (pixel (i, j) of the size x size grid is
    the square of half-width 1/size around ((2j+1)/size - 1, (2i+1)/size - 1)): H must be a multiple of `size`, the mask is box-averaged
    down to (size, size) and the pixels with a mean >= 0.5 are kept; with p_v = exp(log s) v_xy + t,
        inside = mean over the vertices of the distance from p_v to the nearest kept pixel square (0 inside the mask: pulls the mesh in)
        cover  = mean over the kept pixels of the distance from the pixel's centre to the nearest p_v (pulls the mesh over the whole mask)
        dist   = inside + cover
    Exact (no soft rasteriser) and deterministic; ties go to the lowest index.  An image with an empty mask gives 0 and a zero gradient,
    a row with a non-finite projected vertex NaN and a zero gradient.  Differentiable with respect to verts and logs_t (the z column of the
    vertices and the mask get none; inside and cover are returned detached).  Runs on csrc/silhouette.hip, nothing on the host reads the
    pixel count: the call can be captured into a HIP graph.  HIP tensors only (MheError otherwise); ValueError for a bad rank or shape, H not
    a multiple of size, V outside 1..778.  The reverse of the mesh exists (ManoLayer.verts carries the gradient on to z: ops.mano_verts_bwd), and
    the training term is MHEnt.get_loss(sil_w=...): log_p -= sil_w * mean_n of this distance, whose reverse (ops.silhouette_dist_grad) holds the
    argmins in registers and LDS instead of the two index tensors this function's autograd node keeps.
    occluder (B, H, H) with the mask's H, bool / uint8 / float (the input pipeline's target['object_mask']): the object in front of the hand.
    Its kept pixels that are not hand pixels are where the mesh MAY project but need not: inside takes its minimum over the hand's and the
    occluder's pixels (a vertex behind the object costs 0, and is pulled toward the object no more than toward the hand), cover stays the mean
    over the hand's pixels alone (the occluder attracts nothing).  At equal distance the hand pixel is chosen.  An image with no hand pixel
    gives 0 and a zero gradient whatever the occluder holds; an all-zero occluder gives the bits of occluder=None.  ValueError for an
    occluder of another rank, B or H, before any launch."""
    v, lt, mask, size, occ = _silhouette_operands(verts, logs_t, hand_mask, size, occluder)
    lists = ops.silhouette_pixels(mask, size, occ)
    dist, pt = _Silhouette.apply(v, lt, lists[0], lists[1], lists[2] if occ is not None else None)
    return (dist, pt[..., 0], pt[..., 1]) if parts else dist


def silhouette_select(output, target, Q=1, size=64, occluder=False):
    """chamfer_select with silhouette_dist: keep, per image, the Q hypotheses of a sample() output whose mesh (output['verts'] under
    output['logs_t']) lies closest to target['hand_mask'], closest first, ties to the lower n.  Every (N, B, ...) tensor of `output` is cut
    to (Q, B, ...); 'faces' and 'image' pass through.  Added: 'silhouette' (Q, B), the distances, and 'silhouette_index' (Q, B) int64.
    occluder: True reads target['object_mask'] (ValueError when it is absent), a tensor is used as given - silhouette_dist's occluder, so a
    hypothesis is not ranked down for the fingers it puts behind the object."""
    for k in ("verts", "logs_t"):
        if k not in output:
            raise ValueError(f"silhouette_select: output has no {k!r}")
    if "hand_mask" not in target:
        raise ValueError("silhouette_select: target has no 'hand_mask'")
    if occluder is True:
        if "object_mask" not in target:
            raise ValueError("silhouette_select(occluder=True): target has no 'object_mask'")
        occluder = target["object_mask"]
    elif occluder is False:
        occluder = None
    N, B = _select_shape("silhouette_select", "verts", output["verts"], Q)
    with torch.no_grad():
        dist = silhouette_dist(output["verts"].detach(), output["logs_t"].detach(), target["hand_mask"], size=size, occluder=occluder)
    return _cut(output, dist, Q, "silhouette")


def _depth_operands(who, verts, logs_t, faces, depth, hand_mask, scale, root_z, size, trunc):
    """the checks of depth_dist that need no device -> (verts [N,B,V,3], logs_t [N,B,3], faces [F,3] int32, depth, hand_mask, scale [B],
    root_z [B] | None)"""
    if not isinstance(verts, torch.Tensor) or verts.dim() not in (3, 4) or (verts.dim() == 4 and verts.shape[-1] != 3) or verts[0, 0].numel() % 3:
        raise ValueError(f"{who}: verts must be (N, B, V*3) or (N, B, V, 3), got {tuple(getattr(verts, 'shape', ()))}")
    N, B = verts.shape[:2]
    V = verts[0, 0].numel() // 3
    if not 1 <= V <= ops.DEPTH_MAX_VERTS:
        raise ValueError(f"{who}: V={V} vertices per hypothesis (1..{ops.DEPTH_MAX_VERTS})")
    if not isinstance(logs_t, torch.Tensor) or tuple(logs_t.shape) != (N, B, 3):
        raise ValueError(f"{who}: logs_t must be (N, B, 3) = ({N}, {B}, 3), got {tuple(getattr(logs_t, 'shape', ()))}")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point() or \
            not 1 <= faces.shape[0] <= ops.DEPTH_MAX_FACES:
        raise ValueError(f"{who}: faces must be an integer (F, 3) tensor with F in 1..{ops.DEPTH_MAX_FACES}, got "
                         f"{tuple(getattr(faces, 'shape', ()))} {getattr(faces, 'dtype', None)}")
    if not isinstance(size, int) or not 1 <= size <= ops.DEPTH_MAX_SIZE:
        raise ValueError(f"{who}: size={size!r} (1..{ops.DEPTH_MAX_SIZE})")
    for name, img in (("depth", depth), ("hand_mask", hand_mask)):
        if not isinstance(img, torch.Tensor) or img.dim() != 3 or img.shape[0] != B or img.shape[1] != img.shape[2]:
            raise ValueError(f"{who}: {name} must be (B, H, H) with B={B}, got {tuple(getattr(img, 'shape', ()))}")
    if tuple(hand_mask.shape) != tuple(depth.shape):
        raise ValueError(f"{who}: hand_mask is {tuple(hand_mask.shape)}, depth {tuple(depth.shape)}")
    H = depth.shape[1]
    if H < size or H % size:
        raise ValueError(f"{who}: depth is {H} x {H}, not a multiple of size={size}")
    if not isinstance(scale, torch.Tensor) or tuple(scale.shape) != (B,):
        raise ValueError(f"{who}: scale must be (B,) = ({B},), got {tuple(getattr(scale, 'shape', ()))}")
    if root_z is not None and (not isinstance(root_z, torch.Tensor) or tuple(root_z.shape) != (B,)):
        raise ValueError(f"{who}: root_z must be (B,) = ({B},) or None, got {tuple(getattr(root_z, 'shape', ()))}")
    if isinstance(trunc, bool) or not isinstance(trunc, (int, float)) or not 0 < trunc < float("inf"):
        raise ValueError(f"{who}: trunc={trunc!r} (a positive, finite number)")
    if faces.dtype != torch.int32:          # (sample()'s output['faces'] is int64: converted once per tensor and kept beside it, with its adjacency)
        kept = getattr(faces, "_mhe_i32", None)
        if kept is None or kept[0] != faces._version:
            kept = (faces._version, faces.to(torch.int32).contiguous())
            faces._mhe_i32 = kept
        faces = kept[1]
    return (verts.reshape(N, B, V, 3).float().contiguous(), logs_t.float().contiguous(), faces.contiguous(), depth, hand_mask,
            scale.detach().float().contiguous(), None if root_z is None else root_z.detach().float().contiguous())


class _Depth(torch.autograd.Function):
    """(dist, parts) of ops.depth_dist; the gradient of dist reaches verts and logs_t (parts is returned for reading only).  Only the inputs are
    saved: the reverse rasterises again."""
    @staticmethod
    def forward(ctx, verts, logs_t, faces, zscale, obs, root_z, trunc, adjacency):
        dist, parts = ops.depth_dist(verts, faces, logs_t, zscale, obs, root_z, trunc)
        ctx.save_for_backward(verts, logs_t, faces, zscale, obs, *(() if root_z is None else (root_z,)), *adjacency)
        ctx.trunc, ctx.root = trunc, root_z is not None
        ctx.mark_non_differentiable(parts)
        return dist, parts

    @staticmethod
    def backward(ctx, g_dist, _g_parts):
        saved = ctx.saved_tensors
        verts, logs_t, faces, zscale, obs = saved[:5]
        root_z = saved[5] if ctx.root else None
        g_verts, g_logs_t = ops.depth_dist_bwd(verts, faces, logs_t, zscale, obs, root_z, ctx.trunc, g_dist.contiguous(), adjacency=tuple(saved[-2:]))
        return g_verts, g_logs_t, None, None, None, None, None, None


def depth_dist(verts, logs_t, faces, depth, hand_mask, scale, root_z=None, size=64, trunc=0.05, parts=False):
    """Depth agreement of every hypothesis' mesh with its image's depth crop: verts (N, B, V*3) or (N, B, V, 3) and logs_t (N, B, 3) =
    (log s, tx, ty) of a sample() output, faces (F, 3) (ManoLayer's `mano_layer.faces_i32`; an int64 tensor is converted once and the copy kept on it), depth
    (B, H, H) in metres, 0 where the sensor saw nothing, and hand_mask (B, H, H) (the input pipeline's target['depth'] and target['hand_mask']),
    scale (B,) metres per normalised unit (target['scale']) -> (N, B) f32, in metres; with parts=True (dist, overlap, offset, inliers).
    In the normalised image coordinates of silhouette_iou, one sample per pixel of the size x size grid (H a multiple of size):
        R(p)   the mesh rendered under p = exp(log s) v_xy + t with depth v_z scale[b]: nearest covering face, lowest face index among equals
        obs    ops.depth_obs: depth sampled at each block's centre, valid where the hand mask's box mean is >= 0.5 and the sample is finite and > 0
        off    root_z[b] (target['pose3d_root'][:, 2]) - or, with root_z=None, the mean of obs - R over the compared samples, fitted per
               hypothesis: no ground truth is needed, so this is the mode for selection at test time
        dist   (sum over the compared samples of min(|R + off - obs|, trunc) + trunc x the observed samples the mesh does not cover) / the observed
               samples: a truncated L1 over every observed hand pixel, in [0, trunc]
        overlap = compared / observed samples, offset = off, inliers = the share of the compared samples with |R + off - obs| < trunc
    An image with no observed sample gives 0 and a zero gradient, a row with a non-finite projected vertex, scale or root_z NaN and a zero
    gradient.  Differentiable with respect to verts and logs_t with coverage and face assignment held fixed (truncated and uncovered samples
    contribute nothing; with the fitted offset the weights are centred, because the offset moves with the mesh); depth, hand_mask, scale and
    root_z get no gradient, the parts are returned detached.  Runs on csrc/depth_dist.hip: one number per hypothesis leaves the kernel, no
    image tensor exists; forward and reverse are bit-reproducible; nothing is read on the host once ops.face_adjacency(faces) has been built
    (the first call with a faces tensor), so the call can be captured into a HIP graph.  HIP tensors only (MheError otherwise); ValueError for
    a bad rank or shape, H not a multiple of size, V, F or size outside 1..1024 / 1..2048 / 1..64, trunc not positive - before any launch."""
    v, lt, f, depth, hand_mask, zs, rz = _depth_operands("depth_dist", verts, logs_t, faces, depth, hand_mask, scale, root_z, size, trunc)
    if not (v.is_cuda and f.is_cuda):
        raise ops._lib.MheError("depth_dist: expected CUDA/HIP tensors (the hot path has no CPU fallback)")
    with torch.no_grad():
        obs = ops.depth_obs(depth, hand_mask, size)
        adjacency = ops.face_adjacency(f, v.shape[2])
    dist, pt = _Depth.apply(v, lt, f, zs, obs, rz, float(trunc), adjacency)
    return (dist, pt[..., 0], pt[..., 1], pt[..., 2]) if parts else dist


def depth_select(output, target, Q=1, size=64, trunc=0.05, root=False):
    """chamfer_select with depth_dist: keep, per image, the Q hypotheses of a sample() output whose mesh (output['verts'] under
    output['logs_t'], triangulated by output['faces']) agrees best with target['depth'] on target['hand_mask'] (scale from target['scale']),
    best first, ties to the lower n.  root=False fits the depth offset per hypothesis (no ground truth), root=True reads
    target['pose3d_root'][:, 2].  Every (N, B, ...) tensor of `output` is cut to (Q, B, ...); 'faces' and 'image' pass through.  Added:
    'depth_dist' (Q, B), the distances in metres, and 'depth_index' (Q, B) int64."""
    for k in ("verts", "logs_t", "faces"):
        if k not in output:
            raise ValueError(f"depth_select: output has no {k!r}")
    for k in ("depth", "hand_mask", "scale") + (("pose3d_root",) if root else ()):
        if k not in target:
            raise ValueError(f"depth_select{'(root=True)' if k == 'pose3d_root' else ''}: target has no {k!r}")
    N, B = _select_shape("depth_select", "verts", output["verts"], Q)
    root_z = None
    if root:
        pr = target["pose3d_root"]
        if not isinstance(pr, torch.Tensor) or tuple(pr.shape) != (B, 3):
            raise ValueError(f"depth_select: target['pose3d_root'] must be (B, 3) = ({B}, 3), got {tuple(getattr(pr, 'shape', ()))}")
        root_z = pr[:, 2]
    with torch.no_grad():
        dist = depth_dist(output["verts"].detach(), output["logs_t"].detach(), output["faces"], target["depth"], target["hand_mask"], target["scale"],
                          root_z=root_z, size=size, trunc=trunc)
    out = _cut(output, dist, Q, "depth_dist")
    out["depth_index"] = out.pop("depth_dist_index")
    return out


def kmeans_select(output, Q, points="xyz", iters=10, score=None):
    """Summarise a sample() output by Q distinct, weighted hypotheses per image (the n-quantised-best-of-M protocol): the N hypotheses are
    clustered by k-means on output[points] ('xyz', the joints, or 'verts', the mesh) and each cluster is kept as its member nearest the
    cluster mean, largest cluster first (ops.kmeans_select; DESIGN.md "k-means quantisation" has the algorithm and its tie rules).  score:
    an (N, B) tensor or the name of one in `output` (log q) - the first seed is the hypothesis of highest score, hypothesis 0 without it.
    Every (N, B, ...) tensor of `output` is cut to (Q, B, ...) at the representatives; 'faces' and 'image' pass through.  Added:
    'kmeans_index' (Q, B) int64, the hypotheses kept, 'kmeans_count' (Q, B) int64, the cluster sizes (their share of N is the weight of
    each answer), 'kmeans_assign' (N, B) int32, the position in the output of every hypothesis' cluster, and 'kmeans_converged' (B,) int32."""
    if points not in ("xyz", "verts"):
        raise ValueError(f"kmeans_select: points={points!r} (xyz or verts)")
    if points not in output:
        raise ValueError(f"kmeans_select: output has no {points!r}")
    src = output[points]
    N, B = _select_shape("kmeans_select", points, src, Q)
    if isinstance(score, str):
        if score not in output:
            raise ValueError(f"kmeans_select: output has no {score!r} to take the score from")
        score = output[score]
    if score is not None:
        if not isinstance(score, torch.Tensor) or score.numel() != N * B or tuple(score.shape) not in ((N, B), (N * B,)):
            raise ValueError(f"kmeans_select: score must be (N, B) = ({N}, {B}), got {tuple(getattr(score, 'shape', ()))}")
        score = score.detach().reshape(N, B).float().contiguous()
    with torch.no_grad():
        km = ops.kmeans_select(src.detach().reshape(N, B, -1).float().contiguous(), Q, score=score, iters=iters)
    keep, cols = km["index"], torch.arange(B, device=km["index"].device)
    out = {}
    for k, v in output.items():
        cut = isinstance(v, torch.Tensor) and k not in ("faces", "image") and v.dim() >= 2 and tuple(v.shape[:2]) == (N, B)
        out[k] = v[keep, cols] if cut else v
    out["kmeans_index"], out["kmeans_count"] = keep, km["count"].long()
    out["kmeans_assign"], out["kmeans_converged"] = km["assign"], km["converged"]
    return out


def silhouette_iou(verts, logs_t, faces, hand_mask, size=64):
    """Intersection over union of every hypothesis' silhouette with its image's hand mask: verts (N, B, V*3) or (N, B, V, 3) and logs_t
    (N, B, 3) = (log s, tx, ty) of a sample() output, faces (F, 3) int32 (ManoLayer's `mano_layer.faces_i32`; an int64 tensor is converted on
    every call), hand_mask (B, H, H) bool or float in [0, 1] (the input pipeline's target['hand_mask']) -> (N, B) f32.  H must be a
    multiple of `size`; the mask is box-averaged down to (size, size) when it is larger.  The silhouette is ops.render_mesh's anti-aliased mask
    under the camera p = exp(log s) v_xy + t; IoU = sum min(mask, target) / sum max(mask, target), 0 where the union is empty.  The fused
    path: only the two sums per hypothesis leave the kernel, no mask tensor exists.  Forward only (no gradient).
        iou = silhouette_iou(out['verts'], out['logs_t'], faces, target['hand_mask'])
        best = iou.max(0).values          # (B,) best of N
        keep = iou.argmax(0)              # (B,) a selection index, used like chamfer_select's: out['xyz'][keep, torch.arange(B)]"""
    if not isinstance(verts, torch.Tensor) or verts.dim() not in (3, 4) or (verts.dim() == 4 and verts.shape[-1] != 3) or verts[0, 0].numel() % 3:
        raise ValueError(f"silhouette_iou: verts must be (N, B, V*3) or (N, B, V, 3), got {tuple(getattr(verts, 'shape', ()))}")
    N, B = verts.shape[:2]
    if tuple(logs_t.shape) != (N, B, 3):
        raise ValueError(f"silhouette_iou: logs_t must be (N, B, 3) = ({N}, {B}, 3), got {tuple(logs_t.shape)}")
    if hand_mask.dim() != 3 or hand_mask.shape[0] != B or hand_mask.shape[1] != hand_mask.shape[2]:
        raise ValueError(f"silhouette_iou: hand_mask must be (B, H, H) with B={B}, got {tuple(hand_mask.shape)}")
    H = hand_mask.shape[1]
    if H < size or H % size:
        raise ValueError(f"silhouette_iou: hand_mask is {H} x {H}, not a multiple of size={size}")
    with torch.no_grad():
        tgt = hand_mask.float()
        if H != size:
            k = H // size
            tgt = tgt.view(B, size, k, size, k).mean((2, 4))
        lt = logs_t.detach().reshape(N * B, 3).float()
        if faces.dtype != torch.int32:
            faces = faces.to(torch.int32)
        sums = ops.render_mesh(verts.detach().reshape(N * B, -1, 3).float().contiguous(), faces.contiguous(), lt[:, 0].exp().contiguous(),
                               lt[:, 1:].contiguous(), size=size, anti_aliasing=True, want=("iou_sums",), target=tgt.contiguous())["iou_sums"]
        inter, union = sums[:, 0], sums[:, 1]
        return torch.where(union > 0, inter / union.clamp_min(1e-30), torch.zeros_like(inter)).view(N, B)


class MHEntLoss(nn.Module):
    def __init__(self, loss_weights=None, aligned=False):
        """aligned: the reference's evaluation branch (criteria.py:62-87) - every hypothesis' joints and mesh are Procrustes-aligned
        with scale to target['pose3d'] / target['verts'] (a label whose target is absent is left as it is); output['xyz'] and
        output['verts'] are replaced by new aligned tensors.  The 3D error rows are taken of the aligned joints, the 3D spread rows
        of the unaligned ones (criteria.py:63-68,141), the 2D rows are unchanged.
        chamfer_select (an attribute, False here; MHEntChamferLoss below is this criterion with it set): the reference's switch of that name
        (criteria.py:87-89), which computes the distance and drops it.  Here, when output has 'xyz', metrics gain the Chamfer distance of the
        unaligned joints to target['object_verts']: chamfer_rgb_sample (B,), the least over the N hypotheses in mm, chamfer_rgb_sample_mean
        (B,), their mean, and chamfer_rgb_select (B,) int64, the n that attains the least (the lowest on a tie).  ValueError when target
        has no 'object_verts'.  The constructor keeps the two parameters of the aligned evaluation, which tests/test_aligned_oracle.py pins."""
        super().__init__()
        self.loss_weights = loss_weights
        self.aligned = aligned
        self.chamfer_select = False

    def forward(self, output, target):
        if self.chamfer_select and "object_verts" not in target:
            raise ValueError("MHEntLoss with chamfer_select: target has no 'object_verts'")
        losses = {"neg_log_p": -output["log_p"]}          # criteria.py:55
        metrics = {}
        unaligned_xyz = output.get("xyz")
        if self.aligned:
            for lbl in ("xyz", "verts"):
                tgt = target["pose3d"] if lbl == "xyz" else target.get("verts")
                if lbl in output and tgt is not None:
                    output[lbl] = ops.procrustes_align(output[lbl].contiguous(), tgt.contiguous())
        if "xyz" in output:
            if "uv" not in output:
                raise NotImplementedError("uv from ground-truth s,t (criteria.py:100-104) is not on the MHEnt path")
            rest = (output["uv"].contiguous(), target["pose3d"].contiguous(), target["scale"].contiguous(), target["crop_uv"].contiguous(),
                    target["vis"].contiguous())
            if output["xyz"] is unaligned_xyz:
                m = ops.metrics(output["xyz"].contiguous(), *rest)
            else:
                m = ops.metrics_split(output["xyz"], unaligned_xyz.contiguous(), *rest)
            metrics = {k: m[i] for i, k in enumerate(METRIC_KEYS)}
            if self.chamfer_select:
                N, B = unaligned_xyz.shape[:2]
                with torch.no_grad():
                    dist = chamfer_dist(unaligned_xyz.detach().reshape(N, B, -1, 3), target)
                    val, order = _rank(dist)
                metrics["chamfer_rgb_sample"], metrics["chamfer_rgb_select"] = val[0], order[0]
                metrics["chamfer_rgb_sample_mean"] = dist.mean(0)
        return sum(v.mean() for v in losses.values()), losses, metrics


class MHEntChamferLoss(MHEntLoss):
    """MHEntLoss with chamfer_select on: the 14 metrics unchanged plus chamfer_rgb_sample, chamfer_rgb_sample_mean and chamfer_rgb_select"""
    def __init__(self, loss_weights=None, aligned=False):
        super().__init__(loss_weights, aligned)
        self.chamfer_select = True
