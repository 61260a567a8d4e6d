"""Float64 reference of the MANO loss pass and its reverse (csrc/mano.hip, csrc/mano_joint_pass.h, csrc/mano_bwd.hip): every output the C
entries mhe_mano_joints_f32 / _mods_f32 / _chamfer_f32 can write, and by autograd what the three reverse entries write.  A helper module, not
a test.  It wraps the committed CPU restatements oracle/mano_ref.py and oracle/network_ref.py (pinned by the reference's own vectors,
tests/test_mano_pass_ref_host.py) and, for the hand-object Chamfer term, the distances of tests/chamfer_ref.py on the reference's own joints.

Called with dtype=torch.float32 the same code is the yardstick of the bounds: a tensor's bound is
max(3 max|f32 call - f64 call|, 2e-6 max|f64 call|) over that tensor and case (bound() below; the rule of
test_generic_lbs_at_smpl_size_matches_oracle), z - a pure copy - has bound 0.

Rows: row r belongs to image img[r] (default r % B, the kernels' layout); the pass is row-independent, so a test may pass any subset of the
rows with their img.  d loss / d log_p[r] = g_log_p[img[r]] * row_w, as the reverse kernels define it."""
import functools
import math

import numpy as np
import torch

import chamfer_ref
from mhentropy_amd import synth
from oracle import mano_ref, network_ref

MODS_UV, MODS_XYZ = 1, 2
FLOOR = 2e-6          # of the tensor's largest magnitude in the reference
CH_GAP = 1e-4         # least relative distance of a Chamfer minimum's runner-up in the cases whose reverse is compared (see chamfer_rows)


@functools.lru_cache(None)
def tables(dtype=torch.float64, zero_mean=False):
    """synth.mano_tables(0) under the reference's buffer names; zero_mean: hands_mean = 0 (th45 = 0 then gives 15 axis-angles of exactly 0)"""
    t = dict(synth.mano_tables(0))
    if zero_mean:
        t["hands_mean"] = np.zeros_like(t["hands_mean"])
    return mano_ref.tables_from_numpy(t, dtype=dtype)


def packed_tables(zero_mean=False):
    """the same tables as the kernels' blob (numpy float32)"""
    from mhentropy_amd import mano_pack
    t = synth.mano_tables(0)
    mean = np.zeros_like(t["hands_mean"]) if zero_mean else t["hands_mean"]
    return mano_pack.pack_tables(t["shapedirs"], t["posedirs"], t["v_template"], t["J_regressor"], t["weights"], t["hands_components"][:45], mean)


def clamp_count(count, VO):
    """the kernels' documented clamp of obj_count: min(max(count, 1), VO); None means VO"""
    return None if count is None else np.clip(np.asarray(count, np.int64), 1, VO)


def chamfer_rows(xyz, img, scale, root, obj, count):
    """xyz (R,21,3) torch -> (dist (R,) torch (differentiable, argmins fixed at the lowest index of a tie, 0 sub-gradient at a zero distance),
    gap: the least relative difference between a minimum and its nearest strictly larger candidate over all rows - an exact tie is decided by
    the index, anything closer than an f32 evaluation resolves is not)"""
    dt = xyz.dtype
    s, r, o = (torch.as_tensor(np.asarray(a)).to(dt) for a in (scale, root, obj))
    VO = o.shape[1]
    cnt = clamp_count(count, VO)
    dist = [None] * xyz.shape[0]
    gap = np.inf
    for b in sorted(set(int(i) for i in img)):
        rows = [i for i in range(xyz.shape[0]) if int(img[i]) == b]
        Vb = VO if cnt is None else int(cnt[b])
        d = chamfer_ref._pair_dist(xyz[rows][:, None], s[b:b + 1], r[b:b + 1], o[b:b + 1], 0, Vb)          # (rows, 21, Vb)
        dn = d.detach().double().numpy()
        for axis in (2, 1):
            best = dn.min(axis, keepdims=True)
            second = np.where(dn > best, dn, np.inf).min(axis, keepdims=True)
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.where(np.isfinite(second), (second - best) / np.maximum(second, 1e-300), np.inf)
            gap = min(gap, float(rel.min()))
        ip = torch.as_tensor(dn.argmin(2))[:, :, None]          # first occurrence: the lowest index on a tie
        io = torch.as_tensor(dn.argmin(1))[:, None, :]
        both = d.gather(2, ip).mean((1, 2)) + d.gather(1, io).mean((1, 2))
        for k, i in enumerate(rows):
            dist[i] = both[k]
    return torch.stack(dist), gap


def mano_pass(th45, det, crop_uv=None, vis=None, pose3d=None, mods=MODS_UV, laplace_b=0.03, laplace_b_3d=0.03, th45_alpha=50.0,
              inv_norm=False, image_size=256.0, dtype=torch.float64, zero_mean=False, img=None, chamfer=None, chamfer_w=0.0, grad=False,
              g_log_p=None, row_w=1.0):
    """th45 [R,45], det [B,16] = [th3 bt logs t], crop_uv [B,42], vis [B,21], pose3d [B,63] (float32 values, evaluated in `dtype`) -> dict of
    float64 numpy arrays: z [R,61], xyz [R,63], uv [R,42] (as inv_norm says) and uv_inv [R,42] (inv_norm=True at image_size), terms5 [R,5] =
    (uv, xyz, th3, th45, bt; 0 for a likelihood that is off), terms4 [R,4] (mods = uv only), log_p [R], norms [R,2], joints_mm [R,63];
    chamfer = (scale [B], root [B,3], obj [B,VO,3], count [B] | None) adds dist [R] and gap.
    grad=True: g_th45 [R,45] and the per-row g_det [R,16] of sum_r g_log_p[img[r]] row_w (log_p[r] - chamfer_w dist[r])."""
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    th45, det, crop_uv, vis, pose3d = t(th45), t(det), t(crop_uv), t(vis), t(pose3d)
    R, B = th45.shape[0], det.shape[0]
    img = np.arange(R) % B if img is None else np.asarray(img)
    det_rows = det[img]
    if grad:
        assert not inv_norm, "the reverse kernels differentiate the inv_norm=False pass"
        th45, det_rows = th45.clone().requires_grad_(True), det_rows.clone().requires_grad_(True)
    tb = tables(dtype, zero_mean)
    with torch.enable_grad() if grad else torch.no_grad():
        z = network_ref.combine_z(det_rows, th45)
        joints = mano_ref.wrapper_forward(tb, z[:, :48], z[:, 48:58])["mano_joints"]                     # (R,21,3) mm, RHD order
        xyz, _, _ = mano_ref.normalize_pose3d(joints, network_ref.ROOT_IDX, network_ref.NORM_IDX)
        s_cam, t_cam = torch.exp(z[:, 58:59]), z[:, 59:61]
        uv_raw = mano_ref.orth_proj(xyz, s_cam, t_cam, image_size, False).flatten(-2)
        uv_inv = mano_ref.orth_proj(xyz, s_cam, t_cam, image_size, True).flatten(-2)
        uv = uv_inv if inv_norm else uv_raw
        zero = torch.zeros(R, dtype=dtype)
        lp_uv = lp_xyz = zero
        if (mods & MODS_UV) and crop_uv is not None:
            lp_uv = network_ref.laplace_log_prob(crop_uv[img], uv, vis[img][..., None].repeat(1, 1, 2).flatten(-2), b=laplace_b)
        if (mods & MODS_XYZ) and pose3d is not None:
            lp_xyz = network_ref.laplace_log_prob(pose3d[img], xyz.flatten(-2), vis[img][..., None].repeat(1, 1, 3).flatten(-2), b=laplace_b_3d)
        lp_3 = network_ref.approx_uniform_ball(z[:, :3], math.pi, 5.0)
        lp_45 = network_ref.approx_uniform_rec(z[:, 3:48], -2.0, 2.0, th45_alpha)
        lp_bt = network_ref.approx_uniform_rec(z[:, 48:58], -0.03, 0.03, 50.0)
        log_p = lp_uv + lp_xyz + lp_3 + lp_45 + lp_bt
        out = {"z": z, "xyz": xyz.flatten(-2), "uv": uv, "uv_inv": uv_inv, "terms5": torch.stack([lp_uv, lp_xyz, lp_3, lp_45, lp_bt], 1),
               "log_p": log_p, "norms": torch.stack([z[:, :48].norm(p=2, dim=1), z[:, 48:58].norm(p=2, dim=1)], 1), "joints_mm": joints.flatten(-2)}
        if mods == MODS_UV:
            out["terms4"] = out["terms5"][:, [0, 2, 3, 4]]
        gap = None
        if chamfer is not None:
            out["dist"], gap = chamfer_rows(xyz, img, *chamfer)
        if grad:
            g = torch.as_tensor(np.asarray(g_log_p)).to(dtype)[img] * row_w
            total = (g * (log_p - chamfer_w * out["dist"] if chamfer is not None else log_p)).sum()
            out["g_th45"], out["g_det"] = torch.autograd.grad(total, (th45, det_rows))
    res = {k: v.detach().double().numpy() for k, v in out.items()}
    if gap is not None:
        res["gap"] = gap
    return res


def bound(ref64, ref32, key):
    """max(3 max|f32 call - f64 call|, FLOOR max|f64 call|) of one tensor of one case; 0 for z"""
    if key == "z":
        return 0.0
    a, b = np.asarray(ref64[key], np.float64), np.asarray(ref32[key], np.float64)
    return max(3.0 * float(np.abs(a - b).max()), FLOOR * float(np.abs(a).max()))
