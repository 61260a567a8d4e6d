"""Float64 reference of the body-model kernels (csrc/body.hip, csrc/lbs_skin.hip, csrc/lbs_skin_bwd.hip, the skinning half of csrc/body_kp.hip)
at every size class of their launchers.  A helper module, not a test: a table builder for any 1 <= J <= 32, the kernel-side layouts of
BodyLayer.__init__ at a free pitch VP and padding fill, the size formulas of the launchers restated, the references and the case table of
tests/test_gpu_body_edges.py (checked on the CPU by tests/test_body_edge_ref_host.py).

References: vertices and posed joints are oracle.body_ref.lbs (pinned at the MANO sizes, tests/test_oracle_golden.py) in float64; the same call
in float32 is the yardstick of the bounds: per tensor and case max(3 max|f32 call - f64 call|, 2e-6 max|f64 call|) (bound() below; the rule of
test_generic_lbs_at_smpl_size_matches_oracle).  The workspace row of the pose kernel and the skinning reverse's intermediates need the two halves
of that function apart: pose_parts (rotations, betas -> pose map, transforms [J][12], posed joints) and skin_parts (pose map, betas, transforms
-> vertices) restate them; the host test pins skin_parts(pose_parts(.)) to body_ref.lbs.  Reverse quantities are float64 autograd: the totals
(g_rotmats, g_betas) through body_ref.lbs itself, the intermediates (g_transforms, g_posemap, the blend-shape g_betas) through skin_parts.

dyadic=True gives an exact-arithmetic model: template, blend shapes small multiples of 2^-4, one-hot skinning weights and regressor rows; with
integer betas, signed permutation matrices as rotations and a power-of-two scale every product and every partial sum of the forward pass is a
multiple of 2^-4 below 2^15, representable in f32 (and, piece by piece, in the bf16 splits of the matrix-core kernels): the f32 and f64
references are bit-identical and a kernel that is not has taken a wrong operand, not a rounding."""
import functools

import numpy as np
import torch

from mhentropy_amd.body import SMPL_PARENTS
from oracle import body_ref

FLOOR = 2e-6
SENT, SPARE = -7.0, 40

# ---- the case table ------------------------------------------------------------------------------------------------------------------------------
MODELS = [(1, 7), (2, 1), (2, 6), (3, 12), (3, 13), (3, 14), (3, 15), (4, 10), (8, 10), (12, 10), (16, 10), (20, 10), (24, 10), (28, 10),
          (28, 13), (32, 1), (32, 33), (32, 64), (17, 10)]          # (J, nb)
VERTS = [(1, 32), (31, 32), (32, 32), (33, 64), (96, 96), (127, 128), (129, 160), (129, 224), (203, 256)]          # (NV, VP)
ROWS = [1, 31, 32, 33, 65]
SCALES = [1.0, -2.5, 1000.0]
NKS = [1, 31, 32, 33, 64]
R_BIG = 2048 * 4 + 7          # the pose kernels cap the grid at 2048 workgroups of 4 rows: rows 8192 .. 8198 run on the second loop trip
ROWS_BIG = np.concatenate([np.arange(16), np.arange(R_BIG - 23, R_BIG)])
BIG_MODELS = [(2, 1), (24, 10)]


def _cases():
    """every model class at two vertex classes; the vertex classes cycle separately over the JS = 1 and the JS = 2 models so that each of them meets
    both; rows, scales and keypoint counts cycle over the cases (periods 5, 3, 5 against 38 cases: every value is met several times)"""
    out, nxt = [], {1: 0, 2: 0}
    for J, nb in MODELS:
        for _ in range(2):
            g = js(J)
            NV, VP = VERTS[nxt[g] % len(VERTS)]
            nxt[g] += 1
            k = len(out)
            out.append(dict(name="J%d_nb%d_NV%d_VP%d" % (J, nb, NV, VP), seed=100 + k, J=J, nb=nb, NV=NV, VP=VP, R=ROWS[k % 5],
                            scale=SCALES[k % 3], NK=NKS[(k // 2 + k) % 5]))
    return out


# the error variant's image classes, on one JS = 1 and one JS = 2 model: (J, nb, NV, VP, R, B): rows per image 32; 16 and 48 at R = 96 (a
# workgroup of 32 rows, and of 8, straddles images)
ERR_CASES = [dict(name="err_J%d_R%d_B%d" % (J, R, B), seed=300 + i, J=J, nb=nb, NV=NV, VP=VP, R=R, B=B, scale=s, NK=0)
             for i, (J, nb, NV, VP, R, B, s) in enumerate([(8, 10, 129, 160, 64, 2, 1.0), (8, 10, 33, 64, 96, 6, -2.5), (8, 10, 127, 128, 96, 2, 1000.0),
                                                           (24, 10, 129, 224, 64, 2, -2.5), (24, 10, 31, 32, 96, 6, 1000.0), (24, 10, 203, 256, 96, 2, 1.0)])]


# ---- the launchers' size formulas, restated ----------------------------------------------------------------------------------------------------------
def ws_stride(J, nb):
    return (9 * (J - 1) + nb + 15 * J + 15) // 16 * 16


def ks(J, nb):
    """k-steps of 16 of the matrix-core forward, rounded up to even: K = 9 (J - 1) + nb + 2"""
    return ((9 * (J - 1) + nb + 2 + 15) // 16 + 1) // 2 * 2


def js(J):
    return (J + 15) // 16


def nt(J, nb):
    """32-column coefficient tiles of the skinning reverse: the launch_coef<NT> instantiation"""
    return (9 * (J - 1) + nb + 31) // 32


def split_floats(J, nb, VP):
    VT = VP // 32
    return ((VT * ks(J, nb) * 6 * 512 + VT * js(J) * 3 * 512) * 2 + 3) // 4


def kp_split_floats(NK, VP):
    return ((VP // 32) * 2 * ((NK + 31) // 32) * 3 * 512 * 2 + 3) // 4


def bwd_tables_floats(J, nb, VP):
    return VP * 3 * 32 * nt(J, nb) + VP * 32


def skin_lds(J, nb):
    return ks(J, nb) * 2048 + 12 * js(J) * 3072 + 4 * 4096


def kp_lds(J, nb, NK):
    """bytes of LDS of the matrix-core keypoint kernel: the skinning's pieces and store tiles + four staging tiles of 3 x 32 x 40 bf16, or the four
    waves' partial sums, whichever is larger; (32, 64) gives 22 * 2048 + 12 * 2 * 3072 + 16384 + 30720 = 165,888 > 160 KiB: not supported"""
    return max(skin_lds(J, nb) + 4 * 3 * 32 * 40 * 2, 4 * 3 * ((NK + 31) // 32) * 32 * 33 * 4)


LDS_LIMIT = 160 * 1024


# ---- tables and inputs ---------------------------------------------------------------------------------------------------------------------------
def parents(J):
    """SMPL's tree for the first 24 joints, a chain behind it"""
    return np.asarray([SMPL_PARENTS[j] if j < 24 else j - 1 for j in range(J)], np.int32)


@functools.lru_cache(None)
def tables(seed, NV, J, nb, NK=0, dyadic=False):
    """SMPL-named float32 tables for any 1 <= J <= 32 and NV >= 1 (+ 'keypoint_regressor' (NK, NV)): the value ranges of synthetic_body_tables with
    min(J, 4) joints per vertex; keypoint row 0 and every fourth row from row 2 are one-hot, row 0 on the last vertex.  dyadic: see the module"""
    rng = np.random.default_rng(seed + 9100)
    NP = 9 * (J - 1)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    if dyadic:
        w = np.zeros((NV, J))
        jv = rng.integers(0, J, NV)
        jv[:min(NV, J)] = rng.permutation(J)[:min(NV, J)]
        w[np.arange(NV), jv] = 1.0
        jr = np.zeros((J, NV))
        jr[np.arange(J), rng.integers(0, NV, J)] = 1.0
        t = {"v_template": f32(rng.integers(-8, 9, (NV, 3)) / 16.0), "shapedirs": f32(rng.integers(-4, 5, (NV, 3, nb)) / 16.0),
             "posedirs": f32(rng.integers(-4, 5, (NV, 3, NP)) / 16.0)}
    else:
        w = np.zeros((NV, J))
        for v in range(NV):
            sel = rng.choice(J, min(J, 4), replace=False)
            w[v, sel] = rng.random(len(sel)) + 0.05
        w /= w.sum(1, keepdims=True)
        jr = rng.random((J, NV)) * (rng.random((J, NV)) < min(1.0, 8.0 / NV))
        jr[:, 0] += 1e-3
        jr /= jr.sum(1, keepdims=True)
        t = {"v_template": f32(rng.normal(0, 0.3, (NV, 3))), "shapedirs": f32(rng.normal(0, 0.01, (NV, 3, nb))),
             "posedirs": f32(rng.normal(0, 0.002, (NV, 3, NP)))}
    t.update({"J_regressor": f32(jr), "weights": f32(w), "parents": parents(J)})
    if NK:
        kr = rng.random((NK, NV)) * (rng.random((NK, NV)) < min(1.0, 8.0 / NV))
        kr[:, 0] += 1e-3
        kr /= kr.sum(1, keepdims=True)
        for k in range(NK):
            if dyadic or k == 0 or k % 4 == 2:
                kr[k] = 0.0
                kr[k, NV - 1 if k == 0 else rng.integers(NV)] = 1.0
        t["keypoint_regressor"] = f32(kr)
    for a in t.values():
        a.setflags(write=False)
    return t


@functools.lru_cache(None)
def inputs(seed, R, J, nb, dyadic=False):
    """rotmats (R, J, 3, 3), betas (R, nb) float32: random rotations (Gram-Schmidt of normal draws, in float64) and N(0, 1) betas; dyadic: signed
    permutation matrices and integers in -2..2"""
    rng = np.random.default_rng(seed + 9200)
    if dyadic:
        rot = np.zeros((R, J, 3, 3))
        for r in range(R):
            for j in range(J):
                rot[r, j, np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
        betas = rng.integers(-2, 3, (R, nb)).astype(np.float64)
    else:
        a, b = rng.normal(0, 1, (R, J, 3)), rng.normal(0, 1, (R, J, 3))
        x = a / np.linalg.norm(a, axis=-1, keepdims=True)
        z = np.cross(x, b)
        z /= np.linalg.norm(z, axis=-1, keepdims=True)
        rot = np.stack([x, np.cross(z, x), z], -1)
        betas = rng.normal(0, 1, (R, nb))
    rot, betas = np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(betas, np.float32)
    rot.setflags(write=False); betas.setflags(write=False)
    return rot, betas


def layouts(t, VP, fill=0.0):
    """the kernel-side layouts of BodyLayer.__init__ (float32 numpy): jt [J,3] and jsd [J,3,nb] through float64, the vertex-fastest tables vt
    [3][VP], vsd [nb][3][VP], vpd [9(J-1)][3][VP], vw [J][VP] at pitch VP (any multiple of 32 >= NV) with the columns NV..VP-1 set to `fill`"""
    NV = t["v_template"].shape[0]
    assert VP % 32 == 0 and VP >= NV
    vp = lambda a: np.ascontiguousarray(np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, VP - NV)], constant_values=fill), np.float32)
    jr = t["J_regressor"].astype(np.float64)
    return {"jt": np.ascontiguousarray(jr @ t["v_template"].astype(np.float64), np.float32),
            "jsd": np.ascontiguousarray(np.einsum("jv,vck->jck", jr, t["shapedirs"].astype(np.float64)), np.float32),
            "vt": vp(t["v_template"].T), "vsd": vp(t["shapedirs"].transpose(2, 1, 0)), "vpd": vp(t["posedirs"].transpose(2, 1, 0)),
            "vw": vp(t["weights"].T), "parents": np.ascontiguousarray(t["parents"], np.int32)}


def bwd_tables(t, VP):
    """what mhe_lbs_bwd_tables_f32 writes (a re-arrangement: exact): PDT [VP][3][32 NT] (pose map | betas | 0), then WT [VP][32]; zero past NV"""
    NV, J = t["weights"].shape
    nb, NP = t["shapedirs"].shape[2], 9 * (J - 1)
    pdt = np.zeros((VP, 3, 32 * nt(J, nb)), np.float32)
    pdt[:NV, :, :NP] = t["posedirs"]
    pdt[:NV, :, NP:NP + nb] = t["shapedirs"]
    wt = np.zeros((VP, 32), np.float32)
    wt[:NV, :J] = t["weights"]
    return np.concatenate([pdt.reshape(-1), wt.reshape(-1)])


# ---- references ----------------------------------------------------------------------------------------------------------------------------------
def tb_torch(t, dtype):
    return {k: (torch.as_tensor(np.array(v)).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(np.array(v))) for k, v in t.items()}


def pose_parts(tb, rot, betas):
    """the pose half of body_ref.lbs: -> pose map (R, 9(J-1)), transforms (R, J, 12) = [Rw_j row-major | t_j - Rw_j J_j], posed joints (R, J, 3)"""
    R, J = rot.shape[:2]
    par = [int(p) for p in tb["parents"]]
    pm = (rot[:, 1:] - torch.eye(3, dtype=rot.dtype)).reshape(R, 9 * (J - 1))
    v_shaped = torch.matmul(tb["shapedirs"], betas.t()).permute(2, 0, 1) + tb["v_template"]
    jr = torch.matmul(tb["J_regressor"], v_shaped)
    Rw, tj = [rot[:, 0]], [jr[:, 0]]
    for j in range(1, J):
        p = par[j]
        Rw.append(torch.matmul(Rw[p], rot[:, j]))
        tj.append(torch.matmul(Rw[p], (jr[:, j] - jr[:, p]).unsqueeze(2)).squeeze(2) + tj[p])
    Rw, tj = torch.stack(Rw, 1), torch.stack(tj, 1)
    a = tj - torch.matmul(Rw, jr.unsqueeze(3)).squeeze(3)
    return pm, torch.cat([Rw.reshape(R, J, 9), a], 2), tj


def skin_parts(tb, pm, betas, A):
    """the skinning half: pose map, betas, transforms -> vertices (R, NV, 3), unscaled"""
    R, J = A.shape[:2]
    x = tb["v_template"] + torch.matmul(tb["shapedirs"], betas.t()).permute(2, 0, 1) + torch.matmul(tb["posedirs"], pm.t()).permute(2, 0, 1)
    T = torch.einsum("vj,rje->rve", tb["weights"], A)
    return (T[..., :9].reshape(R, -1, 3, 3) * x.unsqueeze(2)).sum(3) + T[..., 9:]


def err_rows(verts, target, center, scale, rpi):
    """_err64 of tests/test_gpu_body_eval.py in the dtype of `verts`: mean over v of || scale vert[r, v] - center[r] - target[r // rpi, v] ||"""
    d = scale * verts - target.repeat_interleave(rpi, 0)
    if center is not None:
        d = d - center[:, None, :]
    return (d * d).sum(-1).sqrt().mean(-1)


def forward(t, rot, betas, scale=1.0, dtype=torch.float64, target=None, center=None, rpi=1):
    """-> dict of float64 numpy: verts (scaled), joints, pm, A, ws (the defined part of the workspace row: pm | betas | A | joints), kp (with a
    'keypoint_regressor'), err (with a target (B, NV, 3))"""
    tb = tb_torch(t, dtype)
    rt, bt = torch.as_tensor(np.array(rot)).to(dtype), torch.as_tensor(np.array(betas)).to(dtype)
    with torch.no_grad():
        verts, joints = body_ref.lbs(tb, rt, bt)
        pm, A, _ = pose_parts(tb, rt, bt)
        out = {"verts": verts * scale, "joints": joints, "pm": pm, "A": A, "ws": torch.cat([pm, bt, A.flatten(1), joints.flatten(1)], 1)}
        if "keypoint_regressor" in tb:
            out["kp"] = torch.matmul(tb["keypoint_regressor"], verts * scale)
        if target is not None:
            cn = None if center is None else torch.as_tensor(np.array(center)).to(dtype)
            out["err"] = err_rows(verts, torch.as_tensor(np.array(target)).to(dtype), cn, scale, rpi)
    return {k: np.ascontiguousarray(v.double().numpy()) for k, v in out.items()}


def reverse(t, rot, betas, scale=1.0, g_verts=None, g_joints=None, g_kp=None, dtype=torch.float64):
    """autograd of sum(g_verts . scale verts) + sum(g_joints . joints) + sum(g_kp . regressor scale verts): the totals g_rot (R,J,3,3), g_betas (R,nb)
    through body_ref.lbs; and through skin_parts at fixed transforms what mhe_lbs_skin_bwd_f32 writes: g_tf (R,J,12), g_pm, g_bt; gv = the vertex
    gradient after mhe_lbs_keypoints_bwd_f32 (g_verts + regressor^T g_kp)"""
    tb = tb_torch(t, dtype)
    cv = lambda a: None if a is None else torch.as_tensor(np.array(a)).to(dtype)
    rt, bt = cv(rot).requires_grad_(True), cv(betas).requires_grad_(True)
    gv, gj, gk = cv(g_verts), cv(g_joints), cv(g_kp)
    if gk is not None:
        back = torch.einsum("kv,rkc->rvc", tb["keypoint_regressor"], gk)
        gv = back if gv is None else gv + back
    verts, joints = body_ref.lbs(tb, rt, bt)
    total = verts.sum() * 0
    if gv is not None:
        total = total + (gv * verts).sum() * scale
    if gj is not None:
        total = total + (gj * joints).sum()
    out = dict(zip(("g_rot", "g_betas"), torch.autograd.grad(total, (rt, bt))))
    if gv is not None:
        out["gv"] = gv
        pm, A, _ = pose_parts(tb, rt.detach(), bt.detach())
        pm, A, b2 = pm.requires_grad_(True), A.requires_grad_(True), bt.detach().clone().requires_grad_(True)
        g = torch.autograd.grad((gv * skin_parts(tb, pm, b2, A)).sum() * scale, (A, pm, b2), allow_unused=True)
        out.update({"g_tf": g[0], "g_pm": g[1] if g[1] is not None else torch.zeros_like(pm), "g_bt": g[2]})
    return {k: np.ascontiguousarray(v.detach().double().numpy()) for k, v in out.items()}


def keypoints_reverse(t, g_kp, g_verts=None, dtype=torch.float64):
    """what mhe_lbs_keypoints_bwd_f32 leaves in g_verts: regressor^T g_kp, added to g_verts when it accumulates"""
    kr = torch.as_tensor(np.array(t["keypoint_regressor"])).to(dtype)
    back = torch.einsum("kv,rkc->rvc", kr, torch.as_tensor(np.array(g_kp)).to(dtype))
    if g_verts is not None:
        back = torch.as_tensor(np.array(g_verts)).to(dtype) + back
    return back.double().numpy()


def transforms_reverse(t, rot, betas, g_tf, g_pm, g_joints=None, g_betas_in=None, dtype=torch.float64):
    """what mhe_lbs_transforms_bwd_f32 writes: autograd of sum(g_tf . A) + sum(g_pm . pm) + sum(g_joints . joints) + sum(g_betas_in . betas) through
    pose_parts -> g_rot, g_betas"""
    tb = tb_torch(t, dtype)
    cv = lambda a: None if a is None else torch.as_tensor(np.array(a)).to(dtype)
    rt, bt = cv(rot).requires_grad_(True), cv(betas).requires_grad_(True)
    pm, A, joints = pose_parts(tb, rt, bt)
    total = (cv(g_tf) * A).sum() + (cv(g_pm) * pm).sum()
    if g_joints is not None:
        total = total + (cv(g_joints) * joints).sum()
    if g_betas_in is not None:
        total = total + (cv(g_betas_in) * bt).sum()
    g = torch.autograd.grad(total, (rt, bt))
    return {"g_rot": g[0].double().numpy(), "g_betas": g[1].double().numpy()}


def bound(ref64, ref32):
    """max(3 max|f32 call - f64 call|, FLOOR max|f64 call|) of one tensor of one case"""
    a, b = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    return max(3.0 * float(np.abs(a - b).max()), FLOOR * float(np.abs(a).max())) if a.size else 0.0


CASES = _cases()
