"""Body-model decoder of a ProHMR-style multi-hypothesis head (reference README.md:26-42):
K samples of a 144-D pose (24 joints x 6D rotation) per image -> rotation matrices (reference hand/manopth/rot6d.py:4-24)
-> linear-blend skinning of a 24-joint / 6,890-vertex body (the arithmetic of hand/manopth/manolayer.py:181-246 at SMPL's
sizes), on the HIP kernels of csrc/body.hip.

PARITY: `rot6d` is in the reference tree and pinned by fixtures generated from it (tests/golden/rot6d.npz).  The skinning
arithmetic is pinned at the MANO sizes through oracle/body_ref.py == oracle/mano_ref.py (itself pinned by reference
fixtures).  ProHMR's SMPLFlow / SMPL classes and the SMPL model file are out of tree (README.md:30; licence): at body size
the tables are synthetic and parity with ProHMR itself is UNPINNED.

Hypotheses are independent given the conditioning feature, so `forward` takes any slice of the K hypotheses: the
hypothesis-sharded form is `dist.HypothesisShards` around this layer."""
import ctypes as C

import os

import numpy as np
import torch
from torch import nn

from . import ops, _lib

# SMPL's kinematic tree (24 joints; published with the model, Loper et al. 2015)
SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


def synthetic_body_tables(seed=0, NV=6890, J=24, nb=10, parents=SMPL_PARENTS, keypoints=0):
    """SMPL-SHAPED random tables (the real model is licence-restricted): template ~ N(0, 0.3), small blend shapes,
    positive row-normalised skinning weights concentrated on 4 joints per vertex, a joint regressor with rows summing to 1.
    keypoints=NK adds "keypoint_regressor" (NK, NV): sparse positive rows summing to 1 and, from the third row on, every fourth row one-hot (a
    picked vertex); drawn after the other tables, which do not depend on it."""
    rng = np.random.default_rng(seed + 9000)
    f32 = lambda a: np.asarray(a, np.float32)
    w = np.zeros((NV, J))
    for v in range(NV):
        js = rng.choice(J, 4, replace=False)
        w[v, js] = rng.random(4) + 0.05
    w /= w.sum(1, keepdims=True)
    jr = rng.random((J, NV)) * (rng.random((J, NV)) < 0.01)
    jr[:, 0] += 1e-3
    jr /= jr.sum(1, keepdims=True)
    t = {"v_template": f32(rng.normal(0, 0.3, (NV, 3))), "shapedirs": f32(rng.normal(0, 0.01, (NV, 3, nb))),
         "posedirs": f32(rng.normal(0, 0.002, (NV, 3, 9 * (J - 1)))), "J_regressor": f32(jr), "weights": f32(w),
         "parents": np.asarray(parents, np.int32)}
    if keypoints:
        kr = rng.random((keypoints, NV)) * (rng.random((keypoints, NV)) < 0.01)
        kr[:, 0] += 1e-3
        kr /= kr.sum(1, keepdims=True)
        for k in range(2, keypoints, 4):
            kr[k] = 0.0
            kr[k, rng.integers(NV)] = 1.0
        t["keypoint_regressor"] = f32(kr)
    return t


def rot6d_to_rotmat(poses6, robust=False):
    """(..., 6) -> (..., 3, 3); reference hand/manopth/rot6d.py:4-24 (robust: :26-51)"""
    p = poses6.reshape(-1, 6)
    ops._chk(p, torch.float32, "rot6d.poses")
    out = torch.empty(p.shape[0], 3, 3, device=p.device, dtype=torch.float32)
    ops.launch("mhe_rot6d_to_rotmat_f32", p, out, p.shape[0], int(robust))
    return out.view(*poses6.shape[:-1], 3, 3)


def rotmat_to_rot6d(rotmats):
    """(..., 3, 3) -> (..., 6): the first two COLUMNS [R[:, 0] | R[:, 1]], the layout rot6d_to_rotmat reads (reference hand/manopth/rot6d.py:12-23),
    so that rot6d_to_rotmat(rotmat_to_rot6d(R)) == R for a rotation R.  A re-arrangement only (no arithmetic; any device)"""
    if rotmats.shape[-2:] != (3, 3):
        raise ValueError(f"rotmat_to_rot6d: (..., 3, 3) expected, got {tuple(rotmats.shape)}")
    return torch.cat([rotmats[..., :, 0], rotmats[..., :, 1]], -1)


def rot6d_to_rotmat_bwd(poses6, g_rotmats):
    p, g = poses6.reshape(-1, 6), g_rotmats.reshape(-1, 9)
    ops._chk(p, torch.float32, "rot6d.poses"); ops._chk(g, torch.float32, "rot6d.g", (p.shape[0], 9))
    out = torch.empty_like(p)
    ops.launch("mhe_rot6d_to_rotmat_bwd_f32", p, g, out, p.shape[0])
    return out.view(poses6.shape)


class BodyLayer(nn.Module):
    """linear-blend skinning of a (J, NV) body model from rotation matrices or a 6D pose; buffers carry SMPL's names"""
    def __init__(self, tables):
        super().__init__()
        t = {k: np.asarray(v) for k, v in tables.items()}
        self.NV, self.J, self.nb = t["v_template"].shape[0], t["weights"].shape[1], t["shapedirs"].shape[2]
        if self.J > 32 or t["posedirs"].shape[2] != 9 * (self.J - 1):
            raise ValueError("BodyLayer: J <= 32 and posedirs with 9 (J-1) pose-blend coefficients")
        parents = t["parents"].astype(np.int64)
        if parents[0] != -1 or (parents[1:] >= np.arange(1, self.J)).any():
            raise ValueError("BodyLayer: parents[0] must be -1 and parents[j] < j")
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32))
        for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"):          # SMPL-named buffers (state_dict surface)
            self.register_buffer(k, f(t[k]))
        self.register_buffer("parents", torch.as_tensor(parents.astype(np.int32)))
        # kernel-side layouts: joint regression folded into the tables, vertex-fastest blend shapes with a padded pitch
        self.VP = (self.NV + 63) // 64 * 64
        vp = lambda a: np.ascontiguousarray(np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, self.VP - self.NV)]), np.float32)
        jr = t["J_regressor"].astype(np.float64)
        self.register_buffer("_jt", f(jr @ t["v_template"].astype(np.float64)), persistent=False)                          # [J,3]
        self.register_buffer("_jsd", f(np.einsum("jv,vck->jck", jr, t["shapedirs"].astype(np.float64))), persistent=False)  # [J,3,nb]
        self.register_buffer("_vt", f(vp(t["v_template"].T)), persistent=False)                                             # [3][VP]
        self.register_buffer("_vsd", f(vp(t["shapedirs"].transpose(2, 1, 0))), persistent=False)                            # [nb][3][VP]
        self.register_buffer("_vpd", f(vp(t["posedirs"].transpose(2, 1, 0))), persistent=False)                             # [9(J-1)][3][VP]
        self.register_buffer("_vw", f(vp(t["weights"].T)), persistent=False)                                                # [J][VP]
        self.NK = 0
        if t.get("keypoint_regressor") is not None:          # keypoints = regressor x vertices (reference hand/ManoLayer.py:141-148 at other sizes)
            kr = t["keypoint_regressor"]
            if kr.ndim != 2 or kr.shape[1] != self.NV or not 1 <= kr.shape[0] <= 64:
                raise ValueError(f"BodyLayer: keypoint_regressor must be (NK, {self.NV}) with 1 <= NK <= 64, got {tuple(kr.shape)}")
            self.NK = kr.shape[0]
            self.register_buffer("keypoint_regressor", f(kr))

    def _split_tables(self, dev):
        """the vertex tables as bf16 pieces in MFMA operand order (19 MB for SMPL), made on first use per device; the tables are fixed buffers"""
        key = (dev.type, dev.index, self._vt.data_ptr())
        if getattr(self, "_split_key", None) != key:
            L = _lib.lib()
            sp = torch.empty(L.mhe_lbs_split_floats(self.J, self.nb, self.VP), device=dev, dtype=torch.float32)
            ops.launch("mhe_lbs_split_tables_f32", self._vt, self._vsd, self._vpd, self._vw, sp, self.J, self.nb, self.VP)
            self._split, self._split_key = sp, key
        return self._split

    def _kp_split(self, dev):
        """the keypoint regressor as bf16 pieces in MFMA operand order (mhe_lbs_kp_split_tables_f32), made on first use per device like _split_tables
        and again whenever the buffer is written in place (it is persistent: load_state_dict copies into it without moving it)"""
        key = (dev.type, dev.index, self.keypoint_regressor.data_ptr(), self.keypoint_regressor._version)
        if getattr(self, "_kp_key", None) != key:
            L = _lib.lib()
            sp = torch.empty(L.mhe_lbs_kp_split_floats(self.NK, self.VP), device=dev, dtype=torch.float32)
            ops.launch("mhe_lbs_kp_split_tables_f32", self.keypoint_regressor, sp, self.NK, self.NV, self.VP)
            self._kp_sp, self._kp_key = sp, key
        return self._kp_sp

    def _bwd_tables(self, dev):
        """coefficient-fastest copies of the blend-shape and weight tables for the skinning reverse (mhe_lbs_bwd_tables_f32, 19 MB for SMPL), made
        on first use per device like _split_tables"""
        key = (dev.type, dev.index, self._vt.data_ptr())
        if getattr(self, "_bwd_key", None) != key:
            L = _lib.lib()
            tb = torch.empty(L.mhe_lbs_bwd_tables_floats(self.J, self.nb, self.VP), device=dev, dtype=torch.float32)
            ops.launch("mhe_lbs_bwd_tables_f32", self._vsd, self._vpd, self._vw, tb, self.J, self.nb, self.NV, self.VP)
            self._bwd_tab, self._bwd_key = tb, key
        return self._bwd_tab

    def forward(self, betas, rotmats=None, pose6d=None, scale=1.0, want_verts=True, want_keypoints=False):
        """betas (R,nb); rotmats (R,J,3,3) or pose6d (R,6J) -> {'vertices' (R,NV,3), 'joints' (R,J,3), 'rotmats'}; want_keypoints adds
        'keypoints' (R,NK,3) = keypoint_regressor x vertices, accumulated inside the skinning pass (with want_verts=False no (R,NV,3) tensor exists)"""
        if want_keypoints and not self.NK:
            raise ValueError("BodyLayer: want_keypoints=True needs tables with a 'keypoint_regressor'")
        if rotmats is None:
            rotmats = rot6d_to_rotmat(pose6d.reshape(-1, self.J, 6).contiguous())
        R = rotmats.shape[0]
        rotmats, betas = rotmats.contiguous(), betas.contiguous()
        ops._chk(rotmats, torch.float32, "body.rotmats", (R, self.J, 3, 3)); ops._chk(betas, torch.float32, "body.betas", (R, self.nb))
        L, dev = _lib.lib(), rotmats.device
        ws = torch.empty(L.mhe_lbs_workspace_floats(R, self.J, self.nb), device=dev, dtype=torch.float32)
        joints = torch.empty(R, self.J, 3, device=dev, dtype=torch.float32)
        ops.launch("mhe_lbs_pose_f32", rotmats, betas, self._jt, self._jsd, self.parents, ws, joints, R, self.J, self.nb)
        out = {"joints": joints, "rotmats": rotmats}
        if want_keypoints:
            verts = torch.empty(R, self.NV, 3, device=dev, dtype=torch.float32) if want_verts else None
            kp = torch.empty(R, self.NK, 3, device=dev, dtype=torch.float32)
            if os.environ.get("MHE_LBS_MFMA", "1") == "1" and L.mhe_lbs_skin_kp_supported(R, self.J, self.nb, self.NV, self.VP, self.NK, int(want_verts)):
                ops.launch("mhe_lbs_skin_kp_mfma_f32", ws, self._split_tables(dev), self._kp_split(dev), verts, kp, R, self.J, self.nb, self.NV, self.VP, self.NK,
                           float(scale))
            else:
                ops.launch("mhe_lbs_skin_kp_f32", ws, self._vt, self._vsd, self._vpd, self._vw, self.keypoint_regressor, verts, kp, R, self.J, self.nb, self.NV,
                           self.VP, self.NK, float(scale))
            out["keypoints"] = kp
            if want_verts:
                out["vertices"] = verts
            return out
        if want_verts:
            verts = torch.empty(R, self.NV, 3, device=dev, dtype=torch.float32)
            if os.environ.get("MHE_LBS_MFMA", "1") == "1" and self.VP % 32 == 0 and L.mhe_lbs_skin_mfma_supported(R, self.J, self.nb, self.NV, self.VP):
                # both products on the matrix cores from bf16 pieces of the f32 operands (csrc/lbs_skin.hip); the table pieces are made once
                ops.launch("mhe_lbs_skin_mfma_f32", ws, self._split_tables(dev), verts, R, self.J, self.nb, self.NV, self.VP, float(scale))
                out["vertices"] = verts
                return out
            ops.launch("mhe_lbs_skin_f32", ws, self._vt, self._vsd, self._vpd, self._vw, verts, R, self.J, self.nb, self.NV, self.VP, float(scale))
            out["vertices"] = verts
        return out

    def vertex_error(self, betas, rotmats=None, pose6d=None, target_verts=None, center=None, scale=1.0):
        """mean per-vertex error of R hypotheses against B target meshes without a vertex tensor: betas (R,nb); rotmats (R,J,3,3) or pose6d (R,6J);
        target_verts (B,NV,3) with R % B == 0 (row r belongs to image r // (R // B): the head's batch-major order); center (R,3) or None (zero) ->
        err (R,) = mean over v of || scale * vert[r, v] - center[r] - target_verts[b, v] ||_2, accumulated inside the skinning pass
        (mhe_lbs_skin_err_mfma_f32, or mhe_lbs_skin_err_f32 with MHE_LBS_MFMA=0 / sizes the matrix-core kernel does not take) from the values
        `forward` would store as 'vertices'; fixed summation order (two calls give the same bits).  Inference only: no gradient."""
        if not isinstance(target_verts, torch.Tensor) or target_verts.dim() != 3 or tuple(target_verts.shape[1:]) != (self.NV, 3):
            raise ValueError(f"BodyLayer.vertex_error: target_verts must be a (B, {self.NV}, 3) tensor, got {tuple(getattr(target_verts, 'shape', ()))}")
        if (rotmats is None) == (pose6d is None):
            raise ValueError("BodyLayer.vertex_error: give exactly one of rotmats and pose6d")
        R, B = (rotmats if rotmats is not None else pose6d).shape[0], target_verts.shape[0]
        if B < 1 or R % B:
            raise ValueError(f"BodyLayer.vertex_error: R={R} rows are not a multiple of B={B} target meshes")
        if tuple(betas.shape) != (R, self.nb):
            raise ValueError(f"BodyLayer.vertex_error: betas must be ({R}, {self.nb}), got {tuple(betas.shape)}")
        if center is not None and tuple(center.shape) != (R, 3):
            raise ValueError(f"BodyLayer.vertex_error: center must be ({R}, 3), got {tuple(center.shape)}")
        with torch.no_grad():
            if rotmats is None:
                rotmats = rot6d_to_rotmat(pose6d.reshape(-1, self.J, 6).contiguous())
            rotmats, betas, target_verts = rotmats.contiguous(), betas.contiguous(), target_verts.contiguous()
            ops._chk(rotmats, torch.float32, "body.rotmats", (R, self.J, 3, 3)); ops._chk(betas, torch.float32, "body.betas", (R, self.nb))
            ops._chk(target_verts, torch.float32, "body.target_verts", (B, self.NV, 3))
            if center is not None:
                center = center.contiguous()
                ops._chk(center, torch.float32, "body.center", (R, 3))
            L, dev = _lib.lib(), rotmats.device
            ws = torch.empty(L.mhe_lbs_workspace_floats(R, self.J, self.nb), device=dev, dtype=torch.float32)
            ops.launch("mhe_lbs_pose_f32", rotmats, betas, self._jt, self._jsd, self.parents, ws, None, R, self.J, self.nb)
            err = torch.empty(R, device=dev, dtype=torch.float32)
            if os.environ.get("MHE_LBS_MFMA", "1") == "1" and L.mhe_lbs_skin_err_supported(R, self.J, self.nb, self.NV, self.VP, B):
                ops.launch("mhe_lbs_skin_err_mfma_f32", ws, self._split_tables(dev), target_verts, center, err, R, B, self.J, self.nb, self.NV, self.VP,
                           float(scale))
            else:
                ops.launch("mhe_lbs_skin_err_f32", ws, self._vt, self._vsd, self._vpd, self._vw, target_verts, center, err, R, B, self.J, self.nb, self.NV, self.VP,
                           float(scale))
        return err


def _root_indices(root, P, who):
    """root = None | int | tuple of ints -> a tuple of distinct indices in 0..P-1 (ValueError otherwise)"""
    if root is None:
        return ()
    try:
        idx = (root,) if isinstance(root, (int, np.integer)) else tuple(root)
    except TypeError:
        idx = ()
    if not idx or any(not isinstance(q, (int, np.integer)) or isinstance(q, bool) for q in idx):
        raise ValueError(f"{who}: root must be None, an int or a non-empty tuple of ints, got {root!r}")
    if any(not 0 <= q < P for q in idx):
        raise ValueError(f"{who}: root index outside 0..{P - 1}: {root!r}")
    if len(set(idx)) != len(idx):
        raise ValueError(f"{who}: root indices repeat: {root!r}")
    return tuple(int(q) for q in idx)


def _check_ns(ns, K, who):
    ns = tuple(ns) if not isinstance(ns, (int, np.integer)) else (ns,)
    if not 1 <= len(ns) <= 8 or any(not isinstance(n, (int, np.integer)) or isinstance(n, bool) for n in ns):
        raise ValueError(f"{who}: ns must hold 1 to 8 integers, got {ns!r}")
    if any(not 1 <= n <= K for n in ns) or any(b <= a for a, b in zip(ns, ns[1:])):
        raise ValueError(f"{who}: ns must be strictly increasing within 1..K={K}, got {ns!r}")
    return tuple(int(n) for n in ns)


def _point_errors_launch(points, target, mask):
    B, K, P = points.shape[:3]
    err = torch.empty(B, K, device=points.device, dtype=torch.float32)
    ops.launch("mhe_point_errors_f32", points, target, err, B, K, P, mask)
    return err


def point_errors(points, target, root=None):
    """points (B,K,P,3), target (B,P,3), 1 <= P <= 64 -> {'mpjpe' (B,K), 'pa_mpjpe' (B,K)}.  `root` (None, an index or a tuple of indices, e.g. the
    two hips): the mean of those points is subtracted from each prediction and from the target before the error is taken.
    mpjpe = mean over P of the Euclidean distance (mhe_point_errors_f32: one wave per row, fixed summation order).  pa_mpjpe = the same error
    after the project's Procrustes alignment with scale of every hypothesis to its target (ops.procrustes_align on the sample-major view, then the
    same kernel without centring).  Convention, pinned with that kernel: the reference's align_w_scale (hand/utils.py:502-525), R = U V^T WITHOUT
    the determinant correction, so the optimal map may be a reflection where the data ask for one.  ProHMR's own evaluation code is out of tree:
    whether it corrects the determinant is unpinned.  Inference only."""
    if not isinstance(points, torch.Tensor) or points.dim() != 4 or points.shape[-1] != 3:
        raise ValueError("point_errors: points must be a (B, K, P, 3) tensor")
    B, K, P = points.shape[:3]
    if not 1 <= P <= 64:
        raise ValueError(f"point_errors: P={P} outside 1..64")
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (B, P, 3):
        raise ValueError(f"point_errors: target must be ({B}, {P}, 3), got {tuple(getattr(target, 'shape', ()))}")
    idx = _root_indices(root, P, "point_errors")
    mask = sum(1 << q for q in idx)
    with torch.no_grad():
        points, target = points.contiguous(), target.contiguous()
        ops._chk(points, torch.float32, "point_errors.points", (B, K, P, 3)); ops._chk(target, torch.float32, "point_errors.target", (B, P, 3))
        mpjpe = _point_errors_launch(points, target, mask)
        aligned = ops.procrustes_align(points.permute(1, 0, 2, 3).contiguous(), target)                 # (K, B, P, 3), in the target's frame
        pa = _point_errors_launch(aligned.permute(1, 0, 2, 3).contiguous(), target, 0)
    return {"mpjpe": mpjpe, "pa_mpjpe": pa}


def min_of_n(err, ns):
    """err (B,K), ns = 1 to 8 strictly increasing integers in 1..K -> (values (B,len(ns)) f32, index (B,len(ns)) int32): values[b, i] =
    min err[b, :ns[i]], index = the lowest k attaining it (mhe_min_of_n_f32).  Non-finite input is rejected nowhere and its result is
    unspecified.  Inference only."""
    if not isinstance(err, torch.Tensor) or err.dim() != 2:
        raise ValueError("min_of_n: err must be a (B, K) tensor")
    B, K = err.shape
    ns = _check_ns(ns, K, "min_of_n")
    with torch.no_grad():
        err = err.contiguous()
        ops._chk(err, torch.float32, "min_of_n.err", (B, K))
        val = torch.empty(B, len(ns), device=err.device, dtype=torch.float32)
        idx = torch.empty(B, len(ns), device=err.device, dtype=torch.int32)
        arr = (C.c_int * len(ns))(*ns)
        ops.launch("mhe_min_of_n_f32", err, val, idx, B, K, C.cast(arr, C.c_void_p), len(ns))
    return val, idx


class BodyFlowHead(nn.Module):
    """ProHMR's sampling surface (reference README.md:26-42): `flow(conditioning_feats, num_samples)` draws K poses with
    log-probabilities from a ConditionalGlow over the 144-D 6D pose (features 144, hidden 1024, 4 layers x 2 blocks, context
    2048: SURVEY.md appendix A5), decoded by the body layer; and its likelihood surface `log_prob(feats, pose6d= | rotmats=)` (README.md:32-34: the
    NLL on annotated poses).  Both are trainable: the sampling direction's tape and reverse (_HeadFn) and the density direction's
    (ConditionalGlow.log_prob under grad).  Parity unpinned (ProHMR's SMPLFlow is out of tree)."""
    def __init__(self, tables, context_features=2048, hidden=1024, num_layers=4, num_blocks=2):
        super().__init__()
        from .glow import ConditionalGlow
        self.body = BodyLayer(tables)
        self.flow = ConditionalGlow(6 * self.body.J, hidden, num_layers, num_blocks, context_features=context_features,
                                    dropout_probability=0.0)

    def forward(self, feats, num_samples, betas=None, noise=None, hyp_slice=None, want_verts=True, verts_grad=False, want_keypoints=False):
        """feats (B,F) -> pose6d (B,K,6J), log_prob (B,K), vertices (B,K,NV,3), joints (B,K,J,3); hyp_slice = (lo, hi) decodes only
        hypotheses lo..hi-1 of every image (the hypothesis-sharded form).  want_keypoints adds keypoints (B, hi-lo, NK, 3) from the body layer's
        keypoint_regressor (no vertex tensor is needed for them: want_verts=False); under grad they carry gradients like the joints, through the
        skinning reverse, without verts_grad.

        Differentiable when grad is enabled and `feats` or `betas` require grad, or the head is in train mode with flow parameters that require
        grad (one autograd node, _HeadFn, whose backward is the hand-written reverse pass; an eval-mode call on plain inputs stays the
        inference pass and returns plain tensors): log_prob, pose6d and joints carry gradients to every flow parameter, feats and betas; with
        verts_grad=True so do vertices (the skinning reverse, lbs_bwd).  Refused there (NotImplementedError): a non-zero gradient on vertices
        without verts_grad=True, compute_dtype bfloat16, dropout p > 0 in train mode.  verts_grad changes nothing on the inference pass."""
        if verts_grad and not want_verts:
            raise ValueError("BodyFlowHead: verts_grad=True needs want_verts=True")
        if want_keypoints and not self.body.NK:
            raise ValueError("BodyFlowHead: want_keypoints=True needs body tables with a 'keypoint_regressor'")
        params = [p for p in self.flow.parameters()]
        if torch.is_grad_enabled() and ((self.training and any(p.requires_grad for p in params)) or feats.requires_grad
                                        or (betas is not None and betas.requires_grad)):
            if noise is None:
                noise = ops.randn(feats.shape[0] * num_samples, self.flow.features, feats.device).view(feats.shape[0], num_samples, self.flow.features)
            lo, hi = hyp_slice if hyp_slice is not None else (0, num_samples)
            vals = _HeadFn.apply(self, feats, betas, noise, num_samples, lo, hi, want_verts, bool(verts_grad), bool(want_keypoints), *params)
            res = {"pose6d": vals[0], "log_prob": vals[1], "joints": vals[2]}
            if want_verts:
                res["vertices"] = vals[3]
            if want_keypoints:
                res["keypoints"] = vals[-1]
            return res
        B = feats.shape[0]
        pose, logp, _ = self.flow.sample_and_log_prob(num_samples, noise=noise, context=feats)
        lo, hi = hyp_slice if hyp_slice is not None else (0, num_samples)
        p = pose[:, lo:hi].reshape(B * (hi - lo), -1).contiguous()
        bt = betas if betas is not None else torch.zeros(B, self.body.nb, device=feats.device)
        bt = bt[:, None, :].expand(B, hi - lo, self.body.nb).reshape(B * (hi - lo), self.body.nb).contiguous()
        out = self.body(bt, pose6d=p, want_verts=want_verts, want_keypoints=want_keypoints)
        res = {"pose6d": pose, "log_prob": logp, "joints": out["joints"].view(B, hi - lo, self.body.J, 3)}
        if want_verts:
            res["vertices"] = out["vertices"].view(B, hi - lo, self.body.NV, 3)
        if want_keypoints:
            res["keypoints"] = out["keypoints"].view(B, hi - lo, self.body.NK, 3)
        return res

    def evaluate(self, feats, num_samples, target_keypoints, target_verts=None, betas=None, noise=None, ns=(1, 5, 10, 25), root=None, mode_first=True):
        """the multi-hypothesis evaluation protocol on the GPU, under no_grad in whatever mode the module is in: feats (B,F), target_keypoints
        (B,NK,3) (the frame of the body layer's 'keypoints'), target_verts (B,NV,3) or None, betas (B,nb) or None (zero) -> a dict of plain tensors:
        'mpjpe', 'pa_mpjpe' (B,K) (point_errors of the mesh-regressed keypoints; `root` as there), 'pve' (B,K) (only with target_verts:
        BodyLayer.vertex_error, the prediction centred on its own root keypoint and the target on its own - nothing is centred with root=None),
        'min_mpjpe', 'min_pa_mpjpe', 'min_pve' (B,len(ns)) and 'argmin_*' (int32) = min_of_n over the first ns[i] hypotheses, 'log_prob' (B,K),
        'pose6d' (B,K,6J).  mode_first: hypothesis 0 of every image is decoded from zero noise, the mode of the flow (ProHMR's protocol); a given
        `noise` (B,K,6J) is copied, never written.  No (B K, NV, 3) tensor is allocated.  ProHMR's own joint maps, camera and Procrustes variant
        are out of tree: parity with its published numbers is unpinned (see point_errors).  ValueError before any GPU work: tables without a
        'keypoint_regressor', a root index outside NK, ns outside 1..K or not increasing, shape mismatches."""
        NK, NV, nb, D = self.body.NK, self.body.NV, self.body.nb, self.flow.features
        if not NK:
            raise ValueError("BodyFlowHead.evaluate: needs body tables with a 'keypoint_regressor'")
        if not isinstance(feats, torch.Tensor) or feats.dim() != 2:
            raise ValueError("BodyFlowHead.evaluate: feats must be a (B, F) tensor")
        B, K = feats.shape[0], int(num_samples)
        if K < 1:
            raise ValueError(f"BodyFlowHead.evaluate: num_samples={num_samples}")
        if not isinstance(target_keypoints, torch.Tensor) or tuple(target_keypoints.shape) != (B, NK, 3):
            raise ValueError(f"BodyFlowHead.evaluate: target_keypoints must be ({B}, {NK}, 3), got {tuple(getattr(target_keypoints, 'shape', ()))}")
        if target_verts is not None and (not isinstance(target_verts, torch.Tensor) or tuple(target_verts.shape) != (B, NV, 3)):
            raise ValueError(f"BodyFlowHead.evaluate: target_verts must be ({B}, {NV}, 3), got {tuple(getattr(target_verts, 'shape', ()))}")
        if betas is not None and tuple(betas.shape) != (B, nb):
            raise ValueError(f"BodyFlowHead.evaluate: betas must be ({B}, {nb}), got {tuple(betas.shape)}")
        if noise is not None and tuple(noise.shape) != (B, K, D):
            raise ValueError(f"BodyFlowHead.evaluate: noise must be ({B}, {K}, {D}), got {tuple(noise.shape)}")
        idx = _root_indices(root, NK, "BodyFlowHead.evaluate")
        ns = _check_ns(ns, K, "BodyFlowHead.evaluate")
        with torch.no_grad():
            dev = feats.device
            if noise is None:
                noise = ops.randn(B * K, D, dev).view(B, K, D)
            elif mode_first:
                noise = noise.clone()
            if mode_first:
                noise[:, 0] = 0.0
            pose, logp, _ = self.flow.sample_and_log_prob(K, noise=noise, context=feats)
            p = pose.reshape(B * K, D).contiguous()
            bt = betas if betas is not None else torch.zeros(B, nb, device=dev)
            bt = bt[:, None, :].expand(B, K, nb).reshape(B * K, nb).contiguous()
            out = self.body(bt, pose6d=p, want_verts=False, want_keypoints=True)
            kp = out["keypoints"].view(B, K, NK, 3)
            res = {"pose6d": pose, "log_prob": logp, **point_errors(kp, target_keypoints, root)}
            if target_verts is not None:
                center, tv = None, target_verts
                if idx:
                    center = kp[:, :, list(idx)].mean(2).reshape(B * K, 3)
                    tv = target_verts - target_keypoints[:, list(idx)].mean(1, keepdim=True)
                res["pve"] = self.body.vertex_error(bt, rotmats=out["rotmats"], target_verts=tv, center=center).view(B, K)
            for k in ("mpjpe", "pa_mpjpe", "pve"):
                if k in res:
                    res["min_" + k], res["argmin_" + k] = min_of_n(res[k], ns)
        return res

    def log_prob(self, feats, pose6d=None, rotmats=None):
        """ProHMR's NLL call form `flow.log_prob(smpl_params, conditioning_feats)` (reference README.md:32-34): one annotated pose per context row,
        pose6d (R, 6J) or rotmats (R, J, 3, 3) (exactly one; rotations are re-arranged by rotmat_to_rot6d) -> (log_prob (R,), z (R, 6J)).
        Differentiable under ConditionalGlow.log_prob's rule, so `-head.log_prob(f, rotmats=M)[0].mean()` trains the flow by maximum likelihood,
        alone or in one loss with the entropy term of `forward`."""
        if (pose6d is None) == (rotmats is None):
            raise ValueError("BodyFlowHead.log_prob: give exactly one of pose6d and rotmats")
        if pose6d is None:
            pose6d = rotmat_to_rot6d(rotmats)
        return self.flow.log_prob(pose6d.reshape(-1, self.flow.features), feats)


def lbs_pose_bwd(layer, rotmats, betas, g_joints):
    """reverse of BodyLayer's posed joints: g_joints (R,J,3) -> (g_rotmats (R,J,3,3), g_betas (R,nb)) (mhe_lbs_pose_bwd_f32)"""
    R = rotmats.shape[0]
    ops._chk(rotmats, torch.float32, "lbs_bwd.rotmats", (R, layer.J, 3, 3)); ops._chk(betas, torch.float32, "lbs_bwd.betas", (R, layer.nb))
    ops._chk(g_joints, torch.float32, "lbs_bwd.g_joints", (R, layer.J, 3))
    g_rot, g_bt = torch.empty_like(rotmats), torch.empty_like(betas)
    ops.launch("mhe_lbs_pose_bwd_f32", rotmats, betas, layer._jt, layer._jsd, layer.parents, g_joints, g_rot, g_bt, R, layer.J, layer.nb)
    return g_rot, g_bt


KP_BWD_MAX_ROWS = 262144    # rows per mhe_lbs_keypoints_bwd_f32 launch (the entry takes up to 524,280: 8 rows per workgroup, 65,535 in grid y)
KP_BWD_ROWS = 8192          # rows per pass of lbs_bwd when only keypoints carry a gradient: bounds the (rows, NV, 3) vertex-gradient buffer (677 MB for
                            # SMPL) and still gives the skinning reverse one 32-row workgroup per CU (4,096 rows left half of the CUs idle)


def lbs_bwd(layer, rotmats, betas, g_verts, g_joints=None, scale=1.0, g_keypoints=None):
    """reverse of BodyLayer's vertices, keypoints and posed joints: g_verts (R,NV,3) = dL/dvertices of `layer(betas, rotmats=rotmats, scale=scale)`
    (or None), g_keypoints (R,NK,3) or None (at least one of the two), g_joints (R,J,3) or None -> (g_rotmats (R,J,3,3), g_betas (R,nb)).  The pose
    pass is run again for its workspace rows; the keypoints' reverse (mhe_lbs_keypoints_bwd_f32: regressor^T g_keypoints added to a copy of g_verts
    - a second (R, NV, 3) buffer, 1.35 GB at R = 16,384 for SMPL: the caller's gradient is not written - or, without g_verts, written into a buffer of KP_BWD_ROWS rows that the skinning reverse then walks chunk by chunk); the skinning reverse
    (mhe_lbs_skin_bwd_f32, exact-f32 matrix-core reductions over the vertices) then the pose chain's (mhe_lbs_transforms_bwd_f32)."""
    R, J, nb = rotmats.shape[0], layer.J, layer.nb
    if g_verts is None and g_keypoints is None:
        raise ValueError("lbs_bwd: give g_verts or g_keypoints (joints alone: lbs_pose_bwd)")
    if g_keypoints is not None and not layer.NK:
        raise ValueError("lbs_bwd: g_keypoints given but the layer has no 'keypoint_regressor'")
    ops._chk(rotmats, torch.float32, "lbs_bwd.rotmats", (R, J, 3, 3)); ops._chk(betas, torch.float32, "lbs_bwd.betas", (R, nb))
    if g_verts is not None:
        ops._chk(g_verts, torch.float32, "lbs_bwd.g_verts", (R, layer.NV, 3))
    if g_keypoints is not None:
        ops._chk(g_keypoints, torch.float32, "lbs_bwd.g_keypoints", (R, layer.NK, 3))
    if g_joints is not None:
        ops._chk(g_joints, torch.float32, "lbs_bwd.g_joints", (R, J, 3))
    L, dev = _lib.lib(), rotmats.device
    ws = torch.empty(L.mhe_lbs_workspace_floats(R, J, nb), device=dev, dtype=torch.float32)
    ops.launch("mhe_lbs_pose_f32", rotmats, betas, layer._jt, layer._jsd, layer.parents, ws, None, R, J, nb)
    g_tf = torch.empty(R, J, 12, device=dev, dtype=torch.float32)
    g_pm = torch.empty(R, 9 * (J - 1), device=dev, dtype=torch.float32)
    g_bt = torch.empty_like(betas)
    wstride = ws.numel() // R

    def skin_bwd(gv, lo, n):          # rows lo .. lo + n - 1 (row slices of contiguous tensors are contiguous)
        ops.launch("mhe_lbs_skin_bwd_f32", ws[lo * wstride:], layer._vt, layer._vsd, layer._vpd, layer._vw, layer._bwd_tables(dev), gv, g_tf[lo:], g_pm[lo:],
                   g_bt[lo:], n, J, nb, layer.NV, layer.VP, float(scale))

    def kp_bwd(gv, lo, n, accumulate):
        ops.launch("mhe_lbs_keypoints_bwd_f32", layer.keypoint_regressor, g_keypoints[lo:], gv, n, layer.NK, layer.NV, int(accumulate))

    if g_keypoints is None:
        skin_bwd(g_verts, 0, R)
    elif g_verts is not None:
        gv = g_verts.clone()
        for lo in range(0, R, KP_BWD_MAX_ROWS):
            kp_bwd(gv[lo:], lo, min(KP_BWD_MAX_ROWS, R - lo), True)
        skin_bwd(gv, 0, R)
    else:
        gv = torch.empty(min(R, KP_BWD_ROWS), layer.NV, 3, device=dev, dtype=torch.float32)
        for lo in range(0, R, KP_BWD_ROWS):
            n = min(KP_BWD_ROWS, R - lo)
            kp_bwd(gv, lo, n, False)
            skin_bwd(gv, lo, n)
    g_rot = torch.empty_like(rotmats)
    ops.launch("mhe_lbs_transforms_bwd_f32", rotmats, betas, layer._jt, layer._jsd, layer.parents, g_joints, g_tf, g_pm, g_bt, g_rot, g_bt, R, J, nb)
    return g_rot, g_bt


def _flow_sample_with_tape(g, noise_rows, context, N):
    """the flow's f32 sampling pass on batch-major rows (r = b N + n) with its tape: ConditionalGlow._run, the no-grad pass's own code ->
    (x (B N, D), log_prob (B N,), tape)"""
    if g.compute_dtype != torch.float32:
        raise NotImplementedError("the Glow reverse pass runs in f32 parity mode: compute_dtype must be torch.float32 under grad")
    if g.training and g.p_drop > 0.0:
        raise NotImplementedError("the wide Glow reverse pass has no dropout: build the flow with dropout_probability=0 or call eval()")
    ops._chk(noise_rows, torch.float32, "glow.noise", (noise_rows.shape[0], g.features))
    pk = g._packed()
    aff = pk["aff"]         # the wide float64 affine maps + workspace (the pack holds them above 64 features)
    if not ("ws" in aff and aff["A"].shape[-1] == g.Dp and aff["ws"].numel() == _lib.lib().mhe_glow_affine_wide_workspace_doubles(g.num_layers, g.features)):
        aff = ops.glow_affine_wide(g.small_param_table(), g.num_layers, g.features, g._transform._transforms[1].eps)
    tape = {"aff": aff, "context": context, "sample_major": False}
    x, lp = g._run(noise_rows, context, True, N, context.shape[0], pk=pk, tape=tape)
    return x, lp, tape


def _flow_backward(g, tp, g_x, g_logq):
    """the flow's reverse pass over that tape: ConditionalGlow._reverse into fresh gradients, then the context weights' gradient from the
    per-image rows, dL/dcontext and the ActNorm / LU gradients from dA^-1, dc^-1 and sum dL/dlog q in float64 (mhe_glow_affine_wide_bwd_f64).
    g_x (B N, D) = dL/dx (or None), g_logq (B N,) = dL/dlog_prob (or None) -> ({parameter: gradient}, dL/dcontext (B, F)).  The noise is an
    input, not differentiated."""
    D, Lr, Dp = g.features, g.num_layers, g.Dp
    pk, aff, ctab, B = tp["pk"], tp["aff"], tp["ctab"], tp["n_img"]
    R, cs, dev = B * tp["row_div"], ctab.shape[1], ctab.device
    gv = torch.zeros(R, Dp, device=dev)
    if g_x is not None:
        ops.launch("mhe_pad64_f32", g_x, gv, R, D)
    if g_logq is not None:
        ops._chk(g_logq, torch.float32, "glow.g_log_prob", (R,))
    Gct = torch.zeros(B, cs, device=dev)
    dAinv, dcinv = torch.zeros(Lr, Dp, Dp, device=dev), torch.empty(Lr, Dp, device=dev)
    z = lambda *shape: torch.zeros(*shape, device=dev)
    dst = [{**o, "dAinv": dAinv[l], "dcinv": dcinv[l]} for l, o in enumerate(g._net_grad_buffers(pk, dev))]
    # the transposed operands one layer at a time, as the reverse reaches it
    g._reverse(tp, gv, g_logq, Gct, ({**o, "AinvT": aff["AinvT"][l], "wfT": d["wf"].t().contiguous(), "wxT": d["wx"].t().contiguous(),
                                      "blocksT": [(w0.t().contiguous(), w1.t().contiguous()) for (w0, _, w1, _) in d["blocks"]]}
                                     for l, (d, o) in enumerate(zip(pk["layers"], dst))))
    dW, db = z(cs, g.context_features), z(cs)
    ops.linear_wgrad(tp["context"], Gct, dW); ops.colsum(Gct, db)
    g_ctx = ops.linear(Gct, pk["wctx"].t().contiguous())
    ga = ops.glow_affine_wide_bwd(dAinv, dcinv, g_logq, Lr, D, aff["ws"]).float()
    return g._grads_by_param(pk, dst, dW, db, ga), g_ctx


class _HeadFn(torch.autograd.Function):
    """BodyFlowHead.forward as one autograd node: forward = the f32 sampling pass with a tape (_flow_sample_with_tape, bit-identical to the
    no-grad pass) + the body decode; backward = joints -> rotations -> 6D poses (mhe_lbs_pose_bwd_f32, mhe_rot6d_to_rotmat_bwd_f32) added to
    dL/dpose6d on the slice's rows, then the flow's reverse pass (_flow_backward).  With verts_grad, a vertex gradient takes lbs_bwd (the
    skinning reverse together with the joints'); without one the route is the joints-only one whatever verts_grad says.  A gradient on the
    keypoints (want_kp: one more output) takes lbs_bwd too, through mhe_lbs_keypoints_bwd_f32, with or without verts_grad / want_verts."""
    @staticmethod
    def forward(ctx, head, feats, betas, noise, K, lo, hi, want_verts, verts_grad, want_kp, *params):
        B, D, nb, J = feats.shape[0], head.flow.features, head.body.nb, head.body.J
        x, lp, tape = _flow_sample_with_tape(head.flow, noise.reshape(B * K, D).contiguous(), feats.contiguous(), K)
        pose = x.view(B, K, D)
        p = pose[:, lo:hi].reshape(B * (hi - lo), D).contiguous()
        bt = betas.contiguous() if betas is not None else torch.zeros(B, nb, device=feats.device)
        bt = bt[:, None, :].expand(B, hi - lo, nb).reshape(B * (hi - lo), nb).contiguous()
        out = head.body(bt, pose6d=p, want_verts=want_verts, want_keypoints=want_kp)
        ctx.head, ctx.tape, ctx.shape, ctx.has_betas, ctx.verts_grad = head, tape, (B, K, lo, hi), betas is not None, verts_grad
        ctx.outs = (want_verts, want_kp)
        ctx.save_for_backward(p, out["rotmats"], bt)
        ctx.set_materialize_grads(False)
        joints = out["joints"].view(B, hi - lo, J, 3)
        verts = out["vertices"].view(B, hi - lo, head.body.NV, 3) if want_verts else None
        kp = (out["keypoints"].view(B, hi - lo, head.body.NK, 3),) if want_kp else ()
        return (pose, lp.view(B, K), joints) + ((verts,) if want_verts else ()) + kp

    @staticmethod
    def backward(ctx, g_pose, g_lp, g_joints, *g_rest):
        want_verts, want_kp = ctx.outs
        gk = g_rest[-1] if want_kp else None
        g_verts = g_rest[:1] if want_verts else ()
        gv = g_verts[0] if g_verts and g_verts[0] is not None and bool(g_verts[0].ne(0).any()) else None
        if gv is not None and not ctx.verts_grad:
            raise NotImplementedError("BodyFlowHead: no reverse pass through the vertex skinning by default - a loss on 'vertices' cannot be "
                                      "differentiated (use 'joints' / 'pose6d', or pass verts_grad=True)")
        head, (B, K, lo, hi) = ctx.head, ctx.shape
        p, rotmats, bt = ctx.saved_tensors
        D, nb, J = head.flow.features, head.body.nb, head.body.J
        gx = torch.zeros(B, K, D, device=p.device) if g_pose is None else g_pose.float().contiguous().clone()
        g_betas = None
        if g_joints is not None or gv is not None or gk is not None:
            n = hi - lo
            gj = None if g_joints is None else g_joints.float().reshape(B * n, J, 3).contiguous()
            if gv is None and gk is None:
                g_rot, g_bt = lbs_pose_bwd(head.body, rotmats, bt, gj)
            else:          # a keypoint gradient takes the skinning reverse whatever verts_grad says (its vertex-gradient buffer is lbs_bwd's own)
                g_rot, g_bt = lbs_bwd(head.body, rotmats, bt, None if gv is None else gv.float().reshape(B * n, head.body.NV, 3).contiguous(), gj,
                                      g_keypoints=None if gk is None else gk.float().reshape(B * n, head.body.NK, 3).contiguous())
            g6 = rot6d_to_rotmat_bwd(p.view(B * n, J, 6), g_rot)
            gx[:, lo:hi] += g6.view(B, n, D)
            if ctx.has_betas and ctx.needs_input_grad[2]:
                g_betas = ops.sum_row_blocks(g_bt, B, n)
        elif ctx.has_betas and ctx.needs_input_grad[2]:
            g_betas = torch.zeros(B, nb, device=p.device)
        glp = None if g_lp is None else g_lp.float().reshape(B * K).contiguous()
        grads, g_feats = _flow_backward(head.flow, ctx.tape, gx.view(B * K, D), glp)
        ctx.tape = None
        params = list(head.flow.parameters())
        return (None, g_feats if ctx.needs_input_grad[1] else None, g_betas, None, None, None, None, None, None, None) + tuple(grads.get(q) for q in params)


class _KpLogProbFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, keypoints, cam, uv, vis, b):
        B, K, NK = keypoints.shape[:3]
        log_p = torch.empty(B, K, device=keypoints.device, dtype=torch.float32)
        ops.launch("mhe_kp_log_prob_f32", keypoints, cam, uv, vis, log_p, B, K, NK, int(cam.dim() == 3), b)
        ctx.save_for_backward(keypoints, cam, uv, vis)
        ctx.b = b
        return log_p

    @staticmethod
    def backward(ctx, g):
        keypoints, cam, uv, vis = ctx.saved_tensors
        B, K, NK = keypoints.shape[:3]
        g = g.float().contiguous()
        g_kp, g_cam = torch.empty_like(keypoints), torch.empty_like(cam)
        ops.launch("mhe_kp_log_prob_bwd_f32", keypoints, cam, uv, vis, g, g_kp, g_cam, B, K, NK, int(cam.dim() == 3), ctx.b)
        return g_kp, g_cam, None, None, None


def keypoint_log_prob(keypoints, cam, uv, vis, b=0.03):
    """log-likelihood of annotated 2D keypoints under each hypothesis (the data term of the reference's loss, hand/network.py:233-258 on the
    orthographic projection of hand/ManoLayer.py:150-165, inv_norm=False): keypoints (B,K,NK,3), cam (B,K,3) or (B,3) = (s, tx, ty), uv (B,NK,2),
    vis (B,NK) -> (B,K):  proj = s * keypoints[..., :2] + t;  sum over NK x 2 of [vis == 1] * (-(relu(|uv - proj| - 1e-4) + 1e-4) / b - log(2 b)).
    One autograd node (mhe_kp_log_prob_f32 / mhe_kp_log_prob_bwd_f32): gradients to keypoints (z column 0) and cam; uv, vis and b are constants.
    b = 0.03 is the reference's shipped value (ho3d.yaml:44).  ProHMR's own perspective camera is out of tree: unpinned, not this function."""
    if not isinstance(keypoints, torch.Tensor) or keypoints.dim() != 4 or keypoints.shape[-1] != 3:
        raise ValueError("keypoint_log_prob: keypoints must be a (B, K, NK, 3) tensor")
    B, K, NK = keypoints.shape[:3]
    if not 1 <= NK <= 64:
        raise ValueError(f"keypoint_log_prob: NK={NK} outside 1..64")
    if not isinstance(cam, torch.Tensor) or tuple(cam.shape) not in ((B, K, 3), (B, 3)):
        raise ValueError(f"keypoint_log_prob: cam must be ({B}, {K}, 3) or ({B}, 3), got {tuple(getattr(cam, 'shape', ()))}")
    if not float(b) > 0.0:
        raise ValueError("keypoint_log_prob: b must be positive")
    keypoints, cam = keypoints.contiguous(), cam.contiguous()
    ops._chk(keypoints, torch.float32, "keypoint_log_prob.keypoints", (B, K, NK, 3)); ops._chk(cam, torch.float32, "keypoint_log_prob.cam")
    ops._chk(uv, torch.float32, "keypoint_log_prob.uv", (B, NK, 2)); ops._chk(vis, torch.float32, "keypoint_log_prob.vis", (B, NK))
    return _KpLogProbFn.apply(keypoints, cam, uv, vis, float(b))
