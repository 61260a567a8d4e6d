"""The optional terms of the hand loss for ONE call of it - get_loss(mods=, chamfer_w=, sil_w=, sil_occluder=) - as one object: MHEnt._reverse_kld and
train.TrainStep build it, ask it for the loss pass, its reverse and the result dictionary, and TrainStep keeps it on its tape.  A new
term is added here (and in the kernels), not in the layers between."""
from . import ops


class LossTerms:
    def __init__(self, model, y, mods=None, chamfer_w=None, sil_w=None, B=None, who="get_loss", sharded=False, pixels=True, sil_occluder=None):
        """every host check of the call, before any launch: the likelihood bit set (mods: get_loss's names or the bits themselves), the
        Chamfer weight and operands (MHEnt.chamfer_operands), the silhouette weight and - pixels=True, the one launch here - the kept pixels
        of y['hand_mask'] for B images (MHEnt.sil_operands) - with sil_occluder (None: the model's) those of y['object_mask'] behind them,
        and sil_all, the length of both sections.  sharded: the hypothesis-sharded step, which has no silhouette term."""
        self.model, self.y = model, y
        self.bits = mods if isinstance(mods, int) else ops.mods_bits(mods)
        if self.bits & ops.MODS_XYZ and "pose3d" not in y:
            raise ValueError(f"{who}(mods=[..., 'xyz']) needs the 3D target y['pose3d'] (B, 63)")
        self.chamfer_w, self.chamfer = model.chamfer_operands(y, chamfer_w)
        self.sil_w, self.sil, self.sil_all = float(model.sil_w if sil_w is None else sil_w), None, None
        self.sil_occluder = bool(model.sil_occluder if sil_occluder is None else sil_occluder) and self.sil_w > 0
        if sharded and self.sil_w > 0:
            raise NotImplementedError("hypothesis sharding with sil_w > 0: the masks of the other ranks' images are not gathered")
        if pixels:
            self.sil_w, self.sil, *rest = model.sil_operands(y, self.sil_w, B, self.sil_occluder)
            self.sil_all = rest[0] if rest else None
        self._pass = None

    def weights(self):
        """the call's arguments, checked and with the model's defaults filled in; 'sil_occluder' is carried when the occluder is on (the
        silhouette term on, too): a call without it is the call it was before the argument existed"""
        w = {"mods": self.bits, "chamfer_w": self.chamfer_w, "sil_w": self.sil_w}
        if self.sil_occluder:
            w["sil_occluder"] = True
        return w

    def keys(self):
        """the keys of reduce()'s dictionary, in its order"""
        return (["th_norm", "bt_norm", "q_log_p_z_giv_y", "log_p"] + ["h_q_z_giv_i"] * bool(self.model.entropy) + ["chamfer"] * (self.chamfer_w > 0)
                + ["silhouette"] * (self.sil_w > 0))

    def gather(self, hs):
        """hypothesis sharding (dist.HypothesisShards): the targets and Chamfer operands of every rank's images, rank-major like the features"""
        self.y = {k: hs.gather_rows(self.y[k]) for k in ("crop_uv", "vis") + (("pose3d",) if self.bits & ops.MODS_XYZ else ())}
        if self.chamfer is not None:
            self.chamfer = tuple(None if t is None else hs.gather_rows(t) for t in self.chamfer)

    def _args(self):
        """what ops.mano_joints and ops.mano_joints_bwd share: the targets the bit set reads, the model's constants, and the entry - Chamfer
        operands: the chamfer one; else uv alone: the 4-term one (mods None at the ops level); else the one with the bit set"""
        if self._pass is None:
            y, m, uv, xyz = self.y, self.model, self.bits & ops.MODS_UV, self.bits & ops.MODS_XYZ
            self._pass = dict(crop_uv=y["crop_uv"].contiguous() if uv else None, vis=y["vis"].contiguous(), laplace_b=m.b_2d, th45_alpha=m.th45_ref_alpha,
                              pose3d=y["pose3d"].contiguous().float() if xyz else None, laplace_b_3d=m.b_3d, chamfer=self.chamfer,
                              mods=None if self.chamfer is None and self.bits == ops.MODS_UV else self.bits)
        return self._pass

    def joints(self, th45, det, blob, want=("log_p", "norms")):
        """the loss pass (ops.mano_joints) with this call's terms; the silhouette term only adds z to `want`"""
        return ops.mano_joints(th45, det, blob, want=tuple(want) + (("z",) if self.sil is not None else ()), **self._args())

    def joints_bwd(self, th45, det, blob, g_log_p, N, out=None):
        """its reverse (the Chamfer term's included): ops.mano_joints_bwd, or with out = (g_th45, g_rows) into those, d/d det unsummed"""
        if out is None:
            return ops.mano_joints_bwd(th45, det, blob, g_log_p=g_log_p, N=N, chamfer_w=self.chamfer_w, **self._args())
        return ops.mano_joints_bwd_rows(th45, det, blob, g_log_p=g_log_p, N=N, g_th45=out[0], g_rows=out[1], chamfer_w=self.chamfer_w, **self._args())

    def reduce(self, o, log_q, N, B, share=None):
        """the loss pass' outputs o and log q (None: no entropy term) -> get_loss's dictionary: means over the N hypotheses, the Chamfer and
        silhouette means with log_p -= weight * term.  share (hypothesis sharding) maps the local (q_log_p, h, chamfer | None) to the
        means over every rank's hypotheses, for this rank's images."""
        q_log_p, h, log_p = ops.elbo_reduce(o["log_p"], log_q, N, B)
        ch = ops.elbo_reduce(o["chamfer"], None, N, B)[0] if self.chamfer is not None else None
        # mesh of the loss pass' z, its distance without index tensors, mean over the hypotheses; the mesh is kept for the reverse
        self.sil_verts, self.sil_logs_t, sl = self.model.silhouette_rows(o["z"], self.sil, N, B, self.sil_all) if self.sil is not None else (None, None, None)
        if share is not None:
            q_log_p, h, ch = share(q_log_p, h, ch)
            log_p = h + q_log_p
        log_p = log_p if self.model.entropy else q_log_p
        if ch is not None:
            log_p = log_p - self.chamfer_w * ch
        if sl is not None:
            log_p = log_p - self.sil_w * sl
        vals = {"th_norm": o["norms"][:, 0], "bt_norm": o["norms"][:, 1], "q_log_p_z_giv_y": q_log_p, "log_p": log_p, "h_q_z_giv_i": h, "chamfer": ch,
                "silhouette": sl}
        return {k: vals[k] for k in self.keys()}
