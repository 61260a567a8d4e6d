"""MHEnt - image encoder -> K pose/shape hypotheses with log-probability -> MANO
joints -> entropy + 2D re-projection ELBO - with the reference's module API
(reference hand/network.py: `BasicEnc` :27-140, `MHEnt` :309-887) on HIP kernels.

Kept from the reference: constructor (`MHEnt(special_cfg, **common_cfg)`), child
module names (feat_extractor, q_z_giv_i, mano_dec, det_head -> identical
state_dict keys), `get_loss` / `log_prob` / `sample` / `training_step_start`
signatures and the keys + shapes of the dicts they return.
Extensions (all optional, defaults reproduce the reference):
  * `N=` hypotheses per image for the loss (the reference hard-codes 10, :780),
  * `noise=` host-supplied base noise for reproducible parity,
  * `fused_entropy=True`: log q from the sampling pass instead of a second,
    inverse pass through the flow (same value to fp32 round-off, SURVEY.md A2 ii);
    set False to run the reference's two-pass form,
  * `chamfer_w=` / the attribute `MHEnt.chamfer_w` (0.0): the weight of the hand-object Chamfer term the reference has behind a literal
    `use_chamfer_loss = False` (hand/network.py:821-826, its w_chamfer = 10): log_p -= chamfer_w * chamfer, new key 'chamfer' (B,) in mm.
  * `sil_w=` / the attribute `MHEnt.sil_w` (0.0): the weight of the silhouette term the reference only prepared for (`mask_sz=64`,
    hand/network.py:363; its renderer is commented out): log_p -= sil_w * silhouette, new key 'silhouette' (B,), the mean over the hypotheses
    of criteria.silhouette_dist of the mesh against y['hand_mask'] at grid size `MHEnt.sil_size` (64).
  * `sil_occluder=` / the attribute `MHEnt.sil_occluder` (False): the silhouette term with y['object_mask'] as criteria.silhouette_dist's
    occluder - the object the hand holds excuses the vertices behind it and attracts nothing.
The `q_z_giv_i_model='glow'` branch (hand/network.py:342-344,736-742) runs on mhentropy_amd/glow.py's ConditionalGlow - a
restatement of the published nflows algorithm, parity UNPINNED (the third-party class is absent from the reference tree).
Dead reference branches (VAE prior, GT evidences) raise NotImplementedError.  The renderer (hand/network.py:528-558, whose third-party
rasteriser the reference has commented out) is ops.render_mesh: `sample(mods=[..., 'm', 'depth'])` adds mask / depth, forward only.
"""
from typing import Union

import numpy as np
import torch
from torch import nn

from . import ops, resnet
from .ManoLayer import ManoLayer
from .flows import RealNVP
from .glow import ConditionalGlow
from .loss_terms import LossTerms


class BasicEnc(nn.Module):
    """reference hand/network.py:27-140: ResNet trunk + two Linear heads; returns (z, mn, sd) with sd = exp(l2 / 2) (or
    sigmoid, `sigma_act`) and z = mn + sd * eps, eps ~ N(0, I) (z = mn when deterministic) - `full_outputs=True`, the default
    of the stand-alone class.  MHEnt consumes only `mn` (:779,862); l2 / exp / the epsilon draw are dead for it, so it
    builds its encoder with `full_outputs=False` (-> (mn, mn, None), no l2 product, no draw).  `eps=` supplies the noise for
    reproducible runs; otherwise it is drawn on the device (ops.randn) - a device generator cannot follow the reference's CPU stream."""
    def __init__(self, cfg=None, n_latent: Union[int, list] = 64, backbone="resnet18", pretrained=True,
                 conditional_p=False, K=21, D=3, feat_dim=None, sigma_act="exp", deterministic=False,
                 compute_dtype=torch.float32, full_outputs=True, **kwargs):
        super().__init__()
        if conditional_p:
            raise NotImplementedError("conditional_p is deprecated in the reference (network.py:63)")
        self.n_latent = [n_latent, n_latent] if isinstance(n_latent, int) else list(n_latent)
        if backbone not in resnet.CFG:
            raise NotImplementedError(backbone)
        self.res = resnet.ResNetTrunk(backbone, compute_dtype=compute_dtype)      # random init: no network for pretrained weights
        feat_dim = feat_dim or resnet.CFG[backbone][2]
        self.l1 = nn.Sequential(nn.Linear(feat_dim, self.n_latent[0]))
        self.l2 = nn.Sequential(nn.Linear(feat_dim, self.n_latent[1]))
        if sigma_act not in ("exp", "sigmoid"):
            raise NotImplementedError(f"sigma_act={sigma_act!r}")
        self.sigma_act, self.deterministic, self.full_outputs = sigma_act, deterministic, full_outputs
        self._feat = None

    def forward(self, x, deterministic=False, p=None, eps=None):
        f = self.res(x)
        self._feat = f
        # bf16 mode: the same launch also leaves mn as the bf16 operand of the flow's conditioning product (read by RealNVP._cond_table)
        mn = ops.linear(f, self.l1[0].weight.detach(), self.l1[0].bias.detach(), want_bf16=self.res.compute_dtype == torch.bfloat16)
        if isinstance(mn, tuple):
            mn, mnb = mn
            if mnb is not None:
                mn._mhe_bf16 = mnb
        if not self.full_outputs:
            return mn, mn, None
        l2 = ops.linear(f, self.l2[0].weight.detach(), self.l2[0].bias.detach())
        if mn.shape != l2.shape:
            # list-valued n_latent: the reference returns z = mn with sd in l2's OWN shape (hand/network.py:133-136); the fused launch
            # wants one shape, so sd comes from a deterministic launch on l2 alone (its z output, a copy of l2, is dropped)
            sd, _ = ops.reparam(l2, l2, None, sigmoid_act=self.sigma_act == "sigmoid", deterministic=True)
            return mn, mn, sd
        det = bool(self.deterministic or deterministic)      # hand/network.py:133-136
        if not det and eps is None:
            eps = ops.randn(mn.shape[0], mn.shape[1], mn.device)
        sd, z = ops.reparam(mn, l2, None if det else eps.contiguous(), sigmoid_act=self.sigma_act == "sigmoid", deterministic=det)
        return z, mn, sd


class MHEnt(nn.Module):
    def __init__(self, special_cfg, **common_cfg):
        super().__init__()
        self.integrated = True
        if common_cfg["input"] != "image":
            raise NotImplementedError
        self.feat_extractor = BasicEnc(**dict(common_cfg, full_outputs=False))      # only mn is consumed (hand/network.py:779,862)
        model = special_cfg["q_z_giv_i_model"]
        if model == "realnvp":
            self.q_z_giv_i = RealNVP(**special_cfg["q_z_giv_i_cfg"])
        elif model == "glow":       # reference hand/network.py:342-344; parity unpinned (third-party class absent, see glow.py)
            self.q_z_giv_i = ConditionalGlow(45, 512, 4, 2, context_features=512, dropout_probability=0.2)
        else:
            raise NotImplementedError(f"q_z_giv_i_model={model!r}")
        self.ds = special_cfg["ds"]
        if self.ds not in ("rhd", "ho3d"):
            raise NotImplementedError(self.ds)
        self.image_size = max(special_cfg["image_size"])
        mano_cfg = special_cfg["mano_cfg"]
        self.mano_dec = ManoLayer(skeidx="RHD", flat_hand_mean=mano_cfg["flat_hand_mean"], ncomps=mano_cfg["ncomps"],
                                  use_pca=mano_cfg["use_pca"], output_size=self.image_size, mask_sz=64,
                                  tables=mano_cfg.get("tables"),
                                  **({"MANO_dir": mano_cfg["MANO_dir"]} if "MANO_dir" in mano_cfg else {}))
        self.zdims = {"th3": 3, "th45": 45, "bt": 10, "logs": 1, "t": 2}
        self.zdets = {"th3": True, "th45": False, "bt": True, "logs": True, "t": True}
        self.z_dim = 45
        feat_dim = 512
        self.det_head = nn.Sequential(nn.Linear(feat_dim, feat_dim), nn.ReLU(inplace=True), nn.Linear(feat_dim, 16))
        self.b_2d = float(special_cfg["data_prior_cfg"]["b_2d"])                   # network.py:392
        self.b_3d = 0.03                        # network.py:393 (constant, independent of b_2d)
        prior_cfg = special_cfg["prior_cfg"]
        if prior_cfg.get("p_theta45_pth"):
            raise NotImplementedError("VAE4Pose prior is undefined in the reference (network.py:423)")
        self.th45_ref_alpha = float(prior_cfg.get("th45_ref_alpha", 50.0))       # network.py:427
        self.kld_w = self.kld_w_final = special_cfg.get("kld_w", 1.0)
        self.kld_w_annealing = special_cfg["kld_w_annealing"]
        self.T = special_cfg.get("T", 1.0)
        if self.T != 1.0:
            raise NotImplementedError("T != 1")
        self.entropy = special_cfg["loss_cfg"]["entropy"]
        self.best_mode = special_cfg["loss_cfg"]["mode"]
        self._extra_ws = {"log_p_vis_giv_z": 1.0}
        self.loss_N = 10                        # network.py:780
        self.fused_entropy = True
        self.chamfer_w = 0.0                    # network.py:821-826: use_chamfer_loss = False as shipped; its w_chamfer is 10
        self.sil_w = 0.0                        # the silhouette term (no reference counterpart: its renderer is commented out)
        self.sil_size = 64                      # network.py:363: mask_sz
        self.sil_occluder = False               # the silhouette term reads y['object_mask'] as its occluder

    # ---- pieces ---------------------------------------------------------------
    def _det(self, feat):
        """det_head (network.py:380-383) on the B image rows."""
        h = ops.linear(feat, self.det_head[0].weight.detach(), self.det_head[0].bias.detach(), relu=True)
        return ops.linear(h, self.det_head[2].weight.detach(), self.det_head[2].bias.detach())

    def _noise(self, rows, temp, noise, device):
        """z0 = prior.sample((N*B,)) * temp (hand/flows.py:339, hand/network.py:733-735): drawn on the device inside the step unless the
        caller supplies `noise` (parity runs: a device generator cannot reproduce the reference's CPU stream)"""
        if noise is None:
            return ops.randn(rows, 45, device, scale=temp)
        noise = noise.reshape(rows, 45)
        return (noise * temp).contiguous() if temp != 1.0 else noise.contiguous()

    def _glow_sample(self, feat, N, temp, noise):
        """reference hand/network.py:736-742: noise (B,N,45)*temp -> sample_and_log_prob -> rows permuted to sample-major.
        Here the flow runs directly on sample-major rows (row n*B+b uses feat[b]); a `noise` given in the reference's
        (B,N,45) layout is re-ordered, a (N*B,45) one is taken as sample-major."""
        B = feat.shape[0]
        if noise is not None and noise.dim() == 3:
            noise = noise.permute(1, 0, 2).reshape(N * B, 45)
        z0 = self._noise(N * B, temp, noise, feat.device)
        return self.q_z_giv_i._run(z0, feat.contiguous(), True, 1, B)

    def chamfer_operands(self, y, chamfer_w=None):
        """(weight, operands | None) of the hand-object Chamfer term for the target y: chamfer_w None falls back to self.chamfer_w; a weight
        of 0 is the term off (None).  The checks are criteria.chamfer_dist's, on the host, before any launch."""
        w = float(self.chamfer_w if chamfer_w is None else chamfer_w)
        if not w >= 0.0:
            raise ValueError(f"get_loss: chamfer_w={w} (>= 0)")
        if w == 0.0:
            return 0.0, None
        if "object_verts" not in y:
            raise ValueError("get_loss(chamfer_w > 0) needs the object target y['object_verts'] (B, VO*3) or (B, VO, 3)")
        from .criteria import chamfer_target_operands
        scale, root, obj, count = chamfer_target_operands(y, who="get_loss(chamfer_w)")
        return w, (scale.float(), root.float(), obj.float(), count)

    def sil_operands(self, y, sil_w=None, B=None, sil_occluder=None):
        """(weight, (pixels, count) | None) of the silhouette term for the target y: sil_w None falls back to self.sil_w; a weight of 0 is
        the term off (None, nothing launched).  y['hand_mask'] (B, H, H) (B None: whatever the mask has) bool / uint8 / float32 with H a multiple of self.sil_size; the shape
        checks are criteria.silhouette_dist's, on the host, before any launch; the kept-pixel list (ops.silhouette_pixels) is the one launch.
        sil_occluder (None: self.sil_occluder) on and the weight > 0: y['object_mask'] (B, H, H) like the mask is the occluder, its kept pixels
        follow the hand's in the list, and the result is (weight, (pixels, count), count_all) as ops.silhouette_pixels(occluder=...) has it."""
        w = float(self.sil_w if sil_w is None else sil_w)
        if not w >= 0.0:
            raise ValueError(f"get_loss: sil_w={w} (>= 0)")
        if w == 0.0:
            return 0.0, None
        if "hand_mask" not in y:
            raise ValueError("get_loss(sil_w > 0) needs the mask target y['hand_mask'] (B, H, H)")
        from .criteria import silhouette_mask_checks
        mask = y["hand_mask"]
        silhouette_mask_checks(mask, B, int(self.sil_size), who="get_loss(sil_w)")
        if mask.dtype not in (torch.bool, torch.uint8, torch.float32):
            raise ValueError(f"get_loss(sil_w): y['hand_mask'] must be bool, uint8 or float32, got {mask.dtype}")
        if not (self.sil_occluder if sil_occluder is None else sil_occluder):
            return w, ops.silhouette_pixels(mask.contiguous(), int(self.sil_size))
        if "object_mask" not in y:
            raise ValueError("get_loss(sil_w > 0, sil_occluder) needs the occluder target y['object_mask'] (B, H, H)")
        from .criteria import silhouette_occluder_checks
        occ = silhouette_occluder_checks(y["object_mask"], mask, who="get_loss(sil_occluder)")
        pixels, count, count_all = ops.silhouette_pixels(mask.contiguous(), int(self.sil_size), occ)
        return w, (pixels, count), count_all

    def silhouette_rows(self, z, sil, N, B, count_all=None):
        """the silhouette term's forward on the loss pass' z [N*B,61]: the normalised mesh (ops.mano_verts), its distance to the kept pixels
        sil = (pixels, count) - with count_all, the occluder section behind them too - without index tensors, the mean over the hypotheses
        -> (verts [N*B,778,3], logs_t [N*B,3], silhouette [B])"""
        if sil[0].shape[0] != B:
            raise ValueError(f"get_loss(sil_w): y['hand_mask'] has {sil[0].shape[0]} images, the batch {B}")
        verts = ops.mano_verts(z, self.mano_dec.table_blob())
        logs_t = z[:, 58:61].contiguous()
        dist, _ = ops.silhouette_dist(verts.view(N, B, 778, 3), logs_t.view(N, B, 3), *sil, count_all=count_all)
        return verts, logs_t, ops.elbo_reduce(dist.view(N * B), None, N, B)[0]

    # ---- reference surface ------------------------------------------------------
    def _reverse_kld(self, y, x, mods=None, return_dict=True, N=None, noise=None, chamfer_w=None, sil_w=None, sil_occluder=None):
        """reference hand/network.py:760-831.  mods: ['uv'] (None; weak supervision), ['xyz'] or ['xyz', 'uv'] (3D supervision,
        hand/CrossModalHand.py:354: adds the Laplace likelihood of the normalised joints against y['pose3d'], network.py:620-643).
        chamfer_w (None: self.chamfer_w) > 0: the Chamfer term of network.py:821-826 for N hypotheses - out['chamfer'][b] = mean_n of
        criteria.chamfer_dist of row n*B+b's joints against y['object_verts'] (y['object_count'], 'scale', 'original_pose3d'), and
        log_p -= chamfer_w * chamfer; the other keys are not touched by it.
        sil_w (None: self.sil_w) > 0: the silhouette term - out['silhouette'][b] = mean_n of criteria.silhouette_dist of row n*B+b's normalised
        mesh (ops.mano_verts(z), the 'verts' of sample()) under logs_t = z[:, 58:61] against y['hand_mask'][b] at grid size self.sil_size, and
        log_p -= sil_w * silhouette; the other keys are not touched by it.  Both terms may be on.
        sil_occluder (None: self.sil_occluder): the silhouette term takes y['object_mask'] as its occluder (criteria.silhouette_dist's)."""
        N = N or self.loss_N
        tr = getattr(self, "_trainer", None)
        if tr is not None and self.training and torch.is_grad_enabled():
            # a train.TrainStep is attached: the loss dict comes out as ONE autograd node whose backward is the
            # hand-written reverse pass, so the reference's `total_loss.backward()` works unchanged
            from .train import differentiable_get_loss
            return differentiable_get_loss(tr, x, y, N=N, noise=noise, mods=mods, chamfer_w=chamfer_w, sil_w=sil_w, sil_occluder=sil_occluder)
        # every host check, then the kept-pixel launch
        terms = LossTerms(self, y, mods, chamfer_w, sil_w, None if x is None else x.shape[0], sil_occluder=sil_occluder)
        _, feat, _ = self.feat_extractor(x)
        B = feat.shape[0]
        if isinstance(self.q_z_giv_i, ConditionalGlow):      # entropy from the sampling pass itself (network.py:781-783,798-799)
            th45, log_q = self._glow_sample(feat, N, 1.0, noise)
        elif self.entropy and self.fused_entropy:
            z0 = self._noise(N * B, 1.0, noise, feat.device)
            th45, log_q = self.q_z_giv_i.sample_with_log_prob(z0, feat)
        else:
            z0 = self._noise(N * B, 1.0, noise, feat.device)
            th45 = self.q_z_giv_i.forward_p(z0, cond=feat)
            log_q = self.q_z_giv_i.log_prob(th45, logvar=feat) if self.entropy else None       # network.py:801
        out = terms.reduce(terms.joints(th45, self._det(feat), self.mano_dec.table_blob()), log_q, N, B)
        if not return_dict:
            raise NotImplementedError
        return out

    def log_prob(self, y, x, div_type=0, mods=None, return_dict=True, **kw):
        return self._reverse_kld(y, x, mods=mods, return_dict=return_dict, **kw)

    def get_loss(self, x, y, div_type=0, mods=None, return_dict=True, **kw):
        """reference hand/network.py:838-844."""
        return self.log_prob(y, x, div_type=div_type, mods=mods, return_dict=return_dict, **kw)

    def sample(self, x, N: Union[int, list] = 5, temp=0.5, mods=None, y=None, noise=None, feat=None, quant="log_q", quant_iters=10):
        """reference hand/network.py:846-883 -> th_bt (N,B,58), logs_t (N,B,3), verts (N,B,2334),
        xyz (N,B,63), uv (N,B,42) in pixels, faces.  mods may also hold 'm' and / or 'depth' (hand/network.py:541-558): mask / depth
        (N,B,64,64) of every hypothesis' mesh through ManoLayer.render - camera exp(logs_t[0]), logs_t[1:], depth scaled by the normaliser
        |J11 - J12| of the un-normalised joints.  The default mods (None) returns what it always did.
        quant: how N = [M, n] with n < M cuts the M hypotheses drawn to n.  'log_q' (default) is the reference's: the n most likely.
        'kmeans' is the n-quantised-best-of-M protocol: the M hypotheses' normalised root-relative joints (a joints-only decode) are
        clustered into n modes (ops.kmeans_select, seeded by log q, at most quant_iters Lloyd rounds), the member nearest each mode's mean
        is kept and decoded, largest mode first; the result gains quant_index (n, B) int64, the hypotheses kept, and quant_count (n, B)
        int64, the sizes of their modes.  With N an int or n == M it is ignored, as N_quant is."""
        N_quant = N
        if isinstance(N, (list, tuple)):
            N, N_quant = N
        if quant not in ("log_q", "kmeans"):
            raise ValueError(f"sample: quant={quant!r} (log_q or kmeans)")
        out = {}
        if y is not None and "image" in y:
            out["image"] = y["image"]
        if feat is None:       # `feat=` (extension): the conditioning feature of a forward already run on x
            _, feat, _ = self.feat_extractor(x)
        B = feat.shape[0]
        if isinstance(self.q_z_giv_i, ConditionalGlow):
            th45, log_q = self._glow_sample(feat, N, temp, noise)
        else:                   # log q comes from the sampling pass itself (only needed for the top-k selection)
            z0 = self._noise(N * B, temp, noise, feat.device)
            if N_quant < N:
                th45, log_q = self.q_z_giv_i.sample_with_log_prob(z0, feat)
            else:
                th45 = self.q_z_giv_i.forward_p(z0, cond=feat)
        if N_quant < N and quant == "kmeans":       # keep one representative of each of N_quant modes per image
            xyz = ops.mano_joints(th45, self._det(feat), self.mano_dec.table_blob(), inv_norm=True, image_size=float(self.image_size),
                                  want=("xyz",))["xyz"]
            km = ops.kmeans_select(xyz.view(N, B, 63), N_quant, score=log_q.view(N, B), iters=quant_iters)
            th45 = th45.view(N, B, 45)[km["index"], torch.arange(B, device=th45.device)].reshape(N_quant * B, 45)
            out["quant_index"], out["quant_count"] = km["index"], km["count"].long()
            N = N_quant
        elif N_quant < N:       # keep the N_quant most likely hypotheses per image (network.py:866-871)
            _, th45 = ops.topk_gather(log_q, th45, N, B, N_quant)
            N = N_quant
        mods = {"xyz", "uv", "verts"} if mods is None else set(mods)
        render = [k for m, k in (("m", "mask"), ("depth", "depth")) if m in mods]
        blob = self.mano_dec.table_blob()
        o = ops.mano_joints(th45, self._det(feat), blob, inv_norm=True, image_size=float(self.image_size),
                            want=("z", "xyz", "uv") + (("verts",) if "verts" in mods or render else ()) +      # the mesh from the joint pass' operands
                            (("joints_mm",) if render else ()))
        z = o["z"].view(N, B, 61)
        out["th_bt"], out["logs_t"] = z[..., :58], z[..., -3:]
        if "verts" in mods:
            out["verts"] = o["verts"].view(N, B, -1)
            out["faces"] = self.mano_dec.mano_faces
        if "xyz" in mods:
            out["xyz"] = o["xyz"].view(N, B, -1)
        if "uv" in mods:
            out["uv"] = o["uv"].view(N, B, -1)
        if render:
            J = o["joints_mm"].view(N * B, 21, 3)
            logs_t = o["z"][:, -3:]
            img = self.mano_dec.render(logs_t[:, :1].exp(), logs_t[:, 1:].contiguous(), vertex=o["verts"], norm=(J[:, 11] - J[:, 12]).norm(dim=-1),
                                       render=render)
            for k, v in img.items():
                out[k] = v.view(N, B, *v.shape[1:])
        return out

    def training_step_start(self, step):
        """reference hand/network.py:885-887."""
        kld_w_init, kld_w_steps = self.kld_w_annealing
        self.kld_w = kld_w_init + (self.kld_w_final - kld_w_init) * min(1.0, step / kld_w_steps)
