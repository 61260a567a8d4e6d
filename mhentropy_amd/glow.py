"""ConditionalGlow with the call surface the reference uses for `q_z_giv_i_model == 'glow'`
(reference hand/network.py:342-344 ctor `(45, 512, 4, 2, context_features=512, dropout_probability=0.2)`;
:693-694 `log_prob(z, context=feat) -> (log_prob, z)`; :736-742 `sample_and_log_prob(N, noise, context)
-> (samples (B,N,D), log_prob (B,N), z)`; `_distribution._shape`), on HIP kernels.

**PARITY UNPINNED.**  The reference imports the class from the ProHMR fork of nflows
(`git+https://github.com/nkolot/nflows.git`, unpinned, hand/environment.yml:284), which is neither vendored
nor installed; no reference test or fixture covers it.  This module follows the published nflows algorithm as
restated in oracle/glow_ref.py (per layer ActNorm -> LULinear -> AffineCouplingTransform whose scale/shift come
from a context-conditioned ResidualNet with GLU gating; alternating +-1 mask; StandardNormal base) and keeps
nflows' module tree so that its state_dict keys (`_transform._transforms.{i}...`) line up.  Dropout (p = 0.2 in the reference's
constructor call) is active in train mode as in the reference - masks drawn on the device (mhe_dropout; the reference's draws come from
torch's generator and cannot be reproduced, so parity tests record the masks and hand them to the oracle) - and the identity in eval mode;
batch norm inside the nets is off (nflows' default).

MI355X shape of the computation: ActNorm and the LU product collapse into one 45x45 affine map per layer (and its
inverse for sampling), the flow variable is carried zero-padded to 64 columns so every dense product is an
mhe_linear_f32 call, and everything that depends on the context only (initial-layer context columns, the GLU
gates of every block of every layer) is ONE GEMM per image, indexed per hypothesis row by the kernels.

Both directions are differentiable in f32: the sampling direction (noise -> pose; `_run(inverse=True, tape=)` + `_reverse`, driven by the train
step and by body.BodyFlowHead) and the density direction (pose -> noise; `log_prob` under grad = `_LogProbFn`: `_run(inverse=False, tape=)` +
`_reverse_density`, the maximum-likelihood loss of the reference's README.md:32-34).  The residual net's reverse (`_net_reverse`) is one piece
of code for the two.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import ops


def _colsum(rows, B, N, out):
    """out = column sums of batch-major rows [B N, C] in a fixed order - per image, then over images (ops.colsum takes C | 256 or C >= 256;
    the body flow's variable and coupling parameters are 192 wide)"""
    ops.sum_row_blocks(ops.sum_row_blocks(rows, B, N), 1, B, out=out.view(1, -1))


class _ActNorm(nn.Module):
    def __init__(self, features):
        super().__init__()
        self.register_buffer("initialized", torch.tensor(True))
        self.log_scale = nn.Parameter(torch.zeros(features))
        self.shift = nn.Parameter(torch.zeros(features))


class _LULinear(nn.Module):
    def __init__(self, features, eps=1e-3):
        super().__init__()
        self.features, self.eps = features, eps
        n = features * (features - 1) // 2
        self.lower_entries = nn.Parameter(torch.zeros(n))
        self.upper_entries = nn.Parameter(torch.zeros(n))
        self.unconstrained_upper_diag = nn.Parameter(torch.full((features,), math.log(math.exp(1 - eps) - 1)))   # identity init
        self.bias = nn.Parameter(torch.zeros(features))


class _ResidualBlock(nn.Module):
    def __init__(self, features, context_features, dropout_probability):
        super().__init__()
        self.context_layer = nn.Linear(context_features, features)
        self.linear_layers = nn.ModuleList([nn.Linear(features, features) for _ in range(2)])
        self.dropout = nn.Dropout(p=dropout_probability)
        nn.init.uniform_(self.linear_layers[-1].weight, -1e-3, 1e-3)     # nflows zero_initialization
        nn.init.uniform_(self.linear_layers[-1].bias, -1e-3, 1e-3)


class _ResidualNet(nn.Module):
    def __init__(self, in_features, out_features, hidden_features, context_features, num_blocks, dropout_probability):
        super().__init__()
        self.initial_layer = nn.Linear(in_features + context_features, hidden_features)
        self.blocks = nn.ModuleList([_ResidualBlock(hidden_features, context_features, dropout_probability) for _ in range(num_blocks)])
        self.final_layer = nn.Linear(hidden_features, out_features)


class _AffineCoupling(nn.Module):
    def __init__(self, mask, make_net):
        super().__init__()
        idx = torch.arange(len(mask))
        self.register_buffer("identity_features", idx[mask <= 0])
        self.register_buffer("transform_features", idx[mask > 0])
        self.transform_net = make_net(int((mask <= 0).sum()), 2 * int((mask > 0).sum()))


class _Composite(nn.Module):
    def __init__(self, transforms):
        super().__init__()
        self._transforms = nn.ModuleList(transforms)


class _StandardNormal(nn.Module):
    def __init__(self, shape):
        super().__init__()
        self._shape = torch.Size(shape)
        self.register_buffer("_log_z", torch.tensor(0.5 * np.prod(shape) * np.log(2 * np.pi), dtype=torch.float64), persistent=False)


class ConditionalGlow(nn.Module):
    def __init__(self, features, hidden_features, num_layers, num_blocks_per_layer, activation=F.relu, dropout_probability=0.5,
                 context_features=None, batch_norm_within_layers=False):
        super().__init__()
        if context_features is None or batch_norm_within_layers or activation is not F.relu:
            raise NotImplementedError("only the context-conditioned, batch-norm-free ReLU configuration the reference builds")
        if features > 256 or hidden_features % 64 or context_features % 64:
            raise NotImplementedError(f"unsupported geometry features={features} hidden={hidden_features} context={context_features}")
        # the flow variable / the nets' parameter rows are carried zero-padded to multiples of 64 columns
        # (45 -> 64 for the hand flow; 144 -> 192 for a ProHMR-style 24 x 6D body pose)
        self.Dp = (features + 63) // 64 * 64
        self.features, self.hidden, self.num_layers, self.num_blocks, self.context_features = \
            features, hidden_features, num_layers, num_blocks_per_layer, context_features
        mask = torch.ones(features)
        mask[::2] = -1
        make = lambda i, o: _ResidualNet(i, o, hidden_features, context_features, num_blocks_per_layer, dropout_probability)
        layers = []
        for _ in range(num_layers):
            layers += [_ActNorm(features), _LULinear(features), _AffineCoupling(mask.clone(), make)]
            mask = -mask
        self._transform = _Composite(layers)
        self._distribution = _StandardNormal([features])
        self._embedding_net = nn.Identity()
        self._pack = None
        # train-mode dropout of the residual blocks (nflows ResidualBlock: after the second activation; hand/network.py:343-344 builds the
        # flow with dropout_probability=0.2 and trains it that way, :781 "Since uses Dropout"): masks drawn on the device (ops.dropout_).
        # mask_feed: a list of mask-bit tensors consumed in call order instead of drawing (parity tests); record_masks: the bits of every
        # dropout of a pass are appended to last_masks (handed to the oracle, which cannot draw the same stream)
        self.p_drop = float(dropout_probability)
        self.mask_feed, self.record_masks, self.last_masks = None, False, []
        # operand dtype of the four hidden x hidden products per layer (95 % of the flow's FLOP): float32 (parity mode) or
        # bfloat16 with f32 accumulate (performance mode; the train step follows it, train_glow.GlowPart)
        self.compute_dtype = torch.float32

    # ---- derived device operands, rebuilt when a parameter changes --------------------------------------
    def small_param_table(self):
        """int64 [layers, 6] device tensor: addresses of log_scale, shift, lower_entries, upper_entries, unconstrained_upper_diag, bias of
        every layer (the operand of ops.glow_affine); rebuilt when a parameter's storage moves"""
        T = self._transform._transforms
        rows = [[p.data_ptr() for p in (T[3 * l].log_scale, T[3 * l].shift, T[3 * l + 1].lower_entries, T[3 * l + 1].upper_entries,
                                        T[3 * l + 1].unconstrained_upper_diag, T[3 * l + 1].bias)] for l in range(self.num_layers)]
        key = tuple(map(tuple, rows))
        if getattr(self, "_ptab", None) is None or self._ptab[0] != key:
            self._ptab = (key, torch.tensor(rows, dtype=torch.int64, device=next(self.parameters()).device))
        return self._ptab[1]

    def _packed(self):
        ext = getattr(self, "_external_pack", None)
        if ext is not None:          # a train.TrainStep owns the parameters: its device-resident operand layouts, refreshed every step
            return ext()
        dev = next(self.parameters()).device
        ver = tuple(p._version for p in self.parameters()) + (str(dev),)
        if self._pack is not None and self._pack[0] == ver:
            return self._pack[1]
        D, H, Fc, T = self.features, self.hidden, self.context_features, self._transform._transforms
        if D <= 64:
            # ActNorm + LU of every layer as one 45x45 affine map and its inverse: one launch, float64 on the device (no host round trip)
            aff = ops.glow_affine(self.small_param_table(), self.num_layers, D, T[1].eps)
        else:
            # the wide body flow (144-D pose, padded to 192 columns): float64 on the device with a global workspace (csrc/glow_affine_wide.hip)
            aff = ops.glow_affine_wide(self.small_param_table(), self.num_layers, D, T[1].eps)
        pk = {"layers": [], "const_parts": aff["const_parts"], "aff": aff}
        wctx, bctx = [], []
        for l in range(self.num_layers):
            cp = T[3 * l + 2]
            d = {"A": aff["A"][l], "c": aff["c"][l], "Ainv": aff["Ainv"][l], "cinv": aff["cinv"][l]}
            net = cp.transform_net
            idf = cp.identity_features
            w0 = net.initial_layer.weight.detach()
            wx = torch.zeros(H, self.Dp, device=dev)
            wx[:, idf.to(dev)] = w0[:, :idf.numel()]
            d["wx"] = wx.contiguous()
            wctx.append(w0[:, idf.numel():]); bctx.append(net.initial_layer.bias.detach())
            d["blocks"] = []
            for blk in net.blocks:
                d["blocks"].append(tuple(t.detach().contiguous() for t in (blk.linear_layers[0].weight, blk.linear_layers[0].bias,
                                                                         blk.linear_layers[1].weight, blk.linear_layers[1].bias)))
                d.setdefault("blocks_bf16", []).append((blk.linear_layers[0].weight.detach().to(torch.bfloat16).contiguous(),
                                                        blk.linear_layers[1].weight.detach().to(torch.bfloat16).contiguous()))
                wctx.append(blk.context_layer.weight.detach()); bctx.append(blk.context_layer.bias.detach())
            nt = int(cp.transform_features.numel())
            Pp = (2 * nt + 63) // 64 * 64
            wf = torch.zeros(Pp, H, device=dev); wf[:2 * nt] = net.final_layer.weight.detach()
            bf = torch.zeros(Pp, device=dev); bf[:2 * nt] = net.final_layer.bias.detach()
            d["wf"], d["bf"], d["T"], d["first"] = wf.contiguous(), bf.contiguous(), nt, 1 - (l % 2)      # (the alternating mask: odd columns first)
            pk["layers"].append(d)
        pk["wctx"], pk["bctx"] = torch.cat(wctx).contiguous(), torch.cat(bctx).contiguous()
        if H == 512 and self.num_blocks == 2 and D <= 48:
            # the one-launch kernel's operands (csrc/glow_fwd.hip): bf16 copies in MFMA fragment order, the final layer's rows at the flow
            # variable's own columns
            nets = [T[3 * l + 2].transform_net for l in range(self.num_layers)]
            st = lambda f: torch.stack([f(n) for n in nets])
            fp = ops.glow_fused_layout(torch.stack([d["wx"] for d in pk["layers"]]),
                                       st(lambda n: torch.stack([b.linear_layers[0].weight.detach() for b in n.blocks])),
                                       st(lambda n: torch.stack([b.linear_layers[1].weight.detach() for b in n.blocks])),
                                       torch.stack([d["wf"] for d in pk["layers"]]), torch.stack([d["bf"] for d in pk["layers"]]),
                                       st(lambda n: torch.stack([b.linear_layers[0].bias.detach() for b in n.blocks])),
                                       st(lambda n: torch.stack([b.linear_layers[1].bias.detach() for b in n.blocks])), D)
            pk["fused"] = {k: (v.to(torch.bfloat16) if k.endswith("F") else v.float()).contiguous() for k, v in fp.items() if not k.endswith("T")}
        self._pack = (ver, pk)
        return pk

    def _drop_bits(self, R):
        """the dropout masks of one sampling pass of the one-launch kernel: uint8 [L, 2, R * 64] (layer, block; ops.dropout_'s bit format over
        [R, hidden]) or None (eval mode / p = 0).  mask_feed / record_masks speak the layer-by-layer path's CALL ORDER - layers L-1 .. 0, blocks
        0 .. 1 - so that tests written against it feed and read the same lists"""
        if not (self.training and self.p_drop > 0.0):
            return None
        L, NB = self.num_layers, self.num_blocks
        if self.mask_feed:
            fed = [self.mask_feed.pop(0) for _ in range(L * NB)]
            bits = torch.stack([torch.stack([fed[(L - 1 - l) * NB + b].reshape(-1) for b in range(NB)]) for l in range(L)]).contiguous()
        else:
            bits = ops.dropout_bits(L * NB * R * self.hidden, self.p_drop, next(self.parameters()).device).view(L, NB, R * self.hidden // 8)
        if self.record_masks:
            self.last_masks += [bits[L - 1 - k // NB, k % NB] for k in range(L * NB)]
        return bits

    def dropout_(self, t):
        """the residual block's dropout on its second activation `t`, in place (train mode only); returns the mask bits or None"""
        if not (self.training and self.p_drop > 0.0):
            return None
        given = self.mask_feed.pop(0) if self.mask_feed else None
        bits = ops.dropout_(t, self.p_drop, bits=given)
        if self.record_masks:
            self.last_masks.append(bits)
        return bits

    # ---- the two directions ------------------------------------------------------------------------------
    def _net(self, d, v, ctab, slot, R, row_div, n_img, bf16, bufs, rec):
        """coupling parameters [R,Pp] of layer `d` from the (padded) variable v whose identity columns are current.  bufs (h, t, t2): reused
        in place, h as the residual stream; with a tape record `rec` every stage writes a fresh tensor instead, kept in rec"""
        H, cs = self.hidden, ctab.shape[1]
        fresh = rec is not None
        h = ops.linear(v, d["wx"], out=None if fresh else bufs[0])
        ops.launch("mhe_glow_add_image_rows_f32", h, ctab[:, slot * H:], cs, R, H, row_div, n_img)
        if fresh:
            rec.update(hs=[h], t2=[], t3=[], drop=[])
        elif bf16:
            t, t2 = (torch.empty(R, 1, 1, H, device=v.device, dtype=torch.bfloat16) for _ in range(2))
        else:
            t, t2 = bufs[1:]
        for b, (w0, b0, w1, b1) in enumerate(d["blocks"]):
            if fresh:
                t = torch.empty(R, 1, 1, H, device=v.device, dtype=torch.bfloat16) if bf16 else torch.empty(R, H, device=v.device)
            ops.launch("mhe_relu_copy_f32", h, t, h.numel(), ops.dtype_code(t.dtype))
            if bf16:        # relu(h) -> bf16, two h x h products on bf16 MFMA (bias + relu in the kernel's epilogue), gate in f32
                w0b, w1b = d["blocks_bf16"][b]
                t2 = ops.conv2d_nhwc(t, w0b, 1, 1, 1, 0, out_shift=b0, relu_out=True, out=None if fresh else t2)
                drop = self.dropout_(t2)
                t3 = ops.conv2d_nhwc(t2, w1b, 1, 1, 1, 0, out_shift=b1, out=None if fresh else t)
            else:
                t2 = ops.linear(t, w0, b0, relu=True, out=None if fresh else t2)
                drop = self.dropout_(t2)
                t3 = ops.linear(t2, w1, b1, out=None if fresh else t)
            if fresh:
                h = h.clone()
                rec["hs"].append(h); rec["t2"].append(t2); rec["t3"].append(t3); rec["drop"].append(drop)
            ops.launch("mhe_glow_glu_residual_f32", h, t3, ops.dtype_code(t3.dtype), ctab[:, (slot + 1 + b) * H:], cs, R, H, row_div, n_img)
        return ops.linear(h, d["wf"], d["bf"])

    def _run(self, v_in, context, inverse, row_div, n_img, pk=None, tape=None, bf16=None):
        """v_in (R,D) data (forward) or noise (inverse); returns (out (R,D), log_prob (R,)).  Row r belongs to image r // row_div % n_img.
        pk: the operand pack (default: the module's own); bf16: the block products on bf16 MFMA (default: compute_dtype is bfloat16).
        tape (a dict; either direction, layer by layer): holds the caller's "sample_major" (the row layout, which row_div alone does not tell
        at one row per image; the reverse passes pick their reductions by it) and is filled with what `_reverse` (sampling direction) or
        `_reverse_density` (density direction) reads - the pack, the context table, row_div, n_img and per layer v, the residual stream
        h_0 .. h_NB, every block's second activation t2 (after dropout), its second product t3 and dropout bits, the coupling parameters and y;
        in the density direction also u, the layer's affine input (v = A u + c)"""
        ops._chk(v_in, torch.float32, "glow.in"); ops._chk(context, torch.float32, "glow.context", (context.shape[0], self.context_features))
        pk = self._packed() if pk is None else pk
        D, H = self.features, self.hidden
        bf16 = self.compute_dtype == torch.bfloat16 if bf16 is None else bf16
        R = v_in.shape[0]
        dev = v_in.device
        ctab = ops.linear(context, pk["wctx"], pk["bctx"])                       # every context-only term, once per image
        N = R // n_img
        if (tape is None and inverse and bf16 and pk.get("fused") is not None and row_div in (1, N)
                and os.environ.get("MHE_GLOW_FUSED", "1") == "1" and ops.glow_layers_supported(N, n_img, D, H, self.num_layers, self.num_blocks)):
            # the sampling direction of all layers in ONE launch (csrc/glow_fwd.hip; bf16 operands on the products, f32 residual stream,
            # flow variable, coupling and affine map)
            rn, rb = (n_img, 1) if row_div == 1 else (1, N)
            return ops.glow_layers(v_in, ctab, pk["fused"], pk["aff"], self._drop_bits(R), self.p_drop, N, n_img, D, rn, rb)
        v = torch.empty(R, self.Dp, device=dev)
        ops.launch("mhe_pad64_f32", v_in, v, R, D)
        z_in = v
        logdet = torch.zeros(R, device=dev)
        bufs = None if tape is not None else tuple(torch.empty(R, H, device=dev) for _ in range(3))
        if tape is not None:
            tape.update(pk=pk, ctab=ctab, row_div=row_div, n_img=n_img, layers=[None] * self.num_layers)
        per = 1 + self.num_blocks
        order = range(self.num_layers - 1, -1, -1) if inverse else range(self.num_layers)
        for l in order:
            d = pk["layers"][l]
            if not inverse:
                u, v = v, ops.linear(v, d["A"], d["c"])
            rec = None if tape is None else {"v": v} if inverse else {"v": v, "u": u}
            prm = self._net(d, v, ctab, l * per, R, row_div, n_img, bf16, bufs, rec)
            y = torch.empty(R, self.Dp, device=dev)
            ops.launch("mhe_glow_coupling_f32", v, prm, y, logdet, R, D, d["first"], d["T"], int(inverse))
            if rec is not None:
                rec.update(prm=prm, y=y)
                tape["layers"][l] = rec
            v = ops.linear(y, d["Ainv"], d["cinv"]) if inverse else y
        z = z_in if inverse else v                                               # the base-density argument
        return ops.glow_finish(z, v, logdet, R, D, inverse, pk["const_parts"])

    def _reducers(self, tape, R):
        """(img_sum(rows, out), flow_colsum(rows, out)) of a tape's row layout (see `_reverse`): the per-image sums into a view of the context
        table's gradient, and the column sums of the flow-width rows"""
        B, cs = tape["n_img"], tape["ctab"].shape[1]
        N = R // B
        if not tape["sample_major"]:
            return (lambda rows, out: ops.sum_row_blocks(rows, B, N, out=out, out_stride=cs)), (lambda rows, out: _colsum(rows, B, N, out))
        img_sum = lambda rows, out: ops.sum_over_hypotheses(rows, N, B, out=out, out_stride=cs)
        if self.Dp == 64:
            return img_sum, ops.colsum
        # a wide variable (ops.colsum has no 192-column form): two levels of mhe_sum_row_blocks_f32 over g blocks of R / g consecutive rows,
        # g the largest divisor of R up to sqrt(R) - any grouping gives the column sums, this one keeps both levels short
        g = max(k for k in range(1, int(R ** 0.5) + 1) if R % k == 0)
        return img_sum, (lambda rows, out: _colsum(rows, g, R // g, out))

    def _net_reverse(self, t, o, ctab, slot, gprm, Gct, row_div, B, img_sum, flow_colsum):
        """the reverse of one layer's residual net over its tape record `t`, shared by both directions: gprm (R, Pp) = dL/d(coupling parameters) ->
        final layer; per block (last first) gate, second product, dropout, ReLU, first product, ReLU of the residual stream; initial layer's
        weight gradient and the per-image sums into Gct.  Returns gh = dL/dh_0 (R, H); the caller adds gh Wx to the variable's gradient."""
        H = self.hidden
        R, cs = gprm.shape[0], ctab.shape[1]
        dev = gprm.device
        ops.linear_wgrad(t["hs"][-1], gprm, o["dwf"]); flow_colsum(gprm, o["dbf"])
        gh = ops.linear(gprm, o["wfT"])
        for b in range(self.num_blocks - 1, -1, -1):
            (w0T, w1T), (dw0, db0, dw1, db1) = o["blocksT"][b], o["dblocks"][b]
            t2, t3, hb = t["t2"][b], t["t3"][b], t["hs"][b]
            bf16 = t3.dtype == torch.bfloat16
            gt3, ggate = torch.empty_like(t3), torch.empty(R, H, device=dev)
            ops.launch("mhe_glow_glu_bwd_f32", gh, t3, ctab[:, (slot + 1 + b) * H:], cs, gt3, ggate, R, H, row_div, B,
                       ops.dtype_code(t3.dtype))
            img_sum(ggate, Gct[:, (slot + 1 + b) * H:])
            # the four h x h products of the block's reverse pass: on bf16 MFMA over a bf16 tape (bias sums of the bf16 gradients)
            wgrad = (lambda x, gy_, dw: ops.conv_wgrad(x, gy_, 1, 1, 1, 0, dw)) if bf16 else ops.linear_wgrad
            dgrad = (lambda gy_, wT: ops.conv2d_nhwc(gy_, wT, 1, 1, 1, 0)) if bf16 else ops.linear
            wgrad(t2, gt3, dw1); ops.colsum(gt3, db1)
            gt2 = dgrad(gt3, w1T)
            if t["drop"][b] is not None:          # dropout's reverse: the same mask and scale on the gradient
                ops.dropout_(gt2, self.p_drop, bits=t["drop"][b])
            if bf16:
                ops.flow_lrelu_bwd_mixed(gt2.view(R, H), t2.view(R, H), out_bf16=gt2.view(R, H), slope=0.0)
            else:
                ops.flow_lrelu_bwd(gt2, t2, slope=0.0)
            tt = torch.empty_like(t2)
            ops.launch("mhe_relu_copy_f32", hb, tt, tt.numel(), ops.dtype_code(tt.dtype))
            wgrad(tt, gt2, dw0); ops.colsum(gt2, db0)
            gt = dgrad(gt2, w0T)
            ops.launch("mhe_relu_bwd_add_f32", gh, gt, hb, gh.numel(), ops.dtype_code(gt.dtype))
        ops.linear_wgrad(t["v"], gh, o["dwx"])
        img_sum(gh, Gct[:, slot * H:])
        return gh

    def _reverse(self, tape, gv, g_logp, Gct, layers):
        """the staged reverse pass over a `_run` tape, layers 0 .. L-1:
            dA^-1 = gv^T y, dc^-1 = sum gv;  gy = gv A^-1;  coupling reverse -> g_v, g_prm;  final layer;
            per block (last first) gate, second product, dropout, ReLU, first product, ReLU of the residual stream;  gv = g_v + gh Wx.
        gv (R, Dp) = dL/dx padded; g_logp = dL/dlog q or None; Gct (B, cs) zeroed: receives the per-image gradient of the context table.
        layers (consumed layer by layer: a generator keeps one layer's transposes alive at a time), per layer: the transposed operands AinvT,
        wfT, wxT, blocksT [(w0T, w1T) of the tape's dtype] and the gradient destinations dAinv, dcinv, dwf, dbf, dwx, dblocks [(dw0, db0, dw1,
        db1)] (the weight gradients and ops.colsum add to theirs, _colsum writes).  The reductions follow the tape's row layout:
          sample-major (the train step's entropy term): g_logp per image, weight -1/N per row (mhe_glow_coupling_inv_bwd_f32 at 64
            columns); per-image sums mhe_sum_over_hypotheses; column sums ops.colsum;
          batch-major: g_logp per row (mhe_glow_coupling_inv_bwd_wide_f32); per-image sums mhe_sum_row_blocks_f32; column sums of
            the flow-width rows (gv, g_prm) per image then over images (_colsum), of the hidden-width rows ops.colsum.
        bf16 tapes (t2, t3 as [R, 1, 1, H] bfloat16) take the block's four products on bf16 MFMA."""
        D, H = self.features, self.hidden
        ctab, row_div, B, sample_major = tape["ctab"], tape["row_div"], tape["n_img"], tape["sample_major"]
        R, N = gv.shape[0], gv.shape[0] // B
        dev = gv.device
        img_sum, flow_colsum = self._reducers(tape, R)
        per = 1 + self.num_blocks
        for l, (t, d, o) in enumerate(zip(tape["layers"], tape["pk"]["layers"], layers)):
            slot = l * per
            ops.linear_wgrad(t["y"], gv, o["dAinv"]); flow_colsum(gv, o["dcinv"])
            gy = ops.linear(gv, o["AinvT"])
            if sample_major:
                gvc, gprm = torch.empty(R, 64, device=dev), torch.empty(R, 64, device=dev)
                ops.launch("mhe_glow_coupling_inv_bwd_f32", t["v"], t["prm"], gy, g_logp, -1.0 / N, gvc, gprm, R, B, D, d["first"], d["T"])
            else:
                gvc, gprm = ops.glow_coupling_inv_bwd_wide(t["v"], t["prm"], gy, g_logp, D, d["first"], d["T"])
            gh = self._net_reverse(t, o, ctab, slot, gprm, Gct, row_div, B, img_sum, flow_colsum)
            gv = ops.add(gvc, ops.linear(gh, o["wxT"]))          # (after the last layer: dL/dnoise, which no caller reads)

    def _reverse_density(self, tape, g_z, g_logp, Gct, layers):
        """the staged reverse pass of the DENSITY direction (pose -> noise: what maximum-likelihood training differentiates) over a
        `_run(..., inverse=False, tape=)` tape, layers L-1 .. 0:
            gy = g_z - g_logp z (the base density; mhe_glow_base_density_bwd_f32);  per layer: forward-coupling reverse -> g_v, g_prm
            (mhe_glow_coupling_fwd_bwd_f32);  the net's reverse (`_net_reverse`, shared with `_reverse`);  g_v += gh Wx;
            dA = g_v^T u, dc = sum g_v;  gy = g_v A.
        g_z (R, D) = dL/dz or None, g_logp (R,) = dL/dlog_prob or None; Gct as for `_reverse`.  layers(l): called as the pass reaches layer l, gives
        its transposed operands AT, wfT, wxT, blocksT and its ZEROED gradient destinations dA, dc, dwf, dbf, dwx, dblocks.  Returns dL/dinputs padded
        (R, Dp).  Rows are sample-major (row r belongs to image r % B; B = R is one row per context row)."""
        D = self.features
        ctab, row_div, B = tape["ctab"], tape["row_div"], tape["n_img"]
        R = tape["layers"][-1]["y"].shape[0]
        img_sum, flow_colsum = self._reducers(tape, R)
        per = 1 + self.num_blocks
        gy = ops.glow_base_density_bwd(tape["layers"][-1]["y"], g_z, g_logp, D)
        for l in range(self.num_layers - 1, -1, -1):
            t, d, o = tape["layers"][l], tape["pk"]["layers"][l], layers(l)
            gvc, gprm = ops.glow_coupling_fwd_bwd(t["v"], t["prm"], gy, g_logp, D, d["first"], d["T"])
            gh = self._net_reverse(t, o, ctab, l * per, gprm, Gct, row_div, B, img_sum, flow_colsum)
            gv = ops.add(gvc, ops.linear(gh, o["wxT"]))
            ops.linear_wgrad(t["u"], gv, o["dA"]); flow_colsum(gv, o["dc"])
            gy = ops.linear(gv, o["AT"])
        return gy

    def _net_grad_buffers(self, pk, dev):
        """zeroed destinations of the nets' weight gradients, per layer (dwf, dbf, dwx, dblocks: what `_net_reverse` adds to)"""
        H, z = self.hidden, (lambda *shape: torch.zeros(*shape, device=dev))
        return [{"dwf": z(d["wf"].shape[0], H), "dbf": z(d["wf"].shape[0]), "dwx": z(H, self.Dp),
                 "dblocks": [(z(H, H), z(H), z(H, H), z(H)) for _ in d["blocks"]]} for d in pk["layers"]]

    def _grads_by_param(self, pk, dst, dW, db, ga):
        """{parameter: gradient} from a reverse pass's buffers: dst (per layer dwf, dbf, dwx, dblocks), dW / db (the context table's weight and
        bias gradients, [cs, F] / [cs]) and ga [L, 4 D + D (D - 1)] (the ActNorm / LU gradients in the packed order log_scale, shift,
        lower_entries, upper_entries, unconstrained_upper_diag, bias)"""
        D, H, per = self.features, self.hidden, 1 + self.num_blocks
        T, n, grads = self._transform._transforms, D * (D - 1) // 2, {}
        for l, (d, o) in enumerate(zip(pk["layers"], dst)):
            an, lu, cp = T[3 * l], T[3 * l + 1], T[3 * l + 2]
            net, r, slot = cp.transform_net, ga[l], l * per
            grads[an.log_scale], grads[an.shift] = r[:D], r[D:2 * D]
            grads[lu.lower_entries], grads[lu.upper_entries] = r[2 * D:2 * D + n], r[2 * D + n:2 * D + 2 * n]
            grads[lu.unconstrained_upper_diag], grads[lu.bias] = r[2 * D + 2 * n:3 * D + 2 * n], r[3 * D + 2 * n:]
            grads[net.initial_layer.weight] = torch.cat([o["dwx"][:, cp.identity_features], dW[slot * H:(slot + 1) * H]], 1)
            grads[net.initial_layer.bias] = db[slot * H:(slot + 1) * H]
            grads[net.final_layer.weight], grads[net.final_layer.bias] = o["dwf"][:2 * d["T"]], o["dbf"][:2 * d["T"]]
            for b, (blk, (dw0, db0, dw1, db1)) in enumerate(zip(net.blocks, o["dblocks"])):
                k = slot + 1 + b
                grads[blk.linear_layers[0].weight], grads[blk.linear_layers[0].bias] = dw0, db0
                grads[blk.linear_layers[1].weight], grads[blk.linear_layers[1].bias] = dw1, db1
                grads[blk.context_layer.weight], grads[blk.context_layer.bias] = dW[k * H:(k + 1) * H], db[k * H:(k + 1) * H]
        return grads

    def _log_prob_backward(self, tape, g_z, g_logp):
        """`_reverse_density` into fresh gradients, then the context weights' gradient from the per-image rows, dL/dcontext, and the ActNorm / LU
        gradients from dA, dc and sum dL/dlog_prob in float64 (ops.glow_affine_density_bwd) -> ({parameter: gradient}, dL/dinputs (R, D),
        dL/dcontext (B, F))"""
        D, Lr, Dp = self.features, self.num_layers, self.Dp
        pk, ctab, B = tape["pk"], tape["ctab"], tape["n_img"]
        cs, dev = ctab.shape[1], ctab.device
        Gct = torch.zeros(B, cs, device=dev)
        dA, dc = torch.zeros(Lr, Dp, Dp, device=dev), torch.zeros(Lr, Dp, device=dev)
        dst = self._net_grad_buffers(pk, dev)
        def layer(l):           # the transposed operands one layer at a time, as the reverse reaches it
            d = pk["layers"][l]
            return {**dst[l], "dA": dA[l], "dc": dc[l], "AT": d["A"].t().contiguous(), "wfT": d["wf"].t().contiguous(),
                    "wxT": d["wx"].t().contiguous(), "blocksT": [(w0.t().contiguous(), w1.t().contiguous()) for (w0, _, w1, _) in d["blocks"]]}
        g_in = self._reverse_density(tape, g_z, g_logp, Gct, layer)
        dW, db = torch.zeros(cs, self.context_features, device=dev), torch.zeros(cs, device=dev)
        ops.linear_wgrad(tape["context"], Gct, dW); ops.colsum(Gct, db)
        g_ctx = ops.linear(Gct, pk["wctx"].t().contiguous())
        ga = ops.glow_affine_density_bwd(dA, dc, g_logp, Lr, D, pk["aff"]["ws"]).float()
        return self._grads_by_param(pk, dst, dW, db, ga), g_in[:, :D].contiguous(), g_ctx

    # ---- reference call surface ----------------------------------------------------------------------------
    def log_prob(self, inputs, context=None, rows_per_context=None):
        """(log_prob (R,), noise (R,D)).  `context` has R rows (the reference passes `feat.repeat(N,1)`), or B rows with
        sample-major inputs (row r uses context[r % B]; extension, hoists the context terms).

        Differentiable - the maximum-likelihood loss `-log_prob.mean()` of the reference's README.md:32-34 - when grad is enabled and `inputs` or
        `context` require grad, or the module is in train mode with parameters that require grad: one autograd node (_LogProbFn) whose forward
        is this very pass with a tape (bit-identical values) and whose backward is the hand-written `_reverse_density`; both results carry
        gradients to every flow parameter, `context` (with B rows: the per-image sum) and `inputs`.  Train-mode dropout is on the tape for flows
        of up to 64 features.  Refused there (NotImplementedError): compute_dtype bfloat16; train-mode dropout on a wider flow.  Otherwise the
        inference pass, returning plain tensors."""
        R, Bc = inputs.shape[0], context.shape[0]
        if R % Bc:
            raise ValueError(f"glow rows ({R}) must be a multiple of context rows ({Bc})")
        if torch.is_grad_enabled() and (inputs.requires_grad or context.requires_grad
                                        or (self.training and any(p.requires_grad for p in self.parameters()))):
            return _LogProbFn.apply(self, inputs, context, *self.parameters())
        z, lp = self._run(inputs.contiguous(), context.contiguous(), False, 1, Bc)
        return lp, z

    def sample_and_log_prob(self, num_samples, noise=None, context=None):
        """samples (B,N,D), log_prob (B,N), noise - rows batch-major as nflows lays them out."""
        B = context.shape[0]
        if noise is None:
            noise = ops.randn(B * num_samples, self.features, context.device).view(B, num_samples, self.features)      # drawn on the device (mhe_randn_f32)
        x, lp = self._run(noise.reshape(B * num_samples, self.features).contiguous(), context.contiguous(), True, num_samples, B)
        return x.view(B, num_samples, -1), lp.view(B, num_samples), noise

    def forward(self, context, num_samples=1):
        """ProHMR call form `flow(conditioning_feats, num_samples)` (reference README.md:34,39)"""
        s, lp, _ = self.sample_and_log_prob(num_samples, context=context)
        return s, lp


class _LogProbFn(torch.autograd.Function):
    """ConditionalGlow.log_prob as one autograd node: forward = the f32 density pass with a tape (ConditionalGlow._run, the no-grad pass's own
    code: bit-identical values); backward = ConditionalGlow._log_prob_backward"""
    @staticmethod
    def forward(ctx, g, inputs, context, *params):
        if g.compute_dtype != torch.float32:
            raise NotImplementedError("the Glow reverse pass runs in f32 parity mode: compute_dtype must be torch.float32 under grad")
        if g.features > 64 and g.training and g.p_drop > 0.0:
            raise NotImplementedError("the wide Glow reverse pass has no dropout: build the flow with dropout_probability=0 or call eval()")
        inputs, context = inputs.contiguous(), context.contiguous()
        tape = {"context": context, "sample_major": True}
        z, lp = g._run(inputs, context, False, 1, context.shape[0], tape=tape)
        ctx.g, ctx.tape = g, tape
        ctx.set_materialize_grads(False)
        return lp, z

    @staticmethod
    def backward(ctx, g_lp, g_z):
        g, tape = ctx.g, ctx.tape
        params = list(g.parameters())
        if g_lp is None and g_z is None:
            return (None,) * (3 + len(params))
        grads, g_in, g_ctx = g._log_prob_backward(tape, None if g_z is None else g_z.float().contiguous(),
                                                  None if g_lp is None else g_lp.float().contiguous())
        ctx.tape = None
        return (None, g_in if ctx.needs_input_grad[1] else None, g_ctx if ctx.needs_input_grad[2] else None) + tuple(grads.get(q) for q in params)
