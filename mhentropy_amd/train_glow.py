"""Train-step part for the conditional Glow branch (`q_z_giv_i_model == 'glow'`): the sampling pass
`sample_and_log_prob` with a tape, and its hand-written reverse pass - what autograd does for the reference in
`loss_ent = log_prob.mean()` (reference README.md:36-42) / hand/network.py:736-742,781-799 + CrossModalHand.py:455-470.

PARITY UNPINNED like the forward (mhentropy_amd/glow.py): checked against torch autograd on the nflows restatement
(oracle/glow_ref.py), not against the absent third-party class.

Per layer (sampling order L-1 .. 0, reverse pass 0 .. L-1):
    params = ResidualNet(v[identity columns], context);  y = (v - shift) / scale on the transform columns;  v' = Ainv y + cinv
with (A, c) the ActNorm + LU affine map.  Dense products: mhe_linear_f32 / mhe_conv_wgrad_nhwc; elementwise stages: csrc/glow.hip.
The 45x45 re-parameterisation - A, A^-1, the log-det constant from (log_scale, shift, LU entries, softplus diagonal, bias), and their
gradients from dAinv, dcinv and the constant - runs in float64 ON THE DEVICE since round 5 (csrc/glow_affine.hip: one workgroup per layer;
rounds 2-4 did it in numpy on the host, a queue drain per step that kept this branch out of HIP graphs).  Dropout (train mode, p = 0.2: hand/network.py:343-344,781) is applied to the second activation
of every residual block in the sampling pass (mask bits kept on the tape) and to its gradient in the reverse pass (glow.py, mhe_dropout).
"""
import os

import torch

from . import ops


class GlowPart:
    def __init__(self, arena, glow):
        ar = self.ar = arena
        self.g, self.g_feat = glow, None
        D, H, Fc, L, NB = glow.features, glow.hidden, glow.context_features, glow.num_layers, glow.num_blocks
        if D > 64:
            raise NotImplementedError("the Glow reverse pass is built for the hand flow (features <= 64); the 144-D body geometry runs "
                                      "forward / sample / log_prob only")
        self.per = 1 + NB
        self.mixed = glow.compute_dtype == torch.bfloat16 and H % 64 == 0
        T = glow._transform._transforms
        slots = L * self.per
        self.raw_wctx, self.raw_bctx = ar.raw_slot((slots * H, Fc)), ar.raw_slot((slots * H,))
        self.layers = []
        wctx_idx, bctx_idx = [], []
        ix = lambda n: torch.arange(n, dtype=torch.int64)
        # the residual blocks' gradients in (layer, block) order, one pitch apart: what the grouped weight-gradient launches and the single
        # bias column sum of the fused reverse pass write ([L NB][H][H] x 2; [L NB][b0 | b1][H])
        self.raw_w0, self.raw_w1, self.raw_bias = ar.raw_slot((L * NB * H * H,)), ar.raw_slot((L * NB * H * H,)), ar.raw_slot((L * NB * 2 * H,))
        # ... and the initial / final layers' ([L][H][64], [L][64][H], [L][64]): the one-launch reverse chain's grouped launches write [L]-strided
        self.raw_wx, self.raw_wf, self.raw_bf = ar.raw_slot((L * H * 64,)), ar.raw_slot((L * 64 * H,)), ar.raw_slot((L * 64,))
        for l in range(L):
            an, lu, cp = T[3 * l], T[3 * l + 1], T[3 * l + 2]
            net = cp.transform_net
            idf = cp.identity_features.cpu()
            nid, nt = idf.numel(), int(cp.transform_features.numel())
            d = {"an": an, "lu": lu, "cp": cp, "nid": nid, "nt": nt, "idf": idf}
            # small re-parameterisation gradients land in exact-size raw slots (written from the host chain)
            for name, p in (("log_scale", an.log_scale), ("shift", an.shift), ("lower", lu.lower_entries), ("upper", lu.upper_entries),
                            ("udiag", lu.unconstrained_upper_diag), ("bias", lu.bias)):
                d["r_" + name] = ar.raw_slot(p.shape)
                ar.map_grad(p, ix(p.numel()).view(p.shape) + d["r_" + name])
            d["r_ainv"], d["r_cinv"] = ar.raw_slot((64, 64)), ar.raw_slot((64,))
            d["r_wx"], d["r_wf"], d["r_bf"] = self.raw_wx + l * H * 64, self.raw_wf + l * 64 * H, self.raw_bf + l * 64
            s0 = l * self.per
            wi = torch.empty(H, nid + Fc, dtype=torch.int64)
            wi[:, :nid] = (ix(H * 64).view(H, 64) + d["r_wx"])[:, idf]
            wi[:, nid:] = ix(H * Fc).view(H, Fc) + self.raw_wctx + s0 * H * Fc
            ar.map_grad(net.initial_layer.weight, wi)
            ar.map_grad(net.initial_layer.bias, ix(H) + self.raw_bctx + s0 * H)
            ar.map_grad(net.final_layer.weight, (ix(64 * H).view(64, H) + d["r_wf"])[:2 * nt])
            ar.map_grad(net.final_layer.bias, ix(2 * nt) + d["r_bf"])
            d["r_blocks"] = []
            for b, blk in enumerate(net.blocks):
                kb = l * NB + b
                rb = {"w0": self.raw_w0 + kb * H * H, "w1": self.raw_w1 + kb * H * H, "b0": self.raw_bias + (2 * kb) * H, "b1": self.raw_bias + (2 * kb + 1) * H}
                for j in range(2):
                    ar.map_grad(blk.linear_layers[j].weight, ix(H * H).view(H, H) + rb[f"w{j}"])
                    ar.map_grad(blk.linear_layers[j].bias, ix(H) + rb[f"b{j}"])
                ar.map_grad(blk.context_layer.weight, ix(H * Fc).view(H, Fc) + self.raw_wctx + (s0 + 1 + b) * H * Fc)
                ar.map_grad(blk.context_layer.bias, ix(H) + self.raw_bctx + (s0 + 1 + b) * H)
                d["r_blocks"].append(rb)
                # operand layouts refreshed on the device by the trainer's gather tables (like every other derived weight)
            wxi = torch.full((H, 64), -1, dtype=torch.int64)
            wxi[:, idf] = ar.pidx(net.initial_layer.weight)[:, :nid]
            wfi = torch.full((64, H), -1, dtype=torch.int64)
            wfi[:2 * nt] = ar.pidx(net.final_layer.weight)
            bfi = torch.full((64,), -1, dtype=torch.int64)
            bfi[:2 * nt] = ar.pidx(net.final_layer.bias)
            f32 = torch.float32
            d["wxi"], d["wfi"], d["bfi"] = wxi, wfi, bfi
            d["wx"], d["wxT"] = ar.derived(wxi, f32), ar.derived(wxi.t().contiguous(), f32)
            d["wf"], d["wfT"], d["bf"] = ar.derived(wfi, f32), ar.derived(wfi.t().contiguous(), f32), ar.derived(bfi, f32)
            d["blocks"] = [(blk.linear_layers[0].weight.data, blk.linear_layers[0].bias.data, blk.linear_layers[1].weight.data,
                            blk.linear_layers[1].bias.data) for blk in net.blocks]
            d["blocksT"] = [(ar.derived(ar.pidx(blk.linear_layers[0].weight).t().contiguous(), f32),
                             ar.derived(ar.pidx(blk.linear_layers[1].weight).t().contiguous(), f32)) for blk in net.blocks]
            d["first"], d["T"] = int(cp.transform_features[0]), nt
            if self.mixed:      # operands of the hidden x hidden products on bf16 MFMA (performance mode)
                bf = torch.bfloat16
                d["blocks_b"] = [(ar.derived(ar.pidx(blk.linear_layers[0].weight), bf), ar.derived(ar.pidx(blk.linear_layers[1].weight), bf),
                                  ar.derived(ar.pidx(blk.linear_layers[0].weight).t().contiguous(), bf),
                                  ar.derived(ar.pidx(blk.linear_layers[1].weight).t().contiguous(), bf)) for blk in net.blocks]
            wctx_idx.append(ar.pidx(net.initial_layer.weight)[:, nid:]); bctx_idx.append(ar.pidx(net.initial_layer.bias))
            for blk in net.blocks:
                wctx_idx.append(ar.pidx(blk.context_layer.weight)); bctx_idx.append(ar.pidx(blk.context_layer.bias))
            self.layers.append(d)
        self.wctx = ar.derived(torch.cat(wctx_idx), torch.float32)
        self.bctx = ar.derived(torch.cat(bctx_idx), torch.float32)
        self.wctxT = ar.derived(torch.cat(wctx_idx).t().contiguous(), torch.float32)
        # the six small tensors of every layer (in the flat parameter buffer) -> A, A^-1, c, c^-1, constant parts: one launch per refresh
        self._ptab = torch.tensor([[p.data_ptr() for p in (d["an"].log_scale, d["an"].shift, d["lu"].lower_entries, d["lu"].upper_entries,
                                                           d["lu"].unconstrained_upper_diag, d["lu"].bias)] for d in self.layers],
                                  dtype=torch.int64, device=ar.dev)
        self.aff = ops.glow_affine(self._ptab, L, D, self.layers[0]["lu"].eps)
        self._gtabs = None
        self._tp = None
        # operands of the one-launch sampling kernel (csrc/glow_fwd.hip): gather tables like every other derived layout
        self.fused = None
        if self.mixed and H == 512 and NB == 2 and D <= 48:
            nets = [d["cp"].transform_net for d in self.layers]
            st = lambda f: torch.stack([f(n) for n in nets])
            pi = ar.pidx
            fp = ops.glow_fused_layout(torch.stack([d["wxi"] for d in self.layers]),
                                       st(lambda n: torch.stack([pi(b.linear_layers[0].weight) for b in n.blocks])),
                                       st(lambda n: torch.stack([pi(b.linear_layers[1].weight) for b in n.blocks])),
                                       torch.stack([d["wfi"] for d in self.layers]), torch.stack([d["bfi"] for d in self.layers]),
                                       st(lambda n: torch.stack([pi(b.linear_layers[0].bias) for b in n.blocks])),
                                       st(lambda n: torch.stack([pi(b.linear_layers[1].bias) for b in n.blocks])), D)
            self.fused = {k: ar.derived(v.contiguous(), torch.bfloat16 if (k.endswith("F") or k.endswith("T")) else torch.float32) for k, v in fp.items()}
            # the final layer's rows move to the flow variable's columns in the chain's [g_shift | g_us] gradient: row c of the first / second half
            # is the shift / scale row of transform column c -> back to nflows' [shift (T) | scale (T)] rows by one index_select per step
            perm = torch.zeros(L, 64, dtype=torch.int64)
            for l in range(L):
                first = 1 - (l & 1)
                T_ = D // 2 if first else (D + 1) // 2
                cols = torch.arange(first, D, 2)
                perm[l, :T_], perm[l, T_:2 * T_] = cols, 64 + cols
                perm[l, 2 * T_:] = 63                          # (a zero row of the first half: columns >= dim are never transform columns)
            self._wf_perm = (perm + 128 * torch.arange(L)[:, None]).reshape(-1).to(ar.dev)
        glow._external_pack = self.module_pack

    # ------------------------------------------------------------------ the 45x45 affine maps (float64 on the device, tiny)
    def refresh_affine(self):
        """A = W diag(exp(log_scale)), c = W shift + b, their inverse (padded to 64) and the per-layer log-det constants from the CURRENT
        parameters: mhe_glow_affine_f64 into the same tensors (graph-capturable: no host value depends on the parameters)"""
        ops.glow_affine(self._ptab, self.g.num_layers, self.g.features, self.layers[0]["lu"].eps, out=self.aff)

    def _pack(self):
        """the operand dict ConditionalGlow._run reads (glow.py:_packed), on the trainer's device-resident layouts"""
        pk = {"layers": [], "const_parts": self.aff["const_parts"], "aff": self.aff, "wctx": self.wctx, "bctx": self.bctx, "fused": self.fused}
        for l, d in enumerate(self.layers):
            pk["layers"].append({"A": self.aff["A"][l], "c": self.aff["c"][l], "Ainv": self.aff["Ainv"][l], "cinv": self.aff["cinv"][l], "wx": d["wx"],
                                 "blocks": d["blocks"], "wf": d["wf"], "bf": d["bf"], "T": d["T"], "first": d["first"],
                                 "blocks_bf16": [bb[:2] for bb in d["blocks_b"]] if self.mixed else None})
        return pk

    def module_pack(self):
        """_pack for the modules' own forward / sample / log_prob paths: they follow the optimizer without any host-side re-packing"""
        self.ar.sync()
        self.refresh_affine()
        pk = self._pack()
        if not self.mixed and self.g.compute_dtype == torch.bfloat16:         # (bf16 chosen after this trainer was built)
            for e, d in zip(pk["layers"], self.layers):
                e["blocks_bf16"] = [(w0.to(torch.bfloat16), w1.to(torch.bfloat16)) for (w0, _, w1, _) in d["blocks"]]
        return pk

    # ------------------------------------------------------------------ sampling pass with tape
    def _forward_fused(self, z0, feat):
        """the sampling pass with its tape from ONE launch (mhe_glow_layers_bf16): the reverse pass below reads the kernel's tape tensors"""
        ar, g = self.ar, self.g
        D, H, B, R, L, NB = g.features, g.hidden, feat.shape[0], z0.shape[0], g.num_layers, g.num_blocks
        self.refresh_affine()
        ctab = ops.linear(feat, self.wctx, self.bctx)
        bits = g._drop_bits(R)
        bf = torch.bfloat16
        tape = {"v": ar.buf("glow_v", (L, R, 64)), "y": ar.buf("glow_y", (L, R, 64)), "prm": ar.buf("glow_prm", (L, R, 64)),
                "tb": ar.buf("glow_tb", (L, NB, R, H), bf), "t2": ar.buf("glow_t2", (L, NB, R, H), bf), "t3": ar.buf("glow_t3", (L, NB, R, H), bf),
                "hf": ar.buf("glow_hf", (L, R, H), bf)}
        chain = (os.environ.get("MHE_GLOW_REV_FUSED", "1") == "1" and ops.glow_reverse_chain_supported(R, B, D, H, L, NB))
        if chain:           # what the one-launch reverse chain reads besides t3: parameters in column order, the bf16 layer input, the ReLU gates as bits
            tape.update({"prmc": ar.buf("glow_prmc", (L, R, 128)), "vb": ar.buf("glow_vb", (L, R, 64), bf),
                         "bits": ar.buf("glow_bits", (L, NB, 2, B, 512, 2), torch.int32)})
        x, logq = ops.glow_layers(z0, ctab, self.fused, self.aff, bits, g.p_drop, R // B, B, D, B, 1, tape=tape)
        self._tp = {"fused": tape, "bits": bits, "ctab": ctab, "feat": feat, "chain": chain}
        return x, logq

    def forward(self, z0, feat):
        g, B, R = self.g, feat.shape[0], z0.shape[0]
        if (self.fused is not None and os.environ.get("MHE_GLOW_FUSED", "1") == "1" and R % B == 0
                and ops.glow_layers_supported(R // B, B, g.features, g.hidden, g.num_layers, g.num_blocks)):
            return self._forward_fused(z0, feat)
        self.refresh_affine()
        tape = {"sample_major": True}           # the module's own layer-by-layer pass on sample-major rows (r = n B + b), with its tape
        x, logq = g._run(z0, feat, True, 1, B, pk=self._pack(), tape=tape, bf16=self.mixed)
        self._tp = {"glow": tape, "feat": feat}
        return x, logq

    # ------------------------------------------------------------------ the train step's three calls (as train_flow.RealNVPPart)
    def sample(self, feat, feat_b, N, B, noise, draw):
        if noise is not None and noise.dim() == 3:          # the reference's (B,N,45) layout -> sample-major rows
            noise = noise.permute(1, 0, 2).reshape(N * B, 45)
        return self.forward(draw(noise), feat)

    def reverse(self, x_out, g_x, g_logp, N, B, N_all=None):
        self.g_feat = self.backward(g_x, g_logp, N, B)

    def feat_grad(self, feat):
        """d loss / d feat through the context terms (computed by reverse(): the Glow chain has no second stage)"""
        return self.g_feat

    # ------------------------------------------------------------------ reverse pass
    def _backward_chain(self, g_x, g_logp, N, B):
        """the reverse pass with the data-gradient chain of all layers in ONE launch (mhe_glow_reverse_chain_bf16, csrc/glow_rev.hip): what is
        left around it are the weight gradients - grouped launches over the tape and the chain's outputs as they lie ([L]- / [L, 2]-strided) -,
        the 45 x 45 products for dA^-1, the column sums of the per-image rows and the float64 re-parameterisation kernel"""
        ar, g = self.ar, self.g
        D, H, R, L, NB = g.features, g.hidden, g_x.shape[0], g.num_layers, g.num_blocks
        tp = self._tp
        ft, ctab = tp["fused"], tp["ctab"]
        raw, cs, bf = ar.raw_view, ctab.shape[1], torch.bfloat16
        out = {"gv": ar.buf("glow_gv", (L, R, 64)), "gpc": ar.buf("glow_gpc", (L, R, 128), bf), "gt3": ar.buf("glow_gt3", (L, NB, R, H), bf),
               "gt2": ar.buf("glow_gt2", (L, NB, R, H), bf), "gh0": ar.buf("glow_gh0", (L, R, H), bf), "gct": ar.buf("glow_Gct", (B, cs)),
               "bsum": ar.buf("glow_bsum", (B, L * NB * 2 * H)), "bfsum": ar.buf("glow_bfsum", (B, L * 128))}
        ops.glow_reverse_chain(g_x, g_logp, -1.0 / N, ft, ctab, self.fused, self.aff, g.p_drop if tp["bits"] is not None else 0.0, out, B, D)
        for l in range(L):          # dA^-1 = gv^T y, dc^-1 = sum gv (f32: they feed the float64 re-parameterisation)
            rs = self.layers[l]
            ops.linear_wgrad(ft["y"][l], out["gv"][l], raw(rs["r_ainv"], (64, 64))); ops.colsum(out["gv"][l], raw(rs["r_cinv"], (64,)))
        ops.conv_wgrad_batched(ft["t2"].view(L * NB, R, H), out["gt3"].view(L * NB, R, H), raw(self.raw_w1, (H, H)), H * H, L * NB)
        ops.conv_wgrad_batched(ft["tb"].view(L * NB, R, H), out["gt2"].view(L * NB, R, H), raw(self.raw_w0, (H, H)), H * H, L * NB)
        ops.conv_wgrad_batched(ft["vb"], out["gh0"], raw(self.raw_wx, (H, 64)), H * 64, L)                      # dWx[l] = gh0^T v   [H, 64]
        wfp = ar.buf("glow_wfp", (L * 128, H)); wfp.zero_()
        ops.conv_wgrad_batched(ft["hf"], out["gpc"], wfp[:128], 128 * H, L)                                     # [g_shift | g_us]^T h  [128, H] per layer
        torch.index_select(wfp, 0, self._wf_perm, out=raw(self.raw_wf, (L * 64, H)))                            # -> nflows' [shift | scale] rows
        bfp = ar.buf("glow_bfp", (L * 128,)); bfp.zero_()
        ops.colsum(out["bfsum"], bfp)
        torch.index_select(bfp, 0, self._wf_perm, out=raw(self.raw_bf, (L * 64,)))
        ops.colsum(out["bsum"], raw(self.raw_bias, (L * NB * 2 * H,)))
        Gct = out["gct"]
        ops.linear_wgrad(tp["feat"], Gct, raw(self.raw_wctx, (cs, g.context_features))); ops.colsum(Gct, raw(self.raw_bctx, (cs,)))
        g_feat = ops.linear(Gct, self.wctxT)
        self._reparam_backward(g_logp)
        return g_feat

    def _backward_fused(self, g_x, g_logp, N, B):
        """the reverse pass over the one-launch kernel's tape: per layer the small stages as before, per residual block two products on bf16
        MFMA and three per-image kernels (gate / dropout + ReLU reverse with the per-image sums inside, csrc/glow.hip); the 16 hidden x hidden
        weight gradients as TWO grouped launches after the chain (x = the tape's [L, 2, R, 512] tensors as they lie), all 16 bias gradients
        as ONE column sum of the per-image rows"""
        ar, g = self.ar, self.g
        D, H, R, L, NB = g.features, g.hidden, g_x.shape[0], g.num_layers, g.num_blocks
        tp = self._tp
        ft, bits, ctab = tp["fused"], tp["bits"], tp["ctab"]
        dev, raw, cs, bf = g_x.device, ar.raw_view, ctab.shape[1], torch.bfloat16
        gv = torch.empty(R, 64, device=dev)
        ops.launch("mhe_pad64_f32", g_x, gv, R, D)
        Gct = ar.buf("glow_Gct", (B, cs)); Gct.zero_()
        gt3_all, gt2_all = ar.buf("glow_gt3", (L, NB, R, H), bf), ar.buf("glow_gt2", (L, NB, R, H), bf)
        bs_w = L * NB * 2 * H
        bsum = ar.buf("glow_bsum", (B, bs_w))                  # per-image rows of all 16 bias gradients: every slice is written below
        dscale = 1.0 / (1.0 - g.p_drop) if bits is not None else 1.0
        for l in range(L):
            d = rs = self.layers[l]
            slot = l * self.per
            y, v, prm, hf = ft["y"][l], ft["v"][l], ft["prm"][l], ft["hf"][l]
            ops.linear_wgrad(y, gv, raw(rs["r_ainv"], (64, 64))); ops.colsum(gv, raw(rs["r_cinv"], (64,)))
            gy = ops.linear(gv, self.aff["AinvT"][l])
            gvc, gprm = torch.empty(R, 64, device=dev), torch.empty(R, 64, device=dev)
            ops.launch("mhe_glow_coupling_inv_bwd_f32", v, prm, gy, g_logp, -1.0 / N, gvc, gprm, R, B, D, d["first"], d["T"])
            # the final layer's operand was kept as bf16: its weight gradient on bf16 operands, f32 accumulation
            ops.conv_wgrad(hf.view(R, 1, 1, H), gprm.to(bf).view(R, 1, 1, 64), 1, 1, 1, 0, raw(rs["r_wf"], (64, H)))
            ops.colsum(gprm, raw(rs["r_bf"], (64,)))
            gh = ops.linear(gprm, d["wfT"])
            for b in range(NB - 1, -1, -1):
                kb = l * NB + b
                _, _, w0Tb, w1Tb = d["blocks_b"][b]
                gt3, gt2 = gt3_all[l, b].view(R, 1, 1, H), gt2_all[l, b].view(R, 1, 1, H)
                ops.launch("mhe_glow_glu_bwd_sum", gh, ft["t3"][l, b], ctab[:, (slot + 1 + b) * H:], cs, gt3, Gct[:, (slot + 1 + b) * H:], cs,
                           bsum[:, (2 * kb + 1) * H:], bs_w, N, B, H)
                ops.conv2d_nhwc(gt3, w1Tb, 1, 1, 1, 0, out=gt2)
                # dropout's and the ReLU's reverse in one pass: t2 = dropout(relu(.)) is zero exactly where either gate is closed
                ops.launch("mhe_glow_mask_scale_sum", gt2, ft["t2"][l, b], dscale, bsum[:, (2 * kb) * H:], bs_w, N, B, H)
                gt = ops.conv2d_nhwc(gt2, w0Tb, 1, 1, 1, 0)
                ops.launch("mhe_relu_bwd_add_mixed", gh, gt, ft["tb"][l, b], gh.numel(), ops.BF16, ops.BF16)
            ops.linear_wgrad(v, gh, raw(rs["r_wx"], (H, 64)))
            ops.sum_over_hypotheses(gh, N, B, out=Gct[:, slot * H:], out_stride=cs)
            gv = ops.add(gvc, ops.linear(gh, d["wxT"]))
        # dW1[l, b] = gt3^T t2, dW0[l, b] = gt2^T relu(h): two grouped launches over the tape tensors as they lie
        ops.conv_wgrad_batched(ft["t2"].view(L * NB, R, H), gt3_all.view(L * NB, R, H), raw(self.raw_w1, (H, H)), H * H, L * NB)
        ops.conv_wgrad_batched(ft["tb"].view(L * NB, R, H), gt2_all.view(L * NB, R, H), raw(self.raw_w0, (H, H)), H * H, L * NB)
        ops.colsum(bsum, raw(self.raw_bias, (bs_w,)))
        ops.linear_wgrad(tp["feat"], Gct, raw(self.raw_wctx, (cs, g.context_features))); ops.colsum(Gct, raw(self.raw_bctx, (cs,)))
        g_feat = ops.linear(Gct, self.wctxT)
        self._reparam_backward(g_logp)
        return g_feat

    def backward(self, g_x, g_logp, N, B):
        """g_x (R,45) = dL/d sample, g_logp (B,) = dL/d log_p per image (None: no entropy term).  Writes every Glow
        parameter's gradient into the trainer's raw arena and returns dL/d feat (B, F) through the context terms."""
        tp = self._tp
        if "fused" in tp:           # the one-launch kernel's tape (mixed mode)
            return (self._backward_chain if tp["chain"] else self._backward_fused)(g_x, g_logp, N, B)
        ar, g = self.ar, self.g
        D, H, R = g.features, g.hidden, g_x.shape[0]
        raw, cs = ar.raw_view, tp["glow"]["ctab"].shape[1]
        gv = torch.empty(R, 64, device=g_x.device)
        ops.launch("mhe_pad64_f32", g_x, gv, R, D)
        Gct = torch.zeros(B, cs, device=g_x.device)
        # the staged reverse (glow.py: ConditionalGlow._reverse) with the gradients landing in the raw arena
        layers = [{"AinvT": self.aff["AinvT"][l], "wfT": d["wfT"], "wxT": d["wxT"], "blocksT": [bb[2:] for bb in d["blocks_b"]] if self.mixed else d["blocksT"],
                   "dAinv": raw(d["r_ainv"], (64, 64)), "dcinv": raw(d["r_cinv"], (64,)), "dwf": raw(d["r_wf"], (64, H)), "dbf": raw(d["r_bf"], (64,)),
                   "dwx": raw(d["r_wx"], (H, 64)),
                   "dblocks": [(raw(rb["w0"], (H, H)), raw(rb["b0"], (H,)), raw(rb["w1"], (H, H)), raw(rb["b1"], (H,))) for rb in d["r_blocks"]]}
                  for l, d in enumerate(self.layers)]
        g._reverse(tp["glow"], gv, g_logp, Gct, layers)
        ops.linear_wgrad(tp["feat"], Gct, raw(self.raw_wctx, (cs, g.context_features))); ops.colsum(Gct, raw(self.raw_bctx, (cs,)))
        g_feat = ops.linear(Gct, self.wctxT)
        self._reparam_backward(g_logp)
        return g_feat

    def _reparam_backward(self, g_logp):
        """ActNorm / LU parameter gradients from dAinv, dcinv (in the raw arena) and the log-det constant: mhe_glow_reparam_bwd_f64, one
        workgroup per layer, float64, written straight into the six raw-gradient slots of every layer"""
        ar = self.ar
        if self._gtabs is None or self._gtabs[0] != ar.raw.data_ptr():
            base = ar.raw.data_ptr()
            at = lambda o: base + 4 * o
            mk = lambda rows: torch.tensor(rows, dtype=torch.int64, device=ar.dev)
            self._gtabs = (base, mk([at(d["r_ainv"]) for d in self.layers]), mk([at(d["r_cinv"]) for d in self.layers]),
                           mk([[at(d["r_" + k]) for k in ("log_scale", "shift", "lower", "upper", "udiag", "bias")] for d in self.layers]))
        _, ga, gc, gp = self._gtabs
        # sum_r dL/dlog q[r] = -sum_b g_logp[b] (the entropy term: each image's K rows carry g_logp[b] * (-1 / K))
        ops.glow_reparam_bwd(ga, gc, g_logp, self.g.num_layers, self.g.features, self.aff["ws"], gp, q_sign=-1.0)
