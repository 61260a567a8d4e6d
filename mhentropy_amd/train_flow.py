"""Train-step part for the RealNVP branch (`q_z_giv_i`): its operand tables, the sampling pass with what the reverse pass needs, the
reverse pass of the couplings (one launch, or coupling by coupling - csrc/flow_rev.hip, flow_bwd.hip + mhe_conv_wgrad_nhwc) and the
reverse of the conditioning projections.  Same three calls as train_glow.GlowPart: sample(), reverse(), feat_grad()."""
import os

import numpy as np
import torch

from . import ops


def flow_stream_table(dim, h, bf16):
    """gather table of ONE net's fragment-ordered weight stream, as local indices into [W0 | W1 | W2]
    (obtained by running the host packer on index-valued weights)"""
    n0, n1, n2 = h * dim, h * h, dim * h
    loc = np.arange(n0 + n1 + n2, dtype=np.int64)
    parts = lambda a: (a[:n0].reshape(h, dim), a[n0:n0 + n1].reshape(h, h), a[n0 + n1:].reshape(dim, h))
    if not bf16:
        w = parts((loc + 1).astype(np.float32))               # < 2^24: exact in f32
        return ops.flow_pack_net(*w).astype(np.int64) - 1
    out, pad = None, None
    for dig in range(3):                                        # base-128 digits (+1) are exact in bf16
        w = parts((((loc >> (7 * dig)) & 127) + 1).astype(np.float32))
        s = ops.flow_pack_net_bf16(*w)
        v = (s.astype(np.uint32) << 16).view(np.float32).astype(np.int64)
        if dig == 0:
            pad, out = v == 0, np.zeros_like(v)
        out += (np.maximum(v, 1) - 1) << (7 * dig)
    out[pad] = -1
    return out


class RealNVPPart:
    def __init__(self, arena, flow, cond_bwd_bf16=True):
        """tables only (host integer work on the arena): no kernel is launched"""
        ar, fl = arena, flow
        self.ar, self.flow, self.cond_bwd_bf16 = ar, fl, cond_bwd_bf16
        dim, h, ncoup = fl.dim, fl.hidden, len(fl.mask)
        bf16 = self.bf16 = fl.compute_dtype == torch.bfloat16 and h % 128 == 0
        # the one-launch forward / reverse kernels (hidden 512) read fragment-major layouts of their own: everything else is a fallback layout
        self.fused_tables = bool(bf16 and h == 512 and ar.fb_lazy)
        # per step: kept activations (h1, h2, s / t pre-activations), their sign bits, conditioning table, bf16 feature; its gradient's layouts
        self.kept = self.sign = self.cond = self.feat_b = self.Gc = self.GcT = self.Gc_packed = self.z0_recovered = None
        pidx, derived = ar.pidx, ar.derived
        loc = torch.from_numpy(flow_stream_table(dim, h, bf16))
        n0, n1 = h * dim, h * h
        streams, b2, wc, bc1, bc2 = [], [], [], [], []
        self.nets = []
        for i in range(ncoup):
            for net in (fl.s[i], fl.t[i]):
                o0, o1, o2 = (ar.off[id(net.l[j].weight)] for j in range(3))
                g = torch.where(loc < 0, loc, torch.where(loc < n0, loc + o0, torch.where(loc < n0 + n1, loc - n0 + o1, loc - n0 - n1 + o2)))
                streams.append(g)
                bi = torch.full((64 if bf16 else dim,), -1, dtype=torch.int64)
                bi[:dim] = pidx(net.l[2].bias)
                b2.append(bi)
                for j in range(2):
                    wc.append(pidx(net.c[j].weight))
                    bc1.append(pidx(net.c[j].bias)); bc2.append(pidx(net.l[j].bias))
                d = {"net": net}
                # reverse-pass operands (f32): padded W0 [h,64], W1 [h,h] (the parameter itself), padded W2 [64,h] + transposes
                w0i = torch.full((h, 64), -1, dtype=torch.int64); w0i[:, :dim] = pidx(net.l[0].weight)
                w1i = pidx(net.l[1].weight)
                w2i = torch.full((64, h), -1, dtype=torch.int64); w2i[:dim] = pidx(net.l[2].weight)
                b2i = torch.full((64,), -1, dtype=torch.int64); b2i[:dim] = pidx(net.l[2].bias)
                fb = self.fused_tables             # (the f32 / plain bf16 layouts below are the fallback paths' when the fragment-major ones exist)
                f32, bf, tr = torch.float32, torch.bfloat16, lambda t: t.t().contiguous()
                d["w0"], d["w0T"] = derived(w0i, f32, fallback=fb), derived(tr(w0i), f32, fallback=fb)
                d["w1"], d["w1T"] = net.l[1].weight.data, derived(tr(w1i), f32, fallback=fb)
                if bf16:
                    # bf16 operand copies for the products that run on bf16 MFMA (all but the two 64-wide f32 ones): w0b [h, 64]: XP W0^T,
                    # w2Tb [h, 64]: GO W2, w2b [64, h]: H1 W2^T (f32 result), w0Tb [64, h]: G1 W0 (f32 result)
                    for key, t in (("w1b", w1i), ("w1Tb", tr(w1i)), ("w0b", w0i), ("w2Tb", tr(w2i)), ("w2b", w2i), ("w0Tb", tr(w0i))):
                        d[key] = derived(t, bf, fallback=fb)
                    # the three [out][k] operands again in MFMA fragment order: what the one-launch reverse chain reads (csrc/flow_rev.hip)
                    # ... and the forward's own operands W1 [out][in], W0 (padded) [h][64], W2 (padded) [64][h] (csrc/flow_fwd.hip)
                    for key, t in (("w1Fb", w1i.t()), ("w2Fb", w2i.t()), ("w0Fb", w0i.t()), ("f1F", w1i), ("f0F", w0i), ("f2F", w2i)):
                        d[key] = derived(ops.mfma_fragment_major(t), bf)
                d["w2"], d["w2T"] = derived(w2i, f32, fallback=fb), derived(tr(w2i), f32, fallback=fb)
                d["b2"] = derived(b2i, f32, fallback=fb)
                d["r0"], d["r1"], d["r2"], d["rb2"] = (ar.raw_slot(s) for s in ((h, 64), (h, h), (64, h), (64,)))
                ar.map_grad(net.l[0].weight, (torch.arange(h * 64, dtype=torch.int64).view(h, 64) + d["r0"])[:, :dim])
                ar.map_grad(net.l[1].weight, torch.arange(h * h, dtype=torch.int64).view(h, h) + d["r1"])
                ar.map_grad(net.l[2].weight, (torch.arange(64 * h, dtype=torch.int64).view(64, h) + d["r2"])[:dim])
                ar.map_grad(net.l[2].bias, torch.arange(dim, dtype=torch.int64) + d["rb2"])
                self.nets.append(d)
        self.f_stream = derived(torch.cat(streams), torch.bfloat16 if bf16 else torch.float32, fallback=self.fused_tables)
        self.f_b2 = derived(torch.stack(b2), torch.float32)
        # bf16 mode with the conditioning products in bf16 (forward table, dWc, g_feat): the two f32 copies (2 x 12.6 M elements at C2) would
        # only be gathered every step to be read by nobody
        self.cond_f32 = not (bf16 and fl.tsfm_on % 64 == 0 and cond_bwd_bf16)
        self.f_wc = derived(torch.cat(wc), torch.float32) if self.cond_f32 else None       # [2*ncoup*2*h, 512]
        self.f_wcb = derived(torch.cat(wc), torch.bfloat16) if bf16 and fl.tsfm_on % 64 == 0 else None      # forward operand in the bf16 mode
        self.f_bc = derived(torch.cat(bc1), torch.float32, torch.cat(bc2))       # c_j.bias + l_j.bias
        self.f_wcT = derived(torch.cat(wc).t().contiguous(), torch.float32) if self.cond_f32 else None     # [512, slots*h]
        slots = self.slots = 4 * ncoup
        raw_wc, raw_bc = ar.raw_slot((slots * h, fl.tsfm_on)), ar.raw_slot((slots * h,))
        k = 0
        for i in range(ncoup):
            for net in (fl.s[i], fl.t[i]):
                for j in range(2):
                    ar.map_grad(net.c[j].weight, torch.arange(h * fl.tsfm_on, dtype=torch.int64).view(h, fl.tsfm_on) + raw_wc + k * h * fl.tsfm_on)
                    bidx = torch.arange(h, dtype=torch.int64) + raw_bc + k * h
                    ar.map_grad(net.c[j].bias, bidx); ar.map_grad(net.l[j].bias, bidx)
                    k += 1

        def views():
            self.dwc, self.dbc = ar.raw_view(raw_wc, (slots * h, fl.tsfm_on)), ar.raw_view(raw_bc, (slots * h,))
            for d in self.nets:
                d["dw0"], d["dw1"], d["dw2"], d["db2"] = (ar.raw_view(d[k_], s) for k_, s in (("r0", (h, 64)), ("r1", (h, h)), ("r2", (64, h)), ("rb2", (64,))))
        ar.after_finalize(views)
        # the module's own forward paths (eval, sample) read the same device-resident operand packs: no host re-pack, never stale
        f0 = self.nets[0]
        fragp = (f0["f0F"], f0["f1F"], f0["f2F"], self._pitch("f1F")) if "f1F" in f0 and len(self.nets) > 1 else None
        fl._external_pack = (self.f_stream, self.f_b2, self.f_wc, self.f_bc, self.f_wcb, fragp)
        fl._external_sync = ar.sync_all

    def _pitch(self, key):
        """elements between two consecutive nets' bf16 operand `key` (the one-launch kernels walk the nets at one pitch)"""
        return (self.nets[1][key].data_ptr() - self.nets[0][key].data_ptr()) // 2

    # ------------------------------------------------------------------ sampling pass
    def sample(self, feat, feat_b, N, B, noise, draw):
        """conditioning product, z0 = draw(noise), the coupling stack; returns (sample, log q) and keeps what reverse() reads"""
        fl, ar = self.flow, self.ar
        h, ncoup = fl.hidden, len(fl.mask)
        if self.f_wcb is not None:
            if feat_b is None:
                feat_b = feat.to(torch.bfloat16)
            cond = ops.linear_bf16_f32out(feat_b, self.f_wcb, self.f_bc).view(B, 2 * ncoup, 2, h)
        else:
            cond = ops.linear(feat, self.f_wc, self.f_bc).view(B, 2 * ncoup, 2, h)
        self.cond, self.feat_b = cond, feat_b
        z0 = draw(noise)
        self.kept, self.sign = None, None
        if self.bf16 and h == 512 and os.environ.get("MHE_FLOW_RECOMPUTE", "0") != "1":
            # the 512-wide kernel writes the nets' activations out on the way: the reverse pass reads them instead of re-evaluating
            # the nets coupling by coupling (what autograd would have kept)
            Rr = N * B
            kept = (ar.buf("fl_h1", (2 * ncoup, Rr, h), torch.bfloat16), ar.buf("fl_h2", (2 * ncoup, Rr, h), torch.bfloat16),
                    ar.buf("fl_o", (2 * ncoup, Rr, 64)))
            f0 = self.nets[0]
            if (os.environ.get("MHE_FLOW_FRAG", "1") == "1" and "f1F" in f0 and N % 64 == 0          # (the tape form needs whole 64-row chunks)
                    and ops.flow_couplings_frag_supported(Rr, B, z0.shape[1], h, ncoup)):
                sg = ar.buf("fl_sign", (2 * ncoup, Rr // 64, 2, 8, 64, 2), torch.int32)
                x, _, log_q = ops.flow_couplings_frag(z0, cond, f0["f0F"], f0["f1F"], f0["f2F"], self._pitch("f1F"), self.f_b2, fl.mask, B, h,
                                                      ops.FLOW_FORWARD, emit=kept, sign_bits=sg)
                self.sign = sg
            else:
                ar.need_fallback()                 # the second-generation kernel's stream
                x, _, log_q = ops.flow_couplings_emit(z0, cond, self.f_stream, self.f_b2, fl.mask, B, h, ops.FLOW_FORWARD, *kept)
            self.kept = kept
        else:
            ar.need_fallback()
            x, _, log_q = ops.flow_couplings(z0, cond, self.f_stream, self.f_b2, fl.mask, B, h, ops.FLOW_FORWARD)
        return x, log_q

    # ------------------------------------------------------------------ reverse pass
    def reverse(self, x_out, g_x, g_logp, N, B, N_all=None):
        """reverse of the couplings; leaves the conditioning table's gradient for feat_grad().  N: hypotheses per image among the rows;
        N_all: hypotheses per image the means are taken over (differs only under hypothesis sharding)"""
        N_all = N_all or N
        fl, ar, nets, buf = self.flow, self.ar, self.nets, self.ar.buf
        h, dim, ncoup = fl.hidden, fl.dim, len(fl.mask)
        R, cstride = x_out.shape[0], self.slots * h
        lp_scale = -1.0 / N_all if g_logp is not None else 0.0
        XP = buf("XP", (R, 64))
        Hb = [[buf(f"H{n}{j}", (R, h)) for j in range(2)] for n in range(2)]
        O, GO, GX = ([buf(f"{k}{n}", (R, 64)) for n in range(2)] for k in ("O", "GO", "GX"))
        G2, G1 = buf("G2", (R, h)), buf("G1", (R, h))
        xa, xb = buf("xa", (R, dim)), buf("xb", (R, dim))
        ga, gb = buf("ga", (R, dim)), buf("gb", (R, dim))
        gpart = buf("gpart", (R, dim))
        Gc = self.Gc = buf("Gcond", (B, cstride))                # gradient of the conditioning table, all nets / layers
        cflat = self.cond.view(B, cstride)
        x_cur, g_cur = x_out, g_x
        mixed = self.bf16
        if mixed:
            bf = torch.bfloat16
            H1b = [buf(f"H1b{n}", (R, h), bf) for n in range(2)]
            P2b, G2b, GH1b = buf("P2b", (R, h), bf), buf("G2b", (R, h), bf), buf("GH1b", (R, h), bf)
            v4 = lambda t: t.view(R, 1, 1, t.shape[1])
            # bf16 performance mode: every product except the two that feed exp/tanh (H1 W2^T -> s, t) or the flow variable's own
            # gradient chain (G1 W0 -> GX) takes bf16 operands with f32 accumulation - as the forward kernel does; the leaky-ReLU
            # reverse is fused with the per-image sums that give the conditioning table's gradient
            XPb, P0b = buf("XPb", (R, 64), bf), buf("P0b", (R, h), bf)
            H2b = [buf(f"H2b{n}", (R, h), bf) for n in range(2)]
            GOb = [buf(f"GOb{n}", (R, 64), bf) for n in range(2)]
            G1b = buf("G1b", (R, h), bf)
            GcT = self.GcT = buf("GcondT", (cstride, B))         # the same sums as Gc, [column][image]: split-K operand of g_feat
            self.Gc_packed = None
            kept = self.kept
            if kept is not None and kept[0].shape[1] != R:
                kept = None
            # grouped weight gradients (ops.conv_wgrad_batched): with the forward's activations kept, every net's reverse operands are kept
            # too (GO, G2, G1, the masked inputs: 0.9 GB at C2) and the 72 per-net weight-gradient launches (4 - 16 output tiles each,
            # 30 - 55 us apiece) become four grouped ones after the chain - MHE_FLOW_WGRAD_GROUPED=0: per net, as the chain goes
            grouped = kept is not None and os.environ.get("MHE_FLOW_WGRAD_GROUPED", "1") == "1"
            if grouped:
                GOb_all = buf("GOb_all", (2 * ncoup, R, 64), bf)
                G2b_all, G1b_all = buf("G2b_all", (2 * ncoup, R, h), bf), buf("G1b_all", (2 * ncoup, R, h), bf)
                XPb_all = buf("XPb_all", (ncoup, R, 64), bf)
            # the whole data-gradient chain in one launch (csrc/flow_rev.hip): 64 hypotheses per image, one workgroup per image.
            # MHE_FLOW_REV_FUSED=0: coupling by coupling (13 launches each)
            fused = (grouped and os.environ.get("MHE_FLOW_REV_FUSED", "1") == "1" and N == N_all and R == 64 * B
                     and ops.flow_reverse_chain_supported(R, B, dim, h, ncoup))
            if fused:
                f0 = nets[0]
                wst = self._pitch("w1Fb")
                assert wst > 0 and all((nets[k][key].data_ptr() - f0[key].data_ptr()) // 2 == k * wst
                                       for k in range(2 * ncoup) for key in ("w2Fb", "w1Fb", "w0Fb"))
                z0r = buf("z0_rec", (R, dim))
                sg = self.sign
                if sg is None or sg.shape[1] != B:      # (activations kept by the second-generation kernel: signs from the tensors themselves)
                    sg = ops.flow_sign_bits(kept[0], kept[1], B)
                ops.flow_reverse_chain(x_out, g_x, g_logp, lp_scale, fl.mask, kept[2], sg,
                                       f0["w2Fb"], f0["w1Fb"], f0["w0Fb"], wst, GOb_all, G2b_all, G1b_all, XPb_all, Gc, f0["db2"],
                                       nets[1]["rb2"] - f0["rb2"], z0r)
                # (the kernel leaves the per-image sums as [image][column] rows only; both bf16 operands of the conditioning layer's
                # reverse - the rows and their transpose - come from one pack launch instead of a scattered second layout + two casts)
                self.Gc_packed = ops.pack_transpose_bf16(Gc, out=buf("Gcond_b", (B, cstride), bf), outT=buf("GcondT_b", (cstride, B), bf))
                x_cur = z0r
            if not fused:
                ar.need_fallback()                     # the coupling-by-coupling pass reads the plain operand layouts
            for i in range(ncoup - 1, -1, -1) if not fused else ():
                m = fl.mask[i]
                if grouped:
                    XPb, GOb, G2b_n, G1b_n = XPb_all[i], [GOb_all[2 * i], GOb_all[2 * i + 1]], [G2b_all[2 * i], G2b_all[2 * i + 1]], [G1b_all[2 * i], G1b_all[2 * i + 1]]
                ops.flow_mask_pad_mixed(x_cur, m, out_bf16=XPb)
                if kept is not None:                   # written out by the forward kernel (mhe_flow_couplings_bf16_emit)
                    H1b, H2b, O = [[k[2 * i + n] for n in range(2)] for k in kept]
                for n in range(2 if kept is None else 0):
                    d, slot = nets[2 * i + n], (2 * i + n) * 2
                    ops.conv2d_nhwc(v4(XPb), d["w0b"], 1, 1, 1, 0, out=v4(P0b))
                    ops.flow_cond_lrelu_mixed(P0b, cflat[:, slot * h:], cstride, B, out_bf16=H1b[n])
                    ops.conv2d_nhwc(v4(H1b[n]), d["w1b"], 1, 1, 1, 0, out=v4(P2b))
                    ops.flow_cond_lrelu_mixed(P2b, cflat[:, (slot + 1) * h:], cstride, B, out_bf16=H2b[n])
                    ops.linear_bf16_f32out(H2b[n], d["w2b"], d["b2"], out=O[n])            # s, t pre-activations: f32 result, as the forward kernel
                x_in, g_in = (xa, ga) if x_cur is not xa else (xb, gb)
                ops.flow_couple_bwd(x_cur, O[0], O[1], m, g_cur, g_logp, lp_scale, B, x_in, GO[0], GO[1], gpart,
                                    GOb[0], GOb[1], db_s=nets[2 * i]["db2"], db_t=nets[2 * i + 1]["db2"])
                for n in range(2):
                    d, slot = nets[2 * i + n], (2 * i + n) * 2
                    if grouped:
                        G2b, G1b = G2b_n[n], G1b_n[n]
                    else:
                        ops.conv_wgrad(v4(H2b[n]), v4(GOb[n]), 1, 1, 1, 0, d["dw2"])
                    ops.conv2d_nhwc(v4(GOb[n]), d["w2Tb"], 1, 1, 1, 0, out=v4(P2b))
                    ops.flow_lrelu_bwd_sum(P2b, H2b[n], N, B, Gc[:, (slot + 1) * h:], Gc.shape[1], out_bf16=G2b, sum_out_t=GcT[(slot + 1) * h:])
                    if not grouped:
                        ops.conv_wgrad(v4(H1b[n]), v4(G2b), 1, 1, 1, 0, d["dw1"])
                    ops.conv2d_nhwc(v4(G2b), d["w1Tb"], 1, 1, 1, 0, out=v4(GH1b))
                    ops.flow_lrelu_bwd_sum(GH1b, H1b[n], N, B, Gc[:, slot * h:], Gc.shape[1], out_bf16=G1b, sum_out_t=GcT[slot * h:])
                    if not grouped:
                        ops.conv_wgrad(v4(XPb), v4(G1b), 1, 1, 1, 0, d["dw0"])
                    ops.linear_bf16_f32out(G1b, d["w0Tb"], out=GX[n])
                ops.flow_couple_accum(gpart, GX[0], GX[1], m, g_in)
                x_cur, g_cur = x_in, g_in
            if grouped:
                f0, nn = nets[0], 2 * ncoup
                stride = nets[1]["r1"] - f0["r1"]                   # the nets' raw-gradient slots are laid out at one pitch
                assert all(nets[k][key] - f0[key] == k * stride for k in range(nn) for key in ("r0", "r1", "r2"))
                ops.conv_wgrad_batched(kept[1], GOb_all, f0["dw2"], stride, nn)           # dW2 = GO^T H2   [64, h]  x 24
                ops.conv_wgrad_batched(kept[0], G2b_all, f0["dw1"], stride, nn)           # dW1 = G2^T H1   [h, h]   x 24
                for n in range(2):      # dW0 = G1^T XP [h, 64]: the s (t) nets of the 12 couplings share their coupling's masked input
                    ops.conv_wgrad_batched(XPb_all, G1b_all[n], nets[n]["dw0"], 2 * stride, ncoup, gy_batch_stride=2 * R * h)
            self.z0_recovered = x_cur
            return
        for i in range(ncoup - 1, -1, -1):
            m = fl.mask[i]
            ops.flow_mask_pad(x_cur, m, XP)
            for n in range(2):
                d, slot = nets[2 * i + n], (2 * i + n) * 2
                ops.linear(XP, d["w0"], out=Hb[n][0])
                ops.flow_cond_lrelu(Hb[n][0], cflat[:, slot * h:], cstride, B)
                ops.linear(Hb[n][0], d["w1"], out=Hb[n][1])
                ops.flow_cond_lrelu(Hb[n][1], cflat[:, (slot + 1) * h:], cstride, B)
                ops.linear(Hb[n][1], d["w2"], d["b2"], out=O[n])
            x_in, g_in = (xa, ga) if x_cur is not xa else (xb, gb)
            ops.flow_couple_bwd(x_cur, O[0], O[1], m, g_cur, g_logp, lp_scale, B, x_in, GO[0], GO[1], gpart)
            for n in range(2):
                d, slot = nets[2 * i + n], (2 * i + n) * 2
                ops.linear_wgrad(Hb[n][1], GO[n], d["dw2"]); ops.colsum(GO[n], d["db2"])
                ops.linear(GO[n], d["w2T"], out=G2)
                ops.flow_lrelu_bwd(G2, Hb[n][1])
                ops.linear_wgrad(Hb[n][0], G2, d["dw1"])
                ops.sum_over_hypotheses(G2, N, B, out=Gc[:, (slot + 1) * h:], out_stride=Gc.shape[1])
                ops.linear(G2, d["w1T"], out=G1); ops.flow_lrelu_bwd(G1, Hb[n][0])
                ops.linear_wgrad(XP, G1, d["dw0"])
                ops.sum_over_hypotheses(G1, N, B, out=Gc[:, slot * h:], out_stride=Gc.shape[1])
                ops.linear(G1, d["w0T"], out=GX[n])
            ops.flow_couple_accum(gpart, GX[0], GX[1], m, g_in)
            x_cur, g_cur = x_in, g_in
        self.z0_recovered = x_cur

    def feat_grad(self, feat):
        """reverse of the conditioning projections of all nets in one pass (dWc, dbc into the raw arena); returns d loss / d feat through them"""
        Gc, B = self.Gc, feat.shape[0]
        # bf16 mode: both products of the conditioning projections take bf16 operands like the rest of the flow's reverse pass (f32
        # accumulation; the two f32 launches were 0.19 ms); the bias gradient sums the f32 Gc
        cond_bf16 = self.bf16 and self.f_wcb is not None and B % 8 == 0 and self.cond_bwd_bf16
        # (a batch that is not a multiple of 8 cannot feed the bf16 kernel's 16-byte rows: f32 operands, the weights widened from
        # the bf16 copy for this call when the f32 copy is not kept)
        wc32 = self.f_wc if (cond_bf16 or self.cond_f32) else self.f_wcb.float()
        packed = self.Gc_packed
        if cond_bf16:
            fb = self.feat_b
            ops.linear_wgrad(fb if fb is not None else feat.to(torch.bfloat16), packed[0] if packed else Gc.to(torch.bfloat16), self.dwc)
        else:
            ops.linear_wgrad(feat, Gc, self.dwc)
        ops.colsum(Gc, self.dbc)
        if not (self.bf16 and B % 4 == 0):
            return ops.linear(Gc, self.f_wcT if self.f_wcT is not None else wc32.t().contiguous())
        # g_feat = Gc Wc is a (B x 24,576) x (24,576 x 512) product: 8 output tiles walking K serially as a plain GEMM
        # (~0.75 ms); as a split-K reduction over the 24,576 columns ("pixels" of the weight-gradient kernel, operands
        # GcT [k][b] and Wc [k][f] as they lie) it fills the chip
        K_, F_ = (self.f_wcb if self.f_wcb is not None else self.f_wc).shape
        g_feat = self.ar.buf("g_feat_flow", (B, F_)); g_feat.zero_()
        if cond_bf16:
            ops.conv_wgrad(self.f_wcb.view(K_, 1, 1, F_), (packed[1] if packed else self.GcT.to(torch.bfloat16)).view(K_, 1, 1, B), 1, 1, 1, 0, g_feat)
        else:
            GcT32 = self.GcT if packed is None else Gc.t().contiguous()
            ops.conv_wgrad(wc32.view(K_, 1, 1, F_), GcT32.view(K_, 1, 1, B), 1, 1, 1, 0, g_feat)
        return g_feat
