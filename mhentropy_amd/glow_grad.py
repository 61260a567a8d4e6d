"""Staged reverse pass of `ConditionalGlow.sample_and_log_prob` for any flow width (features <= 256; the 144-D body pose is what needs it), with
the gradients going to the caller - not to a trainer's arena like train_glow.GlowPart, which is built for the 64-column hand flow.

PARITY UNPINNED like the forward (mhentropy_amd/glow.py): checked against torch autograd on the nflows restatement (oracle/glow_ref.py).

`sample_with_tape` runs the same launches, on the same operands, as the module's own f32 sampling pass (glow.py: ConditionalGlow._run with
batch-major rows r = b N + n), so its values are bit-identical to it, and keeps per layer v, the residual stream h_0 .. h_NB, every block's
relu(h W0^T + b0) and its second product, the coupling parameters and y.  `backward` walks the layers 0 .. L-1:
    dA^-1 = gv^T y, dc^-1 = sum gv;  gy = gv A^-1;  coupling reverse (mhe_glow_coupling_inv_bwd_wide_f32) -> g_v, g_prm;
    residual net reverse (the f32 kernels of csrc/glow.hip; gate and context-column gradients summed per image with mhe_sum_row_blocks_f32);
    gv = g_v + gh Wx;
then the context weights' gradient from the per-image rows, dL/dcontext, and the ActNorm / LU gradients from dA^-1, dc^-1 and sum dL/dlog q in
float64 (mhe_glow_affine_wide_bwd_f64).  The noise is an input, not differentiated.
"""
import ctypes as C

import torch

from . import ops, _lib


def _affine(g, pk):
    """the wide float64 affine maps + workspace of the pack's parameters (the pack already holds them above 64 features)"""
    aff = pk["aff"]
    if aff is not None and "ws" in aff and aff["A"].shape[-1] == g.Dp and aff["ws"].numel() == _lib.lib().mhe_glow_affine_wide_workspace_doubles(
            g.num_layers, g.features):
        return aff
    T = g._transform._transforms
    return ops.glow_affine_wide(g.small_param_table(), g.num_layers, g.features, T[1].eps)


def _colsum(rows, B, N, out):
    """out = column sums of rows [B N, C] in a fixed order - per image, then over images (ops.colsum takes C | 256 or C >= 256; the flow
    variable and the coupling parameters are 192 wide)"""
    ops.sum_row_blocks(ops.sum_row_blocks(rows, B, N), 1, B, out=out.view(1, -1))


def sample_with_tape(g, noise_rows, context, N):
    """noise_rows (B N, D) batch-major, context (B, F) -> (x (B N, D), log_prob (B N,), tape)"""
    if g.compute_dtype != torch.float32:
        raise NotImplementedError("the Glow reverse pass runs in f32 parity mode: compute_dtype must be torch.float32 under grad")
    if g.training and g.p_drop > 0.0:
        raise NotImplementedError("the wide Glow reverse pass has no dropout: build the flow with dropout_probability=0 or call eval()")
    L_, D, H, R, B = _lib.lib(), g.features, g.hidden, noise_rows.shape[0], context.shape[0]
    ops._chk(noise_rows, torch.float32, "glow.noise", (R, D)); ops._chk(context, torch.float32, "glow.context", (B, g.context_features))
    pk = g._packed()
    aff = _affine(g, pk)
    s, dev = ops._stream, noise_rows.device
    ctab = ops.linear(context, pk["wctx"], pk["bctx"])
    cs = ctab.shape[1]
    v = torch.empty(R, g.Dp, device=dev)
    ops.check(L_.mhe_pad64_f32(ops._ptr(noise_rows), ops._ptr(v), R, D, s()), "mhe_pad64_f32")
    z_in = v
    logdet = torch.zeros(R, device=dev)
    per = 1 + g.num_blocks
    tape = [None] * g.num_layers
    for l in range(g.num_layers - 1, -1, -1):
        d = pk["layers"][l]
        slot = l * per
        h = ops.linear(v, d["wx"])
        ops.check(L_.mhe_glow_add_image_rows_f32(ops._ptr(h), C.c_void_p(ctab[:, slot * H:].data_ptr()), cs, R, H, N, B, s()), "mhe_glow_add_image_rows_f32")
        hs, t2s, t3s = [h], [], []
        for b, (w0, b0, w1, b1) in enumerate(d["blocks"]):
            t = torch.empty(R, H, device=dev)
            ops.check(L_.mhe_relu_copy_f32(ops._ptr(hs[-1]), ops._ptr(t), t.numel(), ops.F32, s()), "mhe_relu_copy_f32")
            t2 = ops.linear(t, w0, b0, relu=True)
            t3 = ops.linear(t2, w1, b1)
            hn = hs[-1].clone()
            ops.check(L_.mhe_glow_glu_residual_f32(ops._ptr(hn), ops._ptr(t3), ops.F32, C.c_void_p(ctab[:, (slot + 1 + b) * H:].data_ptr()), cs, R, H, N, B, s()),
                      "mhe_glow_glu_residual_f32")
            hs.append(hn); t2s.append(t2); t3s.append(t3)
        prm = ops.linear(hs[-1], d["wf"], d["bf"])
        y = torch.empty(R, g.Dp, device=dev)
        ops.check(L_.mhe_glow_coupling_f32(ops._ptr(v), ops._ptr(prm), ops._ptr(y), ops._ptr(logdet), R, D, d["first"], d["T"], 1, s()),
                  "mhe_glow_coupling_f32")
        tape[l] = {"v": v, "hs": hs, "t2": t2s, "t3": t3s, "prm": prm, "y": y}
        v = ops.linear(y, d["Ainv"], d["cinv"])
    x, lp = ops.glow_finish(z_in, v, logdet, R, D, True, pk["const_parts"])
    return x, lp, {"tape": tape, "pk": pk, "aff": aff, "ctab": ctab, "context": context, "N": N, "B": B}


def backward(g, tp, g_x, g_logq):
    """g_x (B N, D) = dL/dx (or None), g_logq (B N,) = dL/dlog_prob (or None) -> ({parameter: gradient}, dL/dcontext (B, F))"""
    L_, D, H, Fc, Lr, NB = _lib.lib(), g.features, g.hidden, g.context_features, g.num_layers, g.num_blocks
    pk, aff, ctab, N, B = tp["pk"], tp["aff"], tp["ctab"], tp["N"], tp["B"]
    R, Dp, cs, per = B * N, g.Dp, ctab.shape[1], 1 + NB
    s, dev = ops._stream, ctab.device
    gv = torch.zeros(R, Dp, device=dev)
    if g_x is not None:
        ops.check(L_.mhe_pad64_f32(ops._ptr(g_x), ops._ptr(gv), R, D, s()), "mhe_pad64_f32")
    if g_logq is not None:
        ops._chk(g_logq, torch.float32, "glow.g_log_prob", (R,))
    Gct = torch.zeros(B, cs, device=dev)
    dAinv, dcinv = torch.zeros(Lr, Dp, Dp, device=dev), torch.empty(Lr, Dp, device=dev)
    T = g._transform._transforms
    grads = {}
    for l in range(Lr):
        t, d = tp["tape"][l], pk["layers"][l]
        net = T[3 * l + 2].transform_net
        slot = l * per
        ops.linear_wgrad(t["y"], gv, dAinv[l]); _colsum(gv, B, N, dcinv[l])
        gy = ops.linear(gv, aff["AinvT"][l])
        gvc, gprm = ops.glow_coupling_inv_bwd_wide(t["v"], t["prm"], gy, g_logq, D, d["first"], d["T"])
        Pp = gprm.shape[1]
        dwf, dbf = torch.zeros(Pp, H, device=dev), torch.empty(Pp, device=dev)
        ops.linear_wgrad(t["hs"][-1], gprm, dwf); _colsum(gprm, B, N, dbf)
        grads[net.final_layer.weight], grads[net.final_layer.bias] = dwf[:2 * d["T"]], dbf[:2 * d["T"]]
        gh = ops.linear(gprm, d["wf"].t().contiguous())
        for b in range(NB - 1, -1, -1):
            blk = net.blocks[b]
            w0, _, w1, _ = d["blocks"][b]
            t2, t3 = t["t2"][b], t["t3"][b]
            gt3, ggate = torch.empty(R, H, device=dev), torch.empty(R, H, device=dev)
            ops.check(L_.mhe_glow_glu_bwd_f32(ops._ptr(gh), ops._ptr(t3), C.c_void_p(ctab[:, (slot + 1 + b) * H:].data_ptr()), cs, ops._ptr(gt3), ops._ptr(ggate),
                                              R, H, N, B, ops.F32, s()), "mhe_glow_glu_bwd_f32")
            ops.sum_row_blocks(ggate, B, N, out=Gct[:, (slot + 1 + b) * H:], out_stride=cs)
            dw1, db1 = torch.zeros(H, H, device=dev), torch.zeros(H, device=dev)
            ops.linear_wgrad(t2, gt3, dw1); ops.colsum(gt3, db1)
            gt2 = ops.linear(gt3, w1.t().contiguous())
            ops.flow_lrelu_bwd(gt2, t2, slope=0.0)
            tt = torch.empty(R, H, device=dev)
            ops.check(L_.mhe_relu_copy_f32(ops._ptr(t["hs"][b]), ops._ptr(tt), tt.numel(), ops.F32, s()), "mhe_relu_copy_f32")
            dw0, db0 = torch.zeros(H, H, device=dev), torch.zeros(H, device=dev)
            ops.linear_wgrad(tt, gt2, dw0); ops.colsum(gt2, db0)
            gt = ops.linear(gt2, w0.t().contiguous())
            ops.check(L_.mhe_relu_bwd_add_f32(ops._ptr(gh), ops._ptr(gt), ops._ptr(t["hs"][b]), gh.numel(), ops.F32, s()), "mhe_relu_bwd_add_f32")
            grads[blk.linear_layers[0].weight], grads[blk.linear_layers[0].bias] = dw0, db0
            grads[blk.linear_layers[1].weight], grads[blk.linear_layers[1].bias] = dw1, db1
        dwx = torch.zeros(H, Dp, device=dev)
        ops.linear_wgrad(t["v"], gh, dwx)
        ops.sum_row_blocks(gh, B, N, out=Gct[:, slot * H:], out_stride=cs)
        grads[net.initial_layer.weight] = dwx[:, T[3 * l + 2].identity_features]          # (context columns added below)
        gv = ops.add(gvc, ops.linear(gh, d["wx"].t().contiguous()))
    dW, db = torch.zeros(cs, Fc, device=dev), torch.zeros(cs, device=dev)
    ops.linear_wgrad(tp["context"], Gct, dW); ops.colsum(Gct, db)
    g_ctx = ops.linear(Gct, pk["wctx"].t().contiguous())
    ga = ops.glow_affine_wide_bwd(dAinv, dcinv, g_logq, Lr, D, aff["ws"]).float()
    n = D * (D - 1) // 2
    for l in range(Lr):
        an, lu, net = T[3 * l], T[3 * l + 1], T[3 * l + 2].transform_net
        r = ga[l]
        grads[an.log_scale], grads[an.shift] = r[:D], r[D:2 * D]
        grads[lu.lower_entries], grads[lu.upper_entries] = r[2 * D:2 * D + n], r[2 * D + n:2 * D + 2 * n]
        grads[lu.unconstrained_upper_diag], grads[lu.bias] = r[2 * D + 2 * n:3 * D + 2 * n], r[3 * D + 2 * n:]
        slot = l * per
        grads[net.initial_layer.weight] = torch.cat([grads[net.initial_layer.weight], dW[slot * H:(slot + 1) * H]], 1)
        grads[net.initial_layer.bias] = db[slot * H:(slot + 1) * H]
        for b, blk in enumerate(net.blocks):
            k = slot + 1 + b
            grads[blk.context_layer.weight], grads[blk.context_layer.bias] = dW[k * H:(k + 1) * H], db[k * H:(k + 1) * H]
    return grads, g_ctx
