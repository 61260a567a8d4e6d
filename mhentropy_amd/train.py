"""The reference's train step on HIP kernels, with an explicit reverse pass.

Reference (hand/CrossModalHand.py:455-470, optimizer :191-203):
    output = model(image, target); total_loss, losses, metrics = criterion(output, target)
    optimizer.zero_grad(); total_loss.backward()
    clip_grad_norm_(encoderRGB.parameters(), 1.);  optimizer.step()        # torch.optim.Adam(lr)
with total_loss = mean_b(-log_p[b]) (hand/criteria.py:55,173).

There is no autograd graph here: `TrainStep` runs the forward of MHEnt.get_loss stage by stage keeping
what the reverse pass needs (raw convolution outputs, post-activation tensors, BatchNorm batch
statistics, the flow sample), then walks the stages backwards through hand-written reverse kernels:
    loss -> MANO likelihood and the optional terms of the call (loss_terms.LossTerms.joints_bwd) -> RealNVP couplings (re-evaluated layer by layer,
    csrc/flow_bwd.hip + mhe_conv_wgrad_nhwc) -> conditioning / det-head / l1 dense layers -> ResNet trunk
    (data gradients through the forward implicit-GEMM kernel on transposed, tap-flipped weights; weight
    gradients through mhe_conv_wgrad_nhwc; train-mode BatchNorm reverse) -> clip + Adam (one fused pass).

Memory plan (sized for 288 GB HBM): arena.py - one flat parameter buffer, derived operand layouts refreshed by one gather per step,
a raw gradient arena un-packed by one gather.  The flow's part of the step: train_flow.py (RealNVP), train_glow.py (Glow).
"""
import collections
import os

import torch

from . import ops, resnet
from .arena import OperandArena, _ceil
from .loss_terms import LossTerms
from .resnet import BN_EPS, BN_MOMENTUM
from .train_flow import RealNVPPart, flow_stream_table  # noqa: F401  (flow_stream_table: named as train.flow_stream_table by its test)


def dgrad_operand_index(idx):
    """index table of the data-gradient convolution's weight operand from the index tensor of a torch conv
    weight [Cout,Cin,KH,KW]:  W'[ci][kh'][kw'][co] = W[co][ci][KH-1-kh'][KW-1-kw'], rows = Cin, k = (kh',kw',co)"""
    Cout, Cin, KH, KW = idx.shape
    return idx.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, KH * KW * Cout)


def dgrad_s2_operand_indices(idx):
    """the four parity-class operands of a 3x3 / stride-2 / pad-1 convolution's data gradient (mhe_conv3x3s2_dgrad_nhwc) as index
    tables into the torch weight [Cout,Cin,3,3]: class (py, px) -> [Cin][(th, tw, co)] with forward taps kh = (1,) for py = 0 and
    (2, 0) for py = 1 (output row 2i+py reads gy rows i + th), likewise kw"""
    Cout, Cin, KH, KW = idx.shape
    assert KH == 3 and KW == 3
    taps = ((1,), (2, 0))
    out = []
    for py in range(2):
        for px in range(2):
            sub = idx[:, :, list(taps[py])][:, :, :, list(taps[px])]            # [Cout, Cin, th, tw]
            out.append(sub.permute(1, 2, 3, 0).reshape(Cin, len(taps[py]) * len(taps[px]) * Cout))
    return out


def conv_dgrad(gy, w_dg, k, stride, pad, H, W, residual=None, mask=None, bn=None, w_s2=None, res_half=False, coarse=False, mask_bits=None):
    """gradient of a k x k / stride / pad convolution w.r.t. its [B,H,W,Cin] input (+ residual), through the
    FORWARD implicit-GEMM kernel: stride 1 is a convolution of gy with the transposed, tap-flipped weights at
    padding k-1-pad; a stride-2 3x3 runs the same on the zero-dilated gy; a stride-2 1x1 is computed on the
    coarse grid and scattered to the even positions.  mask (the convolution's own post-ReLU input): the result is
    gated by [mask > 0] in the kernel's epilogue, i.e. it leaves as the gradient w.r.t. the PRE-activation."""
    if stride == 1:
        return ops.conv2d_nhwc(gy, w_dg, k, k, 1, k - 1 - pad, residual=residual, mask=mask, bn=bn, res_half=res_half,
                               mask_bits=mask_bits if mask is not None else None)
    if stride != 2 or k not in (1, 3):
        raise NotImplementedError(f"conv_dgrad: k={k} stride={stride}")
    if k == 3 and w_s2 is not None and pad == 1 and H == 2 * gy.shape[1] and W == 2 * gy.shape[2]:
        return ops.conv3x3s2_dgrad(gy, w_s2, residual=residual, mask=mask, bn=bn)       # four parity classes, no zero-dilated copy
    if k == 3:
        return ops.conv2d_nhwc(ops.upsample2(gy, H, W), w_dg, 3, 3, 1, 1, residual=residual, mask=mask, bn=bn)
    if mask is not None:
        raise NotImplementedError("conv_dgrad: mask with a stride-2 1x1 (only the un-gated downsample branch uses it)")
    half = ops.conv2d_nhwc(gy, w_dg, 1, 1, 1, 0)
    if coarse and residual is None:     # the consumer adds it at the even positions itself (mhe_conv_desc.res_half): no scattered copy
        return half
    return ops.upsample2(half, H, W, base=residual)


def halo_operand_index(f):
    """standard 3x3 pack [Cout][9 Cin] (index table) -> the fragment-major stages of csrc/conv_halo.hip (ops.conv3x3_halo_pack on indices):
    [Cout / 128][Cin / 64][9][4 channel tiles x 4 k-steps][2 k halves x 32 rows][8]"""
    Cout, K = f.shape
    Cin = K // 9
    v = f.view(Cout // 128, 4, 32, 9, Cin // 64, 4, 2, 8)          # ntile, nt32, row, tap, chunk, ks, kg, e
    return v.permute(0, 4, 3, 1, 5, 6, 2, 7).reshape(Cout, K).contiguous()


class _Unit:
    """one convolution + BatchNorm of the trunk: its tables (fixed at construction) and what a step hangs onto it"""
    __slots__ = ("conv", "bn", "k", "stride", "pad", "cin", "cout", "cin_w", "pairs", "w_fwd", "w_dg", "w_halo", "w_dg_halo", "w_s2",
                 "raw_w", "raw_g", "raw_b", "dw", "dgamma", "dbeta",
                 "x", "y", "scale", "shift", "mi", "gram_tot", "fold_rev", "rev_stats", "rev_dummy", "y_recomputed")

    def __init__(self, conv, bn, k, stride, pad):
        self.conv, self.bn, self.k, self.stride, self.pad = conv, bn, k, stride, pad
        self.cin, self.cout = conv.in_channels, conv.out_channels
        self.cin_w, self.pairs = self.cin, False
        self.w_fwd = self.w_dg = self.w_halo = self.w_dg_halo = self.w_s2 = None
        self.raw_w = self.raw_g = self.raw_b = self.dw = self.dgamma = self.dbeta = None
        # forward: input, raw output (None: never written), BatchNorm scale / shift / (mean, invstd), the Gram totals its statistics came from
        # (None: from its output) and whether the reverse may run on them (shortcuts; conv3 decides from gram_tot)
        self.x = self.y = self.scale = self.shift = self.mi = self.gram_tot = None
        self.fold_rev = self.y_recomputed = False
        self.reset_step()

    def reset_step(self):
        """end of a reverse pass: the sums a producer's epilogue accumulated for this unit's BatchNorm reverse (rev_dummy: against the gate
        tensor instead of its output) are spent, a raw output evaluated for this pass only is dropped"""
        self.rev_stats, self.rev_dummy = None, False
        if self.y_recomputed:
            self.y, self.y_recomputed = None, False


class _Block:
    """one residual block: u = its units in order, ud = the shortcut's unit | None; per step a = its input, a_bits = [a > 0] as bits | None
    (its output is the next block's `a`; the activations inside it are its units' `x`)"""
    __slots__ = ("kind", "layer", "u", "ud", "a", "a_bits")

    def __init__(self, kind, layer, u, ud):
        self.kind, self.layer, self.u, self.ud, self.a, self.a_bits = kind, layer, u, ud, None, None


# a block tail relu(bn3(y3) + identity) left to the next block's entry kernel.  recompute: conv3 is evaluated in that kernel too -
# y = conv2's raw output, bn2 = its (scale, shift); else y = conv3's raw output
_Tail = collections.namedtuple("_Tail", "y bn2 ul idt ud recompute")


def trunk_tables(arena, trunk, conv_halo=True, stem_pairs=True):
    """the trunk's units and blocks with their operand layouts and raw-gradient slots declared on the arena (host work only).
    Returns (units, blocks); units[0] is the stem"""
    T = trunk.compute_dtype
    bke = 32 if T == torch.float32 else 64
    units = []

    def add(conv, bn, k, stride, pad, stem=False):
        u = _Unit(conv, bn, k, stride, pad)
        w = conv.weight
        Cout, Cin, KH, KW = w.shape
        idx = arena.pidx(w)
        if stem:
            wp = torch.full((64, 8, 24), -1, dtype=torch.int64)
            wp[:, :7, :21] = idx.permute(0, 2, 3, 1).reshape(64, 7, 21)
            u.w_fwd = arena.derived(wp.reshape(64, 192), T)
            u.cin_w = 4 if T == torch.float32 else 8              # channel padding of the NHWC image copy
            # bf16: the weight gradient reads the image as PIXEL PAIRS (two neighbours x 3 channels padded to 4 = one 8-channel pixel):
            # a 7 x 4 / stride (2, 1) / pad (3, 2) convolution with 224 weight columns instead of 7 x 7 x 8 = 392 of which 245 multiply
            # zeros (ops.conv_wgrad_rect); raw gradient [64][7][4][2 x 4], column kw = 2 kw' + parity - 1
            u.pairs = T != torch.float32 and stem_pairs
        else:
            kk = KH * KW * Cin
            f = torch.full((Cout, _ceil(kk, bke)), -1, dtype=torch.int64)
            f[:, :kk] = idx.permute(0, 2, 3, 1).reshape(Cout, kk)
            u.w_fwd = arena.derived(f, T)
            # data-gradient operand: W'[ci][kh'][kw'][co] = W[co][ci][KH-1-kh'][KW-1-kw']
            kd = KH * KW * Cout
            d = torch.full((Cin, _ceil(kd, bke)), -1, dtype=torch.int64)
            d[:, :kd] = dgrad_operand_index(idx)
            u.w_dg = arena.derived(d, T)
            # the 3x3 / stride-1 units also in the layout of the resident-tile kernel (csrc/conv_halo.hip), forward and data gradient
            # (layer2 / layer3: layer4's 8 x 8 maps are not taken by it, and every table here is gathered every step)
            if (KH == 3 and stride == 1 and pad == 1 and T == torch.bfloat16 and Cin % 128 == 0 and Cout % 128 == 0 and Cin <= 256 and Cout <= 256
                    and conv_halo):
                u.w_halo = arena.derived(halo_operand_index(f[:, :kk]), T)
                u.w_dg_halo = arena.derived(halo_operand_index(d[:, :kd]), T)
            if KH == 3 and stride == 2 and pad == 1:
                u.w_s2 = []
                for tbl in dgrad_s2_operand_indices(idx):
                    f2 = torch.full((Cin, _ceil(tbl.shape[1], bke)), -1, dtype=torch.int64)
                    f2[:, :tbl.shape[1]] = tbl
                    u.w_s2.append(arena.derived(f2, T))
        # raw weight gradient [Cout][KH*KW*cin_w]
        wshape = (Cout, 7 * 4 * 8 if u.pairs else KH * KW * u.cin_w)
        u.raw_w = arena.raw_slot(wshape)
        if u.pairs:
            co, ci, kh, kw = torch.meshgrid(torch.arange(Cout), torch.arange(Cin), torch.arange(7), torch.arange(7), indexing="ij")
            arena.map_grad(w, ((co * 7 + kh) * 4 + (kw + 1) // 2) * 8 + ((kw + 1) % 2) * 4 + ci + u.raw_w)
        else:
            r = torch.arange(Cout * KH * KW * u.cin_w, dtype=torch.int64).view(Cout, KH, KW, u.cin_w)[..., :Cin] + u.raw_w
            arena.map_grad(w, r.permute(0, 3, 1, 2))
        u.raw_g = arena.raw_slot((Cout,)); u.raw_b = arena.raw_slot((Cout,))
        arena.map_grad(bn.weight, torch.arange(Cout) + u.raw_g)
        arena.map_grad(bn.bias, torch.arange(Cout) + u.raw_b)

        def views():
            u.dw, u.dgamma, u.dbeta = arena.raw_view(u.raw_w, wshape), arena.raw_view(u.raw_g, (Cout,)), arena.raw_view(u.raw_b, (Cout,))
        arena.after_finalize(views)
        units.append(u)
        return u

    add(trunk.conv1, trunk.bn1, 7, 2, 3, stem=True)
    blocks = []
    for li in range(4):
        for blk in getattr(trunk, f"layer{li + 1}"):
            if blk.kind == "bottleneck":
                us = [add(blk.conv1, blk.bn1, 1, 1, 0), add(blk.conv2, blk.bn2, 3, blk.stride, 1), add(blk.conv3, blk.bn3, 1, 1, 0)]
            else:
                us = [add(blk.conv1, blk.bn1, 3, blk.stride, 1), add(blk.conv2, blk.bn2, 3, 1, 1)]
            ud = add(blk.downsample[0], blk.downsample[1], 1, blk.stride, 0) if blk.downsample is not None else None
            blocks.append(_Block(blk.kind, li + 1, us, ud))
    return units, blocks


def dense_tables(arena, lin, n_pad=None, k_pad=None):
    """tables of one nn.Linear: optional padded copy, transposed (padded) copy for the data gradient,
    raw slots for dW [Npad, Kpad] and db [Npad]"""
    N, K = lin.weight.shape
    Np, Kp = n_pad or N, k_pad or K
    wi = torch.full((Np, Kp), -1, dtype=torch.int64)
    wi[:N, :K] = arena.pidx(lin.weight)
    d = {}
    d["w"] = lin.weight.data if (Np, Kp) == (N, K) else arena.derived(wi, torch.float32)
    bi = torch.full((Np,), -1, dtype=torch.int64)
    bi[:N] = arena.pidx(lin.bias)
    d["b"] = lin.bias.data if Np == N else arena.derived(bi, torch.float32)
    d["wT"] = arena.derived(wi.t().contiguous(), torch.float32)
    d["raw_w"], d["raw_b"] = arena.raw_slot((Np, Kp)), arena.raw_slot((Np,))
    arena.map_grad(lin.weight, (torch.arange(Np * Kp, dtype=torch.int64).view(Np, Kp) + d["raw_w"])[:N, :K])
    arena.map_grad(lin.bias, torch.arange(N, dtype=torch.int64) + d["raw_b"])

    def views():
        d["dw"], d["db"] = arena.raw_view(d["raw_w"], (Np, Kp)), arena.raw_view(d["raw_b"], (Np,))
    arena.after_finalize(views)
    return d


def head_tables(arena, model):
    """(l1, det_head[0], det_head[2]); feat_extractor.l2 is dead for MHEnt (hand/network.py:779): its gradient stays zero (-1 in the
    unpack table)"""
    return (dense_tables(arena, model.feat_extractor.l1[0]), dense_tables(arena, model.det_head[0]),
            dense_tables(arena, model.det_head[2], n_pad=32))         # 16 outputs padded to the GEMM's K granule for the data gradient


class TrainStep:
    def __init__(self, model, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, dist=None, shard_hypotheses=False):
        self.model, self.lr, self.betas, self.eps, self.max_norm, self.dist = model, lr, betas, eps, max_norm, dist
        self.world = dist.get_world_size() if dist is not None else 1
        from .dist import forced
        # collectives are issued: more than one rank, or a forced group of ONE (the one-GPU rehearsal of the RCCL path, MHE_DIST_FORCE=1)
        self.comm = dist is not None and (self.world > 1 or forced())
        # hypothesis-sharded exchange (dist.HypothesisShards): images stay sharded for the encoder, every rank evaluates its
        # slice of the K hypotheses for ALL images from the gathered conditioning features
        self.shard_hypotheses = bool(shard_hypotheses) and self.comm
        trunk = model.feat_extractor.res
        self.trunk = trunk
        self.T = trunk.compute_dtype
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("TrainStep needs the model on a HIP device (there is no CPU path)")
        ar = self.arena = OperandArena(model.parameters(), self.dev)
        # (what outside code names on the train step itself)
        self.P, self.G, self.M, self.V, self.off, self.n_params, self.grad_of = ar.P, ar.G, ar.M, ar.V, ar.off, ar.n_params, ar.grad_of
        self.repack, self.sync, self.sync_all = ar.repack, ar.sync, ar.sync_all
        self.cond_bwd_bf16 = os.environ.get("MHE_COND_BWD_BF16", "1") == "1"
        # 3x3 / stride-1 units of layer2 / layer3: the resident-tile kernel (csrc/conv_halo.hip) - forward with conv1's BatchNorm + ReLU on its
        # load (the normalised tensor written once on the way, no bn_act pass); their data gradients too (MHE_CONV_HALO_DG=0: the im2col kernels)
        self.conv_halo = os.environ.get("MHE_CONV_HALO", "1") == "1"
        self.conv_halo_dg = os.environ.get("MHE_CONV_HALO_DG", "1") == "1"
        self.units, self.blocks = trunk_tables(ar, trunk, self.conv_halo, os.environ.get("MHE_STEM_WGRAD_PAIRS", "1") == "1")
        self.stem = self.units[0]
        self.l1, self.d0, self.d2 = head_tables(ar, model)
        fl = self.flow = model.q_z_giv_i
        from .flows import RealNVP
        from .glow import ConditionalGlow
        if isinstance(fl, RealNVP):
            self.part, self.glow = RealNVPPart(ar, fl, self.cond_bwd_bf16), None
            self.flow_bf16, self.flow_fused_tables = self.part.bf16, self.part.fused_tables
        elif isinstance(fl, ConditionalGlow):
            from .train_glow import GlowPart
            self.part = self.glow = GlowPart(ar, fl)        # parity unpinned (third-party class absent)
            self.flow_bf16, self.flow_fused_tables = False, False
        else:
            raise NotImplementedError(f"TrainStep: no reverse pass for {type(fl).__name__}")
        # BatchNorm-reverse sums accumulated by the data-gradient epilogues (no separate reduce pass); MHE_BN_REDUCE_FUSED=0: separate pass
        self.fuse_bn_reduce = os.environ.get("MHE_BN_REDUCE_FUSED", "1") == "1"
        self.train_recompute = os.environ.get("MHE_TRAIN_RECOMPUTE", "1") == "1"
        self.conv3_fold = os.environ.get("MHE_CONV3_FOLD", "1") == "1"
        self.conv3_fold_cat = os.environ.get("MHE_CONV3_FOLD_CAT", "1") == "1"
        self.shortcut_fold = os.environ.get("MHE_SHORTCUT_FOLD", "1") == "1"
        self.stem_bwd_two_pass = os.environ.get("MHE_STEM_BWD_TWO_PASS", "1") == "1"
        self.gate_bits = os.environ.get("MHE_GATE_BITS", "1") == "1"
        # (... with their own BatchNorm reverse on that launch's operand load: built, equal - 26.35 / 26.38 ms)
        self.halo_bn_on_load = os.environ.get("MHE_HALO_BN_ON_LOAD", "0") == "1"
        # the stem's BatchNorm + ReLU folded into its max pool, forward and reverse (ops.maxpool3x3s2_idx / maxpool3x3s2_bwd_bn)
        self.stem_pool_fused = os.environ.get("MHE_STEM_POOL_FUSED", "1") == "1"
        # the stem's BatchNorm-reverse sums from the pooled tensors (+ the raw winners kept by the forward's pool), not a walk over its output
        self.stem_pooled_sums = os.environ.get("MHE_STEM_POOLED_SUMS", "1") == "1"
        self.bn_apply_on_load = os.environ.get("MHE_BN_BWD_ON_LOAD", "1") == "1"
        self.bn_on_load_max_cin = int(os.environ.get("MHE_BN_BWD_ON_LOAD_MAXC", "128"))   # layer1 / layer2: wider layers lose more on the 128-row tile than the pass costs (measured)
        self.bn_on_load_wide = os.environ.get("MHE_BN_BWD_ON_LOAD_WIDE", "1") == "1"
        # the trunk's weight gradients queued per gradient bucket and launched together (MHE_WGRAD_MULTI=0: one launch per layer)
        self.wgrad_multi = os.environ.get("MHE_WGRAD_MULTI", "1") == "1"
        self._wq = []
        self._bucket_bounds = self._gradient_buckets()
        self._xchg = None
        ar.finalize()
        self.raw = ar.raw
        self.step_t = torch.zeros(1, device=self.dev, dtype=torch.int32)
        self._zeros_c = torch.zeros(4096, device=self.dev, dtype=torch.float32)
        self.sq = torch.zeros(1, device=self.dev, dtype=torch.float32)
        # per step: the heads' tape, the stem's tensors, the last block's output, the reverse pass's sum arena; _capture: a capturing GraphedStep
        self.tape = self.x_nhwc = self.r0 = self.pool_idx = self.pool_win = self.pool_out = self.a_last = self._rev_pool = self._capture = None
        self.n_fold, self.n_fold_ds, self.last_grad_scale, self._G_averaged = 0, 0, None, False
        ar.repack()
        # the trunk's own forward paths (eval, sample) read the same device-resident operand packs: no host re-pack, never stale
        self.trunk._external_w = {id(u.conv.weight): u.w_fwd for u in self.units}
        self.trunk._external_sync = ar.sync

    _flow_kept = property(lambda self: self.part.kept)                  # (tests: the RealNVP part's kept activations,
    z0_recovered = property(lambda self: self.part.z0_recovered)        #  the flow input its reverse pass arrived at)

    # ------------------------------------------------------------------ gradient buckets
    def _gradient_buckets(self):
        """flat-buffer ranges in the order the reverse pass completes them: [l1, l2, flow, det head] (done before the trunk's
        reverse pass starts), layer4, layer3, [stem, layer1, layer2].  Each range is un-packed and handed to RCCL as soon as
        it is complete, so its all-reduce runs under the rest of the reverse pass."""
        t = self.trunk
        first = lambda mod: self.off[id(next(mod.parameters()))]
        cuts = [0, first(t.layer3), first(t.layer4), self.off[id(self.model.feat_extractor.l1[0].weight)], self.n_params]
        return [(cuts[i], cuts[i + 1]) for i in range(4)]           # index 3 = ready first ... index 0 = ready last

    def _grad_ready(self, i):
        lo, hi = self._bucket_bounds[i]
        self._wgrad_flush()              # the bucket's queued weight gradients, one multi-problem launch per tile shape
        ops.gather(self.raw, self.arena.unpack_idx[lo:hi], self.G[lo:hi])
        if self.comm:
            cap = self._capture
            if cap is not None:              # GraphedStep: the graph ends here, the collective is issued between two graph launches
                cap.cut(("allreduce", i))
            else:
                self._all_reduce_bucket(i)

    def _all_reduce_bucket(self, i):
        """hand bucket i of the flat gradient to the communicator (dist.GradExchange: event-scoped, on its own stream; f32 all-reduce or the
        bf16 all-to-all + all-gather exchange with f32 accumulation)"""
        lo, hi = self._bucket_bounds[i]
        if self._xchg is None:
            from .dist import GradExchange
            self._xchg = GradExchange(self.dist, device=self.dev)
        self._xchg.start(self.G[lo:hi], key=i)

    @property
    def _works(self):           # (tests: how many bucket exchanges are in flight)
        return [None] * (self._xchg.in_flight() if self._xchg is not None else 0)

    def finish_allreduce(self):
        """wait for the gradient buckets' exchanges (sum over ranks; the mean is taken by grad_scale = 1/world)"""
        cap = self._capture
        if cap is not None and self.comm:
            cap.cut(("wait",))
            return
        if self._xchg is not None:
            self._xchg.finish()

    # ------------------------------------------------------------------ trunk forward / backward
    def _unit_fwd(self, u, x, pool):
        st = pool.take(u.cout)
        y = ops.conv2d_nhwc(x, u.w_fwd, u.k, u.k, u.stride, u.pad, stats=st)
        return self._bn_tape(u, x, y, st)

    def _bn_tape(self, u, x, y, st):
        count = y.numel() // u.cout
        bn = u.bn
        u.scale, u.shift, u.mi = ops.bn_finalize(st, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, count, BN_MOMENTUM,
                                                 BN_EPS, want_mean_invstd=True, clear=True, num_batches_tracked=bn.num_batches_tracked)
        u.x, u.y = x, y
        return y

    def _block_entry(self, b, a, y, st):
        """what the two fused block tails share once their kernel has run (a: the previous block's output = this block's input, y: conv1's
        raw output): conv1's BatchNorm, then its activation by a pass - or left to conv2's operand load.  Returns (h | None, raw_prev | None)"""
        u0 = b.u[0]
        self._bn_tape(u0, a, y, st)
        b.a = a
        if self._halo_ok(b.u[1], y):      # conv2 normalises its operand on its own load and writes it out on the way
            return None, (y, u0)
        return ops.bn_act(y, u0.scale, u0.shift, relu=True), None

    def _trunk_forward(self, x):
        T = self.T
        pool = self.trunk._stats_pool(self.dev)       # self-cleaning arena shared with the module's own forward
        u = self.stem
        if u.pairs:
            if x.shape[3] % 2 or x.shape[2] % 2:
                raise ValueError("TrainStep (bf16): the stem's weight gradient reads pixel pairs - even image sizes only (MHE_STEM_WGRAD_PAIRS=0 lifts this)")
            self.x_nhwc = ops.nchw_to_nhwc(x, T, cpad=4).view(x.shape[0], x.shape[2], x.shape[3] // 2, 8)
        else:
            self.x_nhwc = ops.nchw_to_nhwc(x, T)
        st = pool.take(64)
        y0 = ops.stem_conv7x7s2(x, u.w_fwd, T, stats=st)
        self._bn_tape(u, self.x_nhwc, y0, st)
        if self.stem_pool_fused:
            # pool straight from the raw stem output, BatchNorm + ReLU on the load: the normalised full-resolution copy is never written
            if self.stem_pooled_sums:       # ... and keep the raw winners: the reverse pass takes the BatchNorm-reverse sums from the pooled tensors
                a, self.pool_idx, self.pool_win = ops.maxpool3x3s2_idx_win(y0, u.scale, u.shift)
                self.pool_out = a
            else:
                a, self.pool_idx = ops.maxpool3x3s2_idx(y0, u.scale, u.shift)
            self.r0 = None
        else:
            self.r0 = ops.bn_act(y0, u.scale, u.shift, relu=True)
            a, self.pool_idx = ops.maxpool3x3s2_idx(self.r0)
        pending = None          # _Tail: the previous block's tail, not yet evaluated
        raw_prev = None         # (conv1's raw output, its unit): normalisation left to conv2's operand load
        fuse = self.trunk.fuse_tail
        for bi, b in enumerate(self.blocks):
            us = b.u
            if pending is not None:
                p, u0, pending = pending, us[0], None
                st = pool.take(u0.cout)
                if p.recompute:
                    # ... with the previous block's conv3 evaluated again inside the same kernel: its raw output was never written (the reverse
                    # pass evaluates it once more when it gets there, _ensure_y)
                    # (+ [a > 0] as bits: the reverse pass's gate at a sixteenth of a's bytes, MHE_GATE_BITS=0: it reads a)
                    a, y, abits = ops.bottleneck_tail(p.y, p.bn2, p.ul.w_fwd, (p.ul.scale, p.ul.shift), p.idt,
                                                      None if p.ud is None else (p.ud.scale, p.ud.shift), u0.w_fwd, stats=st, want_bits=True)
                    b.a_bits = abits if self.gate_bits else None
                else:
                    # relu(bn3(y3) + identity) of the previous block is evaluated inside this conv1's operand load, which also
                    # writes it out once (this block's input / identity and the reverse pass's ReLU mask): one read of the widest
                    # tensor of the block saved, as in the inference path (resnet.py)
                    a = torch.empty_like(p.y)
                    y = ops.conv1x1_residual_in(p.y, p.idt, u0.w_fwd, p.ul.scale, p.ul.shift, None if p.ud is None else p.ud.scale,
                                                None if p.ud is None else p.ud.shift, a_out=a, stats=st)
                    b.a_bits = None
                h, raw_prev = self._block_entry(b, a, y, st)
                rest = us[1:-1]
            else:
                b.a, b.a_bits = a, None
                h = a
                rest = us[:-1]
            ul = us[-1]
            nxt = self.blocks[bi + 1] if bi + 1 < len(self.blocks) else None
            h_by_gram = False
            for u in rest:
                if raw_prev is not None:
                    y1, up = raw_prev
                    raw_prev = None
                    h = torch.empty_like(y1)
                    st = pool.take(u.cout)
                    y = ops.conv3x3_halo(y1, u.w_halo, up.scale, up.shift, relu_in=True, a_out=h, stats=st)
                    self._bn_tape(u, h, y, st)
                else:
                    y = self._unit_fwd(u, h, pool)
                # conv2's output of a block whose conv3 runs on Gram statistics: the Gram launch below reads it raw anyway and writes the
                # normalised tensor on the way (no bn_act pass of its own)
                h_by_gram = (u is us[-2] and self._foldable(b, nxt, us, y) and (self.conv3_fold and self.fuse_bn_reduce or
                             ops.bottleneck_tail_supported(y.shape[0], y.shape[1], y.shape[2], y.shape[3], nxt.u[0].cout)))
                h = torch.empty_like(y) if h_by_gram else ops.bn_act(y, u.scale, u.shift, relu=True)
            # layer1 / layer2 bottlenecks (bf16, 64 / 128 bottleneck channels): conv3 is not run here at all - bn3's batch statistics come
            # from the Gram matrix of its input, the tail kernel of the next block evaluates it on the fly (as the module's own forward
            # does, resnet.py), and the reverse pass evaluates it once when it needs it: a write + a read of the block's widest tensor
            # traded for one plain 1x1 launch in the reverse pass (MHE_TRAIN_RECOMPUTE=0: conv3 written in the forward pass)
            foldable = self._foldable(b, nxt, us, h)
            recompute = foldable and ops.bottleneck_tail_supported(h.shape[0], h.shape[1], h.shape[2], h.shape[3], nxt.u[0].cout)
            # (a block whose tail the fused kernel cannot take - layer2's last, which feeds layer3 - still runs conv3 for the forward's sake,
            # but on the Gram statistics as well, so that the REVERSE pass can do without y3: it is dropped from the tape)
            semi = foldable and not recompute and self.conv3_fold and self.fuse_bn_reduce
            if recompute or semi:
                u2, bn3 = us[-2], ul.bn
                gbufs = pool.gram(ul.cin)
                if self.conv3_fold:      # the Gram totals of THIS block stay for the reverse pass (csrc/conv_fold.hip)
                    tot = self.arena.workspace(("gram_tot", bi), lambda: ops.gram_workspace(ul.cin, self.dev))
                    gbufs, ul.gram_tot = (gbufs[0], tot), tot
                else:
                    ul.gram_tot = None
                ul.scale, ul.shift, ul.mi = ops.conv1x1_gram_bn(u2.y, u2.scale, u2.shift, ul.w_fwd, bn3.weight.data, bn3.bias.data, bn3.running_mean,
                                                                bn3.running_var, gbufs, BN_MOMENTUM, BN_EPS,
                                                                num_batches_tracked=bn3.num_batches_tracked, want_mean_invstd=True,
                                                                a_out=h if h_by_gram else None)
                ul.x, ul.y = h, None
                yl = ops.conv2d_nhwc(h, ul.w_fwd, 1, 1, 1, 0) if semi else None
            else:
                yl = self._unit_fwd(ul, h, pool)
            ud = b.ud
            yd = self._shortcut_fwd(bi, b, ud, pool) if ud is not None else None
            idt = yd if ud is not None else b.a
            if recompute:
                pending = _Tail(us[-2].y, (us[-2].scale, us[-2].shift), ul, idt, ud, True)
                continue
            if fuse and nxt is not None and nxt.kind == "bottleneck" and b.kind == "bottleneck":
                pending = _Tail(yl, None, ul, idt, ud, False)
                continue
            if ud is not None:
                a = ops.bn_act(yl, ul.scale, ul.shift, yd, ud.scale, ud.shift, relu=True)
            else:
                a = ops.bn_act(yl, ul.scale, ul.shift, b.a, relu=True)
        pool.done()
        self.a_last = a
        return ops.avgpool(a)

    def _bn_bwd(self, u, g, a, pool, stats=None):
        """g: gradient w.r.t. the unit's BatchNorm OUTPUT (already ReLU-gated by its producer when a is None).  stats: the
        reverse sums already accumulated by the producer's epilogue (then only finalize + apply run here)."""
        return ops.bn_backward(g, a, u.y, u.mi, u.bn.weight.data, stats if stats is not None else pool.take(u.cout), u.dgamma, u.dbeta,
                               reduced=stats is not None)

    def _bn_bwd_coef(self, u, g, pool):
        """dgamma / dbeta and the coefficients of the unit's BatchNorm reverse, which its data-gradient launch applies on its operand load"""
        rs = u.rev_stats
        return ops.bn_backward(g, None, u.y, u.mi, u.bn.weight.data, rs if rs is not None else pool.take(u.cout), u.dgamma, u.dbeta,
                               reduced=rs is not None, coef_only=True)

    def _rev_sums_of(self, cons, pool):
        """(raw output, mean_invstd, sums) of the BatchNorm unit that consumes the gradient a launch is about to produce: its reverse sums
        are accumulated by that launch's epilogue (None: by a pass of their own)"""
        if not self.fuse_bn_reduce:
            return None
        cons.rev_stats = pool.take(cons.cout)
        return (cons.y, cons.mi, cons.rev_stats)

    def _shortcut_fwd(self, bi, b, ud, pool):
        """the block's shortcut convolution + its BatchNorm's batch statistics.  Layer1's (1x1, stride 1, 64 input channels): the statistics
        from the Gram matrix of the block's input, whose totals stay for the reverse pass - there the BatchNorm reverse then needs neither the
        shortcut's raw output nor a pass of its own over three block-wide tensors (csrc/conv_fold.hip, as for conv3; MHE_SHORTCUT_FOLD=0: as the others)"""
        a = b.a
        ud.fold_rev = False
        if not (self.shortcut_fold and self.conv3_fold and self.fuse_bn_reduce and ud.k == 1 and ud.stride == 1 and ud.cin in (64, 128)
                and a.dtype == torch.bfloat16 and (a.numel() // ud.cin) % 128 == 0 and bi + 1 < len(self.blocks) and self.blocks[bi + 1].ud is None
                and self.blocks[bi + 1].u[0].k == 1):
            return self._unit_fwd(ud, a, pool)
        tot = self.arena.workspace(("gram_tot_ds", bi), lambda: ops.gram_workspace(ud.cin, self.dev))
        ones = self.arena.workspace("ones_c", lambda: torch.ones(4096, device=self.dev))
        bn = ud.bn
        ud.scale, ud.shift, ud.mi = ops.conv1x1_gram_bn(a, ones[:ud.cin], self._zeros_c[:ud.cin], ud.w_fwd, bn.weight.data, bn.bias.data,
                                                        bn.running_mean, bn.running_var, (pool.gram(ud.cin)[0], tot), BN_MOMENTUM, BN_EPS,
                                                        num_batches_tracked=bn.num_batches_tracked, want_mean_invstd=True)
        ud.gram_tot, ud.fold_rev = tot, True
        ud.x = a
        ud.y = ops.conv2d_nhwc(a, ud.w_fwd, 1, 1, 1, 0)
        return ud.y

    def _halo_ok(self, u, x):
        return (self.conv_halo and u.w_halo is not None and u.k == 3 and u.stride == 1 and x.dtype == torch.bfloat16
                and ops.conv3x3_halo_supported(x.shape[0], x.shape[1], x.shape[2], u.cin, u.cout))

    def _foldable(self, b, nxt, us, h):
        """a bottleneck of layer1 / layer2 whose conv3 + bn3 can run on the Gram statistics of conv3's input (h: that input, or conv2's raw
        output - same shape)"""
        ul = us[-1]
        return (self.train_recompute and self.trunk.fuse_tail and nxt is not None and nxt.kind == "bottleneck" and b.kind == "bottleneck"
                and len(us) == 3 and ul.k == 1 and ul.stride == 1 and h.dtype == torch.bfloat16 and us[-2].y is not None
                and nxt.u[0].k == 1 and nxt.u[0].stride == 1 and ul.cin in (64, 128) and (h.numel() // ul.cin) % 128 == 0)

    def _ensure_y(self, u):
        """the raw output of a unit whose forward launch was skipped (conv3 of a layer1 / layer2 bottleneck): evaluated now, bit-identical
        to what the fused tail kernel worked with"""
        if u.y is None:
            u.y = ops.conv2d_nhwc(u.x, u.w_fwd, u.k, u.k, u.stride, u.pad)
            u.y_recomputed = True
        return u.y

    def _wgrad(self, u, gy):
        """dW of a trunk unit.  bf16 trunk: QUEUED - a gradient bucket's weight gradients do not depend on one another, so they are launched
        together when the bucket completes (ops.conv_wgrad_multi: the layers share the chip, every pixel range is cut 4 - 8 ways instead of
        28 - 64, layer4 not at all - the partial-slab traffic of one launch per layer, 5.4 GB of the step's 98 GB, falls accordingly).  The
        queue holds x and gy alive; nothing in the reverse pass writes into either after this point (gy is this unit's own tensor, x a
        forward activation)."""
        if self.wgrad_multi and gy.dtype == torch.bfloat16:
            self._wq.append((u.x, gy, u.k, u.k, u.stride, u.pad, u.dw))
        else:
            ops.conv_wgrad(u.x, gy, u.k, u.k, u.stride, u.pad, u.dw)

    def _wgrad_flush(self):
        if self._wq:
            ops.conv_wgrad_multi(self._wq)
            self._wq = []

    def _dgrad(self, u, gy, residual=None, gate=True, consumers=(), pool=None, res_half=False, coarse=False, mask_bits=None):
        """gradient w.r.t. the pre-activation of the unit's input (+ residual): every unit input in the trunk is a post-ReLU
        tensor, so the ReLU gate [x > 0] is applied in the producing kernel's epilogue and the BatchNorm reverse passes
        downstream read one tensor less"""
        bn = None
        if gate and consumers and self.fuse_bn_reduce:
            # the BatchNorm units that consume this gradient: their reverse sums are accumulated by this kernel's epilogue
            # (a unit whose raw output was never written and whose reverse runs on the Gram statistics, csrc/conv_fold.hip, needs sum g only:
            # the gate tensor - same shape, read by this epilogue anyway - stands in for its output; the second sum is not used)
            dummy = [c.y is None or c.fold_rev for c in consumers]
            bn = [(u.x if dm else c.y, c.mi, pool.take(c.cout)) for c, dm in zip(consumers, dummy)]
            for c, (_, _, st), dm in zip(consumers, bn, dummy):
                c.rev_stats = st
                c.rev_dummy = dm
        if (self.conv_halo_dg and gate and residual is None and mask_bits is None and len(consumers) <= 1 and u.w_dg_halo is not None
                and u.k == 3 and u.stride == 1 and gy.dtype == torch.bfloat16
                and ops.conv3x3_halo_supported(gy.shape[0], gy.shape[1], gy.shape[2], u.cout, u.cin)):
            return ops.conv3x3_halo(gy, u.w_dg_halo, mask=u.x, bn=None if bn is None else bn[0])
        return conv_dgrad(gy, u.w_dg, u.k, u.stride, u.pad, u.x.shape[1], u.x.shape[2], residual, u.x if gate else None, bn,
                          w_s2=u.w_s2, res_half=res_half, coarse=coarse, mask_bits=mask_bits)

    def _fold_reverse(self, u, g, names, cat):
        """conv + BatchNorm of unit u reversed on the forward's Gram statistics (csrc/conv_fold.hip): D = g^T x by a weight-gradient launch,
        then dW / dgamma / dbeta and the operands of the data-gradient launch(es) out of the fold.  Returns those operands (weights
        [(k2 W)^T | W^T diag(k1) W] if cat else (k2 W)^T, the Cb x Cb factor | None, the constant row), in workspace buffers named `names`..."""
        Cn, Cb = u.cout, u.cin
        D = self.arena.workspace(("foldD", Cn, Cb), lambda: torch.zeros(Cn, Cb, device=self.dev))      # cleared by the fold kernel on its way out
        ops.conv_wgrad(u.x, g, 1, 1, 1, 0, D)
        buf, bf = self.arena.buf, torch.bfloat16
        fw = (buf(f"{names}wcat{Cn}", (Cb, Cn + Cb), bf) if cat else buf(f"{names}wdg{Cn}", (Cb, Cn), bf),
              None if cat else buf(f"{names}S{Cb}", (Cb, Cb), bf), buf(f"{names}c0{Cb}", (Cb,)))
        ops.conv3_bn_fold(D, u.w_fwd, u.gram_tot, u.rev_stats, u.bn.weight.data, u.mi, g.numel() // Cn, u.dgamma, u.dbeta, u.dw,
                          fw[0], fw[1], fw[2], buf(f"{names}coef{Cn}", (2 * Cn,)))
        return fw

    def _trunk_backward(self, g_f):
        # the reverse pass's BatchNorm sums: ONE arena kept across steps; a pass zeroes the slice the previous pass used (ResNet-50 takes
        # ~27k channels = 55 MB of fixed-point words; round 4 allocated and zeroed a fresh 134 MB arena every step - and every graph replay)
        pool = self._rev_pool
        if pool is None:
            pool = self._rev_pool = resnet._StatsPool(self.dev, channels=65536, persistent=True)
            pool.high = 0
        else:
            pool.buf[:pool.high].zero_()
        pool.off = 0
        self.n_fold = 0                 # blocks whose conv3 + bn3 were reversed on the Gram statistics in this pass
        self.n_fold_ds = 0              # ... and shortcuts
        B, Hh, Ww, Cc = self.a_last.shape
        # g is always the gradient w.r.t. the block output's PRE-ReLU value: the gate is applied where g is produced
        g = ops.avgpool_bwd(g_f, Hh * Ww, self.T, mask=self.a_last.view(B, Hh * Ww, Cc)).view(B, Hh, Ww, Cc)
        for bi in range(len(self.blocks) - 1, -1, -1):
            b = self.blocks[bi]
            if bi + 1 < len(self.blocks) and self.blocks[bi + 1].layer != b.layer and self.blocks[bi + 1].layer >= 3:
                self._grad_ready(self.blocks[bi + 1].layer - 2)      # layer4 complete -> bucket 2, layer3 -> bucket 1
            us, ud = b.u, b.ud
            ul = us[-1]
            # conv3 + bn3 reversed on the forward's Gram statistics (layer1 / layer2, csrc/conv_fold.hip): neither y3 nor gy3 exists
            fold = ul.y is None and ul.gram_tot is not None and ul.rev_stats is not None and ul.rev_dummy and self.fuse_bn_reduce
            if not fold:
                self._ensure_y(ul)
            # bottleneck conv3 (1x1, stride 1): its BatchNorm reverse is applied in the operand load of its own data gradient
            # (ops.conv1x1_dgrad_bn_apply) instead of by a pass over three block-wide tensors
            # (the register-staged kernel pays for it up to 128 bottleneck channels; the wide layers take it where the transfer-wave
            # kernel, csrc/conv_tail.hip, runs their data gradient)
            on_load = self.bn_apply_on_load and len(us) == 3 and ul.k == 1 and ul.stride == 1 and (
                ul.cin <= self.bn_on_load_max_cin or (self.bn_on_load_wide and ops.conv_tile_choice(
                    g.shape[0], g.shape[1], g.shape[2], ul.cout, ul.cin, 1, 1, 0, g.dtype, 2) == 10))
            if fold:
                self.n_fold += 1
                # [(k2 W)^T | W^T diag(k1) W]: the weights of one data-gradient launch on [g | A] (MHE_CONV3_FOLD_CAT=0: two launches, the
                # Cb x Cb product on A as the residual of the one on g)
                fw = self._fold_reverse(ul, g, "fold_", self.conv3_fold_cat)
                gy = None
            elif on_load:
                coef = self._bn_bwd_coef(ul, g, pool)
                gy = None
            else:
                gy = self._bn_bwd(ul, g, None, pool, stats=ul.rev_stats)
            if ud is not None and ud.fold_rev and ud.rev_stats is not None and ud.rev_dummy:
                # the shortcut likewise, on the Gram statistics of the block's input, then ONE ungated data-gradient launch on [g | a]
                # (buffers of its own: conv3's fold of this block has run already, its data-gradient launch - further down - has not)
                wcat, _, c0 = self._fold_reverse(ud, g, "fold_ds_", True)
                self.n_fold_ds += 1
                skip = ops.conv2d_nhwc(g, wcat, 1, 1, 1, 0, xcat=ud.x, out_shift=c0)
                half_skip = False
            elif ud is not None:
                gyd = self._bn_bwd(ud, g, None, pool, stats=ud.rev_stats)
                self._wgrad(ud, gyd)
                # summed with the main branch before the gate; a stride-2 shortcut's gradient stays on its coarse grid and the main
                # branch's data gradient adds it at the even positions (bottleneck: conv1 is 1x1 stride 1, so that launch takes it)
                half_skip = ud.stride == 2 and ud.k == 1 and us[0].stride == 1 and bi > 0
                skip = self._dgrad(ud, gyd, gate=False, coarse=half_skip)
            else:
                skip = g
            for j in range(len(us) - 1, 0, -1):
                u = us[j]
                if isinstance(gy, tuple):
                    # a 3x3 unit of layer2 / layer3: its BatchNorm reverse applied on the operand load of its own data gradient (the
                    # resident-tile kernel's transfer waves, csrc/conv_halo.hip), gy written on the way for the weight gradient
                    graw, coef = gy
                    gy = torch.empty_like(graw)
                    ga = ops.conv3x3_halo_dgrad_bn(graw, u.y, coef, u.w_dg_halo, u.x, gy_out=gy, bn=self._rev_sums_of(us[j - 1], pool))
                    self._wgrad(u, gy)
                elif gy is None:                             # conv3 with its BatchNorm reverse on load
                    bn = self._rev_sums_of(us[j - 1], pool)
                    bn = None if bn is None else [bn]
                    if fold:
                        # gy3 W = g (k2 W) + A (W^T diag(k1) W) + k0^T W: the Cb x Cb product on conv3's input as the residual, the constant
                        # as the bias of ONE data-gradient launch on g; the weight gradient came out of the fold
                        if fw[1] is None:
                            ga = ops.conv2d_nhwc(g, fw[0], 1, 1, 1, 0, mask=u.x, bn=bn, out_shift=fw[2], xcat=u.x)
                        else:
                            t_res = ops.conv2d_nhwc(u.x, fw[1], 1, 1, 1, 0)
                            ga = ops.conv2d_nhwc(g, fw[0], 1, 1, 1, 0, residual=t_res, mask=u.x, bn=bn, out_shift=fw[2])
                    else:
                        gy = torch.empty_like(g)
                        ga = ops.conv1x1_dgrad_bn_apply(g, u.y, coef, u.w_dg, gy, u.x, bn, zeros=self._zeros_c[:u.cout])
                        self._wgrad(u, gy)
                else:
                    self._wgrad(u, gy)
                    ga = self._dgrad(u, gy, consumers=(us[j - 1],), pool=pool)
                nu = us[j - 1]
                if (j - 1 >= 1 and self.conv_halo_dg and self.halo_bn_on_load and nu.w_dg_halo is not None and nu.k == 3
                        and nu.stride == 1 and ga.dtype == torch.bfloat16
                        and ops.conv3x3_halo_supported(ga.shape[0], ga.shape[1], ga.shape[2], nu.cout, nu.cin)):
                    gy = (ga, self._bn_bwd_coef(nu, ga, pool))
                else:
                    gy = self._bn_bwd(nu, ga, None, pool, stats=nu.rev_stats)
            self._wgrad(us[0], gy)
            first = bi == 0            # the first block's input is the max-pooled stem output (>= 0; the pool's reverse gates it)
            prev = self.blocks[bi - 1] if bi else None
            if prev is not None and not (self.conv3_fold and self.fuse_bn_reduce and prev.u[-1].gram_tot is not None):
                self._ensure_y(prev.u[-1])
            cons = () if first else tuple(x for x in (prev.u[-1], prev.ud) if x is not None)
            g = self._dgrad(us[0], gy, residual=skip, gate=not first, consumers=cons, pool=pool, res_half=ud is not None and half_skip,
                            mask_bits=b.a_bits)
        for u in self.units:
            u.reset_step()
        u = self.stem
        if self.stem_pool_fused:
            # pool scatter + ReLU gate (recomputed from the raw output) + the BatchNorm-reverse sums in one pass
            st = pool.take(u.cout)
            if self.stem_bwd_two_pass:
                # the same walk twice - sums, then the BatchNorm reverse applied where the scattered gradient is formed: that gradient (as
                # large as the stem's output: 0.54 GB at C2) is never written or read back (MHE_STEM_BWD_TWO_PASS=0: one walk + an apply pass)
                if self.stem_pooled_sums:   # the sums from the pooled tensors (the gradient is non-zero at the pool's winners only): no first walk
                    ops.pooled_bn_sums(g, self.pool_out, self.pool_win, u.mi, st)
                else:
                    ops.maxpool3x3s2_bwd_bn(g, self.pool_idx, u.y, u.scale, u.shift, u.mi, st, want_gx=False)
                coef = ops.bn_bwd_coef(st, u.bn.weight.data, u.mi, u.dgamma, u.dbeta, u.y.numel() // u.cout)
                gy0 = ops.maxpool3x3s2_bwd_bn_apply(g, self.pool_idx, u.y, u.scale, u.shift, u.mi, coef)
            else:
                g_r0 = ops.maxpool3x3s2_bwd_bn(g, self.pool_idx, u.y, u.scale, u.shift, u.mi, st)
                gy0 = self._bn_bwd(u, g_r0, None, pool, stats=st)
        else:
            g_r0 = ops.maxpool3x3s2_bwd(g, self.pool_idx, self.r0.shape[1], self.r0.shape[2])
            gy0 = self._bn_bwd(u, g_r0, self.r0, pool)
        if u.pairs:
            ops.conv_wgrad_rect(self.x_nhwc, gy0, 7, 4, 2, 1, 3, 2, u.dw)
        else:
            ops.conv_wgrad(self.x_nhwc, gy0, 7, 7, 2, 3, u.dw)
        self._grad_ready(0)

    # ------------------------------------------------------------------ the step
    def forward(self, x, y, noise=None, N=None, trunk_out=None, mods=None, chamfer_w=None, sil_w=None, sil_occluder=None):
        """forward of MHEnt.get_loss (hand/network.py:760-831) keeping what the reverse pass needs.  Returns the get_loss dict.
        trunk_out (B, feat_dim) f32 (testing aid): stands in for the ResNet trunk's output, whose forward and reverse
        passes are then skipped - the reference's golden gradients are pinned from the trunk feature on.
        mods: get_loss's likelihoods (None = ['uv']; ['xyz'] / ['xyz', 'uv'] read y['pose3d'], hand/CrossModalHand.py:354).
        chamfer_w: get_loss's weight of the hand-object Chamfer term (None: the model's chamfer_w; > 0 reads y['object_verts'], 'scale',
        'original_pose3d' and, if present, 'object_count'; 0 launches what the step launched without the argument).
        sil_w: get_loss's weight of the silhouette term (None: the model's sil_w; > 0 reads y['hand_mask']; 0 launches what the step launched
        without the argument).  Between forward and reverse the term keeps z, the mesh (N*B x 778 x 3 f32) and the kept-pixel list; no index
        tensor exists: the reverse re-evaluates both minima (ops.silhouette_dist_grad).
        sil_occluder: get_loss's (None: the model's sil_occluder); on, the term reads y['object_mask'] as its occluder and keeps the length of
        the list's two sections next to the list."""
        m = self.model
        N = N or m.loss_N
        B = x.shape[0] if trunk_out is None else trunk_out.shape[0]
        terms = LossTerms(m, y, mods, chamfer_w, sil_w, B, who="TrainStep.forward", sharded=self.shard_hypotheses, sil_occluder=sil_occluder)
        self.arena.sync()     # someone else (torch.optim, load_state_dict) may have written the parameters
        f = self._trunk_forward(x.contiguous()) if trunk_out is None else trunk_out.contiguous()
        feat, feat_b = ops.linear(f, self.l1["w"], self.l1["b"], want_bf16=True) if self.flow_bf16 else (ops.linear(f, self.l1["w"], self.l1["b"]), None)
        hs, B_own, N_all, feat_own = None, B, N, feat
        if self.shard_hypotheses:
            if self.glow is not None:
                raise NotImplementedError("hypothesis sharding is wired for the RealNVP branch")
            from .dist import HypothesisShards
            hs = HypothesisShards(self.dist, N)
            feat_own, feat = feat, hs.gather_rows(feat)                       # (world*B, 512): every image's conditioning feature
            feat_b = None
            terms.gather(hs)
            if noise is not None:
                noise = hs.gather_hypothesis_rows(noise.reshape(N * B, 45), B)
            lo, hi = hs.hypotheses()
            N, B = hi - lo, feat.shape[0]                                      # local hypotheses x all images
        hd = ops.linear(feat, self.d0["w"], self.d0["b"], relu=True)
        det = ops.linear(hd, self.d2["w"], self.d2["b"])[:, :16].contiguous()
        th45, log_q = self.part.sample(feat, feat_b, N, B, noise, lambda nz: m._noise(N * B, 1.0, nz, self.dev))
        blob = m.mano_dec.table_blob()
        o = terms.joints(th45, det, blob)
        share = None
        if hs is not None:
            def share(q_log_p, hq, ch):
                # means over the local hypotheses -> sums -> all-reduce -> means over all K; each rank reports its own images
                part = torch.stack([q_log_p, hq] + ([ch] if ch is not None else [])) * (float(N) / N_all)
                hs.reduce_images(part)
                own = slice(hs.rank * B_own, (hs.rank + 1) * B_own)
                return part[0, own].contiguous(), part[1, own].contiguous(), None if ch is None else part[2, own].contiguous()
        out = terms.reduce(o, log_q if m.entropy else None, N, B, share)
        self.tape = {"f": f, "feat": feat, "hd": hd, "det": det, "th45": th45, "blob": blob, "terms": terms, "sil": terms.sil, "sil_all": terms.sil_all, "z": o.get("z"),
                     "sil_verts": terms.sil_verts, "sil_logs_t": terms.sil_logs_t, "N": N, "B": B, "trunk": trunk_out is None, "hs": hs, "B_own": B_own,
                     "N_all": N_all, "feat_own": feat_own}
        return out

    def backward(self, g_log_p=None):
        """reverse pass of the last forward() for d loss / d log_p = g_log_p (B,) - default -1/B, the reference's
        total = mean_b(-log_p[b]) (hand/criteria.py:55,173); fills self.G."""
        m, t = self.model, self.tape
        N, B, f, feat, hd, det, th45 = t["N"], t["B"], t["f"], t["feat"], t["hd"], t["det"], t["th45"]
        hs, B_own, N_all = t["hs"], t["B_own"], t["N_all"]
        self._wq = []                   # (a reverse pass that raised half way must not leave its queued weight gradients to the next one)
        self.raw.zero_()
        g_logp = self.arena.buf("g_logp", (B,))
        if g_log_p is None:
            g_logp.fill_(-1.0 / B_own)          # per-rank mean over its own images; the ranks' gradients are averaged (/ world)
        elif hs is not None:
            g_logp.copy_(hs.gather_rows(g_log_p.reshape(B_own).contiguous()))
        else:
            g_logp.copy_(g_log_p.reshape(B))
        g45, gdet_rows = t["terms"].joints_bwd(th45, det, t["blob"], g_logp, N_all,
                                               out=(self.arena.buf("g45", (N * B, 45)), self.arena.buf("gdet_rows", (N * B, 16))))
        if t["sil"] is not None:
            self._sil_bwd(t, g_logp, g45, gdet_rows)
        self.part.reverse(th45, g45, g_logp if m.entropy else None, N, B, N_all)
        # det head: gdet [B,16] -> padded [B,32]
        gdet = self.arena.buf("gdet", (B, 32)); gdet.zero_()
        ops.sum_over_hypotheses(gdet_rows, N, B, out=gdet, out_stride=32)
        ops.linear_wgrad(hd, gdet, self.d2["dw"]); ops.colsum(gdet, self.d2["db"])
        ghd = ops.linear(gdet, self.d2["wT"]); ops.flow_lrelu_bwd(ghd, hd, slope=0.0)
        ops.linear_wgrad(feat, ghd, self.d0["dw"]); ops.colsum(ghd, self.d0["db"])
        g_feat = self.part.feat_grad(feat)       # (RealNVP: the conditioning projections' reverse runs here, after the det head's launches)
        ops.add(g_feat, ops.linear(ghd, self.d0["wT"]))
        if hs is not None:          # partial over the local hypotheses, all images -> this rank's images, all hypotheses
            g_feat = hs.scatter_grad(g_feat)
        ops.linear_wgrad(f, g_feat, self.l1["dw"]); ops.colsum(g_feat, self.l1["db"])
        g_f = ops.linear(g_feat, self.l1["wT"])
        self._grad_ready(3)
        if t["trunk"]:
            self._trunk_backward(g_f)
        else:
            for i in (2, 1, 0):
                self._grad_ready(i)
        t.update({"g_feat": g_feat, "g_th45": g45, "g_trunk_out": g_f})
        if getattr(self.model, "_trainer", None) is self and self.world > 1:
            # autograd-bridge use under data parallelism: torch's optimizer expects the averaged gradient in .grad
            self.finish_allreduce()
            self.G.mul_(1.0 / self.world)
            self._G_averaged = True        # optimizer_step() must not divide by world a second time

    def forward_backward(self, x, y, noise=None, N=None, trunk_out=None, mods=None, chamfer_w=None, sil_w=None, sil_occluder=None):
        """forward + reverse pass of total = mean_b(-log_p[b]); fills self.G.  Returns the get_loss dict + 'total'."""
        out = self.forward(x, y, noise=noise, N=N, trunk_out=trunk_out, mods=mods, chamfer_w=chamfer_w, sil_w=sil_w, sil_occluder=sil_occluder)
        self.backward()
        out["total"] = -out["log_p"].mean()
        return out

    # ------------------------------------------------------------------ torch.autograd bridge
    def attach(self):
        """make `model.get_loss(...)` (training mode, grad enabled) differentiable: `total_loss.backward()` of the reference's
        loop (hand/CrossModalHand.py:455-470) then runs the hand-written reverse pass and leaves the gradients in every
        parameter's `.grad` (views of the flat gradient buffer), so the reference's own `clip_grad_norm_` and
        `torch.optim.Adam` work unchanged.  (The fused `step()` stays the fast path.)"""
        self.model._trainer = self
        return self

    def _sil_bwd(self, t, g_logp, g45, gdet_rows):
        """reverse of log_p[b] -= sil_w mean_n dist[n B + b]: g_dist[r] = -sil_w g_logp[b] / N (one elementwise launch), both minima
        re-evaluated with the gradients in the same launch, the mesh's reverse to z, z's adjoint added to the loss pass' two buffers"""
        N, B = t["N"], t["B"]
        g_dist = self.arena.buf("g_sil_dist", (N, B))
        torch.mul(g_logp.view(1, B).expand(N, B), -t["terms"].sil_w / t["N_all"], out=g_dist)
        g_verts, g_logs_t = ops.silhouette_dist_grad(t["sil_verts"].view(N, B, 778, 3), t["sil_logs_t"].view(N, B, 3), *t["sil"], g_dist, count_all=t["sil_all"])
        g_z = ops.mano_verts_bwd(t["z"], t["blob"], g_verts.view(N * B, 778, 3))
        ops.mano_z_grad_add(g_z, g_logs_t.view(N * B, 3), g45, gdet_rows)

    def optimizer_step(self):
        """all-reduce (sum) over ranks, clip_grad_norm_(max_norm) and Adam in one fused pass"""
        self.finish_allreduce()          # the buckets were handed to RCCL as the reverse pass completed them
        ops.train_tick(self.step_t, self.sq)
        if self.max_norm and self.max_norm > 0:
            ops.sqnorm(self.G, self.sq)
        self.last_grad_scale = 1.0 if self._G_averaged else 1.0 / self.world
        ops.adam_step(self.P, self.G, self.M, self.V, self.sq, self.step_t, self.lr, self.betas[0], self.betas[1], self.eps,
                      self.max_norm or 0.0, self.last_grad_scale)
        self._G_averaged = False
        self.arena.repack()          # every derived operand layout follows the new parameters
        self.arena.mark_synced()

    def second_bn_update(self):
        """what a SECOND train-mode encoder pass over the same batch does to the BatchNorm buffers (the reference's metrics
        pass, hand/CrossModalHand.py:355-361: identical batch statistics, so running = (1-m) running + m stat once more and
        num_batches_tracked + 1), from the statistics the forward kept - a handful of multi-tensor launches, no second pass"""
        units = [u for u in self.units if u.mi is not None]
        means = [u.mi[0] for u in units]
        var = torch._foreach_pow([u.mi[1] for u in units], -2.0)            # 1/invstd^2 = biased var + eps
        torch._foreach_sub_(var, BN_EPS)
        # pixels per channel of the unit's output (a folded conv3 - 1x1, stride 1 - never wrote it: its input has the same pixels)
        npix = [float(u.y.numel() // u.cout) if u.y is not None else float(u.x.numel() // u.cin) for u in units]
        torch._foreach_mul_(var, [n / max(n - 1.0, 1.0) for n in npix])
        torch._foreach_lerp_([u.bn.running_mean for u in units], means, BN_MOMENTUM)
        torch._foreach_lerp_([u.bn.running_var for u in units], var, BN_MOMENTUM)
        torch._foreach_add_([u.bn.num_batches_tracked for u in units], 1)

    def step(self, x, y, noise=None, N=None, test_samples=0, temp=0.8, double_bn_update=True, mods=None, chamfer_w=None, sil_w=None,
             test_quant=0, quant="log_q", sil_occluder=None):
        """one iteration of the reference's training loop (hand/CrossModalHand.py:353-361,455-470).  test_samples > 0
        adds its per-iteration metrics pass `sample(N=[n,n], temp=0.8, mods={uv,xyz,verts})` to the returned dict,
        from the conditioning feature of THIS forward.  The reference runs the encoder a second time on the same
        batch in train mode for it: same feature, but the BatchNorm running statistics advance twice per iteration -
        double_bn_update=True (default) reproduces that on the buffers, so checkpoints / eval-mode results match a
        reference-trained model.  mods, chamfer_w, sil_w, sil_occluder: get_loss's likelihoods, Chamfer and silhouette weights and the
        silhouette term's occluder switch, as in forward().
        test_quant (0: test_samples) and quant: the metrics pass is sample(N=[test_samples, test_quant], quant=quant)."""
        out = self.forward_backward(x, y, noise=noise, N=N, mods=mods, chamfer_w=chamfer_w, sil_w=sil_w, sil_occluder=sil_occluder)
        if test_samples:
            if double_bn_update and self.tape["trunk"]:
                self.second_bn_update()
            with torch.no_grad():
                out.update(self.model.sample(None, N=[test_samples, test_quant or test_samples], temp=temp, mods={"uv", "xyz", "verts"}, y=y,
                                             feat=self.tape["feat_own"], quant=quant))
        self.optimizer_step()
        return out


class GraphedStep:
    """TrainStep.step replayed from HIP graphs (launch-bound: ~840 kernels per step).  One process: one graph.  Data parallel:
    the step is cut where a gradient bucket is complete - a graph ends there, the bucket's all-reduce is issued eagerly
    (RCCL, async_op: it runs on the communicator's stream under the next graph's kernels), the next graph starts; the last
    graph (norm, clip, Adam, operand re-pack) is launched after the waits.  Six graphs and four collectives per step."""

    def __init__(self, ts, x, y, noise=None, N=None, test_samples=0, criterion=None, mods=None, chamfer_w=None, sil_w=None, sil_occluder=None):
        """test_samples / criterion: the reference's whole iteration (hand/CrossModalHand.py:349-361,452-470) in the graph - the
        metrics pass sample(N=[n,n], temp=0.8) from this forward's feature and `criterion(out, y)` (MHEntLoss: 14 metrics);
        self.out then carries 'criterion' = (total, losses, metrics).  mods: get_loss's likelihoods (TrainStep.forward); with 'xyz'
        the graphs read y['pose3d'] - a new target is copied into that static tensor like the rest of the batch.  chamfer_w > 0 (None: the
        model's): y['object_verts'], 'scale', 'original_pose3d' and 'object_count' are static inputs in the same way; the count's range is
        checked on the host by the warm-up step only (a capturing stream takes no host read: the kernels clamp it to 1..VO).  sil_w > 0
        (None: the model's): y['hand_mask'] is a static input too; its kept-pixel list is rebuilt inside the graph on every replay.
        sil_occluder (None: the model's): y['object_mask'] is a static input like the mask, and both sections of the list are rebuilt"""
        if ts.shard_hypotheses:
            raise NotImplementedError("GraphedStep: the hypothesis-sharded forward has collectives inside the forward pass")
        self.ts, self.graphs, self.actions = ts, [], []
        # the graphs hold the ADDRESSES of their static inputs; the step itself keeps no reference to x (the trunk keeps its NHWC copy only).
        # A caller that passes a temporary (x.clone()) would leave the graphs reading a freed block that the next allocation may take.
        self.static = (x, y, noise)
        _step = ts.step

        def step(x, y, noise=None, N=None):
            out = _step(x, y, noise=noise, N=N, test_samples=test_samples, mods=mods, chamfer_w=chamfer_w, sil_w=sil_w, sil_occluder=sil_occluder)
            if criterion is not None:
                with torch.no_grad():
                    out["criterion"] = criterion(dict(out), y)
            return out
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            # allocations and lazy initialisation happen here, not under capture.  This warm-up IS one real optimizer step on the
            # batch held by x / y: `warm_out` is that iteration's result, and a training loop must not replay() the same batch
            # again (mhentropy_amd/run.py takes warm_out for the capture iteration; the reference steps once per iteration,
            # hand/CrossModalHand.py:455-470)
            self.warm_out = step(x, y, noise=noise, N=N)
        cur.wait_stream(side)
        torch.cuda.synchronize()
        self._mode = "thread_local" if ts.comm else "global"           # the communicator's watchdog thread may touch the device
        with torch.cuda.stream(side):
            self._cur = torch.cuda.CUDAGraph()
            self._cur.capture_begin(capture_error_mode=self._mode)
            ts._capture = self
            try:
                self.out = step(x, y, noise=noise, N=N)
            finally:
                ts._capture = None
                self._cur.capture_end()
            self.graphs.append(self._cur)
        cur.wait_stream(side)
        torch.cuda.synchronize()
        self._fb_in_graph = ts.arena.fb_keep        # does the captured end-of-step repack refresh the flow's fallback layouts? (replay())

    def cut(self, action):
        self._cur.capture_end()
        self.graphs.append(self._cur)
        self.actions.append(action)
        self._cur = torch.cuda.CUDAGraph()
        self._cur.capture_begin(pool=self.graphs[0].pool(), capture_error_mode=self._mode)

    def replay(self):
        ts = self.ts
        if not self._fb_in_graph:              # the captured repack did not refresh the fallback layouts: they no longer follow the parameters
            ts.arena.fb_stale = True
            ts.arena.poison_fallback()
        for k, g in enumerate(self.graphs):
            g.replay()
            if k < len(self.actions):
                a = self.actions[k]
                if a[0] == "allreduce":
                    ts._all_reduce_bucket(a[1])
                elif ts._xchg is not None:
                    ts._xchg.finish()
        return self.out


class _LossFn(torch.autograd.Function):
    """MHEnt.get_loss as one autograd node: forward = TrainStep.forward, backward = TrainStep.backward(d loss / d log_p)."""
    @staticmethod
    def forward(ctx, trainer, x, y, N, noise, mods, chamfer_w, sil_w, sil_occluder, *params):
        out = trainer.forward(x, y, noise=noise, N=N, mods=mods, chamfer_w=chamfer_w, sil_w=sil_w, sil_occluder=sil_occluder)
        ctx.trainer, ctx.keys = trainer, list(out)
        vals = tuple(out[k] for k in ctx.keys)
        ctx.mark_non_differentiable(*[v for k, v in zip(ctx.keys, vals) if k != "log_p"])
        return vals

    @staticmethod
    def backward(ctx, *grads):
        tr = ctx.trainer
        g = grads[ctx.keys.index("log_p")]
        tr.backward(None if g is None else g.contiguous().float())
        params = tr.arena.params
        return (None,) * (len(ctx.needs_input_grad) - len(params)) + tuple(tr.grad_of(p) for p in params)     # one per input of forward


def differentiable_get_loss(trainer, x, y, N=None, noise=None, mods=None, chamfer_w=None, sil_w=None, sil_occluder=None):
    # (forward checks the mask and lists its pixels, before any other launch)
    terms = LossTerms(trainer.model, y, mods, chamfer_w, sil_w, pixels=False, sil_occluder=sil_occluder)
    w = terms.weights()
    vals = _LossFn.apply(trainer, x, y, N, noise, w["mods"], w["chamfer_w"], w["sil_w"], w.get("sil_occluder", False), *trainer.arena.params)
    return dict(zip(terms.keys(), vals))
