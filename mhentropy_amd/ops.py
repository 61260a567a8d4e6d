"""Tensor-level wrappers over the C ABI (include/mhe.h).

torch is plumbing here: it owns device memory and the HIP stream; every number is
produced by the hand-written kernels in csrc/.  All functions require CUDA (HIP)
tensors and raise on anything else - there is no CPU path in the product.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, check

F32, BF16 = 0, 1
FLOW_FORWARD, FLOW_INVERSE = 0, 1

# bench.py instrumentation: when TIMING is set every conv launch is bracketed by
# HIP events on the launch stream and logged as (kernel name, algorithmic flops, ev0, ev1)
TIMING = False
TIMING_DG = False        # tools/train_lines.py: also the data-gradient launches, under descriptive names (not rocprofv3's: bench.py leaves it off)
KERNEL_TIMES = []


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _chk(t, dtype, name, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.MheError(f"{name}: expected a CUDA/HIP tensor (the hot path has no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.MheError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.MheError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.MheError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def launch(entry, *args):
    """one kernel launch through the C ABI: tensors go as their device address (None as null; ints, floats, byref and explicit c_void_p
    sub-addresses as they are), the current stream is appended, the status is checked under the entry's own name.  A tensor that is not on
    the GPU is refused here: its host address must never reach a kernel."""
    conv = []
    for i, a in enumerate(args):
        if a is None or isinstance(a, torch.Tensor):
            if a is not None and not a.is_cuda:
                raise _lib.MheError(f"{entry}: argument {i} is a {a.device.type} tensor, every tensor operand must be device memory (the hot path has no CPU fallback)")
            a = _ptr(a)
        conv.append(a)
    check(getattr(_lib.lib(), entry)(*conv, _stream()), entry)


class _Timed:
    """HIP events on the launch stream around the launches of its body, appended to KERNEL_TIMES while TIMING is on (bench.py's live roofline
    pass).  what() -> (kernel name, algorithmic flops, algorithmic HBM bytes), evaluated only then; what=None: never timed"""
    def __init__(self, what):
        self.what = what if TIMING else None

    def __enter__(self):
        if self.what is not None:
            self.rec = self.what()
            self.ev0, self.ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.ev0.record()
        return self

    def __exit__(self, exc_type, *exc):
        if self.what is not None and exc_type is None:
            self.ev1.record()
            name, flops, nbytes = self.rec
            KERNEL_TIMES.append((name, flops, self.ev0, self.ev1, nbytes))
        return False


def _bn_consumers(bn, n, dt, shape, Cn, prefix, only_one=None):
    """bn: up to n (raw output y, mean_invstd [2, Cn], stats) triples of the BatchNorm units whose reverse sums a data-gradient epilogue
    accumulates.  Checks every triple given and returns the flat operand list [y, mean_invstd, stats] * n with None for the units that are
    absent; only_one: the ValueError of a form that takes a single consumer"""
    bn = list(bn or [])
    if only_one and len(bn) > 1:
        raise ValueError(only_one)
    flat = []
    for by, bmi, bst in (bn + [(None, None, None)] * n)[:n]:
        if by is not None:
            _chk(by, dt, prefix + ".bn_y", shape); _chk(bmi, torch.float32, prefix + ".bn_mean_invstd", (2, Cn))
            _chk_stats(bst, prefix + ".bn_stats", Cn)
        flat += [by, bmi, bst]
    return flat


def _grow_only_workspace():
    """get(device, need): one f32 workspace per device, grown to the largest request.  A superseded buffer stays referenced for the life of
    the process: a captured HIP graph (train.GraphedStep) may have baked its address in"""
    live, retired = {}, []

    def get(device, need):
        ws = live.get(device)
        if ws is None or ws.numel() < need:
            if ws is not None:
                retired.append(ws)
            ws = live[device] = torch.empty(need, device=device, dtype=torch.float32)
        return ws
    return get


def stat_shards():
    return _lib.lib().mhe_conv_stat_shards()


STAT_DTYPE = torch.int64


def stat_shape(C):
    """one unit of sharded fixed-point accumulators for C channels (include/mhe.h, mhe_stat_t): [2 planes][S shards][2 statistics][C]"""
    return (2, stat_shards(), 2, C)


def stat_unit(C, device):
    return torch.zeros(stat_shape(C), device=device, dtype=STAT_DTYPE)


def stat_totals(st):
    """[2, C] float64 totals of a unit: sum over shards of plane0 * 2^-16 + plane1 * 2^-56 (what the finalize kernels compute; the
    marker of a non-finite partial is not decoded here - tests and diagnostics only)"""
    t = st.sum(1)                                     # integer sums: exact
    return t[0].double() * 2.0 ** -16 + t[1].double() * 2.0 ** -56


def stat_from_float(t):
    """[S, 2, C] float shard values -> a unit holding them (the encoding fx::add2 of csrc/common.h applies to one partial; tests)"""
    d = t.double() * 2.0 ** 16
    hi = torch.round(d)
    lo = torch.round((d - hi) * 2.0 ** 40)
    return torch.stack([hi.to(torch.int64), lo.to(torch.int64)]).contiguous()


def _chk_stats(t, name, C):
    _chk(t, STAT_DTYPE, name, stat_shape(C))


_TILES = {0: "128, 64, 2, 2", 1: "128, 128, 2, 2", 2: "256, 256, 2, 4", 3: "256, 128, 4, 2", 4: "256, 64, 4, 2"}


def _conv_kernel_name(d, dt, mode):
    """the template instantiation the launcher will pick, spelled as rocprofv3 prints it"""
    bke = 32 if dt == torch.float32 else 64
    tile = _lib.lib().mhe_conv_tile_mode(C.byref(d), mode)
    mode = 0 if mode == 3 else mode          # (3 = plain operand load + a residual in the epilogue: the kernel's MODE is 0)
    if tile == 11:
        return "mhe::conv::conv_wide_kernel<%s, %s>" % ("128, 4" if d.Cin == 256 else "64, 8", "true" if mode == 1 else "false")
    if tile == 10:
        return "mhe::conv::conv_tail_kernel<false>"
    if tile == 9:
        # (BatchNorm on load: the three-role form; plain: two roles)
        return "mhe::conv::conv3x3_c64_roles3_kernel<true>" if mode == 1 else "mhe::conv::conv3x3_c64_stream_kernel<false, false>"
    if tile == 8:
        return "mhe::conv::conv1x1_stream_kernel<%d, %d, %s, false>" % (d.Cin // 64, 64 if (d.Cin == 64 and d.Cout == 64) else 256 if d.Cin <= 128 else 128, "true" if mode == 1 else "false")
    if tile == 13:
        return "mhe::conv::conv_p8_kernel<false, %s, 0, 1>" % ("false" if d.KH == 1 and d.KW == 1 and d.pad == 0 else "true")
    if tile == 7:
        return "mhe::conv::conv_p8_kernel<false, %s, 0, 2>" % ("false" if d.KH == 1 and d.KW == 1 and d.pad == 0 else "true")
    return "mhe::conv::conv_kernel<%s, %s, %s, %d, false>" % ("float" if dt == torch.float32 else "unsigned short",
                                                             _TILES[tile],
                                                             "true" if d.Cin % bke == 0 else "false", mode)


def dtype_code(dt):
    return F32 if dt == torch.float32 else BF16


def conv_tile_choice(B, H, W, Cin, Cout, k, stride, pad, dt, mode=0):
    """the tile variant the launcher picks for this convolution (mhe_conv_tile_mode; include/mhe.h lists the variants).  mode 1 = with the
    producer's BatchNorm on the operand load.  9 = the row-streaming 3x3 kernel, whose on-load form costs one multiply-add per element read
    ONCE (rows are normalised on their way into the LDS ring), unlike the tiled kernels that normalise every tap's re-read."""
    d = ConvDesc(B, H, W, Cin, Cout, k, k, stride, pad, dtype_code(dt), int(mode == 1), 0, 0, 0)
    return _lib.lib().mhe_conv_tile_mode(C.byref(d), mode)


def linear(x, w, bias=None, relu=False, out=None, want_bf16=False):
    """act(x @ w.T + bias) in f32 (mhe_linear_f32).  want_bf16: returns (y, y as bf16) from the same launch where the shape admits it
    (mhe_linear_f32_bf16copy: M <= 256, K % 64 == 0), else (y, None)."""
    M, K = x.shape
    N = w.shape[0]
    _chk(x, torch.float32, "linear.x"); _chk(w, torch.float32, "linear.w", (N, K))
    if bias is not None:
        _chk(bias, torch.float32, "linear.bias", (N,))
    y = out if out is not None else torch.empty(M, N, device=x.device, dtype=torch.float32)
    _chk(y, torch.float32, "linear.out", (M, N))
    if want_bf16:
        if M <= 256 and K % 64 == 0 and N % 4 == 0:
            yb = torch.empty(M, N, device=x.device, dtype=torch.bfloat16)
            launch("mhe_linear_f32_bf16copy", x, w, bias, y, yb, M, N, K, int(relu))
            return y, yb
        launch("mhe_linear_f32", x, w, bias, y, M, N, K, int(relu))
        return y, None
    launch("mhe_linear_f32", x, w, bias, y, M, N, K, int(relu))
    return y


_RNG_STATE = {}


def rng_state(device, seed=None):
    """the device-resident generator state {seed, next counter, 0} of mhe_randn_f32 for `device`; created on first use from torch's
    seed (torch.manual_seed(s) before the first draw makes runs repeatable), or re-seeded explicitly with seed="""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = _RNG_STATE.get(device)
    if st is None:
        s = torch.initial_seed() if seed is None else int(seed)
        st = _RNG_STATE[device] = torch.tensor([s & 0x7FFFFFFFFFFFFFFF, 0, 0], dtype=torch.int64, device=device)
    elif seed is not None:
        # re-seed IN PLACE: a captured HIP graph has this tensor's address baked into its randn_kernel node
        st.copy_(torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, 0, 0], dtype=torch.int64))
    return st


def rng_get_state(device):
    """the three int64 words {seed, next counter, draws} of the device generator, on the host (for checkpoints)"""
    return rng_state(device).cpu().clone()


def rng_set_state(device, words):
    """restore rng_get_state()'s words in place (a resumed run continues the base-noise stream instead of replaying it)"""
    st = rng_state(device)
    st.copy_(torch.as_tensor(words, dtype=torch.int64).reshape(3))
    return st


def randn(rows, cols, device, scale=1.0, state=None):
    """[rows, cols] f32 ~ N(0, scale^2) drawn on the device by mhe_randn_f32 (graph-capturable: the launch advances its own counter)"""
    out = torch.empty(rows, cols, device=device, dtype=torch.float32)
    st = state if state is not None else rng_state(out.device)
    launch("mhe_randn_f32", out, out.numel(), st, float(scale))
    return out


def dropout_(x, p, bits=None, state=None):
    """x <- x * keep / (1 - p) in place (mhe_dropout).  bits=None: the mask is drawn on the device (the generator state of randn advances) and
    its bits are returned (uint8 [x.numel() / 8], bit k of byte i = element 8 i + k kept); bits given: that mask is applied."""
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda or not x.is_contiguous() or x.numel() % 8:
        raise _lib.MheError("dropout_: contiguous f32 / bf16 device tensor with a multiple of 8 elements expected")
    draw = bits is None
    if draw:
        bits = torch.empty(x.numel() // 8, device=x.device, dtype=torch.uint8)
        st = state if state is not None else rng_state(x.device)
    else:
        _chk(bits, torch.uint8, "dropout.bits", (x.numel() // 8,))
        st = None
    launch("mhe_dropout", x, dtype_code(x.dtype), bits, x.numel(), float(p), st, int(draw))
    return bits


def dropout_mask(bits, shape, p):
    """the float mask (0 or 1 / (1 - p)) that dropout_ applied, from its bits (tests: the oracle is fed the same mask)"""
    m = ((bits.view(-1, 1).int() >> torch.arange(8, device=bits.device, dtype=torch.int32)) & 1).float().reshape(shape)
    return m / (1.0 - p)


def reparam(mn, l2, eps=None, sigmoid_act=False, deterministic=False):
    """(sd, z) of BasicEnc's stochastic head (mhe_reparam_f32)"""
    _chk(mn, torch.float32, "reparam.mn"); _chk(l2, torch.float32, "reparam.l2", mn.shape)
    if eps is not None:
        _chk(eps, torch.float32, "reparam.eps", mn.shape)
    sd, z = torch.empty_like(mn), torch.empty_like(mn)
    launch("mhe_reparam_f32", mn, l2, eps, sd, z, mn.numel(), int(sigmoid_act), int(deterministic or eps is None))
    return sd, z


def flow_pack_net(w0, w1, w2):
    """Host repack of one coupling network's weights (numpy float32) into the
    fragment-ordered stream (mhe_flow_pack_net_host)."""
    hidden, dim = w0.shape
    L = _lib.lib()
    n = L.mhe_flow_packed_floats_per_net(dim, hidden)
    if n == 0:
        raise _lib.MheError(f"flow_pack_net: unsupported geometry dim={dim} hidden={hidden}")
    out = np.empty(n, np.float32)
    w0, w1, w2 = (np.ascontiguousarray(a, np.float32) for a in (w0, w1, w2))
    check(L.mhe_flow_pack_net_host(w0.ctypes.data_as(C.c_void_p), w1.ctypes.data_as(C.c_void_p),
                                   w2.ctypes.data_as(C.c_void_p), dim, hidden, out.ctypes.data_as(C.c_void_p)),
          "mhe_flow_pack_net_host")
    return out


def flow_pack_net_bf16(w0, w1, w2):
    """Host repack of one coupling network into the bf16 fragment stream (mhe_flow_pack_net_bf16_host)."""
    hidden, dim = w0.shape
    L = _lib.lib()
    n = L.mhe_flow_packed_bytes_per_net_bf16(dim, hidden)
    if n == 0:
        raise _lib.MheError(f"flow_pack_net_bf16: unsupported geometry dim={dim} hidden={hidden}")
    out = np.empty(n // 2, np.uint16)
    w0, w1, w2 = (np.ascontiguousarray(a, np.float32) for a in (w0, w1, w2))
    check(L.mhe_flow_pack_net_bf16_host(w0.ctypes.data_as(C.c_void_p), w1.ctypes.data_as(C.c_void_p),
                                        w2.ctypes.data_as(C.c_void_p), dim, hidden, out.ctypes.data_as(C.c_void_p)),
          "mhe_flow_pack_net_bf16_host")
    return out


def flow_couplings(x_in, cond, wstream, bias2, mask, B, hidden, direction, want_log_prob=True):
    """All couplings in one launch; returns (out, sum_s, log_prob).  The dtype of `wstream` selects the
    kernel: float32 stream -> f32 MFMA, int16/bf16 stream -> bf16 MFMA."""
    R, dim = x_in.shape
    ncoup = mask.shape[0]
    _chk(x_in, torch.float32, "flow.in")
    _chk(cond, torch.float32, "flow.cond", (B, 2 * ncoup, 2, hidden))
    bf16 = wstream.dtype != torch.float32
    _chk(wstream, wstream.dtype, "flow.wstream"); _chk(bias2, torch.float32, "flow.bias2", (2 * ncoup, 64 if bf16 else dim))
    _chk(mask, torch.float32, "flow.mask", (ncoup, dim))
    out = torch.empty_like(x_in)
    sum_s = torch.empty(R, device=x_in.device, dtype=torch.float32)
    logp = torch.empty(R, device=x_in.device, dtype=torch.float32) if want_log_prob else None
    launch("mhe_flow_couplings_bf16" if bf16 else "mhe_flow_couplings_f32", x_in, out, cond, wstream, bias2, mask, sum_s, logp, R, B, dim, hidden, ncoup,
           direction)
    return out, sum_s, logp


def flow_couplings_emit(x_in, cond, wstream, bias2, mask, B, hidden, direction, h1, h2, o):
    """flow_couplings (bf16 stream, hidden 512) that also writes the nets' hidden activations h1, h2 (bf16 [nets, R, 512]) and
    the s / t pre-activations o (f32 [nets, R, 64]) for the reverse pass; returns (out, sum_s, log_prob)."""
    R, dim = x_in.shape
    ncoup = mask.shape[0]
    _chk(x_in, torch.float32, "flow.in"); _chk(cond, torch.float32, "flow.cond", (B, 2 * ncoup, 2, hidden))
    _chk(wstream, wstream.dtype, "flow.wstream"); _chk(bias2, torch.float32, "flow.bias2", (2 * ncoup, 64))
    _chk(mask, torch.float32, "flow.mask", (ncoup, dim))
    _chk(h1, torch.bfloat16, "flow.h1", (2 * ncoup, R, hidden)); _chk(h2, torch.bfloat16, "flow.h2", (2 * ncoup, R, hidden))
    _chk(o, torch.float32, "flow.o", (2 * ncoup, R, 64))
    out = torch.empty_like(x_in)
    sum_s = torch.empty(R, device=x_in.device, dtype=torch.float32)
    logp = torch.empty(R, device=x_in.device, dtype=torch.float32)
    launch("mhe_flow_couplings_bf16_emit", x_in, out, cond, wstream, bias2, mask, sum_s, logp, h1, h2, o, R, B, dim, hidden, ncoup, direction)
    return out, sum_s, logp


def flow_couplings_frag_supported(R, B, dim, hidden, ncoup):
    return bool(_lib.lib().mhe_flow_couplings_frag_supported(R, B, dim, hidden, ncoup))


def flow_frag_pack(w0, w1, w2):
    """one net's layer weights (torch [h, dim], [h, h], [dim, h]; or index tensors of those shapes) -> (w1F, w0F, w2F) in MFMA fragment order,
    dim zero-padded (index tensors: -1) to 64 - the operands of mhe_flow_couplings_frag_bf16"""
    h, dim = w0.shape
    fill = -1 if not w0.is_floating_point() else 0
    w0p = torch.full((h, 64), fill, dtype=w0.dtype, device=w0.device); w0p[:, :dim] = w0
    w2p = torch.full((64, h), fill, dtype=w2.dtype, device=w2.device); w2p[:dim] = w2
    return mfma_fragment_major(w1), mfma_fragment_major(w0p), mfma_fragment_major(w2p)


def flow_couplings_frag(x_in, cond, w0F, w1F, w2F, w_net_stride, bias2, mask, B, hidden, direction, want_log_prob=True, emit=None, sign_bits=None):
    """flow_couplings / flow_couplings_emit (emit = (h1, h2, o)) on the fragment-streaming kernel (mhe_flow_couplings_frag_bf16);
    sign_bits (with emit, int32 [nets, R / 64, 2, 8, 64, 2]): also the signs of h1 / h2 as the reverse chain reads them"""
    R, dim = x_in.shape
    ncoup = mask.shape[0]
    _chk(x_in, torch.float32, "flow.in"); _chk(cond, torch.float32, "flow.cond", (B, 2 * ncoup, 2, hidden))
    _chk(bias2, torch.float32, "flow.bias2", (2 * ncoup, 64)); _chk(mask, torch.float32, "flow.mask", (ncoup, dim))
    for t, nm in ((w0F, "w0F"), (w1F, "w1F"), (w2F, "w2F")):
        _chk(t, torch.bfloat16, "flow." + nm)
    h1 = h2 = o = None
    if emit is not None:
        h1, h2, o = emit
        _chk(h1, torch.bfloat16, "flow.h1", (2 * ncoup, R, hidden)); _chk(h2, torch.bfloat16, "flow.h2", (2 * ncoup, R, hidden))
        _chk(o, torch.float32, "flow.o", (2 * ncoup, R, 64))
    if sign_bits is not None:
        _chk(sign_bits, torch.int32, "flow.sign_bits", (2 * ncoup, R // 64, 2, 8, 64, 2))
    out = torch.empty_like(x_in)
    sum_s = torch.empty(R, device=x_in.device, dtype=torch.float32)
    logp = torch.empty(R, device=x_in.device, dtype=torch.float32) if want_log_prob else None
    launch("mhe_flow_couplings_frag_bf16", x_in, out, cond, 4 * ncoup * hidden, w0F, w1F, w2F, int(w_net_stride), bias2, mask, sum_s, logp, h1, h2, o, sign_bits, R,
           B, dim, hidden, ncoup, direction)
    return out, sum_s, logp


MODS_UV, MODS_XYZ = 1, 2           # MHE_MODS_* of include/mhe.h


def mods_bits(mods):
    """the reference's get_loss `mods` (hand/network.py:620-643; None means ['uv']) -> the MHE_MODS_* bit set.  'uv' and 'xyz' in any
    order; anything else (the dead p_ys branch) is not built.  The render mods 'm' / 'depth' are no likelihood here: MHEnt.sample(mods=)
    takes them (ops.render_mesh, forward only).  Nor are the chamfer and the silhouette term mods: their distances are ops.chamfer /
    criteria.chamfer_dist and ops.silhouette_dist / criteria.silhouette_dist, and the loss takes them through get_loss(chamfer_w=...)
    (mano_joints(chamfer=...)) and get_loss(sil_w=...)"""
    if mods is None:
        return MODS_UV
    names = [mods] if isinstance(mods, str) else list(mods)
    bits = 0
    for m in names:
        if m not in ("uv", "xyz"):
            raise NotImplementedError(f"mods={names!r}: only the 'uv' and 'xyz' likelihoods are built (hand/network.py:620-643)")
        bits |= MODS_UV if m == "uv" else MODS_XYZ
    if not bits or len(names) != len(set(names)):
        raise NotImplementedError(f"mods={names!r}: expected ['uv'], ['xyz'] or ['xyz', 'uv']")
    return bits


def _chamfer_target(chamfer, B, who):
    """chamfer = (scale [B], root [B,3], obj [B,VO,3], count [B] int32 | None), as criteria.chamfer_target_operands returns them -> VO"""
    if not isinstance(chamfer, (tuple, list)) or len(chamfer) != 4:
        raise ValueError(f"{who}: chamfer must be (scale, root, obj, count)")
    scale, root, obj, count = chamfer
    if not isinstance(obj, torch.Tensor) or obj.dim() != 3:
        raise _lib.MheError(f"{who}.obj: expected a [B,VO,3] tensor")
    VO = obj.shape[1]
    _chk(scale, torch.float32, f"{who}.scale", (B,)); _chk(root, torch.float32, f"{who}.root", (B, 3)); _chk(obj, torch.float32, f"{who}.obj", (B, VO, 3))
    if count is not None:
        _chk(count, torch.int32, f"{who}.count", (B,))
    return VO


def mano_joints(th45, det, tables, crop_uv=None, vis=None, laplace_b=0.03, th45_alpha=50.0, inv_norm=False,
                image_size=256.0, want=("z", "xyz", "uv", "terms", "log_p", "norms"), pose3d=None, mods=None, laplace_b_3d=0.03,
                chamfer=None):
    """want may also include "joints_mm", and "verts" (the full mesh, normalised like xyz) or "mesh_mm" (ManoLayer's mesh in mm): the mesh
    of the same hypotheses through mhe_mano_decode_f32 - the joint pass leaves the skinning operands, no second pose pass.
    mods (None, or a MHE_MODS_* bit set / the reference's list of names): the likelihoods in terms / log_p through
    mhe_mano_joints_mods_f32 - terms is then [R,5] = (uv, xyz, th3, th45, bt); 'xyz' needs pose3d [B,63] (Laplace with b = laplace_b_3d).
    chamfer = (scale [B], root [B,3], obj [B,VO,3], count [B] int32 | None): the same pass through mhe_mano_joints_chamfer_f32 (mods None
    means uv there, terms [R,5]) - adds "chamfer" [R], every row's hand-object Chamfer distance in mm (ops.chamfer's, of the 21 joints);
    log_p and the other outputs do not change by a bit."""
    R, B = th45.shape[0], det.shape[0]
    dev = th45.device
    _chk(th45, torch.float32, "mano.th45", (R, 45)); _chk(det, torch.float32, "mano.det", (B, 16))
    _chk(tables, torch.float32, "mano.tables")
    if crop_uv is not None:
        _chk(crop_uv, torch.float32, "mano.crop_uv", (B, 42))
    if vis is not None:
        _chk(vis, torch.float32, "mano.vis", (B, 21))
    if pose3d is not None:
        _chk(pose3d, torch.float32, "mano.pose3d", (B, 63))
    bits = None if mods is None else (int(mods) if isinstance(mods, int) else mods_bits(mods))
    mesh = [k for k in ("verts", "mesh_mm") if k in want]
    if chamfer is not None:
        VO = _chamfer_target(chamfer, B, "mano.chamfer")
        if vis is None:
            raise ValueError("mano_joints(chamfer=...): vis is required")
        bits = MODS_UV if bits is None else bits
    if mesh and bits is not None:
        raise ValueError("mano_joints: the mesh outputs come from the uv-only pass (mods=None" + (")" if chamfer is None else ", chamfer=None)"))
    if len(mesh) > 1:
        raise ValueError("mano_joints: 'verts' or 'mesh_mm', one mesh per call")
    shapes = {"z": (R, 61), "xyz": (R, 63), "uv": (R, 42), "terms": (R, 4 if bits is None else 5), "log_p": (R,), "norms": (R, 2),
              "joints_mm": (R, 63)}
    o = {k: (torch.empty(shapes[k], device=dev, dtype=torch.float32) if k in want else None) for k in shapes}
    outs = tuple(o.values())
    lb, lb3, alpha, tail = float(laplace_b), float(laplace_b_3d), float(th45_alpha), (int(inv_norm), float(image_size))
    # the four entries of the pass, each with its argument list: Chamfer target > likelihood bit set > mesh decode > the 4-term uv pass
    if chamfer is not None:
        o["chamfer"] = torch.empty(R, device=dev, dtype=torch.float32)
        entry, args = "mhe_mano_joints_chamfer_f32", (th45, det, crop_uv, vis, pose3d, tables, *chamfer, *outs, o["chamfer"], R, B, VO, bits, lb, lb3, alpha, *tail)
    elif bits is not None:
        entry, args = "mhe_mano_joints_mods_f32", (th45, det, crop_uv, vis, pose3d, tables, *outs, R, B, bits, lb, lb3, alpha, *tail)
    elif mesh:
        o[mesh[0]] = torch.empty(R, 778, 3, device=dev, dtype=torch.float32)
        ws = torch.empty(_lib.lib().mhe_mano_verts_workspace_floats(R), device=dev, dtype=torch.float32)
        entry, args = "mhe_mano_decode_f32", (th45, det, crop_uv, vis, tables, *outs, o[mesh[0]], ws, R, B, lb, alpha, *tail, int(mesh[0] == "mesh_mm"))
    else:
        entry, args = "mhe_mano_joints_f32", (th45, det, crop_uv, vis, tables, *outs, R, B, lb, alpha, *tail)
    launch(entry, *args)
    return o


def mano_joints_bwd_rows(th45, det, tables, crop_uv, vis, g_log_p, N, g_th45, g_rows, laplace_b=0.03, th45_alpha=50.0, pose3d=None, mods=None,
                         laplace_b_3d=0.03, chamfer=None, chamfer_w=0.0):
    """mano_joints_bwd into the caller's g_th45 [R,45] and g_rows [R,16]: d/d det stays one row per hypothesis -> (g_th45, g_rows)"""
    R, B = th45.shape[0], det.shape[0]
    _chk(th45, torch.float32, "mano_bwd.th45", (R, 45)); _chk(det, torch.float32, "mano_bwd.det", (B, 16))
    if crop_uv is not None or mods is None:
        _chk(crop_uv, torch.float32, "mano_bwd.crop_uv", (B, 42))
    _chk(vis, torch.float32, "mano_bwd.vis", (B, 21))
    if pose3d is not None:
        _chk(pose3d, torch.float32, "mano_bwd.pose3d", (B, 63))
    _chk(g_log_p, torch.float32, "mano_bwd.g_log_p", (B,))
    _chk(g_th45, torch.float32, "mano_bwd.g_th45", (R, 45)); _chk(g_rows, torch.float32, "mano_bwd.g_rows", (R, 16))
    bits = None if mods is None else (int(mods) if isinstance(mods, int) else mods_bits(mods))
    lb, lb3, alpha = float(laplace_b), float(laplace_b_3d), float(th45_alpha)
    if chamfer is not None:
        VO = _chamfer_target(chamfer, B, "mano_bwd.chamfer")
        launch("mhe_mano_joints_chamfer_bwd_f32", th45, det, crop_uv, vis, pose3d, tables, *chamfer, g_log_p, g_th45, g_rows, R, B, VO,
               MODS_UV if bits is None else bits, lb, lb3, alpha, 1.0 / N, float(chamfer_w))
    elif bits is None:
        launch("mhe_mano_joints_bwd_f32", th45, det, crop_uv, vis, tables, g_log_p, g_th45, g_rows, R, B, lb, alpha, 1.0 / N)
    else:
        launch("mhe_mano_joints_mods_bwd_f32", th45, det, crop_uv, vis, pose3d, tables, g_log_p, g_th45, g_rows, R, B, bits, lb, lb3, alpha, 1.0 / N)
    return g_th45, g_rows


def mano_joints_bwd(th45, det, tables, crop_uv, vis, g_log_p, N, laplace_b=0.03, th45_alpha=50.0, pose3d=None, mods=None,
                    laplace_b_3d=0.03, chamfer=None, chamfer_w=0.0):
    """reverse of mano_joints' log_p: (d/d th45 [R,45], d/d det [B,16]) for d loss/d log_p[n*B+b] = g_log_p[b]/N;
    mods / pose3d / laplace_b_3d as in mano_joints (crop_uv may be None when 'uv' is off).
    chamfer (as in mano_joints) with chamfer_w: the reverse of log_p[r] - chamfer_w * chamfer[r] (mhe_mano_joints_chamfer_bwd_f32)"""
    g_th45, g_rows = (torch.empty(th45.shape[0], c, device=th45.device, dtype=torch.float32) for c in (45, 16))
    mano_joints_bwd_rows(th45, det, tables, crop_uv, vis, g_log_p, N, g_th45, g_rows, laplace_b, th45_alpha, pose3d, mods, laplace_b_3d, chamfer, chamfer_w)
    return g_th45, sum_over_hypotheses(g_rows, N, det.shape[0])


def sum_over_hypotheses(rows, N, B, out=None, accumulate=False, out_stride=0):
    """out[b] (+)= sum_n rows[n*B + b]; `out` may be a view into a wider [B, out_stride] matrix"""
    Cc = rows.shape[1]
    _chk(rows, torch.float32, "sum_over_hypotheses.rows", (N * B, Cc))
    if out is None:
        out = torch.empty(B, Cc, device=rows.device, dtype=torch.float32)
    launch("mhe_sum_over_hypotheses_f32", rows, out, N, B, Cc, int(accumulate), int(out_stride))
    return out


def mano_verts(z, tables, mm=False):
    R = z.shape[0]
    _chk(z, torch.float32, "mano_verts.z", (R, 61))
    verts = torch.empty(R, 778, 3, device=z.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().mhe_mano_verts_workspace_floats(R), device=z.device, dtype=torch.float32)
    launch("mhe_mano_verts_f32", z, tables, verts, ws, R, int(mm))
    return verts


def mano_regress_joints(verts, tables):
    R = verts.shape[0]
    _chk(verts, torch.float32, "regress.verts", (R, 778, 3))
    j = torch.empty(R, 21, 3, device=verts.device, dtype=torch.float32)
    launch("mhe_mano_regress_joints_f32", verts, tables, j, R)
    return j


def mano_verts_bwd(z, tables, g_verts, mm=False, g_joints_mm=None):
    """reverse of mano_verts (and of mano_joints' mesh_mm / joints_mm with mm=True): g_verts [R,778,3] = dL/dverts of the same mode,
    g_joints_mm [R,63] | None = dL/djoints_mm -> g_z [R,61] in z's column order; the camera columns 58..60 are 0 (mhe_mano_verts_bwd_f32)"""
    R = z.shape[0]
    _chk(z, torch.float32, "mano_verts_bwd.z", (R, 61))
    _chk(tables, torch.float32, "mano_verts_bwd.tables", (_lib.lib().mhe_mano_table_floats(),))
    _chk(g_verts, torch.float32, "mano_verts_bwd.g_verts", (R, 778, 3))
    if g_joints_mm is not None:
        _chk(g_joints_mm, torch.float32, "mano_verts_bwd.g_joints_mm", (R, 63))
    g_z = torch.empty(R, 61, device=z.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().mhe_mano_verts_bwd_workspace_floats(R), device=z.device, dtype=torch.float32)
    launch("mhe_mano_verts_bwd_f32", z, tables, g_verts, g_joints_mm, g_z, ws, R, int(mm))
    return g_z


def mano_z_grad_add(g_z, g_logs_t, g_th45, g_det_rows):
    """adds the adjoint of z = gather(det, th45) into the loss pass' reverse buffers, in place (mhe_mano_z_grad_add_f32): g_z [R,61] of
    mano_verts_bwd, g_logs_t [R,3] | None (the camera columns, det[13:16]), g_th45 [R,45], g_det_rows [R,16]"""
    R = g_z.shape[0]
    _chk(g_z, torch.float32, "mano_z_grad_add.g_z", (R, 61))
    if g_logs_t is not None:
        _chk(g_logs_t, torch.float32, "mano_z_grad_add.g_logs_t", (R, 3))
    _chk(g_th45, torch.float32, "mano_z_grad_add.g_th45", (R, 45)); _chk(g_det_rows, torch.float32, "mano_z_grad_add.g_det_rows", (R, 16))
    launch("mhe_mano_z_grad_add_f32", g_z, g_logs_t, g_th45, g_det_rows, R)


def mano_regress_joints_bwd(g_joints, tables, out=None):
    """transpose of mano_regress_joints: g_joints [R,21,3] -> g_verts [R,778,3]; added to `out` when given (mhe_mano_regress_joints_bwd_f32)"""
    R = g_joints.shape[0]
    _chk(g_joints, torch.float32, "regress_bwd.g_joints", (R, 21, 3))
    _chk(tables, torch.float32, "regress_bwd.tables", (_lib.lib().mhe_mano_table_floats(),))
    if out is not None:
        _chk(out, torch.float32, "regress_bwd.out", (R, 778, 3))
    g_verts = torch.empty(R, 778, 3, device=g_joints.device, dtype=torch.float32) if out is None else out
    launch("mhe_mano_regress_joints_bwd_f32", g_joints, tables, g_verts, R, int(out is not None))
    return g_verts


def elbo_reduce(log_p_rows, log_q_rows, N, B):
    dev = log_p_rows.device
    _chk(log_p_rows, torch.float32, "elbo.log_p_rows", (N * B,))
    if log_q_rows is not None:
        _chk(log_q_rows, torch.float32, "elbo.log_q_rows", (N * B,))
    q, h, lp = (torch.empty(B, device=dev, dtype=torch.float32) for _ in range(3))
    launch("mhe_elbo_reduce_f32", log_p_rows, log_q_rows, q, h, lp, N, B)
    return q, h, lp


def topk_gather(score, rows, N, B, Q):
    """per image the Q rows of highest score, descending (torch.topk order): returns (idx [Q,B] int32, rows [Q*B,D])"""
    D = rows.shape[1]
    _chk(score, torch.float32, "topk.score", (N * B,)); _chk(rows, torch.float32, "topk.rows", (N * B, D))
    idx = torch.empty(Q, B, device=rows.device, dtype=torch.int32)
    out = torch.empty(Q * B, D, device=rows.device, dtype=torch.float32)
    launch("mhe_topk_gather_f32", score, rows, idx, out, N, B, Q, D)
    return idx, out


def kmeans_select(points, Q, score=None, iters=10):
    """k-means quantisation of a hypothesis set (include/mhe.h, mhe_kmeans_select_f32; DESIGN.md "k-means quantisation"): points [N,B,D]
    sample-major, score [N,B] or None (log q: the first seed is the row of highest score, row 0 without it), at most `iters` Lloyd rounds
    from farthest-point seeds.  Returns a dict: index [Q,B] int64 (each cluster's representative hypothesis, the member nearest the mean),
    count [Q,B] int32, assign [N,B] int32 (every row's cluster, as a position in the output order), centre [Q,B,D] f32, converged [B]
    int32.  Clusters come largest first.  One launch, one workgroup per image with the image in LDS: ValueError, before any launch, when
    (N, Q, D) does not fit the 160 KiB of a CU (kmeans_lds_bytes), for Q outside 1..N and for iters < 0."""
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or 0 in points.shape:
        raise ValueError(f"kmeans_select.points: expected a non-empty [N,B,D] tensor, got {tuple(getattr(points, 'shape', ()))}")
    N, B, D = points.shape
    if not isinstance(Q, int) or isinstance(Q, bool) or not 1 <= Q <= N:
        raise ValueError(f"kmeans_select: Q={Q!r} outside 1..N={N}")
    if not isinstance(iters, int) or isinstance(iters, bool) or iters < 0:
        raise ValueError(f"kmeans_select: iters={iters!r} (an int >= 0)")
    need, limit = kmeans_lds_bytes(N, Q, D), _lib.lib().mhe_kmeans_lds_limit()
    if need > limit:
        raise ValueError(f"kmeans_select: N={N}, Q={Q}, D={D} needs {need} bytes of LDS, over the {limit} (160 KiB) of one CU; there is no slower path")
    _chk(points, torch.float32, "kmeans_select.points")
    if score is not None:
        _chk(score, torch.float32, "kmeans_select.score", (N, B))
    dev = points.device
    index, count = (torch.empty(Q, B, device=dev, dtype=torch.int32) for _ in range(2))
    assign = torch.empty(N, B, device=dev, dtype=torch.int32)
    centre = torch.empty(Q, B, D, device=dev, dtype=torch.float32)
    converged = torch.empty(B, device=dev, dtype=torch.int32)
    launch("mhe_kmeans_select_f32", points, score, index, count, assign, centre, converged, N, B, D, Q, iters)
    return {"index": index.long(), "count": count, "assign": assign, "centre": centre, "converged": converged}


def kmeans_lds_bytes(N, Q, D):
    """the LDS one workgroup of kmeans_select takes for N points and Q centres of D coordinates (mhe_kmeans_lds_bytes)"""
    return int(_lib.lib().mhe_kmeans_lds_bytes(int(N), int(Q), int(D)))


def metrics(xyz, uv, pose3d, scale, crop_uv, vis):
    N, B = xyz.shape[:2]
    _chk(xyz, torch.float32, "metrics.xyz", (N, B, 63)); _chk(uv, torch.float32, "metrics.uv", (N, B, 42))
    _chk(pose3d, torch.float32, "metrics.pose3d", (B, 63)); _chk(scale, torch.float32, "metrics.scale", (B,))
    _chk(crop_uv, torch.float32, "metrics.crop_uv", (B, 42)); _chk(vis, torch.float32, "metrics.vis", (B, 21))
    out = torch.empty(14, B, device=xyz.device, dtype=torch.float32)
    launch("mhe_metrics_f32", xyz, uv, pose3d, scale, crop_uv, vis, out, N, B)
    return out


def metrics_split(xyz_err, xyz_spread, uv, pose3d, scale, crop_uv, vis):
    """metrics() with the 3D error rows taken of xyz_err and the 3D spread rows of xyz_spread (both [N,B,63]): the aligned
    evaluation passes the Procrustes-aligned and the unaligned joints (include/mhe.h, mhe_metrics_split_f32)"""
    N, B = xyz_err.shape[:2]
    _chk(xyz_err, torch.float32, "metrics_split.xyz_err", (N, B, 63)); _chk(xyz_spread, torch.float32, "metrics_split.xyz_spread", (N, B, 63))
    _chk(uv, torch.float32, "metrics_split.uv", (N, B, 42))
    _chk(pose3d, torch.float32, "metrics_split.pose3d", (B, 63)); _chk(scale, torch.float32, "metrics_split.scale", (B,))
    _chk(crop_uv, torch.float32, "metrics_split.crop_uv", (B, 42)); _chk(vis, torch.float32, "metrics_split.vis", (B, 21))
    out = torch.empty(14, B, device=xyz_err.device, dtype=torch.float32)
    launch("mhe_metrics_split_f32", xyz_err, xyz_spread, uv, pose3d, scale, crop_uv, vis, out, N, B)
    return out


def procrustes_align(pred, target, want_transform=False):
    """Procrustes alignment with scale of every hypothesis to its image's target (hand/utils.py:502-525 align_w_scale, without the
    determinant correction that scipy's orthogonal_procrustes also leaves out).  pred [N,B,...] and target [B,...] hold P*3
    coordinates per row (joints [N,B,63], meshes [N,B,2334] or [N,B,778,3]); returns a new tensor shaped like pred, in the
    target's unit.  want_transform: also return R [N,B,3,3] and s [N,B] of each row (M = A0^T B0 = U S V^T, R = U V^T, s = tr S)."""
    if not isinstance(pred, torch.Tensor) or pred.dim() < 3:
        raise _lib.MheError("procrustes_align.pred: expected an [N,B,...] tensor")
    N, B = pred.shape[:2]
    F = pred[0, 0].numel()
    if F % 3 or F == 0:
        raise _lib.MheError(f"procrustes_align.pred: {F} coordinates per row is not P x 3")
    _chk(pred, torch.float32, "procrustes_align.pred")
    _chk(target, torch.float32, "procrustes_align.target")
    if target.dim() < 1 or target.shape[0] != B or target[0].numel() != F:
        raise _lib.MheError(f"procrustes_align.target: expected [B={B}, ...] with {F} coordinates per image, got {tuple(target.shape)}")
    if target.device != pred.device:
        raise _lib.MheError("procrustes_align: pred and target are on different devices")
    P = F // 3
    L = _lib.lib()
    out = torch.empty_like(pred)
    nws = L.mhe_procrustes_workspace_floats(B, P)
    ws = torch.empty(nws, device=pred.device, dtype=torch.float32)
    R = torch.empty(N, B, 3, 3, device=pred.device, dtype=torch.float32) if want_transform else None
    s = torch.empty(N, B, device=pred.device, dtype=torch.float32) if want_transform else None
    launch("mhe_procrustes_align_f32", pred, target, out, R, s, ws, nws, N, B, P)
    return (out, R, s) if want_transform else out


def _chamfer_operands(points, scale, root, obj, count, who):
    if not isinstance(points, torch.Tensor) or points.dim() != 4 or points.shape[-1] != 3:
        raise _lib.MheError(f"{who}.points: expected an [N,B,P,3] tensor")
    N, B, P = points.shape[:3]
    if not isinstance(obj, torch.Tensor) or obj.dim() != 3:
        raise _lib.MheError(f"{who}.obj: expected a [B,VO,3] tensor")
    VO = obj.shape[1]
    _chk(points, torch.float32, f"{who}.points"); _chk(scale, torch.float32, f"{who}.scale", (B,)); _chk(root, torch.float32, f"{who}.root", (B, 3))
    _chk(obj, torch.float32, f"{who}.obj", (B, VO, 3))
    if count is not None:
        _chk(count, torch.int32, f"{who}.count", (B,))
    return N, B, P, VO


def chamfer(points, scale, root, obj, count=None, unit=1000.0, want_idx=False):
    """hand-object Chamfer distance (include/mhe.h, mhe_chamfer_f32): points [N,B,P,3] normalised and root-relative, scale [B], root [B,3],
    obj [B,VO,3], count [B] int32 (valid vertices per image) or None -> dist [N,B], parts [N,B,2] = (hand-to-object, object-to-hand);
    want_idx: also the argmins idx_p [N,B,P] and idx_o [N,B,VO] (int32) that chamfer_bwd reads"""
    N, B, P, VO = _chamfer_operands(points, scale, root, obj, count, "chamfer")
    dev = points.device
    dist = torch.empty(N, B, device=dev, dtype=torch.float32)
    parts = torch.empty(N, B, 2, device=dev, dtype=torch.float32)
    idx_p = torch.empty(N, B, P, device=dev, dtype=torch.int32) if want_idx else None
    idx_o = torch.empty(N, B, VO, device=dev, dtype=torch.int32) if want_idx else None
    launch("mhe_chamfer_f32", points, scale, root, obj, count, dist, parts, idx_p, idx_o, N, B, P, VO, float(unit))
    return (dist, parts, idx_p, idx_o) if want_idx else (dist, parts)


def chamfer_bwd(points, scale, root, obj, count, idx_p, idx_o, g_dist, unit=1000.0):
    """reverse of chamfer's dist with respect to points (mhe_chamfer_bwd_f32): idx_p / idx_o of the forward call, g_dist [N,B] -> [N,B,P,3]"""
    N, B, P, VO = _chamfer_operands(points, scale, root, obj, count, "chamfer_bwd")
    _chk(idx_p, torch.int32, "chamfer_bwd.idx_p", (N, B, P)); _chk(idx_o, torch.int32, "chamfer_bwd.idx_o", (N, B, VO))
    _chk(g_dist, torch.float32, "chamfer_bwd.g_dist", (N, B))
    g_points = torch.empty_like(points)
    launch("mhe_chamfer_bwd_f32", points, scale, root, obj, count, idx_p, idx_o, g_dist, g_points, N, B, P, VO, float(unit))
    return g_points


MESH_EVAL_MAX_VERTS, MESH_EVAL_MAX_THRESHOLDS = 778, 4         # MHE_CHAMFER_MAX_POINTS / MHE_MESH_EVAL_MAX_THRESHOLDS of include/mhe.h


def mesh_eval(pred, target, scale, thresholds, unit=1000.0):
    """hand mesh evaluation (include/mhe.h, mhe_mesh_eval_f32): pred [N,B,V,3], target [B,V,3], scale [B], thresholds = 1 to 4 numbers in the
    output's unit (unit 1000: mm) -> err [N,B], the mean vertex-to-vertex distance by correspondence, and prf [3,T,N,B] = (precision, recall,
    F-score) of the two vertex sets at every threshold (nearest distance strictly below it)"""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or pred.shape[-1] != 3:
        raise _lib.MheError("mesh_eval.pred: expected an [N,B,V,3] tensor")
    N, B, V = pred.shape[:3]
    _chk(pred, torch.float32, "mesh_eval.pred"); _chk(target, torch.float32, "mesh_eval.target", (B, V, 3)); _chk(scale, torch.float32, "mesh_eval.scale", (B,))
    thr = [float(t) for t in thresholds]
    T = len(thr)
    if not 1 <= T <= MESH_EVAL_MAX_THRESHOLDS:
        raise _lib.MheError(f"mesh_eval.thresholds: {T} thresholds (1..{MESH_EVAL_MAX_THRESHOLDS})")
    err = torch.empty(N, B, device=pred.device, dtype=torch.float32)
    prf = torch.empty(3, T, N, B, device=pred.device, dtype=torch.float32)
    arr = (C.c_float * T)(*thr)
    launch("mhe_mesh_eval_f32", pred, target, scale, C.cast(arr, C.c_void_p), err, prf, N, B, V, T, float(unit))
    return err, prf


PCK_MAX_POINTS, PCK_MAX_THRESHOLDS = 778, 256         # MHE_PCK_MAX_POINTS / MHE_PCK_MAX_THRESHOLDS of include/mhe.h
_PCK_TABLES = {}          # (f32 bytes of the thresholds, device) -> the uploaded table


def pck_thresholds(values, device):
    """a Python sequence of thresholds -> the device f32 table [T] mhe_pck_curve_f32 reads: checked here for 2..256 finite values that are
    strictly ascending as f32, uploaded once per (values, device) and kept.  The first call with a new sequence copies from the host: make it
    before a HIP graph is captured, not inside the capture (a later call with the same values only looks the table up).  The tables (1 KB at
    most each) are kept for the life of the process, like the grow-only workspaces: a captured graph may have baked a table's address in, so
    none is ever dropped - pass a device tensor of your own where the values change from call to call."""
    try:
        thr = np.asarray([float(t) for t in values], np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise _lib.MheError(f"pck_curve.thresholds: expected a device tensor or a sequence of numbers, got {values!r}") from None
    if not 2 <= thr.size <= PCK_MAX_THRESHOLDS:
        raise _lib.MheError(f"pck_curve.thresholds: {thr.size} thresholds (2..{PCK_MAX_THRESHOLDS})")
    if not np.isfinite(thr).all() or not (np.diff(thr) > 0).all():
        raise _lib.MheError("pck_curve.thresholds: must be finite and strictly ascending as float32")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.MheError("pck_curve.thresholds: expected a CUDA/HIP device (the hot path has no CPU fallback)")
    key = (thr.tobytes(), device.index if device.index is not None else torch.cuda.current_device())
    table = _PCK_TABLES.get(key)
    if table is None:
        table = _PCK_TABLES[key] = torch.from_numpy(thr).to(device)
    return table


def pck_curve(pred, target, scale, thresholds, valid=None, unit=1000.0, want_hits=True):
    """3D PCK curve (include/mhe.h, mhe_pck_curve_f32): pred [N,B,P,3], target [B,P,3], scale [B], thresholds = a device f32 tensor [T], taken as
    given (strictly ascending is the caller's word: nothing is read on the host), or a Python sequence (pck_thresholds), in the output's unit
    (unit 1000: mm); valid [B,P] bool / uint8 or None (all points) -> (hits [N,B,T] int32, the valid points within each threshold (inclusive),
    or None without want_hits; auc [N,B], the normalised trapezoid area under hits / n_valid; err [N,B], the mean distance over the valid points)"""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or pred.shape[-1] != 3:
        raise _lib.MheError("pck_curve.pred: expected an [N,B,P,3] tensor")
    N, B, P = pred.shape[:3]
    _chk(pred, torch.float32, "pck_curve.pred"); _chk(target, torch.float32, "pck_curve.target", (B, P, 3)); _chk(scale, torch.float32, "pck_curve.scale", (B,))
    if isinstance(thresholds, torch.Tensor):
        _chk(thresholds, torch.float32, "pck_curve.thresholds")
        if thresholds.dim() != 1 or not 2 <= thresholds.shape[0] <= PCK_MAX_THRESHOLDS:
            raise _lib.MheError(f"pck_curve.thresholds: expected a [T] tensor with T in 2..{PCK_MAX_THRESHOLDS}, got {tuple(thresholds.shape)}")
    else:
        thresholds = pck_thresholds(thresholds, pred.device)
    T = thresholds.shape[0]
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
            raise _lib.MheError(f"pck_curve.valid: expected a bool or uint8 tensor, got {getattr(valid, 'dtype', type(valid))}")
        _chk(valid, valid.dtype, "pck_curve.valid", (B, P))
    hits = torch.empty(N, B, T, device=pred.device, dtype=torch.int32) if want_hits else None
    auc = torch.empty(N, B, device=pred.device, dtype=torch.float32)
    err = torch.empty(N, B, device=pred.device, dtype=torch.float32)
    launch("mhe_pck_curve_f32", pred, target, scale, valid, thresholds, float(unit), hits, auc, err, N, B, P, T)
    return hits, auc, err


SILHOUETTE_MAX_SIZE, SILHOUETTE_MAX_VERTS = 64, 778         # MHE_SILHOUETTE_MAX_SIZE / _MAX_VERTS of include/mhe.h


def silhouette_pixels(hand_mask, size=64, occluder=None):
    """kept pixels of every image's hand mask (include/mhe.h, mhe_silhouette_pixels): hand_mask [B,H,H] bool / uint8 (non-zero counts as 1) or
    float32 in [0,1], H a multiple of size -> pixels [B,size*size] int32, packed (i << 16) | j in row-major order and -1 past the count, and
    count [B] int32, which stays on the device.  occluder [B,H,H] (the same types; mhe_silhouette_pixels_occ): its kept pixels that are not
    the hand's follow the hand's in the list -> (pixels, count, count_all), count_all [B] int32 the length of both sections"""
    if not isinstance(hand_mask, torch.Tensor) or hand_mask.dim() != 3 or hand_mask.shape[1] != hand_mask.shape[2]:
        raise _lib.MheError("silhouette_pixels.hand_mask: expected a [B,H,H] tensor")
    B, H, S = hand_mask.shape[0], hand_mask.shape[1], int(size)
    if hand_mask.dtype not in (torch.bool, torch.uint8, torch.float32):
        raise _lib.MheError(f"silhouette_pixels.hand_mask: expected bool, uint8 or float32, got {hand_mask.dtype}")
    _chk(hand_mask, hand_mask.dtype, "silhouette_pixels.hand_mask")
    if occluder is not None:
        if not isinstance(occluder, torch.Tensor) or occluder.dtype not in (torch.bool, torch.uint8, torch.float32):
            raise _lib.MheError(f"silhouette_pixels.occluder: expected a bool, uint8 or float32 tensor, got {getattr(occluder, 'dtype', type(occluder))}")
        _chk(occluder, occluder.dtype, "silhouette_pixels.occluder", (B, H, H))
    if not 1 <= S <= SILHOUETTE_MAX_SIZE or B < 1 or H < S or H % S:
        raise ValueError(f"silhouette_pixels: B={B} H={H} size={S} (B >= 1, size in 1..{SILHOUETTE_MAX_SIZE}, H a multiple of size)")
    pixels = torch.empty(B, S * S, device=hand_mask.device, dtype=torch.int32)
    count = torch.empty(B, device=hand_mask.device, dtype=torch.int32)
    if occluder is None:
        launch("mhe_silhouette_pixels", hand_mask, int(hand_mask.dtype == torch.float32), pixels, count, B, H, S)
        return pixels, count
    count_all = torch.empty_like(count)
    launch("mhe_silhouette_pixels_occ", hand_mask, int(hand_mask.dtype == torch.float32), occluder, int(occluder.dtype == torch.float32), pixels, count,
           count_all, B, H, S)
    return pixels, count, count_all


def _silhouette_entry(name, count_all, B, who):
    """the entry and the operand that follows count: (name, ()) without an occluder section, (name_occ, (count_all,)) with one"""
    if count_all is None:
        return f"mhe_silhouette_{name}_f32", ()
    _chk(count_all, torch.int32, f"{who}.count_all", (B,))
    return f"mhe_silhouette_{name}_occ_f32", (count_all,)


def _silhouette_operands(verts, logs_t, pixels, count, who):
    if not isinstance(verts, torch.Tensor) or verts.dim() != 4 or verts.shape[-1] != 3:
        raise _lib.MheError(f"{who}.verts: expected an [N,B,V,3] tensor")
    if not isinstance(pixels, torch.Tensor) or pixels.dim() != 2:
        raise _lib.MheError(f"{who}.pixels: expected a [B,size*size] tensor")
    N, B, V = verts.shape[:3]
    P = pixels.shape[1]
    S = int(round(P ** 0.5))
    if S * S != P or not 1 <= S <= SILHOUETTE_MAX_SIZE:
        raise ValueError(f"{who}: pixels has {P} columns, not size*size with size in 1..{SILHOUETTE_MAX_SIZE}")
    if not 1 <= V <= SILHOUETTE_MAX_VERTS:
        raise ValueError(f"{who}: V={V} vertices (1..{SILHOUETTE_MAX_VERTS})")
    _chk(verts, torch.float32, f"{who}.verts"); _chk(logs_t, torch.float32, f"{who}.logs_t", (N, B, 3))
    _chk(pixels, torch.int32, f"{who}.pixels", (B, P)); _chk(count, torch.int32, f"{who}.count", (B,))
    return N, B, V, S


def silhouette_dist(verts, logs_t, pixels, count, want_idx=False, count_all=None):
    """silhouette distance of every hypothesis' projected vertices to its image's kept pixels (include/mhe.h, mhe_silhouette_dist_f32): verts
    [N,B,V,3], logs_t [N,B,3] = (log s, tx, ty), pixels / count of silhouette_pixels -> dist [N,B], parts [N,B,2] = (inside, cover);
    want_idx: also the argmins idx_v [N,B,V] and idx_m [N,B,size*size] (int32) that silhouette_dist_bwd reads.  count_all [B] (the third
    result of silhouette_pixels(occluder=...); mhe_silhouette_dist_occ_f32): the vertices' minima also run over the list's occluder section"""
    N, B, V, S = _silhouette_operands(verts, logs_t, pixels, count, "silhouette_dist")
    dev = verts.device
    dist = torch.empty(N, B, device=dev, dtype=torch.float32)
    parts = torch.empty(N, B, 2, device=dev, dtype=torch.float32)
    idx_v = torch.empty(N, B, V, device=dev, dtype=torch.int32) if want_idx else None
    idx_m = torch.empty(N, B, S * S, device=dev, dtype=torch.int32) if want_idx else None
    entry, occ = _silhouette_entry("dist", count_all, B, "silhouette_dist")
    launch(entry, verts, logs_t, pixels, count, *occ, dist, parts, idx_v, idx_m, N, B, V, S)
    return (dist, parts, idx_v, idx_m) if want_idx else (dist, parts)


def silhouette_dist_bwd(verts, logs_t, pixels, count, idx_v, idx_m, g_dist, count_all=None):
    """reverse of silhouette_dist's dist (mhe_silhouette_dist_bwd_f32): idx_v / idx_m of the forward call, g_dist [N,B] -> g_verts [N,B,V,3]
    (its z column is zero), g_logs_t [N,B,3]; count_all: the forward call's"""
    N, B, V, S = _silhouette_operands(verts, logs_t, pixels, count, "silhouette_dist_bwd")
    _chk(idx_v, torch.int32, "silhouette_dist_bwd.idx_v", (N, B, V)); _chk(idx_m, torch.int32, "silhouette_dist_bwd.idx_m", (N, B, S * S))
    _chk(g_dist, torch.float32, "silhouette_dist_bwd.g_dist", (N, B))
    g_verts, g_logs_t = torch.empty_like(verts), torch.empty_like(logs_t)
    entry, occ = _silhouette_entry("dist_bwd", count_all, B, "silhouette_dist_bwd")
    launch(entry, verts, logs_t, pixels, count, *occ, idx_v, idx_m, g_dist, g_verts, g_logs_t, N, B, V, S)
    return g_verts, g_logs_t


def silhouette_dist_grad(verts, logs_t, pixels, count, g_dist, want_dist=False, count_all=None):
    """silhouette_dist(want_idx=True) + silhouette_dist_bwd in one launch, without the two index tensors (mhe_silhouette_dist_grad_f32: the
    argmins stay in registers and LDS): g_dist [N,B] -> (g_verts [N,B,V,3], g_logs_t [N,B,3]), with want_dist (dist [N,B], g_verts, g_logs_t);
    count_all as in silhouette_dist (mhe_silhouette_dist_grad_occ_f32)"""
    N, B, V, S = _silhouette_operands(verts, logs_t, pixels, count, "silhouette_dist_grad")
    _chk(g_dist, torch.float32, "silhouette_dist_grad.g_dist", (N, B))
    dist = torch.empty(N, B, device=verts.device, dtype=torch.float32) if want_dist else None
    g_verts, g_logs_t = torch.empty_like(verts), torch.empty_like(logs_t)
    entry, occ = _silhouette_entry("dist_grad", count_all, B, "silhouette_dist_grad")
    launch(entry, verts, logs_t, pixels, count, *occ, g_dist, dist, g_verts, g_logs_t, N, B, V, S)
    return (dist, g_verts, g_logs_t) if want_dist else (g_verts, g_logs_t)


RENDER_OUTPUTS = ("mask", "depth", "iou_sums")


def _faces_index_range(faces):
    """(lowest, highest) index of a faces tensor: one host read per tensor (and per in-place change of it), kept on the tensor"""
    cached = getattr(faces, "_mhe_index_range", None)
    if cached is None or cached[0] != faces._version:
        cached = (faces._version, int(faces.min()), int(faces.max()))
        faces._mhe_index_range = cached
    return cached[1:]


def render_mesh(verts, faces, scale, trans, zscale=None, size=64, anti_aliasing=True, far=100.0, want=("mask",), target=None):
    """silhouette and depth of R meshes under the orthographic camera p = |scale| v_xy + trans (include/mhe.h, mhe_render_mesh_f32, whose
    comment is the contract): verts [R,V,3], faces [F,3] int32 (one set for all rows), scale [R] or [R,1], trans [R,2], zscale [R] or None
    (depth = v_z zscale / 1000, v_z without it) -> dict of the outputs named in `want`: 'mask' [R,size,size] in [0,1] (multiples of 1/4 with
    anti_aliasing, which renders at 2 size and averages), 'depth' [R,size,size] (`far` where nothing covers) and 'iou_sums' [R,2] =
    (sum min(mask, target), sum max(mask, target)) against target [B,size,size] in [0,1], row r against image r % B.  With
    want=('iou_sums',) no image is allocated or written.  ValueError for a face index outside [0,V) (checked once per faces tensor)."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 3 or verts.shape[-1] != 3:
        raise _lib.MheError("render_mesh.verts: expected an [R,V,3] tensor")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[-1] != 3:
        raise _lib.MheError("render_mesh.faces: expected an [F,3] tensor")
    R, V, F, S = verts.shape[0], verts.shape[1], faces.shape[0], int(size)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in RENDER_OUTPUTS for k in want):
        raise ValueError(f"render_mesh: want={want!r} (any of {RENDER_OUTPUTS})")
    if "iou_sums" in want and target is None:
        raise ValueError("render_mesh: 'iou_sums' needs target=")
    if not 8 <= S <= 256:
        raise ValueError(f"render_mesh: size={S} (8..256)")
    _chk(verts, torch.float32, "render_mesh.verts"); _chk(faces, torch.int32, "render_mesh.faces")
    if isinstance(scale, torch.Tensor) and tuple(scale.shape) == (R, 1):
        scale = scale.view(R)
    _chk(scale, torch.float32, "render_mesh.scale", (R,)); _chk(trans, torch.float32, "render_mesh.trans", (R, 2))
    if zscale is not None:
        _chk(zscale, torch.float32, "render_mesh.zscale", (R,))
    B = 1
    if target is not None:
        if not isinstance(target, torch.Tensor) or target.dim() != 3:
            raise _lib.MheError("render_mesh.target: expected a [B,size,size] tensor")
        B = target.shape[0]
        _chk(target, torch.float32, "render_mesh.target", (B, S, S))
        if B < 1 or R % B:
            raise ValueError(f"render_mesh: R={R} rows are not a multiple of the B={B} target images")
    if R < 1 or V < 1 or F < 1:
        raise ValueError(f"render_mesh: R={R} V={V} F={F} (each >= 1)")
    lo, hi = _faces_index_range(faces)
    if lo < 0 or hi >= V:
        raise ValueError(f"render_mesh: faces index {lo}..{hi} outside the V={V} vertices")
    shapes = {"mask": (R, S, S), "depth": (R, S, S), "iou_sums": (R, 2)}
    o = {k: (torch.empty(shapes[k], device=verts.device, dtype=torch.float32) if k in want else None) for k in RENDER_OUTPUTS}
    launch("mhe_render_mesh_f32", verts, faces, scale, trans, zscale, target, o["mask"], o["depth"], o["iou_sums"], R, B, V, F, S, int(bool(anti_aliasing)),
           float(far))
    return {k: v for k, v in o.items() if v is not None}


DEPTH_MAX_SIZE, DEPTH_MAX_VERTS, DEPTH_MAX_FACES = 64, 1024, 2048         # MHE_DEPTH_MAX_SIZE / _MAX_VERTS / _MAX_FACES of include/mhe.h


def depth_obs(depth, hand_mask, size=64):
    """the observation image of depth_dist: depth [B,H,H] (metres, 0 where the sensor saw nothing) and hand_mask [B,H,H] (bool, uint8 or float
    in [0,1]), H a multiple of size -> obs [B,size,size] f32.  With k = H / size, sample (i, j) is depth[b, i k + k//2, j k + k//2] (one sample,
    never a mean: depth is not averaged across a discontinuity) where the box mean of the mask over the k x k block is >= 0.5 and the sample is
    finite and > 0, and 0 elsewhere.  torch ops only, nothing is read back; works on any device."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or depth.shape[1] != depth.shape[2]:
        raise ValueError(f"depth_obs: depth must be (B, H, H), got {tuple(getattr(depth, 'shape', ()))}")
    if not isinstance(hand_mask, torch.Tensor) or tuple(hand_mask.shape) != tuple(depth.shape):
        raise ValueError(f"depth_obs: hand_mask must be (B, H, H) = {tuple(depth.shape)} like depth, got {tuple(getattr(hand_mask, 'shape', ()))}")
    B, H, S = depth.shape[0], depth.shape[1], size
    if not isinstance(S, int) or not 1 <= S <= DEPTH_MAX_SIZE:
        raise ValueError(f"depth_obs: size={S!r} (1..{DEPTH_MAX_SIZE})")
    if H < S or H % S:
        raise ValueError(f"depth_obs: depth is {H} x {H}, not a multiple of size={S}")
    k = H // S
    sample = depth[:, k // 2::k, k // 2::k].float()
    kept = hand_mask.view(B, S, k, S, k).to(torch.float64).sum((2, 4)) >= 0.5 * k * k
    valid = kept & torch.isfinite(sample) & (sample > 0)
    return torch.where(valid, sample, torch.zeros_like(sample)).contiguous()


def face_adjacency(faces, V=None):
    """the vertex -> face table mhe_depth_dist_bwd_f32 reads, built once per faces tensor on the host (and per in-place change of it; one host
    read, so the first call must not fall into a stream capture) and kept on the tensor: faces [F,3] int32 -> (vf_start [V+1], vf_list [3F]) int32
    on the faces' device.  Entries vf_start[v] .. vf_start[v+1]-1 of vf_list are (face << 2) | corner for every corner that is vertex v, ascending;
    a face with an index outside [0,V) has no entry (the kernels skip it); the tail of the list is -1.  V: the vertex count, the highest index
    + 1 when not given."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[-1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"face_adjacency: faces must be an (F, 3) int32 tensor, got {tuple(getattr(faces, 'shape', ()))} {getattr(faces, 'dtype', None)}")
    cache = getattr(faces, "_mhe_adjacency", None)
    if cache is None or cache[0] != faces._version:
        cache = (faces._version, {})
        faces._mhe_adjacency = cache
    if V is None:
        V = max(int(faces.max()) + 1, 1)
    if V not in cache[1]:
        f = faces.detach().cpu().numpy().astype(np.int64)
        ok = ((f >= 0) & (f < V)).all(1)
        ent = (np.arange(f.shape[0])[:, None] * 4 + np.arange(3)[None, :])[ok].reshape(-1)
        vert = f[ok].reshape(-1)
        order = np.argsort(vert, kind="stable")          # entries ascend already: a stable sort by vertex keeps them so
        start = np.concatenate([[0], np.cumsum(np.bincount(vert, minlength=V))]).astype(np.int32)
        lst = np.full(3 * f.shape[0], -1, np.int32)
        lst[:ent.size] = ent[order]
        cache[1][V] = (torch.as_tensor(start).to(faces.device), torch.as_tensor(lst).to(faces.device))
    return cache[1][V]


def _depth_operands(who, verts, faces, logs_t, zscale, obs, root_z, trunc):
    if not isinstance(verts, torch.Tensor) or verts.dim() != 4 or verts.shape[-1] != 3:
        raise _lib.MheError(f"{who}.verts: expected an [N,B,V,3] tensor")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[-1] != 3:
        raise _lib.MheError(f"{who}.faces: expected an [F,3] tensor")
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[1] != obs.shape[2]:
        raise _lib.MheError(f"{who}.obs: expected a [B,size,size] tensor")
    N, B, V = verts.shape[:3]
    F, S = faces.shape[0], obs.shape[1]
    if N < 1 or B < 1 or not 1 <= V <= DEPTH_MAX_VERTS or not 1 <= F <= DEPTH_MAX_FACES or not 1 <= S <= DEPTH_MAX_SIZE:
        raise ValueError(f"{who}: N={N} B={B} V={V} F={F} size={S} (N, B >= 1, V in 1..{DEPTH_MAX_VERTS}, F in 1..{DEPTH_MAX_FACES}, "
                         f"size in 1..{DEPTH_MAX_SIZE})")
    if not float(trunc) > 0 or float(trunc) == float("inf"):
        raise ValueError(f"{who}: trunc={trunc!r} (positive and finite)")
    _chk(verts, torch.float32, f"{who}.verts"); _chk(faces, torch.int32, f"{who}.faces"); _chk(logs_t, torch.float32, f"{who}.logs_t", (N, B, 3))
    _chk(zscale, torch.float32, f"{who}.zscale", (B,)); _chk(obs, torch.float32, f"{who}.obs", (B, S, S))
    if root_z is not None:
        _chk(root_z, torch.float32, f"{who}.root_z", (B,))
    return N, B, V, F, S


def depth_dist(verts, faces, logs_t, zscale, obs, root_z=None, trunc=0.05, want_images=False):
    """depth agreement of every hypothesis' rendered mesh with its image's observed depth (include/mhe.h, mhe_depth_dist_f32, whose comment is the
    contract): verts [N,B,V,3], faces [F,3] int32, logs_t [N,B,3] = (log s, tx, ty), zscale [B] (metres per normalised unit), obs [B,size,size]
    of depth_obs, root_z [B] or None (the offset is then fitted per hypothesis) -> dist [N,B] in metres, parts [N,B,3] = (overlap, offset,
    inliers); want_images: also face_img [N,B,size,size] int32 (-1 where nothing covers) and resid_img [N,B,size,size] (NaN outside the
    compared set), which exist for tests and debugging - the product path writes no image."""
    N, B, V, F, S = _depth_operands("depth_dist", verts, faces, logs_t, zscale, obs, root_z, trunc)
    dev = verts.device
    dist = torch.empty(N, B, device=dev, dtype=torch.float32)
    parts = torch.empty(N, B, 3, device=dev, dtype=torch.float32)
    face_img = torch.empty(N, B, S, S, device=dev, dtype=torch.int32) if want_images else None
    resid_img = torch.empty(N, B, S, S, device=dev, dtype=torch.float32) if want_images else None
    launch("mhe_depth_dist_f32", verts, faces, logs_t, zscale, obs, root_z, float(trunc), dist, parts, face_img, resid_img, N, B, V, F, S)
    return (dist, parts, face_img, resid_img) if want_images else (dist, parts)


def depth_dist_bwd(verts, faces, logs_t, zscale, obs, root_z, trunc, g_dist, adjacency=None):
    """reverse of depth_dist's dist (mhe_depth_dist_bwd_f32): the forward call's operands, g_dist [N,B] -> g_verts [N,B,V,3], g_logs_t [N,B,3].
    It rasterises again - nothing of the forward call is kept - and is bit-reproducible.  adjacency: face_adjacency(faces, V), looked up (and
    built on first use) when not given."""
    N, B, V, F, S = _depth_operands("depth_dist_bwd", verts, faces, logs_t, zscale, obs, root_z, trunc)
    _chk(g_dist, torch.float32, "depth_dist_bwd.g_dist", (N, B))
    vf_start, vf_list = face_adjacency(faces, V) if adjacency is None else adjacency
    _chk(vf_start, torch.int32, "depth_dist_bwd.vf_start", (V + 1,)); _chk(vf_list, torch.int32, "depth_dist_bwd.vf_list", (3 * F,))
    g_verts, g_logs_t = torch.empty_like(verts), torch.empty_like(logs_t)
    launch("mhe_depth_dist_bwd_f32", verts, faces, logs_t, zscale, obs, root_z, float(trunc), vf_start, vf_list, g_dist, g_verts, g_logs_t, N, B, V, F, S)
    return g_verts, g_logs_t


def conv2d_nhwc(x, w, KH, KW, stride, pad, in_scale=None, in_shift=None, relu_in=False, out_scale=None,
                out_shift=None, residual=None, relu_out=False, stats=None, out=None, mask=None, bn=None, tile=0, res_half=False, xcat=None,
                mask_bits=None):
    """x [B,H,W,Cin], w packed [Cout, Kpad]; returns y [B,Ho,Wo,Cout] of x.dtype.  mask (shaped like y, data-gradient
    form only): y = (conv + residual) * [mask > 0]; bn = up to two (bn_y, mean_invstd [2,C], stats [S,2,C]) triples: the epilogue
    also accumulates the BatchNorm-reverse sums of y for those units (see mhe_conv2d_masked_nhwc).  tile > 0 forces kernel
    variant tile-1 (mhe_conv_desc.tile; tests and tuning)."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    dt = x.dtype
    _chk(x, dt, "conv.x"); _chk(w, dt, "conv.w")
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    y = out if out is not None else torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=dt)
    _chk(y, dt, "conv.y", (B, Ho, Wo, Cout))
    for t, n, c in ((in_scale, "in_scale", Cin), (in_shift, "in_shift", Cin), (out_scale, "out_scale", Cout),
                    (out_shift, "out_shift", Cout)):
        if t is not None:
            _chk(t, torch.float32, "conv." + n, (c,))
    if residual is not None:
        _chk(residual, dt, "conv.residual", (B, (Ho + 1) // 2, (Wo + 1) // 2, Cout) if res_half else (B, Ho, Wo, Cout))
    if stats is not None:
        _chk_stats(stats, "conv.stats", Cout)
    d = ConvDesc(B, H, W, Cin, Cout, KH, KW, stride, pad, dtype_code(dt), int(relu_in), int(relu_out), int(tile), int(res_half))
    if mask is not None:
        if in_scale is not None or out_scale is not None or stats is not None or relu_in or relu_out:
            raise ValueError("conv2d_nhwc: mask= is the plain data-gradient form (no affine / statistics / relu; out_shift = a per-channel constant)")
        _chk(mask, dt, "conv.mask", (B, Ho, Wo, Cout))
        if out_shift is not None:        # y = (conv + out_shift + residual) [mask > 0], one consumer's sums at most
            ext = _bn_consumers(bn, 1, dt, y.shape, Cout, "conv", only_one="conv2d_nhwc: out_shift= with mask= takes one bn consumer")
            cin2 = 0
            if xcat is not None:         # the operand's K range continued on a second tensor: w is [Cout][Cin + cin2]
                cin2 = xcat.shape[-1]
                _chk(xcat, dt, "conv.xcat", (B, H, W, cin2))
                if tuple(w.shape) != (Cout, Cin + cin2):
                    raise ValueError(f"conv2d_nhwc: xcat= needs w [{Cout}, {Cin + cin2}], got {tuple(w.shape)}")
            with _dg_timed(d, x, y, w, residual, mask, None, ext[:1], "cat" if xcat is not None else "bias", xcat):
                launch("mhe_conv2d_masked_bias_nhwc", C.byref(d), x, xcat, int(cin2), w, y, residual, mask, out_shift, *ext)
            return y
        if xcat is not None:
            raise ValueError("conv2d_nhwc: xcat= comes with mask= and out_shift=")
        ext = _bn_consumers(bn, 2, dt, y.shape, Cout, "conv")
        if mask_bits is not None:        # the gate also as bits [pixel][Cout / 8] (bottleneck_tail want_bits=): read instead of `mask` where the kernel can
            _chk(mask_bits, torch.uint8, "conv.mask_bits", (B, Ho, Wo, Cout // 8))
            with _dg_timed(d, x, y, w, residual, mask, mask_bits, [b[0] for b in (bn or [])], "bits"):
                launch("mhe_conv2d_masked_bits_nhwc", C.byref(d), x, w, y, residual, mask, mask_bits, *ext)
            return y
        with _dg_timed(d, x, y, w, residual, mask, None, [b[0] for b in (bn or [])], ""):
            launch("mhe_conv2d_masked_nhwc", C.byref(d), x, w, y, residual, mask, *ext)
        return y
    if bn:
        raise ValueError("conv2d_nhwc: bn= needs mask= (data-gradient form)")
    if xcat is not None:                 # ungated product on two operand tensors (+ out_shift as a per-channel constant, + residual)
        if in_scale is not None or out_scale is not None or stats is not None or relu_in or relu_out:
            raise ValueError("conv2d_nhwc: xcat= without mask= takes out_shift and residual only")
        cin2 = xcat.shape[-1]
        _chk(xcat, dt, "conv.xcat", (B, H, W, cin2))
        if tuple(w.shape) != (Cout, Cin + cin2):
            raise ValueError(f"conv2d_nhwc: xcat= needs w [{Cout}, {Cin + cin2}], got {tuple(w.shape)}")
        launch("mhe_conv1x1_cat_bias_nhwc", C.byref(d), x, xcat, int(cin2), w, y, residual, out_shift)
        return y
    # (algorithmic HBM bytes: input once, output once, weights once (+ residual))
    with _Timed(lambda: (_conv_kernel_name(d, dt, 1 if in_scale is not None else 3 if residual is not None else 0), 2.0 * B * Ho * Wo * Cout * KH * KW * Cin,
                         x.element_size() * (x.numel() + y.numel() + w.numel() + (residual.numel() if residual is not None else 0)))):
        launch("mhe_conv2d_nhwc", C.byref(d), x, w, y, in_scale, in_shift, out_scale, out_shift, residual, stats)
    return y


def conv1x1_stats(x, w, in_scale, in_shift, stats):
    """batch statistics of conv1x1(relu(x * in_scale + in_shift), w) as it would be stored, without storing it (mhe_conv1x1_stats_nhwc)"""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    _chk(x, torch.bfloat16, "conv_stats.x"); _chk(w, torch.bfloat16, "conv_stats.w", (Cout, Cin))
    _chk(in_scale, torch.float32, "conv_stats.in_scale", (Cin,)); _chk(in_shift, torch.float32, "conv_stats.in_shift", (Cin,))
    _chk_stats(stats, "conv_stats.stats", Cout)
    d = ConvDesc(B, H, W, Cin, Cout, 1, 1, 1, 0, BF16, 1, 0, 0, 0)
    name = "mhe::conv::conv_wide_kernel<128, 4, true>" if Cin == 256 else "mhe::conv::conv1x1_stream_kernel<%d, 256, true, false>" % (Cin // 64)
    with _Timed(lambda: (name, 2.0 * B * H * W * Cout * Cin, 2 * (x.numel() + w.numel()))):
        launch("mhe_conv1x1_stats_nhwc", C.byref(d), x, w, in_scale, in_shift, stats)
    return stats


def gram_buffers(Cb, device):
    """(partial-slab workspace, f64 totals) for conv1x1_gram_bn: every workgroup of the Gram launch stores its partial sums as a slab, the
    finalize sums the slabs in slab order (csrc/conv_gram.hip) - nothing to clear between steps"""
    L = _lib.lib()
    return (torch.zeros(L.mhe_gram_stats_words(Cb), device=device, dtype=STAT_DTYPE),
            torch.empty(L.mhe_gram_stats_workspace_bytes(Cb) // 8, device=device, dtype=torch.float64))


def conv1x1_gram_bn(x, in_scale, in_shift, w, bn_weight, bn_bias, running_mean, running_var, bufs, momentum=0.1, eps=1e-5, num_batches_tracked=None,
                    want_mean_invstd=False, a_out=None):
    """train-mode BatchNorm affine (scale, shift) of conv1x1(relu(x * in_scale + in_shift), w) from the Gram matrix of the convolution's
    INPUT - the product itself is never evaluated (mhe_conv1x1_gram_nhwc + mhe_gram_bn_finalize; csrc/conv_gram.hip)"""
    B, H, W, Cb = x.shape
    Cn = w.shape[0]
    _chk(x, torch.bfloat16, "gram.x"); _chk(w, torch.bfloat16, "gram.w", (Cn, Cb))
    _chk(in_scale, torch.float32, "gram.in_scale", (Cb,)); _chk(in_shift, torch.float32, "gram.in_shift", (Cb,))
    gram, ws = bufs
    L = _lib.lib()
    _chk(gram, STAT_DTYPE, "gram.accumulators", (L.mhe_gram_stats_words(Cb),))
    if a_out is not None:        # also relu(x * in_scale + in_shift) itself, as the matrix cores multiplied it
        _chk(a_out, torch.bfloat16, "gram.a_out", (B, H, W, Cb))
    with _Timed(lambda: ("mhe::conv::gram_kernel<%d>" % Cb, 2.0 * B * H * W * Cb * Cb, 2 * x.numel())):
        launch("mhe_conv1x1_gram_store_nhwc", x, in_scale, in_shift, 1, gram, a_out, B * H * W, Cb)
    scale = torch.empty(Cn, device=x.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    mi = torch.empty(2, Cn, device=x.device, dtype=torch.float32) if want_mean_invstd else None
    launch("mhe_gram_bn_finalize", gram, ws, w, bn_weight, bn_bias, running_mean, running_var, scale, shift, mi, Cn, Cb, float(B * H * W), float(momentum),
           float(eps), num_batches_tracked)
    return (scale, shift, mi) if want_mean_invstd else (scale, shift)


def gram_workspace(Cb, device):
    """an f64 workspace of conv1x1_gram_bn of one's own (its totals - Gram matrix [Cb][Cb], then column sums [Cb] - stay valid until reused)"""
    return torch.empty(_lib.lib().mhe_gram_stats_workspace_bytes(Cb) // 8, device=device, dtype=torch.float64)


def conv3_bn_fold(D, w, gram_totals, rev_stats, gamma, mean_invstd, count, dgamma, dbeta, dW, w_dg, S, c0, coef_ws):
    """reverse of conv3 + train-mode BatchNorm from D = g^T A and the forward's Gram statistics (mhe_conv3_bn_fold; csrc/conv_fold.hip).
    S=None: w_dg is [Cb][C + Cb] and receives [(k2 W)^T | S] - the weights of ONE K-concatenated data-gradient launch (conv2d_nhwc xcat=)"""
    Cn, Cb = w.shape
    if S is None:
        _chk(w_dg, torch.bfloat16, "fold.w_cat", (Cb, Cn + Cb))
        s_ptr, ld_s = C.c_void_p(w_dg.data_ptr() + 2 * Cn), Cn + Cb
    else:
        _chk(S, torch.bfloat16, "fold.S", (Cb, Cb))
        s_ptr, ld_s = S, Cb
    _chk(D, torch.float32, "fold.D", (Cn, Cb)); _chk(w, torch.bfloat16, "fold.w", (Cn, Cb)); _chk(gram_totals, torch.float64, "fold.gram")
    _chk_stats(rev_stats, "fold.rev_stats", Cn); _chk(gamma, torch.float32, "fold.gamma", (Cn,))
    _chk(mean_invstd, torch.float32, "fold.mean_invstd", (2, Cn)); _chk(dgamma, torch.float32, "fold.dgamma", (Cn,)); _chk(dbeta, torch.float32, "fold.dbeta", (Cn,))
    _chk(dW, torch.float32, "fold.dW"); _chk(w_dg, torch.bfloat16, "fold.w_dg")
    _chk(c0, torch.float32, "fold.c0", (Cb,)); _chk(coef_ws, torch.float32, "fold.coef_ws")
    if gram_totals.numel() < Cb * Cb + Cb or dW.numel() < Cn * Cb or w_dg.shape[0] != Cb or w_dg.shape[1] < Cn or coef_ws.numel() < 2 * Cn:
        raise ValueError("conv3_bn_fold: operand sizes")
    launch("mhe_conv3_bn_fold", D, w, gram_totals, rev_stats, gamma, mean_invstd, float(count), dgamma, dbeta, dW, w_dg, int(w_dg.shape[1]), s_ptr, int(ld_s), c0,
           coef_ws, Cn, Cb)


def conv3x3_halo_supported(B, H, W, Cin, Cout):
    return bool(_lib.lib().mhe_conv3x3_halo_supported(int(B), int(H), int(W), int(Cin), int(Cout)))


def conv3x3_halo_pack(w):
    """standard bf16 pack [Cout][9 Cin] -> the fragment-major 16 KiB stages csrc/conv_halo.hip streams (same byte count)"""
    _chk(w, torch.bfloat16, "halo_pack.w")
    Cout, K = w.shape
    if K % 9 or (K // 9) % 64 or Cout % 128:
        raise ValueError(f"conv3x3_halo_pack: weight rows [{Cout}][{K}] are not 9 x (a multiple of 64) wide / a multiple of 128 many")
    out = torch.empty_like(w)
    launch("mhe_conv3x3_halo_pack_bf16", w, out, int(Cout), int(K // 9))
    return out


def conv3x3_halo(x, w_halo, in_scale=None, in_shift=None, relu_in=False, a_out=None, stats=None, residual=None, mask=None, bn=None):
    """3x3 / stride 1 / pad 1 with the input tile resident in LDS (mhe_conv3x3_halo_nhwc).  in_scale / in_shift: the producer's BatchNorm on
    the way in; a_out: that operand written once; mask (+ residual, bn = (raw output, mean_invstd, stats) of ONE consumer): data-gradient form."""
    B, H, W, Cin = x.shape
    Cout = w_halo.shape[0]
    _chk(x, torch.bfloat16, "halo.x"); _chk(w_halo, torch.bfloat16, "halo.w", (Cout, 9 * Cin))
    y = torch.empty(B, H, W, Cout, device=x.device, dtype=torch.bfloat16)
    for t, name, shape in ((in_scale, "in_scale", (Cin,)), (in_shift, "in_shift", (Cin,))):
        if t is not None:
            _chk(t, torch.float32, "halo." + name, shape)
    if stats is not None:
        _chk_stats(stats, "halo.stats", Cout)
    for t, name, shape in ((a_out, "a_out", tuple(x.shape)), (residual, "residual", tuple(y.shape)), (mask, "mask", tuple(y.shape))):
        if t is not None:
            _chk(t, torch.bfloat16, "halo." + name, shape)
    ext = _bn_consumers(None if bn is None else [bn], 1, torch.bfloat16, y.shape, Cout, "halo")
    with _Timed(lambda: ("mhe::conv::conv_halo_kernel<%d, %s>" % (W, "true" if mask is not None else "false"), 2.0 * B * H * W * Cout * 9 * Cin,
                         2 * (x.numel() + y.numel() + w_halo.numel()))):
        launch("mhe_conv3x3_halo_nhwc", B, H, W, Cin, Cout, x, w_halo, y, in_scale, in_shift, int(bool(relu_in)), a_out, stats, residual, mask, *ext)
    return y


def conv3x3_halo_dgrad_bn(g, y_raw, coef, w_halo, mask, gy_out=None, residual=None, bn=None):
    """data gradient of a 3x3 / stride-1 unit with the BatchNorm reverse of its own output gradient on the operand load: operand = k2 g + k1 y_raw
    + k0 (coef [3, C] of bn_backward(coef_only=True)), written to gy_out for the weight gradient (mhe_conv3x3_halo_dgrad_bn_nhwc)"""
    B, H, W, Cin = g.shape
    Cout = w_halo.shape[0]
    _chk(g, torch.bfloat16, "halo_dg.g"); _chk(y_raw, torch.bfloat16, "halo_dg.y", tuple(g.shape)); _chk(coef, torch.float32, "halo_dg.coef", (3, Cin))
    _chk(w_halo, torch.bfloat16, "halo_dg.w", (Cout, 9 * Cin)); _chk(mask, torch.bfloat16, "halo_dg.mask", (B, H, W, Cout))
    gx = torch.empty(B, H, W, Cout, device=g.device, dtype=torch.bfloat16)
    if gy_out is not None:
        _chk(gy_out, torch.bfloat16, "halo_dg.gy_out", tuple(g.shape))
    if residual is not None:
        _chk(residual, torch.bfloat16, "halo_dg.residual", tuple(gx.shape))
    ext = _bn_consumers(None if bn is None else [bn], 1, torch.bfloat16, gx.shape, Cout, "halo_dg")
    launch("mhe_conv3x3_halo_dgrad_bn_nhwc", B, H, W, Cin, Cout, g, y_raw, coef, w_halo, gx, gy_out, residual, mask, *ext)
    return gx


def bottleneck_tail_supported(B, H, W, Cb, Cout):
    d = ConvDesc(B, H, W, 4 * Cb, Cout, 1, 1, 1, 0, BF16, 1, 0, 0, 0)
    return bool(_lib.lib().mhe_bottleneck_tail_supported(C.byref(d), int(Cb)))


def bottleneck_tail(y2, bn2, w3, bn3, identity, id_aff, w1, stats=None, want_bits=False, quarter=False, a_out=None):
    """(a, y1) of mhe_bottleneck_tail_nhwc: a = relu(bn3(conv3(relu(bn2(y2)))) + identity) with conv3 re-evaluated in place of being read
    back, y1 = the next block's conv1 of a (+ its batch statistics).  bn2 / bn3 / id_aff = (scale, shift) pairs (id_aff may be None).
    quarter: a is the compact [B, ceil(H/2), ceil(W/2), C] tensor a[:, ::2, ::2] (mhe_bottleneck_tail_quarter_nhwc); a_out: where a goes."""
    B, H, W, Cb = y2.shape
    Cw, Cout = w3.shape[0], w1.shape[0]
    _chk(y2, torch.bfloat16, "tail.y2"); _chk(w3, torch.bfloat16, "tail.w3", (Cw, Cb)); _chk(w1, torch.bfloat16, "tail.w1", (Cout, Cw))
    _chk(identity, torch.bfloat16, "tail.identity", (B, H, W, Cw))
    for (sc, sh), n, c in ((bn2, "bn2", Cb), (bn3, "bn3", Cw)) + (((id_aff, "id", Cw),) if id_aff is not None else ()):
        _chk(sc, torch.float32, f"tail.{n}_scale", (c,)); _chk(sh, torch.float32, f"tail.{n}_shift", (c,))
    if stats is not None:
        _chk_stats(stats, "tail.stats", Cout)
    a_shape = (B, (H + 1) // 2, (W + 1) // 2, Cw) if quarter else (B, H, W, Cw)
    if quarter and want_bits:
        raise _lib.MheError("tail: the compact block output has no gate bits (forward-only path)")
    a = a_out if a_out is not None else torch.empty(a_shape, device=y2.device, dtype=torch.bfloat16)
    _chk(a, torch.bfloat16, "tail.a_out", a_shape)
    y1 = torch.empty(B, H, W, Cout, device=y2.device, dtype=torch.bfloat16)
    # want_bits: also [a > 0] as bits, byte [pixel][channel / 8] - the gate the reverse pass reads instead of `a` (conv2d_nhwc mask_bits=)
    bits = torch.empty(B, H, W, Cw // 8, device=y2.device, dtype=torch.uint8) if want_bits else None
    d = ConvDesc(B, H, W, Cw, Cout, 1, 1, 1, 0, BF16, 1, 0, 0, 0)
    ida = id_aff if id_aff is not None else (None, None)
    with _Timed(lambda: ("mhe::conv::bottleneck_tail%s_kernel<%d, %d>" % ("_quarter" if quarter else "", Cb, Cout), 2.0 * B * H * W * Cw * (Cb + Cout),
                         2 * (y2.numel() + identity.numel() + a.numel() + y1.numel() + w3.numel() + w1.numel()))):
        if quarter:
            launch("mhe_bottleneck_tail_quarter_nhwc", C.byref(d), Cb, y2, bn2[0], bn2[1], w3, bn3[0], bn3[1], identity, *ida, w1, a, y1, stats)
        else:
            launch("mhe_bottleneck_tail_bits_nhwc", C.byref(d), Cb, y2, bn2[0], bn2[1], w3, bn3[0], bn3[1], identity, *ida, w1, a, bits, y1, stats)
    return (a, y1, bits) if want_bits else (a, y1)


def linear_bf16_f32out(x, w, bias=None, out=None):
    """out[R,N] (f32) = x[R,K] (bf16) w[N,K]^T (bf16) + bias, f32 accumulation (mhe_conv2d_f32out_nhwc); K % 64 == 0, N % 4 == 0"""
    R, K = x.shape
    N = w.shape[0]
    _chk(x, torch.bfloat16, "linear_bf16.x"); _chk(w, torch.bfloat16, "linear_bf16.w", (N, K))
    if bias is not None:
        _chk(bias, torch.float32, "linear_bf16.bias", (N,))
    y = out if out is not None else torch.empty(R, N, device=x.device, dtype=torch.float32)
    _chk(y, torch.float32, "linear_bf16.out", (R, N))
    d = ConvDesc(R, 1, 1, K, N, 1, 1, 1, 0, BF16, 0, 0, 0)
    launch("mhe_conv2d_f32out_nhwc", C.byref(d), x, w, y, bias)
    return y


def conv3x3s2_dgrad(gy, w4, residual=None, mask=None, bn=None, tile=0):
    """dx [B,2Ho,2Wo,Cin] of a 3x3 / stride-2 / pad-1 convolution from gy [B,Ho,Wo,Cout] by the four parity classes
    (mhe_conv3x3s2_dgrad_nhwc); w4 = the four packed tap subsets (train.dgrad_s2_operand_indices)."""
    B, Ho, Wo, Cout = gy.shape
    dt = gy.dtype
    Cin = w4[0].shape[0]
    _chk(gy, dt, "dgrad_s2.gy")
    for i, w in enumerate(w4):
        _chk(w, dt, f"dgrad_s2.w{i}")
    dx = torch.empty(B, 2 * Ho, 2 * Wo, Cin, device=gy.device, dtype=dt)
    for t, name in ((residual, "residual"), (mask, "mask")):
        if t is not None:
            _chk(t, dt, "dgrad_s2." + name, dx.shape)
    ext = _bn_consumers(bn, 2, dt, dx.shape, Cin, "dgrad_s2")
    wp = (C.c_void_p * 4)(*[w.data_ptr() for w in w4])
    launch("mhe_conv3x3s2_dgrad_nhwc", B, Ho, Wo, Cout, Cin, dtype_code(dt), gy, wp, dx, residual, mask, *ext, int(tile))
    return dx


def conv1x1_residual_in(x, x2, w, in_scale, in_shift, x2_scale=None, x2_shift=None, a_out=None, stats=None, tile=0, quarter=False):
    """y = conv1x1(relu(x*in_scale+in_shift + (x2*x2_scale+x2_shift | x2))); optionally writes that operand to a_out.
    quarter: a_out is the compact [B, ceil(H/2), ceil(W/2), Cin] tensor and receives operand[:, ::2, ::2] only
    (mhe_conv1x1_residual_in_quarter_nhwc: the residual-tail kernel, conv_tile_choice(..., mode=2) == 10, or an error)."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    dt = x.dtype
    _chk(x, dt, "conv_res.x"); _chk(x2, dt, "conv_res.x2", x.shape); _chk(w, dt, "conv_res.w")
    _chk(in_scale, torch.float32, "conv_res.in_scale", (Cin,)); _chk(in_shift, torch.float32, "conv_res.in_shift", (Cin,))
    if x2_scale is not None:
        _chk(x2_scale, torch.float32, "conv_res.x2_scale", (Cin,)); _chk(x2_shift, torch.float32, "conv_res.x2_shift", (Cin,))
    if quarter and (a_out is None or tile):
        raise _lib.MheError("conv_res: quarter needs a_out and the launcher's own kernel choice")
    if a_out is not None:
        _chk(a_out, dt, "conv_res.a_out", (B, (H + 1) // 2, (W + 1) // 2, Cin) if quarter else x.shape)
    if stats is not None:
        _chk_stats(stats, "conv_res.stats", Cout)
    y = torch.empty(B, H, W, Cout, device=x.device, dtype=dt)
    d = ConvDesc(B, H, W, Cin, Cout, 1, 1, 1, 0, dtype_code(dt), 1, 0, int(tile))
    with _Timed(lambda: ("mhe::conv::conv_tail_quarter_kernel" if quarter else _conv_kernel_name(d, dt, 2), 2.0 * B * H * W * Cout * Cin,
                         x.element_size() * (2 * x.numel() + y.numel() + w.numel() + (a_out.numel() if a_out is not None else 0)))):
        launch("mhe_conv1x1_residual_in_quarter_nhwc" if quarter else "mhe_conv1x1_residual_in_nhwc", C.byref(d), x, x2, w, y, in_scale, in_shift, x2_scale,
               x2_shift, a_out, stats)
    return y


def conv1x1_dgrad_bn_apply(g, y_raw, coef, w_dg, a_out, mask, bn=None, zeros=None, tile=0):
    """data gradient of a 1x1 convolution whose output gradient is still to receive its BatchNorm reverse: the operand
    gy = k2 g + k1 y_raw + k0 (coef = [k2, k1, k0] of mhe_bn_bwd_finalize) is formed in the operand load and written once to a_out;
    the result is gated by mask and (optionally) feeds the BatchNorm-reverse sums of one consumer (mhe_conv1x1_residual_in_masked_nhwc)."""
    B, H, W, Cin = g.shape
    Cout = w_dg.shape[0]
    dt = g.dtype
    _chk(g, dt, "dgrad_apply.g"); _chk(y_raw, dt, "dgrad_apply.y", g.shape); _chk(w_dg, dt, "dgrad_apply.w"); _chk(a_out, dt, "dgrad_apply.a_out", g.shape)
    _chk(coef, torch.float32, "dgrad_apply.coef", (3, Cin)); _chk(mask, dt, "dgrad_apply.mask", (B, H, W, Cout))
    if zeros is None:
        zeros = torch.zeros(Cin, device=g.device, dtype=torch.float32)
    _chk(zeros, torch.float32, "dgrad_apply.zeros", (Cin,))
    out = torch.empty(B, H, W, Cout, device=g.device, dtype=dt)
    ext = _bn_consumers(bn, 1, dt, out.shape, Cout, "dgrad_apply")
    d = ConvDesc(B, H, W, Cin, Cout, 1, 1, 1, 0, dtype_code(dt), 0, 0, int(tile))
    launch("mhe_conv1x1_residual_in_masked_nhwc", C.byref(d), g, y_raw, w_dg, out, coef[0], coef[2], coef[1], zeros, a_out, None, mask, *ext)
    return out


def stem_conv7x7s2(x, w, dtype, stats=None):
    """x [B,3,H,W] f32 NCHW, w packed [64, Kpad] (dtype) -> raw conv1 output [B,Ho,Wo,64] NHWC (dtype)."""
    B, Cn, H, W = x.shape
    _chk(x, torch.float32, "stem.x"); _chk(w, dtype, "stem.w", (64, 192))
    if Cn != 3:
        raise _lib.MheError("stem.x: expected 3 input channels")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, 64, device=x.device, dtype=dtype)
    if stats is not None:
        _chk_stats(stats, "stem.stats", 64)
    with _Timed(lambda: ("mhe::conv::stem_kernel<%s>" % ("float" if dtype == torch.float32 else "unsigned short"), 2.0 * B * Ho * Wo * 64 * 147,
                         4 * x.numel() + y.element_size() * y.numel())):
        launch("mhe_stem_conv7x7s2", x, w, y, stats, B, H, W, dtype_code(dtype))
    return y


def stem_pool_supported(B, H, W, dtype):
    return bool(_lib.lib().mhe_stem_pool_supported(B, H, W, dtype_code(dtype)))


def stem_conv7x7s2_pool(x, w, bn_gamma, stats=None):
    """x [B,3,256,256] f32 NCHW -> pooled [B,64,64,64] bf16: per channel the 3x3 / stride-2 window max (gamma >= 0) or min (gamma < 0) of the raw
    conv1 output; relu(scale * pooled + shift) = maxpool(relu(bn1(conv1(x)))) (mhe_stem_conv7x7s2_pool).  stats: conv1's batch statistics."""
    B, Cn, H, W = x.shape
    _chk(x, torch.float32, "stem_pool.x"); _chk(w, torch.bfloat16, "stem_pool.w", (64, 192)); _chk(bn_gamma, torch.float32, "stem_pool.gamma", (64,))
    if Cn != 3:
        raise _lib.MheError("stem_pool.x: expected 3 input channels")
    if stats is not None:
        _chk_stats(stats, "stem_pool.stats", 64)
    y = torch.empty(B, 64, 64, 64, device=x.device, dtype=torch.bfloat16)
    with _Timed(lambda: ("mhe::conv::stem_pool_kernel", 2.0 * B * 128 * 128 * 64 * 147, 4 * x.numel() + 2 * y.numel())):
        launch("mhe_stem_conv7x7s2_pool", x, w, bn_gamma, y, stats, B, H, W)
    return y


def bn_finalize(stats, gamma, beta, running_mean, running_var, count, momentum=0.1, eps=1e-5, want_mean_invstd=False, clear=False,
                num_batches_tracked=None):
    """clear: the accumulators are zeroed once read (self-cleaning arena); num_batches_tracked (int64 scalar on the device): += 1"""
    Cn = gamma.shape[0]
    _chk_stats(stats, "bn_finalize.stats", Cn)
    scale = torch.empty(Cn, device=gamma.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    mi = torch.empty(2, Cn, device=gamma.device, dtype=torch.float32) if want_mean_invstd else None
    if clear or num_batches_tracked is not None:
        if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or not num_batches_tracked.is_cuda):
            raise _lib.MheError("bn_finalize.num_batches_tracked: int64 device tensor expected")
        launch("mhe_bn_finalize_step", stats, gamma, beta, running_mean, running_var, scale, shift, mi, Cn, float(count), float(momentum), float(eps), int(clear),
               num_batches_tracked)
    else:
        launch("mhe_bn_finalize", stats, gamma, beta, running_mean, running_var, scale, shift, mi, Cn, float(count), float(momentum), float(eps))
    return (scale, shift, mi) if want_mean_invstd else (scale, shift)


def bn_finalize_pair(unit0, unit1, momentum=0.1, eps=1e-5, clear=True):
    """two independent BatchNorm units finalized in ONE launch (mhe_bn_finalize_pair_step), each bit for bit as bn_finalize(clear=...) would.
    unit = (stats, gamma, beta, running_mean, running_var, count, num_batches_tracked | None) -> ((scale0, shift0), (scale1, shift1))"""
    args, outs = [], []
    for k, (stats, gamma, beta, rmean, rvar, count, nbt) in enumerate((unit0, unit1)):
        Cn = gamma.shape[0]
        _chk_stats(stats, f"bn_finalize_pair.stats{k}", Cn)
        if nbt is not None and (nbt.dtype != torch.int64 or not nbt.is_cuda):
            raise _lib.MheError("bn_finalize_pair.num_batches_tracked: int64 device tensor expected")
        scale = torch.empty(Cn, device=gamma.device, dtype=torch.float32)
        shift = torch.empty_like(scale)
        outs.append((scale, shift))
        args += [stats, gamma, beta, rmean, rvar, scale, shift, None, Cn, float(count), nbt]
    launch("mhe_bn_finalize_pair_step", *args, float(momentum), float(eps), int(clear))
    return outs[0], outs[1]


def bn_act(x, scale, shift, res=None, res_scale=None, res_shift=None, relu=True, out=None):
    Cn = x.shape[-1]
    P = x.numel() // Cn
    y = out if out is not None else torch.empty_like(x)
    with _Timed(lambda: ("mhe::conv::bn_act_kernel<%s>" % ("float" if x.dtype == torch.float32 else "unsigned short"), 0.0,
                         x.element_size() * x.numel() * (2 + (res is not None)))):
        launch("mhe_bn_act_nhwc", x, scale, shift, res, res_scale, res_shift, y, P, Cn, int(relu), dtype_code(x.dtype))
    return y


def maxpool3x3s2(x, scale=None, shift=None):
    B, H, W, Cn = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, Cn, device=x.device, dtype=x.dtype)
    launch("mhe_maxpool3x3s2_nhwc", x, scale, shift, y, B, H, W, Cn, dtype_code(x.dtype))
    return y


def avgpool(x):
    B, H, W, Cn = x.shape
    y = torch.empty(B, Cn, device=x.device, dtype=torch.float32)
    launch("mhe_avgpool_nhwc", x, y, B, H * W, Cn, dtype_code(x.dtype))
    return y


def bn_act_avgpool(x, scale, shift, res=None, rscale=None, rshift=None, relu=True):
    """avgpool(bn_act(x, scale, shift, res, rscale, rshift, relu)) in one pass (mhe_bn_act_avgpool_nhwc): the same bits, no block-wide store"""
    B, H, W, Cn = x.shape
    _chk(x, x.dtype, "bn_act_avgpool.x"); _chk(scale, torch.float32, "bn_act_avgpool.scale", (Cn,)); _chk(shift, torch.float32, "bn_act_avgpool.shift", (Cn,))
    if res is not None:
        _chk(res, x.dtype, "bn_act_avgpool.res", x.shape)
    if rscale is not None:
        _chk(rscale, torch.float32, "bn_act_avgpool.rscale", (Cn,)); _chk(rshift, torch.float32, "bn_act_avgpool.rshift", (Cn,))
    y = torch.empty(B, Cn, device=x.device, dtype=torch.float32)
    launch("mhe_bn_act_avgpool_nhwc", x, scale, shift, res, rscale, rshift, y, B, H * W, Cn, int(relu), dtype_code(x.dtype))
    return y


def nchw_to_nhwc(x, dtype=torch.float32, cpad=None):
    """NCHW f32 -> NHWC `dtype`, channels zero-padded to a 16-byte chunk (or to cpad: mhe_nchw_to_nhwc_pad)"""
    B, Cn, H, W = x.shape
    _chk(x, torch.float32, "nchw_to_nhwc.x")
    ce = 4 if dtype == torch.float32 else 8
    Cp = (Cn + ce - 1) // ce * ce if cpad is None else int(cpad)
    y = torch.empty(B, H, W, Cp, device=x.device, dtype=dtype)
    if cpad is None:
        launch("mhe_nchw_to_nhwc", x, y, B, Cn, H, W, dtype_code(dtype))
    else:
        launch("mhe_nchw_to_nhwc_pad", x, y, B, Cn, Cp, H, W, dtype_code(dtype))
    return y


# ---- train-step (reverse) kernels ---------------------------------------------------------------------
_wgrad_ws = _grow_only_workspace()      # the partial slabs of the pixel-range split, grown to the largest layer
WGRAD_SLABS = True      # False: f32 atomics into dw (the form without a workspace)


_WG_WAVES = {(256, 256): "4, 4" if os.environ.get("MHE_WGRAD_W16", "1") != "0" else "4, 2", (128, 128): "2, 2", (64, 128): "1, 4", (128, 64): "4, 1",
             (64, 64): "2, 2"}


def _wgrad_kernel_name(d, Ho=0, Wo=0, nbatch=1):
    """the weight-gradient instantiation the launcher will pick, spelled as rocprofv3 prints it"""
    v = _lib.lib().mhe_conv_wgrad_variant(C.byref(d), Ho, Wo, nbatch)
    kind, bm, bn = v // 1000000, (v % 1000000) // 1000, v % 1000
    if kind == 1:
        return "mhe::wgrad::wgrad_dma_kernel<%d, %d, %s>" % (bm, bn, _WG_WAVES.get((bm, bn), "?"))
    if kind == 2:
        return "mhe::wgrad::wgrad_bf16_kernel<%d, %d, %s>" % (bm, bn, _WG_WAVES.get((bm, bn), "?"))
    return "mhe::wgrad::wgrad_kernel<%s, %d, %d>" % ("float" if d.dtype == F32 else "unsigned short", bm, bn)


def _dg_timed(d, x, y, w, residual, mask, mask_bits, bn_ys, tag, xcat=None):
    """tools/train_lines.py: a data-gradient launch under a descriptive name with the bytes it has to move (operand, result, weights,
    residual, the gate - as bits where the kernel reads bits - and the raw tensors of the BatchNorm-reverse sums that are not the gate)"""
    if not (TIMING and TIMING_DG):
        return _Timed(None)
    es = x.element_size()
    nb = es * (x.numel() + y.numel() + w.numel() + (residual.numel() if residual is not None else 0) + (xcat.numel() if xcat is not None else 0))
    nb += mask_bits.numel() if mask_bits is not None else es * mask.numel()
    nb += sum(es * b.numel() for b in bn_ys if b is not None and b.data_ptr() != mask.data_ptr())
    name = "dgrad %dx%d s%d %d->%d @%dx%d%s%s bn%d %s" % (d.KH, d.KW, d.stride, d.Cin, d.Cout, y.shape[1], y.shape[2], " +res" if residual is not None else "",
                                                      " half" if d.res_half else "", sum(b is not None for b in bn_ys), tag)
    flops = 2.0 * y.shape[0] * y.shape[1] * y.shape[2] * d.Cout * d.KH * d.KW * (d.Cin + (xcat.shape[-1] if xcat is not None else 0))
    return _Timed(lambda: (name, flops, nb))


def conv_wgrad(x, gy, KH, KW, stride, pad, dw, ldw=0):
    """dw[Cout, KH*KW*Cin] (f32, pre-zeroed or accumulating) += gy^T (*) x ; x [B,H,W,Cin], gy [B,Ho,Wo,Cout]."""
    B, H, W, Cin = x.shape
    Cout = gy.shape[-1]
    dt = x.dtype
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    _chk(x, dt, "wgrad.x"); _chk(gy, dt, "wgrad.gy", (B, Ho, Wo, Cout)); _chk(dw, torch.float32, "wgrad.dw")
    if dw.numel() < (Cout - 1) * (ldw or KH * KW * Cin) + KH * KW * Cin:
        raise ValueError(f"wgrad.dw: {dw.numel()} floats cannot hold [{Cout}, {KH * KW * Cin}] at pitch {ldw or KH * KW * Cin}")
    d = ConvDesc(B, H, W, Cin, Cout, KH, KW, stride, pad, dtype_code(dt), 0, 0)
    L = _lib.lib()
    need = L.mhe_conv_wgrad_workspace_floats(C.byref(d)) if WGRAD_SLABS else 0
    # (timed: the kernel + its slab reducer; algorithmic bytes: both operands once + the gradient)
    with _Timed(lambda: (_wgrad_kernel_name(d), 2.0 * B * Ho * Wo * Cout * KH * KW * Cin, x.element_size() * (x.numel() + gy.numel()) + 4 * Cout * KH * KW * Cin)):
        if need:
            ws = _wgrad_ws(x.device, need)
            launch("mhe_conv_wgrad_ws_nhwc", C.byref(d), x, gy, dw, int(ldw), ws, ws.numel())
        else:
            launch("mhe_conv_wgrad_nhwc", C.byref(d), x, gy, dw, int(ldw))
    return dw


def conv_wgrad_multi(items):
    """several independent weight gradients in one call (mhe_conv_wgrad_multi_nhwc): items = [(x, gy, KH, KW, stride, pad, dw), ...] as for
    conv_wgrad.  Problems of one tile shape share launches: the chip is filled by the tiles of all of them, each pixel range is cut only as far
    as a common slice length asks (the partial-slab traffic of one launch per layer falls by the number of layers that share the chip).
    Fixed summation order; dW += as in conv_wgrad."""
    if not items:
        return
    if TIMING and len(items) > 1:
        # bench.py's live roofline pass: one call per tile class, so that every timed interval is ONE kernel instantiation (+ its reducer) under
        # the name rocprofv3 prints - the product path makes one call for the whole bucket
        groups = {}
        for it in items:
            x, gy, KH, KW, stride, pad, dw = it
            d = ConvDesc(x.shape[0], x.shape[1], x.shape[2], x.shape[3], gy.shape[-1], KH, KW, stride, pad, dtype_code(x.dtype), 0, 0)
            groups.setdefault(_lib.lib().mhe_conv_wgrad_variant(C.byref(d), 0, 0, 1), []).append(it)
        if len(groups) > 1:
            for g in groups.values():
                conv_wgrad_multi(g)
            return
    n = len(items)
    arr = (_lib.WgradItem * n)()
    flops = nbytes = 0.0
    for i, (x, gy, KH, KW, stride, pad, dw) in enumerate(items):
        B, H, W, Cin = x.shape
        Cout = gy.shape[-1]
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        _chk(x, x.dtype, "wgrad_multi.x"); _chk(gy, x.dtype, "wgrad_multi.gy", (B, Ho, Wo, Cout)); _chk(dw, torch.float32, "wgrad_multi.dw")
        if dw.numel() < Cout * KH * KW * Cin:
            raise ValueError(f"wgrad_multi.dw[{i}]: {dw.numel()} floats cannot hold [{Cout}, {KH * KW * Cin}]")
        arr[i].d = ConvDesc(B, H, W, Cin, Cout, KH, KW, stride, pad, dtype_code(x.dtype), 0, 0)
        arr[i].x, arr[i].gy, arr[i].dw, arr[i].ldw = x.data_ptr(), gy.data_ptr(), dw.data_ptr(), 0
        flops += 2.0 * B * Ho * Wo * Cout * KH * KW * Cin
        nbytes += x.element_size() * (x.numel() + gy.numel()) + 4 * Cout * KH * KW * Cin
    L = _lib.lib()
    need = L.mhe_conv_wgrad_multi_workspace_floats(C.byref(arr), n)
    ws = _wgrad_ws(items[0][0].device, need) if need else None
    def what():
        k = _wgrad_kernel_name(arr[0].d)
        return k.replace("wgrad_dma_kernel", "wgrad_dma_multi_kernel") if n > 1 else k, flops, nbytes
    with _Timed(what):
        launch("mhe_conv_wgrad_multi_nhwc", C.byref(arr), n, ws, ws.numel() if ws is not None else 0)


def conv_wgrad_batched(x, gy, dw, dw_batch_stride, nbatch, x_batch_stride=None, gy_batch_stride=None):
    """nbatch dense weight gradients dw_b [N, K] += gy_b [R, N]^T x_b [R, K] in one grouped launch (mhe_conv_wgrad_batched_nhwc).  x / gy: bf16
    tensors whose storage holds the problems at the given element strides (default: x [nbatch, R, K], gy [nbatch, R, N] contiguous); dw: the
    f32 view of the FIRST problem's gradient, the others lie dw_batch_stride floats apart (the train step's raw gradient arena)."""
    R, K = x.shape[-2], x.shape[-1]
    N = gy.shape[-1]
    if x.dtype != torch.bfloat16 or gy.dtype != torch.bfloat16 or not x.is_cuda or not gy.is_cuda or dw.dtype != torch.float32:
        raise _lib.MheError("conv_wgrad_batched: bf16 device operands and an f32 gradient expected")
    xs = R * K if x_batch_stride is None else int(x_batch_stride)
    gs = R * N if gy_batch_stride is None else int(gy_batch_stride)
    d = ConvDesc(R, 1, 1, K, N, 1, 1, 1, 0, BF16, 0, 0)
    L = _lib.lib()
    need = L.mhe_conv_wgrad_batched_workspace_floats(C.byref(d), nbatch) if WGRAD_SLABS else 0
    ws = _wgrad_ws(x.device, need) if need else None
    with _Timed(lambda: (_wgrad_kernel_name(d, 0, 0, nbatch), 2.0 * nbatch * R * N * K, nbatch * (2 * R * (K + N) + 4 * N * K))):
        launch("mhe_conv_wgrad_batched_nhwc", C.byref(d), nbatch, x, xs, gy, gs, dw, int(dw_batch_stride), 0, ws, ws.numel() if ws is not None else 0)
    return dw


def conv_wgrad_rect(x, gy, KH, KW, stride_h, stride_w, pad_h, pad_w, dw):
    """dw[Cout, KH*KW*Cin] += gy^T (*) x for a convolution with separate height / width stride and (top / left) padding whose output size is
    gy's (mhe_conv_wgrad_rect_nhwc): the stem's weight gradient over pixel pairs (train.TrainStep)."""
    B, H, W, Cin = x.shape
    Ho, Wo, Cout = gy.shape[1], gy.shape[2], gy.shape[3]
    dt = x.dtype
    _chk(x, dt, "wgrad_rect.x"); _chk(gy, dt, "wgrad_rect.gy", (B, Ho, Wo, Cout)); _chk(dw, torch.float32, "wgrad_rect.dw")
    if dw.numel() < Cout * KH * KW * Cin:
        raise ValueError(f"wgrad_rect.dw: {dw.numel()} floats cannot hold [{Cout}, {KH * KW * Cin}]")
    d = ConvDesc(B, H, W, Cin, Cout, KH, KW, stride_h, pad_h, dtype_code(dt), 0, 0)
    L = _lib.lib()
    need = L.mhe_conv_wgrad_rect_workspace_floats(C.byref(d), Ho, Wo) if WGRAD_SLABS else 0
    ws = None
    if need:
        ws = _wgrad_ws(x.device, need)
    with _Timed(lambda: (_wgrad_kernel_name(d, Ho, Wo), 2.0 * B * Ho * Wo * Cout * KH * KW * Cin,
                         x.element_size() * (x.numel() + gy.numel()) + 4 * Cout * KH * KW * Cin)):
        launch("mhe_conv_wgrad_rect_nhwc", C.byref(d), stride_w, pad_w, Ho, Wo, x, gy, dw, 0, ws, ws.numel() if ws is not None else 0)
    return dw


def linear_wgrad(x, gy, dw):
    """dw[N,K] += gy[R,N]^T x[R,K] (torch.nn.Linear weight layout), f32."""
    R, K = x.shape
    return conv_wgrad(x.view(R, 1, 1, K), gy.view(R, 1, 1, gy.shape[1]), 1, 1, 1, 0, dw)


_colsum_ws = _grow_only_workspace()


def colsum(rows, out, group_width=0, group_stride=0):
    """out[c] += sum_r rows[r][c], summed in a fixed order (mhe_colsum_ws_f32); with group_width g: column c is added to
    out[(c // g) * group_stride + c % g] (the l2 bias gradients of the flow's nets lie one raw-gradient slot apart)"""
    Cc = rows.shape[-1]
    R = rows.numel() // Cc
    _chk(rows, rows.dtype, "colsum.rows"); _chk(out, torch.float32, "colsum.out")
    if not group_width and out.numel() < Cc:          # (grouped: `out` is the first group's view into a larger arena)
        raise _lib.MheError(f"colsum.out: {out.numel()} floats cannot hold {Cc} columns")
    L = _lib.lib()
    need = L.mhe_colsum_workspace_floats(R, Cc)
    ws = _colsum_ws(rows.device, need) if need else None
    launch("mhe_colsum_ws_f32", rows, out, R, Cc, dtype_code(rows.dtype), int(group_width), int(group_stride), ws, ws.numel() if ws is not None else 0)
    return out


def gather(src, idx, dst, idx2=None):
    """dst[i] = src[idx[i]] (+ src[idx2[i]]), negative index = 0 ; src f32 flat, idx int32, dst f32 or bf16 of idx.numel() elements"""
    _chk(src, torch.float32, "gather.src"); _chk(idx, torch.int32, "gather.idx")
    if idx2 is not None:
        _chk(idx2, torch.int32, "gather.idx2", idx.shape)
    if dst.numel() != idx.numel() or dst.dtype not in (torch.float32, torch.bfloat16) or not dst.is_contiguous():
        raise ValueError("gather.dst: contiguous f32/bf16 tensor with idx.numel() elements expected")
    launch("mhe_gather_f32", src, idx, idx2, dst, idx.numel(), dtype_code(dst.dtype))
    return dst


def affine8(idx, with_bad=False):
    """host side of gather_affine8: int64 index vector (numel a multiple of 8, -1 = zero) -> (base_stride int32 [n/8, 2], mask uint8 [n/8]) if
    every group of eight is src[base + k * stride] on its valid positions, else None.  with_bad: always the pair plus a bool vector of the
    groups that are NOT affine (their entries are meaningless: the caller gathers those groups by index)"""
    I = idx.reshape(-1, 8).to(torch.int64)
    valid = I >= 0
    k = torch.arange(8, dtype=torch.int64)
    nv = valid.sum(1)
    first = torch.where(valid, k, torch.full_like(k, 8)).min(1).values.clamp(max=7)                 # first valid position
    second = torch.where(valid & (k > first[:, None]), k, torch.full_like(k, 8)).min(1).values      # next valid position (8: none)
    rows = torch.arange(I.shape[0])
    v0 = I[rows, first]
    has2 = second < 8
    v1 = I[rows, second.clamp(max=7)]
    num = v1 - v0
    den = (second - first).clamp(min=1)
    stride = torch.where(has2, torch.div(num, den, rounding_mode="floor"), torch.zeros_like(num))
    base = torch.where(nv > 0, v0 - first * stride, torch.zeros_like(v0))
    pred = base[:, None] + k[None, :] * stride[:, None]
    bad = ~(((pred == I) | ~valid).all(1)) | (stride.abs() >= 2 ** 31) | (base < -2 ** 31) | (base >= 2 ** 31)
    if not with_bad and bool(bad.any()):
        return None
    base, stride = torch.where(bad, torch.zeros_like(base), base), torch.where(bad, torch.zeros_like(stride), stride)
    mask = torch.where(bad, torch.zeros_like(nv), (valid.to(torch.int64) << k[None, :]).sum(1)).to(torch.uint8)
    enc = torch.stack([base, stride], 1).to(torch.int32).contiguous(), mask.contiguous()
    return enc + (bad,) if with_bad else enc


def gather_affine8(src, base_stride, mask, dst):
    """dst[8 g + k] = bf16(src[base_g + k stride_g]) where bit k of mask[g] is set, else 0 (mhe_gather_affine8_bf16)"""
    n8 = mask.numel()
    _chk(src, torch.float32, "gather.src"); _chk(base_stride, torch.int32, "gather.base_stride", (n8, 2)); _chk(mask, torch.uint8, "gather.mask", (n8,))
    if dst.numel() != 8 * n8 or dst.dtype != torch.bfloat16 or not dst.is_contiguous():
        raise ValueError("gather_affine8.dst: contiguous bf16 tensor of 8 x mask.numel() elements expected")
    launch("mhe_gather_affine8_bf16", src, base_stride, mask, dst, 8 * n8)
    return dst


def flow_mask_pad(x, mask_row, out):
    R, dim = x.shape
    _chk(x, torch.float32, "mask_pad.x"); _chk(mask_row, torch.float32, "mask_pad.mask", (dim,)); _chk(out, torch.float32, "mask_pad.out", (R, 64))
    launch("mhe_flow_mask_pad_f32", x, mask_row, out, R, dim)
    return out


def flow_mask_pad_mixed(x, mask_row, out_f32=None, out_bf16=None):
    R, dim = x.shape
    _chk(x, torch.float32, "mask_pad.x"); _chk(mask_row, torch.float32, "mask_pad.mask", (dim,))
    if out_f32 is not None:
        _chk(out_f32, torch.float32, "mask_pad.out", (R, 64))
    if out_bf16 is not None:
        _chk(out_bf16, torch.bfloat16, "mask_pad.out_bf16", (R, 64))
    launch("mhe_flow_mask_pad_mixed", x, mask_row, out_f32, out_bf16, R, dim)


def flow_lrelu_bwd_sum(g, h, N, B, sum_out, sum_stride, out_f32=None, out_bf16=None, slope=0.01, sum_out_t=None):
    """out = g * (h > 0 ? 1 : slope) (f32 and / or bf16) and sum_out[b] = sum over the image's N hypothesis rows; sum_out may be a
    column slice of a wider [B, sum_stride] matrix"""
    R, H = g.shape
    _chk(g, g.dtype, "lrelu_bwd_sum.g", (N * B, H)); _chk(h, h.dtype, "lrelu_bwd_sum.h", (R, H))
    if out_f32 is not None:
        _chk(out_f32, torch.float32, "lrelu_bwd_sum.out_f32", (R, H))
    if out_bf16 is not None:
        _chk(out_bf16, torch.bfloat16, "lrelu_bwd_sum.out_bf16", (R, H))
    launch("mhe_flow_lrelu_bwd_sum", g, dtype_code(g.dtype), h, dtype_code(h.dtype), out_f32, out_bf16, sum_out, int(sum_stride),
           0 if sum_out_t is None else sum_out_t, N, B, H, float(slope))


def flow_cond_lrelu(P, cond_slice, cond_stride, B):
    """P[r] = leaky_relu(P[r] + cond_slice[(r % B) * cond_stride : +H]) in place; cond_slice = view starting at the net/layer's column"""
    R, H = P.shape
    _chk(P, torch.float32, "cond_lrelu.P")
    launch("mhe_flow_cond_lrelu_f32", P, cond_slice, int(cond_stride), R, B, H)
    return P


def flow_lrelu_bwd(G, Hact, slope=0.01):
    _chk(G, torch.float32, "lrelu_bwd.G"); _chk(Hact, torch.float32, "lrelu_bwd.H", G.shape)
    launch("mhe_flow_lrelu_bwd_f32", G, Hact, G.numel(), float(slope))
    return G


def add(a, b, out=None):
    _chk(a, torch.float32, "add.a"); _chk(b, torch.float32, "add.b", a.shape)
    out = a if out is None else out
    launch("mhe_add_f32", a, b, out, a.numel())
    return out


def flow_couple_bwd(x_out, Os, Ot, mask_row, g_out, g_log_p, q_weight, B, x_in, GOs, GOt, g_part, GOs_bf16=None, GOt_bf16=None, db_s=None,
                    db_t=None):
    """db_s / db_t (optional, [64] f32): += the column sums of GOs / GOt (the l2 bias gradients of the s and t nets)"""
    R, dim = x_out.shape
    if GOs_bf16 is not None:
        _chk(GOs_bf16, torch.bfloat16, "couple_bwd.GOs_bf16", (R, 64)); _chk(GOt_bf16, torch.bfloat16, "couple_bwd.GOt_bf16", (R, 64))
    for t, n, s in ((x_out, "x_out", (R, dim)), (Os, "Os", (R, 64)), (Ot, "Ot", (R, 64)), (g_out, "g_out", (R, dim)),
                    (x_in, "x_in", (R, dim)), (GOs, "GOs", (R, 64)), (GOt, "GOt", (R, 64)), (g_part, "g_part", (R, dim))):
        _chk(t, torch.float32, "couple_bwd." + n, s)
    # the kernel's own column sums are f32 atomics from every 64-row workgroup: order-dependent beyond one workgroup - there the sums are
    # taken from the written GOs / GOt rows in a fixed order instead (two more launches on a fallback path)
    in_kernel = db_s is not None and R <= 64
    launch("mhe_flow_couple_bwd_mixed", x_out, Os, Ot, mask_row, g_out, g_log_p, float(q_weight), x_in, GOs, GOt, g_part, GOs_bf16, GOt_bf16,
           db_s if in_kernel else None, db_t if in_kernel else None, R, B, dim)
    if db_s is not None and not in_kernel:
        colsum(GOs, db_s); colsum(GOt, db_t)


def mfma_fragment_major(t):
    """[rows][K] (rows % 16 == 0, K % 32 == 0) -> the same elements in the order mhe_flow_reverse_chain_bf16 reads its operands:
    [rows / 16][K / 32][k-group 4][row 16][8] (lane = k-group * 16 + row of v_mfma_f32_16x16x32_bf16); works on index tensors too"""
    rows, K = t.shape
    return t.reshape(rows // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def flow_reverse_chain_supported(R, B, dim, hidden, ncoup):
    return bool(_lib.lib().mhe_flow_reverse_chain_supported(R, B, dim, hidden, ncoup))


def flow_sign_bits(h1, h2, B):
    """the signs of the kept activations h1, h2 (bf16 [nets, 64 B, 512], rows n B + b) in the layout mhe_flow_reverse_chain_bf16 reads and
    mhe_flow_couplings_frag_bf16 writes: int32 [nets, B, 2 layers, 8 waves, 64 lanes, 2] - lane (q, l15) of wave w holds bit
    (nt * 4 + mt) * 4 + e = [h[row mt * 16 + l15 of image b][unit 64 w + 16 nt + 4 q + e] > 0] (low word: nt < 2)"""
    nets = h1.shape[0]
    out = []
    for h in (h1, h2):
        t = (h.float() > 0).view(nets, 4, 16, B, 8, 4, 4, 4)                  # [net, mt, l15, b, w, nt, q, e]
        t = t.permute(0, 3, 4, 6, 2, 5, 1, 7).reshape(nets, B, 8, 64, 2, 32).to(torch.int64)      # [net, b, w, lane = q * 16 + l15, half, bit (nt % 2, mt, e)]
        wts = (1 << torch.arange(32, device=h.device, dtype=torch.int64))
        words = (t * wts).sum(-1)                                              # < 2^32
        out.append(torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32))
    return torch.stack(out, 2).contiguous()                                    # [net, b, layer, w, lane, 2]


_DB2_ROWS = {}


def flow_reverse_chain(x_out, g_x, g_logp, q_weight, mask, o_pre, sign_bits, w2F, w1F, w0F, w_net_stride, GOb, G2b, G1b, XPb, Gc, db2,
                       db_net_stride, z0):
    """the RealNVP reverse pass's data-gradient chain over all couplings in one launch (mhe_flow_reverse_chain_bf16; csrc/flow_rev.hip);
    sign_bits: flow_couplings_frag(..., sign_bits=) / flow_sign_bits"""
    R, dim = x_out.shape
    B = Gc.shape[0]
    nets, hidden = o_pre.shape[0], 512
    _chk(x_out, torch.float32, "rev_chain.x_out"); _chk(g_x, torch.float32, "rev_chain.g_x", (R, dim))
    _chk(mask, torch.float32, "rev_chain.mask", (nets // 2, dim)); _chk(o_pre, torch.float32, "rev_chain.o", (nets, R, 64))
    _chk(sign_bits, torch.int32, "rev_chain.sign_bits", (nets, B, 2, 8, 64, 2))
    _chk(GOb, torch.bfloat16, "rev_chain.GO", (nets, R, 64)); _chk(G2b, torch.bfloat16, "rev_chain.G2", (nets, R, hidden))
    _chk(G1b, torch.bfloat16, "rev_chain.G1", (nets, R, hidden)); _chk(XPb, torch.bfloat16, "rev_chain.XP", (nets // 2, R, 64))
    _chk(Gc, torch.float32, "rev_chain.Gc"); _chk(z0, torch.float32, "rev_chain.z0", (R, dim))
    if g_logp is not None:
        _chk(g_logp, torch.float32, "rev_chain.g_logp", (B,))
    rows = _DB2_ROWS.get((x_out.device, B, nets))
    if rows is None:
        rows = _DB2_ROWS[(x_out.device, B, nets)] = torch.empty(B, nets * 64, device=x_out.device, dtype=torch.float32)
    launch("mhe_flow_reverse_chain_bf16", x_out, g_x, g_logp, float(q_weight), mask, o_pre, sign_bits, w2F, w1F, w0F, int(w_net_stride), GOb, G2b, G1b, XPb, Gc,
           Gc.shape[1], rows, z0, R, B, dim, hidden, nets // 2)
    # db2 (+ net * db_net_stride) += the sum over images of the kernel's per-image rows, in a fixed order
    colsum(rows, db2, group_width=64, group_stride=db_net_stride)


def pack_transpose_bf16(src, out=None, outT=None, want_rows=True):
    """src [R][C] f32 -> (bf16 copy [R][C] | None, bf16 transpose [C][R]) in one launch (mhe_pack_transpose_bf16)"""
    R, Cc = src.shape
    _chk(src, torch.float32, "pack_transpose.src")
    if want_rows and out is None:
        out = torch.empty(R, Cc, device=src.device, dtype=torch.bfloat16)
    if outT is None:
        outT = torch.empty(Cc, R, device=src.device, dtype=torch.bfloat16)
    if out is not None:
        _chk(out, torch.bfloat16, "pack_transpose.out", (R, Cc))
    _chk(outT, torch.bfloat16, "pack_transpose.outT", (Cc, R))
    launch("mhe_pack_transpose_bf16", src, src.stride(0), out, outT, R, Cc)
    return out, outT


def flow_couple_accum(g_part, GXs, GXt, mask_row, g_in):
    R, dim = g_part.shape
    launch("mhe_flow_couple_accum_f32", g_part, GXs, GXt, mask_row, g_in, R, dim)
    return g_in


def bn_mean_invstd(stats, count, eps=1e-5):
    Cc = stats.shape[-1]
    _chk_stats(stats, "bn_mean_invstd.stats", Cc)
    mi = torch.empty(2, Cc, device=stats.device, dtype=torch.float32)
    launch("mhe_bn_mean_invstd", stats, mi, Cc, float(count), float(eps))
    return mi


def bn_backward(g, a, y, mean_invstd, gamma, stats, dgamma, dbeta, want_masked=False, out=None, reduced=False, coef_only=False):
    """train-mode BatchNorm(+ReLU) reverse: returns gy (and g [a>0] when want_masked); writes dgamma / dbeta.
    reduced=True: `stats` already holds the sums (accumulated by the epilogue of the kernel that produced g)."""
    Cc = y.shape[-1]
    P = y.numel() // Cc
    dt = y.dtype
    _chk(g, dt, "bn_bwd.g", y.shape); _chk(y, dt, "bn_bwd.y")
    if a is not None:
        _chk(a, dt, "bn_bwd.a", y.shape)
    _chk_stats(stats, "bn_bwd.stats", Cc); _chk(mean_invstd, torch.float32, "bn_bwd.mean_invstd", (2, Cc))
    _chk(gamma, torch.float32, "bn_bwd.gamma", (Cc,)); _chk(dgamma, torch.float32, "bn_bwd.dgamma", (Cc,)); _chk(dbeta, torch.float32, "bn_bwd.dbeta", (Cc,))
    if not reduced:
        launch("mhe_bn_bwd_reduce_nhwc", g, a, y, mean_invstd, stats, P, Cc, dtype_code(dt))
    coef = torch.empty(3, Cc, device=y.device, dtype=torch.float32)
    launch("mhe_bn_bwd_finalize", stats, gamma, mean_invstd, dgamma, dbeta, coef, Cc, float(P))
    if coef_only:              # the consumer applies gy = k2 g + k1 y + k0 itself (conv1x1_dgrad_bn_apply)
        return coef
    gy = out if out is not None else torch.empty_like(y)
    gm = torch.empty_like(y) if want_masked else None
    with _Timed(lambda: ("mhe::tb::bn_bwd_apply_wide_kernel<%s, %d>" % ("float" if dt == torch.float32 else "unsigned short", 4 if y.numel() * y.element_size() <= (80 << 20) else 1),
                         0.0, y.element_size() * y.numel() * (3 + (a is not None) + (gm is not None)))):
        launch("mhe_bn_bwd_apply_nhwc", g, a, y, coef, gy, gm, P, Cc, dtype_code(dt))
    return (gy, gm) if want_masked else gy


def bn_bwd_coef(stats, gamma, mean_invstd, dgamma, dbeta, count):
    """finish a BatchNorm reverse whose sums are in `stats`: writes dgamma / dbeta, returns coef = k2 | k1 | k0 [3, C] of gy = k2 g + k1 y + k0"""
    Cc = gamma.shape[0]
    _chk_stats(stats, "bn_bwd.stats", Cc); _chk(mean_invstd, torch.float32, "bn_bwd.mean_invstd", (2, Cc))
    _chk(gamma, torch.float32, "bn_bwd.gamma", (Cc,)); _chk(dgamma, torch.float32, "bn_bwd.dgamma", (Cc,)); _chk(dbeta, torch.float32, "bn_bwd.dbeta", (Cc,))
    coef = torch.empty(3, Cc, device=stats.device, dtype=torch.float32)
    launch("mhe_bn_bwd_finalize", stats, gamma, mean_invstd, dgamma, dbeta, coef, Cc, float(count))
    return coef


def maxpool3x3s2_idx_win(x, scale, shift):
    """maxpool3x3s2_idx(x, scale, shift) that also returns the RAW input at every winner (mhe_maxpool3x3s2_idx_affine_win_nhwc): what
    pooled_bn_sums needs of the full-resolution tensor"""
    B, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, Cc, device=x.device, dtype=x.dtype)
    xwin = torch.empty_like(y)
    idx = torch.empty(B, Ho, Wo, Cc, device=x.device, dtype=torch.uint8)
    _chk(x, x.dtype, "maxpool_idx.x"); _chk(scale, torch.float32, "maxpool_idx.scale", (Cc,)); _chk(shift, torch.float32, "maxpool_idx.shift", (Cc,))
    launch("mhe_maxpool3x3s2_idx_affine_win_nhwc", x, scale, shift, y, idx, xwin, B, H, W, Cc, dtype_code(x.dtype))
    return y, idx, xwin


def pooled_bn_sums(g, pooled, xwin, mean_invstd, stats):
    """the stem's BatchNorm-reverse sums from the pooled tensors alone (mhe_pooled_bn_sums_nhwc): g = the gradient of the pooled output,
    pooled = maxpool(relu(bn(y))) (its gate), xwin = the raw y at the winners; adds sum g', sum g' xhat per channel to `stats`"""
    Cc = g.shape[-1]
    dt = g.dtype
    _chk(g, dt, "pooled_bn_sums.g"); _chk(pooled, dt, "pooled_bn_sums.pooled", g.shape); _chk(xwin, dt, "pooled_bn_sums.xwin", g.shape)
    _chk(mean_invstd, torch.float32, "pooled_bn_sums.mean_invstd", (2, Cc)); _chk_stats(stats, "pooled_bn_sums.stats", Cc)
    launch("mhe_pooled_bn_sums_nhwc", g, pooled, xwin, mean_invstd, stats, g.numel() // Cc, Cc, dtype_code(dt))
    return stats


def maxpool3x3s2_idx(x, scale=None, shift=None):
    """(pooled, winning taps) of a 3x3 / stride-2 / pad-1 max pool; with scale / shift: of relu(x * scale + shift), evaluated on the load
    (mhe_maxpool3x3s2_idx_affine_nhwc: the normalised activation is never materialised)"""
    B, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, Cc, device=x.device, dtype=x.dtype)
    idx = torch.empty(B, Ho, Wo, Cc, device=x.device, dtype=torch.uint8)
    _chk(x, x.dtype, "maxpool_idx.x")
    if scale is not None:
        _chk(scale, torch.float32, "maxpool_idx.scale", (Cc,)); _chk(shift, torch.float32, "maxpool_idx.shift", (Cc,))
        launch("mhe_maxpool3x3s2_idx_affine_nhwc", x, scale, shift, y, idx, B, H, W, Cc, dtype_code(x.dtype))
        return y, idx
    launch("mhe_maxpool3x3s2_idx_nhwc", x, y, idx, B, H, W, Cc, dtype_code(x.dtype))
    return y, idx


def maxpool3x3s2_bwd_bn(gy, idx, y, scale, shift, mean_invstd, stats, want_gx=True):
    """reverse of maxpool(relu(bn(y))) up to the BatchNorm's sums: returns gx = scatter(gy, idx) [relu(y * scale + shift) > 0] and adds
    sum gx, sum gx * xhat per channel to `stats` (then bn_backward(gx, None, y, ..., stats, reduced=True) finishes the BatchNorm reverse)"""
    B, Ho, Wo, Cc = gy.shape
    dt = gy.dtype
    _chk(gy, dt, "maxpool_bwd_bn.gy"); _chk(idx, torch.uint8, "maxpool_bwd_bn.idx", gy.shape)
    _chk(y, dt, "maxpool_bwd_bn.y")
    H, W = y.shape[1], y.shape[2]
    if y.shape[0] != B or y.shape[3] != Cc or ((H - 1) // 2 + 1, (W - 1) // 2 + 1) != (Ho, Wo):
        raise ValueError(f"maxpool_bwd_bn: y {tuple(y.shape)} does not pool to gy {tuple(gy.shape)}")
    _chk(scale, torch.float32, "maxpool_bwd_bn.scale", (Cc,)); _chk(shift, torch.float32, "maxpool_bwd_bn.shift", (Cc,))
    _chk(mean_invstd, torch.float32, "maxpool_bwd_bn.mean_invstd", (2, Cc)); _chk_stats(stats, "maxpool_bwd_bn.stats", Cc)
    gx = torch.empty_like(y) if want_gx else None
    launch("mhe_maxpool3x3s2_bwd_bn_nhwc", gy, idx, y, scale, shift, mean_invstd, stats, gx, B, H, W, Cc, dtype_code(dt))
    return gx


def maxpool3x3s2_bwd_bn_apply(gy, idx, y, scale, shift, mean_invstd, coef):
    """the BatchNorm reverse's result k2 gx + k1 y + k0 for gx = scatter(gy, idx) [relu(y * scale + shift) > 0], gx itself never stored
    (mhe_maxpool3x3s2_bwd_bn_apply_nhwc; coef from bn_backward(..., coef_only=True) on the sums of maxpool3x3s2_bwd_bn(want_gx=False))"""
    B, Ho, Wo, Cc = gy.shape
    dt = gy.dtype
    _chk(gy, dt, "maxpool_bwd_apply.gy"); _chk(idx, torch.uint8, "maxpool_bwd_apply.idx", gy.shape); _chk(y, dt, "maxpool_bwd_apply.y")
    H, W = y.shape[1], y.shape[2]
    _chk(scale, torch.float32, "maxpool_bwd_apply.scale", (Cc,)); _chk(shift, torch.float32, "maxpool_bwd_apply.shift", (Cc,))
    _chk(mean_invstd, torch.float32, "maxpool_bwd_apply.mean_invstd", (2, Cc)); _chk(coef, torch.float32, "maxpool_bwd_apply.coef", (3, Cc))
    out = torch.empty_like(y)
    launch("mhe_maxpool3x3s2_bwd_bn_apply_nhwc", gy, idx, y, scale, shift, mean_invstd, coef, out, B, H, W, Cc, dtype_code(dt))
    return out


def maxpool3x3s2_bwd(gy, idx, H, W):
    B, Ho, Wo, Cc = gy.shape
    _chk(gy, gy.dtype, "maxpool_bwd.gy"); _chk(idx, torch.uint8, "maxpool_bwd.idx", gy.shape)
    gx = torch.empty(B, H, W, Cc, device=gy.device, dtype=gy.dtype)
    launch("mhe_maxpool3x3s2_bwd_nhwc", gy, idx, gx, B, H, W, Cc, dtype_code(gy.dtype))
    return gx


def avgpool_bwd(g, HW, dtype, mask=None):
    """gx[b,p,c] = g[b,c] / HW, zeroed where mask[b,p,c] <= 0 (ReLU gate of the pooled tensor) when a mask is given"""
    B, Cc = g.shape
    _chk(g, torch.float32, "avgpool_bwd.g")
    gx = torch.empty(B, HW, Cc, device=g.device, dtype=dtype)
    if mask is not None:
        _chk(mask, dtype, "avgpool_bwd.mask")
        if mask.numel() != gx.numel():
            raise ValueError("avgpool_bwd.mask: wrong size")
    launch("mhe_avgpool_bwd_nhwc", g, mask, gx, B, HW, Cc, dtype_code(dtype))
    return gx


def upsample2(g, H, W, base=None):
    """out[b,2i,2j] = g[b,i,j] (+ base), zero (+ base) elsewhere; out [B,H,W,C]"""
    B, Ho, Wo, Cc = g.shape
    if (Ho, Wo) != ((H + 1) // 2, (W + 1) // 2):
        raise ValueError(f"upsample2: g {tuple(g.shape)} does not match output {H}x{W}")
    _chk(g, g.dtype, "upsample2.g")
    if base is not None:
        _chk(base, g.dtype, "upsample2.base", (B, H, W, Cc))
    out = torch.empty(B, H, W, Cc, device=g.device, dtype=g.dtype)
    launch("mhe_upsample2_nhwc", g, base, out, B, H, W, Cc, dtype_code(g.dtype))
    return out


_SQ_WS = {}


def sqnorm(g, out):
    """out[0] = |g|^2, summed in a fixed order (bitwise reproducible for equal inputs)"""
    _chk(g, torch.float32, "sqnorm.g"); _chk(out, torch.float32, "sqnorm.out", (1,))
    ws = _SQ_WS.get(g.device)
    if ws is None:
        ws = _SQ_WS[g.device] = torch.empty(_lib.lib().mhe_sqnorm_workspace_floats(), device=g.device, dtype=torch.float32)
    launch("mhe_sqnorm_f32", g, g.numel(), ws, out)
    return out


def train_tick(step, sq):
    _chk(step, torch.int32, "tick.step", (1,)); _chk(sq, torch.float32, "tick.sqnorm", (1,))
    launch("mhe_train_tick", step, sq)


def adam_step(p, g, m, v, sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, grad_scale=1.0):
    n = p.numel()
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, torch.float32, "adam." + nm, (n,))
    launch("mhe_adam_step_f32", p, g, m, v, n, sq, step, float(lr), float(beta1), float(beta2), float(eps), float(max_norm), float(grad_scale))


def flow_cond_lrelu_mixed(pre, cond_slice, cond_stride, B, out_f32=None, out_bf16=None):
    """leaky_relu(pre + cond[r % B]) from f32 or bf16 `pre` into f32 and / or bf16 outputs"""
    R, H = pre.shape
    _chk(pre, pre.dtype, "cond_lrelu_mixed.pre")
    if out_f32 is not None:
        _chk(out_f32, torch.float32, "cond_lrelu_mixed.out_f32", (R, H))
    if out_bf16 is not None:
        _chk(out_bf16, torch.bfloat16, "cond_lrelu_mixed.out_bf16", (R, H))
    launch("mhe_flow_cond_lrelu_mixed", pre, dtype_code(pre.dtype), cond_slice, int(cond_stride), out_f32, out_bf16, R, B, H)


def flow_lrelu_bwd_mixed(g, h, out_f32=None, out_bf16=None, slope=0.01):
    _chk(g, g.dtype, "lrelu_bwd_mixed.g"); _chk(h, h.dtype, "lrelu_bwd_mixed.h", g.shape)
    launch("mhe_flow_lrelu_bwd_mixed", g, dtype_code(g.dtype), h, dtype_code(h.dtype), out_f32, out_bf16, g.numel(), float(slope))


# ---- conditional Glow: the ActNorm + LU re-parameterisation on the device (csrc/glow_affine.hip) ---------------------------------------
def glow_affine(ptr_table, layers, features, eps, out=None):
    """ptr_table: int64 [layers, 6] device tensor of parameter addresses (log_scale, shift, lower, upper, unconstrained diag, bias).
    Returns / refreshes dict(A, Ainv, AinvT [L,64,64], c, cinv [L,64], const_parts [L], ws float64): mhe_glow_affine_f64"""
    dev = ptr_table.device
    if out is None:
        out = {k: torch.zeros(layers, 64, 64, device=dev) for k in ("A", "Ainv", "AinvT")}
        out.update({k: torch.zeros(layers, 64, device=dev) for k in ("c", "cinv")})
        out["const_parts"] = torch.zeros(layers, device=dev)
        out["ws"] = torch.zeros(int(_lib.lib().mhe_glow_affine_workspace_doubles(layers, features)), device=dev, dtype=torch.float64)
    launch("mhe_glow_affine_f64", ptr_table, layers, features, float(eps), out["A"], out["c"], out["Ainv"], out["AinvT"], out["cinv"], out["const_parts"], out["ws"])
    return out


def glow_reparam_bwd(g_ainv_ptrs, g_cinv_ptrs, g_logp, layers, features, ws, grad_ptrs, q_sign=-1.0):
    """gradients of every layer's six small tensors, written through grad_ptrs (int64 [layers, 6] addresses): mhe_glow_reparam_bwd_f64"""
    launch("mhe_glow_reparam_bwd_f64", g_ainv_ptrs, g_cinv_ptrs, g_logp, 0 if g_logp is None else g_logp.numel(), float(q_sign), layers, features, ws, grad_ptrs)


def glow_affine_wide(ptr_table, layers, features, eps, out=None):
    """glow_affine for a wide flow variable (2 <= features <= 256; the 144-D body pose): the same dict with [L, Dp, Dp] / [L, Dp] outputs,
    Dp = ceil64(features), and the float64 workspace the reverse reads: mhe_glow_affine_wide_f64"""
    dev, Dp = ptr_table.device, (features + 63) // 64 * 64
    if out is None:
        out = {k: torch.empty(layers, Dp, Dp, device=dev) for k in ("A", "Ainv", "AinvT")}
        out.update({k: torch.empty(layers, Dp, device=dev) for k in ("c", "cinv")})
        out["const_parts"] = torch.empty(layers, device=dev)
        out["ws"] = torch.empty(int(_lib.lib().mhe_glow_affine_wide_workspace_doubles(layers, features)), device=dev, dtype=torch.float64)
    launch("mhe_glow_affine_wide_f64", ptr_table, layers, features, float(eps), out["A"], out["c"], out["Ainv"], out["AinvT"], out["cinv"], out["const_parts"],
           out["ws"])
    return out


def glow_affine_wide_bwd(g_ainv, g_cinv, g_logq, layers, features, ws):
    """float64 gradients [layers, 4 D + D (D - 1)] of every layer's (log_scale, shift, lower, upper, unconstrained diag, bias) from dL/dA^-1
    [L, Dp, Dp], dL/dc^-1 [L, Dp] and dL/dlog q per row (or None): mhe_glow_affine_wide_bwd_f64"""
    Dp = (features + 63) // 64 * 64
    _chk(g_ainv, torch.float32, "affine_wide_bwd.g_ainv", (layers, Dp, Dp)); _chk(g_cinv, torch.float32, "affine_wide_bwd.g_cinv", (layers, Dp))
    if g_logq is not None:
        _chk(g_logq, torch.float32, "affine_wide_bwd.g_logq")
    L = _lib.lib()
    out = torch.empty(layers, int(L.mhe_glow_affine_wide_grad_doubles(layers, features)) // layers, device=g_ainv.device, dtype=torch.float64)
    launch("mhe_glow_affine_wide_bwd_f64", g_ainv, g_cinv, g_logq, 0 if g_logq is None else g_logq.numel(), layers, features, ws, out)
    return out


def glow_coupling_inv_bwd_wide(v, prm, g_y, g_logq, dim, first, n_transform):
    """reverse of the inverse coupling at the pitches of v [R, ld] and prm [R, ldp]: (g_v [R, ld], g_prm [R, ldp])"""
    R, ld = v.shape
    ldp = prm.shape[1]
    _chk(v, torch.float32, "coupling_bwd.v"); _chk(prm, torch.float32, "coupling_bwd.prm", (R, ldp)); _chk(g_y, torch.float32, "coupling_bwd.g_y", (R, ld))
    if g_logq is not None:
        _chk(g_logq, torch.float32, "coupling_bwd.g_logq", (R,))
    g_v, g_prm = torch.empty_like(v), torch.empty_like(prm)
    launch("mhe_glow_coupling_inv_bwd_wide_f32", v, prm, g_y, g_logq, g_v, g_prm, R, dim, first, n_transform, ld, ldp)
    return g_v, g_prm


def glow_coupling_fwd_bwd(v, prm, g_y, g_logp, dim, first, n_transform):
    """reverse of the forward coupling (the density direction) at the pitches of v [R, ld] and prm [R, ldp]: (g_v [R, ld], g_prm [R, ldp]);
    g_logp [R] = dL/dlog p per row or None: mhe_glow_coupling_fwd_bwd_f32"""
    R, ld = v.shape
    ldp = prm.shape[1]
    _chk(v, torch.float32, "coupling_fwd_bwd.v"); _chk(prm, torch.float32, "coupling_fwd_bwd.prm", (R, ldp)); _chk(g_y, torch.float32, "coupling_fwd_bwd.g_y", (R, ld))
    if g_logp is not None:
        _chk(g_logp, torch.float32, "coupling_fwd_bwd.g_logp", (R,))
    g_v, g_prm = torch.empty_like(v), torch.empty_like(prm)
    launch("mhe_glow_coupling_fwd_bwd_f32", v, prm, g_y, g_logp, g_v, g_prm, R, dim, first, n_transform, ld, ldp)
    return g_v, g_prm


def glow_base_density_bwd(z_padded, g_z, g_logp, dim):
    """g_y [R, ld] = g_z - g_logp[r] z on the padded rows z_padded [R, ld]; g_z [R, dim] or None, g_logp [R] or None: mhe_glow_base_density_bwd_f32"""
    R, ld = z_padded.shape
    _chk(z_padded, torch.float32, "base_density_bwd.z")
    if g_z is not None:
        _chk(g_z, torch.float32, "base_density_bwd.g_z", (R, dim))
    if g_logp is not None:
        _chk(g_logp, torch.float32, "base_density_bwd.g_logp", (R,))
    g_y = torch.empty_like(z_padded)
    launch("mhe_glow_base_density_bwd_f32", z_padded, g_z, g_logp, g_y, R, dim, ld)
    return g_y


def glow_affine_density_bwd(g_a, g_c, g_logp, layers, features, ws):
    """the density direction's reverse of the ActNorm + LU re-parameterisation: float64 gradients [layers, 4 D + D (D - 1)] of every layer's
    (log_scale, shift, lower, upper, unconstrained diag, bias) from dL/dA [L, Dp, Dp], dL/dc [L, Dp] and dL/dlog p per row (or None).  `ws`: the
    float64 workspace of glow_affine (features <= 64 with 64-pitch operands: mhe_glow_affine_density_bwd_f64) or of glow_affine_wide
    (mhe_glow_affine_wide_density_bwd_f64); which one is told by its size"""
    Dp = (features + 63) // 64 * 64
    _chk(g_a, torch.float32, "affine_density_bwd.g_a", (layers, Dp, Dp)); _chk(g_c, torch.float32, "affine_density_bwd.g_c", (layers, Dp))
    _chk(ws, torch.float64, "affine_density_bwd.ws")
    if g_logp is not None:
        _chk(g_logp, torch.float32, "affine_density_bwd.g_logp")
    L = _lib.lib()
    n = 0 if g_logp is None else g_logp.numel()
    out = torch.empty(layers, int(L.mhe_glow_affine_wide_grad_doubles(layers, features)) // layers, device=g_a.device, dtype=torch.float64)
    if features <= 64 and ws.numel() == L.mhe_glow_affine_workspace_doubles(layers, features):
        launch("mhe_glow_affine_density_bwd_f64", g_a, g_c, g_logp, n, layers, features, ws, out)
    elif ws.numel() == L.mhe_glow_affine_wide_workspace_doubles(layers, features):
        launch("mhe_glow_affine_wide_density_bwd_f64", g_a, g_c, g_logp, n, layers, features, ws, out)
    else:
        raise _lib.MheError(f"affine_density_bwd.ws: {ws.numel()} doubles is the workspace of neither glow_affine nor glow_affine_wide at "
                            f"{layers} layers x {features} features")
    return out


def sum_row_blocks(rows, groups, N, out=None, out_stride=0, accumulate=False):
    """out[g] (+)= sum_n rows[g*N + n] (per-image sums of batch-major rows); `out` may be a view into a wider [groups, out_stride] matrix"""
    Cc = rows.shape[1]
    _chk(rows, torch.float32, "sum_row_blocks.rows", (groups * N, Cc))
    if out is None:
        out = torch.empty(groups, Cc, device=rows.device, dtype=torch.float32)
    launch("mhe_sum_row_blocks_f32", rows, out, groups, N, Cc, int(out_stride or Cc), int(accumulate))
    return out


def glow_finish(z_padded, v_padded, logdet, R, dim, inverse, const_parts, want_out=True):
    """(out [R,dim] | None, log_prob [R]) with the log-determinant constant summed from the device-resident per-layer parts"""
    out = torch.empty(R, dim, device=z_padded.device) if want_out else None
    logp = torch.empty(R, device=z_padded.device)
    launch("mhe_glow_finish_dev_f32", z_padded, v_padded, logdet, out, logp, R, dim, -1.0 if inverse else 1.0, const_parts, const_parts.numel())
    return out, logp


# ---- conditional Glow: the sampling direction of all layers in one launch (csrc/glow_fwd.hip) -------------------------------------------
def dropout_bits(n, p, device, state=None):
    """keep bits of n elements (uint8 [n / 8], the format dropout_ writes / applies), drawn on the device: mhe_dropout_bits"""
    bits = torch.empty(n // 8, device=device, dtype=torch.uint8)
    st = state if state is not None else rng_state(device)
    launch("mhe_dropout_bits", bits, n, float(p), st)
    return bits


def glow_layers_supported(N, B, dim, hidden, layers, blocks):
    return bool(_lib.lib().mhe_glow_layers_supported(N, B, dim, hidden, layers, blocks))


def glow_fused_layout(wx, w0, w1, wf, bf, b0, b1, dim):
    """the weight operands of mhe_glow_layers_bf16 from per-layer stacks - wx [L, 512, 64] (initial layer on the padded variable), w0 / w1
    [L, 2, 512, 512], wf [L, >= 2 T, 512] / bf [L, >= 2 T] (final layer, rows [shift (T) | unconstrained scale (T)]), b0 / b1 [L, 2, 512] - as
    VALUES (float tensors: zero fill) or as INDEX tensors into a flat parameter buffer (integer tensors: -1 fill; the trainer's gather tables).
    The final layer's rows move to the flow variable's own columns: row c of wsF / wuF = the shift / scale row of transform column c."""
    L = wx.shape[0]
    idx = not wx.is_floating_point()
    fill = -1 if idx else 0
    ws, wu = (torch.full((L, 64, 512), fill, dtype=wf.dtype, device=wf.device) for _ in range(2))
    bs, bu = (torch.full((L, 64), fill, dtype=bf.dtype, device=bf.device) for _ in range(2))
    for l in range(L):
        first = 1 - (l & 1)
        T = dim // 2 if first else (dim + 1) // 2
        cols = torch.arange(first, dim, 2, device=wf.device)
        ws[l, cols], wu[l, cols] = wf[l, :T], wf[l, T:2 * T]
        bs[l, cols], bu[l, cols] = bf[l, :T], bf[l, T:2 * T]
    fr = mfma_fragment_major
    tr = lambda m: m.t().contiguous()
    rev = {"wsT": torch.stack([fr(tr(ws[l])) for l in range(L)]), "wuT": torch.stack([fr(tr(wu[l])) for l in range(L)]),
           "w0T": torch.stack([torch.stack([fr(tr(w0[l, b])) for b in range(2)]) for l in range(L)]),
           "w1T": torch.stack([torch.stack([fr(tr(w1[l, b])) for b in range(2)]) for l in range(L)]),
           "wxT": torch.stack([fr(tr(wx[l])) for l in range(L)])}                       # operands of the reverse chain (mhe_glow_reverse_chain_bf16)
    return {**rev, "wxF": torch.stack([fr(wx[l]) for l in range(L)]), "w0F": torch.stack([torch.stack([fr(w0[l, b]) for b in range(2)]) for l in range(L)]),
            "w1F": torch.stack([torch.stack([fr(w1[l, b]) for b in range(2)]) for l in range(L)]),
            "wsF": torch.stack([fr(ws[l]) for l in range(L)]), "wuF": torch.stack([fr(wu[l]) for l in range(L)]),
            "bs": bs, "bu": bu, "b0": b0.contiguous(), "b1": b1.contiguous()}


def glow_layers(noise, ctab, fp, aff, drop_bits, p_drop, N, B, dim, row_n, row_b, tape=None):
    """(sample [R, dim], log q [R]) of the conditional Glow's sampling direction, all layers in one launch (mhe_glow_layers_bf16).
    fp: glow_fused_layout's dict as bf16 (weights) / f32 (biases) device tensors; aff: glow_affine's dict; drop_bits: uint8 [L, 2, R * 64] | None;
    tape: dict(v, y, prm f32 [L, R, 64]; tb, t2, t3 bf16 [L, 2, R, 512]; hf bf16 [L, R, 512]) | None"""
    R = N * B
    _chk(noise, torch.float32, "glow_layers.noise", (R, dim)); _chk(ctab, torch.float32, "glow_layers.ctab")
    L = fp["wxF"].shape[0]
    for k, dt in (("wxF", torch.bfloat16), ("w0F", torch.bfloat16), ("w1F", torch.bfloat16), ("wsF", torch.bfloat16), ("wuF", torch.bfloat16),
                  ("b0", torch.float32), ("b1", torch.float32), ("bs", torch.float32), ("bu", torch.float32)):
        _chk(fp[k], dt, "glow_layers." + k)
    if fp["w0F"].numel() != L * 2 * 512 * 512 or fp["wxF"].numel() != L * 512 * 64 or fp["wsF"].numel() != L * 64 * 512:
        raise _lib.MheError("glow_layers: weight operands do not match hidden 512 / 2 blocks per layer")
    if drop_bits is not None:
        _chk(drop_bits, torch.uint8, "glow_layers.drop_bits")
        if drop_bits.numel() != L * 2 * R * 64:
            raise _lib.MheError(f"glow_layers.drop_bits: {L * 2 * R * 64} bytes expected, got {drop_bits.numel()}")
    out, logq = torch.empty(R, dim, device=noise.device), torch.empty(R, device=noise.device)
    t = tape or {}
    if tape is not None:
        for k, dt, shp in (("v", torch.float32, (L, R, 64)), ("y", torch.float32, (L, R, 64)), ("prm", torch.float32, (L, R, 64)),
                           ("tb", torch.bfloat16, (L, 2, R, 512)), ("t2", torch.bfloat16, (L, 2, R, 512)), ("t3", torch.bfloat16, (L, 2, R, 512)),
                           ("hf", torch.bfloat16, (L, R, 512))):
            _chk(tape[k], dt, "glow_layers.tape." + k, shp)
    launch("mhe_glow_layers_bf16", noise, ctab, ctab.shape[1], fp["wxF"], fp["w0F"], fp["w1F"], fp["wsF"], fp["wuF"], fp["b0"], fp["b1"], fp["bs"], fp["bu"],
           aff["AinvT"], aff["cinv"], aff["const_parts"], drop_bits, float(p_drop), out, logq, t.get("v"), t.get("y"), t.get("prm"), t.get("tb"), t.get("t2"),
           t.get("t3"), t.get("hf"), t.get("prmc"), t.get("vb"), t.get("bits"), N, B, dim, 512, L, 2, row_n, row_b)
    return out, logq


def glow_reverse_chain_supported(R, B, dim, hidden, layers, blocks):
    return bool(_lib.lib().mhe_glow_reverse_chain_supported(R, B, dim, hidden, layers, blocks))


def glow_reverse_chain(g_x, g_logp, q_weight, tape, ctab, fp, aff, p_drop, out, B, dim):
    """the data-gradient chain of the conditional Glow's sampling direction in one launch (mhe_glow_reverse_chain_bf16) over the tape of
    glow_layers (v, prmc, t3, bits).  out: dict(gv f32 [L,R,64]; gpc bf16 [L,R,128]; gt3, gt2 bf16 [L,2,R,512]; gh0 bf16 [L,R,512];
    gct f32 [B,cs]; bsum f32 [B, L*2*2*512]; bfsum f32 [B, L*128]) - all written"""
    R = g_x.shape[0]
    L = tape["v"].shape[0]
    _chk(g_x, torch.float32, "glow_reverse_chain.g_x", (R, dim))
    for k, dt, shp in (("v", torch.float32, (L, R, 64)), ("prmc", torch.float32, (L, R, 128)), ("t3", torch.bfloat16, (L, 2, R, 512))):
        _chk(tape[k], dt, "glow_reverse_chain.tape." + k, shp)
    _chk(tape["bits"], torch.int32, "glow_reverse_chain.tape.bits", (L, 2, 2, B, 512, 2))
    for k, dt, shp in (("gv", torch.float32, (L, R, 64)), ("gpc", torch.bfloat16, (L, R, 128)), ("gt3", torch.bfloat16, (L, 2, R, 512)),
                       ("gt2", torch.bfloat16, (L, 2, R, 512)), ("gh0", torch.bfloat16, (L, R, 512)), ("gct", torch.float32, (B, ctab.shape[1])),
                       ("bsum", torch.float32, (B, L * 2 * 2 * 512)), ("bfsum", torch.float32, (B, L * 128))):
        _chk(out[k], dt, "glow_reverse_chain.out." + k, shp)
    for k in ("wsT", "wuT", "w1T", "w0T", "wxT"):
        _chk(fp[k], torch.bfloat16, "glow_reverse_chain." + k)
    launch("mhe_glow_reverse_chain_bf16", g_x, g_logp, float(q_weight), tape["v"], tape["prmc"], tape["t3"], tape["bits"], ctab, ctab.shape[1], fp["wsT"], fp["wuT"],
           fp["w1T"], fp["w0T"], fp["wxT"], aff["Ainv"], float(p_drop), out["gv"], out["gpc"], out["gt3"], out["gt2"], out["gh0"], out["gct"], out["bsum"],
           out["bfsum"], R, B, dim, 512, L, 2)
    return out
