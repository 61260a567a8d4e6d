"""CPU: the host layer between the convolution / weight-gradient entry points of csrc/conv.hip, csrc/conv_halo.hip and csrc/wgrad.hip and their
launches.  The library loads without a device; every call here is refused before a launch (MHE_ERR_ARG, mhe_last_error() carrying the entry's
text) or is a pure query.  A call that got past its checks would come back as a launch error and fail its case.

The dispatch tables at the end are literal values read from the build before the request-struct refactor of this layer, with no MHE_*
switch set: the kernel variant per operand-load form over the trunk's layers, and the weight-gradient variant / workspace sizes."""
import ctypes as C

import pytest

from mhentropy_amd import _lib
from mhentropy_amd._lib import ConvDesc, WgradItem

MHE_ERR_ARG = 1
F32, BF16 = 0, 1
Z = None
_BUF = C.create_string_buffer(64)
P = C.cast(_BUF, C.c_void_p)                  # a non-null pointer for operands that a refused call never reads


def D(B=2, H=16, W=16, Cin=64, Cout=128, k=1, stride=1, pad=0, dtype=BF16, relu_in=0, relu_out=0, tile=0, res_half=0):
    return C.byref(ConvDesc(B, H, W, Cin, Cout, k, k, stride, pad, dtype, relu_in, relu_out, tile, res_half))


def _items(descs, ptr=P, ldw=0):
    arr = (WgradItem * len(descs))()
    for j, d in enumerate(descs):
        arr[j].d = ConvDesc(*d, 0, 0, 0, 0)
        arr[j].x = arr[j].gy = arr[j].dw = ptr
        arr[j].ldw = ldw
    return arr


def _refusals(L):
    """(entry, call, text that mhe_last_error() must contain): null required pointers, violated pairings, each entry's own geometry limits"""
    c2, f32o, rin, rinq, cat = L.mhe_conv2d_nhwc, L.mhe_conv2d_f32out_nhwc, L.mhe_conv1x1_residual_in_nhwc, L.mhe_conv1x1_residual_in_quarter_nhwc, L.mhe_conv1x1_cat_bias_nhwc
    rinm, msk, mbits, mbias, dg2 = (L.mhe_conv1x1_residual_in_masked_nhwc, L.mhe_conv2d_masked_nhwc, L.mhe_conv2d_masked_bits_nhwc, L.mhe_conv2d_masked_bias_nhwc,
                                    L.mhe_conv3x3s2_dgrad_nhwc)
    w4 = (C.c_void_p * 4)(P.value, P.value, P.value, P.value)
    w4hole = (C.c_void_p * 4)(P.value, P.value, None, P.value)
    tail, tbits, tq = L.mhe_bottleneck_tail_nhwc, L.mhe_bottleneck_tail_bits_nhwc, L.mhe_bottleneck_tail_quarter_nhwc
    T = D(Cin=256, Cout=64)                  # a geometry the fused tail takes at Cb = 64
    halo, hdg, hpack = L.mhe_conv3x3_halo_nhwc, L.mhe_conv3x3_halo_dgrad_bn_nhwc, L.mhe_conv3x3_halo_pack_bf16
    wg, wgws, wgb, wgr, wgm = L.mhe_conv_wgrad_nhwc, L.mhe_conv_wgrad_ws_nhwc, L.mhe_conv_wgrad_batched_nhwc, L.mhe_conv_wgrad_rect_nhwc, L.mhe_conv_wgrad_multi_nhwc
    ok = (2, 16, 16, 64, 128, 1, 1, 1, 0, BF16)
    return [
        ("mhe_conv2d_nhwc", lambda: c2(D(), Z, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: null pointer"),
        ("mhe_conv2d_nhwc", lambda: c2(Z, P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: null pointer"),
        ("mhe_conv2d_nhwc", lambda: c2(D(), P, P, P, P, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: in_scale/in_shift must come together"),
        ("mhe_conv2d_nhwc", lambda: c2(D(dtype=7), P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: dtype=7"),
        ("mhe_conv2d_nhwc", lambda: c2(D(stride=0), P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: bad geometry"),
        ("mhe_conv2d_nhwc", lambda: c2(D(Cin=12), P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: Cin=12 must be a multiple of 8 (pad channels)"),
        ("mhe_conv2d_nhwc", lambda: c2(D(Cout=10, dtype=F32), P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: Cout=10 must be a multiple of 4"),
        ("mhe_conv2d_nhwc", lambda: c2(D(Cin=4096), P, P, P, P, P, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: fused input affine supports Cin <= 2048"),
        ("mhe_conv2d_nhwc", lambda: c2(D(res_half=1), P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: res_half needs a residual (and no output scatter)"),
        ("mhe_conv2d_nhwc", lambda: c2(D(H=2, k=3), P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: empty output"),
        ("mhe_conv2d_nhwc", lambda: c2(D(B=1 << 15, H=256, W=256), P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: too many output pixels"),
        ("mhe_conv2d_f32out_nhwc", lambda: f32o(D(), P, P, Z, Z, Z), "mhe_conv2d_f32out_nhwc: null output"),
        ("mhe_conv2d_f32out_nhwc", lambda: f32o(D(), Z, P, P, Z, Z), "mhe_conv2d_nhwc: null pointer"),
        ("mhe_conv2d_f32out_nhwc", lambda: f32o(D(dtype=F32), P, P, P, Z, Z), "mhe_conv2d_f32out_nhwc: bf16 operands, optional out_shift only"),
        ("mhe_conv2d_f32out_nhwc", lambda: f32o(D(relu_out=1), P, P, P, P, Z), "mhe_conv2d_f32out_nhwc: bf16 operands, optional out_shift only"),
        ("mhe_conv1x1_residual_in_nhwc", lambda: rin(D(), P, Z, P, P, P, P, Z, Z, Z, Z, Z), "mhe_conv1x1_residual_in_nhwc: x2, in_scale and in_shift are required"),
        ("mhe_conv1x1_residual_in_nhwc", lambda: rin(D(), P, P, P, P, P, Z, Z, Z, Z, Z, Z), "mhe_conv1x1_residual_in_nhwc: x2, in_scale and in_shift are required"),
        ("mhe_conv1x1_residual_in_nhwc", lambda: rin(D(), P, P, P, P, P, P, P, Z, Z, Z, Z), "mhe_conv1x1_residual_in_nhwc: x2_scale/x2_shift must come together"),
        ("mhe_conv1x1_residual_in_nhwc", lambda: rin(D(k=3, pad=1), P, P, P, P, P, P, Z, Z, Z, Z, Z), "mhe_conv1x1_residual_in_nhwc: 1x1 stride-1 only"),
        ("mhe_conv1x1_residual_in_nhwc", lambda: rin(D(), Z, P, P, P, P, P, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: null pointer"),
        ("mhe_conv1x1_residual_in_quarter_nhwc", lambda: rinq(D(), P, P, P, P, P, P, Z, Z, Z, Z, Z),
         "mhe_conv1x1_residual_in_quarter_nhwc: x2, in_scale, in_shift and a_quarter are required"),
        ("mhe_conv1x1_residual_in_quarter_nhwc", lambda: rinq(D(), P, P, P, P, P, P, Z, P, P, Z, Z), "mhe_conv1x1_residual_in_quarter_nhwc: x2_scale/x2_shift must come together"),
        ("mhe_conv1x1_residual_in_quarter_nhwc", lambda: rinq(D(stride=2), P, P, P, P, P, P, Z, Z, P, Z, Z), "mhe_conv1x1_residual_in_quarter_nhwc: 1x1 stride-1 only"),
        ("mhe_conv1x1_residual_in_quarter_nhwc", lambda: rinq(D(dtype=F32), P, P, P, P, P, P, Z, Z, P, Z, Z),
         "mhe_conv1x1_residual_in_quarter_nhwc: geometry not taken by the residual-tail kernel (variant 10; Cin=64 Cout=128 M=512)"),
        ("mhe_conv1x1_cat_bias_nhwc", lambda: cat(D(), P, Z, 64, P, P, Z, Z, Z), "mhe_conv1x1_cat_bias_nhwc: a bf16 1x1 stride-1 launch on two operand tensors with Cin and cin2 multiples of 64"),
        ("mhe_conv1x1_cat_bias_nhwc", lambda: cat(D(), P, P, 32, P, P, Z, Z, Z), "mhe_conv1x1_cat_bias_nhwc: a bf16 1x1 stride-1 launch on two operand tensors with Cin and cin2 multiples of 64"),
        ("mhe_conv1x1_cat_bias_nhwc", lambda: cat(D(tile=4), P, P, 64, P, P, Z, Z, Z), "mhe_conv1x1_cat_bias_nhwc: 128-row register-staged tiles only (tile 0, 1 or 2)"),
        ("mhe_conv1x1_cat_bias_nhwc", lambda: cat(D(), P, P, 64, Z, P, Z, Z, Z), "mhe_conv2d_nhwc: null pointer"),
        ("mhe_conv1x1_residual_in_masked_nhwc", lambda: rinm(D(), P, P, P, P, P, P, Z, Z, Z, Z, Z, Z, Z, Z, Z),
         "mhe_conv1x1_residual_in_masked_nhwc: x2, in_scale, in_shift and mask are required"),
        ("mhe_conv1x1_residual_in_masked_nhwc", lambda: rinm(D(k=3, pad=1), P, P, P, P, P, P, Z, Z, Z, Z, P, Z, Z, Z, Z), "mhe_conv1x1_residual_in_masked_nhwc: 1x1 stride-1 only"),
        ("mhe_conv1x1_residual_in_masked_nhwc", lambda: rinm(D(), P, P, P, P, P, P, Z, P, Z, Z, P, Z, Z, Z, Z), "mhe_conv1x1_residual_in_masked_nhwc: x2_scale/x2_shift must come together"),
        ("mhe_conv1x1_residual_in_masked_nhwc", lambda: rinm(D(), P, P, P, P, P, P, Z, Z, Z, Z, P, P, P, Z, Z), "mhe_conv1x1_residual_in_masked_nhwc: bn_y needs its mean_invstd and stats"),
        ("mhe_conv1x1_residual_in_masked_nhwc", lambda: rinm(D(tile=8), P, P, P, P, P, P, Z, Z, Z, Z, P, Z, Z, Z, Z),
         "mhe_conv1x1_residual_in_masked_nhwc: 128-row tiles only (tile 0, 1, 2, or 11 = the transfer-wave kernel)"),
        ("mhe_conv2d_masked_nhwc", lambda: msk(D(), P, P, P, Z, Z, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_masked_nhwc: mask is required"),
        ("mhe_conv2d_masked_nhwc", lambda: msk(D(), P, P, P, Z, P, P, Z, P, Z, Z, Z, Z), "mhe_conv2d_masked_nhwc: each bn_y needs its mean_invstd and stats (and bn_y1 needs bn_y0)"),
        ("mhe_conv2d_masked_nhwc", lambda: msk(D(), P, P, P, Z, P, Z, Z, Z, P, P, P, Z), "mhe_conv2d_masked_nhwc: each bn_y needs its mean_invstd and stats (and bn_y1 needs bn_y0)"),
        ("mhe_conv2d_masked_nhwc", lambda: msk(D(), P, Z, P, Z, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: null pointer"),
        ("mhe_conv2d_masked_nhwc", lambda: msk(D(B=0), P, P, P, Z, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_nhwc: bad geometry"),
        ("mhe_conv2d_masked_bits_nhwc", lambda: mbits(D(), P, P, P, Z, Z, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_masked_bits_nhwc: mask is required (kernels without the bit path read it)"),
        ("mhe_conv2d_masked_bits_nhwc", lambda: mbits(D(), P, P, P, Z, P, P, P, P, Z, Z, Z, Z, Z),
         "mhe_conv2d_masked_bits_nhwc: each bn_y needs its mean_invstd and stats (and bn_y1 needs bn_y0)"),
        ("mhe_conv2d_masked_bits_nhwc", lambda: mbits(D(), P, P, P, Z, P, P, Z, Z, Z, P, P, P, Z),
         "mhe_conv2d_masked_bits_nhwc: each bn_y needs its mean_invstd and stats (and bn_y1 needs bn_y0)"),
        ("mhe_conv2d_masked_bits_nhwc", lambda: mbits(D(Cout=68, dtype=F32), P, P, P, Z, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv2d_masked_bits_nhwc: Cout must be a multiple of 8"),
        ("mhe_conv2d_masked_bias_nhwc", lambda: mbias(D(), P, Z, 0, P, P, Z, P, Z, Z, Z, Z, Z), "mhe_conv2d_masked_bias_nhwc: mask and bias are required"),
        ("mhe_conv2d_masked_bias_nhwc", lambda: mbias(D(), P, P, 32, P, P, Z, P, P, Z, Z, Z, Z),
         "mhe_conv2d_masked_bias_nhwc: a concatenated operand needs a bf16 1x1 stride-1 launch with Cin and cin2 multiples of 64"),
        ("mhe_conv2d_masked_bias_nhwc", lambda: mbias(D(), P, Z, 0, P, P, Z, P, P, P, Z, P, Z), "mhe_conv2d_masked_bias_nhwc: bn_y needs its mean_invstd and stats"),
        ("mhe_conv2d_masked_bias_nhwc", lambda: mbias(D(tile=3), P, Z, 0, P, P, Z, P, P, Z, Z, Z, Z), "mhe_conv2d_masked_bias_nhwc: 128-row register-staged tiles only (tile 0, 1 or 2)"),
        ("mhe_conv2d_masked_bias_nhwc", lambda: mbias(D(pad=-1), P, Z, 0, P, P, Z, P, P, Z, Z, Z, Z), "mhe_conv2d_nhwc: bad geometry"),
        ("mhe_conv3x3s2_dgrad_nhwc", lambda: dg2(2, 8, 8, 128, 64, BF16, Z, w4, P, Z, Z, Z, Z, Z, Z, Z, Z, 0, Z), "mhe_conv3x3s2_dgrad_nhwc: null pointer"),
        ("mhe_conv3x3s2_dgrad_nhwc", lambda: dg2(2, 8, 8, 128, 64, BF16, P, w4hole, P, Z, Z, Z, Z, Z, Z, Z, Z, 0, Z), "mhe_conv3x3s2_dgrad_nhwc: null pointer"),
        ("mhe_conv3x3s2_dgrad_nhwc", lambda: dg2(2, 8, 8, 128, 64, BF16, P, w4, P, Z, Z, P, P, P, Z, Z, Z, 0, Z),
         "mhe_conv3x3s2_dgrad_nhwc: each bn_y needs its mean_invstd and stats (and the gate)"),
        ("mhe_conv3x3s2_dgrad_nhwc", lambda: dg2(2, 8, 8, 128, 64, BF16, P, w4, P, Z, P, Z, Z, Z, P, P, P, 0, Z),
         "mhe_conv3x3s2_dgrad_nhwc: each bn_y needs its mean_invstd and stats (and the gate)"),
        ("mhe_conv3x3s2_dgrad_nhwc", lambda: dg2(2, 0, 8, 128, 64, BF16, P, w4, P, Z, Z, Z, Z, Z, Z, Z, Z, 0, Z), "mhe_conv2d_nhwc: bad geometry"),
        ("mhe_conv1x1_stats_nhwc", lambda: L.mhe_conv1x1_stats_nhwc(D(Cout=256), P, P, Z, Z, Z, Z), "mhe_conv1x1_stats_nhwc: null pointer"),
        ("mhe_conv1x1_stats_nhwc", lambda: L.mhe_conv1x1_stats_nhwc(D(Cin=96, Cout=256), P, P, Z, Z, P, Z),
         "mhe_conv1x1_stats_nhwc: bf16 1x1 stride-1 with 64 / 128 / 256 input channels and a multiple of 256 output channels"),
        ("mhe_conv1x1_stats_nhwc", lambda: L.mhe_conv1x1_stats_nhwc(D(Cout=256), P, P, P, Z, P, Z), "mhe_conv1x1_stats_nhwc: in_scale/in_shift must come together"),
        ("mhe_conv1x1_stats_nhwc", lambda: L.mhe_conv1x1_stats_nhwc(D(B=0, Cout=256), P, P, Z, Z, P, Z), "mhe_conv1x1_stats_nhwc: bad pixel count"),
        ("mhe_conv1x1_stats_nhwc", lambda: L.mhe_conv1x1_stats_nhwc(D(B=1, H=8, W=8, Cin=256, Cout=256), P, P, Z, Z, P, Z),
         "mhe_conv1x1_stats_nhwc: geometry not taken by the resident-slab kernel (M=64 Cout=256)"),
        ("mhe_bottleneck_tail_nhwc", lambda: tail(T, 64, Z, P, P, P, P, P, P, Z, Z, P, P, P, Z, Z), "mhe_bottleneck_tail_nhwc: null pointer"),
        ("mhe_bottleneck_tail_nhwc", lambda: tail(D(Cin=256, Cout=64, dtype=F32), 64, P, P, P, P, P, P, P, Z, Z, P, P, P, Z, Z), "mhe_bottleneck_tail_nhwc: bf16 storage only"),
        ("mhe_bottleneck_tail_nhwc", lambda: tail(T, 64, P, P, P, P, P, P, P, P, Z, P, P, P, Z, Z), "mhe_bottleneck_tail_nhwc: id_scale/id_shift must come together"),
        ("mhe_bottleneck_tail_nhwc", lambda: tail(D(B=0, Cin=256, Cout=64), 64, P, P, P, P, P, P, P, Z, Z, P, P, P, Z, Z), "mhe_bottleneck_tail_nhwc: bad pixel count"),
        ("mhe_bottleneck_tail_nhwc", lambda: tail(T, 32, P, P, P, P, P, P, P, Z, Z, P, P, P, Z, Z),
         "mhe_bottleneck_tail_nhwc: needs Cin = 4 Cb, Cb 64 / 128, Cout 64 / 128, pixels % 128 == 0 (Cin=256 Cb=32 Cout=64 M=512)"),
        ("mhe_bottleneck_tail_bits_nhwc", lambda: tbits(T, 64, P, P, P, P, P, P, P, Z, Z, P, Z, P, P, Z, Z), "mhe_bottleneck_tail_nhwc: null pointer"),
        ("mhe_bottleneck_tail_bits_nhwc", lambda: tbits(T, 64, P, P, P, P, P, P, P, Z, P, P, P, P, P, Z, Z), "mhe_bottleneck_tail_nhwc: id_scale/id_shift must come together"),
        ("mhe_bottleneck_tail_bits_nhwc", lambda: tbits(D(H=15, W=15, Cin=256, Cout=64), 64, P, P, P, P, P, P, P, Z, Z, P, P, P, P, Z, Z),
         "mhe_bottleneck_tail_nhwc: needs Cin = 4 Cb, Cb 64 / 128, Cout 64 / 128, pixels % 128 == 0 (Cin=256 Cb=64 Cout=64 M=450)"),
        ("mhe_bottleneck_tail_quarter_nhwc", lambda: tq(T, 64, P, P, P, P, P, P, P, Z, Z, P, Z, P, Z, Z), "mhe_bottleneck_tail_quarter_nhwc: null pointer"),
        ("mhe_bottleneck_tail_quarter_nhwc", lambda: tq(D(Cin=256, Cout=64, dtype=F32), 64, P, P, P, P, P, P, P, Z, Z, P, P, P, Z, Z), "mhe_bottleneck_tail_quarter_nhwc: bf16 storage only"),
        ("mhe_bottleneck_tail_quarter_nhwc", lambda: tq(T, 64, P, P, P, P, P, P, P, Z, P, P, P, P, Z, Z), "mhe_bottleneck_tail_quarter_nhwc: id_scale/id_shift must come together"),
        ("mhe_bottleneck_tail_quarter_nhwc", lambda: tq(D(H=0, Cin=256, Cout=64), 64, P, P, P, P, P, P, P, Z, Z, P, P, P, Z, Z), "mhe_bottleneck_tail_quarter_nhwc: bad geometry"),
        # 2^22 pixels of 512 channels: the compact tensor's 32-bit byte offsets, which only the quarter form bounds by M * Cin
        ("mhe_bottleneck_tail_quarter_nhwc", lambda: tq(D(B=256, H=128, W=128, Cin=512, Cout=128), 128, P, P, P, P, P, P, P, Z, Z, P, P, P, Z, Z),
         "mhe_bottleneck_tail_quarter_nhwc: bad pixel count"),
        ("mhe_bottleneck_tail_quarter_nhwc", lambda: tq(D(Cin=256, Cout=64, k=3, pad=1), 64, P, P, P, P, P, P, P, Z, Z, P, P, P, Z, Z),
         "mhe_bottleneck_tail_quarter_nhwc: needs Cin = 4 Cb, Cb 64 / 128, Cout 64 / 128, pixels % 128 == 0 (Cin=256 Cb=64 Cout=64 M=512)"),
        ("mhe_conv3x3_halo_nhwc", lambda: halo(8, 32, 32, 64, 128, Z, P, P, Z, Z, 0, Z, Z, Z, Z, Z, Z, Z, Z), "mhe_conv3x3_halo_nhwc: null pointer"),
        ("mhe_conv3x3_halo_nhwc", lambda: halo(8, 32, 32, 64, 128, P, P, P, P, Z, 0, Z, Z, Z, Z, Z, Z, Z, Z), "mhe_conv3x3_halo_nhwc: in_scale/in_shift must come together"),
        ("mhe_conv3x3_halo_nhwc", lambda: halo(8, 32, 32, 64, 128, P, P, P, Z, Z, 0, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv3x3_halo_nhwc: a_out is the normalised operand: it needs in_scale / in_shift"),
        ("mhe_conv3x3_halo_nhwc", lambda: halo(8, 32, 32, 64, 128, P, P, P, Z, Z, 0, Z, P, Z, P, Z, Z, Z, Z),
         "mhe_conv3x3_halo_nhwc: statistics in the forward form, residual in the data-gradient form only"),
        ("mhe_conv3x3_halo_nhwc", lambda: halo(8, 32, 32, 64, 128, P, P, P, Z, Z, 0, Z, Z, Z, Z, P, P, P, Z), "mhe_conv3x3_halo_nhwc: bn_y needs the gate, its mean_invstd and stats"),
        ("mhe_conv3x3_halo_nhwc", lambda: halo(0, 32, 32, 64, 128, P, P, P, Z, Z, 0, Z, Z, Z, Z, Z, Z, Z, Z), "mhe_conv3x3_halo_nhwc: bad geometry"),
        ("mhe_conv3x3_halo_nhwc", lambda: halo(1 << 21, 32, 32, 64, 128, P, P, P, Z, Z, 0, Z, Z, Z, Z, Z, Z, Z, Z), "mhe_conv3x3_halo_nhwc: bad geometry"),
        ("mhe_conv3x3_halo_nhwc", lambda: halo(8, 20, 20, 64, 128, P, P, P, Z, Z, 0, Z, Z, Z, Z, Z, Z, Z, Z),
         "mhe_conv3x3_halo_nhwc: geometry not taken (3x3 stride 1 pad 1, W 32 / 16, Cin % 64, Cin <= 512, Cout % 128)"),
        ("mhe_conv3x3_halo_dgrad_bn_nhwc", lambda: hdg(8, 32, 32, 64, 128, P, P, P, P, P, Z, Z, Z, Z, Z, Z, Z), "mhe_conv3x3_halo_dgrad_bn_nhwc: null pointer"),
        ("mhe_conv3x3_halo_dgrad_bn_nhwc", lambda: hdg(8, 32, 32, 64, 128, P, P, P, P, P, Z, Z, P, P, P, Z, Z), "mhe_conv3x3_halo_dgrad_bn_nhwc: bn_y needs its mean_invstd and stats"),
        ("mhe_conv3x3_halo_dgrad_bn_nhwc", lambda: hdg(8, -1, 32, 64, 128, P, P, P, P, P, Z, Z, P, Z, Z, Z, Z), "mhe_conv3x3_halo_dgrad_bn_nhwc: bad geometry"),
        ("mhe_conv3x3_halo_dgrad_bn_nhwc", lambda: hdg(8, 32, 32, 96, 128, P, P, P, P, P, Z, Z, P, Z, Z, Z, Z),
         "mhe_conv3x3_halo_dgrad_bn_nhwc: geometry not taken (see mhe_conv3x3_halo_nhwc)"),
        ("mhe_conv3x3_halo_pack_bf16", lambda: hpack(P, Z, 128, 64, Z), "mhe_conv3x3_halo_pack_bf16: null pointer"),
        ("mhe_conv3x3_halo_pack_bf16", lambda: hpack(P, P, 100, 64, Z), "mhe_conv3x3_halo_pack_bf16: Cout % 128 and Cin % 64 must be 0"),
        ("mhe_conv_wgrad_nhwc", lambda: wg(D(), P, Z, P, 0, Z), "mhe_conv_wgrad_nhwc: null pointer"),
        ("mhe_conv_wgrad_nhwc", lambda: wg(D(stride=0), P, P, P, 0, Z), "mhe_conv_wgrad_nhwc: bad geometry"),
        ("mhe_conv_wgrad_nhwc", lambda: wg(D(Cin=6), P, P, P, 0, Z), "mhe_conv_wgrad_nhwc: Cin=6 and Cout=128 must be multiples of 4"),
        ("mhe_conv_wgrad_nhwc", lambda: wg(D(dtype=7), P, P, P, 0, Z), "mhe_conv_wgrad_nhwc: dtype=7"),
        ("mhe_conv_wgrad_nhwc", lambda: wg(D(H=2, k=3), P, P, P, 0, Z), "mhe_conv_wgrad_nhwc: empty output"),
        ("mhe_conv_wgrad_nhwc", lambda: wg(D(), P, P, P, 8, Z), "mhe_conv_wgrad_nhwc: ldw=8 < KH*KW*Cin=64"),
        ("mhe_conv_wgrad_ws_nhwc", lambda: wgws(D(), Z, P, P, 0, P, 1 << 30, Z), "mhe_conv_wgrad_nhwc: null pointer"),
        ("mhe_conv_wgrad_ws_nhwc", lambda: wgws(D(pad=-1), P, P, P, 0, P, 1 << 30, Z), "mhe_conv_wgrad_nhwc: bad geometry"),
        ("mhe_conv_wgrad_ws_nhwc", lambda: wgws(D(B=8, H=32, W=32, Cin=64, Cout=64, k=3, pad=1), P, P, P, 0, P, 1, Z),
         "mhe_conv_wgrad_ws_nhwc: workspace of 1 floats, this launch needs 655360 (mhe_conv_wgrad_workspace_floats)"),
        ("mhe_conv_wgrad_batched_nhwc", lambda: wgb(D(), 0, P, 0, P, 0, P, 0, 0, Z, 0, Z), "mhe_conv_wgrad_batched_nhwc: bad arguments"),
        ("mhe_conv_wgrad_batched_nhwc", lambda: wgb(D(), 2, P, -1, P, 0, P, 0, 0, Z, 0, Z), "mhe_conv_wgrad_batched_nhwc: bad arguments"),
        ("mhe_conv_wgrad_batched_nhwc", lambda: wgb(D(dtype=F32), 2, P, 0, P, 0, P, 0, 0, Z, 0, Z), "mhe_conv_wgrad_batched_nhwc: bf16 operands with channel counts in multiples of 8"),
        ("mhe_conv_wgrad_batched_nhwc", lambda: wgb(D(), 2, Z, 0, P, 0, P, 0, 0, Z, 0, Z), "mhe_conv_wgrad_nhwc: null pointer"),
        ("mhe_conv_wgrad_batched_nhwc", lambda: wgb(D(H=11, W=6, Cin=8, Cout=72, k=9, pad=4), 2, P, 0, P, 0, P, 0, 0, Z, 0, Z),
         "mhe_conv_wgrad_batched_nhwc: the grouped form runs on the LDS-DMA kernel (bf16, operands below 2 GiB)"),
        ("mhe_conv_wgrad_rect_nhwc", lambda: wgr(D(), 0, 0, 16, 16, P, P, P, 0, Z, 0, Z), "mhe_conv_wgrad_rect_nhwc: bad width geometry"),
        ("mhe_conv_wgrad_rect_nhwc", lambda: wgr(D(), 1, 0, 17, 16, P, P, P, 0, Z, 0, Z), "mhe_conv_wgrad_rect_nhwc: output larger than the input allows"),
        ("mhe_conv_wgrad_rect_nhwc", lambda: wgr(D(), 1, 0, 16, 16, P, P, Z, 0, Z, 0, Z), "mhe_conv_wgrad_nhwc: null pointer"),
        ("mhe_conv_wgrad_rect_nhwc", lambda: wgr(D(Cout=6), 1, 0, 16, 16, P, P, P, 0, Z, 0, Z), "mhe_conv_wgrad_nhwc: Cin=64 and Cout=6 must be multiples of 4"),
        ("mhe_conv_wgrad_multi_nhwc", lambda: wgm(Z, 1, Z, 0, Z), "mhe_conv_wgrad_multi_nhwc: 1 .. 256 problems"),
        ("mhe_conv_wgrad_multi_nhwc", lambda: wgm(_items([ok]), 0, Z, 0, Z), "mhe_conv_wgrad_multi_nhwc: 1 .. 256 problems"),
        ("mhe_conv_wgrad_multi_nhwc", lambda: wgm(_items([ok, (2, 16, 16, 64, 128, 1, 1, 0, 0, BF16)]), 2, Z, 0, Z), "mhe_conv_wgrad_multi_nhwc: bad geometry"),
        ("mhe_conv_wgrad_multi_nhwc", lambda: wgm(_items([ok, ok], ptr=None), 2, Z, 0, Z), "mhe_conv_wgrad_multi_nhwc: null pointer (problem 0)"),
        ("mhe_conv_wgrad_multi_nhwc", lambda: wgm(_items([ok, ok], ldw=8), 2, Z, 0, Z), "mhe_conv_wgrad_multi_nhwc: ldw=8 < KH*KW*Cin=64 (problem 0)"),
    ]


def test_entries_refuse_before_launching():
    L = _lib.lib()
    seen = set()
    for entry, call, text in _refusals(L):
        rc = call()
        assert rc == MHE_ERR_ARG, (entry, text, rc, L.mhe_last_error())
        assert text.encode() in L.mhe_last_error(), (entry, text, L.mhe_last_error())
        seen.add(entry)
    assert len(seen) == 22, sorted(seen)              # every launching convolution, halo and weight-gradient entry


# what a problem list must not hold (the single launch refuses each; the list form used to plan them first and divided by an empty output's
# size): (descriptors, index of the offender, text)
BAD_ITEMS = [
    ([(2, 16, 16, 64, 128, 1, 1, 1, 0, BF16), (2, 2, 16, 64, 128, 3, 3, 1, 0, BF16)], "mhe_conv_wgrad_multi_nhwc: empty output (problem 1)"),
    ([(2, 16, 16, 6, 128, 1, 1, 1, 0, BF16), (2, 16, 16, 64, 128, 1, 1, 1, 0, BF16)], "mhe_conv_wgrad_multi_nhwc: Cin=6 and Cout=128 must be multiples of 4 (problem 0)"),
    ([(2, 16, 16, 64, 128, 1, 1, 1, 0, BF16)] * 2 + [(2, 16, 16, 64, 130, 1, 1, 1, 0, F32)], "mhe_conv_wgrad_multi_nhwc: Cin=64 and Cout=130 must be multiples of 4 (problem 2)"),
    ([(2, 16, 16, 64, 128, 1, 1, 1, 0, BF16), (2, 16, 16, 64, 128, 1, 1, 1, 0, 7)], "mhe_conv_wgrad_multi_nhwc: dtype=7 (problem 1)"),
]


@pytest.mark.parametrize("descs,text", BAD_ITEMS, ids=["empty-output", "cin-6", "cout-130", "dtype-7"])
def test_problem_list_refuses_what_the_single_launch_refuses(descs, text):
    L = _lib.lib()
    arr = _items(descs)
    assert L.mhe_conv_wgrad_multi_workspace_floats(arr, len(descs)) == 0
    assert L.mhe_conv_wgrad_multi_nhwc(arr, len(descs), Z, 0, Z) == MHE_ERR_ARG
    assert text.encode() in L.mhe_last_error(), L.mhe_last_error()
    good = _items(descs[:1] if "problem 0" not in text else descs[1:2])
    assert L.mhe_conv_wgrad_multi_workspace_floats(good, 1) == L.mhe_conv_wgrad_workspace_floats(C.byref(good[0].d))


def test_queries_refuse_bad_geometry():
    L = _lib.lib()
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(Cin=0), dict(Cout=0), dict(k=0), dict(stride=0)):
        d = D(**bad)
        assert L.mhe_conv_wgrad_variant(d, 0, 0, 1) == -1, bad
        assert L.mhe_conv_wgrad_workspace_floats(d) == 0 and L.mhe_conv_wgrad_batched_workspace_floats(d, 2) == 0 and L.mhe_conv_wgrad_rect_workspace_floats(d, 4, 4) == 0, bad
        assert L.mhe_bottleneck_tail_supported(d, 64) == 0, bad
    assert L.mhe_conv_wgrad_variant(Z, 0, 0, 1) == -1 and L.mhe_conv_wgrad_variant(D(), 0, 0, 0) == -1
    assert L.mhe_conv_wgrad_workspace_floats(Z) == 0 and L.mhe_conv_wgrad_batched_workspace_floats(D(), 0) == 0 and L.mhe_conv_wgrad_rect_workspace_floats(D(), 0, 4) == 0
    assert L.mhe_conv_tile(Z) == -1 and L.mhe_conv_tile_mode(Z, 0) == -1 and L.mhe_conv_tile_mode(D(), 4) == -1 and L.mhe_conv_tile_mode(D(), -1) == -1
    assert L.mhe_bottleneck_tail_supported(Z, 64) == 0 and L.mhe_bottleneck_tail_supported(D(Cin=256, Cout=64, dtype=F32), 64) == 0
    assert L.mhe_bottleneck_tail_supported(D(Cin=256, Cout=64), 64) == 1 and L.mhe_bottleneck_tail_supported(D(Cin=256, Cout=64), 128) == 0
    assert L.mhe_conv3x3_halo_supported(8, 32, 32, 64, 128) == 1
    for g in ((0, 32, 32, 64, 128), (8, 20, 20, 64, 128), (8, 32, 32, 96, 128), (8, 32, 32, 64, 100), (1 << 21, 32, 32, 64, 128)):
        assert L.mhe_conv3x3_halo_supported(*g) == 0, g


# ---- dispatch choices, pinned ------------------------------------------------------------------------------------------------------------
# mhe_conv_tile_mode, modes 0 - 3, bf16, pad = k // 2, at the bench batch (256) and at a batch of 4: ((B, map side, Cin, Cout, k, stride), variants)
TILE_MODES = [
    ((256, 64, 64, 64, 1, 1), (8, 8, 0, 0)),
    ((256, 64, 64, 64, 3, 1), (9, 9, 0, 0)),
    ((256, 64, 64, 256, 1, 1), (8, 8, 1, 7)),
    ((256, 64, 256, 64, 1, 1), (0, 0, 0, 0)),
    ((256, 64, 256, 128, 1, 1), (1, 1, 1, 1)),
    ((256, 64, 128, 128, 3, 2), (1, 1, 1, 1)),
    ((256, 32, 128, 128, 3, 1), (1, 1, 1, 1)),
    ((256, 32, 128, 512, 1, 1), (8, 8, 10, 7)),
    ((256, 32, 512, 128, 1, 1), (1, 1, 1, 1)),
    ((256, 64, 256, 512, 1, 2), (7, 2, 1, 7)),
    ((256, 32, 512, 256, 1, 1), (7, 2, 10, 7)),
    ((256, 32, 256, 256, 3, 2), (7, 2, 1, 7)),
    ((256, 16, 256, 256, 3, 1), (7, 2, 1, 7)),
    ((256, 16, 256, 1024, 1, 1), (11, 11, 10, 7)),
    ((256, 16, 1024, 256, 1, 1), (7, 2, 10, 7)),
    ((256, 32, 512, 1024, 1, 2), (7, 2, 1, 7)),
    ((256, 16, 1024, 512, 1, 1), (7, 2, 10, 7)),
    ((256, 16, 512, 512, 3, 2), (13, 1, 1, 13)),
    ((256, 8, 512, 512, 3, 1), (13, 1, 1, 13)),
    ((256, 8, 512, 2048, 1, 1), (7, 2, 10, 7)),
    ((256, 8, 2048, 512, 1, 1), (1, 1, 10, 1)),
    ((256, 16, 1024, 2048, 1, 2), (7, 2, 1, 7)),
    ((4, 64, 64, 64, 1, 1), (0, 0, 0, 0)),
    ((4, 64, 64, 64, 3, 1), (0, 0, 0, 0)),
    ((4, 64, 64, 256, 1, 1), (1, 1, 1, 1)),
    ((4, 64, 256, 64, 1, 1), (0, 0, 0, 0)),
    ((4, 64, 256, 128, 1, 1), (1, 1, 1, 1)),
    ((4, 64, 128, 128, 3, 2), (1, 1, 1, 1)),
    ((4, 32, 128, 128, 3, 1), (1, 1, 1, 1)),
    ((4, 32, 128, 512, 1, 1), (1, 1, 10, 1)),
    ((4, 32, 512, 128, 1, 1), (1, 1, 1, 1)),
    ((4, 64, 256, 512, 1, 2), (1, 1, 1, 1)),
    ((4, 32, 512, 256, 1, 1), (1, 1, 10, 1)),
    ((4, 32, 256, 256, 3, 2), (1, 1, 1, 1)),
    ((4, 16, 256, 256, 3, 1), (1, 1, 1, 1)),
    ((4, 16, 256, 1024, 1, 1), (1, 1, 10, 1)),
    ((4, 16, 1024, 256, 1, 1), (1, 1, 10, 1)),
    ((4, 32, 512, 1024, 1, 2), (1, 1, 1, 1)),
    ((4, 16, 1024, 512, 1, 1), (1, 1, 10, 1)),
    ((4, 16, 512, 512, 3, 2), (1, 1, 1, 1)),
    ((4, 8, 512, 512, 3, 1), (1, 1, 1, 1)),
    ((4, 8, 512, 2048, 1, 1), (1, 1, 10, 1)),
    ((4, 8, 2048, 512, 1, 1), (1, 1, 10, 1)),
    ((4, 16, 1024, 2048, 1, 2), (1, 1, 1, 1)),
]

# ((B, H, W, Cin, Cout, k, stride, pad, dtype), (Ho, Wo, nbatch) given to the variant / rect / batched queries,
#  (variant, workspace_floats, batched_workspace_floats(nbatch), rect_workspace_floats(Ho, Wo)))
WGRAD = [
    ((3, 7, 5, 24, 72, 3, 1, 1, 1), (0, 0, 1), (1128128, 0, 0, 0)),    # ragged: N = 216, Cout = 72, Ho != Wo
    ((3, 7, 5, 24, 72, 3, 1, 1, 0), (7, 5, 1), (128128, 65536, 65536, 65536)),    # ... in f32
    ((1100, 1, 1, 72, 136, 1, 1, 0, 1), (0, 0, 5), (1128128, 98304, 491520, 0)),    # grouped: five dense products side by side
    ((300, 1, 1, 1032, 256, 1, 1, 0, 1), (0, 0, 3), (1256256, 0, 0, 0)),    # grouped on the 256 x 256 tile
    ((256, 64, 64, 64, 64, 1, 1, 0, 1), (0, 0, 1), (1064064, 2097152, 2097152, 0)),    # narrow + small
    ((256, 64, 64, 64, 256, 1, 1, 0, 1), (0, 0, 1), (1128064, 4194304, 4194304, 0)),    # narrow
    ((256, 64, 64, 64, 64, 3, 1, 1, 1), (0, 0, 1), (1064128, 3932160, 3932160, 0)),    # small
    ((256, 32, 32, 128, 128, 3, 1, 1, 1), (0, 0, 1), (1128128, 8257536, 8257536, 0)),    # 128 x 128
    ((256, 16, 16, 256, 256, 3, 1, 1, 1), (0, 0, 1), (1256256, 16515072, 16515072, 0)),    # big
    ((256, 16, 16, 1024, 256, 1, 1, 0, 1), (0, 0, 1), (1256256, 16777216, 16777216, 0)),    # big, 1x1
    ((256, 8, 8, 512, 2048, 1, 1, 0, 1), (0, 0, 1), (1128128, 8388608, 8388608, 0)),    # 16k pixels: stays on 128 x 128
    ((256, 256, 128, 8, 64, 7, 2, 3, 1), (128, 128, 1), (1064128, 4194304, 4194304, 4194304)),    # the stem over pixel pairs (rect: given output size)
    ((2, 11, 6, 8, 72, 9, 1, 4, 1), (0, 0, 1), (2128128, 0, 0, 0)),    # 81 taps: register-staged bf16 kernel
    ((3, 7, 5, 12, 68, 3, 1, 1, 1), (0, 0, 1), (128128, 32768, 32768, 0)),    # Cin % 8 != 0: generic kernel on bf16 storage
]

# lists of WGRAD rows (mixed tile classes, repeats, the generic kernels) and their mhe_conv_wgrad_multi_workspace_floats
MULTI = [
    ([4, 5, 6, 7, 8, 9, 10], 50266112),
    ([0, 7, 7, 1, 13], 33325056),
    ([8, 9, 8], 49020928),
    ([6], 3932160),
    ([4, 4, 4, 12, 0], 8220672),
]


def test_kernel_variant_per_operand_form_over_the_trunk():
    L = _lib.lib()
    for (B, S, Cin, Cout, k, s), want in TILE_MODES:
        d = D(B, S, S, Cin, Cout, k, s, k // 2)
        got = tuple(L.mhe_conv_tile_mode(d, m) for m in range(4))
        assert got == want, ((B, S, Cin, Cout, k, s), got, want)
        assert L.mhe_conv_tile(d) == want[0]


def test_weight_gradient_variants_and_workspaces():
    L = _lib.lib()
    for (B, H, W, Cin, Cout, k, s, p, dt), (Ho, Wo, nb), want in WGRAD:
        d = D(B, H, W, Cin, Cout, k, s, p, dt)
        got = (L.mhe_conv_wgrad_variant(d, Ho, Wo, nb), L.mhe_conv_wgrad_workspace_floats(d), L.mhe_conv_wgrad_batched_workspace_floats(d, nb),
               L.mhe_conv_wgrad_rect_workspace_floats(d, Ho, Wo))
        assert got == want, ((B, H, W, Cin, Cout, k, s, p, dt), got, want)
    for rows, want in MULTI:
        descs = [(g[0], g[1], g[2], g[3], g[4], g[5], g[5], g[6], g[7], g[8]) for g in (WGRAD[i][0] for i in rows)]
        assert L.mhe_conv_wgrad_multi_workspace_floats(_items(descs), len(descs)) == want, rows
