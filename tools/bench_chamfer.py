#!/usr/bin/env python3
"""Time of the hand-object Chamfer distance (mhe_chamfer_f32 and mhe_chamfer_bwd_f32, csrc/chamfer.hip) at the metrics-pass sizes, next to the
reference's broadcast expression (hand/criteria.py:24-35) written in torch on the same device.  Not the product path.

Per shape (B, N, P, VO): device-event time per call, median of WINDOWS windows of REPS calls after a warm-up of every shape; the forward with and
without the argmin buffers; the reverse.  The forward evaluates 2 N B P VO point pairs (once per direction) at 7 vector instructions a pair
(3 subtractions, a product, 2 fused multiply-adds, a minimum or a compare): the bound is the f32 vector issue rate, 256 CUs x 128 lanes x 2.4 GHz
= 78.6e12 lane-instructions/s (half the 157.3 TFLOP/s peak, which counts a fused multiply-add twice); the bytes (points, vertices, outputs) are
printed beside it and are nowhere near the HBM bound.  The torch expression materialises (N, B, P, VO, 3): it runs at the largest power-of-two
B <= 256 whose difference tensor stays within TORCH_GIB (default 16) GiB, and that B is printed.

    python tools/bench_chamfer.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SHAPES = ((256, 64, 21, 1000), (256, 200, 21, 1000), (256, 64, 778, 1000))          # (B, N, P, VO)
REPS, WINDOWS = int(os.environ.get("REPS", 20)), int(os.environ.get("WINDOWS", 7))
TORCH_GIB = float(os.environ.get("TORCH_GIB", 16))
VALU_RATE = 256 * 128 * 2.4e9


def timed(fn, reps=REPS, windows=WINDOWS):
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), min(out), max(out)


def inputs(B, N, P, VO, dev):
    g = torch.Generator(device="cpu").manual_seed(B + N + P)
    pts = (torch.randn(N, B, P, 3, generator=g) * 0.7).to(dev)
    scale = (torch.rand(B, generator=g) * 0.015 + 0.025).to(dev)
    root = ((torch.rand(B, 3, generator=g) - 0.5) * 160 + torch.tensor([0.0, 0.0, 500.0])).to(dev)
    obj = (root.cpu()[:, None] + (torch.rand(B, VO, 3, generator=g) - 0.5) * 180).to(dev)
    return pts, scale, root, obj


def torch_broadcast(pts, scale, root, obj):
    """hand/criteria.py:24-35 as it stands"""
    a = pts * scale[:, None, None] * 1000 + root[:, None]
    d = (a[:, :, :, None, :] - obj[:, None, :, :]).norm(p=2, dim=-1)
    return d.min(-1)[0].mean(-1) + d.min(-2)[0].mean(-1)


def main():
    from mhentropy_amd import ops
    assert torch.cuda.is_available(), "bench_chamfer needs the GPU: there is no CPU path"
    dev = "cuda"
    print(f"device {torch.cuda.get_device_name(0)}; REPS {REPS}, WINDOWS {WINDOWS}; times are ms per call: median (min-max)")
    for B, N, P, VO in SHAPES:
        pts, scale, root, obj = inputs(B, N, P, VO, dev)
        g = torch.rand(N, B, device=dev) + 0.5
        dist, _, ip, io = ops.chamfer(pts, scale, root, obj, want_idx=True)
        for _ in range(3):
            ops.chamfer(pts, scale, root, obj); ops.chamfer(pts, scale, root, obj, want_idx=True); ops.chamfer_bwd(pts, scale, root, obj, None, ip, io, g)
        torch.cuda.synchronize()
        pairs = 2.0 * N * B * P * VO
        nbytes = N * B * P * 12 + B * VO * 12 + N * B * 12
        rows = (("forward", lambda: ops.chamfer(pts, scale, root, obj), nbytes),
                ("forward + argmins", lambda: ops.chamfer(pts, scale, root, obj, want_idx=True), nbytes + N * B * (P + VO) * 4),
                ("reverse", lambda: ops.chamfer_bwd(pts, scale, root, obj, None, ip, io, g), None))
        print(f"B={B} N={N} P={P} VO={VO}: {pairs:.3e} pair evaluations per forward")
        for name, fn, nb in rows:
            med, lo, hi = timed(fn)
            line = f"  {name:18s} {med:.4f} ({lo:.4f}-{hi:.4f})"
            if nb is not None:
                line += (f"  {7 * pairs / (med * 1e-3) / VALU_RATE * 100:.1f} % of the f32 vector issue rate; {nb / 1e6:.1f} MB = "
                         f"{nb / (med * 1e-3) / 1e12:.3f} TB/s")
            print(line, flush=True)
        Bt = B
        while Bt > 1 and N * Bt * P * VO * 12 > TORCH_GIB * 2 ** 30:
            Bt //= 2
        sub = (pts[:, :Bt].contiguous(), scale[:Bt], root[:Bt], obj[:Bt])
        ref = torch_broadcast(*sub)
        err = float((ref - dist[:, :Bt]).abs().max() / ref.abs().max())
        for _ in range(2):
            torch_broadcast(*sub)
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: torch_broadcast(*sub), reps=3, windows=5)
        ours = timed(lambda: ops.chamfer(*sub))[0]
        print(f"  torch broadcast at B={Bt} (difference tensor {N * Bt * P * VO * 12 / 2 ** 30:.1f} GiB): {med:.3f} ({lo:.3f}-{hi:.3f}); the kernel at that B "
              f"{ours:.4f}; max rel diff of the two {err:.1e}", flush=True)
        del sub, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
