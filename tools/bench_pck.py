#!/usr/bin/env python3
"""Time of the 3D PCK curve (mhe_pck_curve_f32, csrc/pck.hip) at the reference iteration's evaluation shape, N = 200 hypotheses of B = 64 images,
T = 100 thresholds from 0 to 50 mm, for the joints (P = 21) and the mesh (P = 778), next to the route that exists without it: a torch
composition of the same numbers - the distances (N, B, P), then `d[..., None] <= thr` over chunks of hypotheses ((chunk, B, P, T) comparisons
through HBM), a sum over the points, the trapezoid rule in f64 - on the same device.  Not the product path.  The composition's outputs are
compared with the kernel's before anything is timed (its distances round differently, so a few of the R P T comparisons may fall the other way;
their number is reported).

Device-event time per call, median of WINDOWS windows of REPS calls after a warm-up; min and max of the windows beside it.  The kernel reads
every coordinate once and writes T + 2 words a row: its bound is HBM, and its bytes over its time are printed as a rate.

    python tools/bench_pck.py [--json out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

N, B, T = int(os.environ.get("N", 200)), int(os.environ.get("B", 64)), int(os.environ.get("T", 100))
PS = tuple(int(p) for p in os.environ.get("P", "21,778").split(","))
REPS, WINDOWS = int(os.environ.get("REPS", 10)), int(os.environ.get("WINDOWS", 7))
CHUNK_ELEMENTS = 1 << 26          # comparisons of one chunk of the composition


def timed(fn, reps, windows):
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


def torch_composition(pred, target, scale, thr, unit=1000.0):
    """the same outputs by torch: hits (N, B, T) int32, auc (N, B), err (N, B)"""
    n, b, p = pred.shape[:3]
    su = (scale * unit)[None, :, None, None]
    d = (pred * su - target[None] * su).norm(dim=-1)
    hits = torch.empty(n, b, thr.shape[0], device=pred.device, dtype=torch.int32)
    chunk = max(1, CHUNK_ELEMENTS // (b * p * thr.shape[0]))
    for n0 in range(0, n, chunk):
        hits[n0:n0 + chunk] = (d[n0:n0 + chunk, :, :, None] <= thr).sum(2, dtype=torch.int32)
    t = thr.double()
    auc = ((t[1:] - t[:-1]) * (hits[..., :-1] + hits[..., 1:]).double()).sum(-1) / (2.0 * p * (t[-1] - t[0]))
    return hits, auc.float(), d.mean(-1)


def one_shape(ops, P):
    g = torch.Generator().manual_seed(N + B + P)
    target = torch.randn(B, P, 3, generator=g)
    pred = (target[None] + 0.15 * torch.randn(N, B, P, 3, generator=g)).cuda()
    target, scale = target.cuda(), (0.025 + 0.015 * torch.rand(B, generator=g)).cuda()
    thr = ops.pck_thresholds(np.linspace(0.0, 50.0, T).astype(np.float32).tolist(), pred.device)
    kernel = lambda: ops.pck_curve(pred, target, scale, thr)
    comp = lambda: torch_composition(pred, target, scale, thr)
    hits, auc, err = kernel()
    hits_t, auc_t, err_t = comp()
    diff = {"hits_that_differ": int((hits != hits_t).sum()), "hits_compared": hits.numel(), "hits_max_abs": int((hits - hits_t).abs().max()),
            "auc_abs": float((auc - auc_t).abs().max()), "err_rel": float(((err - err_t).abs() / err_t).max())}
    assert diff["hits_max_abs"] <= 2 and diff["auc_abs"] < 1e-3 and diff["err_rel"] < 1e-4, diff          # the two routes compute the same numbers
    for _ in range(3):
        kernel()
    torch.cuda.synchronize()
    k = timed(kernel, REPS, WINDOWS)
    c = timed(comp, 1, WINDOWS)
    k2 = timed(kernel, REPS, WINDOWS)          # again after the composition: the spread within one process
    nbytes = N * B * P * 12 + B * P * 12 + B * 4 + T * 4 + N * B * 4 * (T + 2)
    return {"P": P, "kernel_ms": {"median": k[0], "min": k[1], "max": k[2]}, "kernel_ms_second_pass": {"median": k2[0], "min": k2[1], "max": k2[2]},
            "composition_ms": {"median": c[0], "min": c[1], "max": c[2]}, "kernel_speedup": c[0] / k[0], "max_difference_to_kernel": diff,
            "kernel_bytes": nbytes, "kernel_tb_per_s": nbytes / (k[0] * 1e-3) / 1e12, "composition_comparison_bytes": float(N * B) * P * T,
            "auc_mean": float(auc.mean())}


def main():
    from mhentropy_amd import ops
    assert torch.cuda.is_available(), "bench_pck needs the GPU: there is no CPU path"
    rec = {"device": torch.cuda.get_device_name(0), "N": N, "B": B, "T": T, "reps": REPS, "windows": WINDOWS, "shapes": [one_shape(ops, P) for P in PS]}
    print(json.dumps(rec), flush=True)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
