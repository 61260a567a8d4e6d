#!/usr/bin/env python3
"""Time of the hand mesh evaluation (mhe_mesh_eval_f32, csrc/mesh_eval.hip) at the reference iteration's evaluation shape, N = 200 hypotheses of
B = 64 images, V = 778 vertices, T = 2 thresholds, next to the only route that exists without it: torch.cdist over chunks of rows ((rows, 778, 778)
distances through HBM), two minima and two compares per chunk, on the same device.  Not the product path.  The composition is run in two forms:
the exact differences (compute_mode donot_use_mm_for_euclid_dist) in chunks of 16 rows - at 64 rows and more that form returned wrong distances
here (rows of ones and of other rows' values: 64 x 778 x 778 one-thread-per-pair launches pass 2^32 threads), which is why every form is compared
with the kernel first and one that disagrees is reported as invalid, not timed - and the matrix-multiply form in chunks of 512 rows.

Device-event time per call, median of WINDOWS windows of REPS calls after a warm-up; min and max of the windows beside it.  The kernel evaluates
2 N B V^2 point pairs (once per direction) at 7 vector instructions a pair (3 subtractions, a product, 2 fused multiply-adds, a minimum): the bound is
the f32 vector issue rate, 256 CUs x 128 lanes x 2.4 GHz = 78.6e12 lane-instructions/s; its bytes (meshes in, 1 + 3 T floats a row out) are printed
beside it.  The composition's outputs are compared with the kernel's before anything is timed.

    python tools/bench_mesh_eval.py [--json out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

N, B, V, THR = int(os.environ.get("N", 200)), int(os.environ.get("B", 64)), int(os.environ.get("V", 778)), (5.0, 15.0)
REPS, WINDOWS = int(os.environ.get("REPS", 10)), int(os.environ.get("WINDOWS", 7))
FORMS = (("cdist_exact_16_rows", "donot_use_mm_for_euclid_dist", 16), ("cdist_matmul_512_rows", "use_mm_for_euclid_dist", 512))
VALU_RATE = 256 * 128 * 2.4e9


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


def cdist_composition(pred, target, scale, thr, unit=1000.0, chunk=16, mode="donot_use_mm_for_euclid_dist"):
    """the same outputs by torch.cdist, `chunk` rows at a time (row r = n B + b)"""
    n, b, v = pred.shape[:3]
    su = (scale * unit)[None, :, None, None]
    P = (pred * su).view(n * b, v, 3)
    G = (target[None] * su).expand(n, b, v, 3).reshape(n * b, v, 3)
    th = torch.tensor(thr, device=pred.device)[:, None, None]
    err = (P - G).norm(dim=-1).mean(-1).view(n, b)
    prec, rec = torch.empty(len(thr), n * b, device=pred.device), torch.empty(len(thr), n * b, device=pred.device)
    for r0 in range(0, n * b, chunk):
        D = torch.cdist(P[r0:r0 + chunk], G[r0:r0 + chunk], compute_mode=mode)
        prec[:, r0:r0 + chunk] = (D.min(2).values[None] < th).float().mean(-1)
        rec[:, r0:r0 + chunk] = (D.min(1).values[None] < th).float().mean(-1)
    f = torch.where(prec + rec > 0, 2 * prec * rec / (prec + rec).clamp_min(1e-30), torch.zeros_like(prec))
    return err, torch.stack([prec, rec, f]).view(3, len(thr), n, b)


def main():
    from mhentropy_amd import ops
    assert torch.cuda.is_available(), "bench_mesh_eval needs the GPU: there is no CPU path"
    g = torch.Generator().manual_seed(N + B + V)
    target = torch.randn(B, V, 3, generator=g)
    pred = (target[None] + 0.15 * torch.randn(N, B, V, 3, generator=g)).cuda()
    target, scale = target.cuda(), (0.025 + 0.015 * torch.rand(B, generator=g)).cuda()
    err, prf = ops.mesh_eval(pred, target, scale, THR)
    for _ in range(3):
        ops.mesh_eval(pred, target, scale, THR)
    torch.cuda.synchronize()
    k = timed(lambda: ops.mesh_eval(pred, target, scale, THR), REPS, WINDOWS)
    forms = {}
    for name, mode, chunk in FORMS:
        fn = lambda: cdist_composition(pred, target, scale, THR, chunk=chunk, mode=mode)
        err_t, prf_t = fn()
        diff = {"err_rel": float(((err - err_t).abs() / err_t).max()), "precision_recall_abs": float((prf[:2] - prf_t[:2]).abs().max()),
                "f_abs": float((prf[2] - prf_t[2]).abs().max())}
        valid = diff["err_rel"] < 1e-4 and diff["precision_recall_abs"] < 0.02          # a handful of the 778 vertices may sit on a threshold in f32
        forms[name] = {"chunk_rows": chunk, "compute_mode": mode, "valid": valid, "max_difference_to_kernel": diff}
        if valid:
            torch.cuda.synchronize()
            c = timed(fn, 1, WINDOWS)
            forms[name]["ms"] = {"median": c[0], "min": c[1], "max": c[2]}
            forms[name]["kernel_speedup"] = c[0] / k[0]
    k2 = timed(lambda: ops.mesh_eval(pred, target, scale, THR), REPS, WINDOWS)          # again after the compositions: the spread within one process
    pairs = 2.0 * N * B * V * V
    nbytes = N * B * V * 12 + B * V * 12 + N * B * 4 * (1 + 3 * len(THR))
    rec = {"device": torch.cuda.get_device_name(0), "N": N, "B": B, "V": V, "T": len(THR), "reps": REPS, "windows": WINDOWS,
           "kernel_ms": {"median": k[0], "min": k[1], "max": k[2]}, "kernel_ms_second_pass": {"median": k2[0], "min": k2[1], "max": k2[2]},
           "compositions": forms, "pair_evaluations": pairs, "kernel_share_of_f32_vector_issue_rate": 7 * pairs / (k[0] * 1e-3) / VALU_RATE,
           "kernel_bytes": nbytes, "kernel_tb_per_s": nbytes / (k[0] * 1e-3) / 1e12, "composition_distance_bytes": float(N * B) * V * V * 4}
    print(json.dumps(rec), flush=True)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
