#!/usr/bin/env python3
"""Time of the silhouette distance (mhe_silhouette_pixels, mhe_silhouette_dist_f32, mhe_silhouette_dist_bwd_f32, csrc/silhouette.hip) at the
metrics pass's shape (N = 200, B = 256) and at the loss pass's (N = 64, B = 256): V = 778, S = 64, the hand masks of the GPU input pipeline on
its synthetic decoded samples (256 x 256, box-averaged to 64 x 64 by the pixel-list kernel).  Not the product path; nothing is asserted.

Per shape: device-event time per call, median of WINDOWS windows of REPS calls (min-max beside it) after a warm-up of every form; the pixel
list; the forward with and without the argmin buffers; the reverse.  The forward evaluates R V mean|M_b| vertex-pixel pairs once per direction
(R = N B rows): about 9 vector instructions a pair towards the mask (2 subtractions with |.|, 2 maxima, a product, a fused multiply-add, a minimum
- or a compare and two selects with the argmins) and 5 towards the mesh; the bound is the f32 vector issue rate, 256 CUs x 128 lanes x 2.4 GHz =
78.6e12 lane-instructions/s.  The bytes (vertices read, argmins written) are printed beside it: nowhere near the HBM bound.  The vertices are a
hand-sized sheet (tools/render_bench.py's) with a jitter and a camera per hypothesis.

    python tools/bench_silhouette.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SHAPES = ((200, 256), (64, 256))          # (N, B): the metrics pass, the loss pass
V, S = 778, 64
REPS, WINDOWS = int(os.environ.get("REPS", 10)), int(os.environ.get("WINDOWS", 7))
VALU_RATE = 256 * 128 * 2.4e9
INSTR_PER_PAIR = 9 + 5


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


def pipeline_masks(B):
    from mhentropy_amd import ho3d_dataloader as hd, synth
    pool = [synth.ho3d_sample(i, ((i * 37) % 400 - 200, (i * 53) % 300 - 150)) for i in range(8)]
    rng = np.random.RandomState(0)
    raw = hd.collate_decoded([pool[i] for i in rng.randint(0, len(pool), B)])
    _, y = hd.HO3DBatchPipeline()(raw, aug=hd.draw_aug(B, rng))
    return y["hand_mask"]


def main():
    from mhentropy_amd import ops
    from render_bench import mesh
    assert torch.cuda.is_available(), "bench_silhouette needs the GPU: there is no CPU path"
    print(f"device {torch.cuda.get_device_name(0)}; REPS {REPS}, WINDOWS {WINDOWS}; times are ms per call: median (min-max)")
    sheet = torch.as_tensor(mesh()[0]).cuda()
    res = {"V": V, "S": S, "reps": REPS, "windows": WINDOWS, "rows": []}
    for N, B in SHAPES:
        mask = pipeline_masks(B)
        g = torch.Generator(device="cuda").manual_seed(N)
        verts = (sheet[None, None] + 0.01 * torch.randn(N, B, V, 3, device="cuda", generator=g)).contiguous()
        logs_t = torch.cat([torch.log(0.5 + 0.3 * torch.rand(N, B, 1, device="cuda", generator=g)),
                            0.3 * torch.rand(N, B, 2, device="cuda", generator=g) - 0.15], -1).contiguous()
        gd = torch.rand(N, B, device="cuda", generator=g) + 0.5
        pixels, count = ops.silhouette_pixels(mask, S)
        dist, parts, iv, im = ops.silhouette_dist(verts, logs_t, pixels, count, want_idx=True)
        forms = (("pixel list", lambda: ops.silhouette_pixels(mask, S), mask.numel() * mask.element_size() + B * S * S * 4, False),
                 ("forward", lambda: ops.silhouette_dist(verts, logs_t, pixels, count), N * B * (V * 12 + 24), True),
                 ("forward + argmins", lambda: ops.silhouette_dist(verts, logs_t, pixels, count, want_idx=True), N * B * (V * 16 + S * S * 4 + 24), True),
                 ("reverse", lambda: ops.silhouette_dist_bwd(verts, logs_t, pixels, count, iv, im, gd), N * B * (V * 28 + 24) + int(count.sum()) * N * 4, False))
        for _ in range(2):
            for _, fn, _, _ in forms:
                fn()
        torch.cuda.synchronize()
        mean_m = float(count.float().mean())
        pairs = float(N) * B * V * mean_m
        print(f"N={N} B={B} V={V} S={S}: mean |M_b| = {mean_m:.1f} kept pixels (min {int(count.min())}, max {int(count.max())}); R V mean|M_b| = {pairs:.3e} "
              f"pairs per direction; mean dist {float(dist.mean()):.4f} (inside {float(parts[..., 0].mean()):.4f}, cover {float(parts[..., 1].mean()):.4f})")
        for name, fn, nb, valu in forms:
            med, lo, hi = timed(fn)
            row = {"N": N, "B": B, "form": name, "ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4), "bytes": nb, "pairs_per_direction": pairs,
                   "mean_kept_pixels": round(mean_m, 1)}
            line = f"  {name:18s} {med:.4f} ({lo:.4f}-{hi:.4f})  {nb / 1e6:.1f} MB = {nb / (med * 1e-3) / 1e12:.3f} TB/s"
            if valu:
                row["valu_fraction"] = round(INSTR_PER_PAIR * pairs / (med * 1e-3) / VALU_RATE, 4)
                line += f"  {row['valu_fraction'] * 100:.1f} % of the f32 vector issue rate at {INSTR_PER_PAIR} instructions a pair of both directions"
            res["rows"].append(row)
            print(line, flush=True)
        del verts, iv, im
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
