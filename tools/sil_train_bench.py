#!/usr/bin/env python3
"""What the silhouette training term costs (get_loss(sil_w=...)).  Not the product path; nothing is asserted.

(a) Kernels, same process, interleaved windows: mhe_silhouette_dist_grad_f32 (forward and reverse of a row in one launch, the argmins in
    registers and LDS) against the two launches it replaces, mhe_silhouette_dist_f32 with idx_v / idx_m + mhe_silhouette_dist_bwd_f32, at
    the loss pass's shape N = 64, B = 256, V = 778, S = 64 with the hand masks of the GPU input pipeline (tools/bench_silhouette.py's
    inputs).  Device-event time per call, median of WINDOWS (7) windows of REPS (10) calls with [min, max]; the plain forward beside them.
(b) Train step: TrainStep.step at config C2 (B = 256, K = 64, ResNet-50, bf16), eager, fed by the input pipeline, sil_w = 1 against
    sil_w = 0, alternating windows of STEPS (3) steps, median of TRAIN_WINDOWS (5) with [min, max] (tools/chamfer_train_bench.py's scheme).

    python tools/sil_train_bench.py [out.json]
Not measured here: a second box, hardware counters."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

N, B, V, S = 64, 256, 778, 64
REPS, WINDOWS = int(os.environ.get("REPS", 10)), int(os.environ.get("WINDOWS", 7))
STEPS, TRAIN_WINDOWS = int(os.environ.get("STEPS", 3)), int(os.environ.get("TRAIN_WINDOWS", 5))


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(forms, reps, windows):
    """name -> (median, min, max) ms per call; the forms take turns window by window, so a drift of the box touches all of them alike"""
    times = {name: [] for name, _ in forms}
    for _ in range(windows):
        for name, fn in forms:
            times[name].append(window(fn, reps))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}


def kernels(res):
    from mhentropy_amd import ops
    from bench_silhouette import pipeline_masks
    from render_bench import mesh
    sheet = torch.as_tensor(mesh()[0]).cuda()
    mask = pipeline_masks(B)
    g = torch.Generator(device="cuda").manual_seed(N)
    verts = (sheet[None, None] + 0.01 * torch.randn(N, B, V, 3, device="cuda", generator=g)).contiguous()
    logs_t = torch.cat([torch.log(0.5 + 0.3 * torch.rand(N, B, 1, device="cuda", generator=g)),
                        0.3 * torch.rand(N, B, 2, device="cuda", generator=g) - 0.15], -1).contiguous()
    gd = torch.rand(N, B, device="cuda", generator=g) + 0.5
    pixels, count = ops.silhouette_pixels(mask, S)

    def two_launches():
        _, _, iv, im = ops.silhouette_dist(verts, logs_t, pixels, count, want_idx=True)
        return ops.silhouette_dist_bwd(verts, logs_t, pixels, count, iv, im, gd)
    forms = (("forward", lambda: ops.silhouette_dist(verts, logs_t, pixels, count)),
             ("two launches (dist<IDX> + dist_bwd)", two_launches),
             ("fused (dist_grad)", lambda: ops.silhouette_dist_grad(verts, logs_t, pixels, count, gd)),
             ("fused (dist_grad, with dist)", lambda: ops.silhouette_dist_grad(verts, logs_t, pixels, count, gd, want_dist=True)))
    a, b = two_launches(), ops.silhouette_dist_grad(verts, logs_t, pixels, count, gd)
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    for _ in range(2):
        for _, fn in forms:
            fn()
    torch.cuda.synchronize()
    t = interleaved(forms, REPS, WINDOWS)
    print(f"(a) N={N} B={B} V={V} S={S}, mean |M_b| = {float(count.float().mean()):.1f}; gradients bit-equal: {same}; ms per call: median [min, max]")
    for name, _ in forms:
        med, lo, hi = t[name]
        print(f"  {name:38s} {med:.4f} [{lo:.4f}, {hi:.4f}]", flush=True)
    res["kernels"] = {"N": N, "B": B, "V": V, "S": S, "reps": REPS, "windows": WINDOWS, "mean_kept_pixels": round(float(count.float().mean()), 1),
                      "gradients_bit_equal": same, "index_bytes_not_written": N * B * (V + S * S) * 4,
                      "ms": {k: {"median": round(v[0], 4), "min": round(v[1], 4), "max": round(v[2], 4)} for k, v in t.items()}}
    del verts
    torch.cuda.empty_cache()


def train_step(res):
    from mhentropy_amd import harness, ho3d_dataloader as hd, synth
    from mhentropy_amd.train import TrainStep
    model = harness.build_mhent(backbone="resnet50", h_dims=(512, 512), num_steps=6, tables=synth.mano_tables(0),
                                compute_dtype=torch.bfloat16).cuda().train()
    pool = [synth.ho3d_sample(i, ((i * 37) % 400 - 200, (i * 53) % 300 - 150)) for i in range(8)]
    rng = np.random.RandomState(0)
    raw = hd.collate_decoded([pool[i] for i in rng.randint(0, len(pool), B)])
    x, y = hd.HO3DBatchPipeline()(raw, aug=hd.draw_aug(B, rng))
    noise = torch.as_tensor(synth.noise(0, N * B)).cuda()
    ts = TrainStep(model)
    forms = tuple((f"sil_w={w:g}", (lambda w=w: ts.step(x, y, noise=noise, N=N, sil_w=w))) for w in (0.0, 1.0))
    for _, fn in forms:
        out = fn()
    torch.cuda.synchronize()
    print(f"(b) warm-up: loss {float(out['total']):.4f}, silhouette {float(out['silhouette'].mean()):.4f}", flush=True)
    t = interleaved(forms, STEPS, TRAIN_WINDOWS)
    for name, _ in forms:
        med, lo, hi = t[name]
        print(f"  train step C2 B={B} K={N} bf16 eager, {name}: {med:.2f} ms/step [{lo:.2f}, {hi:.2f}]", flush=True)
    res["train_step"] = {"config": "C2: ResNet-50, bf16, B=256, K=64, eager, input pipeline", "steps": STEPS, "windows": TRAIN_WINDOWS,
                         "ms": {k: {"median": round(v[0], 3), "min": round(v[1], 3), "max": round(v[2], 3)} for k, v in t.items()}}


def main():
    assert torch.cuda.is_available(), "sil_train_bench needs the GPU: there is no CPU path"
    res = {"device": torch.cuda.get_device_name(0), "not_measured": ["a second box", "hardware counters"]}
    kernels(res)
    train_step(res)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
