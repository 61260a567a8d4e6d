#!/usr/bin/env python3
"""What the occluder costs the silhouette term (get_loss(sil_w=..., sil_occluder=True)): the longer mesh -> mask scan and the two-mask
list kernel.  Not the product path; nothing is asserted.  Shapes, inputs and timing scheme are those of tools/sil_train_bench.py; the
occluder is synth.object_masks' over the same hand masks (the covered pixels leave the hand mask), and both forms read THOSE hand masks:
occluder off against on, same process, interleaved windows.

(a) Kernels at N = 64, B = 256, V = 778, S = 64: the pixel list from one mask and from two, the plain forward and the fused forward +
    reverse without and with the list's occluder section.
(b) Train step: TrainStep.step at config C2 (B = 256, K = 64, ResNet-50, bf16), eager, sil_w = 1, sil_occluder off against on.

    python tools/sil_occ_bench.py [out.json]
Not measured here: a second box, hardware counters."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from sil_train_bench import N, B, V, S, REPS, WINDOWS, STEPS, TRAIN_WINDOWS, interleaved


def _ms(t):
    return {k: {"median": round(v[0], 4), "min": round(v[1], 4), "max": round(v[2], 4)} for k, v in t.items()}


def kernels(res):
    from mhentropy_amd import ops, synth
    from bench_silhouette import pipeline_masks
    from render_bench import mesh
    sheet = torch.as_tensor(mesh()[0]).cuda()
    hand, obj = (torch.as_tensor(m).cuda() for m in synth.object_masks(0, pipeline_masks(B).cpu().numpy() != 0))
    g = torch.Generator(device="cuda").manual_seed(N)
    verts = (sheet[None, None] + 0.01 * torch.randn(N, B, V, 3, device="cuda", generator=g)).contiguous()
    logs_t = torch.cat([torch.log(0.5 + 0.3 * torch.rand(N, B, 1, device="cuda", generator=g)),
                        0.3 * torch.rand(N, B, 2, device="cuda", generator=g) - 0.15], -1).contiguous()
    gd = torch.rand(N, B, device="cuda", generator=g) + 0.5
    pixels, count = ops.silhouette_pixels(hand, S)
    p2, c2, call = ops.silhouette_pixels(hand, S, obj)
    forms = (("pixel list, one mask", lambda: ops.silhouette_pixels(hand, S)),
             ("pixel list, two masks", lambda: ops.silhouette_pixels(hand, S, obj)),
             ("forward, occluder off", lambda: ops.silhouette_dist(verts, logs_t, pixels, count)),
             ("forward, occluder on", lambda: ops.silhouette_dist(verts, logs_t, p2, c2, count_all=call)),
             ("fused (dist_grad), occluder off", lambda: ops.silhouette_dist_grad(verts, logs_t, pixels, count, gd)),
             ("fused (dist_grad), occluder on", lambda: ops.silhouette_dist_grad(verts, logs_t, p2, c2, gd, count_all=call)))
    for _ in range(2):
        for _, fn in forms:
            fn()
    torch.cuda.synchronize()
    t = interleaved(forms, REPS, WINDOWS)
    kept, both = float(count.float().mean()), float(call.float().mean())
    print(f"(a) N={N} B={B} V={V} S={S}, mean |M_b| = {kept:.1f}, mean |M_b| + |O_b| = {both:.1f}; ms per call: median [min, max]")
    for name, _ in forms:
        med, lo, hi = t[name]
        print(f"  {name:34s} {med:.4f} [{lo:.4f}, {hi:.4f}]", flush=True)
    res["kernels"] = {"N": N, "B": B, "V": V, "S": S, "reps": REPS, "windows": WINDOWS, "mean_hand_pixels": round(kept, 1),
                      "mean_hand_and_occluder_pixels": round(both, 1), "ms": _ms(t),
                      "ratio_fused_on_over_off": round(t["fused (dist_grad), occluder on"][0] / t["fused (dist_grad), occluder off"][0], 4),
                      "ratio_forward_on_over_off": round(t["forward, occluder on"][0] / t["forward, occluder off"][0], 4)}
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
    y["hand_mask"], y["object_mask"] = (torch.as_tensor(m).cuda() for m in synth.object_masks(0, y["hand_mask"].cpu().numpy() != 0))
    noise = torch.as_tensor(synth.noise(0, N * B)).cuda()
    ts = TrainStep(model)
    forms = tuple((f"sil_occluder={o}", (lambda o=o: ts.step(x, y, noise=noise, N=N, sil_w=1.0, sil_occluder=o))) for o in (False, True))
    for _, fn in forms:
        out = fn()
    torch.cuda.synchronize()
    print(f"(b) warm-up: loss {float(out['total']):.4f}, silhouette {float(out['silhouette'].mean()):.4f}", flush=True)
    t = interleaved(forms, STEPS, TRAIN_WINDOWS)
    for name, _ in forms:
        med, lo, hi = t[name]
        print(f"  train step C2 B={B} K={N} bf16 eager, sil_w=1, {name}: {med:.2f} ms/step [{lo:.2f}, {hi:.2f}]", flush=True)
    res["train_step"] = {"config": "C2: ResNet-50, bf16, B=256, K=64, eager, sil_w=1, input pipeline's batch with synth.object_masks' occluder",
                         "steps": STEPS, "windows": TRAIN_WINDOWS, "ms": _ms(t),
                         "ratio_on_over_off": round(t["sil_occluder=True"][0] / t["sil_occluder=False"][0], 4)}


def main():
    assert torch.cuda.is_available(), "sil_occ_bench needs the GPU: there is no CPU path"
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
