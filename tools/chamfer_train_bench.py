#!/usr/bin/env python3
"""Wall time of TrainStep.step at config C2 (B = 256, K = 64, ResNet-50, bf16) with the hand-object Chamfer term at weight W (0 = off), fed by
the GPU input pipeline's object targets (NOBJ-vertex objects, object_count = the decoded samples' obj_count):
    python tools/chamfer_train_bench.py 10        and        python tools/chamfer_train_bench.py 0
One warm-up step, then the median of WINDOWS (5) windows of STEPS (3) eager steps each, device-event time per step [min, max]."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mhentropy_amd import harness, ho3d_dataloader as hd, synth
from mhentropy_amd.train import TrainStep

W = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
B, K, NOBJ = int(os.environ.get("B", 256)), int(os.environ.get("K", 64)), int(os.environ.get("NOBJ", 1000))
WINDOWS, STEPS = int(os.environ.get("WINDOWS", 5)), int(os.environ.get("STEPS", 3))
model = harness.build_mhent(backbone="resnet50", h_dims=(512, 512), num_steps=6, tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
pool = [synth.ho3d_sample(i, ((i * 37) % 400 - 200, (i * 53) % 300 - 150), n_obj=NOBJ) for i in range(8)]
rng = np.random.RandomState(0)
raw = hd.collate_decoded([pool[i] for i in rng.randint(0, len(pool), B)])
x, y = hd.HO3DBatchPipeline()(raw, aug=hd.draw_aug(B, rng))
y["object_count"] = raw["obj_count"]
noise = torch.as_tensor(synth.noise(0, K * B)).cuda()
ts = TrainStep(model)
out = ts.step(x, y, noise=noise, N=K, chamfer_w=W)
torch.cuda.synchronize()
print("warm-up loss", float(out["total"]), "chamfer" if "chamfer" in out else "", float(out["chamfer"].mean()) if "chamfer" in out else "", flush=True)
times = []
for _ in range(WINDOWS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        out = ts.step(x, y, noise=noise, N=K, chamfer_w=W)
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / STEPS)
print(f"train step C2 B={B} K={K} bf16, VO={y['object_verts'].shape[1] // 3}, chamfer_w={W:g}: median of {WINDOWS} windows of {STEPS} steps "
      f"{np.median(times):.2f} ms/step [{min(times):.2f}, {max(times):.2f}]  loss {float(out['total']):.4f}", flush=True)
