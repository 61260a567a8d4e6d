#!/usr/bin/env python3
"""Time mhe_render_mesh_f32 (csrc/render.hip) at the metrics pass's sizes: R = 16,384 and R = 51,200 hypotheses, V = 778, F = 1,538, a
64 x 64 anti-aliased image - the mask-writing form and the score-only form (criteria.silhouette_iou's).  Beside each time the bytes that form
has to move (vertices read, 9.3 KB a hypothesis; the mask written, 16 KB a hypothesis) and that traffic as a fraction of HBM_PEAK.
The mesh is a closed-surface-like sheet of MANO's counts (a 28 x 28 grid folded over itself cut to 778 vertices plus faces up to 1,538), each
hypothesis its own jitter and camera, the hand filling about a third of the crop.  Nothing is asserted.
    python tools/render_bench.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mhentropy_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X
V, F, S = 778, 1538, 64


def mesh(seed=0):
    """778 vertices of a 28 x 28 jittered grid folded along its middle (front and back of a hand-sized blob), 1,538 faces: the grid's own
    that stay inside the 778 vertices, the rest second-neighbour faces"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.linspace(-1, 1, 28), np.linspace(-1, 1, 28), indexing="ij")
    u = u + rng.uniform(-0.3, 0.3, u.shape) * (2 / 27)
    v = v + rng.uniform(-0.3, 0.3, v.shape) * (2 / 27)
    x, y = 0.45 * (2 * np.abs(u) - 1), 0.6 * v
    z = np.where(u < 0, 0.1 + 0.05 * np.cos(3 * x), -0.1 - 0.05 * np.cos(3 * x))
    verts = np.stack([x, y, z], -1).reshape(-1, 3)[:V]
    i, j = np.meshgrid(np.arange(27), np.arange(27), indexing="ij")
    b = (i * 28 + j).reshape(-1)
    f = np.concatenate([np.stack([b, b + 1, b + 28], 1), np.stack([b + 1, b + 29, b + 28], 1)])
    f = f[(f < V).all(1)]
    k = rng.integers(0, V - 60, F - len(f))
    f = np.concatenate([f, np.stack([k, k + 2, k + 56], 1)])
    assert f.shape == (F, 3) and f.max() < V
    return verts.astype(np.float32), f.astype(np.int32)


def timed(fn, iters=10):
    fn(); fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]))


def main():
    v1, faces = mesh()
    faces = torch.as_tensor(faces).cuda()
    res = {"V": V, "F": F, "S": S, "anti_aliasing": True, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": []}
    for R in (16384, 51200):
        g = torch.Generator(device="cuda").manual_seed(R)
        verts = torch.as_tensor(v1).cuda()[None] + 0.01 * torch.randn(R, V, 3, device="cuda", generator=g)
        scale = 0.8 + 0.4 * torch.rand(R, device="cuda", generator=g)
        trans = 0.4 * torch.rand(R, 2, device="cuda", generator=g) - 0.2
        B = 256
        target = (torch.rand(B, S, S, device="cuda", generator=g) < 0.3).float()
        covered = float(ops.render_mesh(verts[:64], faces, scale[:64], trans[:64], size=S)["mask"].mean())
        forms = {"mask": (lambda: ops.render_mesh(verts, faces, scale, trans, size=S, want=("mask",)), R * (V * 12 + S * S * 4)),
                 "mask+depth": (lambda: ops.render_mesh(verts, faces, scale, trans, size=S, want=("mask", "depth")), R * (V * 12 + 2 * S * S * 4)),
                 "score only": (lambda: ops.render_mesh(verts, faces, scale, trans, size=S, want=("iou_sums",), target=target), R * (V * 12 + 8) + B * S * S * 4)}
        for name, (fn, nbytes) in forms.items():
            ms = timed(fn)
            row = {"R": R, "form": name, "ms": round(ms, 4), "bytes": nbytes, "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4),
                   "us_per_hypothesis": round(ms * 1e3 / R, 4), "mean_coverage": round(covered, 3)}
            res["rows"].append(row)
            print(f"R = {R:6d}  {name:11s} {ms:8.3f} ms   {nbytes / 1e6:8.1f} MB to move ({nbytes / R / 1e3:.1f} KB/hyp)   {row['hbm_fraction']:.1%} of HBM peak", flush=True)
    line = json.dumps(res)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
