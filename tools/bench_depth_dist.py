#!/usr/bin/env python3
"""Time of the depth distance (mhe_depth_dist_f32, mhe_depth_dist_bwd_f32, csrc/depth_dist.hip) at the metrics pass's shape: N = 200, B = 64,
V = 778, F = 1,538, S = 64, fitted offset.  Not the product path; nothing is asserted beyond agreement of the two forwards.

Three forms: the fused forward; forward + reverse; and what the forward replaces, a torch composition of ops.render_mesh(want=('depth',)) -
which writes N B depth images - with elementwise ops and reductions over them.  Device-event time per call, median of WINDOWS windows of REPS
calls (min-max beside it) after a warm-up of every form; the device is named.  The mesh is tools/render_bench.py's hand-sized folded sheet with
a jitter and a camera per hypothesis; the observation is the depth of the unjittered sheet under a mean camera plus noise and sensor holes.

    python tools/bench_depth_dist.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

N, B, V, F, S, TRUNC = 200, 64, 778, 1538, 64, 0.05
REPS, WINDOWS = int(os.environ.get("REPS", 5)), int(os.environ.get("WINDOWS", 7))
LDS_BYTES, WG_PER_CU = 62728, 2          # of either kernel (the compiler's resource report), 160 KiB of LDS per CU


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


def main():
    from mhentropy_amd import ops
    from render_bench import mesh
    assert torch.cuda.is_available(), "bench_depth_dist needs the GPU: there is no CPU path"
    print(f"device {torch.cuda.get_device_name(0)}; REPS {REPS}, WINDOWS {WINDOWS}; times are ms per call: median (min-max)")
    sheet, faces = mesh()
    sheet, faces = torch.as_tensor(sheet.astype(np.float32)).cuda(), torch.as_tensor(faces.astype(np.int32)).cuda().contiguous()
    assert tuple(sheet.shape) == (V, 3) and tuple(faces.shape) == (F, 3)
    g = torch.Generator(device="cuda").manual_seed(N)
    verts = (sheet[None, None] + 0.01 * torch.randn(N, B, V, 3, device="cuda", generator=g)).contiguous()
    logs_t = torch.cat([torch.log(0.9 + 0.2 * torch.rand(N, B, 1, device="cuda", generator=g)),
                        0.1 * torch.rand(N, B, 2, device="cuda", generator=g) - 0.05], -1).contiguous()
    zscale = (0.07 + 0.03 * torch.rand(B, device="cuda", generator=g)).contiguous()
    gd = torch.rand(N, B, device="cuda", generator=g) + 0.5
    one = torch.ones(B, device="cuda")
    truth = ops.render_mesh(sheet[None].expand(B, V, 3).contiguous(), faces, one, torch.zeros(B, 2, device="cuda"), zscale=zscale * 1000.0, size=S,
                            anti_aliasing=False, far=0.0, want=("mask", "depth"))
    mask = truth["mask"] > 0
    depth = torch.where(mask & (torch.rand(B, S, S, device="cuda", generator=g) > 0.05),
                        truth["depth"] + 0.5 + 0.01 * torch.randn(B, S, S, device="cuda", generator=g), torch.zeros(B, S, S, device="cuda"))
    obs = ops.depth_obs(depth, mask, S)
    adjacency = ops.face_adjacency(faces, V)
    rows_zs = (zscale * 1000.0)[None].expand(N, B).reshape(-1).contiguous()

    def composed():
        lt = logs_t.view(N * B, 3)
        R = ops.render_mesh(verts.view(N * B, V, 3), faces, lt[:, 0].exp().contiguous(), lt[:, 1:].contiguous(), zscale=rows_zs, size=S,
                            anti_aliasing=False, far=1e9, want=("depth",))["depth"].view(N, B, S, S)
        valid = obs > 0
        P = (R < 1e8) & valid
        nO, nP = valid.sum((1, 2)).float(), P.sum((2, 3)).float()
        off = (torch.where(P, obs - R, torch.zeros_like(R))).sum((2, 3)) / nP.clamp_min(1)
        t = (R + off[..., None, None] - obs).abs().clamp_max(TRUNC)
        return (torch.where(P, t, torch.zeros_like(t)).sum((2, 3)) + TRUNC * (nO - nP)) / nO.clamp_min(1)

    forms = (("forward", lambda: ops.depth_dist(verts, faces, logs_t, zscale, obs, None, TRUNC)),
             ("forward + reverse", lambda: (ops.depth_dist(verts, faces, logs_t, zscale, obs, None, TRUNC),
                                            ops.depth_dist_bwd(verts, faces, logs_t, zscale, obs, None, TRUNC, gd, adjacency=adjacency))),
             ("torch composition of render_mesh's depth", composed))
    for _ in range(2):
        for _, fn in forms:
            fn()
    torch.cuda.synchronize()
    dist, parts = ops.depth_dist(verts, faces, logs_t, zscale, obs, None, TRUNC)
    dev = float((dist - composed()).abs().max())
    print(f"N={N} B={B} V={V} F={F} S={S}: mean dist {float(dist.mean()):.5f} m, overlap {float(parts[..., 0].mean()):.3f}, inliers "
          f"{float(parts[..., 2].mean()):.3f}; max |fused - composed| = {dev:.2e} m (the composition's camera scale is exp in f32)")
    res = {"device": torch.cuda.get_device_name(0), "N": N, "B": B, "V": V, "F": F, "S": S, "reps": REPS, "windows": WINDOWS,
           "lds_bytes_per_workgroup": LDS_BYTES, "workgroups_per_cu": WG_PER_CU, "max_abs_dev_fused_vs_composed_m": dev, "rows": []}
    for name, fn in forms:
        med, lo, hi = timed(fn)
        res["rows"].append({"form": name, "ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)})
        print(f"  {name:42s} {med:.4f} ({lo:.4f}-{hi:.4f})", flush=True)
    res["composition_over_fused_forward"] = round(res["rows"][2]["ms"] / res["rows"][0]["ms"], 3)
    print(f"  the composition takes {res['composition_over_fused_forward']} x the fused forward's time")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
