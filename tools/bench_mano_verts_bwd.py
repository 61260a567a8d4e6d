#!/usr/bin/env python3
"""Time of the hand-mesh reverse (mhe_mano_verts_bwd_f32: pose pass, table transposition, the two skinning-reverse kernels of
csrc/mano_skin_bwd.hip, the pose chain's reverse of csrc/mano_bwd.hip) alone and behind its forward (mhe_mano_verts_f32), at R = 16,384 (the C2
train shape, 256 images x 64 hypotheses) and R = 51,200 (the metrics pass).  Not the product path; nothing is asserted: there is no earlier
version and no reference on the GPU to compare with.

Per shape: device-event time per call, median of WINDOWS windows of REPS calls (min-max beside it) after a warm-up of every form.  The bytes are
the algorithm's: z, g_verts and g_z once, the forward's verts once more.  The matrix-core work is the exact-f32 MFMA count of the two skinning
kernels per 32 hypotheses x 32 vertices: 219 + 72 + 240 (blend product, transform rotation, coefficient reduction) + 192 (transform reduction).

    python tools/bench_mano_verts_bwd.py [out.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SHAPES = (16384, 51200)
REPS, WINDOWS = int(os.environ.get("REPS", 10)), int(os.environ.get("WINDOWS", 7))
MFMA_PER_TILE = 219 + 72 + 240 + 192          # v_mfma_f32_32x32x2_f32 per (32 hypotheses, 32 vertices), 4096 flop each
F32_MFMA_RATE = 256 * 4 * 64 * 2.4e9          # flop/s: 64 flop per clock and SIMD


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
    from mhentropy_amd import mano_pack, ops, synth
    assert torch.cuda.is_available(), "bench_mano_verts_bwd needs the GPU: there is no CPU path"
    print(f"device {torch.cuda.get_device_name(0)}; REPS {REPS}, WINDOWS {WINDOWS}; times are ms per call: median (min-max)")
    t = synth.mano_tables(0)
    blob = torch.from_numpy(mano_pack.pack_tables(t["shapedirs"], t["posedirs"], t["v_template"], t["J_regressor"], t["weights"],
                                                  t["hands_components"][:45], t["hands_mean"])).cuda()
    res = {"reps": REPS, "windows": WINDOWS, "note": "first timing, not tuned", "rows": []}
    for R in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(R)
        z = torch.randn(R, 61, device="cuda", generator=g)
        z[:, 3:48] *= 0.5
        z[:, 48:58] *= 0.03
        g_verts = torch.randn(R, 778, 3, device="cuda", generator=g)
        flop = (R + 31) // 32 * 25 * MFMA_PER_TILE * 4096
        forms = (("reverse", lambda: ops.mano_verts_bwd(z, blob, g_verts), R * (778 * 12 + 2 * 61 * 4)),
                 ("reverse, mm", lambda: ops.mano_verts_bwd(z, blob, g_verts, mm=True), R * (778 * 12 + 2 * 61 * 4)),
                 ("forward", lambda: ops.mano_verts(z, blob), R * (778 * 12 + 61 * 4)),
                 ("forward + reverse", lambda: (ops.mano_verts(z, blob), ops.mano_verts_bwd(z, blob, g_verts)), R * (2 * 778 * 12 + 3 * 61 * 4)))
        for _ in range(2):
            for _, fn, _ in forms:
                fn()
        torch.cuda.synchronize()
        print(f"R={R}: {flop / 1e9:.1f} Gflop of exact-f32 matrix-core work in the skinning reverse")
        for name, fn, nb in forms:
            med, lo, hi = timed(fn)
            row = {"R": R, "form": name, "ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4), "bytes": nb}
            line = f"  {name:18s} {med:.4f} ({lo:.4f}-{hi:.4f})  {nb / 1e6:.1f} MB = {nb / (med * 1e-3) / 1e12:.3f} TB/s"
            if name.startswith("reverse"):
                row["f32_mfma_fraction"] = round(flop / (med * 1e-3) / F32_MFMA_RATE, 4)
                line += f"  {row['f32_mfma_fraction'] * 100:.1f} % of the f32 matrix-core rate (the whole call over the skinning reverse's flop)"
            res["rows"].append(row)
            print(line, flush=True)
        del g_verts
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
