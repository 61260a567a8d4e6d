#!/usr/bin/env python3
"""Cost of the aligned evaluation (MHEntLoss(aligned=True), csrc/procrustes.hip) at the iteration's metrics-pass size.

  1. the kernels alone at N = 200, B = 256: the mesh alignment (verts [N,B,2334] -> metres), the joint alignment + the split metrics,
     and the unaligned metrics kernel - each launched REPS times; run under `rocprofv3 --kernel-trace --stats` for per-kernel times;
  2. the metrics pass of the reference's iteration (MHEnt.sample(N=[N,N], mods={uv,xyz,verts}) + MHEntLoss, from the conditioning
     feature on, C2 config) captured in a HIP graph, unaligned vs aligned, replays timed with device events, alternating;
  3. the host loop the reference runs instead (align_w_scale per (n, b) with scipy), timed on the CPU at a small N and extrapolated.

    rocprofv3 --kernel-trace --stats -d OUT -o a -- python3 tools/aligned_bench.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

B, N = int(os.environ.get("B", 256)), int(os.environ.get("N", 200))
REPS = int(os.environ.get("REPS", 20))


def host_loop_estimate():
    """the reference's loop (criteria.py:70-84 + utils.py:502-525) over n_small hypotheses of B images, extrapolated to N"""
    from scipy.linalg import orthogonal_procrustes
    rng = np.random.default_rng(0)
    n_small = 2
    res = {}
    for lbl, P in (("xyz", 21), ("verts", 778)):
        tgt = rng.normal(0, 0.03, (B, P, 3)).astype(np.float32) + np.float32(0.6)
        pred = rng.normal(0, 3, (n_small, B, P, 3)).astype(np.float32)
        t0 = time.perf_counter()
        for n in range(n_small):
            for b in range(B):
                m1, m2 = tgt[b].copy(), pred[n, b].copy()
                t1, t2 = m1.mean(0), m2.mean(0)
                m1, m2 = m1 - t1, m2 - t2
                s1, s2 = np.linalg.norm(m1) + 1e-8, np.linalg.norm(m2) + 1e-8
                m1 /= s1
                m2 /= s2
                R, s = orthogonal_procrustes(m1, m2)
                _ = np.dot(m2, R.T) * s * s1 + t1
        res[lbl] = (time.perf_counter() - t0) / (n_small * B) * N * B
    return res


def main():
    from mhentropy_amd import harness, ops, synth
    from mhentropy_amd.criteria import MHEntLoss
    rng = np.random.default_rng(1)
    dev = "cuda"
    # 1. the kernels alone
    tv = torch.as_tensor(rng.normal(0, 0.03, (B, 2334)).astype(np.float32) + np.float32(0.6), device=dev)
    pv = torch.as_tensor(rng.normal(0, 3, (N, B, 2334)).astype(np.float32), device=dev)
    tj = torch.as_tensor(rng.normal(0, 0.3, (B, 63)).astype(np.float32), device=dev)
    pj = torch.as_tensor(rng.normal(0, 1, (N, B, 63)).astype(np.float32), device=dev)
    uv = torch.as_tensor(rng.normal(128, 30, (N, B, 42)).astype(np.float32), device=dev)
    _, yn = synth.batch(0, B, with_image=False)
    y = {k: torch.as_tensor(v).to(dev) for k, v in yn.items()}
    args = (uv, tj, y["scale"], y["crop_uv"], y["vis"])
    for _ in range(3):
        ops.procrustes_align(pv, tv); ops.metrics_split(ops.procrustes_align(pj, tj), pj, *args); ops.metrics(pj, *args)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    for _ in range(REPS):
        ops.procrustes_align(pv, tv)
    ev[1].record()
    for _ in range(REPS):
        ops.metrics_split(ops.procrustes_align(pj, tj), pj, *args)
    ev[2].record()
    for _ in range(REPS):
        ops.metrics(pj, *args)
    ev[3].record()
    torch.cuda.synchronize()
    t = [ev[i].elapsed_time(ev[i + 1]) / REPS for i in range(3)]
    print(f"N={N} B={B} (event time per call, launches included): verts align {t[0] * 1e3:.1f} us "
          f"({N * B * 2334 * 4 * 2 / (t[0] * 1e-3) / 1e12:.2f} TB/s of compulsory traffic); joints align + split metrics {t[1] * 1e3:.1f} us; "
          f"unaligned metrics {t[2] * 1e3:.1f} us", flush=True)
    # 2. the graphed metrics pass, unaligned vs aligned
    model = harness.build_mhent(backbone="resnet50", tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).to(dev).eval()
    y["verts"] = tv
    feat = torch.randn(B, 512, device=dev) * 0.5
    model.feat_extractor.forward = lambda x: (feat, feat, None)
    lp = torch.zeros(B, device=dev)
    graphs = {}
    for name, crit in (("unaligned", MHEntLoss()), ("aligned", MHEntLoss(aligned=True))):
        def run(crit=crit):
            s = model.sample(None, N=[N, N], temp=0.8, mods={"uv", "xyz", "verts"}, y=y)
            s["log_p"] = lp
            return crit(s, y)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run()
        graphs[name] = g
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(5):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / 5)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(f"graphed metrics pass sample(N={N}) + MHEntLoss, B={B}: unaligned {med['unaligned']:.3f} ms, aligned {med['aligned']:.3f} ms "
          f"(+{med['aligned'] - med['unaligned']:.3f} ms; medians of 5 alternating windows of 5 replays; "
          f"spread {min(times['unaligned']):.3f}-{max(times['unaligned']):.3f} / {min(times['aligned']):.3f}-{max(times['aligned']):.3f})",
          flush=True)
    # 3. the reference's host loop
    h = host_loop_estimate()
    print(f"host loop (align_w_scale + scipy per row, this CPU, extrapolated from 2 hypotheses): xyz {h['xyz']:.1f} s, "
          f"verts {h['verts']:.1f} s per metrics pass at N={N} B={B}", flush=True)


if __name__ == "__main__":
    main()
