#!/usr/bin/env python3
"""Benchmark of the multi-hypothesis hot path (BASELINE.json metric):
hypotheses/sec (B x K) of forward + loss on synthetic 256x256 images.

A "step" is one pass of MHEnt.get_loss (ResNet-50 encoder -> 12-coupling RealNVP
-> MANO joints -> entropy + 2D re-projection ELBO) over one resident batch.
One process per GPU; images are sharded across ranks, no data-path collective
(weak scaling).  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times exactly --steps steps in one window and prints
the line.  --full adds everything else: the per-kernel roofline pass, the train-step
and iteration-with-metrics legs, the Glow variant, the CPU baseline, and the median
of --windows timed windows.  --dump-outputs DIR writes the last timed step's
outputs (the get_loss dict of rank 0) as DIR/<name>.npy.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

WORKLOADS = {
    # BASELINE.json configs[2] shape (the K=64 the metric is quoted on), forward + loss
    "c2": dict(B=256, K=64, backbone="resnet50", h=512, steps=6),
    # BASELINE.json configs[1]
    "c1": dict(B=64, K=16, backbone="resnet50", h=512, steps=6),
    # BASELINE.json configs[0] (CPU-runnable plumbing case)
    "c0": dict(B=2, K=4, backbone="resnet18", h=64, steps=2),
}
PMC_TRAFFIC = "r05_pmc_traffic.json"
PMC_TRAFFIC_TRAIN = "r05_train_pmc_traffic.json"
HBM_PEAK = 8.0e12               # MI355X_MICROARCH.md (spec); hand-written copy / read kernels reach 5.4-6.0 / 6.3e12 here (tools/probes/hbm_probe.hip)
PEAK = {"f32": 157.3e12, "bf16": 2.5e15}      # dense MFMA peaks, MI355X_MICROARCH.md "Chip-level parameters"
_T0 = time.time()


def log(msg):
    print(f"[bench +{time.time() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


def build_model(cfg, dtype, seed, flow="realnvp"):
    from mhentropy_amd import harness, synth
    cd = torch.float32 if dtype == "f32" else torch.bfloat16
    model = harness.build_mhent(backbone=cfg["backbone"], h_dims=(cfg["h"], cfg["h"]), num_steps=cfg["steps"],
                                tables=synth.mano_tables(0), compute_dtype=cd, flow=flow)
    feat_dim = 2048 if cfg["backbone"] == "resnet50" else 512
    if flow == "glow":
        sd = {"q_z_giv_i." + k: v for k, v in synth.glow_state(seed).items()}
    else:
        sd = {"q_z_giv_i." + k: v for k, v in synth.flow_state(seed, 45, 512, (cfg["h"], cfg["h"]), cfg["steps"]).items()}
    sd.update(synth.head_state(seed, feat_dim, 512, 16))
    sd.update({"feat_extractor.res." + k: v for k, v in synth.resnet_state(seed, cfg["backbone"]).items()})
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    return model, sd


def cpu_baseline(cfg, sd, seed, budget_s=150.0):
    """The oracle restatement (kind 'port') timed on this host's cores on the SAME workload as the GPU line (same networks, same
    B images x K hypotheses, train-mode BatchNorm over the whole batch): BASELINE.md section 3's protocol - two warm-up passes, then the
    median of five timed ones (~15 s each at C2) - cut short only if the passes run past the budget (the shortfall is stated in `sample`)."""
    from mhentropy_amd import synth
    from oracle import network_ref, mano_ref
    # the GPU box exposes every host CPU but a 1-GPU job owns a 16-core share: oversubscribing stalls torch's pool
    ncores = min(len(os.sched_getaffinity(0)), os.cpu_count() or 1, 16)
    torch.set_num_threads(ncores)
    Bs, K = cfg["B"], cfg["K"]
    sdt = {k: torch.as_tensor(v) for k, v in sd.items()}
    tb = mano_ref.tables_from_numpy(synth.mano_tables(0))
    x, yn = synth.batch(seed + 1, Bs, image_size=256)
    y = {k: torch.as_tensor(v) for k, v in yn.items()}
    z0 = torch.as_tensor(synth.noise(seed + 1, K * Bs))
    xt = torch.as_tensor(x)
    times = []
    t_start = time.time()
    WARM, TIMED = 2, 5
    with torch.no_grad():
        for i in range(WARM + TIMED):
            t0 = time.time()
            network_ref.get_loss(sdt, tb, xt, y, z0, K, cfg["backbone"], True)
            times.append(time.time() - t0)
            log(f"cpu baseline pass {i}: {times[-1]:.2f}s")
            if time.time() - t_start > budget_s and len(times) >= WARM + 1:
                break
    timed = times[WARM:] if len(times) > WARM else times[-1:]
    t = float(np.median(timed))
    return {"value": Bs * K / t, "unit": "hypotheses/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle get_loss (torch CPU fp32, train-mode BN) on the GPU line's own workload: B={Bs} images x K={K} "
                      f"hypotheses, 256x256 (same networks and seeds), median of {len(timed)} passes after {min(WARM, len(times) - 1)} "
                      f"warm-up ({'BASELINE.md protocol' if len(timed) == TIMED else 'cut short by the ' + str(int(budget_s)) + ' s budget: protocol asks for ' + str(TIMED)}), "
                      f"{t * 1e3:.0f} ms/pass"}


def timed_windows(fn, steps, windows, dist, dev):
    """`windows` back-to-back timed regions of exactly `steps` steps each (every one bracketed by barrier + synchronize, MAX over ranks:
    dist.timed_region); returns (seconds of the MEDIAN window, [ms per step of every window]).  One 0.14-s window is at the mercy of a
    clock ramp or a neighbour on the box; the median of three is what the line reports."""
    from mhentropy_amd import dist as mdist
    dts = [mdist.timed_region(fn, steps, dist, dev) for _ in range(max(1, windows))]
    return float(np.median(dts)), [round(d / steps * 1e3, 3) for d in dts]


def dump_outputs(out, d, budget=64 << 20):
    """every tensor of the step's output dict as d/<name>.npy, float32 (float64 kept); were they over `budget` bytes together, each
    would be cut to the same share of its elements, a fixed seeded sample of the flattened array"""
    os.makedirs(d, exist_ok=True)
    arrs = {k: v.detach().to(torch.float64 if v.dtype == torch.float64 else torch.float32).cpu().numpy()
            for k, v in out.items() if torch.is_tensor(v)}
    total = sum(a.nbytes for a in arrs.values())
    for k, a in arrs.items():
        if total > budget:
            keep = np.random.default_rng(0).choice(a.size, max(1, a.size * budget // total), replace=False)
            a = a.reshape(-1)[np.sort(keep)]
        np.save(os.path.join(d, k + ".npy"), a)


def roofline_of(times, dtype, steps_timed, step_seconds, pmc_file, n_next=3):
    """roofline object of the kernel with the most time among `times` (ops.KERNEL_TIMES entries: name, algorithmic flop, two HIP events
    recorded on the launch stream, algorithmic bytes): priced against the roofline that binds its launches IN AGGREGATE - bf16 / f32 MFMA
    when sum(flop) / peak exceeds sum(algorithmic bytes) / 8 TB/s, HBM otherwise.  `traffic` = HBM bytes per launch from the committed PMC
    passes (tools/pmc_traffic.py), reported only while the kernel sources are the ones that were profiled."""
    agg = {}
    bound_all = time_all = 0.0
    for name, flops, ev0, ev1, nbytes in times:
        a = agg.setdefault(name, [0.0, 0.0, 0, 0.0, 0.0])
        t = ev0.elapsed_time(ev1) * 1e-3
        b = max(flops / PEAK[dtype], nbytes / HBM_PEAK)      # this launch's binding roofline (MFMA or HBM), seconds
        a[0] += flops; a[1] += t; a[2] += 1; a[3] += b; a[4] += nbytes
        bound_all += b; time_all += t
    if not agg:
        return None

    def entry(name):
        fl, sec, cnt, bnd, nby = agg[name]
        mfma_bound = fl / PEAK[dtype] >= nby / HBM_PEAK
        ach, peak, unit = (fl / sec / 1e12, PEAK[dtype] / 1e12, "TFLOP/s") if mfma_bound else (nby / sec / 1e9, HBM_PEAK / 1e9, "GB/s")
        e = {"bound": "mfma" if mfma_bound else "hbm", "kernel": name, "achieved": round(ach, 2), "peak": peak, "unit": unit,
             "frac": round(ach / peak, 4), "launches_per_step": cnt // steps_timed, "avg_launch_us": round(sec / cnt * 1e6, 2),
             "algorithmic_flop_per_launch": int(fl / cnt), "algorithmic_bytes_per_launch": int(nby / cnt),
             "tflops": round(fl / sec / 1e12, 1), "share_of_step": round(sec / steps_timed / step_seconds, 3)}
        if "wgrad" in name:         # one C-ABI entry launches both: rocprofv3's average for the kernel alone is ~8-13 us below avg_launch_us
            e["timed_interval"] = ("the weight-gradient kernel + its slab reducer launch (fixed-order sum of the pixel-range partials)" +
                                   ("; a multi-problem launch = up to 16 layers of a gradient bucket that share this tile shape" if "multi" in name else ""))
        return e
    order = sorted(agg, key=lambda k: -agg[k][1])
    roof = entry(order[0])
    traffic, tnote = None, "no PMC summary for this kernel"
    try:
        from tools.pmc_traffic import kernel_sources_sha1
        pmc = json.load(open(os.path.join(ROOT, "profiles", pmc_file)))
        if pmc.get("source_sha1") == kernel_sources_sha1():          # every .hip / .h of csrc/, not the convolutions only
            traffic = pmc["kernels"].get(order[0], {}).get("hbm_bytes_per_launch")
            tnote = f"HBM bytes per launch, rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (profiles/{pmc_file}, same kernel sources)"
        else:
            tnote = f"profiles/{pmc_file} was collected on other kernel sources: not reported (tests/test_abi_and_tables.py fails on this)"
    except Exception as e:
        tnote = f"profiles/{pmc_file}: {type(e).__name__}"
    roof.update({"traffic": traffic, "traffic_note": tnote,
                 # the same launches each against its own binding roofline, and all timed launches of the step
                 "frac_of_binding_roofline": round(agg[order[0]][3] / agg[order[0]][1], 4),
                 "all_timed_launches_frac_of_binding_roofline": round(bound_all / time_all, 4),
                 "next_kernels": [entry(k) for k in order[1:1 + n_next]]})
    return roof


def time_train_step(model, x, y, noise, B, K, args, dist, world, dev):
    """img/s of TrainStep.step (forward + hand-written reverse pass + all-reduce + clip + Adam) on the bench workload"""
    from mhentropy_amd import dist as mdist
    from mhentropy_amd.train import TrainStep
    ts = TrainStep(model, dist=dist)
    tstep = lambda: ts.step(x, y, noise=noise, N=K)          # noise=None: drawn on the device inside the step (mhe_randn_f32)
    for i in range(2):
        tout = tstep()
        torch.cuda.synchronize()
        log(f"train warm-up step {i} done (loss {float(tout['total']):.3f})")
    # per-kernel timing pass (eager; HIP events around every forward convolution and every weight-gradient launch of one step)
    troof = None
    if world == 1:
        from mhentropy_amd import ops
        ops.KERNEL_TIMES.clear()
        ops.TIMING = True
        tstep()
        torch.cuda.synchronize()
        ops.TIMING = False
        train_times = list(ops.KERNEL_TIMES)
        ops.KERNEL_TIMES.clear()
    tlaunch = "eager"
    if args.graph:
        # the whole step (~840 launches; step count and gradient norm live in device memory) replays from one captured HIP
        # graph; with N > 1 from six graphs cut at the gradient buckets, the RCCL all-reduces issued between them
        try:
            from mhentropy_amd.train import GraphedStep
            gstep = GraphedStep(ts, x, y, noise=noise, N=K)
            gstep.replay()
            torch.cuda.synchronize()
            tout, tstep = gstep.out, gstep.replay
            tlaunch = "hip-graph replay" if world == 1 else f"{len(gstep.graphs)} hip graphs, all-reduce between them"
        except Exception as e:          # capture is an optimisation, never a requirement
            log(f"train-step graph capture unavailable ({type(e).__name__}: {e}); timing eager launches")
            torch.cuda.synchronize()
            ts._capture = None
            tstep = lambda: ts.step(x, y, noise=noise, N=K)
    dtt, twin = timed_windows(tstep, args.train_steps, args.windows, dist, dev)
    assert torch.isfinite(tout["log_p"]).all(), "non-finite loss in the train step"
    train = {"img_per_s": round(world * B * args.train_steps / dtt, 1), "ms_per_step": round(dtt / args.train_steps * 1e3, 3),
             "windows_ms": twin, "steps": args.train_steps, "launch": tlaunch, "params": int(ts.n_params),
             "includes": "forward + hand-written reverse pass + %sclip_grad_norm_(1.0) + Adam(lr 2e-4)"
                         % ("RCCL all-reduce of the flat f32 gradient + " if world > 1 else "")}
    if world == 1 and train_times:
        train["roofline"] = roofline_of(train_times, args.dtype, 1, dtt / args.train_steps, PMC_TRAFFIC_TRAIN)
    log(f"train step: {train['ms_per_step']} ms/step, {train['img_per_s']} img/s (windows {twin})")
    if args.metrics_samples > 0:
        train["iteration_with_metrics"] = time_iteration_with_metrics(ts, x, y, noise, B, K, args, dist, world, dev)
    return train


def time_iteration_with_metrics(ts, x, y, noise, B, K, args, dist, world, dev):
    """the reference's REAL loop body (hand/CrossModalHand.py:349-361, 452-470): get_loss + the per-iteration metrics pass
    sample(N=[200,200], temp=0.8, mods={uv,xyz,verts}) + MHEntLoss (14 metrics) + backward + clip + Adam.  The reference runs the encoder a
    second time for the metrics pass; here it reuses this forward's feature and advances the BatchNorm buffers twice (same results)."""
    from mhentropy_amd.criteria import MHEntLoss
    crit, n = MHEntLoss(), args.metrics_samples
    launch = "eager"

    def it():
        out = ts.step(x, y, noise=noise, N=K, test_samples=n)
        with torch.no_grad():
            out["criterion"] = crit(dict(out), y)
        return out
    try:
        out = it()
        torch.cuda.synchronize()
        run = it
        if args.graph:        # (data parallel: the same cut graphs as the train-step leg - a bucket's exchange between two graph launches)
            try:
                from mhentropy_amd.train import GraphedStep
                g = GraphedStep(ts, x, y, noise=noise, N=K, test_samples=n, criterion=crit)
                g.replay()
                torch.cuda.synchronize()
                out, run, launch = g.out, g.replay, "hip-graph replay"
            except Exception as e:
                log(f"iteration-with-metrics graph capture unavailable ({type(e).__name__}: {e}); eager")
                torch.cuda.synchronize()
                ts._capture = None
        dti, win = timed_windows(run, args.train_steps, args.windows, dist, dev)
        m = out["criterion"][2]
        assert all(torch.isfinite(v).all() for v in m.values()) and len(m) == 14, "metrics pass"
        res = {"ms_per_step": round(dti / args.train_steps * 1e3, 3), "windows_ms": win, "img_per_s": round(world * B * args.train_steps / dti, 1),
               "test_samples": n, "launch": launch,
               "includes": "train step + sample(N=[%d,%d], temp=0.8, mods={uv,xyz,verts}) from the step's own feature + MHEntLoss (14 metrics); "
                           "BatchNorm buffers advanced twice like the reference's two train-mode encoder passes" % (n, n)}
        log(f"iteration with metrics (N={n}): {res['ms_per_step']} ms/step ({launch})")
        return res
    except Exception as e:
        log(f"iteration-with-metrics leg failed: {type(e).__name__}: {e}")
        return {"error": f"{type(e).__name__}: {e}"[:300]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="c2", choices=sorted(WORKLOADS))
    ap.add_argument("--dtype", default=None, choices=["f32", "bf16"],
                    help="default: the dtype BASELINE.json's configs name for the workload (c2: bf16; c0, c1: f32)")
    ap.add_argument("--flow", default="realnvp", choices=["realnvp", "glow"],
                    help="realnvp: the flow the reference ships (configs/ho3d.yaml:39) - the measured default; glow: the 4-layer "
                         "ConditionalGlow branch (parity unpinned; its train leg runs eagerly; no CPU baseline)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: per-kernel roofline pass, train-step and iteration-with-metrics "
                         "legs, Glow variant, CPU baseline, median of --windows windows (the options below marked --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0's get_loss dict) as DIR/<name>.npy, "
                         "float32 (float64 kept)")
    ap.add_argument("--no-glow-variant", action="store_true",
                    help="--full: skip the extra forward+loss timing of the same workload with the ConditionalGlow flow (BASELINE.json's "
                         "configs name a 4-block Glow; the reference ships RealNVP, which stays the measured default)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--train-steps", type=int, default=5,
                    help="--full: also time this many full train steps (forward + reverse + all-reduce + clip + Adam) for the metric's "
                         "'img/s train step' part; 0 skips it")
    ap.add_argument("--windows", type=int, default=3,
                    help="--full: timed windows of --steps (--train-steps) steps each; ms_per_step / value are the MEDIAN window's, "
                         "windows_ms lists all (a plain run times one window)")
    ap.add_argument("--metrics-samples", type=int, default=200,
                    help="--full: also time the reference's whole iteration: train step + sample(N=this) + MHEntLoss metrics "
                         "(hand/CrossModalHand.py:349-361); 0 skips it")
    ap.add_argument("--graph", type=int, default=1, help="replay the step from a captured HIP graph (1) or launch eagerly (0)")
    ap.add_argument("--resident-noise", type=int, default=0,
                    help="1: feed a pre-drawn base-noise tensor (parity-style) instead of drawing z0 on the device inside every step")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.dtype is None:
        args.dtype = "bf16" if args.workload == "c2" else "f32"
    if not args.full:
        args.windows = 1

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher.  Nothing has touched the GPU yet in this process; the N ranks
        # are fresh children of torch.distributed.run (one per GPU, RCCL over xGMI), rank 0 prints the JSON line on the
        # inherited stdout, and this process exits with the launcher's status.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        log("spawning " + " ".join(cmd))
        # relay rank 0's JSON line only (a communication backend may chat on stdout: gloo does in the one-GPU rehearsal)
        child = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=subprocess.PIPE, text=True)
        for line in child.stdout.splitlines():
            if line.startswith("{") and line.rstrip().endswith("}"):
                print(line, flush=True)
            elif line.strip():
                print(line, file=sys.stderr, flush=True)
        raise SystemExit(child.returncode)

    from mhentropy_amd import dist as mdist
    # MHE_BENCH_REHEARSE=1 (development only): all ranks share cuda:0 and talk over gloo, to rehearse the N>1 code
    # path on a one-GPU box; the driver's runs use RCCL with one GPU per rank
    rehearse = os.environ.get("MHE_BENCH_REHEARSE") == "1"
    rank, local_rank, world, dist = mdist.init("gloo" if rehearse else "nccl")
    if rehearse:
        local_rank = 0
        torch.cuda.set_device(0)
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with "
                         "python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...")
    if world == 1:
        torch.cuda.set_device(0)
    else:           # host-side table building / synthetic data: share the node's cores between the ranks
        torch.set_num_threads(max(1, (os.cpu_count() or 8) // world))
    dev = torch.device("cuda", local_rank if world > 1 else 0)

    from mhentropy_amd import ops, synth
    cfg = WORKLOADS[args.workload]
    B, K = cfg["B"], cfg["K"]
    log(f"building model for workload {args.workload} ({args.dtype})")
    model, sd = build_model(cfg, args.dtype, args.seed, args.flow)
    if args.flow == "glow":
        args.no_cpu_baseline = True
    model = model.to(dev).train()
    # rank-private shard of synthetic images / targets / base noise, resident in HBM before timing
    x, yn = synth.batch(args.seed + 17 * rank, B, image_size=256)
    x = torch.as_tensor(x).to(dev)
    y = {k: torch.as_tensor(v).to(dev) for k, v in yn.items()}
    # base noise z0 ~ N(0, I): drawn on the device INSIDE the timed step like the reference's per-call prior.sample (hand/flows.py:339);
    # --resident-noise 1 feeds one pre-drawn tensor instead (what parity runs do)
    torch.manual_seed(args.seed + 17 * rank)
    ops.rng_state(dev, seed=args.seed + 17 * rank)
    noise = torch.as_tensor(synth.noise(args.seed + 17 * rank, K * B)).to(dev) if args.resident_noise else None

    def step():
        return model.get_loss(x, y, mods=["uv"], N=K, noise=noise)

    log("inputs resident; warm-up")
    for i in range(max(args.warmup, 1)):
        out = step()
        torch.cuda.synchronize()
        log(f"warm-up step {i} done")
    # ---- per-kernel timing pass (--full; eager, HIP events on the launch stream around every conv launch)
    fwd_times = []
    if args.full:
        ops.KERNEL_TIMES.clear()
        ops.TIMING = True
        for _ in range(min(args.steps, 3)):
            step()
        torch.cuda.synchronize()
        ops.TIMING = False
        fwd_times = list(ops.KERNEL_TIMES)
        ops.KERNEL_TIMES.clear()
    # ---- the timed region: exactly `steps` steps, replayed from one captured HIP graph (launch-bound inner
    # loop: ~250 launches per step) or launched eagerly with --graph 0
    last = {}
    if args.graph:
        gstream = torch.cuda.Stream()
        gstream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(gstream):
            step()
        torch.cuda.current_stream().wait_stream(gstream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            last["out"] = step()
        graph.replay()
        torch.cuda.synchronize()
        log("HIP graph captured")
        run = graph.replay
    else:
        def run():
            last["out"] = step()
    # barrier+sync | K steps | sync+barrier, MAX over ranks - `windows` times, the median window is reported
    dt, windows_ms = timed_windows(run, args.steps, args.windows, dist, dev)
    out = last["out"]
    loss_out = {k: v.clone() for k, v in out.items()}
    log(f"timed region: {dt * 1e3 / args.steps:.2f} ms/step (windows {windows_ms})")
    assert torch.isfinite(loss_out["log_p"]).all(), "non-finite loss"
    if args.dump_outputs and rank == 0:
        dump_outputs(loss_out, args.dump_outputs)
        log(f"outputs of the last timed step written to {args.dump_outputs}")

    # ---- second part of BASELINE.json's metric (--full): img/s of a full train step (hand/CrossModalHand.py:455-470) on
    # the same model, inputs and hypotheses; every rank takes part (gradient all-reduce over RCCL when N > 1)
    train = None
    if args.full and args.train_steps > 0:
        del last, run
        if args.graph:
            del graph
        try:
            train = time_train_step(model, x, y, noise, B, K, args, dist, world, dev)
        except Exception as e:      # the headline (forward + loss) line must survive a failure of the secondary leg
            log(f"train-step leg failed: {type(e).__name__}: {e}")
            train = {"error": f"{type(e).__name__}: {e}"[:300]}

    # ---- the same forward+loss workload with the Glow branch (parity unpinned), reported beside the headline, N=1 and --full only
    glow_variant = None
    if args.full and args.flow == "realnvp" and world == 1 and not args.no_glow_variant:
        try:
            del model
            torch.cuda.empty_cache()
            gmodel, _ = build_model(cfg, args.dtype, args.seed, "glow")
            gmodel = gmodel.to(dev).train()
            gstep = lambda: gmodel.get_loss(x, y, mods=["uv"], N=K, noise=noise)
            for _ in range(2):
                gstep()
            torch.cuda.synchronize()
            glaunch = "eager"
            if args.graph:          # round 5: nothing on the Glow path depends on a host value any more (ActNorm / LU algebra on the device)
                try:
                    gs2 = torch.cuda.Stream()
                    gs2.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(gs2):
                        gstep()
                    torch.cuda.current_stream().wait_stream(gs2)
                    ggraph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(ggraph):
                        gout = gstep()
                    ggraph.replay()
                    torch.cuda.synchronize()
                    assert torch.isfinite(gout["log_p"]).all()
                    gstep, glaunch = ggraph.replay, "hip-graph replay"
                except Exception as e:
                    log(f"glow variant graph capture unavailable ({type(e).__name__}: {e}); eager")
                    torch.cuda.synchronize()
            dtg, gwin = timed_windows(gstep, args.steps, args.windows, None, dev)
            glow_variant = {"flow": "4-layer ConditionalGlow h=512, %s, train-mode dropout p=0.2 drawn on the device (parity unpinned: third-party class absent "
                                    "from the reference)" % ("bf16 hidden products, f32 elsewhere" if args.dtype == "bf16" else "f32"),
                            "value": round(B * K * args.steps / dtg, 1), "unit": "hypotheses/s", "ms_per_step": round(dtg / args.steps * 1e3, 3),
                            "windows_ms": gwin, "launch": glaunch}
            log(f"glow variant: {glow_variant['ms_per_step']} ms/step ({glaunch})")
            if args.train_steps > 0:
                # ... and its full train step (the 45x45 ActNorm / LU re-parameterisation and its gradients run on the device: one HIP graph)
                from mhentropy_amd.train import TrainStep, GraphedStep
                if args.graph:
                    del ggraph
                gts = TrainStep(gmodel)
                gtstep = lambda: gts.step(x, y, noise=noise, N=K)
                for _ in range(2):
                    gtstep()
                torch.cuda.synchronize()
                gtl = "eager"
                if args.graph:
                    try:
                        gg = GraphedStep(gts, x, y, noise=noise, N=K)
                        gg.replay()
                        torch.cuda.synchronize()
                        assert torch.isfinite(gg.out["log_p"]).all()
                        gtstep, gtl = gg.replay, "hip-graph replay"
                    except Exception as e:
                        log(f"glow variant train-step graph capture unavailable ({type(e).__name__}: {e}); eager")
                        torch.cuda.synchronize()
                        gts._capture = None
                dtt, gtw = timed_windows(gtstep, args.train_steps, args.windows, None, dev)
                glow_variant["train_step"] = {"ms_per_step": round(dtt / args.train_steps * 1e3, 3), "img_per_s": round(B * args.train_steps / dtt, 1),
                                              "windows_ms": gtw, "steps": args.train_steps, "launch": gtl}
                log(f"glow variant train step: {glow_variant['train_step']['ms_per_step']} ms/step ({gtl})")
        except Exception as e:
            log(f"glow variant skipped: {type(e).__name__}: {e}")

    if rank == 0:
        # ---- roofline of the dominant kernel: the convolution instantiation with the most time in the step, priced against the
        # roofline that binds its launches IN AGGREGATE - bf16 MFMA (2.5 PFLOP/s dense) when sum(flops)/peak exceeds
        # sum(algorithmic bytes)/8 TB/s, HBM otherwise (the plain 1x1 layers at 64-512 input channels move 128-512 B per
        # pixel for 64-512 MACs per byte pair: HBM-bound on this chip).  Timed live: HIP events on the launch stream around
        # every launch (ops.TIMING), eager pass.  Both this and the CPU baseline run with --full only.
        roof = roofline_of(fwd_times, args.dtype, min(args.steps, 3), dt / args.steps, PMC_TRAFFIC) if args.full else None
        cpu = None if (not args.full or args.no_cpu_baseline or world > 1) else cpu_baseline(cfg, sd, args.seed)      # rank 0 at N=1 only
        line = {
            "metric": "hypotheses/sec (BxK) fwd+loss, 256x256",
            "value": round(world * B * K * args.steps / dt, 1), "unit": "hypotheses/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "windows_ms": windows_ms, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{args.workload}: MHEnt.get_loss forward+loss, {cfg['backbone']} encoder (train-mode BN), "
                                   f"{'4-layer ConditionalGlow h=512 (parity unpinned)' if args.flow == 'glow' else str(2 * cfg['steps']) + '-coupling RealNVP h=' + str(cfg['h'])}, MANO joints, B={B}/GPU, K={K}, 256x256",
                       "images_per_gpu": B, "hypotheses_per_image": K, "global_batch": world * B,
                       "launch": "hip-graph replay" if args.graph else "eager",
                       "base_noise": "resident tensor" if args.resident_noise else "drawn on the device inside the step (Philox4x32-10, mhe_randn_f32)",
                       "img_per_s": round(world * B * args.steps / dt, 1),
                       "timing": (f"median of {args.windows} windows of {args.steps} steps, each" if args.windows > 1 else
                                  f"one window of {args.steps} steps,") + " bracketed by barrier + synchronize",
                       "switches_set": __import__("mhentropy_amd.switches", fromlist=["x"]).non_default(),     # {} = the product path (mhentropy_amd/switches.py)
                       "ranks": world, "rccl_ranks": (world if (dist is not None and dist.get_backend() == "nccl") else 0),
                       "backend": (None if dist is None else "rccl (torch backend 'nccl')" if dist.get_backend() == "nccl" else dist.get_backend()),
                       "glow_variant": glow_variant},
            "train_step": train, "roofline": roof, "cpu_baseline": cpu,
        }
        print(json.dumps(line), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
