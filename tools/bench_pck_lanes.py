#!/usr/bin/env python3
"""How many lanes should serve a hypothesis of few points in mhe_pck_curve_f32 (csrc/pck.hip)?  The kernel's MHE_PCK_SMALL_LANES is a build-time
constant; this tool builds the three forms (16, 32 and 64 lanes: four, two and one hypotheses per wave) as small libraries of their own
(csrc/pck.hip + csrc/api.hip, under build/pck_lanes/, rebuilt when a source is newer) and times them against one another in one process, on
the same tensors, the forms alternating window by window so that a drift of the machine meets all of them.  A form is timed only at shapes
it serves differently from the 64-lane form (P <= its lanes).  Before timing, every form's three outputs are compared bit for bit with the
64-lane form's.

Device-event time per call, 20 calls a window after 3 warm-up calls, WINDOWS windows per form; the outputs are allocated once, outside the timed
region, so that a call is one launch.  Shapes: the joints (P = 21) and a sparse set (P = 8) at the evaluation shape N = 200, B = 64, where the
call is close to the launch floor, and at N = 2000, where the kernel's own time dominates.

    python tools/bench_pck_lanes.py [--json out.json] [--build-only]
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "mhentropy_amd", "csrc")
OUT = os.path.join(ROOT, "build", "pck_lanes")
LANES = (16, 32, 64)
SHAPES = tuple((n, 64, p) for n in (200, 2000) for p in (21, 8))
T, CALLS, WINDOWS = 100, 20, int(os.environ.get("WINDOWS", 9))


def build():
    from mhentropy_amd.build import FLAGS, HIPCC
    os.makedirs(OUT, exist_ok=True)
    srcs = [os.path.join(CSRC, "pck.hip"), os.path.join(CSRC, "api.hip")]
    deps = srcs + [os.path.join(CSRC, "common.h"), os.path.join(ROOT, "include", "mhe.h")]
    libs = {}
    for lanes in LANES:
        lib = libs[lanes] = os.path.join(OUT, f"libpck_{lanes}.so")
        if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
            subprocess.check_call([HIPCC] + FLAGS + [f"-DMHE_PCK_SMALL_LANES={lanes}", "-shared", "-o", lib] + srcs)
    return libs


def main():
    libs = build()
    if "--build-only" in sys.argv:
        print("\n".join(libs.values()))
        return
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench_pck_lanes needs the GPU: there is no CPU path"
    entry = {}
    for lanes, path in libs.items():
        entry[lanes] = C.CDLL(path).mhe_pck_curve_f32
        entry[lanes].argtypes = [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]
    thr = torch.linspace(0.0, 50.0, T).cuda()
    rec = {"device": torch.cuda.get_device_name(0), "T": T, "calls_per_window": CALLS, "windows": WINDOWS, "outputs": "allocated once", "shapes": []}
    for N, B, P in SHAPES:
        g = torch.Generator().manual_seed(N + B + P)
        target = torch.randn(B, P, 3, generator=g)
        pred = (target[None] + 0.15 * torch.randn(N, B, P, 3, generator=g)).cuda()
        target, scale = target.cuda(), (0.025 + 0.015 * torch.rand(B, generator=g)).cuda()
        forms = [lanes for lanes in LANES if P <= lanes]          # (a form with fewer lanes than points launches the 64-lane kernel)
        out = {lanes: (torch.empty(N, B, T, dtype=torch.int32, device="cuda"), torch.empty(N, B, device="cuda"), torch.empty(N, B, device="cuda"))
               for lanes in forms}

        def call(lanes):
            h, a, e = out[lanes]
            st = entry[lanes](pred.data_ptr(), target.data_ptr(), scale.data_ptr(), None, thr.data_ptr(), 1000.0, h.data_ptr(), a.data_ptr(), e.data_ptr(),
                              N, B, P, T, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert st == 0, (lanes, st)
        for lanes in forms:
            call(lanes)
        torch.cuda.synchronize()
        for lanes in forms:
            assert all(torch.equal(x, y) for x, y in zip(out[lanes], out[64])), f"{lanes} lanes differ from 64 at {(N, B, P)}"
        times = {lanes: [] for lanes in forms}
        for _ in range(WINDOWS):
            for lanes in forms:
                for _ in range(3):
                    call(lanes)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(CALLS):
                    call(lanes)
                e1.record()
                torch.cuda.synchronize()
                times[lanes].append(e0.elapsed_time(e1) / CALLS)
        rec["shapes"].append({"N": N, "B": B, "P": P, "ms_per_call": {str(lanes): {"median": float(np.median(v)), "min": min(v), "max": max(v)}
                                                                     for lanes, v in times.items()}})
    print(json.dumps(rec), flush=True)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
