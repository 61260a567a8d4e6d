"""Golden vectors of the reference's chamfer_dist (hand/criteria.py:18-39) for tests/golden/chamfer_small.npz.

Runs on the CPU where the reference tree exists (like oracle/gen_golden.py, whose placeholder modules it installs by importing that
helper).  The reference's own function is called on the seeded inputs of tests/chamfer_ref.py (float32 values, handed over as float64 so
that the fixture pins the definition, not float32 rounding), once with the (N, B, K, 3) input and once with the (B, K, 3) form.  The
fixture holds data only: inputs and the reference's outputs.

    python tools/gen_chamfer_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chamfer_ref  # noqa: E402
from mhentropy_amd import synth  # noqa: E402
from oracle.gen_golden import GOLD, REF, _install_placeholders  # noqa: E402

SEED, SHAPE = 101, (3, 2, 21, 37)          # (N, B, K, VO)


def main():
    _install_placeholders(synth.mano_tables(0))
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir("/tmp")
    import criteria       # noqa: E402  (reference module)
    os.chdir(cwd)
    case = chamfer_ref.make_case(SEED, *SHAPE)
    tgt = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in chamfer_ref.target_of(case).items()}
    pts = torch.as_tensor(case["points"].astype(np.float64))
    with torch.no_grad():
        dist4 = criteria.chamfer_dist(pts, tgt).numpy()
        dist3 = criteria.chamfer_dist(pts[1], tgt).numpy()
    mine = chamfer_ref.chamfer64(case["points"], case["scale"], case["root"], case["obj"])
    err = np.abs(mine["dist"] - dist4).max() / np.abs(dist4).max()
    print(f"reference vs f64 restatement: max rel diff {err:.2e}; gap of the minima {mine['gap']:.2e}")
    assert err < 1e-9 and dist4.shape == SHAPE[:2] and dist3.shape == SHAPE[1:2] and mine["gap"] > chamfer_ref.GAP
    path = os.path.join(GOLD, "chamfer_small.npz")
    np.savez_compressed(path, seed=SEED, shape=np.asarray(SHAPE), points=case["points"], scale=case["scale"], root=case["root"], obj=case["obj"],
                        dist=dist4, hypothesis_3d=1, dist_3d=dist3)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
