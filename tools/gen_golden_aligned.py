"""Golden vectors of the reference's aligned evaluation, MHEntLoss with `aligned` switched on (hand/criteria.py:62-87,93-96,139-165,
helper align_w_scale hand/utils.py:502-525 around scipy.linalg.orthogonal_procrustes), for tests/golden/criteria_aligned_{small,shipped}.npz.

Runs where the reference tree exists (like oracle/gen_golden.py, whose helpers it reuses unchanged).  The reference hard-codes
`aligned = False` inside MHEntLoss.forward: this script compiles the reference's criteria module once more in memory with that one
line switched to True and runs it on CPU (`.cuda()` is the identity under oracle.gen_golden's placeholders).  Nothing of that
text is written anywhere; the fixtures hold data only.

Inputs are sample_xyz / sample_uv / sample_verts, loss_log_p and the y_* targets of tests/golden/mhent_{small,shipped}.npz (N = 4
hypotheses).  Two target cases per size:
  base    y_pose3d as it is; y_verts = another hypothesis' mesh (hypothesis N-1 of the next image), rotated, scaled from the
          sample's units to metres (x 0.01), translated to about 0.6 m from the origin, with 1 mm Gaussian noise;
  mirror  pose3d and verts = hypothesis 0's joints / mesh of the same image, rotated, MIRRORED (x -> -x), scaled and translated
          (verts in metres as above, plus 0.1 mm noise): hypothesis 0 aligns with an R of determinant -1, which
          orthogonal_procrustes keeps.
Per case: the 14 metrics, the aligned xyz / verts the reference writes back into `output`, and R, s of every row from the
reference's own align_w_scale.

    python tools/gen_golden_aligned.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mhentropy_amd import synth  # noqa: E402
from oracle.gen_golden import GOLD, REF, _install_placeholders  # noqa: E402

FLAG = "        aligned = False\n"


def aligned_criteria(criteria):
    """the reference's criteria module with MHEntLoss.forward's `aligned` flag set, compiled in memory"""
    with open(criteria.__file__) as f:
        src = f.read()
    assert src.count(FLAG) == 1, "the reference's aligned flag moved"
    mod = types.ModuleType("criteria_aligned")
    mod.__file__ = criteria.__file__
    exec(compile(src.replace(FLAG, FLAG.replace("False", "True")), criteria.__file__, "exec"), mod.__dict__)
    return mod


def rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def f64_align(A, Bm):
    """the issue's formula in float64 (numpy's SVD): the check the fixtures are generated against"""
    A, Bm = np.asarray(A, np.float64), np.asarray(Bm, np.float64)
    t1, t2 = A.mean(0), Bm.mean(0)
    A0, B0 = A - t1, Bm - t2
    s1, s2 = np.linalg.norm(A0) + 1e-8, np.linalg.norm(B0) + 1e-8
    A0, B0 = A0 / s1, B0 / s2
    u, w, vt = np.linalg.svd(A0.T @ B0)
    R = u @ vt
    return (B0 @ R.T) * w.sum() * s1 + t1, R, w.sum()


def gen(criteria_al, utils, tag):
    print(f"[criteria_aligned_{tag}]")
    d = np.load(os.path.join(GOLD, f"mhent_{tag}.npz"))
    xyz, uv, verts = d["sample_xyz"], d["sample_uv"], d["sample_verts"]
    N, B = xyz.shape[:2]
    rng = np.random.default_rng(7000 + B)
    base_v, mir_v, mir_x = [], [], []
    for b in range(B):
        m = verts[N - 1, (b + 1) % B].reshape(-1, 3).astype(np.float64)
        t = np.array([0.05, -0.08, 0.6]) + rng.normal(0, 0.02, 3)
        base_v.append((m - m.mean(0)) @ rot(rng).T * 0.01 + t + rng.normal(0, 1e-3, m.shape))
        Q = rot(rng) @ np.diag([-1.0, 1.0, 1.0])                            # a reflection: det -1
        m0 = verts[0, b].reshape(-1, 3).astype(np.float64)
        mir_v.append(m0 @ Q.T * 0.01 + t + rng.normal(0, 1e-4, m0.shape))
        x0 = xyz[0, b].reshape(-1, 3).astype(np.float64)
        mir_x.append(x0 @ Q.T * 0.9 + np.array([0.1, -0.2, 0.05]))
    cases = {"base": (d["y_pose3d"], np.stack(base_v).reshape(B, -1).astype(np.float32)),
             "mirror": (np.stack(mir_x).reshape(B, -1).astype(np.float32), np.stack(mir_v).reshape(B, -1).astype(np.float32))}
    gold = {}
    crit = criteria_al.MHEntLoss()
    for cname, (p3, yv) in cases.items():
        y = {k: torch.as_tensor(d["y_" + k]) for k in ("crop_uv", "vis", "st", "scale")}
        y["pose3d"], y["verts"] = torch.as_tensor(p3), torch.as_tensor(yv)
        out = {"log_p": torch.as_tensor(d["loss_log_p"]), "xyz": torch.as_tensor(xyz), "uv": torch.as_tensor(uv), "verts": torch.as_tensor(verts)}
        with torch.no_grad():
            _, _, met = crit(out, y)
        gold[f"{cname}_pose3d"], gold[f"{cname}_verts"] = p3, yv
        gold.update({f"{cname}_metric_{k}": v.numpy() for k, v in met.items()})
        for lbl, tgt in (("xyz", p3), ("verts", yv)):
            al = out[lbl].numpy()
            assert al.shape == (N, B, tgt.shape[1]) and al.dtype == np.float32
            Rs, ss = np.zeros((N, B, 3, 3), np.float32), np.zeros((N, B), np.float32)
            worst = 0.0
            for n in range(N):
                for b in range(B):
                    a_ref, R, s = utils.align_w_scale(tgt[b].reshape(-1, 3), (xyz if lbl == "xyz" else verts)[n, b].reshape(-1, 3),
                                                      return_trafo=True)[:3]
                    assert np.array_equal(a_ref.reshape(-1).astype(np.float32), al[n, b])
                    Rs[n, b], ss[n, b] = R, s
                    a64, R64, s64 = f64_align(tgt[b].reshape(-1, 3), (xyz if lbl == "xyz" else verts)[n, b].reshape(-1, 3))
                    worst = max(worst, np.abs(al[n, b] - a64.reshape(-1)).max() / np.abs(a64).max())
                    assert np.allclose(R, R64, atol=2e-4), (lbl, n, b)
            print(f"  {cname} {lbl}: reference (f32) vs f64 restatement, max rel diff {worst:.2e}; det R of n=0: "
                  f"{np.round(np.linalg.det(Rs[0].astype(np.float64)), 4)}")
            gold[f"{cname}_{lbl}_aligned"], gold[f"{cname}_R_{lbl}"], gold[f"{cname}_s_{lbl}"] = al, Rs, ss
        if cname == "mirror":
            assert (np.linalg.det(gold["mirror_R_xyz"][0].astype(np.float64)) < 0).all()
            assert (np.linalg.det(gold["mirror_R_verts"][0].astype(np.float64)) < 0).all()
    path = os.path.join(GOLD, f"criteria_aligned_{tag}.npz")
    np.savez_compressed(path, **gold)
    print(f"  {path}: {os.path.getsize(path)} bytes")


def main():
    tables = synth.mano_tables(0)
    _install_placeholders(tables)
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir("/tmp")
    import criteria       # noqa: E402  (reference module)
    import utils          # noqa: E402
    os.chdir(cwd)
    criteria_al = aligned_criteria(criteria)
    gen(criteria_al, utils, "small")
    gen(criteria_al, utils, "shipped")
    print("golden fixtures written to", GOLD)


if __name__ == "__main__":
    main()
