"""CPU: the aligned evaluation (MHEntLoss with `aligned`, hand/criteria.py:62-87, align_w_scale hand/utils.py:502-525): a float64
restatement of the alignment against the reference-generated fixtures tests/golden/criteria_aligned_{small,shipped}.npz
(tools/gen_golden_aligned.py), the metrics composed from it through the oracle, and the new call surface."""
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden, assert_close


def align_f64(target, pred):
    """the reference's formula in float64, batched: target [B,P*3], pred [N,B,P*3] -> aligned [N,B,P*3], R [N,B,3,3], s [N,B].
    t1 = mean A, s1 = |A - t1|_F + 1e-8, A0 = (A - t1)/s1 (B0 likewise);  A0^T B0 = U S V^T, R = U V^T (no det correction),
    s = tr S;  aligned = (B0 R^T) s s1 + t1"""
    A = np.asarray(target, np.float64).reshape(target.shape[0], -1, 3)[None]
    Bm = np.asarray(pred, np.float64).reshape(pred.shape[0], pred.shape[1], -1, 3)
    t1, t2 = A.mean(2, keepdims=True), Bm.mean(2, keepdims=True)
    A0, B0 = A - t1, Bm - t2
    s1 = np.sqrt((A0 ** 2).sum((2, 3), keepdims=True)) + 1e-8
    s2 = np.sqrt((B0 ** 2).sum((2, 3), keepdims=True)) + 1e-8
    A0, B0 = A0 / s1, B0 / s2
    u, w, vt = np.linalg.svd(np.swapaxes(A0, 2, 3) @ B0)
    R = u @ vt
    s = w.sum(-1)
    out = (B0 @ np.swapaxes(R, 2, 3)) * s[..., None, None] * s1 + t1
    return out.reshape(pred.shape), R, s


def aligned_metrics_oracle(g, d, case):
    """the 14 metrics of the aligned branch through oracle.criteria_ref (unchanged): the 3D error rows of the f64-aligned joints, the
    3D spread rows of the unaligned ones (criteria.py:63-68,141), the 2D rows as before"""
    from oracle import criteria_ref
    y = {k: torch.as_tensor(d["y_" + k]).double() for k in ("crop_uv", "vis", "scale")}
    y["pose3d"] = torch.as_tensor(g[f"{case}_pose3d"]).double()
    al = align_f64(g[f"{case}_pose3d"], d["sample_xyz"])[0]
    base = {"log_p": torch.as_tensor(d["loss_log_p"]).double(), "uv": torch.as_tensor(d["sample_uv"]).double()}
    _, _, m_al = criteria_ref.mhent_loss(dict(base, xyz=torch.as_tensor(al)), y)
    _, _, m_un = criteria_ref.mhent_loss(dict(base, xyz=torch.as_tensor(d["sample_xyz"]).double()), y)
    return {k: (m_un[k] if k.startswith("eucLoss_3d") and k.endswith("_std") else m_al[k]) for k in m_al}


@pytest.mark.parametrize("tag", ["small", "shipped"])
@pytest.mark.parametrize("case", ["base", "mirror"])
def test_f64_restatement_matches_reference_aligned_outputs(tag, case):
    """the reference runs align_w_scale in float32 (numpy / LAPACK sgesdd): its aligned joints and meshes lie within 1e-6 of the
    float64 restatement, relative to the largest coordinate (measured: <= 8.1e-7); R within 1e-4, s within 1e-5 relative.
    The mirror case pins reflections: det R = -1 for hypothesis 0 of every image"""
    g, d = load_golden(f"criteria_aligned_{tag}"), load_golden(f"mhent_{tag}")
    for lbl, src in (("xyz", "sample_xyz"), ("verts", "sample_verts")):
        tgt = g[f"{case}_pose3d"] if lbl == "xyz" else g[f"{case}_verts"]
        al, R, s = align_f64(tgt, d[src])
        assert_close(g[f"{case}_{lbl}_aligned"], al, 1e-6, what=f"{case} {lbl} aligned")
        assert_close(g[f"{case}_R_{lbl}"], R, 0, 1e-4, what=f"{case} R {lbl}")
        assert_close(g[f"{case}_s_{lbl}"], s, 1e-5, what=f"{case} s {lbl}")
        if case == "mirror":
            assert (np.linalg.det(R[0]) < -0.999).all()
            assert (np.linalg.det(g[f"mirror_R_{lbl}"][0].astype(np.float64)) < -0.999).all()


@pytest.mark.parametrize("tag", ["small", "shipped"])
@pytest.mark.parametrize("case", ["base", "mirror"])
def test_aligned_metrics_oracle_matches_reference(tag, case):
    """the 14 aligned metrics composed through the oracle in float64 equal the reference's float32 ones to 2e-5 relative (1e-6 absolute:
    the mirror case aligns hypothesis 0 exactly, so its best-of-N error rows are ~1e-7, float32 noise)"""
    g, d = load_golden(f"criteria_aligned_{tag}"), load_golden(f"mhent_{tag}")
    met = aligned_metrics_oracle(g, d, case)
    assert len(met) == 14
    for k, v in met.items():
        assert_close(g[f"{case}_metric_{k}"], v.numpy(), 2e-5, 1e-6, what=f"{case} {k}")
    # the spread rows are the unaligned evaluation's: they do not depend on the target
    for k in ("sample_std", "vis_std", "invis_std"):
        assert_close(g[f"{case}_metric_eucLoss_3d_rgb_{k}"], d[f"metric_eucLoss_3d_rgb_{k}"], 1e-6, what=k)


def test_degenerate_rows_in_the_restatement():
    """an all-zero target gives M = 0: s = 0 and every aligned point equals t1 (= 0)"""
    rng = np.random.default_rng(0)
    pred = rng.normal(size=(3, 2, 63))
    al, R, s = align_f64(np.zeros((2, 63)), pred)
    assert np.all(s == 0) and np.all(al == 0)


def test_criterion_accepts_aligned_and_abi_lists_the_new_entry_points():
    from mhentropy_amd import _lib
    from mhentropy_amd.criteria import MHEntLoss
    sig = inspect.signature(MHEntLoss.__init__)
    assert list(sig.parameters)[1:] == ["loss_weights", "aligned"] and sig.parameters["aligned"].default is False
    assert MHEntLoss(aligned=True).aligned and not MHEntLoss().aligned
    for name in ("mhe_procrustes_align_f32", "mhe_procrustes_workspace_floats", "mhe_metrics_split_f32"):
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 4


def test_run_parses_aligned():
    from mhentropy_amd import run
    src = inspect.getsource(run.main)
    assert '"--aligned"' in src and "MHEntLoss(aligned=args.aligned)" in src
