"""CPU: the host side of the hand-mesh reverse - the new C entries declared, exported and bound, refusing bad arguments before any launch; the
workspace size; the ops' argument checks; and the bounds of tests/test_gpu_mano_verts_bwd.py: the float32 restatement, re-measured here, meets
the bounds themselves (four times the recorded constants), and the float64 reference's camera columns are exactly 0."""
import os
import re

import numpy as np
import pytest
import torch

import mano_bwd_ref as mr
from conftest import ROOT
from mhentropy_amd import _lib, mano_pack, ops

NEW = {"mhe_mano_verts_bwd_workspace_floats": 1, "mhe_mano_verts_bwd_f32": 9, "mhe_mano_regress_joints_bwd_f32": 6}


def test_symbols_declared_and_bound_with_matching_arity():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhe.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, arity in NEW.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/mhe.h"
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")) == arity, name
    assert L.mhe_abi_version() == 4
    assert "mano_skin_bwd.hip" in __import__("mhentropy_amd.build", fromlist=["SOURCES"]).SOURCES
    from mhentropy_amd.ManoLayer import ManoLayer
    assert all(callable(f) for f in (ops.mano_verts_bwd, ops.mano_regress_joints_bwd, ManoLayer.verts))


def test_workspace_is_positive_and_monotone():
    f = _lib.lib().mhe_mano_verts_bwd_workspace_floats
    sizes = [f(R) for R in (1, 2, 32, 33, 70, 16384, 51200)]
    assert f(0) == 0 and f(-3) == 0 and sizes[0] > 0
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] - sizes[0] == 2 * 352                 # the forward's workspace row and the adjoint row of one hypothesis


def test_entries_refuse_bad_arguments_before_any_launch():
    L, R = _lib.lib(), 3
    A = lambda t: None if t is None else _lib.C.c_void_p(t.data_ptr())          # host addresses: every call below must return before a kernel could read them
    z, tb, gv, gj = torch.zeros(R, 61), torch.zeros(mano_pack.TOTAL_FLOATS), torch.zeros(R, 778, 3), torch.zeros(R, 63)
    g_z, ws = torch.zeros(R, 61), torch.zeros(L.mhe_mano_verts_bwd_workspace_floats(R))

    def bwd(z_=z, t=tb, g=gv, j=gj, out=g_z, w=ws, r=R):
        return L.mhe_mano_verts_bwd_f32(A(z_), A(t), A(g), A(j), A(out), A(w), r, 0, None)
    bad = {"null z": dict(z_=None), "null tables": dict(t=None), "null g_verts": dict(g=None), "null g_z": dict(out=None), "null workspace": dict(w=None),
           "R = 0": dict(r=0), "R < 0": dict(r=-1), "g_z overlaps z": dict(out=z), "g_z overlaps g_verts": dict(out=gv), "g_z overlaps g_joints_mm": dict(out=gj),
           "g_z overlaps tables": dict(out=tb), "workspace overlaps z": dict(w=z), "workspace overlaps g_verts": dict(w=gv), "g_z inside the workspace": dict(out=ws)}
    for what, kw in bad.items():
        assert bwd(**kw) == 1 and b"mhe_mano_verts_bwd_f32" in L.mhe_last_error(), what          # MHE_ERR_ARG
    g21, out = torch.zeros(R, 21, 3), torch.zeros(R, 778, 3)

    def reg(g=g21, t=tb, o=out, r=R):
        return L.mhe_mano_regress_joints_bwd_f32(A(g), A(t), A(o), r, 0, None)
    for what, kw in {"null g_joints": dict(g=None), "null tables": dict(t=None), "null g_verts": dict(o=None), "R = 0": dict(r=0),
                     "g_verts overlaps g_joints": dict(g=out), "g_verts overlaps tables": dict(o=tb)}.items():
        assert reg(**kw) == 1 and b"mhe_mano_regress_joints_bwd_f32" in L.mhe_last_error(), what


def test_ops_check_their_arguments_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a launch was reached")
    monkeypatch.setattr(ops, "launch", no_launch)
    z, tb, gv = torch.zeros(3, 61), torch.zeros(mano_pack.TOTAL_FLOATS), torch.zeros(3, 778, 3)
    for args in ((z, tb, gv), (z.double(), tb, gv), (z[:, :60], tb, gv), (z, tb, gv.half()), (z, tb, gv[:, :700])):
        with pytest.raises(_lib.MheError):
            ops.mano_verts_bwd(*args)
    for args in ((torch.zeros(3, 21, 3), tb), (torch.zeros(3, 63).double(), tb), (torch.zeros(3, 20, 3), tb)):
        with pytest.raises(_lib.MheError):
            ops.mano_regress_joints_bwd(*args)
    # the checks themselves, with the device test out of the way: wrong dtypes and shapes are named
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for args, msg in (((z.double(), tb, gv), "expected torch.float32"), ((z, tb, torch.zeros(3, 777, 3)), "expected shape"),
                      ((z, tb[:-1], gv), "expected shape"), ((z, tb, gv, False, torch.zeros(3, 21, 3)), "expected shape")):
        with pytest.raises(_lib.MheError, match=msg):
            ops.mano_verts_bwd(*args)
    for args, msg in (((torch.zeros(3, 63), tb), "expected shape"), ((torch.zeros(3, 21, 3), tb, torch.zeros(2, 778, 3)), "expected shape"),
                      ((torch.zeros(3, 21, 3).double(), tb), "expected torch.float32")):
        with pytest.raises(_lib.MheError, match=msg):
            ops.mano_regress_joints_bwd(*args)


@pytest.mark.parametrize("name", list(mr.CASES))
def test_f32_restatement_is_what_the_bounds_were_taken_from(name):
    """the constants are one machine's measurement of a float32 sum whose order depends on the host's threads: re-measured, the restatement
    must itself meet the bound (four times the constant) that the kernel is held to"""
    dev = mr.f32_deviation(name)
    print(f"{name}: f32 restatement vs f64 {dev:.3e}, constant {mr.F32_DEV[name]:.3e}, bound {mr.BOUND[name]:.3e}")
    assert 0 < dev <= mr.BOUND[name]
    ref = mr.reference(name)
    assert (ref[:, 58:] == 0).all() and np.abs(ref).max() > 0
    assert set(mr.F32_DEV) == set(mr.CASES)


def test_wrapper_bound_and_regress_transpose():
    dev = mr.wrapper_f32_deviation()
    print(f"ManoLayer.forward objective: f32 restatement vs f64 {dev:.3e}, constant {mr.F32_DEV_WRAPPER:.3e}")
    assert 0 < dev <= 4 * mr.F32_DEV_WRAPPER
    g = mr.random_g(2, 3, 63).view(2, 21, 3)
    t = mr.regress_transpose(g)
    assert t.shape == (2, 778, 3)
    # a tip vertex takes its joint's gradient on top of the regressor's share; FreiHand joint 4 is RHD joint 1 (vertex 744)
    jr = mr.tables(torch.float64)["th_J_regressor"].numpy()
    kp = g.double().numpy()[:, list(mr.mano_ref.FREIHAND2RHD)]
    want = sum(jr[s, 744] * kp[:, d] for s, d in mr.mano_ref.WRAPPER_JOINT_MAP.items()) + kp[:, 4]
    assert np.abs(t[:, 744] - want).max() <= 1e-14
