"""Reference of the hand-mesh reverse tests: the float64 autograd of the committed CPU restatement (oracle.network_ref.decode for the normalised
mesh, oracle.mano_ref.wrapper_forward for the mesh in mm, `joints` and `mano_joints`), the inputs of every case, the error measure and the
bounds.  A case's bound is four times the same measure of the same restatement run in float32 on the CPU against float64 (F32_DEV below,
measured by f32_deviation; tests/test_mano_verts_bwd_host.py re-measures it) - the rule of the silhouette and Chamfer tests."""
import functools

import numpy as np
import torch

from mhentropy_amd import synth
from oracle import mano_ref, network_ref

NV = 778
TIPS = (745, 317, 444, 556, 673)                  # the five tip vertices of the joint pass: they reach root, bone or centre
ONE_HOT = (0, 777, 768) + TIPS                    # first vertex, last lane and first vertex of the ragged tile, the tips


@functools.lru_cache(None)
def tables(dtype):
    return mano_ref.tables_from_numpy(synth.mano_tables(0), dtype=dtype)


def make_z(R, seed=0):
    """z ~ N(0,1) with th45 scaled by 0.5; row 0 has theta = 0 (all 48), row 1 has th3 = 0"""
    g = torch.Generator().manual_seed(1000 + seed)
    z = torch.randn(R, 61, generator=g, dtype=torch.float64)
    z[:, 3:48] *= 0.5
    z[0, :48] = 0
    if R > 1:
        z[1, :3] = 0
    return z.float()


def random_g(R, seed, cols=NV * 3):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(R, cols, generator=g, dtype=torch.float64).float()


def one_hot_g(R, v):
    """dL/dverts = a different non-zero vector per row at vertex v, zero elsewhere"""
    g = torch.zeros(R, NV, 3)
    g[:, v] = random_g(R, 77 + v, 3)
    return g


# name -> (R, mm, kind of g_verts, with g_joints_mm)
CASES = {}
for _R in (1, 33, 70):
    for _mm in (0, 1):
        CASES[f"random_R{_R}_mm{_mm}"] = (_R, _mm, "random", False)
for _v in ONE_HOT:
    for _mm in (0, 1):
        CASES[f"onehot_v{_v}_mm{_mm}"] = (6, _mm, _v, False)
CASES["joints_alone_mm1"] = (6, 1, "zero", True)
CASES["joints_and_verts_mm1"] = (6, 1, "random", True)
CASES["joints_and_verts_mm0"] = (6, 0, "random", True)


def inputs(name):
    """(z [R,61], g_verts [R,778,3], g_joints_mm [R,63] | None, mm), all float32"""
    R, mm, kind, with_j = CASES[name]
    z = make_z(R)
    if kind == "random":
        gv = random_g(R, 1).view(R, NV, 3)
    elif kind == "zero":
        gv = torch.zeros(R, NV, 3)
    else:
        gv = one_hot_g(R, kind)
    return z, gv, (random_g(R, 2, 63) if with_j else None), mm


def mesh_and_joints(z, mm, dtype):
    """(verts of the mode [R,778,3], joints_mm [R,21,3] = the wrapper's mano_joints) of the restatement in `dtype`"""
    tb = tables(dtype)
    out = mano_ref.wrapper_forward(tb, z[:, :48], z[:, 48:58])
    verts = out["mesh"] if mm else network_ref.decode(tb, z)["verts"]
    return verts, out["mano_joints"]


def grad_z(z, g_verts, g_joints_mm, mm, dtype=torch.float64):
    """d/dz of <g_verts, verts> + <g_joints_mm, joints_mm> by autograd, as float64 numpy [R,61]"""
    zz = z.to(dtype).clone().requires_grad_(True)
    verts, joints = mesh_and_joints(zz, mm, dtype)
    total = (verts * g_verts.to(dtype)).sum()
    if g_joints_mm is not None:
        total = total + (joints.reshape(z.shape[0], 63) * g_joints_mm.to(dtype)).sum()
    (g,) = torch.autograd.grad(total, zz)
    return g.double().numpy()


@functools.lru_cache(None)
def reference(name):
    z, gv, gj, mm = inputs(name)
    return grad_z(z, gv, gj, mm)


def row_error(g_z, ref):
    """per row, max |g_z - ref| / max |ref|"""
    g_z, ref = np.asarray(g_z, np.float64), np.asarray(ref, np.float64)
    return np.abs(g_z - ref).max(1) / np.abs(ref).max(1)


def f32_deviation(name):
    """the measure of the float32 restatement against the float64 one: the largest row of the case"""
    z, gv, gj, mm = inputs(name)
    return float(row_error(grad_z(z, gv, gj, mm, torch.float32), reference(name)).max())


# f32_deviation(name) of every case, measured on the CPU
F32_DEV = {
    "random_R1_mm0": 1.85e-07, "random_R1_mm1": 1.35e-07, "random_R33_mm0": 1.08e-06, "random_R33_mm1": 7.16e-07,
    "random_R70_mm0": 1.90e-06, "random_R70_mm1": 7.80e-07,
    "onehot_v0_mm0": 8.20e-07, "onehot_v0_mm1": 3.38e-07, "onehot_v777_mm0": 3.62e-07, "onehot_v777_mm1": 2.71e-07,
    "onehot_v768_mm0": 5.50e-07, "onehot_v768_mm1": 3.86e-07, "onehot_v745_mm0": 1.66e-07, "onehot_v745_mm1": 3.74e-07,
    "onehot_v317_mm0": 4.46e-07, "onehot_v317_mm1": 3.37e-07, "onehot_v444_mm0": 8.42e-07, "onehot_v444_mm1": 6.49e-07,
    "onehot_v556_mm0": 3.29e-07, "onehot_v556_mm1": 3.34e-07, "onehot_v673_mm0": 5.36e-07, "onehot_v673_mm1": 5.93e-07,
    "joints_alone_mm1": 3.99e-07, "joints_and_verts_mm1": 1.08e-06, "joints_and_verts_mm0": 4.66e-07,
}
BOUND = {k: 4 * v for k, v in F32_DEV.items()}


def wrapper_reference(theta, beta, a, b, c, dtype=torch.float64):
    """(d/dtheta, d/dbeta) of (mesh a).sum() + (joints b).sum() + (mano_joints c).sum() of the restatement, float64 numpy"""
    th, bt = theta.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    out = mano_ref.wrapper_forward(tables(dtype), th, bt)
    total = (out["mesh"] * a.to(dtype)).sum() + (out["joints"] * b.to(dtype)).sum() + (out["mano_joints"] * c.to(dtype)).sum()
    g_th, g_bt = torch.autograd.grad(total, (th, bt))
    return g_th.double().numpy(), g_bt.double().numpy()


def wrapper_inputs(R=6):
    """(theta, beta, a, b, c) of the ManoLayer.forward test: the weights of mesh, joints and mano_joints"""
    z = make_z(R)
    return (z[:, :48].contiguous(), z[:, 48:58].contiguous(), random_g(R, 5).view(R, NV, 3), random_g(R, 6, 63).view(R, 21, 3),
            random_g(R, 7, 63).view(R, 21, 3))


def wrapper_f32_deviation():
    args = wrapper_inputs()
    ref = np.concatenate(wrapper_reference(*args), 1)
    return float(row_error(np.concatenate(wrapper_reference(*args, dtype=torch.float32), 1), ref).max())


F32_DEV_WRAPPER = 7.77e-07          # wrapper_f32_deviation(), measured on the CPU


def regress_transpose(g_joints):
    """float64 transpose of the wrapper's re-regression: g_joints [R,21,3] -> g_verts [R,778,3]"""
    R = g_joints.shape[0]
    v = torch.zeros(R, NV, 3, dtype=torch.float64, requires_grad=True)
    jr = tables(torch.float64)["th_J_regressor"].t()
    reg = torch.stack([v[:, :, c].matmul(jr) for c in range(3)], 2)
    kp = [None] * 21
    for src, dst in mano_ref.WRAPPER_JOINT_MAP.items():
        kp[dst] = reg[:, src]
    for dst, vid in mano_ref.WRAPPER_TIP_VERTS.items():
        kp[dst] = v[:, vid]
    joints = torch.stack(kp, 1)[:, list(mano_ref.FREIHAND2RHD)]
    (g,) = torch.autograd.grad((joints * g_joints.double()).sum(), v)
    return g.numpy()
