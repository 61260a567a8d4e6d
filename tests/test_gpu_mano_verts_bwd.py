"""MI355X: the reverse of the hand mesh (mhe_mano_verts_bwd_f32 = csrc/mano_skin_bwd.hip + mano_verts_bwd_kernel of csrc/mano_bwd.hip,
mhe_mano_regress_joints_bwd_f32) and its autograd surface (ManoLayer.verts, ManoLayer.forward under grad) against the float64 autograd of
the CPU restatement (tests/mano_bwd_ref.py).  Measure: per row, max |g_z - g_z64| / max |g_z64|; a case's bound is four times the same
measure of the float32 restatement on the CPU (mano_bwd_ref.F32_DEV: 1.4e-7 .. 1.9e-6 over the cases).
Measured on the MI355X (each test prints its figure, `pytest -s`): kernel error 8.7e-8 .. 8.9e-7 over the 25 cases against bounds of
5.4e-7 .. 7.6e-6; ManoLayer.forward under grad 3.4e-7 (bound 3.1e-6); silhouette_dist -> z 2.8e-6 (bound 7.9e-6), chamfer_dist -> z 2.0e-6
(bound 7.1e-6); the joint re-regression's transpose 9.5e-8 absolute at max |ref| 2.45."""
import ctypes as C

import numpy as np
import pytest
import torch

import mano_bwd_ref as mr
from mhentropy_amd import _lib, criteria, mano_pack, ops, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blob(gpu_lib):
    t = synth.mano_tables(0)
    return torch.from_numpy(mano_pack.pack_tables(t["shapedirs"], t["posedirs"], t["v_template"], t["J_regressor"], t["weights"],
                                                  t["hands_components"][:45], t["hands_mean"])).cuda()


@pytest.fixture(scope="module")
def layer(gpu_lib):
    from mhentropy_amd.ManoLayer import ManoLayer
    return ManoLayer(skeidx="RHD", flat_hand_mean=False, ncomps=45, use_pca=True, tables=synth.mano_tables(0)).cuda()


def _run(name, blob):
    z, gv, gj, mm = mr.inputs(name)
    return ops.mano_verts_bwd(z.cuda(), blob, gv.cuda(), mm=bool(mm), g_joints_mm=None if gj is None else gj.cuda())


def _check(what, g_z, ref, bound):
    err = mr.row_error(g_z, ref)
    print(f"{what}: kernel error {err.max():.3e} (row {int(err.argmax())}), bound {bound:.3e}")
    assert np.isfinite(g_z).all() and err.max() <= bound, (what, err.max(), bound)


@pytest.mark.parametrize("name", list(mr.CASES))
def test_g_z_matches_the_f64_autograd(blob, name):
    g_z = _run(name, blob).cpu().numpy()
    assert (g_z[:, 58:] == 0).all()                       # the camera columns are written, as zeros
    _check(name, g_z, mr.reference(name), mr.BOUND[name])


@pytest.mark.parametrize("mm", [False, True])
def test_zero_gradient_in_zero_out_and_determinism(blob, mm):
    z = mr.make_z(33).cuda()
    zero = ops.mano_verts_bwd(z, blob, torch.zeros(33, 778, 3, device="cuda"), mm=mm)
    assert (zero == 0).all()
    gv = mr.random_g(33, 1).view(33, 778, 3).cuda()
    a, b = ops.mano_verts_bwd(z, blob, gv, mm=mm), ops.mano_verts_bwd(z, blob, gv, mm=mm)
    assert torch.equal(a, b)
    # poison: g_verts is the leading part of a larger buffer whose rest is NaN - nothing past its end is read
    big = torch.full((40 * 778 * 3,), float("nan"), device="cuda")
    big[:33 * 778 * 3] = gv.reshape(-1)
    c = ops.mano_verts_bwd(z, blob, big[:33 * 778 * 3].view(33, 778, 3), mm=mm)
    assert torch.isfinite(c).all() and torch.equal(a, c)


def test_captured_graph_replays_the_same_bits(blob):
    z, gv = mr.make_z(33).cuda(), mr.random_g(33, 1).view(33, 778, 3).cuda()
    eager = ops.mano_verts_bwd(z, blob, gv)
    g_z = torch.empty(33, 61, device="cuda")
    ws = torch.empty(_lib.lib().mhe_mano_verts_bwd_workspace_floats(33), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.launch("mhe_mano_verts_bwd_f32", z, blob, gv, None, g_z, ws, 33, 0)          # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.launch("mhe_mano_verts_bwd_f32", z, blob, gv, None, g_z, ws, 33, 0)
    for _ in range(2):
        g_z.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_z, eager)


def test_regress_joints_bwd_is_the_transpose(blob):
    R = 5
    gj = mr.random_g(R, 3, 63).view(R, 21, 3)
    ref = mr.regress_transpose(gj)
    # every output is a 16-term fmaf chain over f32 table entries plus at most one addition: (18 roundings) 2^-24 sum |terms|
    jr = np.abs(synth.mano_tables(0)["J_regressor"].astype(np.float64))          # [16,778]
    kp = np.abs(gj.double().numpy()[:, list(mr.mano_ref.FREIHAND2RHD)])          # FreiHand order (the reorder is an involution)
    mag = np.einsum("jv,rjc->rvc", jr, kp[:, [mr.mano_ref.WRAPPER_JOINT_MAP[j] for j in range(16)]])
    for dst, vid in mr.mano_ref.WRAPPER_TIP_VERTS.items():
        mag[:, vid] += kp[:, dst]
    tol = 18 * 2.0 ** -24 * mag
    out = ops.mano_regress_joints_bwd(gj.cuda(), blob)
    err = np.abs(out.cpu().numpy() - ref)
    print(f"regress_joints_bwd: max error {err.max():.3e}, max |ref| {np.abs(ref).max():.3e}")
    assert (err <= tol).all() and np.abs(ref).max() > 0.1
    base = mr.random_g(R, 4).view(R, 778, 3).cuda()
    acc = ops.mano_regress_joints_bwd(gj.cuda(), blob, out=base.clone())
    assert torch.equal(acc, base + out)                   # accumulate = 1: one more addition, in f32
    assert torch.equal(out, ops.mano_regress_joints_bwd(gj.cuda(), blob))


def test_mano_layer_forward_under_grad(layer):
    R = 6
    theta, beta, a, b, c = mr.wrapper_inputs(R)
    th, bt = theta.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    out = layer(beta=bt, theta=th)
    assert all(out[k].grad_fn is not None for k in ("mesh", "joints", "mano_joints"))
    ((out["mesh"] * a.cuda()).sum() + (out["joints"] * b.cuda()).sum() + (out["mano_joints"] * c.cuda()).sum()).backward()
    ref = np.concatenate(mr.wrapper_reference(theta, beta, a, b, c), 1)
    _check("ManoLayer.forward under grad", np.concatenate([th.grad.cpu().numpy(), bt.grad.cpu().numpy()], 1), ref, 4 * mr.F32_DEV_WRAPPER)
    # without grad: today's launches, today's bits
    plain = layer(beta=beta.cuda(), theta=theta.cuda())
    det = torch.zeros(R, 16, device="cuda")
    det[:, :3], det[:, 3:13] = theta[:, :3].cuda(), beta.cuda()
    o = ops.mano_joints(theta[:, 3:].contiguous().cuda(), det, layer.table_blob(), want=("joints_mm", "mesh_mm"))
    assert plain["mesh"].grad_fn is None and not plain["mesh"].requires_grad
    assert torch.equal(plain["mesh"], o["mesh_mm"]) and torch.equal(plain["mano_joints"], o["joints_mm"].view(R, 21, 3))
    assert torch.equal(plain["joints"], ops.mano_regress_joints(o["mesh_mm"], layer.table_blob()))
    for k in ("mesh", "joints", "mano_joints"):
        assert torch.equal(out[k].detach(), plain[k]), k


def _end_to_end(layer, term):
    """z.grad of term(layer.verts(z)).sum() against term's own g_verts pushed through the f64 autograd; the bound is four times the f32
    restatement's deviation for that same g_verts"""
    N, B = 2, 2
    z0 = mr.make_z(N * B, seed=3)
    z = z0.cuda().requires_grad_(True)
    verts = layer.verts(z)
    seen = []
    verts.register_hook(lambda g: seen.append(g.detach().clone()))
    term(verts.view(N, B, 778, 3), z).sum().backward()
    gv = seen[0].cpu().view(N * B, 778, 3)
    assert gv.abs().max() > 0
    ref = mr.grad_z(z0, gv, None, 0)
    dev = float(mr.row_error(mr.grad_z(z0, gv, None, 0, torch.float32), ref).max())
    return z.grad.cpu().numpy(), ref, 4 * dev


def test_silhouette_dist_reaches_z(layer):
    mask = torch.zeros(2, 64, 64, dtype=torch.bool)
    mask[:, 20:44, 16:40] = True
    logs_t = torch.tensor([np.log(0.25), 0.05, -0.05]).float().expand(2, 2, 3).contiguous().cuda()
    g_z, ref, bound = _end_to_end(layer, lambda v, z: criteria.silhouette_dist(v, logs_t, mask.cuda()))
    _check("silhouette_dist -> z", g_z, ref, bound)


def test_chamfer_dist_reaches_z(layer):
    rng = np.random.default_rng(5)
    target = {"scale": torch.tensor([0.08, 0.1]).cuda(), "original_pose3d": torch.as_tensor(rng.normal(0, 30, (2, 21, 3)).astype(np.float32)).cuda(),
              "object_verts": torch.as_tensor(rng.normal(0, 60, (2, 200, 3)).astype(np.float32)).cuda()}
    g_z, ref, bound = _end_to_end(layer, lambda v, z: criteria.chamfer_dist(v, target))
    _check("chamfer_dist -> z", g_z, ref, bound)


def test_argument_errors(blob):
    L, R = _lib.lib(), 3
    z, gv, g_z = mr.make_z(R).cuda(), torch.zeros(R, 778, 3, device="cuda"), torch.empty(R, 61, device="cuda")
    ws = torch.empty(L.mhe_mano_verts_bwd_workspace_floats(R), device="cuda")
    A = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def bwd(z_=z, tb=blob, g=gv, out=g_z, w=ws, r=R):
        return L.mhe_mano_verts_bwd_f32(A(z_), A(tb), A(g), None, A(out), A(w), r, 0, None)
    for what, kw in {"null z": dict(z_=None), "null tables": dict(tb=None), "null g_verts": dict(g=None), "null g_z": dict(out=None),
                     "null workspace": dict(w=None), "R = 0": dict(r=0), "g_z overlaps z": dict(out=z), "workspace overlaps g_verts": dict(w=gv),
                     "g_z inside the workspace": dict(out=ws)}.items():
        assert bwd(**kw) == 1 and b"mhe_mano_verts_bwd_f32" in L.mhe_last_error(), what
    gj, out = torch.zeros(R, 21, 3, device="cuda"), torch.zeros(R, 778, 3, device="cuda")
    for what, args in {"null g_joints": (None, blob, out, R), "null g_verts": (gj, blob, None, R), "R = 0": (gj, blob, out, 0),
                       "overlap": (out, blob, out, R)}.items():
        assert L.mhe_mano_regress_joints_bwd_f32(A(args[0]), A(args[1]), A(args[2]), args[3], 0, None) == 1, what
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        ops.mano_verts_bwd(z.cpu(), blob, gv)
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        ops.mano_regress_joints_bwd(gj.cpu(), blob)
    with pytest.raises(_lib.MheError, match="expected shape"):
        ops.mano_verts_bwd(z, blob, torch.zeros(R, 777, 3, device="cuda"))
    with pytest.raises(_lib.MheError, match="expected torch.float32"):
        ops.mano_verts_bwd(z.double(), blob, gv)
    with pytest.raises(_lib.MheError, match="expected shape"):
        ops.mano_verts_bwd(z, blob, gv, g_joints_mm=torch.zeros(R, 21, 3, device="cuda"))
    with pytest.raises(_lib.MheError, match="expected shape"):
        ops.mano_regress_joints_bwd(gj, blob, out=out[:2])
