"""CPU: the dispatch of loss_terms.LossTerms and ops.mano_joints / mano_joints_bwd with ops.launch replaced by a recorder - which C entry
every combination of get_loss's optional terms reaches, forward and reverse, with how many arguments and which scalar tail; nothing is
launched.  B = 3, N = 4: R = 12 rows, no multiple of the 16-row wave group; VO = 5 object vertices."""
import itertools
import types

import pytest
import torch

from mhentropy_amd import _lib, harness, ops, synth, train
from mhentropy_amd.loss_terms import LossTerms

B, N, VO = 3, 4, 5
R = N * B
B2D, B3D, ALPHA, CW, SW = 0.07, 0.04, 33.0, 10.0, 1.5
MODS = [None, ["uv"], ["xyz"], ["xyz", "uv"]]


@pytest.fixture(scope="module")
def model():
    m = harness.build_mhent(backbone="resnet18", h_dims=(64, 64), num_steps=2, tables=synth.mano_tables(0))
    m.b_2d, m.b_3d, m.th45_ref_alpha = B2D, B3D, ALPHA
    return m


@pytest.fixture(scope="module")
def target():
    _, yn = synth.batch(1, B, with_image=False)
    yn.update(synth.object_targets(1, B, VO=VO, with_count=True))
    yn["hand_mask"] = synth.hand_masks(1, B, H=128, with_image=False)
    return {k: torch.as_tensor(v) for k, v in yn.items()}


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(ops, "launch", lambda entry, *args: rec.append((entry, args)))
    monkeypatch.setattr(ops, "_chk", lambda t, *a, **k: t)
    return rec


def _rows():
    return torch.zeros(R, 45), torch.zeros(B, 16), torch.zeros(8)


def _name(bits, chamfer, bwd):
    kind = "_chamfer" if chamfer else ("" if bits == ops.MODS_UV else "_mods")
    return f"mhe_mano_joints{kind}{'_bwd' if bwd else ''}_f32"


@pytest.mark.parametrize("mods,chamfer,sil", list(itertools.product(MODS, (False, True), (False, True))))
def test_every_combination_reaches_its_entry_with_its_arguments(model, target, calls, mods, chamfer, sil):
    bits = ops.mods_bits(mods)
    terms = LossTerms(model, target, mods, CW * chamfer, SW * sil, B)
    assert [c[0] for c in calls] == ["mhe_silhouette_pixels"] * sil            # the construction's one launch, with the term on only
    assert (terms.bits, terms.chamfer_w, terms.sil_w) == (bits, CW * chamfer, SW * sil) and (terms.chamfer is not None) == chamfer
    assert (terms.sil is not None) == sil and terms.weights() == {"mods": bits, "chamfer_w": CW * chamfer, "sil_w": SW * sil}
    assert terms.keys() == ["th_norm", "bt_norm", "q_log_p_z_giv_y", "log_p", "h_q_z_giv_i"] + ["chamfer"] * chamfer + ["silhouette"] * sil
    del calls[:]
    th45, det, blob = _rows()
    o = terms.joints(th45, det, blob)
    g = torch.zeros(B)
    g45, gdet = terms.joints_bwd(th45, det, blob, g, N)                        # allocates, sums over the hypotheses
    out = (torch.zeros(R, 45), torch.zeros(R, 16))
    assert terms.joints_bwd(th45, det, blob, g, N, out=out) == out             # the caller's buffers, the rows unsummed
    assert [c[0] for c in calls] == [_name(bits, chamfer, False), _name(bits, chamfer, True), "mhe_sum_over_hypotheses_f32", _name(bits, chamfer, True)]
    for entry, args in calls:
        assert len(args) == len(_lib.SIGNATURES[entry][1]) - 1, entry          # launch() appends the stream
    # outputs: the silhouette term adds z to the two the loss reads and changes nothing else
    assert {k for k, v in o.items() if v is not None} == {"log_p", "norms"} | ({"z"} if sil else set()) | ({"chamfer"} if chamfer else set())
    assert g45.shape == (R, 45) and gdet.shape == (B, 16)
    # scalar tails, as the parent passed them
    uv_only = not chamfer and bits == ops.MODS_UV
    lik = (B2D, ALPHA) if uv_only else (bits, B2D, B3D, ALPHA)
    shape = (R, B) + ((VO,) if chamfer else ())
    fwd, bwd = calls[0][1], calls[1][1]
    assert fwd[-len(shape + lik) - 2:] == shape + lik + (0, 256.0)
    rev = shape + lik + (1.0 / N,) + ((CW,) if chamfer else ())
    assert bwd[-len(rev):] == rev and calls[3][1][-len(rev):] == rev
    assert calls[3][1][-len(rev) - 2] is out[0] and calls[3][1][-len(rev) - 1] is out[1] and bwd[-len(rev) - 3] is g
    # targets: crop_uv / pose3d only where the bit set reads them (a null pointer otherwise); the plain entry has no pose3d slot
    for args in (fwd, bwd):
        assert (args[2] is not None) == bool(bits & ops.MODS_UV) and args[3] is not None
        if not uv_only:
            assert (args[4] is not None) == bool(bits & ops.MODS_XYZ) and args[5] is blob
        if chamfer:
            assert all(a is b for a, b in zip(args[6:10], terms.chamfer))


def test_reduce_assembles_the_dictionary_in_key_order(model, target, calls):
    terms = LossTerms(model, target, ["xyz", "uv"], CW, SW, B)
    o = terms.joints(*_rows())
    del calls[:]
    out = terms.reduce(o, torch.zeros(R), N, B)
    assert list(out) == terms.keys() and all(v.shape == ((R,) if k.endswith("norm") else (B,)) for k, v in out.items())
    assert [c[0] for c in calls] == ["mhe_elbo_reduce_f32", "mhe_elbo_reduce_f32", "mhe_mano_verts_f32", "mhe_silhouette_dist_f32", "mhe_elbo_reduce_f32"]
    assert terms.sil_verts.shape == (R, 778, 3) and terms.sil_logs_t.shape == (R, 3)
    shared = []
    out2 = terms.reduce(o, None, N, B, share=lambda q, h, ch: shared.append((q, h, ch)) or (q + 1, h, ch))
    assert len(shared) == 1 and list(out2) == terms.keys()


def test_ops_mano_joints_keeps_the_4_term_and_5_term_entries(calls):
    th45, det, blob = _rows()
    cu, vis = torch.zeros(B, 42), torch.zeros(B, 21)
    o4 = ops.mano_joints(th45, det, blob, cu, vis, mods=None)
    o5 = ops.mano_joints(th45, det, blob, cu, vis, mods=ops.MODS_UV)
    assert [c[0] for c in calls] == ["mhe_mano_joints_f32", "mhe_mano_joints_mods_f32"]
    assert o4["terms"].shape == (R, 4) and o5["terms"].shape == (R, 5)
    ov = ops.mano_joints(th45, det, blob, cu, vis, want=("z", "mesh_mm"))
    assert calls[-1][0] == "mhe_mano_decode_f32" and calls[-1][1][-1] == 1 and ov["mesh_mm"].shape == (R, 778, 3) and ov["xyz"] is None
    for entry, args in calls:
        assert len(args) == len(_lib.SIGNATURES[entry][1]) - 1, entry
    for kw in (dict(mods=ops.MODS_UV), dict(chamfer=(torch.zeros(B), torch.zeros(B, 3), torch.zeros(B, VO, 3), None))):
        with pytest.raises(ValueError, match="uv-only pass"):
            ops.mano_joints(th45, det, blob, cu, vis, want=("verts",), **kw)
    with pytest.raises(ValueError, match="one mesh per call"):
        ops.mano_joints(th45, det, blob, cu, vis, want=("verts", "mesh_mm"))
    assert len(calls) == 3


def test_autograd_bridge_answers_one_gradient_per_input():
    """_LossFn.backward: a None for every input of forward that is no parameter, then the parameters' gradients"""
    import inspect
    names = list(inspect.signature(train._LossFn.forward).parameters)
    assert names[0] == "ctx" and names[-1] == "params"
    params = [object(), object(), object()]
    tr = types.SimpleNamespace(backward=lambda g: None, grad_of=lambda p: ("grad", p), arena=types.SimpleNamespace(params=params))
    ctx = types.SimpleNamespace(trainer=tr, keys=["th_norm", "log_p"], needs_input_grad=(False,) * (len(names) - 2) + (True,) * len(params))
    grads = train._LossFn.backward(ctx, None, None)
    assert grads == (None,) * (len(names) - 2) + tuple(("grad", p) for p in params)
