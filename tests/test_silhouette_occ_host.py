"""CPU: the occlusion-aware silhouette distance's restatement (tests/silhouette_occ_ref.py) against the one without occluder, finite
differences and its own definition; the seeds of the GPU tests; and the argument checks of criteria / MHEnt / LossTerms, which raise on CPU
tensors before any device call; synth.object_masks."""
import numpy as np
import pytest
import torch

import silhouette_occ_ref as so
import silhouette_ref as sr
from mhentropy_amd import criteria, harness, synth
from mhentropy_amd.loss_terms import LossTerms


@pytest.mark.parametrize("name", ["v65_s8_35_rows", "v5_s8_float_mask_2x"])
def test_all_zero_occluder_is_the_restatement_without_one(name):
    case, ref = sr.reference(name)
    S = sr.CASES[name]["S"]
    zero = np.zeros(case["mask"].shape, bool)
    got = so.silhouette(case["verts"], case["logs_t"], case["mask"], zero, S)
    for k in ("dist", "inside", "cover", "idx_v", "idx_m", "pixels", "count", "d_v", "d_m"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert np.array_equal(got["count_all"], ref["count"])
    g = sr.g_dist_of(name, ref["dist"].shape)
    for a, b in zip(so.grad(case["verts"], case["logs_t"], case["mask"], zero, S, g), sr.grad(case["verts"], case["logs_t"], case["mask"], S, g)):
        assert np.array_equal(a, b)


def test_gradient_agrees_with_finite_differences_of_its_own_distance():
    """central differences (step 1e-6) of the f64 distance in 40 drawn coordinates; a coordinate whose step crosses a tie would show as a
    large error - the argmins at both ends are checked to be the same"""
    name = "v5_s8"
    case, ref = so.reference(name)
    S = so.CASES[name]["S"]
    g = so.g_dist_of(name, ref["dist"].shape).astype(np.float64)
    gv, gl = so.grad(case["verts"], case["logs_t"], case["mask"], case["occluder"], S, g)
    assert np.abs(gv).max() > 0 and (ref["idx_v"] >= ref["count"][None, :, None]).any()          # some vertex chose an occluder pixel
    rng = np.random.default_rng(0)
    f = lambda v, lt: so.silhouette(v, lt, case["mask"], case["occluder"], S)
    for _ in range(40):
        n, b = rng.integers(2), rng.integers(3)
        on_verts = rng.random() < 0.7
        pos = (n, b, rng.integers(5), rng.integers(2)) if on_verts else (n, b, rng.integers(3))
        v, lt = [np.array(case["verts"], np.float64) for _ in range(2)], [np.array(case["logs_t"], np.float64) for _ in range(2)]
        for sign, k in ((-1, 0), (1, 1)):
            (v if on_verts else lt)[k][pos] += sign * 1e-6
        lo, hi = f(v[0], lt[0]), f(v[1], lt[1])
        if not (np.array_equal(lo["idx_v"], hi["idx_v"]) and np.array_equal(lo["idx_m"], hi["idx_m"])):
            continue
        fd = float((g * (hi["dist"] - lo["dist"])).sum() / 2e-6)
        want = float((gv if on_verts else gl)[pos])
        assert abs(fd - want) <= 1e-6 * max(1.0, abs(want)), (pos, fd, want)


def test_occluder_that_is_everything_else_makes_inside_zero():
    name = "v257_s8"
    case, _ = so.reference(name)
    mask = np.array(case["mask"])
    verts = np.array(case["verts"]) * 0.3          # every projected vertex inside the image
    got = so.silhouette(verts, case["logs_t"], mask, ~mask, 8)
    assert (got["count_all"] == 64).all() and (got["count"] > 0).all() and (got["inside"] == 0).all() and (got["cover"] > 0).all()
    without = so.silhouette(verts, case["logs_t"], mask, np.zeros_like(mask), 8)
    assert (without["inside"] > 0).all() and np.array_equal(without["cover"], got["cover"])


def test_a_pixel_of_both_masks_is_listed_once_in_the_hand_section():
    S = 4
    mask, occ = np.zeros((2, S, S), bool), np.zeros((2, S, S), bool)
    mask[0, 1, 1:3] = True
    occ[0, 1, 2:4] = occ[0, 0, 0] = True          # (1, 2) is in both; the occluder's own are (0, 0) and (1, 3), row-major
    occ[1] = True                                  # image 1: no hand
    pixels, count, count_all = so.pixel_list(mask, occ, S)
    assert count.tolist() == [2, 0] and count_all.tolist() == [4, 16]
    assert pixels[0, :5].tolist() == [(1 << 16) | 1, (1 << 16) | 2, 0, (1 << 16) | 3, -1]
    assert pixels[1].tolist() == [(i << 16) | j for i in range(S) for j in range(S)]
    out = so.silhouette(np.zeros((1, 2, 3, 3), np.float32), np.zeros((1, 2, 3), np.float32), mask, occ, S)
    assert out["dist"][0, 1] == 0 and (out["idx_v"][0, 1] == -1).all()          # no visible hand: nothing, whatever the occluder holds


@pytest.mark.parametrize("name", list(so.CASES))
def test_seeds_make_the_f32_restatement_attain_the_f64_indices(name):
    """the inputs of the GPU tests: the f32 restatement attains exactly the f64 indices (so the kernel's are compared exactly) and stays
    within the recorded deviations, of which the kernel's bounds are four times"""
    fwd, rev, same = so.f32_deviation(name)
    print(f"{name}: f32 restatement vs f64: forward {fwd:.3e} (recorded {so.F32_FWD[name]:.3e}), reverse {rev:.3e} (recorded {so.F32_REV[name]:.3e})")
    assert same
    assert fwd <= so.F32_FWD[name] and rev <= so.F32_REV[name]
    case, ref = so.reference(name)
    assert (ref["count_all"] > ref["count"]).all()          # every image has an occluder section
    if name == "v257_s64_two_rounds":
        assert (ref["count"] > 1024).all()


# ---- argument checks: CPU tensors, nothing launched --------------------------------------------------------------------------------------------
def _cpu_operands(N=2, B=3, V=5, H=8):
    return torch.zeros(N, B, V, 3), torch.zeros(N, B, 3), torch.ones(B, H, H, dtype=torch.bool)


@pytest.fixture
def no_launch(monkeypatch):
    from mhentropy_amd import ops

    def refuse(entry, *args):
        raise AssertionError(f"{entry} was launched")
    monkeypatch.setattr(ops, "launch", refuse)


@pytest.mark.parametrize("shape", [(2, 8, 8), (3, 16, 16), (3, 8), (3, 8, 8, 1), (3, 8, 4)])
def test_silhouette_dist_refuses_a_misshapen_occluder(no_launch, shape):
    v, lt, mask = _cpu_operands()
    with pytest.raises(ValueError, match="occluder"):
        criteria.silhouette_dist(v, lt, mask, size=8, occluder=torch.zeros(shape, dtype=torch.bool))
    with pytest.raises(ValueError, match="occluder"):
        criteria.silhouette_dist(v, lt, mask, size=8, occluder=np.zeros(shape, bool))


def test_silhouette_select_needs_the_object_mask(no_launch):
    v, lt, mask = _cpu_operands()
    out = {"verts": v.reshape(2, 3, -1), "logs_t": lt}
    with pytest.raises(ValueError, match="object_mask"):
        criteria.silhouette_select(out, {"hand_mask": mask}, occluder=True)
    with pytest.raises(ValueError, match="occluder"):
        criteria.silhouette_select(out, {"hand_mask": mask, "object_mask": mask[:2]}, size=8, occluder=True)
    with pytest.raises(ValueError, match="occluder"):
        criteria.silhouette_select(out, {"hand_mask": mask}, size=8, occluder=mask[:, :4])


@pytest.fixture(scope="module")
def model():
    return harness.build_mhent(backbone="resnet18", h_dims=(64, 64), num_steps=2, tables=synth.mano_tables(0))


def _target(B=3):
    _, yn = synth.batch(1, B, with_image=False)
    yn["hand_mask"], yn["object_mask"] = synth.object_masks(1, synth.hand_masks(1, B, H=128, with_image=False))
    return {k: torch.as_tensor(v) for k, v in yn.items()}


def test_get_loss_needs_the_object_mask_and_checks_its_shape(no_launch, model):
    y = _target()
    x = torch.zeros(3, 3, 64, 64)
    without = {k: v for k, v in y.items() if k != "object_mask"}
    for fn in (lambda yy, **kw: model.get_loss(x, yy, sil_w=1.0, **kw), lambda yy, **kw: model.sil_operands(yy, 1.0, 3, **kw),
               lambda yy, **kw: LossTerms(model, yy, None, None, 1.0, 3, **kw)):
        with pytest.raises(ValueError, match="object_mask"):
            fn(without, sil_occluder=True)
        for bad in (y["object_mask"][:2], y["object_mask"][:, :64, :64], y["object_mask"][0]):
            with pytest.raises(ValueError, match="occluder"):
                fn(dict(y, object_mask=bad), sil_occluder=True)
    model.sil_occluder = True          # the attribute is the argument's default
    try:
        with pytest.raises(ValueError, match="object_mask"):
            model.get_loss(x, without, sil_w=1.0)
        assert model.sil_operands(without, 0.0) == (0.0, None)          # the term off: nothing is asked of the target
    finally:
        model.sil_occluder = False


def test_loss_terms_carry_the_switch(monkeypatch, model):
    from mhentropy_amd import ops
    calls = []
    monkeypatch.setattr(ops, "launch", lambda entry, *args: calls.append((entry, args)))
    monkeypatch.setattr(ops, "_chk", lambda t, *a, **k: t)
    y = _target()
    on = LossTerms(model, y, None, None, 1.5, 3, sil_occluder=True)
    assert on.weights() == {"mods": ops.MODS_UV, "chamfer_w": 0.0, "sil_w": 1.5, "sil_occluder": True} and on.sil_occluder
    assert [c[0] for c in calls] == ["mhe_silhouette_pixels_occ"] and len(on.sil) == 2 and on.sil_all is not None
    assert on.sil_all.shape == (3,) and on.sil_all.dtype == torch.int32
    del calls[:]
    off = LossTerms(model, y, None, None, 1.5, 3)
    assert "sil_occluder" not in off.weights() and not off.sil_occluder and off.sil_all is None
    assert [c[0] for c in calls] == ["mhe_silhouette_pixels"]
    term_off = LossTerms(model, y, None, None, 0.0, 3, sil_occluder=True)          # without the term there is nothing to occlude
    assert term_off.weights() == {"mods": ops.MODS_UV, "chamfer_w": 0.0, "sil_w": 0.0} and term_off.sil is None
    # the loss pass' forward reaches the _occ entry with the list's second count behind the first
    del calls[:]
    o = on.joints(torch.zeros(12, 45), torch.zeros(3, 16), torch.zeros(8))
    on.reduce(o, torch.zeros(12), 4, 3)
    entry, args = [c for c in calls if c[0].startswith("mhe_silhouette")][0]
    assert entry == "mhe_silhouette_dist_occ_f32" and args[4] is on.sil_all and args[3] is on.sil[1]
    from mhentropy_amd import _lib
    assert len(args) == len(_lib.SIGNATURES[entry][1]) - 1
    for e in ("mhe_silhouette_pixels_occ", "mhe_silhouette_dist_bwd_occ_f32", "mhe_silhouette_dist_grad_occ_f32"):
        assert e in _lib.SIGNATURES


# ---- synthetic occluders ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 7])
def test_object_masks_are_seeded_disjoint_and_leave_a_hand(seed):
    hand0 = synth.hand_masks(seed, 4, H=64, with_image=False)
    hand, obj = synth.object_masks(seed, hand0)
    again = synth.object_masks(seed, hand0)
    assert np.array_equal(hand, again[0]) and np.array_equal(obj, again[1])
    other = synth.object_masks(seed + 1, hand0)
    assert not np.array_equal(obj, other[1])
    assert hand.dtype == bool and obj.dtype == bool and hand.shape == obj.shape == (4, 64, 64)
    assert not (hand & obj).any()
    assert hand.reshape(4, -1).any(1).all() and obj.reshape(4, -1).any(1).all()
    assert np.array_equal(hand | (obj & hand0), hand0) and (obj & hand0).reshape(4, -1).any(1).all()          # the occluder covers part of the hand
    drawn = synth.object_masks(seed, B=4, H=64, with_image=False)          # without a mask: the seed's own hand masks
    assert np.array_equal(drawn[0], hand) and np.array_equal(drawn[1], obj)
    tiny = np.zeros((1, 8, 8), bool)
    tiny[0, 3, 3] = True
    h1, o1 = synth.object_masks(seed, tiny)
    assert h1.sum() == 1 and not (h1 & o1).any()
