"""CPU: the host side of the silhouette training term, get_loss(sil_w=...) - the two new C entries (declared, exported, bound), the error
paths that must run before any launch, the keyword on every step surface, and the synthetic masks."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from mhentropy_amd import _lib, harness, ops, synth


def test_new_entries_are_declared_exported_and_bound():
    hdr = open(f"{ROOT}/include/mhe.h").read()
    L = _lib.lib()
    for name, nargs in (("mhe_silhouette_dist_grad_f32", 13), ("mhe_mano_z_grad_add_f32", 6)):
        assert re.search(rf"\bint {name}\(", hdr), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, (name, len(args))
        assert getattr(L, name).argtypes == args
    assert {"silhouette_dist_grad", "mano_z_grad_add"} <= set(dir(ops))
    assert "want_dist" in inspect.signature(ops.silhouette_dist_grad).parameters


def test_entries_refuse_bad_arguments_before_any_launch():
    """host memory stands in for device memory: every call must come back MHE_ERR_ARG (no launch, nothing written)"""
    L = _lib.lib()
    a = np.full(4096, 7.0, np.float32)
    before = a.copy()
    P = lambda off=0: C.c_void_p(a.ctypes.data + 4 * off)
    null = C.c_void_p(0)
    # verts 0..11, logs_t 16..18, pixels 32..35, count 40, g_dist 48, dist 56, g_verts 64..75, g_logs_t 80..82  (N = B = 1, V = 4, S = 2)
    good = [P(0), P(16), P(32), P(40), P(48), P(56), P(64), P(80)]
    shape = (1, 1, 4, 2)
    for i in (0, 1, 2, 3, 4, 6, 7):           # every pointer but dist
        args = list(good); args[i] = null
        assert L.mhe_silhouette_dist_grad_f32(*args, *shape, None) == 1 and b"null pointer" in L.mhe_last_error(), i
    for bad in ((0, 1, 4, 2), (1, 0, 4, 2), (1, 1, 0, 2), (1, 1, 779, 2), (1, 1, 4, 0), (1, 1, 4, 65)):
        assert L.mhe_silhouette_dist_grad_f32(*good, *bad, None) == 1, bad
    for i, j in ((6, 0), (7, 1), (5, 4), (6, 2), (7, 3)):          # an output on an input
        args = list(good); args[i] = good[j]
        assert L.mhe_silhouette_dist_grad_f32(*args, *shape, None) == 1 and b"overlap" in L.mhe_last_error(), (i, j)
    for i, j in ((6, 7), (5, 6), (5, 7)):                          # two outputs on each other
        args = list(good); args[i] = good[j]
        assert L.mhe_silhouette_dist_grad_f32(*args, *shape, None) == 1 and b"overlap" in L.mhe_last_error(), (i, j)
    # z_grad_add: g_z 0..60, g_logs_t 64..66, g_th45 128..172, g_det_rows 192..207  (R = 1)
    good = [P(0), P(64), P(128), P(192)]
    for i in (0, 2, 3):
        args = list(good); args[i] = null
        assert L.mhe_mano_z_grad_add_f32(*args, 1, None) == 1 and b"null pointer" in L.mhe_last_error(), i
    assert L.mhe_mano_z_grad_add_f32(*good, 0, None) == 1
    for args in ([P(0), P(64), P(32), P(192)], [P(0), P(64), P(128), P(60)], [P(0), P(64), P(128), P(160)], [P(0), P(130), P(128), P(192)]):
        assert L.mhe_mano_z_grad_add_f32(*args, 1, None) == 1 and b"overlap" in L.mhe_last_error()
    assert np.array_equal(a, before)


def _cpu_model():
    return harness.build_mhent(backbone="resnet18", h_dims=(64, 64), num_steps=2, tables=synth.mano_tables(0))


def test_get_loss_error_paths_run_before_any_launch():
    model = _cpu_model()
    assert model.sil_w == 0.0 and model.sil_size == 64
    assert "sil_w" in inspect.signature(model._reverse_kld).parameters
    x = torch.zeros(2, 3, 8, 8)
    y = {"crop_uv": torch.zeros(2, 42), "vis": torch.ones(2, 21), "hand_mask": torch.ones(2, 64, 64, dtype=torch.bool)}
    assert model.sil_operands(y) == (0.0, None) and model.sil_operands(y, 0.0) == (0.0, None) and model.sil_operands({}, 0.0) == (0.0, None)
    for fn in (lambda **kw: model.sil_operands(kw.pop("y"), kw["sil_w"], 2), lambda **kw: model.get_loss(x, kw["y"], sil_w=kw["sil_w"]),
               lambda **kw: model._reverse_kld(kw["y"], x, sil_w=kw["sil_w"])):
        with pytest.raises(ValueError, match="sil_w"):
            fn(y=y, sil_w=-1.0)
        with pytest.raises(ValueError, match="sil_w"):
            fn(y=y, sil_w=float("nan"))
        with pytest.raises(ValueError, match="hand_mask"):
            fn(y={k: v for k, v in y.items() if k != "hand_mask"}, sil_w=1.0)
        for bad in (torch.ones(64, 64, dtype=torch.bool), torch.ones(2, 64, 32, dtype=torch.bool), torch.ones(2, 1, 64, 64, dtype=torch.bool),
                    torch.ones(3, 64, 64, dtype=torch.bool)):
            with pytest.raises(ValueError, match="hand_mask must be"):
                fn(y=dict(y, hand_mask=bad), sil_w=1.0)
        for H in (96, 32, 65):
            with pytest.raises(ValueError, match="not a multiple"):
                fn(y=dict(y, hand_mask=torch.ones(2, H, H, dtype=torch.bool)), sil_w=1.0)
        for dt in (torch.float64, torch.int32, torch.float16):
            with pytest.raises(ValueError, match="bool, uint8 or float32"):
                fn(y=dict(y, hand_mask=torch.ones(2, 64, 64, dtype=dt)), sil_w=1.0)
    model.sil_w = -2.0                      # the attribute is the argument's default
    with pytest.raises(ValueError, match="sil_w"):
        model.get_loss(x, y)
    model.sil_w, model.sil_size = 1.0, 16
    with pytest.raises(ValueError, match="not a multiple"):
        model.get_loss(x, dict(y, hand_mask=torch.ones(2, 24, 24, dtype=torch.bool)))


def test_the_shape_checks_are_shared_with_silhouette_dist():
    from mhentropy_amd import criteria, network
    assert "silhouette_mask_checks" in inspect.getsource(criteria._silhouette_operands)
    assert "silhouette_mask_checks" in inspect.getsource(network.MHEnt.sil_operands)
    with pytest.raises(ValueError, match="hand_mask must be"):
        criteria.silhouette_dist(torch.zeros(1, 2, 5, 3), torch.zeros(1, 2, 3), torch.ones(3, 8, 8), size=8)


def test_train_step_surface_carries_sil_w():
    from mhentropy_amd import train
    for fn in (train.TrainStep.forward, train.TrainStep.forward_backward, train.TrainStep.step, train.GraphedStep.__init__,
               train.differentiable_get_loss):
        p = inspect.signature(fn).parameters
        assert "sil_w" in p and p["sil_w"].default is None and "chamfer_w" in p and "mods" in p, fn
    assert "sil_w" in inspect.signature(train._LossFn.forward).parameters


def test_hypothesis_sharding_refuses_the_term_before_any_launch():
    """TrainStep.forward's first statements, run on a stand-in: shard_hypotheses with sil_w > 0 (argument or attribute) raises before the
    arena, the trunk or any kernel is touched; with the term off the stand-in is reached further (AttributeError on what it lacks)"""
    from mhentropy_amd import train
    model = _cpu_model()

    class Stub:
        shard_hypotheses = True
    stub = Stub()
    stub.model = model
    x, y = torch.zeros(2, 3, 8, 8), {"hand_mask": torch.ones(2, 64, 64, dtype=torch.bool)}
    with pytest.raises(NotImplementedError, match="sil_w"):
        train.TrainStep.forward(stub, x, y, sil_w=1.0)
    model.sil_w = 0.5
    with pytest.raises(NotImplementedError, match="sil_w"):
        train.TrainStep.forward(stub, x, y)
    model.sil_w = 0.0
    with pytest.raises(AttributeError):
        train.TrainStep.forward(stub, x, y)


def test_mods_bits_is_unchanged():
    assert ops.mods_bits(None) == 1 and ops.mods_bits(["uv"]) == 1 and ops.mods_bits("xyz") == 2 and ops.mods_bits(["xyz", "uv"]) == 3
    for bad in (["m"], ["uv", "silhouette"], ["uv", "uv"], [], ["depth"]):
        with pytest.raises(NotImplementedError):
            ops.mods_bits(bad)


@pytest.mark.parametrize("H", [64, 16, 128])
def test_hand_masks(H):
    B = 5
    m = synth.hand_masks(9, B, H=H, with_image=False)
    assert m.shape == (B, H, H) and m.dtype == np.bool_
    assert np.array_equal(m, synth.hand_masks(9, B, H=H, with_image=False)) and not np.array_equal(m, synth.hand_masks(10, B, H=H, with_image=False))
    assert m.reshape(B, -1).any(1).all() and not m.reshape(B, -1).all(1).any()
    uv = synth.batch(9, B, with_image=False)[1]["crop_uv"].reshape(B, 21, 2).astype(np.float64)
    assert np.array_equal(m, synth.hand_masks(0, B, H=H, crop_uv=uv.reshape(B, 42)))
    j = np.minimum(np.floor((uv[..., 0] + 1) / 2 * H).astype(int), H - 1)
    i = np.minimum(np.floor((uv[..., 1] + 1) / 2 * H).astype(int), H - 1)
    assert (np.abs(uv) <= 1).all()                                        # every synthetic keypoint is inside the frame
    assert m[np.arange(B)[:, None], i, j].all()
    # a pixel further than the radius plus its own half diagonal from every keypoint is off
    c = (2 * np.arange(H) + 1) / H - 1
    d = np.sqrt((uv[:, :, None, None, 1] - c[None, None, :, None]) ** 2 + (uv[:, :, None, None, 0] - c[None, None, None, :]) ** 2).min(1)
    assert not m[d > 0.08 + 2 ** 0.5 / H].any() and m[d <= 0.08].all()
    # the default draws the batch the way batch() does by default (image first): the masks of run.py's batches
    if H == 64:
        full = synth.batch(9, 2, image_size=16)[1]["crop_uv"]
        assert np.array_equal(synth.hand_masks(9, 2, image_size=16), synth.hand_masks(0, 2, crop_uv=full))


def test_run_refuses_a_negative_weight():
    from mhentropy_amd import run
    with pytest.raises(SystemExit, match="sil-w"):
        run.main(["--sil-w", "-1"])
