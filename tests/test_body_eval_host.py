"""CPU: the body head's evaluation surface - the mesh-error entries of the skinning kernels, mhe_point_errors_f32 / mhe_min_of_n_f32
(csrc/body_eval.hip) and BodyFlowHead.evaluate.  The C ABI declares and binds them with matching arity, their argument checks answer before any
launch, and every ValueError of evaluate() is raised on CPU tensors (the checks run before the first GPU call)."""
import os
import re

import pytest
import torch

from conftest import ROOT
from mhentropy_amd import _lib, body

NEW = ("mhe_lbs_skin_err_supported", "mhe_lbs_skin_err_mfma_f32", "mhe_lbs_skin_err_f32", "mhe_point_errors_f32", "mhe_min_of_n_f32")


def test_new_symbols_declared_and_bound_with_matching_arity():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhe.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in NEW:
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/mhe.h"
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert L.mhe_abi_version() == 4
    assert "body_eval.hip" in __import__("mhentropy_amd.build", fromlist=["SOURCES"]).SOURCES


def test_public_surface_exists():
    assert callable(body.min_of_n) and callable(body.point_errors)
    assert callable(body.BodyFlowHead.evaluate) and callable(body.BodyLayer.vertex_error)


def test_entries_refuse_bad_arguments_before_any_launch():
    L, Z = _lib.lib(), None
    VP = 6912
    assert L.mhe_lbs_skin_err_supported(16384, 24, 10, 6890, VP, 128) == 1 and L.mhe_lbs_skin_err_supported(131072, 24, 10, 6890, VP, 1024) == 1
    assert L.mhe_lbs_skin_err_supported(65, 16, 10, 778, 832, 13) == 1
    assert L.mhe_lbs_skin_err_supported(65, 24, 10, 6890, VP, 12) == 0          # R % B
    assert L.mhe_lbs_skin_err_supported(0, 24, 10, 6890, VP, 1) == 0 and L.mhe_lbs_skin_err_supported(8, 33, 10, 6890, VP, 1) == 0
    assert L.mhe_lbs_skin_err_supported(8, 24, 10, 6890, VP + 8, 1) == 0 and L.mhe_lbs_skin_err_supported(8, 24, 10, 6890, 6880, 1) == 0
    assert L.mhe_lbs_skin_err_supported(1 << 20, 24, 10, 6890, VP, 1 << 20) == 0          # B NV 3 >= 2^31 target elements
    ns3 = (_lib.C.c_int * 3)(1, 3, 3)
    cases = {
        "mhe_lbs_skin_err_mfma_f32": lambda: L.mhe_lbs_skin_err_mfma_f32(Z, Z, Z, Z, Z, 8, 2, 24, 10, 6890, VP, 1.0, Z),
        "mhe_lbs_skin_err_f32": lambda: L.mhe_lbs_skin_err_f32(Z, Z, Z, Z, Z, Z, Z, Z, 8, 2, 24, 10, 6890, VP, 1.0, Z),
        "mhe_point_errors_f32": lambda: L.mhe_point_errors_f32(Z, Z, Z, 2, 3, 17, 0, Z),
        "mhe_min_of_n_f32": lambda: L.mhe_min_of_n_f32(Z, Z, Z, 2, 5, _lib.C.cast(ns3, _lib.C.c_void_p), 3, Z),
    }
    for name, call in cases.items():
        assert call() != 0 and name.encode() in L.mhe_last_error(), name
    one = torch.zeros(1)
    P = lambda t: _lib.C.c_void_p(t.data_ptr())
    for p_ in (0, 65):
        assert L.mhe_point_errors_f32(P(one), P(one), P(one), 2, 3, p_, 0, Z) != 0 and b"P in 1..64" in L.mhe_last_error()
    assert L.mhe_point_errors_f32(P(one), P(one), P(one), 2, 3, 17, 1 << 17, Z) != 0 and b"root index" in L.mhe_last_error()
    for bad in ((0,), (6,), (2, 2), (3, 1)):
        arr = (_lib.C.c_int * len(bad))(*bad)
        assert L.mhe_min_of_n_f32(P(one), P(one), P(one), 2, 5, _lib.C.cast(arr, _lib.C.c_void_p), len(bad), Z) != 0
        assert b"strictly increasing" in L.mhe_last_error()
    assert L.mhe_min_of_n_f32(P(one), P(one), P(one), 2, 5, Z, 9, Z) != 0 and b"outside 1..8" in L.mhe_last_error()


@pytest.fixture(scope="module")
def heads():
    mk = lambda kp: body.BodyFlowHead(body.synthetic_body_tables(3, NV=70, J=24, keypoints=kp), context_features=64, hidden=64, num_layers=2,
                                      num_blocks=1)
    return mk(17), mk(0)


def test_evaluate_value_errors_on_cpu_tensors(heads):
    head, bare = heads
    B, K, NK, NV = 3, 6, 17, 70
    feats, tk, tv = torch.zeros(B, 64), torch.zeros(B, NK, 3), torch.zeros(B, NV, 3)
    with pytest.raises(ValueError, match="keypoint_regressor"):
        bare.evaluate(feats, K, tk)
    for root in (17, -1, (0, 17), (2, 2), (), 1.5):
        with pytest.raises(ValueError, match="root"):
            head.evaluate(feats, K, tk, root=root)
    for ns in ((0,), (7,), (1, 5, 5), (5, 1), (), tuple(range(1, 10)), (1.0,)):
        with pytest.raises(ValueError, match="ns"):
            head.evaluate(feats, max(K, 9) if len(ns) == 9 else K, tk, ns=ns)
    with pytest.raises(ValueError, match="ns"):
        head.evaluate(feats, K, tk)                                   # the default ns = (1, 5, 10, 25) needs K >= 25
    with pytest.raises(ValueError, match="target_keypoints"):
        head.evaluate(feats, K, torch.zeros(B, NK + 1, 3), ns=(1,))
    with pytest.raises(ValueError, match="target_keypoints"):
        head.evaluate(feats, K, torch.zeros(B + 1, NK, 3), ns=(1,))
    with pytest.raises(ValueError, match="target_verts"):
        head.evaluate(feats, K, tk, target_verts=torch.zeros(B, NV + 1, 3), ns=(1,))
    with pytest.raises(ValueError, match="betas"):
        head.evaluate(feats, K, tk, target_verts=tv, betas=torch.zeros(B, 9), ns=(1,))
    with pytest.raises(ValueError, match="noise"):
        head.evaluate(feats, K, tk, noise=torch.zeros(B, K + 1, 144), ns=(1,))
    with pytest.raises(ValueError, match="feats"):
        head.evaluate(torch.zeros(B, 2, 64), K, tk, ns=(1,))


def test_pieces_value_errors_on_cpu_tensors(heads):
    head, _ = heads
    with pytest.raises(ValueError, match="P=65"):
        body.point_errors(torch.zeros(2, 3, 65, 3), torch.zeros(2, 65, 3))
    with pytest.raises(ValueError, match="target"):
        body.point_errors(torch.zeros(2, 3, 17, 3), torch.zeros(3, 17, 3))
    with pytest.raises(ValueError, match="root"):
        body.point_errors(torch.zeros(2, 3, 17, 3), torch.zeros(2, 17, 3), root=17)
    with pytest.raises(ValueError, match="ns"):
        body.min_of_n(torch.zeros(2, 5), (1, 6))
    with pytest.raises(ValueError, match=r"\(B, K\)"):
        body.min_of_n(torch.zeros(2, 5, 1), (1,))
    layer = head.body
    with pytest.raises(ValueError, match="target_verts"):
        layer.vertex_error(torch.zeros(6, 10), pose6d=torch.zeros(6, 144), target_verts=torch.zeros(3, 71, 3))
    with pytest.raises(ValueError, match="multiple"):
        layer.vertex_error(torch.zeros(7, 10), pose6d=torch.zeros(7, 144), target_verts=torch.zeros(3, 70, 3))
    with pytest.raises(ValueError, match="center"):
        layer.vertex_error(torch.zeros(6, 10), pose6d=torch.zeros(6, 144), target_verts=torch.zeros(3, 70, 3), center=torch.zeros(3, 3))
