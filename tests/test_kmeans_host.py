"""CPU: the host side of the k-means quantisation - the float64 restatement the GPU tests compare with (tests/kmeans_ref.py) recovers a
planted partition, keeps its tie rules on integer data and reports a zero margin on a constructed tie; the C entry and its two LDS helpers
(csrc/kmeans.hip) are declared, exported and bound and refuse bad arguments before any launch; ops.kmeans_select, criteria.kmeans_select and
MHEnt.sample(quant=...) raise their argument errors on CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

import kmeans_ref
from conftest import ROOT
from mhentropy_amd import _lib, criteria, ops

ENTRY = "mhe_kmeans_select_f32"


def test_reference_recovers_a_planted_partition():
    N, B, D, Q = 37, 3, 63, 4
    pts, score, centres = kmeans_ref.planted(22, N, B, D, Q)
    r = kmeans_ref.kmeans(pts, Q, score, iters=10)
    rng = np.random.RandomState(22)
    rng.randn(Q, B, D)
    which = np.stack([rng.permutation(N) % Q for _ in range(B)], 1)          # planted()'s own draw of the memberships
    for b in range(B):
        assert r["converged"][b] == 1
        pairs = set(zip(which[:, b].tolist(), r["assign"][:, b].tolist()))
        assert len(pairs) == Q                                                # a bijection between planted and found clusters
        assert sorted(r["count"][:, b].tolist(), reverse=True) == r["count"][:, b].tolist() and r["count"][:, b].sum() == N
        for q in range(Q):
            members = np.nonzero(r["assign"][:, b] == q)[0]
            assert r["index"][q, b] in members and len(members) == r["count"][q, b]
            assert np.allclose(r["centre"][q, b], pts[members, b].astype(np.float64).mean(0), rtol=0, atol=1e-12)
    assert r["margin"] >= 1e-3 and not r["emptied"]


def test_reference_tie_rules_on_integer_data():
    one = lambda rows, Q, score=None, iters=10: kmeans_ref.kmeans_image(np.array(rows, np.float64), Q, score, iters)
    # seed 0 without a score is row 0, with a tied score the lower row; seed 1 is the farthest row, the lower of two equally far
    r = one([[0], [8], [4], [4], [0]], 2)
    assert r["index"].tolist() == [0, 1] and r["count"].tolist() == [4, 1] and r["assign"].tolist() == [0, 1, 0, 0, 0]      # 4 is as far from 0 as from 8: to the lower k
    assert r["centre"].tolist() == [[2.0], [8.0]] and r["converged"] == 1 and r["margin"] == 0.0
    r = one([[4], [0], [8]], 2, score=[1.0, 3.0, 3.0])                                       # seed 0 = row 1 (tied score, lower n); farthest: row 2
    assert r["index"].tolist() == [0, 2] and r["count"].tolist() == [2, 1] and r["assign"].tolist() == [0, 0, 1] and r["margin"] == 0.0
    r = one([[4], [0], [8]], 2)                                                               # seed 0 = row 0 (value 4): rows 1 and 2 equally far -> row 1
    assert r["assign"].tolist() == [0, 1, 0] and r["index"].tolist() == [0, 1] and r["centre"].tolist() == [[6.0], [0.0]]
    # representative: the member nearest the mean, the lower n of two equally near; order: equal counts go by the lower representative
    r = one([[10], [0], [2], [12]], 2)
    assert r["count"].tolist() == [2, 2] and r["index"].tolist() == [0, 1] and r["assign"].tolist() == [0, 1, 1, 0]
    assert r["centre"].tolist() == [[11.0], [1.0]]
    # an empty cluster: count 0, the nearest of all rows, last in the order; duplicates give the same seed twice
    r = one([[3, 3]] * 4, 2)
    assert r["count"].tolist() == [4, 0] and r["index"].tolist() == [0, 0] and r["assign"].tolist() == [0] * 4 and r["converged"] == 1
    # iters = 0: the seeds and one assignment; iters = 1: one round of means and one more assignment, never converged
    r0, r1 = one([[0], [8], [4], [4], [0]], 2, iters=0), one([[0], [8], [4], [4], [0]], 2, iters=1)
    assert r0["centre"].tolist() == [[0.0], [8.0]] and r0["converged"] == 0 and r0["update_counts"] == []
    assert r1["centre"].tolist() == [[2.0], [8.0]] and r1["converged"] == 0 and r1["update_counts"] == [4, 1]
    assert one([[5, 1]], 1)["margin"] == np.inf                                               # one row: no decision had a second candidate


def test_reference_margin_is_zero_on_a_constructed_tie_and_large_without():
    rows = np.array([[0.0, 0.0], [16.0, 0.0], [7.0, 1.0], [1.0, 0.0]])
    assert kmeans_ref.kmeans_image(rows, 2)["margin"] > 1e-2
    rows[2] = [8.0, 0.0]                                                                      # now as far from row 0 as from row 1
    assert kmeans_ref.kmeans_image(rows, 2)["margin"] == 0.0


def test_entry_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhe.h")).read(), flags=re.S)
    L = _lib.lib()
    m = re.search(rf"\b{ENTRY}\s*\(([^)]*)\)\s*;", src)
    assert m, f"{ENTRY} is not declared in include/mhe.h"
    assert ENTRY in _lib.SIGNATURES and hasattr(L, ENTRY)
    assert len(_lib.SIGNATURES[ENTRY][1]) == len(m.group(1).split(",")) == 13
    assert _lib.SIGNATURES["mhe_kmeans_lds_bytes"] == (_lib.C.c_size_t, [_lib.C.c_int] * 3) and _lib.SIGNATURES["mhe_kmeans_lds_limit"] == (_lib.C.c_size_t, [])
    assert L.mhe_abi_version() == 4
    assert "kmeans.hip" in __import__("mhentropy_amd.build", fromlist=["SOURCES"]).SOURCES
    assert callable(ops.kmeans_select) and callable(criteria.kmeans_select)


def test_lds_budget_helper():
    L = _lib.lib()
    assert L.mhe_kmeans_lds_limit() == 160 * 1024
    for N, Q, D in ((200, 10, 63), (37, 4, 63), (8, 3, 2334), (50, 5, 1), (40, 4, 72)):
        assert L.mhe_kmeans_lds_bytes(N, Q, D) == ops.kmeans_lds_bytes(N, Q, D) == 4 * ((N + Q) * (D | 1) + 2 * N + 3 * Q + 16)
    assert ops.kmeans_lds_bytes(200, 10, 63) < 64 * 1024                                      # the workload's shape takes about a third of a CU
    assert L.mhe_kmeans_lds_bytes(0, 1, 1) == 0 and L.mhe_kmeans_lds_bytes(4, 0, 1) == 0 and L.mhe_kmeans_lds_bytes(4, 1, -1) == 0


def test_entry_refuses_bad_arguments_before_any_launch():
    L, Z = _lib.lib(), None
    N, B, D, Q = 6, 2, 5, 3
    A = lambda t: _lib.C.c_void_p(t.data_ptr())          # host addresses: every call below must return before a kernel could read them
    pts, sc, ctr = torch.zeros(N, B, D), torch.zeros(N, B), torch.zeros(Q, B, D)
    idx, cnt, asg, conv = (torch.zeros(s, dtype=torch.int32) for s in ((Q, B), (Q, B), (N, B), (B,)))

    def call(points=pts, index=idx, n=N, b=B, d=D, q=Q, iters=10):
        return L.mhe_kmeans_select_f32(Z if points is None else A(points), A(sc), Z if index is None else A(index), A(cnt), A(asg), A(ctr), A(conv),
                                       n, b, d, q, iters, Z)

    assert call(points=None) != 0 and b"null" in L.mhe_last_error()
    assert call(index=None) != 0
    for kw in ({"q": 0}, {"q": N + 1}, {"n": 0}, {"b": 0}, {"d": 0}, {"iters": -1}):
        assert call(**kw) != 0 and b"0 < Q <= N" in L.mhe_last_error(), kw
    assert call(n=700, q=3, d=63) != 0                                                        # over the LDS of a CU: refused, and the message names the limit
    msg = L.mhe_last_error().decode()
    assert "160 KiB" in msg and str(160 * 1024) in msg and "LDS" in msg
    assert call() != 0 and b"device memory" in L.mhe_last_error()                             # valid sizes, host pointers


def test_ops_argument_checks_raise_without_a_device():
    pts = torch.zeros(6, 2, 5)
    for q in (0, 7, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="outside 1..N"):
            ops.kmeans_select(pts, q)
    for it in (-1, 1.5, None):
        with pytest.raises(ValueError, match="iters"):
            ops.kmeans_select(pts, 2, iters=it)
    for bad in (torch.zeros(6, 5), torch.zeros(6, 2, 5, 1), torch.zeros(0, 2, 5), None):
        with pytest.raises(ValueError, match=r"\[N,B,D\]"):
            ops.kmeans_select(bad, 1)
    with pytest.raises(ValueError, match="LDS"):                                              # over the limit: refused from the shape alone
        ops.kmeans_select(torch.zeros(700, 1, 63), 3)
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):                                      # everything in order but the device
        ops.kmeans_select(pts, 2)


def test_criteria_argument_checks_raise_without_a_device():
    N, B = 6, 2
    out = {"xyz": torch.zeros(N, B, 63), "verts": torch.zeros(N, B, 2334), "log_q": torch.zeros(N, B)}
    for q in (0, N + 1, 1.0):
        with pytest.raises(ValueError, match="outside 1..N"):
            criteria.kmeans_select(out, q)
    with pytest.raises(ValueError, match="xyz or verts"):
        criteria.kmeans_select(out, 2, points="uv")
    with pytest.raises(ValueError, match="has no 'verts'"):
        criteria.kmeans_select({"xyz": out["xyz"]}, 2, points="verts")
    with pytest.raises(ValueError, match=r"\(N, B, \.\.\.\)"):
        criteria.kmeans_select({"xyz": torch.zeros(N, B)}, 2)
    with pytest.raises(ValueError, match="has no 'log_p'"):
        criteria.kmeans_select(out, 2, score="log_p")
    with pytest.raises(ValueError, match="score must be"):
        criteria.kmeans_select(out, 2, score=torch.zeros(N, B + 1))
    with pytest.raises(ValueError, match="iters"):
        criteria.kmeans_select(out, 2, iters=-1)
    with pytest.raises(ValueError, match="LDS"):                                              # 6 meshes and 2 centres do fit, 30 do not
        criteria.kmeans_select({"verts": torch.zeros(30, B, 2334)}, 2, points="verts")
    with pytest.raises(_lib.MheError, match="CUDA/HIP"):
        criteria.kmeans_select(out, 2, score="log_q")


def test_sample_refuses_an_unknown_quant_before_any_work():
    from mhentropy_amd import harness, synth
    model = harness.build_mhent(backbone="resnet18", h_dims=(64, 64), num_steps=2, tables=synth.mano_tables(0))
    with pytest.raises(ValueError, match="log_q or kmeans"):
        model.sample(None, N=[4, 2], quant="topk")
