"""CPU checks of tests/flow_fwd_ref.py, the float64 reference the flow kernels' edge suite (tests/test_gpu_flow_edges.py) compares with: agreement
with oracle/flows_ref.py, known answers, and the exactness condition of every exact-arithmetic case that suite launches."""
import numpy as np
import pytest
import torch

import flow_fwd_ref as fr
from conftest import assert_close
from oracle import flows_ref

SMALL = [(5, 64, 3, 2, 3, 0), (17, 128, 4, 3, 5, 1), (45, 64, 1, 1, 7, 2), (48, 128, 3, 2, 4, 3)]         # dim, h, ncoup, B, N, seed


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a))


@pytest.mark.parametrize("dim,h,ncoup,B,N,seed", SMALL)
def test_reference_agrees_with_the_oracle(dim, h, ncoup, B, N, seed):
    """forward_p, backward_p and log_prob: the oracle run in float64 is the same function (1e-12 of scale); the float32 oracle is as far from
    this reference as it is from its own float64 run (factor 2 for the two float64 evaluations' different summation orders: none of it shows)"""
    c = fr.random_case(dim, h, ncoup, B, N, seed)
    fwd = fr.evaluate(c, c.x, fr.FORWARD)
    xin = fwd.out.astype(np.float32).astype(np.float64)
    inv = fr.evaluate(c, xin, fr.INVERSE)
    got = {}
    for dt in (torch.float64, torch.float32):
        sd, feat = fr.oracle_state(c, torch, dt)
        with torch.no_grad():
            x, tot = flows_ref.forward_p_logdet(sd, _t(c.x).to(dt), feat)
            z, log_det = flows_ref.backward_p(sd, _t(xin).to(dt), feat)
            assert torch.equal(x, flows_ref.forward_p(sd, _t(c.x).to(dt), feat))
            got[dt] = {"x": x, "sum_s": tot, "z": z, "log_det": log_det, "log_prob": flows_ref.log_prob(sd, _t(xin).to(dt), feat)}
    ref = {"x": fwd.out, "sum_s": fwd.sum_s, "z": inv.out, "log_det": -inv.sum_s, "log_prob": inv.log_prob}
    for k, r in ref.items():
        assert_close(got[torch.float64][k], r, 1e-12, 1e-13, what=k + " vs the float64 oracle")
        e32 = float((got[torch.float32][k].double() - got[torch.float64][k]).abs().max())
        assert float(np.abs(got[torch.float32][k].double().numpy() - r).max()) <= 2 * e32 + 1e-12, k


@pytest.mark.parametrize("dim,h,ncoup,B,N,seed", SMALL)
def test_bf16_mode_agrees_with_the_bf16_oracle_on_random_nets(dim, h, ncoup, B, N, seed):
    """forward_p_logdet_bf16 accumulates in float32, this reference in float64: on random nets one hidden unit's bf16 rounding can flip between
    the two, which moves an output by ~1e-3 of its scale - the project's 1e-2 (tests/test_gpu_kernels.py) is the level they agree to"""
    c = fr.random_case(dim, h, ncoup, B, N, seed)
    ref = fr.evaluate(c, c.x, fr.FORWARD, "bf16")
    sd, feat = fr.oracle_state(c, torch)
    with torch.no_grad():
        x, tot = flows_ref.forward_p_logdet_bf16(sd, _t(c.x).float(), feat)
    assert_close(x, ref.out, 1e-2, what="x")
    assert_close(tot, ref.sum_s, 1e-2, 1e-2, what="sum s")


@pytest.mark.parametrize("h,dim,B,N,kind,seed", [(64, 5, 2, 3, "rand", 0), (128, 45, 3, 5, "rand", 1), (128, 17, 1, 9, "zeros", 2)])
def test_bf16_mode_agrees_with_the_bf16_oracle_where_no_rounding_can_flip(h, dim, B, N, kind, seed):
    """on an exact-arithmetic coupling both have the same hidden activations, so only the float32 evaluation of layer 2 and of the coupling
    separates them: the oracle is held to 3 x the distance of this reference's own float32 tail from its float64 one (floor 2e-6 of scale)"""
    c = fr.exact_case(dim, h, B, N, kind, seed)
    ref, r32 = fr.evaluate(c, c.x, fr.FORWARD, "bf16"), fr.evaluate(c, c.x, fr.FORWARD, "bf16", tail=np.float32)
    sd, feat = fr.oracle_state(c, torch)
    with torch.no_grad():
        x, tot = flows_ref.forward_p_logdet_bf16(sd, _t(c.x).float(), feat)
    for name, got, a, b in (("x", x, ref.out, r32.out), ("sum s", tot, ref.sum_s, r32.sum_s)):
        bound = max(3 * float(np.abs(b - a).max()), 2e-6 * float(np.abs(a).max()))
        assert float(np.abs(got.double().numpy() - a).max()) <= bound, (name, bound)


@pytest.mark.parametrize("rounding", [None, "bf16"])
def test_known_answers(rounding):
    c = fr.random_case(17, 64, 3, 2, 5, 4, masks=["ones", "ones", "ones"])
    for direction in (fr.FORWARD, fr.INVERSE):
        r = fr.evaluate(c, c.x, direction, rounding)
        assert np.array_equal(r.out, c.x) and not r.sum_s.any(), "an all-ones mask row is the identity coupling"
        assert_close(r.log_prob, -0.5 * (c.x ** 2).sum(1) - 0.5 * 17 * fr.LOG_2PI, 1e-15, what="log N(x)")
    c = fr.random_case(17, 64, 3, 2, 5, 5, masks=["rand", "zeros", "rand"])
    f = fr.evaluate(c, c.x, fr.FORWARD, rounding)
    assert (f.out != c.x).all(1).any() and f.sum_s.all()
    if rounding is None:           # (with bf16 operands the inverse's nets see the reconstructed pass-through half: equal to rounding flips only)
        b = fr.evaluate(c, f.out, fr.INVERSE)
        assert_close(b.out, c.x, 1e-13, what="inverse(forward(z)) == z")
        assert_close(b.sum_s, f.sum_s, 1e-13, what="the same log-determinant both ways")
        assert_close(b.log_prob, f.log_prob, 1e-13, what="log_prob from the sampling pass == log_prob of the sample")
        # the activations are laid out per net, not per evaluation order
        assert_close(b.o, f.o, 1e-11, what="o"); assert_close(b.h2, f.h2, 1e-11, what="h2")


def test_bf16_helpers_round_to_nearest_even():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.0025, 84.0 - 2.0 ** -16], np.float32)
    assert np.array_equal(fr.bf16_bits(v), torch.as_tensor(v).bfloat16().view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(fr.bf16_round(v), torch.as_tensor(v).bfloat16().double().numpy())


@pytest.mark.parametrize("key", sorted({k for ks in fr.EXACT_CASES.values() for k in ks}))
def test_exact_cases_have_order_independent_hidden_activations(key):
    """the condition the GPU suite's bit-for-bit tape checks and tight output bounds rest on: every layer-0 / layer-1 term is a multiple of one
    quantum with sum of magnitudes < 2^8 quanta-bits (any partial sum is exact in float32), every W1 column is read, and four random term
    orders per unit, fused and unfused, give the float64-accumulated bf16 bits.  A condition, not a tolerance."""
    h, dim, B, N, kind, seed = key
    facts, bad = fr.exactness(fr.exact_case(dim, h, B, N, kind, seed))
    assert all(facts) and bad == 0, (facts, bad)


def test_exactness_check_notices_an_inexact_net():
    """the same check on a net that does not meet the condition (one dense random W1 row) must fail: it is not vacuous"""
    c = fr.exact_case(17, 128, 2, 5, "rand", 0)
    c.W1[0][3] = fr.bf16_round(np.random.default_rng(0).normal(0, 0.3, 128))
    facts, bad = fr.exactness(c)
    assert not all(facts) and bad > 0
