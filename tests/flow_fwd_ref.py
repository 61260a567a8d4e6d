"""Plain float64 reference of the conditional RealNVP coupling stack (hand/flows.py:105-122 the coupling nets, :210-227 forward_p / backward_p,
:314-320 log_prob), written from the formulas - what tests/test_gpu_flow_edges.py holds the four sampling / density kernels against
(csrc/flow.hip, flow_bf16.hip, flow_ns.hip, flow_fwd.hip).  A helper module, not a test; tests/test_flow_fwd_ref_host.py checks it on the CPU.

A case carries the operands the kernels take, not a state_dict: per net (index 2 i for s_i, 2 i + 1 for t_i) W0 [h, dim], W1 [h, h], W2 [dim, h],
b2 [dim]; the conditioning table cond [B, nets, 2, h] = c_j(feat) + c_j.bias + l_j.bias per image; mask [ncoup, dim]; rows r use image r % B.

evaluate(..., rounding=None) is float64 throughout.  rounding="bf16" has the rounding points of oracle/flows_ref.py:coupling_net_bf16: the operands
of every product (masked flow variable, weights, hidden activations) rounded to nearest-even bf16, products summed in float64, the sum rounded once
to float32 (the accumulator's format), the leaky-ReLU as the kernels write it - max(v, f32(0.01f v)) - then bf16; nothing after layer 2 is rounded
(`tail=np.float32` evaluates exactly that part - layer 2, tanh, exp, the affine update, both sums - in float32: the float32 error the GPU suite's
bounds are built from).

exact_case() builds a single coupling whose layer-0 and layer-1 pre-activations are EXACT float32 sums in any summation order, so the bf16 hidden
activations are the same bits however a kernel orders its accumulation:
  x, cond           multiples of 1/4 in [-4, 4]
  W0, W1            entries in {-1, 0, +1}, four non-zeros per row (W0: min(4, dim)) at pseudo-random positions that differ per row and per net; every
                    column of W1 carries a non-zero (row i always takes column perm[i]), so a permutation of k is visible
  layer 0           at most five terms, multiples of 1/4, sum of magnitudes <= 20: exact, and positive values need 7 significant bits (bf16-exact);
                    negative ones go through the one float32 product 0.01f v and one rounding to bf16 - the same bits everywhere
  layer 1           terms are bf16 values of magnitude <= 20: multiples of 2^-16 (the smallest non-zero one, 0.01f / 4, has exponent 2^-9), sum of
                    magnitudes <= 84 < 2^8: every partial sum fits 24 bits
  W2, b2            dense random bf16-exact values, scaled so that s and t are O(1): every hidden unit is observable in the outputs
exactness() checks that condition (structurally and by evaluating random term orders, fused and unfused, in float32).
"""
import math
import zlib
from types import SimpleNamespace

import numpy as np

F64, F32 = np.float64, np.float32
SLOPE32 = np.float32(0.01)                       # the kernels' own constant
LOG_2PI = math.log(2.0 * math.pi)
FORWARD, INVERSE = 0, 1


def bf16_bits(a):
    """float32-representable values -> their nearest-even bf16 as uint16"""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32).astype(F64)


def bf16_round(a):
    return bf16_value(bf16_bits(a))


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _act64(pre):
    return np.where(pre > 0, pre, 0.01 * pre)


def _act_bf16(pre):
    p = pre.astype(F32)
    return bf16_round(np.where(p > 0, p, SLOPE32 * p))


def mask_row(kind, dim, rng):
    """'ones' (identity coupling), 'zeros' (the nets see zeros, every dim is transformed) or 'rand': random binary with the last dim transformed
    and (dim > 1) the first passed through, so that both kinds occur and element dim - 1 is never hidden behind the mask"""
    if kind == "ones":
        return np.ones(dim)
    if kind == "zeros":
        return np.zeros(dim)
    m = rng.integers(0, 2, dim).astype(F64)
    m[-1] = 0.0
    if dim > 1:
        m[0] = 1.0
    return m


def net_layers(case, net, xm, img, rounding=None, tail=F64):
    """one coupling net on the masked flow variable xm [R, dim] -> (h1, h2, o): hidden activations after the leaky-ReLU [R, h] and the
    pre-activation of the output layer incl. bias [R, dim] (before the s net's tanh)"""
    c0, c1 = case.cond[img, net, 0], case.cond[img, net, 1]
    W0, W1, W2, b2 = case.W0[net], case.W1[net], case.W2[net], case.b2[net]
    if rounding is None:
        h1 = _act64(xm @ W0.T + c0)
        h2 = _act64(h1 @ W1.T + c1)
        return h1, h2, h2 @ W2.T + b2
    assert rounding == "bf16", rounding
    h1 = _act_bf16(bf16_round(xm) @ bf16_round(W0).T + c0)
    h2 = _act_bf16(h1 @ bf16_round(W1).T + c1)
    o = h2.astype(tail) @ bf16_round(W2).T.astype(tail) + b2.astype(tail)
    return h1, h2, o


def evaluate(case, x, direction, rounding=None, tail=F64, img=None):
    """all couplings, FORWARD (z -> x, flows.py:210-217) or INVERSE (x -> z, couplings in reverse order, flows.py:219-227).  Returns out [R, dim],
    sum_s [R] = sum_i sum_d s_i,d (forward: log|det dx/dz|; inverse: -log_det), log_prob [R] = logN(z; 0, I) - sum_s with z = the input
    (forward) or the output (inverse), and h1, h2 [nets, R, h], o [nets, R, dim] in the layout of the kernels' written-out activations."""
    x = np.asarray(x, F64)
    R, nets = x.shape[0], 2 * case.ncoup
    img = np.arange(R) % case.B if img is None else img
    h1 = np.zeros((nets, R, case.h)); h2 = np.zeros((nets, R, case.h)); o = np.zeros((nets, R, case.dim), tail)
    v = x.astype(tail)
    sum_s = np.zeros(R, tail)
    order = range(case.ncoup) if direction == FORWARD else reversed(range(case.ncoup))
    for ci in order:
        m = case.mask[ci].astype(tail)
        vm = v * m
        for k in range(2):
            h1[2 * ci + k], h2[2 * ci + k], o[2 * ci + k] = net_layers(case, 2 * ci + k, vm.astype(F64), img, rounding, tail)
        s, t = np.tanh(o[2 * ci]) * (1 - m), o[2 * ci + 1] * (1 - m)
        if direction == FORWARD:
            v = vm + (1 - m) * (v * np.exp(s) + t)
        else:
            v = (1 - m) * (v - t) * np.exp(-s) + vm
        sum_s = sum_s + s.sum(1)
    base = x.astype(tail) if direction == FORWARD else v
    log_prob = (-0.5 * (base * base).sum(1) - tail(0.5 * case.dim * LOG_2PI)) - sum_s
    return SimpleNamespace(out=v, sum_s=sum_s, log_prob=log_prob, h1=h1, h2=h2, o=o)


def random_case(dim, h, ncoup, B, N, seed, masks=None, s_gain=1.0):
    """a chain with dense float32 weights of torch.nn.Linear's scale, a conditioning table of the scale c(feat) + biases has, N(0, 1) input;
    masks: one kind per coupling (default: rand, ones, zeros, rand).  s_gain scales the s nets' output layer (the saturating case)."""
    rng = _rng("random", dim, h, ncoup, B, N, seed)
    nets = 2 * ncoup
    u = lambda shape, n: rng.uniform(-1.0, 1.0, shape).astype(F32).astype(F64) / math.sqrt(n)
    f32 = lambda a: a.astype(F32).astype(F64)
    W0, W1, W2, b2 = f32(u((nets, h, dim), dim)), f32(u((nets, h, h), h)), f32(u((nets, dim, h), h)), f32(u((nets, dim), h))
    W2[0::2] = f32(W2[0::2] * s_gain); b2[0::2] = f32(b2[0::2] * s_gain)
    kinds = masks if masks is not None else ["rand", "ones", "zeros", "rand"][:ncoup]
    assert len(kinds) == ncoup
    return SimpleNamespace(dim=dim, h=h, ncoup=ncoup, B=B, N=N, W0=W0, W1=W1, W2=W2, b2=b2, cond=f32(rng.normal(0, 0.6, (B, nets, 2, h))),
                           mask=np.stack([mask_row(k, dim, rng) for k in kinds]), x=f32(rng.normal(0, 1, (N * B, dim))))


def _sparse_signs(rng, rows, cols, k, cover=False):
    W = np.zeros((rows, cols))
    pos = rng.random((rows, cols)).argsort(1)[:, :k]
    if cover:
        pos[:, 0] = rng.permutation(cols)[:rows]       # rows == cols: every column carries a non-zero
    np.put_along_axis(W, pos, rng.choice([-1.0, 1.0], pos.shape), 1)
    return W


def exact_case(dim, h, B, N, mask_kind, seed):
    """the exact-arithmetic single coupling of the module docstring"""
    rng = _rng("exact", dim, h, B, N, mask_kind, seed)
    quarter = lambda shape: rng.integers(-16, 17, shape) / 4.0 + 0.0
    c = SimpleNamespace(dim=dim, h=h, ncoup=1, B=B, N=N, cond=quarter((B, 2, 2, h)), mask=mask_row(mask_kind, dim, rng)[None], x=quarter((N * B, dim)),
                        W0=np.stack([_sparse_signs(rng, h, dim, min(4, dim)) for _ in range(2)]),
                        W1=np.stack([_sparse_signs(rng, h, h, 4, cover=True) for _ in range(2)]), W2=np.zeros((2, dim, h)), b2=np.zeros((2, dim)))
    img = np.arange(N * B) % B
    for net in range(2):        # W2 scaled from the hidden activations it multiplies: s and t pre-activations of spread ~0.7
        h2 = net_layers(c, net, c.x * c.mask[0], img, "bf16")[1]
        c.W2[net] = bf16_round(rng.normal(0, 0.7, (dim, h)) / math.sqrt((h2 * h2).sum(1).mean()))
        c.b2[net] = bf16_round(rng.normal(0, 0.3, dim))
    return c


def _ordered_f32(terms, rng, fused):
    """terms [R, h, T] (factor pairs a * b, float64 holding float32 values): their float32 sum, accumulated sequentially from +0 in an order
    drawn per unit; fused = a single rounding per step (fma), otherwise product and sum rounded separately"""
    a, b = terms
    order = rng.random(a.shape[1:]).argsort(-1)[None]
    a, b = np.take_along_axis(a, np.broadcast_to(order, a.shape), 2), np.take_along_axis(b, np.broadcast_to(order, b.shape), 2)
    acc = np.zeros(a.shape[:2], F32)
    for k in range(a.shape[2]):
        if fused:
            acc = (acc.astype(F64) + a[:, :, k] * b[:, :, k]).astype(F32)        # exact in float64 (16-bit products, 24-bit sums of one scale)
        else:
            acc = acc + a[:, :, k].astype(F32) * b[:, :, k].astype(F32)
    return acc


def _terms(X, W, c):
    """the non-zero terms of X W^T + c per output unit, padded with zeros ([R, h, T + 1] factor pairs).  A zero product adds an exact zero
    in any position, so only these terms' order matters."""
    T = int((W != 0).sum(1).max())
    idx = np.argsort(W == 0, axis=1, kind="stable")[:, :T]                        # non-zero columns first
    w = np.take_along_axis(W, idx, 1)                                            # [h, T] (zeros where a row has fewer)
    a = np.concatenate([X[:, idx], c[:, :, None]], 2)                            # [R, h, T + 1]
    b = np.broadcast_to(np.concatenate([w, np.ones((W.shape[0], 1))], 1)[None], a.shape)
    return a, b


def exactness(case, orders=4):
    """the exactness condition of an exact_case: (structural facts, bit mismatches).  Layers 0 and 1 are evaluated in float32 under `orders` random
    term orders per unit, fused and unfused; mismatches counts float32 pre-activations and bf16 h1 / h2 bits that differ from the
    float64-accumulated ones of evaluate()."""
    R = case.x.shape[0]
    img = np.arange(R) % case.B
    ref = evaluate(case, case.x, FORWARD, "bf16")
    xm = case.x * case.mask[0]
    facts, bad = [], 0
    act = lambda p: bf16_bits(np.where(p > 0, p, SLOPE32 * p))
    for net in range(2):
        t0 = _terms(xm, case.W0[net], case.cond[img, net, 0])
        t1 = _terms(ref.h1[net], case.W1[net], case.cond[img, net, 1])
        for (a, b), quantum in ((t0, 0.25), (t1, 2.0 ** -16)):
            p = a * b
            facts.append(bool((p / quantum == np.rint(p / quantum)).all()) and float(np.abs(p).sum(2).max()) < 2.0 ** 8)
        rng = _rng("orders", net)
        pre0, pre1 = xm @ case.W0[net].T + case.cond[img, net, 0], ref.h1[net] @ case.W1[net].T + case.cond[img, net, 1]      # float64
        for _ in range(orders):
            for fused in (False, True):
                p0 = _ordered_f32(t0, rng, fused)
                p1 = _ordered_f32(_terms(bf16_value(act(p0)), case.W1[net], case.cond[img, net, 1]), rng, fused)
                bad += int((p0 != pre0).sum()) + int((p1 != pre1).sum())          # the float32 sums themselves are the float64 ones ...
                bad += int((act(p0) != bf16_bits(ref.h1[net])).sum()) + int((act(p1) != bf16_bits(ref.h2[net])).sum())     # ... and so are the bits
        facts.append(bool((case.W1[net] != 0).any(0).all()))                     # every column of W1 is read by some unit
    return facts, bad


# The exact-arithmetic cases of the GPU suite, per kernel: (hidden, dim, B, N, mask kind, seed).  Every dim a kernel accepts, every (B, N) class -
# one row, waves and workgroups that span images part-filled, N % 32 == 0 (wave-uniform conditioning), a ragged last tile - at least once per kernel.
EXACT_CASES = {
    "row": [(128, 1, 1, 1, "rand", 0), (128, 16, 3, 5, "rand", 1), (128, 48, 2, 32, "zeros", 2), (128, 45, 2, 40, "rand", 3), (128, 17, 1, 70, "rand", 4),
            (256, 17, 5, 13, "rand", 5), (256, 45, 1, 70, "ones", 6), (256, 48, 2, 32, "rand", 7), (256, 16, 2, 40, "rand", 8), (256, 1, 3, 5, "rand", 9)],
    "unit": [(512, 1, 3, 5, "rand", 10), (512, 16, 2, 32, "rand", 11), (512, 17, 2, 40, "rand", 12), (512, 45, 5, 13, "rand", 13),
             (512, 48, 1, 70, "rand", 14), (512, 45, 1, 1, "zeros", 15), (512, 48, 2, 32, "ones", 16)],
    "frag": [(512, 1, 3, 5, "rand", 20), (512, 16, 2, 32, "rand", 21), (512, 17, 2, 40, "rand", 22), (512, 45, 5, 13, "rand", 23),
             (512, 48, 1, 70, "rand", 24), (512, 49, 1, 64, "rand", 25), (512, 64, 2, 64, "rand", 26), (512, 45, 1, 200, "rand", 27),
             (512, 64, 1, 1, "zeros", 28), (512, 49, 3, 5, "ones", 29), (512, 48, 2, 64, "zeros", 30)],
}


def oracle_state(case, torch, dtype=None):
    """the case as a state_dict of oracle/flows_ref.py plus the feature rows to call it with: features are one-hot image indicators and c_j.weight
    holds the conditioning table's rows, so c_j(feat) reproduces the table exactly (1 * v + 0 * ...); every other conditioning bias is zero"""
    dtype = dtype or torch.float32
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    sd = {"mask": t(case.mask)}
    for i in range(case.ncoup):
        for k, name in enumerate(("s", "t")):
            net, p = 2 * i + k, f"{name}.{i}."
            for j, W in enumerate((case.W0, case.W1, case.W2)):
                sd[p + f"l.{j}.weight"] = t(W[net])
            sd[p + "l.0.bias"], sd[p + "l.1.bias"], sd[p + "l.2.bias"] = t(np.zeros(case.h)), t(np.zeros(case.h)), t(case.b2[net])
            for j in range(2):
                sd[p + f"c.{j}.weight"], sd[p + f"c.{j}.bias"] = t(case.cond[:, net, j, :].T), t(np.zeros(case.h))
    return sd, t(np.eye(case.B)).repeat(case.N, 1)
