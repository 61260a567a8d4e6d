"""The four kernels that evaluate the conditional RealNVP stack (RealNVP.forward_p, backward_p and log_prob; hand/flows.py:105-122,210-227,314-320)
against the float64 reference of tests/flow_fwd_ref.py at their edges:

  f32   csrc/flow.hip       mhe_flow_couplings_f32                      hidden 64 / 128 / 256 / 512
  row   csrc/flow_bf16.hip  mhe_flow_couplings_bf16, row-split          hidden 128 / 256
  unit  csrc/flow_ns.hip    mhe_flow_couplings_bf16 / _emit, unit-split hidden 512
  frag  csrc/flow_fwd.hip   mhe_flow_couplings_frag_bf16                hidden 512, dim up to 64

Shapes: dim 1, 16, 17, 45, 48 (frag also 49, 64); (B, N) = (1, 1), (3, 5), (5, 13) (waves and workgroups that span images, part-filled), (2, 32) (every
32-row tile inside one image: the wave-uniform conditioning path), (2, 40), (1, 70) (a ragged last tile), frag also N = 64 (the form that writes the
activations out) and 200; 1, 3 and 4 couplings (odd: the inverse's net order ncoup - 1 - step); both directions; random binary mask rows, an all-ones
row (identity coupling) and an all-zeros row (the nets see zeros, every dim is transformed).

Bounds (none of them tuned; the measured max(|diff| / bound) is printed before it is asserted, `pytest -s`):
  a. f32 kernel vs float64: per output max(3 e_f32, 2e-6 extent), e_f32 = the distance of the float32 oracle (oracle/flows_ref.py) from the float64
     reference on the same case, extent = max |reference| - the form of test_full_mesh_on_the_matrix_cores_keeps_f32_accuracy
  b. bf16 kernels on exact-arithmetic single couplings (flow_fwd_ref.exact_case: the hidden activations are the same bits in any accumulation order,
     tests/test_flow_fwd_ref_host.py): the same form against the reference with bf16 rounding points, e_f32 = that reference with layer 2 and
     everything after it in float32; written-out h1 / h2 bit for bit, o[:, :, :dim] within the bound, the fragment kernel's sign_bits those of
     ops.flow_sign_bits.  o past dim: the operands there (W2 rows, bias2) are zero padding, so columns dim .. 47 (unit-split) / dim .. 63
     (fragment kernel) are zero; the unit-split kernel leaves columns >= 48 untouched (include/mhe.h)
  c. bf16 kernels on random chains of 3 and 4 couplings: the project's 1e-2 of the tensor's scale (a flipped bf16 rounding of one hidden unit moves
     an output by ~1e-3) - forward against oracle/flows_ref.py:forward_p_logdet_bf16, inverse z, sum_s and log_prob against the reference's inverse
     with the same rounding points
  d. contracts: out aliasing in, sum_s / log_prob NULL, rows (and activations) behind R keep a sentinel - checked on EVERY launch of this file -,
     two launches give the same bits
  e. dim = 0, and dim = 49 on the three kernels limited to 48, are refused before any launch; mhe_flow_couplings_frag_supported says what the kernel does

Measured on an MI355X, max(|diff| / bound) over the cases of each line (all other checks are exact and hold):
  a. f32 kernel             hidden 64: 0.692 (the saturating case, inverse z)   128: 0.269   256: 0.592   512: 0.615
  b. exact couplings        row-split 0.104   unit-split 0.081, its written-out o 0.060   fragment kernel 0.108, its written-out o 0.143
  c. random chains (1e-2)   row-split 0.015   unit-split 0.045   fragment kernel 0.070
What the exact couplings add over the 1e-2 level, shown on the CPU by putting the reference evaluated on ONE perturbed input in the kernel's place:
one row's conditioning taken from the next image, bias2[dim - 1] of the t net dropped, two columns of W1 swapped give max(|diff| / bound) of
8e4 ... 7e5, 6e3 ... 7e4 and 1e3 ... 2e5 in section b (and h1 / h2 bit mismatches) against 8 ... 110, 1.5 ... 3.6 and 1.3 ... 13 in section c.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import flow_fwd_ref as fr
from edge_measure import Measure

pytestmark = pytest.mark.gpu
SENT, SPARE = -7.0, 3                      # the value behind R, and how many rows of it
SIGN_SENT = 0x5A5A5A5A
ENTRY = {"f32": "mhe_flow_couplings_f32", "row": "mhe_flow_couplings_bf16", "unit": "mhe_flow_couplings_bf16", "frag": "mhe_flow_couplings_frag_bf16"}


def M(kernel):
    return Measure(kernel, "flow-edges")


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _operands(case, kern):
    """the case's weights, bias, mask and conditioning table on the device as the kernel takes them"""
    from mhentropy_amd import ops
    nets = 2 * case.ncoup
    w = lambda a, n: np.ascontiguousarray(a[n], np.float32)
    d = SimpleNamespace(cond=_dev(case.cond), mask=_dev(case.mask))
    d.b2 = _dev(case.b2 if kern == "f32" else np.pad(case.b2, ((0, 0), (0, 64 - case.dim))))
    if kern == "f32":
        d.w = _dev(np.concatenate([ops.flow_pack_net(w(case.W0, n), w(case.W1, n), w(case.W2, n)) for n in range(nets)]))
    elif kern in ("row", "unit"):
        d.w = _dev(np.concatenate([ops.flow_pack_net_bf16(w(case.W0, n), w(case.W1, n), w(case.W2, n)) for n in range(nets)]).view(np.int16), torch.int16)
    else:
        per = []
        for n in range(nets):
            f1, f0, f2 = ops.flow_frag_pack(*(torch.as_tensor(w(a, n)) for a in (case.W0, case.W1, case.W2)))
            per.append(torch.cat([f1.reshape(-1), f0.reshape(-1), f2.reshape(-1)]))
        d.w = torch.stack(per).to(torch.bfloat16).cuda().contiguous()              # per net: W1 | W0 | W2 in fragment-major order
    return d


def _launch(kern, case, d, x, direction, emit=False, signs=False, sum_s=True, logp=True, alias=False):
    """one launch through the C ABI on buffers with SPARE sentinel rows behind R (the ops wrappers allocate exactly R); asserts that the sentinels
    survive and returns the outputs on the CPU"""
    from mhentropy_amd import ops
    R, dim, h, nets, B = x.shape[0], case.dim, case.h, 2 * case.ncoup, case.B
    full = lambda n, dt=torch.float32, v=SENT: torch.full((n,), v, device="cuda", dtype=dt)
    out = full((R + SPARE) * dim).view(R + SPARE, dim)
    xin = _dev(x)
    if alias:
        out[:R] = xin
        xin = out
    ss, lp = full(R + SPARE) if sum_s else None, full(R + SPARE) if logp else None
    h1 = h2 = o = sg = None
    if emit:
        h1, h2, o = full((nets * R + SPARE) * h, torch.bfloat16), full((nets * R + SPARE) * h, torch.bfloat16), full((nets * R + SPARE) * 64)
    if signs:
        sg = full(nets * (R // 64) * 2048 + 64, torch.int32, SIGN_SENT)
    if kern == "frag":
        ops.launch(ENTRY[kern], xin, out, d.cond, 4 * case.ncoup * h, d.w[0, h * h:], d.w[0], d.w[0, h * h + 64 * h:], int(d.w.shape[1]), d.b2, d.mask, ss, lp,
                   h1, h2, o, sg, R, B, dim, h, case.ncoup, direction)
    elif emit:
        ops.launch(ENTRY[kern] + "_emit", xin, out, d.cond, d.w, d.b2, d.mask, ss, lp, h1, h2, o, R, B, dim, h, case.ncoup, direction)
    else:
        ops.launch(ENTRY[kern], xin, out, d.cond, d.w, d.b2, d.mask, ss, lp, R, B, dim, h, case.ncoup, direction)
    torch.cuda.synchronize()
    res = SimpleNamespace(out=out[:R].cpu(), sum_s=None if ss is None else ss[:R].cpu(), log_prob=None if lp is None else lp[:R].cpu())
    tails = [out[R:]] + [t[R:] for t in (ss, lp) if t is not None]
    if emit:
        tails += [h1[nets * R * h:], h2[nets * R * h:], o[nets * R * 64:]]
        res.h1, res.h2 = h1[:nets * R * h].view(nets, R, h).cpu(), h2[:nets * R * h].view(nets, R, h).cpu()
        res.o = o[:nets * R * 64].view(nets, R, 64).cpu()
    assert all(bool((t == SENT).all()) for t in tails), "a row behind R was written"
    if signs:
        assert bool((sg[-64:] == SIGN_SENT).all()), "sign words behind the last workgroup's were written"
        res.sign_bits = sg[:-64].view(nets, R // 64, 2, 8, 64, 2)
        res.sign_ref = ops.flow_sign_bits(h1[:nets * R * h].view(nets, R, h), h2[:nets * R * h].view(nets, R, h), B) if R == 64 * B else None
    return res


def _same(a, b, what):
    for k in ("out", "sum_s", "log_prob", "h1", "h2", "o", "sign_bits"):
        u, v = getattr(a, k, None), getattr(b, k, None)
        if u is not None and v is not None:
            assert torch.equal(_bits(u), _bits(v)), (what, k)


def _bound(ref, ref32):
    ref, ref32 = np.asarray(ref, np.float64), np.asarray(ref32, np.float64)
    return max(3.0 * float(np.abs(ref32 - ref).max()), 2e-6 * float(np.abs(ref).max()))


def _add_outputs(m, tag, got, ref, ref32):
    for k in ("out", "sum_s", "log_prob"):
        m.add(tag + (k,), getattr(got, k).double().numpy(), getattr(ref, k), _bound(getattr(ref, k), getattr(ref32, k)))


DIRS = ((fr.FORWARD, "forward"), (fr.INVERSE, "inverse"))

# ---- a. the f32 kernel against float64 -----------------------------------------------------------------------------------------------------
# (dim, B, N, ncoup, s_gain): s_gain 10 scales the s nets' output layer until |s pre-activation| reaches ~10 (tanh saturates, exp(s) = e^+-1)
F32_CASES = {
    64: [(45, 1, 1, 1, 1.0), (16, 3, 5, 3, 1.0), (45, 2, 32, 4, 10.0), (17, 2, 40, 4, 1.0)],
    128: [(45, 2, 32, 3, 1.0), (48, 2, 40, 4, 1.0), (17, 5, 13, 1, 1.0)],
    256: [(17, 1, 70, 3, 1.0), (48, 3, 5, 1, 1.0), (16, 2, 32, 4, 1.0), (1, 5, 13, 3, 1.0)],
    512: [(45, 5, 13, 4, 1.0), (16, 2, 40, 3, 1.0), (48, 1, 1, 1, 1.0), (1, 1, 70, 4, 1.0)],
}


def _f32_oracle(case, x, direction):
    """oracle/flows_ref.py in float32 on the case: the float32 evaluation whose distance from float64 sets the bound"""
    from oracle import flows_ref
    sd, feat = fr.oracle_state(case, torch)
    xt = torch.as_tensor(x, dtype=torch.float32)
    with torch.no_grad():
        if direction == fr.FORWARD:
            out, tot = flows_ref.forward_p_logdet(sd, xt, feat)
            lp = flows_ref.std_normal_logprob(xt) - tot
        else:
            out, log_det = flows_ref.backward_p(sd, xt, feat)
            tot, lp = -log_det, flows_ref.log_prob(sd, xt, feat)
    return SimpleNamespace(out=out.double().numpy(), sum_s=tot.double().numpy(), log_prob=lp.double().numpy())


@pytest.mark.parametrize("h", sorted(F32_CASES))
def test_f32_kernel_against_f64(gpu_lib, h):
    m = M("mhe_flow_couplings_f32 hidden %d" % h)
    for dim, B, N, ncoup, gain in F32_CASES[h]:
        case = fr.random_case(dim, h, ncoup, B, N, seed=h + dim, masks=["rand"] if ncoup == 1 else None, s_gain=gain)
        d = _operands(case, "f32")
        fwd = fr.evaluate(case, case.x, fr.FORWARD)
        if gain > 1:
            assert 8.0 <= np.abs(fwd.o[0::2]).max() <= 16.0, "the saturating case must saturate"
        for direction, dname in DIRS:
            x = case.x if direction == fr.FORWARD else fwd.out.astype(np.float32).astype(np.float64)
            ref = fwd if direction == fr.FORWARD else fr.evaluate(case, x, direction)
            _add_outputs(m, (dim, B, N, ncoup, gain, dname), _launch("f32", case, d, x, direction), ref, _f32_oracle(case, x, direction))
    m.report()


# ---- b. the bf16 kernels on exact-arithmetic single couplings ---------------------------------------------------------------------------------
@functools.lru_cache(None)
def _exact(key):
    h, dim, B, N, kind, seed = key
    case = fr.exact_case(dim, h, B, N, kind, seed)
    return case, {dr: (fr.evaluate(case, case.x, dr, "bf16"), fr.evaluate(case, case.x, dr, "bf16", tail=np.float32)) for dr, _ in DIRS}


@pytest.mark.parametrize("kern", ["row", "unit", "frag"])
def test_bf16_kernels_on_exact_arithmetic_couplings(gpu_lib, kern):
    """every hidden activation is the same bits in any accumulation order, so the only freedom a kernel has is the float32 order of layer 2 and of
    the coupling: a conditioning row of the wrong image, a dropped bias2 entry, a permuted k or a wrong last dim is far outside the bound"""
    m, mt = M(ENTRY[kern] + " (%s), exact couplings" % kern), M(ENTRY[kern] + " (%s), written-out o" % kern)
    for key in fr.EXACT_CASES[kern]:
        case, refs = _exact(key)
        d = _operands(case, kern)
        emit = kern == "unit" or (kern == "frag" and case.N % 64 == 0)
        for direction, dname in DIRS:
            ref, ref32 = refs[direction]
            got = _launch(kern, case, d, case.x, direction)
            _add_outputs(m, key + (dname,), got, ref, ref32)
            if not emit:
                continue
            tape = _launch(kern, case, d, case.x, direction, emit=True, signs=kern == "frag")
            _same(tape, got, "the launch that writes the activations out")
            for name in ("h1", "h2"):
                want = torch.as_tensor(fr.bf16_bits(getattr(ref, name)).view(np.int16))
                assert torch.equal(_bits(getattr(tape, name)), want), (key, dname, name, int((_bits(getattr(tape, name)) != want).sum()))
            mt.add(key + (dname, "o"), tape.o[:, :, :case.dim].double().numpy(), ref.o, _bound(ref.o, ref32.o))
            pad_end = 48 if kern == "unit" else 64
            assert bool((tape.o[:, :, case.dim:pad_end] == 0).all()), "o past dim: zero padding gives zero"
            assert bool((tape.o[:, :, pad_end:] == SENT).all()), "o columns >= 48 stay untouched (unit-split kernel)"
            if kern == "frag":
                assert tape.sign_ref is not None and torch.equal(tape.sign_bits, tape.sign_ref), (key, dname, "sign_bits")
    m.report()
    if mt.rows:
        mt.report()


# ---- c. the bf16 kernels on random chains --------------------------------------------------------------------------------------------------------
CHAINS = {       # (hidden, dim, B, N, ncoup)
    "row": [(128, 1, 3, 5, 3), (128, 16, 2, 32, 4), (256, 17, 2, 40, 3), (256, 48, 1, 70, 4), (128, 45, 5, 13, 3), (256, 45, 1, 1, 4)],
    "unit": [(512, 1, 5, 13, 3), (512, 16, 2, 32, 4), (512, 17, 1, 70, 3), (512, 48, 2, 40, 4), (512, 45, 3, 5, 3), (512, 48, 1, 1, 4)],
    "frag": [(512, 1, 3, 5, 3), (512, 16, 2, 32, 4), (512, 17, 2, 40, 3), (512, 48, 1, 70, 4), (512, 49, 5, 13, 3), (512, 64, 1, 64, 4),
             (512, 45, 1, 200, 3), (512, 64, 1, 1, 4)],
}


@pytest.mark.parametrize("kern", ["row", "unit", "frag"])
def test_bf16_kernels_on_random_chains(gpu_lib, kern):
    """1e-2 of the tensor's scale (sum_s: + 1e-2 absolute), as tests/test_gpu_kernels.py holds these kernels at dim 45: here the other dims, odd and
    even coupling counts, the identity and the all-transforming mask row, and the inverse direction's z, sum_s AND log_prob
    (= std_normal_logprob(z_ref) + log_det) against a reference instead of a round trip"""
    from oracle import flows_ref
    m = M(ENTRY[kern] + " (%s), random chains" % kern)
    for h, dim, B, N, ncoup in CHAINS[kern]:
        case = fr.random_case(dim, h, ncoup, B, N, seed=7)
        d = _operands(case, kern)
        sd, feat = fr.oracle_state(case, torch)
        z0 = torch.as_tensor(case.x, dtype=torch.float32)
        with torch.no_grad():
            xr, tot = flows_ref.forward_p_logdet_bf16(sd, z0, feat)
        fwd = SimpleNamespace(out=xr.double().numpy(), sum_s=tot.double().numpy(), log_prob=(flows_ref.std_normal_logprob(z0) - tot).double().numpy())
        x = fr.evaluate(case, case.x, fr.FORWARD, "bf16").out.astype(np.float32).astype(np.float64)
        for direction, dname, xin, ref in ((fr.FORWARD, "forward", case.x, fwd), (fr.INVERSE, "inverse", x, fr.evaluate(case, x, fr.INVERSE, "bf16"))):
            got = _launch(kern, case, d, xin, direction)
            for k, atol in (("out", 0.0), ("sum_s", 1e-2), ("log_prob", 0.0)):
                r = getattr(ref, k)
                m.add((h, dim, B, N, ncoup, dname, k), getattr(got, k).double().numpy(), r, atol + 1e-2 * float(np.abs(r).max()))
    m.report()


# ---- d. contracts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern,h,dim,B,N,emit", [("f32", 64, 17, 3, 5, False), ("f32", 256, 48, 2, 40, False), ("row", 128, 17, 3, 5, False),
                                                 ("row", 256, 45, 2, 32, False), ("unit", 512, 17, 3, 5, False), ("unit", 512, 48, 2, 40, True),
                                                 ("frag", 512, 49, 3, 5, False), ("frag", 512, 64, 2, 64, True)])
def test_contracts_alias_null_outputs_and_determinism(gpu_lib, kern, h, dim, B, N, emit):
    """`out` may alias `in`; sum_s and log_prob may be NULL (include/mhe.h) without changing what remains; a second launch gives the same bits.
    (Rows behind R: asserted inside every _launch.)"""
    case = fr.random_case(dim, h, 3, B, N, seed=11)
    d = _operands(case, kern)
    for direction, dname in DIRS:
        kw = dict(emit=emit, signs=emit and kern == "frag")
        base = _launch(kern, case, d, case.x, direction, **kw)
        assert torch.isfinite(base.out).all() and torch.isfinite(base.log_prob).all()
        _same(_launch(kern, case, d, case.x, direction, **kw), base, dname + ": second launch")
        _same(_launch(kern, case, d, case.x, direction, alias=True, **kw), base, dname + ": out aliases in")
        for ss, lp in ((False, True), (True, False), (False, False)):
            _same(_launch(kern, case, d, case.x, direction, sum_s=ss, logp=lp, **kw), base, dname + ": sum_s %s, log_prob %s" % (ss, lp))


# ---- e. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_unsupported_dims_are_refused_without_a_launch(gpu_lib):
    from mhentropy_amd import ops, _lib
    case = fr.random_case(48, 128, 1, 2, 3, seed=0, masks=["rand"])
    big = fr.random_case(48, 512, 1, 2, 3, seed=0, masks=["rand"])
    x = np.zeros((6, 64))
    for dim in (0, 49):
        for kern, c, emit in (("f32", case, False), ("row", case, False), ("unit", big, False), ("unit", big, True)):
            bad = SimpleNamespace(**{**vars(c), "dim": dim})
            d = _operands(c, kern)
            d.b2 = _dev(np.zeros((2, 64)))
            with pytest.raises(_lib.MheError):
                _launch(kern, bad, d, x[:, :max(dim, 1)], fr.FORWARD, emit=emit)
        assert gpu_lib.mhe_flow_packed_floats_per_net(dim, 128) == 0 and gpu_lib.mhe_flow_packed_bytes_per_net_bf16(dim, 128) == 0
        assert gpu_lib.mhe_flow_packed_bytes_per_net_bf16(dim, 512) == 0
    # the fragment kernel takes dim up to 64 (its operands are padded to 64): what _supported says is what sections b and c launch
    assert all(ops.flow_couplings_frag_supported(6, 2, dim, 512, 1) for dim in (1, 48, 49, 64))
    assert not any(ops.flow_couplings_frag_supported(6, 2, dim, 512, 1) for dim in (0, 65, -1))
    d = _operands(big, "frag")
    for dim in (0, 65):
        with pytest.raises(_lib.MheError):
            _launch("frag", SimpleNamespace(**{**vars(big), "dim": dim}), d, x[:, :1], fr.FORWARD)
    torch.cuda.synchronize()
