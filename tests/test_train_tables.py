"""CPU: the host-side index tables of the train step (mhentropy_amd/train.py, arena.py, train_flow.py) - pure data-movement logic that every
derived weight layout and the data-gradient convolutions depend on; checked against torch's own conv / autograd on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mhentropy_amd import arena, harness, ops, synth, train, train_flow


@pytest.mark.parametrize("k,stride,pad", [(1, 1, 0), (3, 1, 1), (3, 2, 1), (1, 2, 0)])
def test_dgrad_operand_index_gives_the_input_gradient(k, stride, pad):
    """a convolution of the (zero-dilated) output gradient with W'[ci][kh'][kw'][co] = W[co][ci][KH-1-kh'][KW-1-kw'] at padding k-1-pad
    is the input gradient - the identity train.conv_dgrad builds on the forward kernel"""
    g = torch.Generator().manual_seed(k * 10 + stride)
    Cin, Cout, H = 6, 5, 8
    x = torch.randn(2, Cin, H, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    idx = train.dgrad_operand_index(torch.arange(w.numel()).view(w.shape))          # [Cin, (kh', kw', co)]
    wd = w.reshape(-1)[idx].view(Cin, k, k, Cout).permute(0, 3, 1, 2)               # as a torch conv weight [Cin, Cout, k, k]
    if stride == 2:                                                                 # zero-dilate: out[2i, 2j] = gy[i, j]
        d = torch.zeros(2, Cout, H, H, dtype=torch.float64)
        d[:, :, ::2, ::2] = gy
    else:
        d = gy
    if k == 1 and stride == 2:          # computed on the coarse grid and scattered (train.conv_dgrad's third form)
        gx = torch.zeros_like(x)
        gx[:, :, ::2, ::2] = F.conv2d(gy, wd)
    else:
        gx = F.conv2d(d, wd, padding=k - 1 - pad)
    assert (gx - x.grad).abs().max() < 1e-10


def test_parity_split_stride2_dgrad_tables():
    """the four parity-class operands of a 3x3 / stride-2 / pad-1 data gradient (train.dgrad_s2_operand_indices, consumed by
    mhe_conv3x3s2_dgrad_nhwc): output pixel (2i+py, 2j+px) = a (1+py) x (1+px)-tap convolution of gy, taps at offsets 0 / +1,
    reads past the edge are zero - restated with torch convs and checked against autograd"""
    g = torch.Generator().manual_seed(5)
    Cin, Cout, H = 6, 5, 10
    x = torch.randn(2, Cin, H, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, stride=2, padding=1)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    tabs = train.dgrad_s2_operand_indices(torch.arange(w.numel()).view(w.shape))
    gx = torch.zeros_like(x)
    for py in range(2):
        for px in range(2):
            tb = tabs[2 * py + px]
            wd = w.reshape(-1)[tb].view(Cin, 1 + py, 1 + px, Cout).permute(0, 3, 1, 2)      # torch conv weight [Cin, Cout, th, tw]
            gp = F.pad(gy, (0, px, 0, py))                                              # zeros past the bottom / right edge
            gx[:, :, py::2, px::2] = F.conv2d(gp, wd)
    assert (gx - x.grad).abs().max() < 1e-10
    used = torch.cat([t.reshape(-1) for t in tabs])
    assert used.numel() == w.numel() and torch.equal(torch.sort(used)[0], torch.arange(w.numel()))      # every weight exactly once


@pytest.mark.parametrize("bf16", [False, True])
def test_flow_stream_table_reproduces_the_host_packer(bf16):
    """gathering [W0|W1|W2] through the table == running the host packer on the weights (the table is obtained by packing
    index-valued weights; for the bf16 stream the index travels as three base-128 digits)"""
    dim, h = 45, 128
    rng = np.random.default_rng(0)
    w0, w1, w2 = (rng.normal(size=s).astype(np.float32) for s in ((h, dim), (h, h), (dim, h)))
    if bf16:        # values exactly representable in bf16, so the packer's rounding is the identity
        w0, w1, w2 = ((torch.from_numpy(a).bfloat16().float().numpy()) for a in (w0, w1, w2))
    tab = train.flow_stream_table(dim, h, bf16)
    flat = np.concatenate([w0.ravel(), w1.ravel(), w2.ravel()])
    got = np.where(tab >= 0, flat[np.maximum(tab, 0)], 0.0).astype(np.float32)
    if bf16:
        want = (ops.flow_pack_net_bf16(w0, w1, w2).astype(np.uint32) << 16).view(np.float32)
    else:
        want = ops.flow_pack_net(w0, w1, w2)
    assert got.shape == want.shape and np.array_equal(got, want)
    used = tab[tab >= 0]
    assert used.size == flat.size and np.array_equal(np.sort(used), np.arange(flat.size))       # every weight exactly once


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def tables(request):
    """the operand arena with every table of the train step declared on it, built on the CPU, and the derived operands as a repack
    would leave them: the gather emulated with torch indexing on a random parameter vector"""
    torch.manual_seed(3)
    model = harness.build_mhent(backbone="resnet18", h_dims=(64, 64), num_steps=2, tables=synth.mano_tables(0), compute_dtype=request.param)
    ar = arena.OperandArena(model.parameters(), "cpu")
    units, blocks = train.trunk_tables(ar, model.feat_extractor.res)
    heads = train.head_tables(ar, model)
    flow = train_flow.RealNVPPart(ar, model.q_z_giv_i)
    ar.finalize()
    ar.P.normal_()                          # (the parameters are views into P)
    for a in list(ar.main.values()) + list(ar.fallback.values()):
        take = lambda i: torch.where(i >= 0, ar.P[i.long().clamp(min=0)], torch.zeros(()))
        a.view.copy_(take(a.idx) + (take(a.idx2) if a.idx2 is not None else 0.0))
    return model, ar, units, blocks, heads, flow


def test_unpack_table_maps_every_trained_element_to_one_raw_position(tables):
    """every element of every parameter but the dead feat_extractor.l2 has one raw-gradient position, no position serves two elements -
    except l_j.bias of a coupling net, which shares c_j.bias's by construction (both enter the net as their sum: one gradient)"""
    model, ar = tables[0], tables[1]
    distinct = []
    for name, p in model.named_parameters():
        o = ar.off[id(p)]
        e = ar._unpack[o:o + p.numel()]
        if name.startswith("feat_extractor.l2."):
            assert bool((e == -1).all()), name
            continue
        assert bool((e >= 0).all()) and int(e.max()) < ar.raw.numel(), name
        parts = name.split(".")
        if name.startswith("q_z_giv_i.") and parts[-3] == "l" and parts[-2] in "01" and parts[-1] == "bias":
            twin = dict(model.named_parameters())[".".join(parts[:-3] + ["c"] + parts[-2:])]
            assert torch.equal(e, ar._unpack[ar.off[id(twin)]:ar.off[id(twin)] + twin.numel()]), name
        else:
            distinct.append(e)
    used = torch.cat(distinct)
    assert used.unique().numel() == used.numel()
    assert int((ar._unpack >= 0).sum()) == sum(p.numel() for n, p in model.named_parameters() if not n.startswith("feat_extractor.l2."))


def test_repacked_operands_are_the_parameters_permuted_and_padded(tables):
    model, ar, units, blocks, (l1, d0, d2), flow = tables
    T = model.feat_extractor.res.compute_dtype
    bke = 32 if T == torch.float32 else 64

    def padded(t, rows, cols):
        out = torch.zeros(rows, cols)
        out[:t.shape[0], :t.shape[1]] = t
        return out.to(T)
    # a 3x3 / stride-1 unit: forward pack [Cout][(kh, kw, ci)] and the tap-flipped data-gradient operand [Cin][(kh', kw', co)]
    u = blocks[0].u[0]
    w = u.conv.weight.data
    Cout, Cin = w.shape[:2]
    assert (u.k, u.stride) == (3, 1)
    assert torch.equal(u.w_fwd, padded(w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), Cout, train._ceil(9 * Cin, bke)))
    assert torch.equal(u.w_dg, padded(w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout), Cin, train._ceil(9 * Cout, bke)))
    # layer2's entry (3x3 / stride 2): the four parity classes (py, px) with forward taps (1,) / (2, 0) per axis
    u = next(b for b in blocks if b.layer == 2).u[0]
    w = u.conv.weight.data
    Cout, Cin = w.shape[:2]
    assert (u.k, u.stride) == (3, 2) and len(u.w_s2) == 4
    taps = ((1,), (2, 0))
    for py in range(2):
        for px in range(2):
            sub = w[:, :, list(taps[py])][:, :, :, list(taps[px])].permute(1, 2, 3, 0).reshape(Cin, -1)
            assert torch.equal(u.w_s2[2 * py + px], padded(sub, Cin, train._ceil(sub.shape[1], bke))), (py, px)
    # the det head's last layer: 16 outputs padded to 32 rows, and its transpose
    lin = model.det_head[2]
    want = torch.zeros(32, lin.weight.shape[1])
    want[:16] = lin.weight.data
    assert torch.equal(d2["w"], want) and torch.equal(d2["wT"], want.t())
    assert torch.equal(d2["b"][:16], lin.bias.data) and not d2["b"][16:].any()
    assert d0["w"].data_ptr() == model.det_head[0].weight.data_ptr() and torch.equal(d0["wT"], d0["w"].t())
    # the conditioning biases: c_j.bias + l_j.bias of every net, (coupling, s | t, layer) order
    fl = model.q_z_giv_i
    want = torch.cat([net.c[j].bias.data + net.l[j].bias.data for i in range(len(fl.mask)) for net in (fl.s[i], fl.t[i]) for j in range(2)])
    assert torch.equal(flow.f_bc, want)
    # ... and one net's padded reverse operands
    d = flow.nets[1]
    w0 = torch.zeros(fl.hidden, 64)
    w0[:, :fl.dim] = d["net"].l[0].weight.data
    assert torch.equal(d["w0"], w0) and torch.equal(d["w0T"], w0.t()) and torch.equal(d["w1T"], d["net"].l[1].weight.data.t())


def test_affine_plan_expands_to_the_index_table(tables):
    """bf16 arena: (base, stride, validity) per eight elements over the plan's `aff` segments is the index table itself; its `idx`
    segments are the rest of the groups"""
    model, ar = tables[0], tables[1]
    a = ar.main[torch.bfloat16]
    if model.feat_extractor.res.compute_dtype != torch.bfloat16:
        assert a.used == 0 and a.aff is None
        return
    assert a.aff is not None and a.idx.numel() == a.used > 0
    bs, msk, segs = a.aff
    at = 0
    for kind, lo, hi in segs:
        assert lo == at and hi > lo and kind in ("aff", "idx")
        at = hi
        if kind == "aff":
            k = torch.arange(8)
            valid = (msk[lo:hi, None].long() >> k) & 1
            want = torch.where(valid == 1, bs[lo:hi, :1].long() + k * bs[lo:hi, 1:].long(), torch.full((), -1))
            assert torch.equal(want, a.idx[8 * lo:8 * hi].view(-1, 8).long())
    assert at * 8 == a.idx.numel() and any(kind == "idx" for kind, _, _ in segs)        # (the stem's 7 x 7 x 3 taps are not affine)
