"""The train step's parameter and operand allocator (no knowledge of ResNet or the flows).

All parameters live in ONE flat f32 buffer `P` (the nn.Parameters become views into it), with flat gradient and Adam moment buffers
`G / M / V` of the same length.  Every derived operand layout (packed forward weights, data-gradient operands, padded / transposed dense
weights, fragment-major flow operands) is a slice of one arena per dtype, refreshed by ONE gather per step over an index table built once
on the host (`derived`); weight gradients land in a raw arena in whatever layout their kernel produces (`raw_slot`) and one gather over
the unpack table (`map_grad`) maps them onto the flat gradient.

Construction and table building are host integer work and run on any device; `repack()` and what follows it launch HIP kernels.
"""
import os

import numpy as np
import torch

from . import ops


def _ceil(a, b):
    return (a + b - 1) // b * b


class _Arena:
    """one dtype's derived layouts: buffer, elements handed out, the gather's index table(s) (lists of pieces until finalize()), used part, affine plan"""
    __slots__ = ("buf", "used", "idx", "idx2", "view", "aff")

    def __init__(self, buf):
        self.buf, self.used, self.idx, self.idx2, self.view, self.aff = buf, 0, [], [], None, None


class OperandArena:
    def __init__(self, params, device):
        self.dev = torch.device(device)
        ps = list(params)
        self.off, n = {}, 0
        for p in ps:
            self.off[id(p)] = n
            n += _ceil(p.numel(), 4)            # 16-byte aligned segments
        self.n_params = n
        self.P = torch.zeros(n, device=self.dev, dtype=torch.float32)
        for p in ps:
            o = self.off[id(p)]
            self.P[o:o + p.numel()].copy_(p.data.reshape(-1).float())
            p.data = self.P[o:o + p.numel()].view(p.shape)
        self.params, self._param_ver = ps, sum(p._version for p in ps)
        self.G, self.M, self.V = (torch.zeros_like(self.P) for _ in range(3))
        # derived operand layouts: two arenas (f32 / bf16), each refreshed by ONE gather per step over one concatenated index table (a gather
        # per tensor was ~340 launches of ~5 us) ... and a second pair for the layouts only the FALLBACK paths of the flow read (coupling-by-
        # coupling reverse pass, the second-generation coupling kernel): refreshed lazily, when such a path runs (`need_fallback`) - they were
        # gathered every step to be read by nobody (33 M of the 118 M+ gathered elements at the shipped flow's size)
        self.main = {dt: _Arena(torch.zeros(4 * n, device=self.dev, dtype=dt)) for dt in (torch.float32, torch.bfloat16)}
        self.fallback = {dt: _Arena(None) for dt in self.main}
        self.fb_lazy = os.environ.get("MHE_LAZY_FALLBACK_TABLES", "1") == "1"
        self.fb_keep, self.fb_stale = not self.fb_lazy, False       # keep: every repack refreshes them (as soon as a step has needed them once)
        self.poison_stale = os.environ.get("MHE_POISON_STALE_TABLES", "0") == "1"
        self.gather_affine = os.environ.get("MHE_GATHER_AFFINE", "1") == "1"
        self.raw, self._raw_n = None, 0       # the raw-gradient arena: allocated by finalize(), once every slot is reserved
        self._unpack = torch.full((n,), -1, dtype=torch.int64)
        self._after, self._ws = [], {}

    # ------------------------------------------------------------------ table building (host)
    def pidx(self, p):
        """int64 index tensor shaped like p holding each element's position in the flat buffer"""
        o = self.off[id(p)]
        return torch.arange(o, o + p.numel(), dtype=torch.int64).view(p.shape)

    def grad_of(self, p):
        o = self.off[id(p)]
        return self.G[o:o + p.numel()].view(p.shape)

    def derived(self, idx, dtype, idx2=None, fallback=False):
        """a tensor refreshed every step as P[idx] (+ P[idx2]); idx int64 with -1 = 0.  fallback=True: a layout only the flow's fallback
        paths read - refreshed when one of them runs (`need_fallback`)"""
        a = (self.fallback if fallback else self.main)[dtype]
        n = idx.numel()
        room = _ceil(n, 8)                                    # 16-byte aligned views
        if a.buf is None:
            a.buf = torch.zeros(2 * self.n_params, device=self.dev, dtype=dtype)
        if a.used + room > a.buf.numel():
            raise RuntimeError("OperandArena: derived-operand arena exhausted")
        dst = a.buf[a.used:a.used + n].view(idx.shape)
        pad = torch.full((room - n,), -1, dtype=torch.int64)
        a.idx += [idx.reshape(-1), pad]
        a.idx2 += [torch.full((n,), -1, dtype=torch.int64) if idx2 is None else idx2.reshape(-1), pad]
        a.used += room
        return dst

    def raw_slot(self, shape):
        """reserve a raw-gradient slot of this shape; returns its offset (raw_view(offset, shape) is the tensor once finalize() has run)"""
        o = self._raw_n
        self._raw_n += _ceil(int(np.prod(shape)), 4)
        return o

    def raw_view(self, o, shape):
        return self.raw[o:o + int(np.prod(shape))].view(shape)

    def map_grad(self, p, raw_index):
        """raw_index: int64 tensor shaped like p giving the raw-arena position of each element's gradient"""
        o = self.off[id(p)]
        self._unpack[o:o + p.numel()] = raw_index.reshape(-1)

    def after_finalize(self, fn):
        """fn() runs at the end of finalize(): where a table builder takes its raw_view()s"""
        self._after.append(fn)

    def finalize(self):
        """every slot reserved, every layout declared: allocate the raw arena, move the tables to the device (no kernel is launched)"""
        self.raw = torch.zeros(self._raw_n, device=self.dev, dtype=torch.float32)
        for fn in self._after:
            fn()
        self.unpack_idx = self._unpack.to(torch.int32).to(self.dev)
        for a in list(self.main.values()) + list(self.fallback.values()):
            if a.buf is None:
                a.buf = torch.zeros(0, device=self.dev, dtype=torch.float32)
            a.view = a.buf[:a.used]
            i1 = torch.cat(a.idx) if a.idx else torch.zeros(0, dtype=torch.int64)
            i2 = torch.cat(a.idx2) if a.idx2 else torch.zeros(0, dtype=torch.int64)
            a.idx = i1.to(torch.int32).to(self.dev).contiguous()
            a.idx2 = i2.to(torch.int32).to(self.dev).contiguous() if bool((i2 >= 0).any()) else None
            # the bf16 operand layouts as (base, stride, validity) per eight elements instead of eight indices (472 -> 133 MB of index reads per
            # step at C2) - when every group of the arena is affine in the parameter vector (permuted / padded weight tensors are)
            if a.buf.dtype == torch.bfloat16 and a.idx2 is None and i1.numel() and i1.numel() % 8 == 0 and self.gather_affine:
                a.aff = self._affine_plan(i1)

    def _affine_plan(self, i1):
        bs, msk, bad = ops.affine8(i1, with_bad=True)
        # groups that are not affine (the stem's 7 x 7 x 3 taps: 1.3 k of 10.6 M groups at ResNet-50) stay on the indexed form: a few
        # ranges of groups, merged when less than 4,096 groups apart
        ranges = []
        for g in bad.nonzero().flatten().tolist():
            if ranges and g - ranges[-1][1] < 4096:
                ranges[-1][1] = g + 1
            else:
                ranges.append([g, g + 1])
        if len(ranges) > 4 or sum(r[1] - r[0] for r in ranges) * 50 >= bad.numel():
            return None
        segs, at = [], 0
        for lo, hi in ranges + [[bad.numel(), bad.numel()]]:
            if lo > at:
                segs.append(("aff", at, lo))
            if hi > lo:
                segs.append(("idx", lo, hi))
            at = hi
        return (bs.to(self.dev), msk.to(self.dev), segs)

    # ------------------------------------------------------------------ per-step plumbing (device)
    def _gather(self, a):
        if a.aff is not None:
            bs, msk, segs = a.aff
            for kind, lo, hi in segs:
                if kind == "aff":
                    ops.gather_affine8(self.P, bs[lo:hi], msk[lo:hi], a.view[8 * lo:8 * hi])
                else:
                    ops.gather(self.P, a.idx[8 * lo:8 * hi], a.view[8 * lo:8 * hi])
        else:
            ops.gather(self.P, a.idx, a.view, a.idx2)

    def repack(self):
        for a in self.main.values():
            if a.idx.numel():
                self._gather(a)
        if self.fb_keep:
            self.repack_fallback()
        else:
            self.fb_stale = True
            self.poison_fallback()

    def poison_fallback(self):
        """debug mode (MHE_POISON_STALE_TABLES=1, tests): a fallback layout left behind by a repack is filled with NaN, so a reader that
        did not go through need_fallback() fails loudly instead of computing with an earlier step's weights"""
        if self.poison_stale:
            for a in self.fallback.values():
                if a.idx.numel():
                    a.view.fill_(float("nan"))

    def repack_fallback(self):
        for a in self.fallback.values():
            if a.idx.numel():
                self._gather(a)
        self.fb_stale = False

    def need_fallback(self):
        """called by every path that reads a fallback layout (the coupling-by-coupling passes, the modules' own paths through sync_all): brings
        them up to the current parameters if the last repack skipped them, and keeps them fresh from now on (this process runs such steps)"""
        if self.fb_stale:
            self.repack_fallback()
        self.fb_keep = True

    def sync_all(self):
        """sync() for the modules' own paths, which may read any layout (RealNVP._packed: the second-generation kernel's stream)"""
        self.sync()
        self.need_fallback()

    def sync(self):
        """refresh every derived layout if someone else (torch.optim through the attach() bridge, load_state_dict) wrote the parameters since
        the last repack; called by every entry point that reads the packs (TrainStep.forward, ResNetTrunk.forward, RealNVP._packed)"""
        ver = sum(p._version for p in self.params)
        if ver != self._param_ver:
            self.repack()
            self._param_ver = ver

    def mark_synced(self):
        self._param_ver = sum(p._version for p in self.params)

    def workspace(self, key, make):
        """a tensor kept across steps under `key`, made by make() the first time"""
        b = self._ws.get(key)
        if b is None:
            b = self._ws[key] = make()
        return b

    def buf(self, name, shape, dtype=torch.float32):
        """an uninitialised workspace tensor kept under (name, shape, dtype): contents are whatever its last user left"""
        return self.workspace((name, tuple(shape), dtype), lambda: torch.empty(shape, device=self.dev, dtype=dtype))
