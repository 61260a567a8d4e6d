"""CPU: the binding layer itself.  ops.launch against a stub library (no GPU is touched, no kernel runs) and the ctypes table
_lib.SIGNATURES as derived from include/mhe.h."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from mhentropy_amd import _lib, ops


class _StubLibrary:
    """stands in for the loaded library: every mhe_* entry records its arguments and returns `status`"""
    def __init__(self, status=0):
        self.status, self.calls = status, []

    def mhe_last_error(self):
        return b"stub says no"

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry


@pytest.fixture
def stub(monkeypatch):
    s = _StubLibrary()
    monkeypatch.setattr(_lib, "lib", lambda: s)
    monkeypatch.setattr(ops, "_stream", lambda: C.c_void_p(0x57))     # (torch.cuda.current_stream() would initialise a device)
    return s


def test_launch_refuses_a_cpu_tensor_before_the_call(stub):
    """a host address must never reach a kernel: the entry and the argument position are named, the library is not called"""
    with pytest.raises(_lib.MheError, match=r"mhe_add_f32: argument 1 "):
        ops.launch("mhe_add_f32", None, torch.zeros(4), 4)
    assert stub.calls == []


def test_launch_converts_none_and_passes_scalars_through(stub):
    d = _lib.ConvDesc()
    ref, sub = C.byref(d), C.c_void_p(0x1000)
    ops.launch("mhe_some_entry", None, 3, 0.25, ref, sub)
    (name, args), = stub.calls
    assert name == "mhe_some_entry" and len(args) == 6
    assert isinstance(args[0], C.c_void_p) and not args[0].value                # None -> a null pointer
    assert args[1] == 3 and type(args[1]) is int and args[2] == 0.25 and type(args[2]) is float
    assert args[3] is ref and args[4] is sub                                    # byref and explicit sub-addresses untouched
    assert isinstance(args[5], C.c_void_p) and args[5].value == 0x57            # the current stream, last


def test_launch_raises_on_a_nonzero_status(stub):
    stub.status = 2
    with pytest.raises(_lib.MheError, match="mhe_pad64_f32.*stub says no"):
        ops.launch("mhe_pad64_f32", None, None, 1, 1)
    assert len(stub.calls) == 1


def test_signatures_are_the_headers():
    p, i, l, sz, f, d = C.c_void_p, C.c_int, C.c_long, C.c_size_t, C.c_float, C.c_double
    S = _lib.SIGNATURES
    assert S["mhe_adam_step_f32"] == (i, [p] * 4 + [sz, p, p] + [f] * 6 + [p])
    assert S["mhe_bn_finalize"] == (i, [p] * 8 + [i, d, f, f, p])
    assert S["mhe_point_errors_f32"] == (i, [p] * 3 + [i] * 3 + [C.c_ulonglong, p])
    assert S["mhe_colsum_ws_f32"] == (i, [p, p, l, i, i, i, l, p, sz, p])
    assert S["mhe_procrustes_workspace_floats"] == (sz, [i, i])
    assert S["mhe_last_error"] == (C.c_char_p, [])
    assert S["mhe_conv2d_f32out_nhwc"] == (i, [C.POINTER(_lib.ConvDesc)] + [p] * 5)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mhe.h")).read(), flags=re.S)
    assert len(S) == len(re.findall(r"\bmhe_[a-z0-9_]+\s*\(", src)) >= 181


@pytest.mark.parametrize("decl", ["int mhe_x(short n, void *stream);", "long long mhe_x(void);", "int mhe_x(int, void *stream);"])
def test_a_declaration_that_does_not_parse_is_an_error(decl):
    with pytest.raises(ImportError, match="mhe_x"):
        _lib._signatures(decl)
