"""et_decode_packed_gather_device's C ABI as far as it can be checked without a GPU: declared, bound, exported, and the
argument check that comes before anything touches a device -- every call-level ET_ERR_ARG, with a null ctx, *res untouched."""
import ctypes
import os
import re
import subprocess

import pytest

from entreepy_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "et_decode_packed_gather_device"
ARG = 6  # ET_ERR_ARG


def test_gather_entry_point_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", f.read()))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    assert NAME in declared and NAME in N.SIGNATURES and NAME in exported
    assert len(N.SIGNATURES[NAME][1]) == 15  # (the argument list of the header's declaration)


def test_the_python_layer_exposes_the_call_and_the_list_helper():
    import entreepy_amd as E

    assert callable(E.Context.decode_packed_gather_device) and callable(E.Context.decode_packed_rows)


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    def __init__(self):
        self.cb = N.Codebook()
        self.res = N.PackedResult(out_bytes=77, n_failed=78, first_failed=79, n_short=80, first_status=81)
        self.buf = (ctypes.c_uint64 * 8)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, cb=ctypes.addressof(self.cb), d_bodies=p, body_bytes=16, d_body_index=p, d_text_index=p + 16, n_records=1, d_rows=p + 32, n_rows=1,
                      d_out=p, cap=16, d_out_index=p + 48, d_written=None, d_status=None, res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        rc = N.lib().et_decode_packed_gather_device(v["ctx"], ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None, v["d_bodies"], v["body_bytes"], v["d_body_index"],
                                                    v["d_text_index"], v["n_records"], v["d_rows"], v["n_rows"], v["d_out"], v["cap"], v["d_out_index"], v["d_written"], v["d_status"],
                                                    ctypes.cast(v["res"], ctypes.POINTER(N.PackedResult)) if v["res"] else None)
        r = self.res
        assert (r.out_bytes, r.n_failed, r.first_failed, r.n_short, r.first_status) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


def test_null_context_is_an_argument_error():
    a = _Args()
    assert a.call() == ARG
    assert N.lib().et_decode_packed_gather_device(None, None, None, 0, None, None, 0, None, 0, None, 0, None, None, None, None) == ARG


@pytest.mark.parametrize("name", ["cb", "res", "d_bodies", "d_body_index", "d_text_index", "d_rows", "d_out_index"])
def test_every_null_pointer_is_an_argument_error_before_a_device_is_touched(name):
    assert _Args().call(**{name: None}) == ARG


@pytest.mark.parametrize("name", ["d_body_index", "d_text_index", "d_out_index"])
@pytest.mark.parametrize("by", [1, 4])
def test_a_misaligned_offset_array_is_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("by", [1, 2, 3])
def test_misaligned_rows_are_an_argument_error(by):
    a = _Args()
    assert a.call(d_rows=a.v["d_rows"] + by) == ARG


@pytest.mark.parametrize("name", ["n_records", "n_rows"])
def test_more_than_2_31_records_or_rows_are_an_argument_error(name):
    assert _Args().call(**{name: 0x80000000}) == ARG
    assert _Args().call(**{name: 1 << 40}) == ARG
