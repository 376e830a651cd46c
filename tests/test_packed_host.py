"""The packed calls' C ABI as far as it can be checked without a GPU: declared, bound, exported; the binding's mirror of
et_packed_result; and the argument check that comes before anything touches a device."""
import ctypes
import os
import re
import subprocess

from entreepy_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("et_encode_packed_device", "et_decode_packed_device", "et_packed_result_size")
ARG = 6  # ET_ERR_ARG


def test_packed_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared, name
        assert name in N.SIGNATURES, name
        assert name in exported, name
    assert "et_packed_result" not in declared  # (the struct's name is not taken for a function by the header test)


def test_the_result_struct_is_mirrored_byte_for_byte():
    assert N.lib().et_packed_result_size() == ctypes.sizeof(N.PackedResult) == 40
    offsets = {name: getattr(N.PackedResult, name).offset for name, _ in N.PackedResult._fields_}
    assert offsets == {"out_bytes": 0, "n_failed": 8, "first_failed": 16, "n_short": 24, "first_status": 32, "pad": 36}


def test_null_context_is_an_argument_error():
    L = N.lib()
    res = N.PackedResult(out_bytes=77)
    cb = N.Codebook()
    index = (ctypes.c_uint64 * 2)(0, 0)
    buf = (ctypes.c_uint8 * 16)()
    p, i = ctypes.addressof(buf), ctypes.addressof(index)
    assert L.et_encode_packed_device(None, ctypes.byref(cb), p, 16, i, 1, p, 16, i, None, ctypes.byref(res)) == ARG
    assert L.et_decode_packed_device(None, ctypes.byref(cb), p, 16, i, i, 1, p, 16, None, None, ctypes.byref(res)) == ARG
    assert L.et_encode_packed_device(None, None, None, 0, None, 0, None, 0, None, None, None) == ARG
    assert L.et_decode_packed_device(None, None, None, 0, None, None, 0, None, 0, None, None, None) == ARG
    assert res.out_bytes == 77  # (nothing was touched)
