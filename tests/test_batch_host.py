"""The batched calls' C ABI, as far as it can be checked without a GPU: declared, bound, exported, and the argument
checks that come before anything touches a device."""
import ctypes
import os
import re
import subprocess

from entreepy_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("et_encode_batch_device", "et_decode_batch_device", "et_batch_small_max", "et_batch_item_size")


def test_batch_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared, name
        assert name in N.SIGNATURES, name
        assert name in exported, name
    assert "typedef struct et_batch_item" in header


def test_small_max_covers_a_64_kib_page():
    assert N.lib().et_batch_small_max() >= 64 * 1024


def test_item_mirror_has_the_c_structs_size_and_layout():
    assert ctypes.sizeof(N.BatchItem) == N.lib().et_batch_item_size() == 48
    offsets = {name: getattr(N.BatchItem, name).offset for name, _ in N.BatchItem._fields_}
    assert offsets == {"in_off": 0, "in_len": 8, "out_off": 16, "out_cap": 24, "out_len": 32, "status": 40, "path": 44}
    import numpy as np

    import entreepy_amd as E

    assert E.Context._ITEM.itemsize == 48
    assert {k: E.Context._ITEM.fields[k][1] for k in offsets} == offsets
    assert np.zeros(1, dtype=E.Context._ITEM)["status"].dtype == np.int32


def test_null_context_is_an_argument_error():
    L = N.lib()
    items = (N.BatchItem * 2)()
    buf = ctypes.create_string_buffer(64)
    for fn in (L.et_encode_batch_device, L.et_decode_batch_device):
        assert fn(None, buf, buf, items, 2) == N.ET_ERR_ARG
        assert fn(None, buf, buf, None, 2) == N.ET_ERR_ARG
        assert fn(None, None, None, None, 1) == N.ET_ERR_ARG
