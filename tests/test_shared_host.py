"""The shared-table calls' C ABI as far as it can be checked without a GPU: declared, bound, exported; et_codebook_is_complete
and et_body_bound (plain host code); and the argument check that comes before anything touches a device.

The hand-made tables of this file are also what tests/test_gpu_shared.py runs on the GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("et_encode_shared_device", "et_decode_shared_device", "et_codebook_is_complete", "et_body_bound")


def canonical(lengths):
    """{symbol: length} -> (data[256] u32, length[256] u8): canonical codes, shorter first, then by symbol.  The lengths must
    not over-fill the tree; a set that under-fills it leaves its hole at the top of the code space."""
    data, length = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    code, prev = 0, 0
    for l, sym in sorted((l, s) for s, l in lengths.items()):
        code <<= l - prev
        assert code < 1 << l, "the lengths over-fill the tree"
        data[sym], length[sym] = code, l
        code, prev = code + 1, l
    return data, length


def table_2bit():
    return canonical({s: 2 for s in b"ACGT"})


def table_6bit():
    return canonical({s: 6 for s in range(32, 96)})


def table_255():
    """255 byte values (1 .. 255): one code of 7 bits, 254 of 8."""
    return canonical({1: 7, **{s: 8 for s in range(2, 256)}})


def table_ladder():
    """33 symbols (the bytes 100 .. 132) of lengths 1, 2, ..., 31, 32, 32: the last two codes fill all 32 bits."""
    return canonical({100 + i: min(i + 1, 32) for i in range(33)})


def oracle_table(text):
    from oracle import oracle as O

    data, length, _ = O.build_dict(O.histogram(text))
    return data, length


def is_complete(data, length):
    return N.lib().et_codebook_is_complete(ctypes.byref(E.Codebook.from_tables(data, length).raw))


def test_shared_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared, name
        assert name in N.SIGNATURES, name
        assert name in exported, name


def test_complete_tables(res_files):
    for name, text in res_files.items():
        data, length = oracle_table(text)
        assert is_complete(data, length) == N.ET_OK, name
    assert int(oracle_table(res_files["a_midsummer_nights_dream.txt"])[1].max()) > 11  # (codes beyond the first-level table)
    for make in (table_2bit, table_6bit, table_255, table_ladder):
        data, length = make()
        assert is_complete(data, length) == N.ET_OK, make.__name__
    data, length = table_255()
    assert np.count_nonzero(length) == 255 and sorted(set(length[length > 0].tolist())) == [7, 8]
    data, length = table_ladder()
    assert sorted(length[length > 0].tolist()) == list(range(1, 33)) + [32]
    assert int(data[131]) == 0xFFFFFFFE and int(data[132]) == 0xFFFFFFFF


def test_incomplete_tables():
    lone = canonical({65: 1})
    assert is_complete(*lone) == N.ET_ERR_UNSUPPORTED  # one coded symbol
    assert is_complete(np.zeros(256, np.uint32), np.zeros(256, np.uint8)) == N.ET_ERR_UNSUPPORTED  # none
    data, length = table_ladder()
    for gone in (100, 117, 132):  # the 33-symbol table with one leaf removed
        d, l = data.copy(), length.copy()
        d[gone], l[gone] = 0, 0
        assert is_complete(d, l) == N.ET_ERR_UNSUPPORTED, gone
    # one code a prefix of another: 0, 00, 10 (the lengths alone would pass: their Kraft sum is 1) -- and 0, 01, 10, 11
    for codes in ([(0b0, 1), (0b00, 2), (0b10, 2)], [(0b0, 1), (0b01, 2), (0b10, 2), (0b11, 2)]):
        d, l = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
        for sym, (code, n) in zip(b"abcd", codes):
            d[sym], l[sym] = code, n
        assert is_complete(d, l) == N.ET_ERR_UNSUPPORTED, codes
    d, l = table_2bit()
    l[ord("A")] = 33  # a length of 33
    assert is_complete(d, l) == N.ET_ERR_UNSUPPORTED
    assert N.lib().et_codebook_is_complete(None) == N.ET_ERR_ARG


def test_codebook_wrappers():
    assert E.Codebook.from_tables(*table_2bit()).is_complete()
    assert not E.Codebook.from_tables(*canonical({65: 1})).is_complete()


@pytest.mark.parametrize("make", [table_2bit, table_6bit, table_255, table_ladder])
def test_body_bound_is_the_formula(make):
    cb = E.Codebook.from_tables(*make())
    max_len = int(cb.raw.max_length)
    assert max_len == int(make()[1].max())
    for n in (0, 1, 2, 7, 8, 9, 4096, 262144, 262145, 1 << 33):
        assert N.lib().et_body_bound(ctypes.byref(cb.raw), n) == cb.body_bound(n) == (n * max_len + 7) // 8, n


def test_null_context_is_an_argument_error():
    L = N.lib()
    items = (N.BatchItem * 2)()
    buf = ctypes.create_string_buffer(64)
    cb = E.Codebook.from_tables(*table_2bit())
    for fn in (L.et_encode_shared_device, L.et_decode_shared_device):
        assert fn(None, ctypes.byref(cb.raw), buf, buf, items, 2) == N.ET_ERR_ARG
        assert fn(None, None, buf, buf, None, 2) == N.ET_ERR_ARG
        assert fn(None, None, None, None, None, 0) == N.ET_ERR_ARG
