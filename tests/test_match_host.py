"""et_match_packed_device and et_encode_pattern as far as they can be checked without a GPU: declared, bound, exported; the needle's
bits against the oracle's pack_body; the argument check that comes before anything touches a device -- every call-level ET_ERR_ARG,
with a null ctx, *res untouched; and, in pure Python with the oracle, that on the stores and needles of tests/test_gpu_match.py the
bit rule the kernels implement selects the rows decode-and-compare selects, and that those fixtures reach the cases the GPU tests name."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from tests.test_gpu_match import BIT_EDGE_STEM, FIXTURES, HEAD_BITS, MODES, NOT, PREFIX, judged, select
from tests.test_shared_host import oracle_table, table_255, table_2bit, table_ladder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("et_match_packed_device", "et_encode_pattern", "et_match_pattern_max", "et_match_result_size")
OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status


def _oracle():
    from oracle import oracle as O

    return O


def test_match_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared and name in N.SIGNATURES and name in exported, name
    assert len(N.SIGNATURES["et_match_packed_device"][1]) == 14  # (the argument list of the header's declaration)
    assert N.lib().et_match_pattern_max() == 4096 and N.lib().et_match_result_size() == ctypes.sizeof(N.MatchResult) == 32
    assert (N.ET_MATCH_EQUAL, N.ET_MATCH_PREFIX, N.ET_MATCH_NOT) == (0, 1, 0x100)
    for name, value in (("ET_MATCH_EQUAL", 0), ("ET_MATCH_PREFIX", 1), ("ET_MATCH_NOT", 0x100)):
        assert re.search(rf"\b{name} = {value if value < 16 else hex(value)}\b", header), name


def test_the_python_layer_exposes_the_calls_and_the_list_helper():
    assert callable(E.Context.match_packed_device) and callable(E.Context.match_packed) and callable(E.Codebook.encode_pattern)
    assert (E.MATCH_EQUAL, E.MATCH_PREFIX, E.MATCH_NOT) == (0, 1, 0x100)
    assert [f.name for f in E.MatchResult.__dataclass_fields__.values()][0] == "status"


# --- et_encode_pattern -------------------------------------------------------------------------------------------------------------


def _midsummer():
    with open(os.path.join(ROOT, "tests", "golden", "res", "a_midsummer_nights_dream.txt"), "rb") as f:
        return np.frombuffer(f.read(), np.uint8)


def _tables():
    text = _midsummer()
    rng = np.random.default_rng(0x3A7C4001)
    ladder = table_ladder()
    comb = (ladder[0].copy(), ladder[1].copy())  # the ladder with its symbols' order reversed: the 32-bit codewords on the low bytes
    coded = np.flatnonzero(ladder[1])
    comb[0][coded], comb[1][coded] = ladder[0][coded[::-1]], ladder[1][coded[::-1]]
    return {
        "midsummer": (oracle_table(text), lambda n: text[1000 : 1000 + n]),
        "table_255": (table_255(), lambda n: rng.integers(1, 256, size=n).astype(np.uint8)),
        "ladder32": (ladder, lambda n: (131 + rng.integers(0, 2, size=n)).astype(np.uint8)),
        "ladder_mixed": (ladder, lambda n: (100 + np.minimum(rng.geometric(0.3, size=n) - 1, 32)).astype(np.uint8)),
        "comb32": (comb, lambda n: (100 + rng.integers(0, 3, size=n)).astype(np.uint8)),
    }


@pytest.mark.parametrize("name", ["midsummer", "table_255", "ladder32", "ladder_mixed", "comb32"])
def test_encode_pattern_is_the_oracles_pack_body(name):
    tab, draw = _tables()[name]
    cb = E.Codebook.from_tables(*tab)
    assert cb.is_complete()
    for n in (0, 1, 2, 7, 8, 9, 4096):
        needle = draw(n).tobytes()
        want, end_bit = (_oracle().pack_body(tab[0], tab[1], needle, 0)) if n else (b"", 0)
        assert cb.encode_pattern(needle) == (want, end_bit), n
        # through the C ABI, into a buffer full of a sentinel and exactly as long as needed
        out = np.full(len(want) + 8, 0xA5, np.uint8)
        bits = ctypes.c_uint64(77)
        assert N.lib().et_encode_pattern(ctypes.byref(cb.raw), needle, n, out.ctypes.data, len(want), ctypes.byref(bits)) == OK
        assert bits.value == end_bit and out[: len(want)].tobytes() == want and bool((out[len(want) :] == 0xA5).all())
    if name in ("ladder32", "comb32"):
        assert cb.encode_pattern(draw(4096).tobytes())[1] >= 4096 * 16  # (the 32-bit codewords occur)
    if name == "ladder32":
        assert cb.encode_pattern(draw(4096).tobytes())[1] == 4096 * 32  # the longest pattern there is: 16 KiB


def test_encode_pattern_errors():
    tab = table_2bit()
    cb = E.Codebook.from_tables(*tab)
    L, c = N.lib(), ctypes.byref(cb.raw)
    out = np.full(16, 0xA5, np.uint8)
    bits = ctypes.c_uint64(77)
    assert L.et_encode_pattern(c, b"ACxGT", 5, out.ctypes.data, 16, ctypes.byref(bits)) == UNSUPPORTED and bits.value == 0
    assert bool((out == 0xA5).all())
    with pytest.raises(E.EntreepyError) as e:
        cb.encode_pattern(b"ACGTN")
    assert e.value.status == UNSUPPORTED
    assert L.et_encode_pattern(c, b"ACGTACGTA", 9, out.ctypes.data, 2, ctypes.byref(bits)) == CAP  # 18 bits: one byte short
    assert bool((out == 0xA5).all())
    assert L.et_encode_pattern(c, b"ACGTACGTA", 9, out.ctypes.data, 3, ctypes.byref(bits)) == OK and bits.value == 18
    assert L.et_encode_pattern(None, b"ACGT", 4, out.ctypes.data, 16, ctypes.byref(bits)) == ARG
    assert L.et_encode_pattern(c, b"ACGT", 4, out.ctypes.data, 16, None) == ARG
    assert L.et_encode_pattern(c, None, 4, out.ctypes.data, 16, ctypes.byref(bits)) == ARG
    assert L.et_encode_pattern(c, b"ACGT", 4, None, 16, ctypes.byref(bits)) == ARG
    assert L.et_encode_pattern(c, None, 0, None, 0, ctypes.byref(bits)) == OK and bits.value == 0


# --- et_match_packed_device: the argument check ------------------------------------------------------------------------------------


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    def __init__(self):
        self.cb = N.Codebook()
        self.res = N.MatchResult(n_match=77, n_failed=78, first_failed=79, first_status=80, pattern_bits=81)
        self.buf = (ctypes.c_uint64 * 8)()  # 8-byte aligned
        self.needle = ctypes.create_string_buffer(b"needle", 4200)
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, cb=ctypes.addressof(self.cb), d_bodies=p, body_bytes=16, d_body_index=p, d_text_index=p + 16, n_records=1, needle=ctypes.addressof(self.needle),
                      needle_len=6, mode=1, d_rows=p + 32, cap_rows=4, d_status=None, res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        rc = N.lib().et_match_packed_device(v["ctx"], ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None, v["d_bodies"], v["body_bytes"], v["d_body_index"],
                                            v["d_text_index"], v["n_records"], v["needle"], v["needle_len"], v["mode"], v["d_rows"], v["cap_rows"], v["d_status"],
                                            ctypes.cast(v["res"], ctypes.POINTER(N.MatchResult)) if v["res"] else None)
        r = self.res
        assert (r.n_match, r.n_failed, r.first_failed, r.first_status, r.pattern_bits) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


def test_null_context_is_an_argument_error():
    assert _Args().call() == ARG
    assert N.lib().et_match_packed_device(None, None, None, 0, None, None, 0, None, 0, 0, None, 0, None, None) == ARG


@pytest.mark.parametrize("name", ["cb", "res", "d_bodies", "d_body_index", "d_text_index", "needle"])
def test_every_null_pointer_is_an_argument_error_before_a_device_is_touched(name):
    assert _Args().call(**{name: None}) == ARG


@pytest.mark.parametrize("name", ["d_body_index", "d_text_index"])
@pytest.mark.parametrize("by", [1, 4])
def test_a_misaligned_offset_array_is_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("by", [1, 2, 3])
def test_misaligned_rows_are_an_argument_error(by):
    a = _Args()
    assert a.call(d_rows=a.v["d_rows"] + by) == ARG


def test_too_many_records_a_needle_too_long_and_unknown_modes_are_argument_errors():
    assert _Args().call(n_records=0x80000000) == ARG
    assert _Args().call(n_records=1 << 40) == ARG
    assert _Args().call(needle_len=N.lib().et_match_pattern_max() + 1) == ARG
    for mode in (2, 0x200, 3, 0x102, -1):
        assert _Args().call(mode=mode) == ARG, mode


# --- the fixtures of the GPU tests -------------------------------------------------------------------------------------------------


def _pattern(tab, needle):
    """-> (bytes, bits, never): the needle's body under the table; never = a byte of it has no code."""
    nd = np.frombuffer(needle, np.uint8)
    if nd.size and bool((tab[1][nd] == 0).any()):
        return b"", 0, True
    body, bits = _oracle().pack_body(tab[0], tab[1], nd, 0) if nd.size else (b"", 0)
    return body, bits, False


def _begins_with(body, pattern, bits):
    """The body holds the pattern's bytes and begins with its bits: whole bytes, the last one masked to its top bits % 8 bits."""
    n = (bits + 7) // 8
    if len(body) < n:
        return False
    if bits % 8 == 0:
        return body[:n] == pattern
    keep = (0xFF << (8 - bits % 8)) & 0xFF
    return body[: n - 1] == pattern[: n - 1] and (body[n - 1] ^ pattern[n - 1]) & keep == 0


def rule_rows(st, needle, mode, ignore_length=False):
    """The rows the kernels' rule selects: no decoding anywhere."""
    pattern, bits, never = _pattern(st.tab, needle)
    blob = st.bodies.tobytes()
    out = []
    for b, (status, _, _) in enumerate(judged(st)):
        if status:
            continue
        b0, b1, length = int(st.body_index[b]), int(st.body_index[b + 1]), int(st.text_index[b + 1]) - int(st.text_index[b])
        fits = ignore_length or (length >= len(needle) if mode & PREFIX else length == len(needle))
        hit = not never and fits and _begins_with(blob[b0:b1], pattern, bits)
        if hit != bool(mode & NOT):
            out.append(b)
    return out


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_bit_rule_selects_what_decode_and_compare_selects(name):
    st, needles = FIXTURES[name]()
    wants = judged(st)
    for needle in needles:
        for mode in MODES:
            assert rule_rows(st, needle, mode) == select(wants, needle, mode), (needle[:20], mode)
    for needle in (b"\xff", bytes(needles[0]) + b"\xff"):  # outside every one of these tables
        if int(st.tab[1][0xFF]) == 0:
            assert rule_rows(st, needle, PREFIX) == select(wants, needle, PREFIX) == []


def test_the_fixtures_reach_the_cases_the_gpu_tests_name():
    # every residue of pattern_bits mod 8
    st, needles = FIXTURES["bit_edges"]()
    assert all(nd.startswith(BIT_EDGE_STEM) for nd in needles)
    assert sorted(_pattern(st.tab, nd)[1] % 8 for nd in needles) == list(range(8))
    # the zero-codeword trap: records the bytes alone would select and the length rejects, under both modes
    for name in ("bit_edges", "bit_edges_2bit"):
        st, needles = FIXTURES[name]()
        trapped = 0
        for nd in needles:
            by_bytes, by_rule = set(rule_rows(st, nd, PREFIX, ignore_length=True)), set(rule_rows(st, nd, PREFIX))
            short = [b for b in by_bytes - by_rule if judged(st)[b][1] == len(nd) - 1]
            trapped += len(short)
            assert all(b not in rule_rows(st, nd, 0) for b in short)
            if name == "bit_edges":
                assert short, nd
        assert trapped >= 3, name
    # survivors: records that pass the head window while pattern remains -- a wavefront of 64 of them, and one with exactly one
    st, needles = FIXTURES["survivors"]()
    blob = st.bodies.tobytes()
    for nd in needles:
        pattern, bits, _ = _pattern(st.tab, nd)
        assert bits > HEAD_BITS
        passed = [b for b in range(st.n) if int(st.text_index[b + 1] - st.text_index[b]) >= len(nd) and int(st.body_index[b + 1] - st.body_index[b]) >= len(pattern)
                  and blob[int(st.body_index[b]) : int(st.body_index[b]) + HEAD_BITS // 8] == pattern[: HEAD_BITS // 8]]
        matched = rule_rows(st, nd, PREFIX)
        assert set(matched) <= set(passed)
        if len(nd) <= 1000:
            assert [b for b in passed if b < 64] == list(range(64)) and [b for b in passed if 64 <= b < 128] == [81]
            assert len(passed) > len(matched)  # some survive the head and fail behind it
    assert _pattern(st.tab, needles[3])[1] == 16384 * 8
    # ... at the byte just behind the head window, in the middle and in the last byte
    base = _pattern(st.tab, needles[2])[0]
    first_difference = set()
    for b in range(128, st.n):
        body = blob[int(st.body_index[b]) : int(st.body_index[b + 1])][: len(base)]
        if len(body) > 3000:
            first_difference.add(next((i for i in range(len(body)) if body[i] != base[i]), None))
    assert {HEAD_BITS // 8, len(base) - 1} <= first_difference and any(1000 < d < 3000 for d in first_difference)
