"""et_search_packed_device as far as it can be checked without a GPU: declared, bound, exported; the argument check that comes before
anything touches a device -- every call-level ET_ERR_ARG, with a null ctx, *res untouched; and, in pure Python with the oracle and
tests/bitwalk.py, that on the stores and needles of tests/test_gpu_search.py the bit rule the kernels implement selects the rows and
positions that Python's `in`, find and endswith select over the texts, and that those fixtures reach the cases the GPU tests name."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from tests import bitwalk
from tests.test_gpu_match import judged
from tests.test_gpu_search import (BLOCK_BITS, CONTAINS, FIXTURES, LANE_BITS, MODES, NOT, SUFFIX, bit_string, bits_of, edges_fixture, lane_bytes, no_boundary_fixture, pad_fixture,
                                   select, slow_fixture)
from tests.test_match_host import _pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("et_search_packed_device", "et_search_needle_max", "et_search_lane_bytes")
OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status


def test_search_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared and name in N.SIGNATURES and name in exported, name
    assert len(N.SIGNATURES["et_search_packed_device"][1]) == 15  # (the argument list of the header's declaration)
    assert N.lib().et_search_needle_max() == 256 and 0 < N.lib().et_search_lane_bytes() < 8192
    assert (N.ET_SEARCH_CONTAINS, N.ET_SEARCH_SUFFIX, N.ET_MATCH_NOT) == (0, 1, 0x100)
    for name, value in (("ET_SEARCH_CONTAINS", 0), ("ET_SEARCH_SUFFIX", 1)):
        assert re.search(rf"\b{name} = {value}\b", header), name


def test_the_python_layer_exposes_the_call_and_the_list_helper():
    assert callable(E.Context.search_packed_device) and callable(E.Context.search_packed)
    assert (E.SEARCH_CONTAINS, E.SEARCH_SUFFIX, E.MATCH_NOT) == (0, 1, 0x100)


# --- the argument check ------------------------------------------------------------------------------------------------------------


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    def __init__(self):
        self.cb = N.Codebook()
        self.res = N.MatchResult(n_match=77, n_failed=78, first_failed=79, first_status=80, pattern_bits=81)
        self.buf = (ctypes.c_uint64 * 12)()  # 8-byte aligned
        self.needle = ctypes.create_string_buffer(b"needle", 300)
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, cb=ctypes.addressof(self.cb), d_bodies=p, body_bytes=16, d_body_index=p, d_text_index=p + 16, n_records=1, needle=ctypes.addressof(self.needle),
                      needle_len=6, mode=0, d_rows=p + 32, cap_rows=4, d_pos=p + 64, d_status=None, res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        rc = N.lib().et_search_packed_device(v["ctx"], ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None, v["d_bodies"], v["body_bytes"], v["d_body_index"],
                                             v["d_text_index"], v["n_records"], v["needle"], v["needle_len"], v["mode"], v["d_rows"], v["cap_rows"], v["d_pos"], v["d_status"],
                                             ctypes.cast(v["res"], ctypes.POINTER(N.MatchResult)) if v["res"] else None)
        r = self.res
        assert (r.n_match, r.n_failed, r.first_failed, r.first_status, r.pattern_bits) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


def test_null_context_is_an_argument_error():
    assert _Args().call() == ARG
    assert N.lib().et_search_packed_device(None, None, None, 0, None, None, 0, None, 0, 0, None, 0, None, None, None) == ARG


@pytest.mark.parametrize("name", ["cb", "res", "d_bodies", "d_body_index", "d_text_index", "needle"])
def test_every_null_pointer_is_an_argument_error_before_a_device_is_touched(name):
    assert _Args().call(**{name: None}) == ARG


@pytest.mark.parametrize("name", ["d_body_index", "d_text_index"])
@pytest.mark.parametrize("by", [1, 4])
def test_a_misaligned_offset_array_is_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("name", ["d_rows", "d_pos"])
@pytest.mark.parametrize("by", [1, 2, 3])
def test_misaligned_rows_and_positions_are_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


def test_too_many_records_a_needle_too_long_and_unknown_modes_are_argument_errors():
    assert _Args().call(n_records=0x80000000) == ARG
    assert _Args().call(n_records=1 << 40) == ARG
    assert _Args().call(needle_len=N.lib().et_search_needle_max() + 1) == ARG
    for mode in (2, 0x200, 3, 0x102, -1):
        assert _Args().call(mode=mode) == ARG, mode


def test_positions_with_not_or_without_rows_are_argument_errors():
    for mode in (CONTAINS | NOT, SUFFIX | NOT):
        assert _Args().call(mode=mode) == ARG
    assert _Args().call(d_rows=None) == ARG


# --- the rule the kernels implement, in pure Python ----------------------------------------------------------------------------------


def _walked(st, b):
    """Record b's body as a string of bits, and the bit at which codeword i of the walk from its first bit begins -- the codewords
    that the pad bits read as among them; at most length + 1 of them matter -- as a dict bit -> i.  Once per store and record."""
    cache = st.__dict__.setdefault("walked", {})
    if b not in cache:
        body = st.bodies[int(st.body_index[b]) : int(st.body_index[b + 1])].tobytes()
        length = int(st.text_index[b + 1]) - int(st.text_index[b])
        symbols = np.zeros(0, np.uint8)
        if body:
            L, S = bitwalk.next_table(body, *st.tab)
            symbols = bitwalk.walk_symbols(L, S, 0, L.size)[1]
        bounds = bitwalk.boundaries(0, st.tab[1], symbols[: length + 1])
        cache[b] = (bit_string(body), {int(q): i for i, q in enumerate(bounds)})
    return cache[b]


def rule(st, needle, mode):
    """-> (rows, positions).  The needle occurs at symbol i of record b exactly when the pattern's bits lie at the bit where codeword i
    begins, they end inside the body, and i + needle_len <= length_b; no text is compared."""
    pattern, pat_bits, never = _pattern(st.tab, needle)
    pat = bit_string(pattern, pat_bits)
    rows, pos = [], []
    for b, (status, _, _) in enumerate(judged(st)):
        if status:
            continue
        length = int(st.text_index[b + 1]) - int(st.text_index[b])
        at = None
        if not never and length >= len(needle):
            bits, index = _walked(st, b)
            found, q = [], bits.find(pat)
            while q >= 0 and pat_bits:  # every bit at which the pattern lies (and ends inside the body), boundary or not
                found.append(q)
                q = bits.find(pat, q + 1)
            where = index.values() if not pat_bits else [index[q] for q in found if q in index]
            last = length - len(needle)
            hits = [i for i in where if (i == last if mode & SUFFIX else i <= last)]
            at = min(hits) if hits else None
        if (at is not None) != bool(mode & NOT):
            rows.append(b)
            pos.append(None if mode & NOT else at)
    return rows, pos


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_bit_rule_selects_what_the_texts_select(name):
    st, needles = FIXTURES[name]()
    wants = judged(st)
    for needle in needles:
        for mode in MODES:
            assert rule(st, needle, mode) == select(wants, needle, mode), (needle[:20], mode)
    if int(st.tab[1][0xFF]) == 0:  # outside the table
        for needle in (b"\xff", bytes(needles[0]) + b"\xff"):
            assert rule(st, needle, CONTAINS) == select(wants, needle, CONTAINS) == ([], [])


def _occurrences(st, b, needle):
    """Every bit of record b's body at which the needle's bits lie, and the bits at which its codewords (pad bits included) begin."""
    pattern, pat_bits, _ = _pattern(st.tab, needle)
    body = st.bodies[int(st.body_index[b]) : int(st.body_index[b + 1])].tobytes()
    bits, pat = bit_string(body), bit_string(pattern, pat_bits)
    at = [m.start() for m in re.finditer(f"(?={pat})", bits)]
    L, S = bitwalk.next_table(body, *st.tab)
    _, starts = bitwalk.walk_positions(L, 0, L.size)
    return at, set(starts.tolist()) | {len(bits)}


def test_the_fixtures_reach_the_cases_the_gpu_tests_name():
    lane = lane_bytes()
    # bits that occur at no boundary: on both paths, under both tables
    for which in ("2bit", "text"):
        st, needles = no_boundary_fixture(which)
        sizes = []
        for b in range(st.n):
            at, starts = _occurrences(st, b, needles[0] if which == "2bit" else needles[b // 2])
            if at and not set(at) & starts:
                assert b not in select(judged(st), needles[0] if which == "2bit" else needles[b // 2], CONTAINS)[0]
                sizes.append(int(st.body_index[b + 1] - st.body_index[b]))
        assert min(sizes) <= lane < max(sizes), (which, sizes)
    # a needle matched by pad bits alone: its bits lie at a boundary and end inside the body, and the length rejects it -- on both paths
    for which in ("table_255", "ladder"):
        st, needles = pad_fixture(which)
        sizes = []
        for b in range(st.n):
            length = int(st.text_index[b + 1] - st.text_index[b])
            at, starts = _occurrences(st, b, needles[0])
            in_pad = [q for q in at if q in starts and q >= bits_of(st.tab, judged(st)[b][2][:length])]
            if in_pad and b not in select(judged(st), needles[0], CONTAINS)[0]:
                assert b not in select(judged(st), needles[0], SUFFIX)[0]
                sizes.append(int(st.body_index[b + 1] - st.body_index[b]))
        assert min(sizes) <= lane < max(sizes), (which, sizes)
    # the walk's edges
    st, needles, where = edges_fixture()
    cases = {}
    for b, (nd, at, case) in where.items():
        b0, size = int(st.body_index[b]), int(st.body_index[b + 1] - st.body_index[b])
        text = judged(st)[b][2]
        first = (b0 % 4) * 8 + bits_of(st.tab, text[:at])  # from the aligned word the body begins in, as the kernels count
        bits = bits_of(st.tab, nd)
        cases.setdefault(case, set()).add(len(nd))
        if case.startswith("short"):
            assert size <= lane
        elif case.startswith("body_"):
            assert size == lane + int(case[5:]) and at + len(nd) == len(text)
        else:
            assert size > 2 * BLOCK_BITS // 8 > lane
        if case == "lane_edge":
            assert first // LANE_BITS < (first + int(st.tab[1][nd[0]])) // LANE_BITS
        if case == "block_edge":
            assert first < BLOCK_BITS < first + bits
        if case == "last_block":
            assert first > 2 * BLOCK_BITS and at + len(nd) < len(text)
        if case in ("suffix", "short_suffix"):
            assert at + len(nd) == len(text)
    assert cases == {"short": {1, 12, 256}, "short_suffix": {256}, "body_-1": {12}, "body_+0": {12}, "body_+1": {12}, **{c: {1, 12, 256} for c in ("lane_edge", "block_edge", "last_block", "suffix")}}
    # on the lane path an occurrence begins at every bit of a 32-bit word
    words = {((int(st.body_index[b]) % 4) * 8 + bits_of(st.tab, judged(st)[b][2][:at])) % 32 for b, (nd, at, case) in where.items() if case == "short"}
    assert len(words) >= 28
    # slow synchronisation: records above 8 KiB, a needle across the block edge
    for name in ("2bit", "uniform255", "zeros90", "ladder32"):
        st, needles = slow_fixture(name)
        assert int(st.body_index[1]) > 8192 and int(st.body_index[2] - st.body_index[1]) > 8192
        assert all(needles[k] != needles[k + 1] and len(needles[k]) == 12 for k in range(0, 8, 2))
