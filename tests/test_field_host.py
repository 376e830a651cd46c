"""et_field_packed_device's C ABI as far as it can be checked without a GPU: declared, bound, exported, the argument check that comes
before anything touches a device, and the fixtures of tests/test_gpu_field.py: the rule the kernels implement, stated here over
tests/bitwalk.py's codeword boundaries -- the delimiters are the boundaries whose codeword decodes to `delim`, numbered below the
length; a run of fields is the bits from the boundary behind delimiter `field` to the boundary of delimiter `field + n_fields`, shifted
to bit 7 of a byte and padded with zeros -- gives on them what the oracle's encode of Python's split and join gives, and they reach
the cases the GPU tests take them for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from entreepy_amd import _native as N
from tests import bitwalk
from tests.test_gpu_field import (ABSENT, ARG, BAR, BLOCK_BITS, COMMA, LANE_BITS, SPACE, TO_END, _starts, behind_length_fixture, cut_fixture, dense_fixture, edge_fixture, ladder_fixture,
                                  lane_bytes, main_fixture, pad_fixture, phase_rows, py_field, reach, set_pad_fixture, small_fields_fixture, stored_text, want_field)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "et_field_packed_device"


def test_field_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in (NAME, "et_field_lane_bytes"):
        assert name in declared and name in N.SIGNATURES and name in exported, name
    args = re.search(r"int et_field_packed_device\(([^;]*)\);", header).group(1)
    assert len(N.SIGNATURES[NAME][1]) == len(args.split(",")) == 21 and "et_codebook" in args and "et_take_result" in args and "uint32_t *d_pos" in args
    assert re.search(r"#define ET_FIELD_TO_END 0xffffffffu", header) and re.search(r"#define ET_FIELD_ABSENT 0xffffffffu", header)
    assert (N.ET_FIELD_TO_END, N.ET_FIELD_ABSENT) == (0xFFFFFFFF, 0xFFFFFFFF)
    assert N.lib().et_field_lane_bytes() > 0
    slice_scope = re.search(r"et_slice_lane_bytes\(\): .*?\* Out of scope:(.*?)\* The call's own status", header, flags=re.S).group(1)
    assert "delimiter" not in slice_scope  # the field call does it now


def test_the_python_layer_exposes_the_call_the_list_helper_and_the_constants():
    import entreepy_amd as E

    assert callable(E.Context.field_packed_device) and callable(E.Context.field_packed)
    assert (E.FIELD_TO_END, E.FIELD_ABSENT) == (0xFFFFFFFF, 0xFFFFFFFF)


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    ORDER = ["ctx", "cb", "d_bodies", "body_bytes", "d_body_index", "d_text_index", "n_records", "d_rows", "n_rows", "d_field", "field", "d_n_fields", "n_fields", "delim", "d_out",
             "cap", "d_out_body_index", "d_out_text_index", "d_pos", "d_status", "res"]

    def __init__(self):
        self.res = N.TakeResult(out_bytes=77, text_bytes=78, n_failed=79, first_failed=80, first_status=81)
        self.cb = N.Codebook()
        self.buf = (ctypes.c_uint64 * 64)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, cb=ctypes.addressof(self.cb), d_bodies=p, body_bytes=16, d_body_index=p + 64, d_text_index=p + 80, n_records=1, d_rows=p + 96, n_rows=1,
                      d_field=p + 104, field=0, d_n_fields=p + 112, n_fields=1, delim=44, d_out=p + 128, cap=16, d_out_body_index=p + 160, d_out_text_index=p + 176, d_pos=p + 192,
                      d_status=None, res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        args = [v[k] for k in self.ORDER]
        args[1] = ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None
        args[-1] = ctypes.cast(v["res"], ctypes.POINTER(N.TakeResult)) if v["res"] else None
        rc = N.lib().et_field_packed_device(*args)
        r = self.res
        assert (r.out_bytes, r.text_bytes, r.n_failed, r.first_failed, r.first_status) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


def test_null_context_is_an_argument_error():
    assert _Args().call() == ARG
    assert N.lib().et_field_packed_device(None, None, None, 0, None, None, 0, None, 0, None, 0, None, 0, 44, None, 0, None, None, None, None, None) == ARG


@pytest.mark.parametrize("change", [dict(cb=None), dict(res=None), dict(d_bodies=None), dict(d_out_body_index=None), dict(delim=-1), dict(delim=256), dict(n_rows=0x80000000),
                                    dict(d_rows=None, n_rows=2)], ids=str)
def test_argument_errors_leave_the_result_untouched(change):
    assert _Args().call(**change) == ARG


@pytest.mark.parametrize("name", ["d_rows", "d_field", "d_n_fields", "d_pos"])
@pytest.mark.parametrize("by", [1, 2, 3])
def test_misaligned_rows_fields_counts_and_positions_are_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


# --- the rule the kernels implement, in pure Python ---------------------------------------------------------------------------------------


def _walked(st, r):
    """Record r's body as an array of bits, the bits at which the codewords of its stored text begin (one entry more: where the last
    one ends) and their symbols: the codewords that end inside the body, numbered below the length.  Once per store and record."""
    cache = st.__dict__.setdefault("walked_for_fields", {})
    if r not in cache:
        body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])]
        length = int(st.text_index[r + 1]) - int(st.text_index[r])
        symbols = np.zeros(0, np.uint8)
        if body.size:
            L, S = bitwalk.next_table(body.tobytes(), *st.tab)
            symbols = bitwalk.walk_symbols(L, S, 0, L.size)[1][:length]
        cache[r] = (np.unpackbits(body), bitwalk.boundaries(0, st.tab[1], symbols), symbols)
    return cache[r]


def rule(st, r, field, n_fields, delim):
    """-> (the new body's bytes, its symbols, d_pos): the delimiters are the boundaries i < length whose codeword decodes to delim."""
    bits, bounds, symbols = _walked(st, r)
    delims = np.flatnonzero(symbols == delim)  # the symbol numbers of delimiters 1, 2, ... (entry k - 1: delimiter k)
    if field > delims.size:
        return b"", 0, ABSENT
    i = int(delims[field - 1]) + 1 if field else 0  # behind delimiter `field`
    closing = field + n_fields
    j = int(delims[closing - 1]) if 0 < closing <= delims.size else symbols.size  # in front of delimiter field + n_fields, or the text's end
    j = max(i, j) if n_fields else i
    return np.packbits(bits[int(bounds[i]) : int(bounds[j])]).tobytes(), j - i, i


def check_rule(st, rows, field, n_fields, delim):
    want = want_field(st, rows, field, n_fields, delim)
    assert not want.status.any()
    rows = np.arange(st.n) if rows is None else rows
    fields = [int(field)] * len(rows) if np.isscalar(field) else field
    counts = [int(n_fields)] * len(rows) if np.isscalar(n_fields) else n_fields
    for k, (r, f, c) in enumerate(zip(rows, fields, counts)):
        body, n, pos = rule(st, int(r), int(f), int(c), delim)
        b0, b1 = int(want.body_index[k]), int(want.body_index[k + 1])
        assert (body, n, pos) == (want.data[b0:b1].tobytes(), int(want.text_index[k + 1] - want.text_index[k]), int(want.pos[k])), (k, int(r), int(f), int(c), delim)
    return want


def test_the_bit_rule_gives_the_oracles_encode_of_pythons_split_and_join():
    st, texts = main_fixture()
    check_rule(st, *phase_rows(), SPACE)
    last = np.array([t.count(b" ") for t in texts], dtype=np.int64)
    for field in (0, 1, last, last + 1, 0xFFFFFFFE):
        for n in (0, 1, 2, TO_END):
            check_rule(st, None, field, n, SPACE)
    check_rule(st, None, 0, 1, 0xFF)
    st, texts, case = edge_fixture()
    for n in (0, 1, 2, TO_END):
        for field in (0, 1, 2, 3, 4, 4999, 5000, 5001):
            check_rule(st, None, field, n, BAR)


def test_the_bit_rule_on_lengths_cut_bodies_pad_bits_and_other_tables():
    st, stored = behind_length_fixture()
    last = np.array([t.count(b" ") for t in stored], dtype=np.int64)
    for field, n in ((last, 1), (last + 1, 1), (last, TO_END), (0, TO_END)):
        check_rule(st, None, field, n, SPACE)
    st = cut_fixture()
    last = np.array([stored_text(st, r).count(b" ") for r in range(st.n)], dtype=np.int64)
    for field, n in ((last, 1), (last + 1, 1), (0, TO_END), (np.maximum(last - 1, 0), 2)):
        check_rule(st, None, field, n, SPACE)
    st, texts = set_pad_fixture()
    own, _ = main_fixture()
    whole = check_rule(st, None, 0, TO_END, SPACE)
    assert np.array_equal(whole.data, own.bodies) and not np.array_equal(st.bodies, own.bodies)  # the pad is masked, not copied
    st, texts = pad_fixture()
    for delim in (ord("A"), ord("T"), ord("G"), ord("x")):
        for field, n in ((0, TO_END), (0, 1), (1, 1), (2, 3)):
            check_rule(st, None, field, n, delim)
    st = ladder_fixture()
    for delim in (131, 132, 100, 116):
        for field, n in ((0, 1), (1, 1), (39, 2), (40, 1), (41, 1), (3, TO_END)):
            check_rule(st, None, field, n, delim)
    st, texts = dense_fixture()
    last = np.array([t.count(b",") for t in texts], dtype=np.int64)
    for field, n in ((0, 1), (last, 1), (last + 1, 1), (last // 2, 5)):
        check_rule(st, None, field, n, COMMA)
    check_rule(*small_fields_fixture(), 100)


# --- the fixtures are what the GPU tests take them for --------------------------------------------------------------------------------------


def _first_bit(st, r):
    return (int(st.body_index[r]) % 4) * 8  # from the aligned word the body begins in, as the kernels count


def _span(st, r, field, n_fields, delim):
    """-> (the bit at which the result begins, as the kernels count; the bits it has); None for an absent field."""
    s, pos = py_field(stored_text(st, r), field, n_fields, delim)
    if pos == ABSENT:
        return None
    at = _starts(st.tab, stored_text(st, r), _first_bit(st, r))
    return int(at[pos]), int(at[pos + len(s)] - at[pos])


def test_the_main_fixture_reaches_begin_bits_and_bit_counts_on_both_paths():
    st, texts = main_fixture()
    lane = lane_bytes()
    sizes = np.array([reach(st, r) for r in range(st.n)])
    assert sizes.min() == 0 and (sizes <= lane).sum() >= 8 and sizes.max() > 2 * BLOCK_BITS // 8  # bodies on both sides of the threshold, and of three blocks
    seen = {"lane": set(), "workgroup": set()}
    spans_lanes = absent = 0
    for r, f, c in zip(*phase_rows()):
        span = _span(st, int(r), int(f), int(c), SPACE)
        if span is None:
            absent += 1
            continue
        begin, bits = span
        if bits == 0:
            continue
        path = "lane" if reach(st, int(r)) <= lane else "workgroup"
        seen[path].add((begin % 8, bits % 8))
        spans_lanes += path == "workgroup" and begin // LANE_BITS < (begin + bits - 1) // LANE_BITS
    for path, pairs in seen.items():  # the reduced grid: every begin bit and every bit count mod 8 on both paths, and most of their pairs
        assert {b for b, _ in pairs} == set(range(8)) and {c for _, c in pairs} == set(range(8)) and len(pairs) >= 48, (path, len(pairs))
    assert spans_lanes >= 50 and absent >= 3


def test_the_edge_fixture_puts_delimiters_at_the_lane_and_block_edges():
    st, texts, case = edge_fixture()
    lane = lane_bytes()
    bar_bits = int(st.tab[1][BAR])
    for tag, edge in (("lane_edge", 7 * LANE_BITS), ("block_edge", BLOCK_BITS)):
        r = case[tag]
        assert reach(st, r) > lane
        at = _starts(st.tab, texts[r], _first_bit(st, r))
        first = texts[r].index(b"|")
        assert texts[r][first : first + 2] == b"||" and texts[r].count(b"|") == 3
        assert at[first] + bar_bits == edge == at[first + 1]  # the last codeword of a lane (of block 0), the first codeword of the next (of block 1)
    r = case["block_edge"]
    at = _starts(st.tab, texts[r], _first_bit(st, r))
    assert at[texts[r].index(b"|") + 1] // LANE_BITS == BLOCK_BITS // LANE_BITS  # the closing delimiter of field 1: in the first lane of block 1
    r = case["three_blocks"]
    begin, bits = _span(st, r, 1, 1, BAR)
    assert begin < LANE_BITS and begin + bits > 2 * BLOCK_BITS and len(texts[r]) <= N.lib().et_batch_small_max()  # begins in block 0, ends in block 2
    assert texts[case["bars_only"]] == b"|" * 5000 and reach(st, case["bars_only"]) > lane
    for tag, long in (("ends_short", False), ("ends_long", True), ("none_short", False), ("none_long", True)):
        r = case[tag]
        assert (reach(st, r) > lane) == long
        assert (texts[r][:1] == texts[r][-1:] == b"|" and texts[r].count(b"|") == 2) if tag.startswith("ends") else b"|" not in texts[r]


def test_the_dense_fixture_has_a_one_bit_delimiter_and_real_counts():
    st, texts = dense_fixture()
    assert int(st.tab[1][COMMA]) == 1
    lane = lane_bytes()
    assert [reach(st, r) > lane for r in range(st.n)] == [False, False, False, True, True]  # (3 000 symbols at a bit and a bit: a lane with 2 700 delimiters)
    r = st.n - 1
    at = _starts(st.tab, texts[r], _first_bit(st, r))
    commas = at[:-1][np.frombuffer(texts[r], np.uint8) == COMMA]
    per_lane = np.bincount((commas // LANE_BITS).astype(np.int64))
    assert per_lane.max() >= 200 and int(at[-1]) > 2 * BLOCK_BITS and np.bincount((commas // BLOCK_BITS).astype(np.int64))[0] > 40000


def test_the_fixtures_for_what_is_no_part_of_the_stored_text():
    st, stored = behind_length_fixture()
    lane = lane_bytes()
    behind = []
    for r in range(st.n):
        body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes()
        L, S = bitwalk.next_table(body, *st.tab)
        symbols = bitwalk.walk_symbols(L, S, 0, L.size)[1]
        assert symbols[: len(stored[r])].tobytes() == stored[r] == stored_text(st, r)
        behind.append(int(np.count_nonzero(symbols[len(stored[r]) :] == SPACE)))  # codewords that end inside the body, at or behind the length
    paths = [reach(st, r) > lane for r in range(st.n)]
    assert any(b > 0 and not p for b, p in zip(behind, paths)) and any(b > 100 and p for b, p in zip(behind, paths))
    st, texts = pad_fixture()
    for delim, rows in ((ord("A"), range(0, 6)), (ord("T"), range(6, 12))):
        sizes = []
        for r in rows:
            body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes()
            L, S = bitwalk.next_table(body, *st.tab)
            symbols = bitwalk.walk_symbols(L, S, 0, L.size)[1]
            assert bytes([delim]) not in texts[r] and symbols.size > len(texts[r]) and symbols[len(texts[r])] == delim  # the pad bits read as the delimiter
            sizes.append(reach(st, r))
        assert min(sizes) <= lane < max(sizes)
    assert int(st.tab[1][ord("x")]) == 0  # a delimiter without a code
    st = cut_fixture()
    stored = [stored_text(st, r) for r in range(st.n)]
    assert all(len(s) < int(l) for s, l in zip(stored, np.diff(st.text_index))) and min(len(s) for s in stored) == 0 and max(len(s) for s in stored) > 30000


def test_the_ladder_and_small_field_fixtures():
    st = ladder_fixture()
    assert [int(st.tab[1][d]) for d in (131, 132, 100, 116)] == [32, 32, 1, 17] and reach(st, 0) > lane_bytes()
    st, rows, field, count = small_fields_fixture()
    bits = {_span(st, 0, int(f), int(c), 100)[1] for f, c in zip(field, count)}
    assert bits >= set(range(34)), sorted(set(range(34)) - bits)


# --- the call's row of the retained-state table ---------------------------------------------------------------------------------------------


def test_the_field_call_has_a_row_that_keeps_both_states():
    from tests import retained as R
    from tests import retained_field as F

    assert R.NAMES.count("field") == 1 and R.row("field") is F.ROW and [r.name for r in R.ROWS] == R.NAMES
    row = R.row("field")
    assert NAME in row.calls and NAME in N.SIGNATURES and (row.hist, row.held, row.names, row.encodes) == (R.KEEPS, R.KEEPS, None, None)
    assert "field" not in R.DROPS_HISTOGRAM | R.DROPS_RANGE
    # what the row's cell asks of the call: Python's split and join over the table's records
    assert [py_field(R.RECORDS[r], 2, 2, SPACE) for r in (2, 4, 3, 0)] == [(b"or not", 6), (b"the question", 8), (b"", ABSENT), (b"", ABSENT)]
