"""et_number_packed_device's C ABI as far as it can be checked without a GPU: declared, bound, exported, the result struct's size, the
argument check that comes before anything touches a device -- every call-level ET_ERR_ARG, with a null ctx, *res untouched -- and the
fixtures of tests/test_gpu_number.py: the rule the kernels implement, stated here over tests/bitwalk.py's codeword boundaries (the
symbols from boundary `first` on, up to the count, the length, the bits' end or the stop, through a digit-by-digit state machine
whose magnitude saturates), gives on them what number_rule() -- a regular expression and int() -- gives over the oracle's texts,
and they reach the cases the GPU tests take them for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from entreepy_amd import _native as N
from tests import bitwalk
from tests.test_gpu_number import (ARG, BLOCK_BITS, GRAMMAR_BAD, GRAMMAR_OK, GRAMMAR_RANGE, I64_MAX, I64_MIN, LADDER_32, LANE_BITS, N_BAD, N_EMPTY, N_OK, N_RANGE,
                                   NONE, STRINGS, SYMBOLS_MAX, TO_END, VARIANTS, bit_at, column_asks, column_fixture, edge_fixture, failures_fixture, grammar_fixture,
                                   grammar_rows, lane_bytes, no_symbol_fixture, number_rule, pages_fixture, per_row, reach, set_pad_fixture, stored_text, tables_fixture,
                                   want_number, wrap64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "et_number_packed_device"
NAMES = (NAME, "et_number_result_size", "et_number_symbols_max", "et_number_lane_bytes")


def test_number_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared and name in N.SIGNATURES and name in exported, name
    args = re.search(r"int et_number_packed_device\(([^;]*)\);", header).group(1)
    assert len(N.SIGNATURES[NAME][1]) == len(args.split(",")) == 24 and "et_codebook" in args and "et_number_result" in args and "const uint32_t *d_group_of" in args
    for name, value in (("OK", 0), ("EMPTY", 1), ("BAD", 2), ("RANGE", 3)):
        assert re.search(r"#define ET_NUMBER_%s %d\b" % (name, value), header) and getattr(N, "ET_NUMBER_" + name) == value
    assert N.lib().et_number_symbols_max() == SYMBOLS_MAX == 32 and N.lib().et_number_lane_bytes() == N.lib().et_slice_lane_bytes() > 0


def test_the_struct_has_the_size_the_headers_layout_implies():
    """uint64_t n_ok, n_empty, n_bad, n_range, n_failed, first_failed; int32_t first_status; uint32_t pad: 6 * 8 + 4 + 4 bytes."""
    assert [(name, ctypes.sizeof(t)) for name, t in N.NumberResult._fields_] == [("n_ok", 8), ("n_empty", 8), ("n_bad", 8), ("n_range", 8), ("n_failed", 8), ("first_failed", 8),
                                                                               ("first_status", 4), ("pad", 4)]
    assert N.lib().et_number_result_size() == ctypes.sizeof(N.NumberResult) == 56


def test_the_python_layer_exposes_the_calls_and_the_constants():
    import entreepy_amd as E

    assert callable(E.Context.number_packed_device) and callable(E.Context.number_packed)
    assert (E.NUMBER_OK, E.NUMBER_EMPTY, E.NUMBER_BAD, E.NUMBER_RANGE) == (0, 1, 2, 3)
    assert [f.name for f in E.NumberResult.__dataclass_fields__.values()] == ["status", "n_ok", "n_empty", "n_bad", "n_range", "n_failed", "first_failed", "first_status"]


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    ORDER = ["ctx", "cb", "d_bodies", "body_bytes", "d_body_index", "d_text_index", "n_records", "d_rows", "n_rows", "d_first", "first", "d_count", "count", "stop", "d_values",
             "d_kind", "d_group_of", "n_groups", "d_sum", "d_n", "d_min", "d_max", "d_status", "res"]

    def __init__(self):
        self.res = N.NumberResult(n_ok=71, n_empty=72, n_bad=73, n_range=74, n_failed=75, first_failed=76, first_status=77)
        self.cb = N.Codebook()
        self.buf = (ctypes.c_uint64 * 64)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, cb=ctypes.addressof(self.cb), d_bodies=p, body_bytes=16, d_body_index=p + 64, d_text_index=p + 80, n_records=1, d_rows=p + 96, n_rows=1,
                      d_first=p + 104, first=0, d_count=p + 112, count=5, stop=-1, d_values=p + 128, d_kind=p + 136, d_group_of=p + 144, n_groups=1, d_sum=p + 160, d_n=p + 168,
                      d_min=p + 176, d_max=p + 184, d_status=None, res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        args = [v[k] for k in self.ORDER]
        args[1] = ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None
        args[-1] = ctypes.cast(v["res"], ctypes.POINTER(N.NumberResult)) if v["res"] else None
        rc = N.lib().et_number_packed_device(*args)
        r = self.res
        assert (r.n_ok, r.n_empty, r.n_bad, r.n_range, r.n_failed, r.first_failed, r.first_status) == (71, 72, 73, 74, 75, 76, 77), "*res was touched"
        return rc


def test_null_context_is_an_argument_error():
    assert _Args().call() == ARG
    assert N.lib().et_number_packed_device(None, None, None, 0, None, None, 0, None, 0, None, 0, None, 0, -1, None, None, None, 0, None, None, None, None, None, None) == ARG


@pytest.mark.parametrize("name", ["cb", "res", "d_bodies", "d_body_index", "d_text_index"])
def test_every_null_pointer_is_an_argument_error_before_a_device_is_touched(name):
    assert _Args().call(**{name: None}) == ARG


@pytest.mark.parametrize("name", ["d_body_index", "d_text_index", "d_values", "d_sum", "d_n", "d_min", "d_max"])
@pytest.mark.parametrize("by", [1, 4])
def test_a_misaligned_array_of_64_bit_entries_is_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("name", ["d_rows", "d_first", "d_count", "d_group_of"])
@pytest.mark.parametrize("by", [1, 2, 3])
def test_a_misaligned_array_of_32_bit_entries_is_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


def test_the_slice_calls_other_argument_errors_and_the_aggregates_own():
    assert _Args().call(n_records=0x80000000) == ARG and _Args().call(n_rows=1 << 40) == ARG
    assert _Args().call(d_rows=None, n_rows=2) == ARG and _Args().call(d_rows=None, n_rows=0) == ARG
    for stop in (-2, 256, 1 << 20, -(1 << 31)):
        assert _Args().call(stop=stop) == ARG
    assert _Args().call(d_sum=None, d_n=None, d_min=None, d_max=None) == ARG  # group numbers without an aggregate output
    assert _Args().call(n_groups=0) == ARG and _Args().call(n_groups=0x80000000) == ARG
    assert _Args().call(d_group_of=None, n_groups=2) == ARG  # without group numbers every row is in group 0


# --- the rule the kernels implement, in pure Python ---------------------------------------------------------------------------------------


def _symbols(st, r):
    """The symbols of record r's stored text by tests/bitwalk.py's walk: the codewords that end inside the body, at most `length`."""
    cache = st.__dict__.setdefault("walked_for_numbers", {})
    if r not in cache:
        body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])]
        length = int(st.text_index[r + 1]) - int(st.text_index[r])
        cache[r] = np.zeros(0, np.uint8)
        if body.size and length:
            L, S = bitwalk.next_table(body.tobytes(), *st.tab)
            cache[r] = bitwalk.walk_symbols(L, S, 0, L.size)[1][:length]
    return cache[r]


def rule(st, r, first, count, stop):
    """-> (kind, value): the state machine over the symbols from `first` on -- sign seen, digits seen, the magnitude saturating at
    2^64 - 1, symbols seen, bad -- ended by the count, the stop or the first symbol that makes the row BAD."""
    symbols = _symbols(st, r)
    mag, n, neg, digits, over = 0, 0, False, False, False
    for sym in symbols[min(first, symbols.size) : min(first + count, symbols.size)].tolist():
        if sym == stop:
            break
        n += 1
        if n > SYMBOLS_MAX:
            return N_BAD, 0
        if ord("0") <= sym <= ord("9"):
            digits = True
            mag = mag * 10 + sym - ord("0")
            if mag > (1 << 64) - 1:
                mag, over = (1 << 64) - 1, True
        elif n == 1 and sym in b"+-":
            neg = sym == ord("-")
        else:
            return N_BAD, 0
    if n == 0:
        return N_EMPTY, 0
    if not digits:
        return N_BAD, 0
    if over or mag > ((1 << 63) if neg else (1 << 63) - 1):
        return N_RANGE, 0
    return N_OK, -mag if neg else mag


def check_rule(st, rows, first, count, stop=None):
    want = want_number(st, rows, first, count, stop)
    assert not want.status.any()
    rows = np.arange(st.n) if rows is None else rows
    if isinstance(stop, bytes):
        (stop,) = stop
    for k, (r, f, c) in enumerate(zip(rows, per_row(first, len(rows)), per_row(count, len(rows)))):
        assert rule(st, int(r), f, c, stop) == (int(want.kind[k]), int(want.values[k])), (k, int(r), f, c, stop, want.texts[k])
    return want


def test_the_rule_on_the_grammar_table():
    st, texts = grammar_fixture()
    lens = np.array([len(s) for s in STRINGS])
    for variant in VARIANTS:
        rows, first = grammar_rows(variant)
        want = check_rule(st, rows, first, TO_END, b";")
        assert want.texts == STRINGS
        kinds = dict(zip(STRINGS, want.kind.tolist()))
        assert kinds[b""] == N_EMPTY and all(kinds[s] == N_OK for s in GRAMMAR_OK) and all(kinds[s] == N_BAD for s in GRAMMAR_BAD) and all(kinds[s] == N_RANGE for s in GRAMMAR_RANGE)
        for count in (0, 1, 5, lens, 0xFFFFFFFF):
            check_rule(st, rows, first, count, b";")
            check_rule(st, rows, first + lens // 2, count)
        check_rule(st, rows, first, TO_END, 0xFF)
        check_rule(st, rows, first, TO_END, b"0")
    assert number_rule(b"1" + b"0" * 31) == (N_RANGE, 0) and number_rule(b"%d" % I64_MIN) == (N_OK, I64_MIN) and number_rule(b"0" * 32 + b"1") == (N_BAD, 0)


def test_the_rule_on_the_other_fixtures():
    st, texts, cases = edge_fixture()
    rows, first, nums = zip(*cases.values())
    assert check_rule(st, list(rows), list(first), TO_END, b";").values.tolist() == [int(x) for x in nums]
    for name, (st, texts, asks) in tables_fixture().items():
        check_rule(st, *(list(x) for x in zip(*asks)))
    st, asks = no_symbol_fixture()
    rows, first = (list(x) for x in zip(*asks))
    check_rule(st, rows, first, TO_END)
    check_rule(st, rows, first, TO_END, b"5")
    st, texts = set_pad_fixture()
    check_rule(st, None, 0, TO_END)
    check_rule(st, None, np.array([len(t) - 3 for t in texts]), 19)
    st, lines = column_fixture()
    want = check_rule(st, None, column_asks(lines), TO_END, b",")
    assert want.texts == [line.split(b",")[2] for line in lines]
    st, pages = pages_fixture()
    hits = [k for k, p in enumerate(pages) if b"user=" in p]
    check_rule(st, hits, [pages[k].index(b"user=") + 5 for k in hits], TO_END, b";")


# --- the fixtures are what the GPU tests take them for --------------------------------------------------------------------------------------


def test_the_grammar_fixture_has_every_string_on_both_paths():
    st, texts = grammar_fixture()
    lane = lane_bytes()
    for variant in VARIANTS:
        rows, first = grammar_rows(variant)
        for r, s in zip(rows, STRINGS):
            assert (reach(st, int(r), first, TO_END) > lane) == variant.startswith("long"), (variant, s)
            assert texts[r][first:].startswith(s) and (texts[r][first + len(s) : first + len(s) + 3] == b";x9") == variant.endswith("closed")
            if s:  # (an ask of the string's own count reaches as far: the long records' numbers lie behind 1 500 symbols)
                assert (reach(st, int(r), first, len(s)) > lane) == variant.startswith("long")
    assert int(st.tab[1][0xFF]) == 0 and all(int(st.tab[1][b]) for b in b" a+-0123456789;=")


def _span(st, r, first, n):
    """-> the bits [a, b), as the kernels count them, of symbols [first, first + n) of record r."""
    return bit_at(st, r, first), bit_at(st, r, first + n)


def test_the_edge_fixture_straddles_the_edges_it_names():
    st, texts, cases = edge_fixture()
    lane = lane_bytes()
    spans = {case: _span(st, r, first, len(num)) for case, (r, first, num) in cases.items()}
    for case in ("lane_edge", "lane_edge_32"):
        a, b = spans[case]
        assert a // LANE_BITS + 1 == (b - 1) // LANE_BITS and a % 8 == 7  # its first and last digit on either side of a lane's 256 bits
    assert len(cases["lane_edge_32"][2]) == SYMBOLS_MAX
    a, b = spans["block_edge"]
    assert a < BLOCK_BITS < b - 8
    a, b = spans["second_block_edge"]
    assert a < 2 * BLOCK_BITS < b - 8
    a, b = spans["body_end"]
    assert 2 * BLOCK_BITS < a and b == 8 * int(st.body_index[1]) - 1 and texts[0].endswith(cases["body_end"][2])  # the body's last codeword, a pad bit behind it
    for d in (-1, 0, 1, 2):
        r, first, num = cases["threshold%+d" % d]
        assert int(st.body_index[r + 1] - st.body_index[r]) == reach(st, r, first, TO_END) == lane + d and texts[r].endswith(num)


def test_the_tables_and_what_is_no_symbol():
    two, _, asks2 = tables_fixture()["digits_2bit"]
    assert sorted(int(two.tab[1][s]) for s in b"0123") == [2, 2, 2, 2] and int(two.tab[1].astype(np.int64).sum()) == 8
    lad, lad_texts, asksl = tables_fixture()["digit_ladder"]
    assert [int(lad.tab[1][s]) for s in b"+-0123456789"] == [22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 32]
    a, b = _span(lad, 1, 400, 32)
    assert b - a == 13 * 24 + 32 + 18 * 32 == 920 and lad_texts[1][400:] == LADDER_32 and reach(lad, 1, 400, TO_END) > lane_bytes() >= reach(lad, 0, 2, TO_END)
    for st, asks in ((two, asks2), (lad, asksl)):
        paths = {reach(st, r, f, c) > lane_bytes() for r, f, c in asks}
        assert paths == {False, True}
    st, asks = no_symbol_fixture()
    want = want_number(st, *(list(x) for x in zip(*asks)), TO_END)
    for half, long_ in ((0, False), (5, True)):
        rows = [r for r, _ in asks[half : half + 5]]
        assert [reach(st, r, f, TO_END) > lane_bytes() for r, f in asks[half : half + 3]] == [long_] * 3
        L, S = bitwalk.next_table(st.bodies[int(st.body_index[rows[0]]) : int(st.body_index[rows[0] + 1])].tobytes(), *st.tab)
        behind = bitwalk.walk_symbols(L, S, 0, L.size)[1][len(stored_text(st, rows[0])) :]
        assert bytes(behind[:9]) == b"567890123"  # codewords behind the length that read as digits
        assert want.texts[half] == b"1234" and 0 < len(want.texts[half + 2]) < len(want.texts[half + 1]) < 13  # cut bodies: the number ends where the bits do
        assert int(st.body_index[rows[3] + 1] - st.body_index[rows[3]]) == 0 < int(st.text_index[rows[3] + 1] - st.text_index[rows[3]])  # kept raw
        assert want.kind[half + 3 : half + 5].tolist() == [N_EMPTY, N_EMPTY]
    st, texts = set_pad_fixture()
    for r, t in enumerate(texts):
        L, S = bitwalk.next_table(st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes(), *st.tab)
        symbols = bitwalk.walk_symbols(L, S, 0, L.size)[1]
        assert b"3" not in t and symbols.size == len(t) + 1 and symbols[len(t)] == ord("3") and stored_text(st, r) == t  # the pad bits read as a digit
    assert [reach(st, r, len(t) - 3, 19) > lane_bytes() for r, t in enumerate(texts)] == [False, False, False, True, True]


def test_the_column_fixture_has_every_kind_and_sums_that_wrap():
    st, lines = column_fixture()
    want = want_number(st, None, column_asks(lines), TO_END, b",", n_groups=1)
    assert st.n == 4097 and min(want.counts[k] for k in ("n_ok", "n_empty", "n_bad", "n_range")) >= 30 and want.counts["n_failed"] == 0
    true_sum = sum(int(v) for v in want.values[want.kind == N_OK])
    assert true_sum > I64_MAX and want.sum[0] == wrap64(true_sum) != true_sum and want.min[0] < I64_MIN + 1000 and want.max[0] > I64_MAX - 1000
    first = want_number(st, np.arange(513), column_asks(lines)[:513], TO_END, b",", n_groups=1)
    assert first.min[0] < I64_MIN + 1000 and first.max[0] > I64_MAX - 1000
    st, pages = pages_fixture()
    hits = [k for k, p in enumerate(pages) if b"user=" in p]
    paths = {reach(st, k, pages[k].index(b"user=") + 5, TO_END) > lane_bytes() for k in hits}
    assert paths == {False, True} and 0 < len(hits) < st.n


def test_the_failures_fixture_fails_the_rows_it_names():
    st, bad = failures_fixture()
    want = want_number(st, np.arange(18), 2, TO_END, b";", group_of=[0] * 18, n_groups=1)
    assert {k: int(s) for k, s in enumerate(want.status) if s} == {**bad, 16: ARG, 17: ARG}
    group_of = [0, 1, 2, NONE] + [0] * 14
    want = want_number(st, np.arange(18), 2, TO_END, b";", group_of=group_of, n_groups=2)
    assert int(want.status[2]) == ARG and int(want.status[3]) == ARG and int(want.status[0]) == int(want.status[1]) == 0 and want.n == [want.counts["n_ok"] - 1, 1]


# --- the call's row of the retained-state table ---------------------------------------------------------------------------------------------


def test_the_number_call_has_a_row_that_keeps_both_states():
    from tests import retained as R
    from tests import retained_number as S

    assert R.NAMES.count("number") == 1 and R.row("number") is S.ROW and [r.name for r in R.ROWS] == R.NAMES
    row = R.row("number")
    assert NAME in row.calls and NAME in N.SIGNATURES and (row.hist, row.held, row.names, row.encodes) == (R.KEEPS, R.KEEPS, None, None)
    assert "number" not in R.DROPS_HISTOGRAM | R.DROPS_RANGE
    cut = lambda t: t[3:12].split(b"t")[0]  # noqa: E731  (what the row's cell asks of the call: Python's slices of the table's records)
    assert [number_rule(cut(R.RECORDS[r]))[0] for r in (2, 4, 3)] == [N_BAD, N_EMPTY, N_EMPTY]
