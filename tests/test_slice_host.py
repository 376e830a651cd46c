"""et_slice_packed_device's C ABI as far as it can be checked without a GPU: declared, bound, exported, the argument check that comes
before anything touches a device -- every call-level ET_ERR_ARG, with a null ctx, *res untouched -- and the fixtures of
tests/test_gpu_slice.py: the rule the kernels implement, stated here over tests/bitwalk.py's codeword boundaries (the bits from boundary
i to boundary j, shifted to bit 7 of a byte and padded with zeros), gives on them what the oracle's encode of Python's slices gives,
and they reach the cases the GPU tests take them for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from entreepy_amd import _native as N
from tests import bitwalk
from tests.test_gpu_slice import (ARG, BLOCK_BITS, LANE_BITS, TO_END, bit_at, bytes_fixture, cut_fixture, edge_rows, ladder_fixture, lane_bytes, main_fixture, pad_fixture,
                                  phase_rows, py_slice, reach, set_pad_fixture, stop_rows, stored_text, triples, want_slice)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "et_slice_packed_device"


def test_slice_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in (NAME, "et_slice_lane_bytes"):
        assert name in declared and name in N.SIGNATURES and name in exported, name
    args = re.search(r"int et_slice_packed_device\(([^;]*)\);", header).group(1)
    assert len(N.SIGNATURES[NAME][1]) == len(args.split(",")) == 20 and "et_codebook" in args and "et_take_result" in args
    assert re.search(r"#define ET_SLICE_TO_END 0xffffffffu", header) and re.search(r"#define ET_SLICE_NO_STOP \(-1\)", header)
    assert (N.ET_SLICE_TO_END, N.ET_SLICE_NO_STOP) == (0xFFFFFFFF, -1)
    assert N.lib().et_slice_lane_bytes() > 0


def test_the_python_layer_exposes_the_call_the_list_helper_and_the_constants():
    import entreepy_amd as E

    assert callable(E.Context.slice_packed_device) and callable(E.Context.slice_packed)
    assert (E.SLICE_TO_END, E.SLICE_NO_STOP) == (0xFFFFFFFF, -1)


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    ORDER = ["ctx", "cb", "d_bodies", "body_bytes", "d_body_index", "d_text_index", "n_records", "d_rows", "n_rows", "d_first", "first", "d_count", "count", "stop", "d_out", "cap",
             "d_out_body_index", "d_out_text_index", "d_status", "res"]

    def __init__(self):
        self.res = N.TakeResult(out_bytes=77, text_bytes=78, n_failed=79, first_failed=80, first_status=81)
        self.cb = N.Codebook()
        self.buf = (ctypes.c_uint64 * 64)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, cb=ctypes.addressof(self.cb), d_bodies=p, body_bytes=16, d_body_index=p + 64, d_text_index=p + 80, n_records=1, d_rows=p + 96, n_rows=1,
                      d_first=p + 104, first=0, d_count=p + 112, count=5, stop=-1, d_out=p + 128, cap=16, d_out_body_index=p + 160, d_out_text_index=p + 176, d_status=None,
                      res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        args = [v[k] for k in self.ORDER]
        args[1] = ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None
        args[-1] = ctypes.cast(v["res"], ctypes.POINTER(N.TakeResult)) if v["res"] else None
        rc = N.lib().et_slice_packed_device(*args)
        r = self.res
        assert (r.out_bytes, r.text_bytes, r.n_failed, r.first_failed, r.first_status) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


def test_null_context_is_an_argument_error():
    assert _Args().call() == ARG
    assert N.lib().et_slice_packed_device(None, None, None, 0, None, None, 0, None, 0, None, 0, None, 0, -1, None, 0, None, None, None, None) == ARG


@pytest.mark.parametrize("name", ["cb", "res", "d_bodies", "d_body_index", "d_text_index", "d_out_body_index", "d_out_text_index"])
def test_every_null_pointer_is_an_argument_error_before_a_device_is_touched(name):
    assert _Args().call(**{name: None}) == ARG


@pytest.mark.parametrize("name", ["d_body_index", "d_text_index", "d_out_body_index", "d_out_text_index"])
@pytest.mark.parametrize("by", [1, 4])
def test_a_misaligned_offset_array_is_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("name", ["d_rows", "d_first", "d_count"])
@pytest.mark.parametrize("by", [1, 2, 3])
def test_misaligned_rows_firsts_and_counts_are_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("name", ["n_records", "n_rows"])
def test_more_than_2_31_records_or_rows_are_an_argument_error(name):
    assert _Args().call(**{name: 0x80000000}) == ARG
    assert _Args().call(**{name: 1 << 40}) == ARG


def test_without_rows_the_row_count_is_the_record_count():
    assert _Args().call(d_rows=None, n_rows=2) == ARG
    assert _Args().call(d_rows=None, n_rows=0) == ARG


@pytest.mark.parametrize("stop", [-2, 256, 1 << 20, -(1 << 31)])
def test_a_stop_that_is_no_byte_is_an_argument_error(stop):
    assert _Args().call(stop=stop) == ARG


@pytest.mark.parametrize("where", ["same", "out_begins_inside", "out_ends_inside", "out_around", "last_byte", "first_byte"])
def test_an_output_that_overlaps_the_bodies_is_an_argument_error(where):
    a = _Args()
    b = a.v["d_bodies"]  # the bodies are [b, b + 16)
    d_out, cap = {"same": (b, 16), "out_begins_inside": (b + 8, 16), "out_ends_inside": (b - 8, 16), "out_around": (b - 8, 48), "last_byte": (b + 15, 4),
                  "first_byte": (b - 3, 4)}[where]
    assert a.call(d_out=d_out, cap=cap) == ARG


# --- the rule the kernels implement, in pure Python ---------------------------------------------------------------------------------------


def _walked(st, r):
    """Record r's body as an array of bits, the bits at which the codewords of its stored text begin (one entry more: where the last
    one ends) and their symbols.  Once per store and record."""
    cache = st.__dict__.setdefault("walked_for_slices", {})
    if r not in cache:
        body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])]
        length = int(st.text_index[r + 1]) - int(st.text_index[r])
        symbols = np.zeros(0, np.uint8)
        if body.size:
            L, S = bitwalk.next_table(body.tobytes(), *st.tab)
            symbols = bitwalk.walk_symbols(L, S, 0, L.size)[1][:length]  # the codewords that end inside the body, at most `length` of them
        cache[r] = (np.unpackbits(body), bitwalk.boundaries(0, st.tab[1], symbols), symbols)
    return cache[r]


def rule(st, r, first, count, stop):
    """-> (the new body's bytes, its symbols): bits [boundary i, boundary j) shifted to bit 7 of a byte, the last byte padded with zeros."""
    bits, bounds, symbols = _walked(st, r)
    n = symbols.size
    i, j = min(first, n), min(first + count, n)
    if stop is not None:
        hit = np.flatnonzero(symbols[i:j] == stop)
        j = i + int(hit[0]) if hit.size else j
    return np.packbits(bits[int(bounds[i]) : int(bounds[max(i, j)])]).tobytes(), max(j - i, 0)


def check_rule(st, rows, first, count, stop=None):
    want = want_slice(st, rows, first, count, stop)
    assert not want.status.any()
    rows = np.arange(st.n) if rows is None else rows
    firsts = [int(first)] * len(rows) if np.isscalar(first) else first
    counts = [int(count)] * len(rows) if np.isscalar(count) else count
    for k, (r, f, c) in enumerate(zip(rows, firsts, counts)):
        body, n = rule(st, int(r), int(f), int(c), stop)
        b0, b1 = int(want.body_index[k]), int(want.body_index[k + 1])
        assert (body, n) == (want.data[b0:b1].tobytes(), int(want.text_index[k + 1] - want.text_index[k])), (k, int(r), int(f), int(c), stop)
    return want


def test_the_bit_rule_gives_the_oracles_encode_of_pythons_slices():
    st, texts = main_fixture()
    check_rule(st, *phase_rows())
    check_rule(st, *triples(edge_rows().values()))
    check_rule(st, *triples(stop_rows().values()), stop=ord(" "))
    for stop in (ord(" "), ord("e"), 0xFF):
        check_rule(st, None, 3, 1000, stop=stop)
    lens = np.array([len(t) for t in texts], dtype=np.int64)
    for first in (0, 1, np.maximum(lens - 1, 0), lens, lens + 1, 0xFFFFFFFF):
        for count in (0, 1, 7, lens, TO_END):
            check_rule(st, None, first, count)


def test_the_bit_rule_on_cut_bodies_set_pad_bits_and_long_codewords():
    st = cut_fixture()
    for first, count in ((0, TO_END), (2, 0xFFFFFFF0), (5, 40)):
        check_rule(st, None, first, count)
    st, texts = set_pad_fixture()
    own, _ = main_fixture()
    whole = check_rule(st, None, 0, TO_END)
    assert np.array_equal(whole.data, own.bodies) and not np.array_equal(st.bodies, own.bodies)  # the pad is masked, not copied
    check_rule(st, None, 1, TO_END)
    st, texts = pad_fixture()
    for stop in (ord("A"), ord("T"), ord("x")):
        check_rule(st, None, 0, TO_END, stop=stop)
        check_rule(st, None, 1, 0xFFFFFFF0, stop=stop)
    st = ladder_fixture()
    check_rule(st, *triples([(0, 33 * k + i, c) for k in (0, 39) for i in range(33) for c in (0, 1, 2)] + [(3, i, c) for i in range(18) for c in (1, 2, 3)]))
    check_rule(st, None, 1, TO_END)
    st = bytes_fixture()
    check_rule(st, [0, 1, 0], [1, 0, 0], [997, 40, 3])


# --- the fixtures are what the GPU tests take them for --------------------------------------------------------------------------------------


def _span(st, r, first, count, stop=None):
    """-> (the bit at which the slice begins, as the kernels count; the bits it has)."""
    n = len(py_slice(stored_text(st, r), first, count, stop))
    return bit_at(st, r, first), bit_at(st, r, first + n) - bit_at(st, r, first)


def test_the_main_fixture_reaches_every_bit_phase_on_both_paths():
    st, texts = main_fixture()
    lane = lane_bytes()
    sizes = np.diff(st.body_index.astype(np.int64))
    assert sizes.min() == 0 and 0 < sizes[sizes > 0].min() <= 2 and sizes[8] <= lane < sizes[9] and sizes.max() > 2 * BLOCK_BITS // 8  # bodies on both sides of the threshold
    seen = {"lane": set(), "workgroup": set()}
    spans_lanes = 0
    for r, f, c in zip(*phase_rows()):
        begin, bits = _span(st, int(r), int(f), int(c))
        if bits == 0:
            continue
        path = "lane" if reach(st, int(r), int(f), int(c)) <= lane else "workgroup"
        seen[path].add((begin % 8, bits % 8))
        spans_lanes += path == "workgroup" and begin // LANE_BITS < (begin + bits - 1) // LANE_BITS
    assert len(seen["lane"]) == 64 and len(seen["workgroup"]) == 64, {k: len(v) for k, v in seen.items()}
    assert spans_lanes >= 50  # slices that begin in one 256-bit lane and end in a later one


def test_the_edge_rows_lie_at_the_lane_and_block_edges():
    st, texts = main_fixture()
    lane = lane_bytes()
    spans = {case: _span(st, *row) for case, row in edge_rows().items()}
    for case, row in edge_rows().items():
        assert (reach(st, *row) > lane) == (case != "short_of_long"), case
    begin, bits = spans["lane_edge"]
    assert begin // LANE_BITS + 1 == (begin + bits - 1) // LANE_BITS and bits <= 64
    begin, bits = spans["lanes"]
    assert (begin + bits) // LANE_BITS - begin // LANE_BITS >= 4
    begin, bits = spans["block_edge"]
    assert begin < BLOCK_BITS < begin + bits  # begins in block 0, ends in block 1
    begin, bits = spans["block_end"]
    assert begin < BLOCK_BITS and BLOCK_BITS - 32 < begin + bits <= BLOCK_BITS  # ends with block 0's last codeword
    begin, bits = spans["block_begin"]
    assert BLOCK_BITS <= begin < BLOCK_BITS + 32
    begin, bits = spans["blocks"]
    assert begin < LANE_BITS and begin + bits > 2 * BLOCK_BITS


def test_the_stop_rows_are_the_cases_they_are_named_for():
    st, texts = main_fixture()
    lane, stop = lane_bytes(), b" "
    for case, (r, first, count) in stop_rows().items():
        t = texts[r]
        assert (reach(st, r, first, count) > lane) == case.startswith("long"), case
        if case.endswith("at_first"):
            assert t[first : first + 1] == stop
        if case.endswith("inside"):
            assert 0 < t[first : first + count].find(stop)
        if case.endswith("behind_count"):  # the stop first occurs only behind first + count
            assert stop not in t[first : first + count] and t[first + count : first + count + 1] == stop and count >= 2
        if case.endswith("absent"):
            assert stop not in t[first : first + count + 1]


def test_the_pad_fixture_has_pad_bits_that_read_as_the_stop():
    st, texts = pad_fixture()
    lane = lane_bytes()
    for stop, rows in ((ord("A"), range(0, 6)), (ord("T"), range(6, 12))):
        sizes = []
        for r in rows:
            body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes()
            L, S = bitwalk.next_table(body, *st.tab)
            symbols = bitwalk.walk_symbols(L, S, 0, L.size)[1]
            assert bytes([stop]) not in texts[r] and symbols.size > len(texts[r]) and symbols[len(texts[r])] == stop  # the pad bits read as the stop
            assert symbols[: len(texts[r])].tobytes() == texts[r] == stored_text(st, r)
            sizes.append(len(body))
        assert min(sizes) <= lane < max(sizes)
    assert int(st.tab[1][ord("x")]) == 0  # a stop byte without a code


def test_the_cut_ladder_and_bytes_fixtures():
    st = cut_fixture()
    stored = [len(stored_text(st, r)) for r in range(st.n)]
    assert all(s < int(l) for s, l in zip(stored, np.diff(st.text_index))) and min(stored) == 0 and max(stored) > 30000
    st = ladder_fixture()
    assert sorted(set(int(st.tab[1][s]) for s in stored_text(st, 0))) == list(range(1, 33)) and int(st.body_index[1]) > lane_bytes()
    one = {_span(st, 0, i, 1)[1] for i in range(33)} | {_span(st, 0, 32, 2)[1], _span(st, 0, 15, 2)[1]}
    assert one == set(range(1, 34))
    st = bytes_fixture()
    assert _span(st, 0, 1, 100) == (7, 800) and _span(st, 1, 1, 100) == ((int(st.body_index[1]) % 4) * 8 + 8, 800)


# --- the call's row of the retained-state table ---------------------------------------------------------------------------------------------


def test_the_slice_call_has_a_row_that_keeps_both_states():
    from tests import retained as R
    from tests import retained_slice as S

    assert R.NAMES.count("slice") == 1 and R.row("slice") is S.ROW and [r.name for r in R.ROWS] == R.NAMES
    row = R.row("slice")
    assert NAME in row.calls and NAME in N.SIGNATURES and (row.hist, row.held, row.names, row.encodes) == (R.KEEPS, R.KEEPS, None, None)
    assert "slice" not in R.DROPS_HISTOGRAM | R.DROPS_RANGE
    cut = lambda t: t[3:12].split(b"t")[0]  # noqa: E731  (what the row's cell asks of the call: Python's slices of the table's records)
    assert [cut(R.RECORDS[r]) for r in (2, 4, 3)] == [b"be or no", b"", b""]
