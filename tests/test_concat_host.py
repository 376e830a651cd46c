"""et_concat_packed_device's C ABI as far as it can be checked without a GPU: declared, bound, exported, the argument check that comes
before anything touches a device -- every call-level ET_ERR_ARG, with a null ctx, *res untouched -- and the fixtures of
tests/test_gpu_concat.py: the rule the kernels implement, stated here over strings of bits (each side's codewords as tests/bitwalk.py
finds them, from the first one's first bit to the last one's last, the literal's bits between them, packed from bit 7 of a byte and
padded with zeros), gives on them what the oracle's encode of the concatenated stored texts gives, and they reach the cases the GPU
tests take them for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from entreepy_amd import _native as N
from tests.test_gpu_concat import (ARG, BLOCK, OK, UNSUPPORTED, bits_of, dna_fixture, edge_fixture, empties_fixture, empty_run_rows, lane_bytes, left_reach, limit_fixture,
                                   literals, main_rows, right_pad_fixture, want_concat)
from tests.test_gpu_shared import _cb, want_decode
from tests.test_gpu_slice import cut_fixture, ladder_fixture, main_fixture, set_pad_fixture, stored_text
from tests.test_gpu_take import C, SCAN_TILE
from tests.test_slice_host import _walked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "et_concat_packed_device"


def test_concat_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in (NAME, "et_concat_lane_bytes", "et_concat_sep_max"):
        assert name in declared and name in N.SIGNATURES and name in exported, name
    args = re.search(r"int et_concat_packed_device\(([^;]*)\);", header).group(1)
    assert len(N.SIGNATURES[NAME][1]) == len(args.split(",")) == 23 and "et_codebook" in args and "et_take_result" in args
    assert N.lib().et_concat_lane_bytes() == N.lib().et_slice_lane_bytes() > 0 and N.lib().et_concat_sep_max() == N.lib().et_search_needle_max() == 256


def test_the_python_layer_exposes_the_call_and_the_list_helper():
    import entreepy_amd as E

    assert callable(E.Context.concat_packed_device) and callable(E.Context.concat_packed)


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    ORDER = ["ctx", "cb", "d_a_bodies", "a_body_bytes", "d_a_body_index", "d_a_text_index", "n_a", "d_rows_a", "sep", "sep_len", "d_b_bodies", "b_body_bytes", "d_b_body_index",
             "d_b_text_index", "n_b", "d_rows_b", "n_rows", "d_out", "cap", "d_out_body_index", "d_out_text_index", "d_status", "res"]

    def __init__(self):
        self.res = N.TakeResult(out_bytes=77, text_bytes=78, n_failed=79, first_failed=80, first_status=81)
        self.cb = N.Codebook()
        self.buf = (ctypes.c_uint64 * 96)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, cb=ctypes.addressof(self.cb), d_a_bodies=p, a_body_bytes=16, d_a_body_index=p + 64, d_a_text_index=p + 80, n_a=1, d_rows_a=p + 96, sep=p + 104,
                      sep_len=2, d_b_bodies=p + 256, b_body_bytes=16, d_b_body_index=p + 320, d_b_text_index=p + 336, n_b=1, d_rows_b=p + 352, n_rows=1, d_out=p + 128, cap=16,
                      d_out_body_index=p + 160, d_out_text_index=p + 176, d_status=None, res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        args = [v[k] for k in self.ORDER]
        args[1] = ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None
        args[-1] = ctypes.cast(v["res"], ctypes.POINTER(N.TakeResult)) if v["res"] else None
        rc = N.lib().et_concat_packed_device(*args)
        r = self.res
        assert (r.out_bytes, r.text_bytes, r.n_failed, r.first_failed, r.first_status) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


ABSENT = {side: {f"d_{side}_bodies": None, f"{side}_body_bytes": 0, f"d_{side}_body_index": None, f"d_{side}_text_index": None, f"n_{side}": 0, f"d_rows_{side}": None}
          for side in "ab"}


def test_null_context_is_an_argument_error():
    assert _Args().call() == ARG
    assert _Args().call(**ABSENT["a"]) == ARG and _Args().call(**ABSENT["b"]) == ARG  # (well-formed; the null ctx alone)
    assert N.lib().et_concat_packed_device(None, None, None, 0, None, None, 0, None, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, None, None, None) == ARG


@pytest.mark.parametrize("name", ["cb", "res", "d_a_body_index", "d_a_text_index", "d_b_body_index", "d_b_text_index", "d_out_body_index", "d_out_text_index", "sep"])
def test_every_null_pointer_is_an_argument_error_before_a_device_is_touched(name):
    assert _Args().call(**{name: None}) == ARG


def test_both_sides_absent_and_half_absent_sides_are_argument_errors():
    assert _Args().call(**ABSENT["a"], **ABSENT["b"]) == ARG
    for side in "ab":
        for name, value in ((f"n_{side}", 1), (f"{side}_body_bytes", 8), (f"d_{side}_body_index", 64), (f"d_{side}_text_index", 64)):
            a = _Args()
            assert a.call(**dict(ABSENT[side], **{name: a.v[f"d_{side}_bodies"] + value if name.startswith("d_") else value})) == ARG, name


@pytest.mark.parametrize("name", ["d_a_body_index", "d_a_text_index", "d_b_body_index", "d_b_text_index", "d_out_body_index", "d_out_text_index"])
@pytest.mark.parametrize("by", [1, 4])
def test_a_misaligned_offset_array_is_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("name", ["d_rows_a", "d_rows_b"])
@pytest.mark.parametrize("by", [1, 2, 3])
def test_misaligned_rows_are_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("name", ["n_a", "n_b", "n_rows"])
def test_more_than_2_31_records_or_rows_are_an_argument_error(name):
    assert _Args().call(**{name: 0x80000000}) == ARG
    assert _Args().call(**{name: 1 << 40}) == ARG


@pytest.mark.parametrize("side", ["a", "b"])
def test_without_rows_the_row_count_is_that_sides_record_count(side):
    assert _Args().call(**{f"d_rows_{side}": None, "n_rows": 2}) == ARG
    assert _Args().call(**{f"d_rows_{side}": None, "n_rows": 0}) == ARG


def test_a_literal_above_the_limit_is_an_argument_error():
    assert _Args().call(sep_len=257) == ARG and _Args().call(sep_len=1 << 40) == ARG


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("where", ["same", "out_begins_inside", "out_ends_inside", "out_around", "last_byte", "first_byte"])
def test_an_output_that_overlaps_either_sides_bodies_is_an_argument_error(side, where):
    a = _Args()
    b = a.v[f"d_{side}_bodies"]  # the bodies are [b, b + 16)
    d_out, cap = {"same": (b, 16), "out_begins_inside": (b + 8, 16), "out_ends_inside": (b - 8, 16), "out_around": (b - 8, 48), "last_byte": (b + 15, 4),
                  "first_byte": (b - 3, 4)}[where]
    assert a.call(d_out=d_out, cap=cap) == ARG


# --- the rule the kernels implement, in pure Python ---------------------------------------------------------------------------------------


def rule(A, ra, sep, B, rb):
    """-> (the new body's bytes, its length): each side's stored text's bits -- from its first codeword's first bit to its last one's
    last, the pad dropped -- with the literal's bits between them, packed from bit 7 of a byte, the last byte padded with zeros; the
    symbols of the three."""
    runs, length = [], len(sep)
    for st, r in ((A, ra), (None, None), (B, rb)):
        if r is None:
            body, n_bits = (A or B).cb.encode_pattern(sep)
            runs.append(np.unpackbits(np.frombuffer(body, np.uint8))[:n_bits])
        elif st is not None:
            bits, bounds, symbols = _walked(st, r)
            runs.append(bits[int(bounds[0]) : int(bounds[-1])])
            length += symbols.size
    return np.packbits(np.concatenate(runs)).tobytes(), length


def check_rule(A, B, rows_a, rows_b, sep):
    """The rule against want_concat(): the oracle's encode of the concatenated stored texts, byte for byte."""
    want = want_concat(A, B, rows_a, rows_b, sep)
    assert not want.status.any()
    n = want.status.size
    rows_a = np.arange(n) if rows_a is None else rows_a
    rows_b = np.arange(n) if rows_b is None else rows_b
    seen, tab = set(), (A or B).tab
    for k, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        if (int(ra), int(rb)) in seen:
            continue
        seen.add((int(ra), int(rb)))
        body, length = rule(A, int(ra), sep, B, int(rb))
        b0, b1 = int(want.body_index[k]), int(want.body_index[k + 1])
        assert (body, length) == (want.data[b0:b1].tobytes(), int(want.text_index[k + 1] - want.text_index[k])), (k, int(ra), int(rb), sep)
        assert want_decode(tab, body, length)[1] == want.texts[k], (k, int(ra), int(rb))
    return want


def test_the_bit_rule_gives_the_oracles_encode_of_the_concatenated_texts():
    st, _ = main_fixture()
    rows_a, rows_b = main_rows()
    for literal in (0, 1, 4, 7, "byte", "long"):
        check_rule(st, st, rows_a[:150], rows_b[:150], literals()[literal])
    check_rule(st, None, rows_a[:60], None, literals()[3])
    check_rule(None, st, None, rows_b[:60], literals()[3])
    st, _ = dna_fixture()
    for sep in (b"", b"A", b"ACGT"):
        check_rule(st, st, np.arange(41), np.arange(41)[::-1], sep)
    st = ladder_fixture()
    check_rule(st, st, [0, 1, 2, 3, 3], [3, 3, 3, 3, 0], bytes([100]))
    st, at = edge_fixture()
    check_rule(st, st, [at["mid"], at["lane+1m"], at["few"]], [at["few"], at["mid"], at["lane"]], b"\x01\x09")


def test_the_bit_rule_on_hand_made_bodies():
    st = empties_fixture()
    rows = np.array([(a, b) for a in range(st.n) for b in range(st.n)])
    check_rule(st, st, rows[:, 0], rows[:, 1], literals()[3])
    own, _ = dna_fixture()
    st = right_pad_fixture()
    rows = np.arange(st.n)
    for A, B in ((st, st), (st, None), (None, st)):  # set pad bits are masked on either side: the encoder's bytes
        want = check_rule(A, B, rows if A else None, rows[::-1] if B else None, b"C")
        assert np.array_equal(want.data, want_concat(A and own, B and own, rows if A else None, rows[::-1] if B else None, b"C").data)
    st, own = cut_fixture(), main_fixture()[0]
    rows = np.arange(st.n)
    right = check_rule(own, st, rows % own.n, rows, b"; ")  # a body that ends before its length gives what it holds
    assert all(len(t) < len(stored_text(own, int(k % own.n))) + 2 + int(st.text_index[k + 1] - st.text_index[k]) for k, t in zip(rows, right.texts))
    check_rule(st, own, rows, rows % own.n, b"; ")


# --- the fixtures are what the GPU tests take them for --------------------------------------------------------------------------------------


def test_the_literals_take_every_bit_count():
    st, _ = main_fixture()
    lit = literals()
    assert [bits_of(st.tab, lit[k]) % 8 for k in range(8)] == list(range(8)) and lit[0] == b"" and bits_of(st.tab, lit["byte"]) % 8 == 0 < bits_of(st.tab, lit["byte"])
    assert bits_of(ladder_fixture().tab, bytes([100])) == 1 and bits_of(dna_fixture()[0].tab, b"ACG") == 6 and bits_of(edge_fixture()[0].tab, b"\x01") == 7  # few bits in all
    assert len(lit["long"]) == N.lib().et_concat_sep_max() and all(st.tab[1][s] for s in lit["long"])
    assert (_cb(st.tab).encode_pattern(lit["long"])[1] + 7) // 8 <= 1024


def test_the_main_rows_reach_every_left_bit_count_on_both_paths_and_rows_that_end_on_bytes():
    st, texts = main_fixture()
    rows_a, rows_b = main_rows()
    lane = lane_bytes()
    seen = {"lane": set(), "workgroup": set()}
    for ra in rows_a:
        if len(texts[ra]):
            seen["lane" if left_reach(st, int(ra)) <= lane else "workgroup"].add(bits_of(st.tab, texts[ra]) % 8)
    assert seen["lane"] == set(range(8)) and len(seen["workgroup"]) >= 4, seen
    sizes = np.diff(st.body_index.astype(np.int64))
    assert sizes.max() > 2 * BLOCK and int((sizes > lane).sum()) >= 5  # the long walk carries across blocks
    both = [(len(texts[a]), len(texts[b])) for a, b in zip(rows_a, rows_b)]
    assert any(x == 0 and y == 0 for x, y in both) and any(x == 0 < y for x, y in both) and any(y == 0 < x for x, y in both)
    st, texts = dna_fixture()
    assert {bits_of(st.tab, t) % 8 for t in texts[:41]} == {0, 2, 4, 6}
    assert any(bits_of(st.tab, t) % 8 == 0 and (bits_of(st.tab, t) + bits_of(st.tab, b"ACGT")) % 8 == 0 for t in texts[1:41])  # left, and left + literal, end on a byte
    assert all(1 <= len(t) <= 3 for t in texts[41:]) and len(texts) - 41 == 60
    st = ladder_fixture()
    assert sorted(set(int(st.tab[1][s]) for s in stored_text(st, 0))) == list(range(1, 33))


def test_the_edge_fixture_lies_at_the_threshold_the_block_and_the_tiles():
    st, at = edge_fixture()
    lane = lane_bytes()
    size = lambda name: int(st.body_index[at[name] + 1] - st.body_index[at[name]])  # noqa: E731
    assert [size(n) for n in ("lane-1", "lane", "lane+1", "lane+2")] == [lane - 1, lane, lane + 1, lane + 2]
    assert [left_reach(st, at[n]) <= lane for n in ("lane-1", "lane", "lane+1", "lane+2", "lane+1m")] == [True, True, False, False, False]
    assert size("block+") > BLOCK and size("block+m") > BLOCK and size("tiles") > 2 * C + 16
    for name in ("mid", "lane+1m", "block+m"):  # a left run of 7 bits mod 8: every byte of what follows straddles two destination bytes
        assert bits_of(st.tab, stored_text(st, at[name])) % 8 == 7
    assert bits_of(st.tab, b"\x01\x02") % 8 == 7 and bits_of(st.tab, b"\x01") == 7  # ... and a literal that brings it to 6, or back to a byte


def test_the_empty_limit_and_pad_fixtures():
    st = empties_fixture()
    sizes, lengths = np.diff(st.body_index.astype(np.int64)), np.diff(st.text_index.astype(np.int64))
    assert (sizes[0], lengths[0]) == (0, 0) and (sizes[3], lengths[3]) == (0, 9) and sizes[1] > 0 and sizes[2] > 0 and lengths[4] == 1
    assert stored_text(st, 3) == b"" and want_concat(st, st, [3, 1], [1, 3], b"").texts == [stored_text(st, 1)] * 2
    rows = empty_run_rows(3000)
    assert rows.size > 2 * SCAN_TILE and sorted(set(rows.tolist())) == [0, 1, 2]
    st, small = limit_fixture()
    lengths = np.diff(st.text_index.astype(np.int64))
    assert small == N.lib().et_batch_small_max() and 10 + 2 + lengths[1] == small and 10 + 2 + lengths[2] == small + 1 and lengths[3] == small
    assert all(left_reach(st, r) > lane_bytes() for r in (1, 2, 3))  # walked by workgroups: the limit is met behind their walk
    want = want_concat(st, st, [0, 0, 0, 3, 1, 2], [1, 2, 0, 3, 0, 0], b"AC")
    assert want.status.tolist() == [OK, UNSUPPORTED, OK, UNSUPPORTED, OK, UNSUPPORTED] and want.text_index[1] == small
    own, texts = dna_fixture()
    st = right_pad_fixture()
    changed = [r for r in range(st.n) if len(texts[r]) % 4]
    assert changed and all(st.bodies[int(st.body_index[r + 1]) - 1] != own.bodies[int(own.body_index[r + 1]) - 1] for r in changed)
    assert all(stored_text(st, r) == texts[r] for r in range(st.n))
    st, _ = set_pad_fixture()
    assert not np.array_equal(st.bodies, main_fixture()[0].bodies)


# --- the call's row of the retained-state table ---------------------------------------------------------------------------------------------


def test_the_concat_call_has_a_row_that_keeps_both_states():
    from tests import retained as R
    from tests import retained_concat as S

    assert R.NAMES.count("concat") == 1 and R.row("concat") is S.ROW and [r.name for r in R.ROWS] == R.NAMES
    row = R.row("concat")
    assert NAME in row.calls and NAME in N.SIGNATURES and (row.hist, row.held, row.names, row.encodes) == (R.KEEPS, R.KEEPS, None, None)
    assert "concat" not in R.DROPS_HISTOGRAM | R.DROPS_RANGE
    assert [R.RECORDS[a] + b" or " + R.RECORDS[b] for a, b in ((0, 1), (3, 0), (1, 3))] == [b"to be or or not", b" or to be", b"or not or "]
