"""et_recode_packed_device's C ABI as far as it can be checked without a GPU: declared, bound, exported, the argument check that comes
before anything touches a device -- every call-level ET_ERR_ARG, with a null ctx, *res untouched --, the Python layer's names and maps,
and the fixtures of tests/test_gpu_recode.py: the rule the kernels implement, stated here over strings of bits (the codewords of the
stored text as tests/bitwalk.py finds them under table IN; for each symbol the codeword of map[s] under table OUT, or nothing; packed
from bit 7 of a byte and padded with zeros), gives on them what the oracle's encode of Python's translate of the oracle's decode gives,
and they reach the cases the GPU tests take them for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from entreepy_amd import _native as N
from tests.test_gpu_concat import dna_fixture, edge_fixture, empties_fixture
from tests.test_gpu_concat import lane_bytes as concat_lane_bytes
from tests.test_gpu_recode import (ARG, DROP, IDENTITY, LOWER, OK, PHASE_MAP, ROUND_BITS, TAB_NO_A, TAB_NO_T, UNSUPPORTED, UPPER, a_map, behind_fixture, contraction_fixture,
                                   drop_fixture, expansion_fixture, ladder_back_fixture, lane_bytes, length_fixture, main_tables, phase_fixture, reach, retabled, table_reddal,
                                   translate, want_recode)
from tests.test_gpu_shared import _cb
from tests.test_gpu_slice import BLOCK_BITS, LANE_BITS, bit_at, cut_fixture, ladder_fixture, main_fixture, pad_fixture, set_pad_fixture, stored_text
from tests.test_gpu_take import SCAN_TILE
from tests.test_shared_host import is_complete, table_255, table_2bit, table_ladder
from tests.test_slice_host import _walked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "et_recode_packed_device"


def test_recode_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in (NAME, "et_recode_lane_bytes"):
        assert name in declared and name in N.SIGNATURES and name in exported, name
    args = re.sub(r"/\*.*?\*/", "", re.search(r"int et_recode_packed_device\(([^;]*)\);", header).group(1))
    assert len(N.SIGNATURES[NAME][1]) == len(args.split(",")) == 17 and args.count("et_codebook") == 2 and "int16_t" in args and "et_take_result" in args
    assert re.search(r"#define ET_RECODE_DROP \(-1\)", header) and N.ET_RECODE_DROP == -1
    assert N.lib().et_recode_lane_bytes() == N.lib().et_search_lane_bytes() > 0 and lane_bytes() == concat_lane_bytes()  # (the concat's edge fixture serves)


def test_the_python_layer_exposes_the_call_the_list_helper_and_the_maps():
    import entreepy_amd as E

    assert callable(E.Context.recode_packed_device) and callable(E.Context.recode_packed) and callable(E.byte_map)
    assert E.RECODE_DROP == N.ET_RECODE_DROP == DROP
    for m in (E.ASCII_UPPER, E.ASCII_LOWER, E.byte_map()):
        assert isinstance(m, np.ndarray) and m.dtype == np.int16 and m.shape == (256,)


def test_the_maps_are_pythons_translate_upper_and_lower_on_all_256_bytes():
    import entreepy_amd as E

    every = bytes(range(256))
    as_bytes = lambda m: bytes(int(x) for x in m if x != DROP)  # noqa: E731  (in order: what `every` becomes)
    assert as_bytes(E.ASCII_UPPER) == every.upper() and as_bytes(E.ASCII_LOWER) == every.lower() and as_bytes(E.byte_map()) == every
    assert not (E.ASCII_UPPER == DROP).any() and not (E.ASCII_LOWER == DROP).any()
    assert np.array_equal(E.ASCII_UPPER, UPPER) and np.array_equal(E.ASCII_LOWER, LOWER)
    for frm, to, delete in ((b"abc", b"xyz", b""), (b"", b"", b"\x00\xff q"), (b"a\x00\xfe", b"\xffbb", b"ez\n"), (every, every[::-1], b"aeiou"), (b"q", b"q", b"q")):
        m = E.byte_map(frm, to, delete)
        assert m.dtype == np.int16 and translate(every, m) == every.translate(bytes.maketrans(frm, to), delete)
        assert sorted(np.flatnonzero(m == DROP).tolist()) == sorted(set(delete)) and np.array_equal(m, a_map(frm, to, delete))
    with pytest.raises(ValueError):
        E.byte_map(b"ab", b"c")


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    ORDER = ["ctx", "cb_in", "cb_out", "map", "d_bodies", "body_bytes", "d_body_index", "d_text_index", "n_records", "d_rows", "n_rows", "d_out", "cap", "d_out_body_index",
             "d_out_text_index", "d_status", "res"]

    def __init__(self):
        self.res = N.TakeResult(out_bytes=77, text_bytes=78, n_failed=79, first_failed=80, first_status=81)
        self.cb = N.Codebook()
        self.map = IDENTITY.copy()
        self.buf = (ctypes.c_uint64 * 64)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, cb_in=ctypes.addressof(self.cb), cb_out=ctypes.addressof(self.cb), map=self.map.ctypes.data, d_bodies=p, body_bytes=16, d_body_index=p + 64,
                      d_text_index=p + 80, n_records=1, d_rows=p + 96, n_rows=1, d_out=p + 128, cap=16, d_out_body_index=p + 160, d_out_text_index=p + 176, d_status=None,
                      res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        args = [v[k] for k in self.ORDER]
        for i in (1, 2):
            args[i] = ctypes.cast(args[i], ctypes.POINTER(N.Codebook)) if args[i] else None
        args[-1] = ctypes.cast(v["res"], ctypes.POINTER(N.TakeResult)) if v["res"] else None
        rc = N.lib().et_recode_packed_device(*args)
        r = self.res
        assert (r.out_bytes, r.text_bytes, r.n_failed, r.first_failed, r.first_status) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


def test_null_context_is_an_argument_error():
    assert _Args().call() == ARG and _Args().call(map=None) == ARG and _Args().call(d_rows=None) == ARG  # (well-formed; the null ctx alone)
    assert N.lib().et_recode_packed_device(None, None, None, None, None, 0, None, None, 0, None, 0, None, 0, None, None, None, None) == ARG


@pytest.mark.parametrize("name", ["cb_in", "cb_out", "res", "d_bodies", "d_body_index", "d_text_index", "d_out_body_index", "d_out_text_index"])
def test_every_null_pointer_is_an_argument_error_before_a_device_is_touched(name):
    assert _Args().call(**{name: None}) == ARG


@pytest.mark.parametrize("name", ["d_body_index", "d_text_index", "d_out_body_index", "d_out_text_index"])
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
    assert _Args().call(**{name: 0x80000000}) == ARG and _Args().call(**{name: 1 << 40}) == ARG


def test_without_rows_the_row_count_is_the_record_count():
    assert _Args().call(d_rows=None, n_rows=2) == ARG and _Args().call(d_rows=None, n_rows=0) == ARG


@pytest.mark.parametrize("where", ["same", "out_begins_inside", "out_ends_inside", "out_around", "last_byte", "first_byte"])
def test_an_output_that_overlaps_the_bodies_is_an_argument_error(where):
    a = _Args()
    b = a.v["d_bodies"]  # the bodies are [b, b + 16)
    d_out, cap = {"same": (b, 16), "out_begins_inside": (b + 8, 16), "out_ends_inside": (b - 8, 16), "out_around": (b - 8, 48), "last_byte": (b + 15, 4), "first_byte": (b - 3, 4)}[where]
    assert a.call(d_out=d_out, cap=cap) == ARG


@pytest.mark.parametrize("value", [-2, 256, 32767, -32768, 1000])
@pytest.mark.parametrize("at", [0, 97, 255])
def test_a_map_entry_that_is_neither_a_byte_nor_drop_is_an_argument_error(value, at):
    a = _Args()
    a.map[at] = value
    assert a.call() == ARG
    a.map[at] = DROP  # (well-formed again: the null ctx alone)
    assert a.call() == ARG


# --- the rule the kernels implement, in pure Python ---------------------------------------------------------------------------------------


def code_bits(tab, s):
    """The codeword of byte s under `tab` as an array of bits, the first at index 0; None: no code."""
    n = int(tab[1][s])
    return np.array([(int(tab[0][s]) >> (n - 1 - i)) & 1 for i in range(n)], np.uint8) if n else None


def rule(st, tab_out, r, bmap):
    """-> (status, the new body's bytes, its length): the symbols of the stored text as the walk under table IN finds them -- the
    codewords that end inside the body, at most `length` of them --, for each one the codeword of map[s] under table OUT or nothing,
    end to end from bit 7 of a byte, the last byte padded with zeros.  A kept symbol without a code fails the row."""
    _, _, symbols = _walked(st, r)
    m = IDENTITY if bmap is None else np.asarray(bmap)
    kept = [int(m[s]) for s in symbols if m[s] != DROP]
    codes = {s: code_bits(tab_out, s) for s in set(kept)}
    if any(c is None for c in codes.values()):
        return UNSUPPORTED, b"", 0
    bits = np.concatenate([codes[s] for s in kept]) if kept else np.zeros(0, np.uint8)
    return OK, np.packbits(bits).tobytes(), len(kept)


def check_rule(st, tab_out, bmap=None, rows=None):
    """The rule against want_recode(): the oracle's encode under table OUT of Python's translate of the oracle's decode, byte for byte."""
    want = want_recode(st, tab_out, rows, bmap)
    for k, r in enumerate(range(st.n) if rows is None else rows):
        status, body, length = rule(st, tab_out, int(r), bmap)
        b0, b1 = int(want.body_index[k]), int(want.body_index[k + 1])
        assert (status, body, length) == (int(want.status[k]), want.data[b0:b1].tobytes(), int(want.text_index[k + 1] - want.text_index[k])), (k, int(r))
    return want


def test_the_bit_rule_gives_the_oracles_encode_of_pythons_translate():
    st, _ = main_fixture()
    T = main_tables()
    assert all(is_complete(*t) == OK for t in T.values()) and not np.array_equal(T["T1"][1], T["T2"][1])
    for tab, bmap in ((T["T2"], None), (T["TU"], UPPER), (T["T1"], LOWER), (T["T1"], None), (T["T2"], np.full(256, DROP, np.int16))):
        check_rule(st, tab, bmap, rows=list(range(12)) + [13])
    check_rule(retabled(st, T["T2"]), T["T1"], rows=range(12))
    st, _ = phase_fixture()
    check_rule(st, table_255(), PHASE_MAP)
    st, _ = dna_fixture()
    for bmap in (None, a_map(b"ACGT", b"TGCA"), a_map(delete=b"G")):
        check_rule(st, table_2bit(), bmap)
    assert is_complete(*table_reddal()) == OK and sorted(table_reddal()[1][100:133].tolist()) == sorted(table_ladder()[1][100:133].tolist())
    check_rule(ladder_fixture(), table_reddal())
    check_rule(ladder_back_fixture(), table_ladder())
    st, at = edge_fixture()
    check_rule(st, table_255(), a_map(delete=b"\x07"), rows=[at[n] for n in ("few", "mid", "lane-1", "lane", "lane+1", "lane+1m")])


def test_the_bit_rule_on_hand_made_bodies():
    T = main_tables()
    want = check_rule(set_pad_fixture()[0], T["T1"])  # set pad bits: the identity gives the encoder's own bodies
    assert np.array_equal(want.data, main_fixture()[0].bodies)
    check_rule(cut_fixture(), T["T2"])
    check_rule(empties_fixture(), T["T2"])
    check_rule(length_fixture()[0], T["T2"])
    for tab in (TAB_NO_A, TAB_NO_T, table_2bit()):
        assert is_complete(*tab) == OK
        check_rule(pad_fixture()[0], tab)
        check_rule(behind_fixture(), tab)
    st, _ = drop_fixture()
    for tab in (table_2bit(), TAB_NO_A):
        check_rule(st, tab, a_map(delete=b"A"))


# --- the fixtures are what the GPU tests take them for --------------------------------------------------------------------------------------


def bits_mod_8(tab, text):
    return int(tab[1][np.frombuffer(text, np.uint8)].astype(np.int64).sum()) % 8


def test_the_phase_fixture_reaches_every_pair_of_bit_counts_on_both_paths():
    st, at = phase_fixture()
    lane = lane_bytes()
    seen = {False: set(), True: set()}
    for (a, c, long), r in at.items():
        assert (reach(st, r) > lane) == long
        t = stored_text(st, r)
        seen[long].add((bits_mod_8(st.tab, t), bits_mod_8(table_255(), translate(t, PHASE_MAP))))
    assert all(pairs == {(i, o) for i in range(8) for o in range(8)} for pairs in seen.values())


def test_the_uncoded_fixtures_hold_their_codeword_where_they_say():
    st, texts = pad_fixture()
    for r, (pad_reads, tab) in enumerate([(ord("A"), TAB_NO_A)] * 6 + [(ord("T"), TAB_NO_T)] * 6):
        bits, bounds, symbols = _walked(st, r)  # (the walk ends with the length: what follows is pad)
        pad = bits[int(bounds[-1]) :]
        assert 0 < pad.size < 8 and pad.size % 2 == 0 and bytes([pad_reads]) not in texts[r] and int(tab[1][pad_reads]) == 0
        assert (pad == (pad_reads == ord("T"))).all()  # only in the pad: zero bits read as A, set bits as T
    short = lambda r: reach(st, r) <= lane_bytes()  # noqa: E731
    assert [short(r) for r in range(12)] == [True] * 3 + [False] * 3 + [True] * 3 + [False] * 3
    assert all(b"A" in texts[r] for r in (9, 10, 11)) and all(b"T" in texts[r] for r in (3, 4, 5))  # ... and inside the stored text, the workgroup's
    st = behind_fixture()
    for r in range(4):
        body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes()
        length = int(st.text_index[r + 1] - st.text_index[r])
        from tests.test_gpu_shared import want_decode

        whole = want_decode(st.tab, body, 4 * len(body))[1]
        assert b"A" in whole[length:] and (b"A" in whole[:length]) == (r >= 2) and stored_text(st, r) == whole[:length]  # only behind the length; inside it too
    assert [reach(st, r) <= lane_bytes() for r in range(4)] == [True, False, True, False]
    want = want_recode(st, TAB_NO_A, None)
    assert want.status.tolist() == [OK, OK, UNSUPPORTED, UNSUPPORTED]


def test_the_expansion_and_contraction_fixtures_exceed_the_rounds_and_the_blocks():
    st = expansion_fixture()
    assert is_complete(*table_reddal()) == OK and int(table_ladder()[1][100]) == 1 and int(table_reddal()[1][100]) == 32
    body0 = int(st.body_index[1] - st.body_index[0])
    out0 = 32 * int(st.text_index[1])
    assert BLOCK_BITS // 8 < body0 <= BLOCK_BITS // 8 + 1 and out0 >= 16 * ROUND_BITS  # one input block, and 3 bits: sixteen flush rounds of it
    assert int(st.text_index[2] - st.text_index[1]) == N.lib().et_batch_small_max() and 4 * int(st.text_index[2] - st.text_index[1]) == 4 * N.lib().et_batch_small_max()
    assert sorted(set(int(st.tab[1][s]) for s in stored_text(st, 2))) == list(range(1, 33))
    st = contraction_fixture()
    in0, out_bits = int(st.body_index[1]), int(st.text_index[1])
    assert in0 * 8 >= 32 * BLOCK_BITS and out_bits < ROUND_BITS  # 32 input blocks feed less than one round of output
    assert all(reach(s, 0) > lane_bytes() for s in (expansion_fixture(), st))


def test_the_length_fixture_ends_where_it_says():
    st, at = length_fixture()
    own, texts = main_fixture()
    starts = bit_at(own, 13, 0) + np.concatenate(([0], np.cumsum(own.tab[1][np.frombuffer(texts[13], np.uint8)].astype(np.int64))))
    length = lambda name: int(st.text_index[at[name] + 1] - st.text_index[at[name]])  # noqa: E731
    lane_of = lambda sym: int(starts[sym]) // LANE_BITS  # noqa: E731  (the lane in which symbol `sym` begins)
    # symbol number `length` -- the first that is no symbol -- is a lane's first codeword, and its last
    assert lane_of(length("lane_first")) == lane_of(length("lane_first") - 1) + 1 and lane_of(length("lane_last")) + 1 == lane_of(length("lane_last") + 1)
    assert [int(starts[length(n)]) // BLOCK_BITS for n in ("block0", "block1", "block2")] == [0, 1, 2]
    assert [int(starts[length(n)]) // BLOCK_BITS for n in ("block1_first-1", "block1_first", "block2_first-1", "block2_first")] == [0, 1, 1, 2]
    inner = set(int(x) for x in starts[1:-1])
    other = bit_at(own, 12, 0) + np.cumsum(own.tab[1][np.frombuffer(texts[12], np.uint8)].astype(np.int64))
    assert BLOCK_BITS not in set(int(x) for x in other) and int(other[-1]) > BLOCK_BITS  # a codeword straddles the block edge: the main fixture's record 12 (and the edge fixture's, below)
    assert sum(1 for k in range(1, int(starts[-1]) // LANE_BITS) if k * LANE_BITS not in inner) > 200  # ... and nearly every lane's
    assert all(reach(st, r) > lane_bytes() for n, r in at.items() if n != "one") and reach(st, at["one"]) <= lane_bytes()
    assert length("beyond") > len(texts[13]) == length("whole")


def test_the_edge_drop_and_row_fixtures():
    st, at = edge_fixture()
    lane = lane_bytes()
    assert [reach(st, at[n]) for n in ("lane-1", "lane", "lane+1", "lane+2")] == [lane - 1, lane, lane + 1, lane + 2]
    r = at["block+m"]  # a 7-bit codeword in front of 8-bit ones: every codeword behind it straddles a byte's edge, the block's among them
    assert stored_text(st, r)[0] == 1 and 1 not in stored_text(st, r)[1:] and (bit_at(st, r, 1) - 7) % 8 == 0 and bit_at(st, r, len(stored_text(st, r))) > BLOCK_BITS + 8
    st, texts = drop_fixture()
    kept = [t.replace(b"A", b"") for t in texts]
    assert any(t[:1] == b"A" != t[-1:] for t in texts) and any(t[-1:] == b"A" != t[:1] for t in texts)  # the first symbol dropped; the last
    assert sum(1 for t, k in zip(texts, kept) if k and len(k) % 4 == 0 and len(t) % 4) >= 4  # drops that make the output whole bytes
    assert sum(1 for k in kept if not k) == 4 and any(reach(st, r) > lane for r in range(st.n) if not kept[r])  # nothing kept, on both paths
    st = empties_fixture()
    sizes, lengths = np.diff(st.body_index.astype(np.int64)), np.diff(st.text_index.astype(np.int64))
    assert (sizes[0], lengths[0]) == (0, 0) and (sizes[3], lengths[3]) == (0, 9)
    assert 5002 > SCAN_TILE + 1
    dna, dna_texts = dna_fixture()
    assert all(1 <= len(t) <= 3 for t in dna_texts[41:]) and len(dna_texts) - 41 == 60


# --- the call's row of the retained-state table ---------------------------------------------------------------------------------------------


def test_the_recode_call_has_a_row_that_keeps_both_states():
    from tests import retained as R
    from tests import retained_recode as S

    assert R.NAMES.count("recode") == 1 and R.row("recode") is S.ROW and [r.name for r in R.ROWS] == R.NAMES
    row = R.row("recode")
    assert NAME in row.calls and NAME in N.SIGNATURES and (row.hist, row.held, row.names, row.encodes) == (R.KEEPS, R.KEEPS, None, None)
    assert "recode" not in R.DROPS_HISTOGRAM | R.DROPS_RANGE
    assert [R.RECORDS[r].translate(bytes.maketrans(b"ot", b"to"), b" ") for r in (0, 3, 1)] == [b"otbe", b"", b"trnto"]
