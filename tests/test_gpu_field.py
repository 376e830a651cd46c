"""GPU: et_field_packed_device -- fields [field, field + n_fields) of a selection's records, split at a delimiter byte, as a new packed
store, found and copied on the compressed bytes -- against the oracle: a row's status is judged from its record's own two pairs of
offsets, its stored text is want_decode's, the field is Python's (delim.join(text.split(delim)[field : field + n_fields]), absent when
field >= len(parts)), and the expected bytes are the oracle's shared-table encode of it (want_field()); never the bit rule the kernels
implement.  d_out lies between sentinel bytes as in tests/test_gpu_take.py, whose check_take() compares bytes, both offset arrays,
the status bytes and the report; check_field() adds d_pos.

The stores and the rows are made by the *_fixture functions below, without a GPU: tests/test_field_host.py checks on the same fixtures
that the bit rule gives what the oracle gives, and that they reach the cases named here."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus
from tests import retained_field  # noqa: F401  (the call's row joins the table of tests/retained.py)
from tests.test_gpu_batch import SENTINEL, _small_max
from tests.test_gpu_gather import dev_rows, make_store, upload
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_gpu_shared import _cb, want_encode
from tests.test_gpu_slice import (BLOCK_BITS, LANE_BITS, cut_fixture, dev_u32, ladder_fixture, main_fixture, pad_fixture, per_row, run_slice, set_pad_fixture, stored_text,
                                  want_slice)
from tests.test_gpu_take import C, LEAD, SCAN_TILE, SELECTIONS, _guards_intact, check_take, failures_store, selection
from tests.test_shared_host import oracle_table, table_255, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
TO_END, ABSENT = 0xFFFFFFFF, 0xFFFFFFFF  # ET_FIELD_TO_END, ET_FIELD_ABSENT
SPACE, BAR, COMMA = ord(" "), ord("|"), ord(",")


def lane_bytes():
    """A body (reach()) up to this many bytes is walked by one lane, a longer one by a workgroup."""
    from entreepy_amd import _native as N

    return int(N.lib().et_field_lane_bytes())


def reach(st, r):
    """The bytes of record r's body that the walks look at: 4 bytes per symbol of the length, and 8 (csrc/et_batch.h clip_body)."""
    nb, length = int(st.body_index[r + 1] - st.body_index[r]), int(st.text_index[r + 1] - st.text_index[r])
    return min(nb, 4 * length + 8)


# --- the expected store: the oracle's texts, Python's split and join, the oracle's encode -----------------------------------------------


def py_field(text, field, n_fields, delim):
    """-> (the row's text, d_pos): SQL's SPLIT_PART over Python's split, n_fields consecutive fields with their delimiters."""
    d = bytes([delim])
    parts = text.split(d)
    if field >= len(parts):
        return b"", ABSENT
    return d.join(parts[field : field + n_fields]), sum(len(p) + 1 for p in parts[:field])  # (Python's ints do not wrap)


def want_field(st, rows, field, n_fields, delim):
    """-> what tests/test_gpu_slice.py's want_slice() returns, for the fields, and .pos: status by the take's rule, then the oracle's
    encode of Python's field."""
    small, body_bytes = _small_max(), st.bodies.size
    rows = np.arange(st.n) if rows is None else np.asarray(rows, dtype=np.int64)
    fields, counts = per_row(field, rows.size), per_row(n_fields, rows.size)
    if isinstance(delim, bytes):
        (delim,) = delim
    memo = st.__dict__.setdefault("fielded", {})
    status, nb, ln, pieces, texts = np.full(rows.size, ARG, np.uint8), np.zeros(rows.size, np.uint64), np.zeros(rows.size, np.uint64), [], []
    pos = np.full(rows.size, ABSENT, np.uint32)
    for k, r in enumerate(int(r) for r in rows):
        texts.append(b"")
        if r >= st.n:
            continue
        b0, b1, t0, t1 = (int(x) for x in (st.body_index[r], st.body_index[r + 1], st.text_index[r], st.text_index[r + 1]))
        if not (b0 <= b1 <= body_bytes and t0 <= t1):
            continue
        if t1 - t0 > small or b1 - b0 > 4 * small:
            status[k] = UNSUPPORTED
            continue
        key = (r, fields[k], counts[k], delim)
        if key not in memo:
            s, p = py_field(stored_text(st, r), fields[k], counts[k], delim)
            rc, body = want_encode(st.tab, s)
            assert rc == OK
            memo[key] = (s, np.frombuffer(body, np.uint8), p)
        s, body, pos[k] = memo[key]
        status[k], nb[k], ln[k], texts[k] = OK, body.size, len(s), s
        pieces.append(body)
    data = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    return SimpleNamespace(status=status, body_index=_index_of(nb), text_index=_index_of(ln), data=data, total=int(nb.sum()), text_total=int(ln.sum()), texts=texts, pos=pos)


def n_parts(st, r, delim):
    return stored_text(st, r).count(bytes([delim])) + 1


# --- the fixtures ----------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_slice.py's main fixture (44 records of text, 0 .. 40 000 bytes, bodies on both sides of the lane's share and up to
# three 8 KiB blocks) with the space as the delimiter is the store of most tests below.


@functools.lru_cache(maxsize=None)
def phase_rows():
    """900 (row, field, n_fields) over the main fixture with the space as the delimiter: a third anywhere, a third on the records a
    lane walks, a third far into the two long records (the workgroup's) -> three arrays."""
    st, texts = main_fixture()
    rng = np.random.default_rng(0xF1E1D001)
    short = [r for r in range(st.n) if 0 < reach(st, r) <= lane_bytes()]
    rows, field, count = [], [], []
    for i in range(900):
        r = (int(rng.integers(0, st.n)), short[int(rng.integers(0, len(short)))], int(rng.integers(12, 14)))[i % 3]
        n = n_parts(st, r, SPACE)
        rows.append(r), field.append(int(rng.integers(0, n + 1))), count.append(int(rng.integers(0, 4)) if i % 2 else int(rng.integers(0, 60)))
    return np.array(rows), np.array(field), np.array(count)


def _starts(tab, text, first_bit):
    """The bit at which every symbol of `text` begins in a body that begins at first_bit, and one entry more: where the last one ends."""
    return first_bit + np.concatenate(([0], np.cumsum(tab[1][np.frombuffer(text, np.uint8)].astype(np.int64))))


@functools.lru_cache(maxsize=None)
def edge_fixture():
    """Records under the table of text with bars in it, the bar the delimiter, hand-placed at the workgroup path's edges ->
    (store, [texts], {case: record}):
      lane_edge   text + "||" + text + "|" + text: the first bar is the LAST codeword of a lane's 256 bits, the second the FIRST of the next
      block_edge  the same at bit 65 536: the first bar ends block 0, the second is the first codeword of block 1's first lane
      three_blocks  "ab|" + a field that begins in block 0 and ends in block 2 + "|cd|ef"
      bars_only   5 000 bars: nothing but empty fields
      ends        "|" + text + "|": a delimiter at symbol 0 and at the last symbol, on a lane's record (ends_short) and a workgroup's
      none        a record without a bar, short and long
    Every body's first bit follows from the bodies in front of it, so the records are made in order."""
    pool = corpus.text_like(60000, 0xF1E1D010)
    assert BAR not in pool
    tab = oracle_table(np.concatenate((pool, np.full(600, BAR, np.uint8))))
    bar_bits = int(tab[1][BAR])
    bits = np.concatenate(([0], np.cumsum(tab[1][pool].astype(np.int64))))
    texts, case, at = [], {}, 0  # at: the byte at which the next body begins

    def add(name, text):
        nonlocal at
        case[name] = len(texts)
        texts.append(text)
        at += len(want_encode(tab, text)[1])

    def ending_at(target):
        """pool[j:i] whose bits, in a body that begins at byte `at`, end bar_bits in front of bit `target` of the aligned word the body begins in."""
        need = target - bar_bits - (at % 4) * 8
        for j in range(2000):
            i = int(np.searchsorted(bits, bits[j] + need))
            if i < bits.size and bits[i] - bits[j] == need:
                return pool[j:i].tobytes()
        raise AssertionError("no run of the pool has that many bits")

    add("ends_short", b"|" + pool[:60].tobytes() + b"|")
    add("lane_edge", ending_at(7 * LANE_BITS) + b"||" + pool[100:3100].tobytes() + b"|" + pool[5000:5400].tobytes())
    add("block_edge", ending_at(BLOCK_BITS) + b"||" + pool[200:3200].tobytes() + b"|" + pool[6000:6300].tobytes())
    add("three_blocks", b"ab|" + pool[1000:36000].tobytes() + b"|cd|ef")
    add("bars_only", b"|" * 5000)
    add("ends_long", b"|" + pool[2000:9000].tobytes() + b"|")
    add("none_short", pool[300:340].tobytes())
    add("none_long", pool[400:4400].tobytes())
    return make_store(tab, texts), texts, case


@functools.lru_cache(maxsize=None)
def dense_fixture():
    """Nine bytes of ten are commas, and the comma's codeword has ONE bit: a lane of the workgroup path holds about 200 delimiters, a
    block about 50 000, and the delimiter prefix carries real counts across lanes and blocks -> (store, [texts])."""
    rng = np.random.default_rng(0xF1E1D020)
    texts = [np.where(rng.random(n) < 0.9, COMMA, rng.choice(np.frombuffer(b"abcd", np.uint8), size=n)).astype(np.uint8).tobytes() for n in (40, 300, 3000, 9000, 130000)]
    st = make_store(oracle_table(np.frombuffer(b"".join(texts), np.uint8)), texts)
    return st, texts


@functools.lru_cache(maxsize=None)
def behind_length_fixture():
    """The main fixture's records 6 .. 13 with their bodies whole and their LENGTHS cut to 5/8: the codewords at and behind the length
    end inside the body, decode (some of them) as the delimiter, and are no part of the stored text -> (store, [the stored texts])."""
    st, texts = main_fixture()
    keep = [texts[r][: 5 * len(texts[r]) // 8] for r in range(6, 14)]
    bodies = [st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes() for r in range(6, 14)]
    return make_store(st.tab, keep, bodies), keep


@functools.lru_cache(maxsize=None)
def small_fields_fixture():
    """Under the ladder table (codewords of 1 .. 32 bits), the 1-bit symbol 100 the delimiter -> (store, rows, field, n_fields): one record
    of single-symbol fields of 2 .. 32 bits, pairs of 33 bits and runs of empty fields -- two empty fields with their delimiter are ONE
    bit --, and 4 000 rows of it that are 0 .. 33 bits long."""
    unit = b"".join(bytes([k, 100]) for k in range(101, 133)) + bytes([100, 100, 115, 116, 100])  # 32 fields of a symbol, three empty ones, 16 + 17 bits
    st = make_store(table_ladder(), [unit * 30])
    rng = np.random.default_rng(0xF1E1D030)
    field = rng.integers(0, 35 * 30, size=4000)  # (35 delimiters, so 35 fields, to a unit)
    count = np.where((field % 35 >= 32) & (field % 35 <= 33), rng.integers(0, 3, size=4000), rng.integers(0, 2, size=4000))  # (two fields: the empty ones alone)
    return st, np.zeros(4000, np.int64), field, count


# --- one call and its check ------------------------------------------------------------------------------------------------------------


def run_field(ctx, st, dev, rows, field, n_fields, delim, cap, sizes_only=False, shift=0, tile_off=None, no_pos=False):
    """One call, every output full of sentinels first (tests/test_gpu_slice.py's run_slice).  rows=None: d_rows == NULL."""
    import torch

    d_bodies, d_body_index, d_text_index = dev
    n = st.n if rows is None else len(rows)
    r = SimpleNamespace(cap=cap, sizes_only=sizes_only)
    r.d_raw = torch.full((3 * C + LEAD + 16 + cap + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert r.d_raw.data_ptr() % 16 == 0
    r.at = LEAD + shift if tile_off is None else (-r.d_raw.data_ptr()) % C + C + tile_off
    r.d_out = r.d_raw[r.at : r.at + max(cap, 1)]
    r.d_body_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_text_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    r.d_pos = torch.full((n + 2,), 0x5E5E5E5E, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.res = ctx.field_packed_device(st.cb, d_bodies, d_body_index, d_text_index, None if rows is None else dev_rows(rows), dev_u32(field), dev_u32(n_fields), delim,
                                    None if sizes_only else r.d_out, r.d_body_index, r.d_text_index, pos=None if no_pos else r.d_pos[1 : n + 1], status=r.d_status)
    torch.cuda.synchronize()
    r.host = r.d_raw.cpu().numpy()
    r.body_index, r.text_index = r.d_body_index.cpu().numpy().view(np.uint64), r.d_text_index.cpu().numpy().view(np.uint64)
    r.status = r.d_status.cpu().numpy()
    r.pos = r.d_pos.cpu().numpy().view(np.uint32)
    return r


def check_field(r, want, call_status=OK, no_pos=False):
    check_take(r, want, call_status)
    assert r.pos[0] == r.pos[-1] == 0x5E5E5E5E, "a word beside d_pos was written"
    if no_pos:
        assert bool((r.pos == 0x5E5E5E5E).all())
    else:
        bad = np.flatnonzero(r.pos[1:-1] != want.pos)
        assert bad.size == 0, f"d_pos differs from Python's, first at row {int(bad[0])}: {int(r.pos[1 + bad[0]])} for {int(want.pos[bad[0]])}"
    return r


def field_(ctx, st, rows, field, n_fields, delim, dev=None, **kw):
    """Run with cap = the need exactly, and check."""
    want = want_field(st, rows, field, n_fields, delim)
    r = check_field(run_field(ctx, st, dev or upload(st), rows, field, n_fields, delim, want.total, **kw), want, no_pos=kw.get("no_pos", False))
    r.want = want
    return r


# --- 1. field arguments and where the delimiters lie -------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_fields", [0, 1, 2, TO_END])
def test_fields_at_the_edges_of_the_record(ctx, n_fields):
    st, texts = main_fixture()
    dev = upload(st)
    last = np.array([t.count(b" ") for t in texts], dtype=np.int64)  # the last field's number
    fields = {"0": 0, "1": 1, "last - 1": np.maximum(last - 1, 0), "last": last, "last + 1": last + 1, "0xfffffffe": 0xFFFFFFFE, "0xffffffff": 0xFFFFFFFF}
    for name, field in fields.items():
        r = field_(ctx, st, None, field, n_fields, SPACE, dev=dev)
        assert r.res.n_failed == 0
        if np.isscalar(field):  # the same as device arrays
            as_arrays = field_(ctx, st, None, np.full(st.n, field), np.full(st.n, n_fields), SPACE, dev=dev)
            assert as_arrays.res == r.res
        if name in ("0", "last"):
            assert bool((r.want.pos != ABSENT).all())
        if name in ("last + 1", "0xfffffffe", "0xffffffff"):
            assert bool((r.want.pos == ABSENT).all()) and r.res.out_bytes == 0
    if n_fields == TO_END:
        whole = field_(ctx, st, None, 0, TO_END, SPACE, dev=dev)  # the identity: the store itself
        assert np.array_equal(whole.body_index, st.body_index) and np.array_equal(whole.text_index, st.text_index) and np.array_equal(whole.want.data, st.bodies)


def test_field_plus_n_fields_does_not_wrap(ctx):
    st, texts = main_fixture()
    dev = upload(st)
    for field, n in ((5, 0xFFFFFFFA), (5, 0xFFFFFFFB), (1, 0xFFFFFFFF), (2, 0xFFFFFFFE), (0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFE, 3)):
        assert field + n >= 0xFFFFFFFF
        r = field_(ctx, st, None, field, n, SPACE, dev=dev)
        assert r.want.texts == [b" ".join(t.split(b" ")[field:]) for t in texts]
        field_(ctx, st, None, np.full(st.n, field), np.full(st.n, n), SPACE, dev=dev)


def test_delimiters_first_last_doubled_and_absent(ctx):
    st, texts, case = edge_fixture()
    dev = upload(st)
    for tag in ("ends_short", "ends_long"):
        r = case[tag]
        got = field_(ctx, st, [r] * 6, [0, 1, 2, 3, 0, 1], [1, 1, 1, 1, TO_END, 2], BAR, dev=dev)
        assert got.want.texts[0] == got.want.texts[2] == b"" and got.want.pos.tolist() == [0, 1, len(texts[r]), ABSENT, 0, 1]
    r = case["bars_only"]
    got = field_(ctx, st, [r] * 7, [0, 1, 4999, 5000, 5001, 17, 100], [1, 1, 1, 1, 1, 3, TO_END], BAR, dev=dev)
    assert got.want.texts[:5] == [b""] * 5 and got.want.pos.tolist() == [0, 1, 4999, 5000, ABSENT, 17, 100] and got.want.texts[5:] == [b"||", b"|" * 4900]
    for tag in ("none_short", "none_long"):
        r = case[tag]
        got = field_(ctx, st, [r] * 4, [0, 1, 0, 0], [1, 1, TO_END, 0], BAR, dev=dev)
        assert got.want.texts == [texts[r], b"", texts[r], b""] and got.want.pos.tolist() == [0, ABSENT, 0, 0]


def test_a_delimiter_without_a_code_makes_every_record_one_field(ctx):
    st, texts = main_fixture()
    dev = upload(st)
    assert int(st.tab[1][0xFF]) == 0
    r = field_(ctx, st, None, 0, 1, 0xFF, dev=dev)
    assert r.want.texts == list(texts) and bool((r.want.pos == 0).all())
    r = field_(ctx, st, None, 1, TO_END, 0xFF, dev=dev)
    assert r.res.out_bytes == 0 and bool((r.want.pos == ABSENT).all())


# --- 2. lane and block edges -----------------------------------------------------------------------------------------------------------------


def test_delimiters_at_lane_and_block_edges(ctx):
    st, texts, case = edge_fixture()
    dev = upload(st)
    for tag in ("lane_edge", "block_edge"):
        r = case[tag]
        got = field_(ctx, st, [r] * 8, [0, 1, 2, 3, 4, 0, 1, 1], [1, 1, 1, 1, 1, 2, 2, TO_END], BAR, dev=dev)
        first = texts[r].index(b"|")
        assert got.want.pos.tolist() == [0, first + 1, first + 2, first + 3003, ABSENT, 0, first + 1, first + 1] and got.want.texts[1] == b""
    r = case["three_blocks"]
    got = field_(ctx, st, [r] * 6, [1, 0, 2, 3, 1, 0], [1, 1, 1, 1, 2, TO_END], BAR, dev=dev)
    assert [len(t) for t in got.want.texts] == [35000, 2, 2, 2, 35003, len(texts[r])]


def test_bodies_on_both_sides_of_the_lanes_share(ctx):
    lane = lane_bytes()
    n = (lane - 8) // 4  # symbols of 8 bits: a body of n + d bytes
    rng = np.random.default_rng(0xF1E1D040)
    texts = [np.where(rng.random(m) < 0.1, 9, rng.integers(10, 256, size=m)).astype(np.uint8).tobytes() for m in (lane - 1, lane, lane + 1, lane + 2, n, n + 3)]
    st = make_store(table_255(), texts)
    assert [reach(st, r) <= lane for r in range(6)] == [True, True, False, False, True, True]
    dev = upload(st)
    for field, count in ((0, 1), (3, 2), (np.array([t.count(b"\t") for t in texts]), 1), (1, TO_END)):
        field_(ctx, st, None, field, count, 9, dev=dev)


# --- 3. tables -------------------------------------------------------------------------------------------------------------------------------


def test_a_one_bit_delimiter_two_hundred_to_a_lane(ctx):
    st, texts = dense_fixture()
    dev = upload(st)
    last = np.array([t.count(b",") for t in texts], dtype=np.int64)
    for field, count in ((0, 1), (last, 1), (last + 1, 1), (last // 2, 5), (last - 3, TO_END), (np.minimum(last, [7, 200, 2000, 7000, 100000]), 40), (0, TO_END)):
        field_(ctx, st, None, field, count, COMMA, dev=dev)
    rng = np.random.default_rng(0xF1E1D021)
    rows = rng.integers(0, st.n, size=400)
    field_(ctx, st, rows, [int(rng.integers(0, last[r] + 2)) for r in rows], rng.integers(0, 30, size=400), COMMA, dev=dev)


@pytest.mark.parametrize("delim", [131, 132, 100, 116])
def test_delimiter_codewords_of_32_bits_and_of_one(ctx, delim):
    st = ladder_fixture()
    dev = upload(st)
    for field, count in ((0, 1), (1, 1), (39, 2), (40, 1), (41, 1), (3, TO_END), (7, 0)):
        field_(ctx, st, None, field, count, delim, dev=dev)
    rng = np.random.default_rng(0xF1E1D050 + delim)
    field_(ctx, st, rng.integers(0, st.n, size=300), rng.integers(0, 45, size=300), rng.integers(0, 4, size=300), delim, dev=dev)


@pytest.mark.parametrize("delim", [ord("A"), ord("T"), ord("G"), ord("x")])
def test_the_two_bit_table_and_pad_bits_that_read_as_the_delimiter(ctx, delim):
    st, texts = pad_fixture()  # zero pad bits read as A, the set ones of the hand-made bodies as T; x has no code
    dev = upload(st)
    whole = field_(ctx, st, None, 0, TO_END, delim, dev=dev)
    assert whole.want.texts == list(texts)
    for field, count in ((0, 1), (1, 1), (np.array([t.count(bytes([delim])) for t in texts]), 1), (np.array([t.count(bytes([delim])) + 1 for t in texts]), 1), (2, 3)):
        r = field_(ctx, st, None, field, count, delim, dev=dev)
    r = field_(ctx, st, None, 1, 1, delim, dev=dev)
    without = [k for k, t in enumerate(texts) if bytes([delim]) not in t]  # one field, whatever the pad bits read as
    assert all(r.want.pos[k] == ABSENT for k in without) and (len(without) >= 6 or delim == ord("G"))


# --- 4. what is no part of the stored text, and odd records -----------------------------------------------------------------------------------


def test_codewords_at_and_behind_the_length_are_never_delimiters(ctx):
    st, stored = behind_length_fixture()
    dev = upload(st)
    last = np.array([t.count(b" ") for t in stored], dtype=np.int64)
    for field, count in ((last, 1), (last + 1, 1), (last, TO_END), (0, TO_END), (last - 2, 5), (last + 1, TO_END)):
        r = field_(ctx, st, None, field, count, SPACE, dev=dev)
    assert bool((r.want.pos == ABSENT).all()) and r.res.out_bytes == 0  # field last + 1 exists in the bodies' codewords, not in the stored texts
    assert field_(ctx, st, None, 0, TO_END, SPACE, dev=dev).want.texts == list(stored)


def test_set_pad_bits_of_hand_made_bodies_are_masked_not_copied(ctx):
    st, texts = set_pad_fixture()
    dev = upload(st)
    own, _ = main_fixture()
    last = np.array([t.count(b" ") for t in texts], dtype=np.int64)
    for field, count in ((last, 1), (np.maximum(last - 1, 0), TO_END), (0, 1)):
        field_(ctx, st, None, field, count, SPACE, dev=dev)
    whole = field_(ctx, st, None, 0, TO_END, SPACE, dev=dev)
    assert np.array_equal(whole.want.data, own.bodies) and not np.array_equal(st.bodies, own.bodies)  # the encoder's own bodies: the pad is zero again


def test_cut_bodies_end_the_field_where_the_stored_text_ends(ctx):
    st = cut_fixture()
    dev = upload(st)
    stored = [stored_text(st, r) for r in range(st.n)]
    assert all(len(s) < int(l) for s, l in zip(stored, np.diff(st.text_index)))
    last = np.array([t.count(b" ") for t in stored], dtype=np.int64)
    for field, count in ((last, 1), (last, TO_END), (last + 1, 1), (0, TO_END), (np.maximum(last - 1, 0), 2), (0, 1)):
        r = field_(ctx, st, None, field, count, SPACE, dev=dev)
        assert r.res.n_failed == 0
    assert [int(x) for x in np.diff(field_(ctx, st, None, 0, TO_END, SPACE, dev=dev).text_index)] == [len(s) for s in stored]


def test_raw_and_empty_records_have_one_empty_field(ctx):
    texts = [corpus.text_like(n, 0xF1E1D060 + n).tobytes() for n in (50, 0, 70, 60, 0)]
    tab = oracle_table(np.frombuffer(b"".join(texts), np.uint8))
    bodies = [want_encode(tab, t)[1] for t in texts]
    bodies[2] = b""  # no bytes under a length of 70: kept raw elsewhere
    st = make_store(tab, texts, bodies)
    rows = np.array([2, 0, 2, 1, 4, 2, 3, 1])
    for field, count in ((0, TO_END), (0, 1), (0, 0), (1, 1), (1, 0)):
        r = field_(ctx, st, rows, field, count, SPACE)
        assert all(r.want.pos[k] == (0 if field == 0 else ABSENT) for k in (0, 2, 3, 4, 5, 7)) and r.res.n_failed == 0
    r = field_(ctx, st, [2, 1, 4, 2], 0, TO_END, SPACE)
    assert r.res.out_bytes == 0 and r.res.text_bytes == 0 and bool((r.host == SENTINEL).all())


# --- 5. copy, scan and selection ---------------------------------------------------------------------------------------------------------------


def test_begin_bits_and_bit_counts_on_both_paths(ctx):
    st, _ = main_fixture()
    rows, field, count = phase_rows()
    r = field_(ctx, st, rows, field, count, SPACE)
    assert r.res.n_failed == 0 and r.res.text_bytes == sum(len(t) for t in r.want.texts)
    field_(ctx, st, rows, field, count, SPACE, no_pos=True)  # d_pos == NULL


def test_fields_of_0_to_33_bits_share_destination_words(ctx):
    st, rows, field, count = small_fields_fixture()
    want = want_field(st, rows, field, count, 100)
    sizes = np.diff(want.body_index)
    assert sizes.max() <= 5 and set(range(6)) == set(int(x) for x in sizes)
    per_word = np.bincount((want.body_index[:-1][sizes > 0] // 16).astype(np.int64))
    assert per_word.max() >= 6  # many rows begin inside one 16-byte destination word
    field_(ctx, st, rows, field, count, 100)


@pytest.mark.parametrize("place", ["between", "start", "end"])
def test_a_run_of_5000_empty_and_absent_results(ctx, place):
    st, texts = main_fixture()
    last9, last13 = texts[9].count(b" "), texts[13].count(b" ")
    kinds = [(5, 0, 0), (0, 0, 1), (6, 0xFFFFFFFE, 1), (8, texts[8].count(b" ") + 1, TO_END), (0, 1, 1)]  # no field asked for, the empty record's, absent ones
    empties = [kinds[i % 5] for i in range(5000)]
    assert 5000 > SCAN_TILE
    full = [(9, 3, last9), (13, last13 // 2, 400)]
    cases = {"between": full[:1] + empties + full[1:], "start": empties + full, "end": full + empties}[place]
    rows, field, count = (np.array(x) for x in zip(*cases))
    r = field_(ctx, st, rows, field, count, SPACE)
    assert int(np.count_nonzero(np.diff(r.body_index))) == 2 and int(np.count_nonzero(r.want.pos == ABSENT)) == 3000


@pytest.mark.parametrize("shift", range(16))
def test_every_output_base_and_body_alignment(ctx, shift):
    import torch

    st, texts = main_fixture()
    lead = shift  # d_bodies at every alignment of 16, and with it every body
    d = torch.full((lead + st.bodies.size + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
    d[lead : lead + st.bodies.size] = torch.from_numpy(st.bodies).cuda()
    dev = (d[lead : lead + st.bodies.size], _dev_index(st.body_index), _dev_index(st.text_index))
    assert d.data_ptr() % 16 == 0 and dev[0].data_ptr() % 16 == lead
    rng = np.random.default_rng(0xF1E1D080 + shift)
    rows = rng.integers(0, st.n, size=300)
    r = field_(ctx, st, rows, [int(rng.integers(0, texts[r].count(b" ") + 2)) for r in rows], np.where(rng.integers(0, 2, size=300) == 0, 1, rng.integers(0, 300, size=300)), SPACE,
               dev=dev, shift=shift)
    assert r.d_out.data_ptr() % 16 == shift
    field_(ctx, st, [13, 0, 2, 13], [1, 0, 0, 5000], [TO_END, 5, 1, TO_END], SPACE, dev=dev, shift=shift)


@pytest.mark.parametrize("name", SELECTIONS)
def test_rows_in_every_order_and_with_repeats(ctx, name):
    st, _ = main_fixture()
    rows = selection(name, st.n)
    rng = np.random.default_rng(0xF1E1D090)
    field_(ctx, st, rows, rng.integers(0, 9, size=rows.size), rng.integers(0, 500, size=rows.size), ord("e"))
    if name == "identity":
        with_rows = field_(ctx, st, rows, 4, 100, SPACE)
        without = field_(ctx, st, None, 4, 100, SPACE)
        assert without.res == with_rows.res and np.array_equal(without.host[without.at : without.at + without.cap], with_rows.host[with_rows.at : with_rows.at + with_rows.cap])


# --- 6. the call's own behaviour ----------------------------------------------------------------------------------------------------------------


def test_failures_stay_local(ctx):
    st, bad = failures_store()  # random bytes: under table_255 every byte string is a text
    st.tab = table_255()
    st.cb = _cb(st.tab)
    dev = upload(st, spare=4096)
    rows = np.array([0, 16, 1, 3, 2, 0xFFFFFFFF, 8, 4, 15, 9, 5, 11, 6, 14, 12, 13, 7, 10, 3, 0], dtype=np.uint32)
    want = want_field(st, rows, 0, 2, 9)
    assert [int(s) for s in want.status] == [bad.get(int(r), OK) if r < 16 else ARG for r in rows]
    r = check_field(run_field(ctx, st, dev, rows, 0, 2, 9, want.total), want)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (9, 1, ARG)
    for k in np.flatnonzero(want.status):  # a failed row is an empty record without a position
        assert r.body_index[k] == r.body_index[k + 1] and r.text_index[k] == r.text_index[k + 1] and r.pos[1 + k] == ABSENT
    r = field_(ctx, st, np.array([0, 1, 2, 15, 9, 3], dtype=np.uint32), 0, TO_END, 9, dev=dev)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 3, UNSUPPORTED)
    r = field_(ctx, st, np.array([13, 0, 1, 2, 4, 5, 6, 7, 10, 12, 13], dtype=np.uint32), 1, 1, 9, dev=dev)  # a bad record that no row selects does not matter
    assert r.res.n_failed == 0 and not r.status.any()
    want = want_field(st, None, 0, 1, 9)  # d_rows == NULL: every record, the bad ones among them
    r = check_field(run_field(ctx, st, dev, None, 0, 1, 9, want.total), want)
    assert r.res.n_failed == len(bad)


def test_capacity_and_sizes_only_leave_the_positions_complete(ctx):
    st, texts = main_fixture()
    rng = np.random.default_rng(0xF1E1D0A0)
    rows = np.concatenate((rng.integers(0, st.n, size=400), [st.n + 5, 0]))  # (one row fails: d_status is complete either way)
    field, count = rng.integers(0, 30, size=402), rng.integers(0, 50, size=402)
    dev = upload(st)
    want = want_field(st, rows, field, count, SPACE)
    args = (ctx, st, dev, rows, field, count, SPACE)
    exact = check_field(run_field(*args, want.total), want)
    assert exact.res.n_failed == 1
    check_field(run_field(*args, want.total - 1), want, call_status=CAP)
    check_field(run_field(*args, 1), want, call_status=CAP)
    sizes_only = check_field(run_field(*args, want.total, sizes_only=True), want)
    assert sizes_only.res == exact.res
    check_field(run_field(*args, want.total + 1000), want)  # the ctx is as good as before; room to spare stays untouched


def _raw_call(ctx, st, dev, n_rows, d_rows, d_out, d_a, d_b, res, cb=None, delim=SPACE, **ptr):
    """One call through the C ABI; ptr: p_rows, p_field, p_n, p_pos, p_out -- addresses (or None) in place of those arrays -- and cap."""
    from entreepy_amd import _native as N

    d_bodies, d_body_index, d_text_index = dev
    return N.lib().et_field_packed_device(ctx._h, ctypes.byref((cb or st.cb).raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n,
                                          ptr.get("p_rows", d_rows.data_ptr()), n_rows, ptr.get("p_field"), 0, ptr.get("p_n"), TO_END, delim, ptr.get("p_out", d_out.data_ptr()),
                                          ptr.get("cap", d_out.numel()), d_a.data_ptr(), d_b.data_ptr(), ptr.get("p_pos"), None, ctypes.byref(res))


def test_argument_errors_no_rows_and_an_incomplete_table_enqueue_nothing(ctx):
    """The checks that come before anything touches a device, with a context that could go on: ET_ERR_ARG, *res untouched, nothing
    enqueued -- every output and the bodies hold what they held; no rows: ET_OK and *res zeroed; a table with a hole: unsupported."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    st, _ = main_fixture()
    dev = upload(st)
    before = dev[0].clone()
    d_rows, d_u32 = dev_rows([1, 2]), dev_rows([0, 0, 0])
    d_out = torch.full((4000,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_a, d_b = (torch.full((3,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_pos = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    fresh = lambda: N.TakeResult(out_bytes=99, text_bytes=98, n_failed=97, first_failed=96, first_status=95)  # noqa: E731
    untouched = lambda res: (res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (99, 98, 97, 96, 95)  # noqa: E731
    inside = dev[0].data_ptr() + 8
    cases = {"a misaligned d_field": dict(p_field=d_u32.data_ptr() + 1), "a misaligned d_n_fields": dict(p_n=d_u32.data_ptr() + 2), "misaligned d_rows": dict(p_rows=d_rows.data_ptr() + 3),
             "a misaligned d_pos": dict(p_pos=d_pos.data_ptr() + 2), "d_out inside d_bodies": dict(p_out=inside, cap=16),
             "d_out around d_bodies' end": dict(p_out=dev[0].data_ptr() + dev[0].numel() - 1, cap=64), "no d_rows, and n_rows is not n_records": dict(p_rows=None),
             "a delimiter below 0": dict(delim=-1), "a delimiter above 255": dict(delim=256), "a delimiter far above": dict(delim=1 << 20)}
    for what, ptr in cases.items():
        res = fresh()
        assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, **ptr) == ARG, what
        assert untouched(res), f"{what}: *res was touched"
    res = fresh()
    assert _raw_call(ctx, st, dev, 0x80000000, d_rows, d_out, d_a, d_b, res) == ARG and untouched(res)
    res = fresh()
    assert _raw_call(ctx, st, dev, 0, d_rows, d_out, d_a, d_b, res) == OK
    assert (res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (0, 0, 0, 0, 0)
    data, length = (a.copy() for a in st.tab)
    length[int(np.flatnonzero(length)[0])] = 0  # a hole in the tree
    res = fresh()
    assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, cb=E.Codebook.from_tables(data, length)) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_a == -1).all()) and bool((d_b == -1).all()) and bool((d_pos == -7).all()) and torch.equal(dev[0], before), "something was enqueued"
    want = want_field(st, [1, 2], 0, TO_END, SPACE)  # the same arguments, well-formed: the aligned arrays are accepted, the ctx is as good as before
    res, d_to_end = N.TakeResult(), dev_rows([TO_END, TO_END])
    assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, p_field=d_u32.data_ptr(), p_n=d_to_end.data_ptr(), p_pos=d_pos.data_ptr()) == OK
    torch.cuda.synchronize()
    assert res.out_bytes == want.total and d_out[: want.total].cpu().numpy().tobytes() == want.data.tobytes() and bool((d_out[want.total :] == SENTINEL).all())
    assert d_pos.tolist() == [0, 0, -7, -7]


def test_offsets_above_4_gib(ctx):
    import torch

    page_len = 256 << 10
    pool = corpus.text_like(page_len, 0xF1E1D0B0)
    pool[pool == BAR] = SPACE
    for first in range(20, 60):  # one delimiter, at symbol first - 1: field 1 begins inside a source byte
        text = pool.copy()
        text[first - 1] = BAR
        tab = oracle_table(text)
        if int(tab[1][text[:first]].astype(np.int64).sum()) % 8:
            break
    cb = _cb(tab)
    body = np.frombuffer(want_encode(tab, text)[1], np.uint8)
    piece = np.frombuffer(want_encode(tab, text[first:])[1], np.uint8)  # what every long row becomes
    small = np.frombuffer(want_encode(tab, text[: first - 1])[1], np.uint8)
    L, P = body.size, piece.size
    assert page_len <= _small_max()
    d_body, d_piece = torch.from_numpy(body.copy()).cuda(), torch.from_numpy(piece.copy()).cuda()
    # output: field 1 of one record n_pages times behind one row of a few bytes (field 0), so that a row straddles 2^32
    n_pages = (1 << 32) // P + 3
    total = small.size + n_pages * P
    n_rows = n_pages + 1
    d_field = torch.ones((n_rows,), dtype=torch.int32, device="cuda")
    d_field[0] = 0
    d_raw = torch.full((LEAD + total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((n_rows + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_status = torch.full((n_rows,), 0xEE, dtype=torch.uint8, device="cuda")
    d_pos = torch.full((n_rows,), -7, dtype=torch.int32, device="cuda")
    res = ctx.field_packed_device(cb, d_body, _dev_index([0, L]), _dev_index([0, page_len]), torch.zeros(n_rows, dtype=torch.int32, device="cuda"), d_field, 1, BAR,
                                  d_raw[LEAD : LEAD + total], d_bi, d_ti, pos=d_pos, status=d_status)
    torch.cuda.synchronize()
    n = page_len - first
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed) == (OK, total, first - 1 + n_pages * n, 0)
    steps = torch.arange(n_rows + 1, dtype=torch.int64, device="cuda")
    want_bi, want_ti = steps * P + (small.size - P), steps * n + (first - 1 - n)
    want_bi[0] = want_ti[0] = 0
    assert torch.equal(d_bi, want_bi) and torch.equal(d_ti, want_ti) and not bool(d_status.any())
    assert int(d_pos[0]) == 0 and bool((d_pos[1:] == first).all())
    assert total > 1 << 32
    d_out = d_raw[LEAD : LEAD + total]
    assert d_out[: small.size].cpu().numpy().tobytes() == small.tobytes()
    assert torch.equal(d_out[small.size :].view(n_pages, P), d_piece.unsqueeze(0).expand(n_pages, P)), "a row differs from the oracle's encode of the field"
    assert bool((d_raw[:LEAD] == SENTINEL).all()) and bool((d_raw[LEAD + total :] == SENTINEL).all())
    del d_out, d_raw
    # input: a body behind offset 2^32 + 37 of a zero-filled buffer, another at 0, a record of length zero that spans what lies between
    far = (1 << 32) + 37
    d_bodies = torch.zeros(far + L + 1, dtype=torch.uint8, device="cuda")
    d_bodies[:L] = d_body
    d_bodies[far : far + L] = d_body
    d_raw = torch.full((LEAD + 3 * P + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((5,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_status = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    d_pos = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    res = ctx.field_packed_device(cb, d_bodies[: far + L], _dev_index([0, L, far, far + L]), _dev_index([0, page_len, page_len, 2 * page_len]), dev_rows([2, 1, 0, 2]), 1, TO_END, BAR,
                                  d_raw[LEAD : LEAD + 3 * P], d_bi, d_ti, pos=d_pos, status=d_status)
    torch.cuda.synchronize()
    # (record 1's body of 2^32 + 37 - L zeros is above 4 * small_max: that row fails alone)
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (OK, 3 * P, 3 * n, 1, 1, UNSUPPORTED)
    assert d_bi.tolist() == [0, P, P, 2 * P, 3 * P] and d_ti.tolist() == [0, n, n, 2 * n, 3 * n] and d_status.tolist() == [OK, UNSUPPORTED, OK, OK]
    assert d_pos.tolist() == [first, -1, first, first]
    assert torch.equal(d_raw[LEAD : LEAD + 3 * P].view(3, P), d_piece.unsqueeze(0).expand(3, P))
    assert bool((d_raw[:LEAD] == SENTINEL).all()) and bool((d_raw[LEAD + 3 * P :] == SENTINEL).all())


# --- 7. consistency with the neighbouring calls ---------------------------------------------------------------------------------------------------


def test_field_0_is_the_slice_up_to_the_delimiter_and_the_positions_slice_the_same_store(ctx):
    st, _ = main_fixture()
    dev = upload(st)
    f = field_(ctx, st, None, 0, 1, SPACE, dev=dev)
    want = want_slice(st, None, 0, TO_END, SPACE)
    s = check_take(run_slice(ctx, st, dev, None, 0, TO_END, SPACE, want.total), want)
    assert s.res == f.res and np.array_equal(s.body_index, f.body_index) and np.array_equal(s.text_index, f.text_index)
    assert np.array_equal(s.host[s.at : s.at + want.total], f.host[f.at : f.at + want.total])
    rows, field, count = phase_rows()
    f = field_(ctx, st, rows, field, count, SPACE, dev=dev)
    present = f.want.pos != ABSENT
    firsts, counts = np.where(present, f.want.pos, 0), np.diff(f.text_index).astype(np.int64)  # (an absent row has length 0: the slice of nothing)
    want = want_slice(st, rows, firsts, counts)
    s = check_take(run_slice(ctx, st, dev, rows, f.pos[1:-1] * present, counts, None, want.total), want)
    assert np.array_equal(s.body_index, f.body_index) and np.array_equal(s.host[s.at : s.at + want.total], f.host[f.at : f.at + want.total])


def _tables_of(cb):
    return np.array(cb.raw.data, dtype=np.uint32), np.array(cb.raw.length, dtype=np.uint8)


def test_field_join_gather_and_match_take_field_on_one_context(ctx):
    """encode_packed of CSV lines and of a key set -> field 2 -> join against the keys -> gather; then match(prefix) -> take -> field 1 of
    the taken store: nothing is synchronised in between, and text appears at the very end only."""
    import torch

    import entreepy_amd as E

    rng = np.random.default_rng(0xF1E1D0C0)
    users = [b"u%03d" % i + bytes(rng.choice(np.frombuffer(b"abc", np.uint8), size=int(rng.integers(0, 4))).tobytes()) for i in range(300)]
    lines = []
    for i in range(2000):
        who = users[int(rng.integers(0, 300))]
        lines.append({0: b"get,%d," % i + who + b",ok", 1: b"put,," + who, 2: b"get,h%d" % i, 3: b"del,1," + who + b"," + who + b",", 4: b"get,x,,y"}[i % 5])
    keys = users[::3]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(lines + users), np.uint8), minlength=256))
    sides = []
    for column in (keys, lines):
        index = _index_of([len(w) for w in column])
        d_text, d_index = _dev_bytes(np.frombuffer(b"".join(column), np.uint8)), _dev_index(index)
        d_out = torch.empty(cb.body_bound(int(index[-1])) + len(column), dtype=torch.uint8, device="cuda")
        sides.append((d_out, torch.empty(len(column) + 1, dtype=torch.int64, device="cuda"), d_index, d_text))
    n = len(lines)
    d_rows, d_hits, d_key, d_pos = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(4))
    d_raw = torch.full((LEAD + 16 * n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ids, d_bi, d_ti = d_raw[LEAD:], torch.full((n + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_texts = torch.full((16 * n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_texts_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_taken, d_tbi, d_tti = torch.full((64 * n,), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((n + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_f1, d_fbi, d_fti = torch.full((16 * n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((n + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    enc = [ctx.encode_packed_device(cb, s[3], s[2], s[0], s[1]) for s in sides]
    key_store, line_store = ((s[0][: e.out_bytes], s[1], s[2]) for s, e in zip(sides, enc))
    f = ctx.field_packed_device(cb, *line_store, None, 2, 1, b",", d_ids[: 16 * n], d_bi, d_ti, pos=d_pos)
    ids = (d_ids[: max(f.out_bytes, 1)], d_bi, d_ti)
    j = ctx.join_packed_device(cb, *ids, *key_store, rows=d_hits, key_of_row=d_key)
    g = ctx.decode_packed_gather_device(cb, *ids, d_hits[: j.n_match], d_texts[: 16 * n], d_texts_index[: j.n_match + 1])
    m = ctx.match_packed_device(cb, *line_store, b"get,", E.MATCH_PREFIX, rows=d_rows)
    t = ctx.take_packed_device(*line_store, d_rows[: m.n_match], d_taken, d_tbi[: m.n_match + 1], d_tti[: m.n_match + 1])
    f1 = ctx.field_packed_device(cb, d_taken[: max(t.out_bytes, 1)], d_tbi[: m.n_match + 1], d_tti[: m.n_match + 1], None, 1, 1, b",", d_f1[: 16 * n], d_fbi[: m.n_match + 1],
                                 d_fti[: m.n_match + 1])
    torch.cuda.synchronize()
    # the same pipelines in Python
    cut = [py_field(l, 2, 1, COMMA) for l in lines]
    hits = [k for k, (c, _) in enumerate(cut) if c in set(keys)]
    assert 0 < len(hits) < n and any(p == ABSENT for _, p in cut) and any(c == b"" and p != ABSENT for c, p in cut)
    assert all(e.status == OK and e.n_failed == 0 for e in enc)
    assert (f.status, f.n_failed, f.text_bytes) == (OK, 0, sum(len(c) for c, _ in cut)) and _guards_intact(d_ids, f.out_bytes)
    assert d_pos.cpu().numpy().view(np.uint32).tolist() == [p for _, p in cut]
    assert d_ids[: f.out_bytes].cpu().numpy().tobytes() == b"".join(want_encode(_tables_of(cb), c)[1] for c, _ in cut)
    assert (j.status, j.n_failed, j.n_keys_failed) == (OK, 0, 0) and d_hits[: j.n_match].tolist() == hits
    assert d_key[: j.n_match].tolist() == [keys.index(cut[k][0]) for k in hits]
    assert (g.status, g.n_failed, g.n_short) == (OK, 0, 0) and d_texts[: g.out_bytes].cpu().numpy().tobytes() == b"".join(cut[k][0] for k in hits)
    gets = [l for l in lines if l.startswith(b"get,")]
    second = [py_field(l, 1, 1, COMMA)[0] for l in gets]
    assert (m.status, m.n_match, t.status, t.n_failed) == (OK, len(gets), OK, 0)
    assert (f1.status, f1.n_failed, f1.text_bytes) == (OK, 0, sum(len(c) for c in second))
    assert d_f1[: f1.out_bytes].cpu().numpy().tobytes() == b"".join(want_encode(_tables_of(cb), c)[1] for c in second) and bool((d_f1[f1.out_bytes :] == SENTINEL).all())


def test_list_helper_returns_a_store_of_the_fields_and_their_positions(ctx):
    import entreepy_amd as E

    assert (E.FIELD_TO_END, E.FIELD_ABSENT) == (TO_END, ABSENT)
    _, texts = main_fixture()
    texts = texts[:30]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(texts), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, texts)
    lengths = [len(t) for t in texts]
    rng = np.random.default_rng(0xF1E1D0D0)
    rows = np.concatenate((rng.integers(0, 30, size=80), [0, 0, 29, 4]))
    field, count = rng.integers(0, 60, size=rows.size), rng.integers(0, 20, size=rows.size)
    for f, c, delim in ((field, count, b" "), (2, 1, b" "), (field, E.FIELD_TO_END, ord("e")), (0, count, b"t")):
        new_blob, new_index, new_lengths, pos = ctx.field_packed(cb, blob, out_index, lengths, rows, f, c, delim=delim)
        want = [py_field(texts[r], ff, cc, delim if isinstance(delim, int) else delim[0]) for r, ff, cc in zip(rows, per_row(f, rows.size), per_row(c, rows.size))]
        assert [int(x) for x in new_lengths] == [len(w) for w, _ in want] and pos.tolist() == [p for _, p in want]
        assert (new_blob, new_index.tolist()) == (lambda b, i: (b, i.tolist()))(*ctx.encode_packed(cb, [w for w, _ in want]))
        assert ctx.decode_packed(cb, new_blob, new_index, new_lengths) == [w for w, _ in want]
    assert ctx.field_packed(cb, blob, out_index, lengths, [], 0)[0] == b""
    csv = [b"a,b,c", b"", b"one", b",x,"]
    csv_cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(csv), np.uint8), minlength=256))
    csv_blob, csv_index = ctx.encode_packed(csv_cb, csv)
    got = ctx.field_packed(csv_cb, csv_blob, csv_index, [len(t) for t in csv], [0, 1, 2, 3], 1)  # the defaults: one field, the comma
    assert ctx.decode_packed(csv_cb, *got[:3]) == [b"b", b"", b"", b"x"] and got[3].tolist() == [2, ABSENT, ABSENT, 1]
    with pytest.raises(E.EntreepyError, match="row 1") as e:
        ctx.field_packed(csv_cb, csv_blob, csv_index, [len(t) for t in csv], [3, 4, 0], 0)
    assert e.value.status == ARG


# --- 8. the state a context keeps between calls -----------------------------------------------------------------------------------------------
# The cells of tests/test_gpu_retained.py for the row `field` (tests/retained_field.py): a field call between the call that sets a state
# and the calls that read it leaves the histogram link, the held range and the last codebook as they were.


@pytest.mark.parametrize("reader", ["body", "head", "on_host"])
def test_histogram_link_survives_a_field_call(reader):
    from tests import test_gpu_retained as G

    G.test_histogram_link("field", reader)


@pytest.mark.parametrize("how", ["sync", "maps", "between", "windows"])
def test_held_range_survives_a_field_call(how):
    from tests import test_gpu_retained as G

    G.test_held_range("field", how)


def test_last_codebook_survives_a_field_call():
    from tests import test_gpu_retained as G

    G.test_last_codebook("field")
