"""GPU: et_slice_packed_device -- symbols [first, first + count) of a selection's records, cut in front of a stop byte, as a new packed
store, found and copied on the compressed bytes -- against the oracle: a row's status is judged from its record's own two pairs of
offsets, its stored text is want_decode's, the slice is Python's (text[first : first + count], then [: find(stop)]), and the expected
bytes are the oracle's shared-table encode of that slice (want_slice()); never the bit rule the kernels implement.  d_out lies between
sentinel bytes as in tests/test_gpu_take.py, whose check_take() compares bytes, both offset arrays, the status bytes and the report.

The stores and the rows are made by the *_fixture functions below, without a GPU: tests/test_slice_host.py checks on the same fixtures
that the bit rule gives what the oracle gives, and that they reach the cases named here."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus, limits
from tests import retained_slice  # noqa: F401  (the call's row joins the table of tests/retained.py)
from tests.test_gpu_batch import SENTINEL, _oracle, _small_max
from tests.test_gpu_gather import dev_rows, make_store, upload
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_gpu_shared import _cb, want_decode, want_encode
from tests.test_gpu_take import C, LEAD, SCAN_TILE, SELECTIONS, _guards_intact, check_take, failures_store, selection
from tests.test_shared_host import oracle_table, table_255, table_2bit, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
TO_END, NO_STOP = 0xFFFFFFFF, -1  # ET_SLICE_TO_END, ET_SLICE_NO_STOP
LANE_BITS = 256  # what a lane of the workgroup path owns of a block (csrc/et_batch.hip settle_block)
BLOCK_BITS = 65536  # the 8 KiB block the workgroup path stages


def lane_bytes():
    """What of a body the slice's end can reach (reach()) up to this many bytes is walked by one lane, more by a workgroup."""
    from entreepy_amd import _native as N

    return int(N.lib().et_slice_lane_bytes())


def reach(st, r, first, count):
    """The bytes of record r's body that the walk to the slice's end can touch: 4 bytes per symbol in front of the end, and 8
    (csrc/et_batch.h clip_body) -- what decides between the lane and the workgroup."""
    nb, length = int(st.body_index[r + 1] - st.body_index[r]), int(st.text_index[r + 1] - st.text_index[r])
    return min(nb, 4 * min(first + count, length) + 8)


# --- the expected store: the oracle's texts, Python's slices, the oracle's encode ------------------------------------------------------


def stored_text(st, r):
    """Record r's stored text: what every packed call takes it for.  Once per store and record."""
    memo = st.__dict__.setdefault("stored", {})
    if r not in memo:
        b0, b1, t0, t1 = (int(x) for x in (st.body_index[r], st.body_index[r + 1], st.text_index[r], st.text_index[r + 1]))
        memo[r] = want_decode(st.tab, st.bodies[b0:b1].tobytes(), t1 - t0)[1]
    return memo[r]


def py_slice(text, first, count, stop):
    s = text[first : first + count]  # (Python's ints do not wrap)
    if stop is not None and 0 <= stop <= 255:
        i = s.find(bytes([stop]))
        s = s[:i] if i >= 0 else s
    return s


def per_row(v, n):
    return [int(v)] * n if np.isscalar(v) else [int(x) for x in v]


def want_slice(st, rows, first, count, stop=None):
    """-> what tests/test_gpu_take.py's model() returns, for the slices: status by the take's rule, then the oracle's encode."""
    small, body_bytes = _small_max(), st.bodies.size
    rows = np.arange(st.n) if rows is None else np.asarray(rows, dtype=np.int64)
    firsts, counts = per_row(first, rows.size), per_row(count, rows.size)
    if isinstance(stop, bytes):
        (stop,) = stop
    memo = st.__dict__.setdefault("sliced", {})
    status, nb, ln, pieces, texts = np.full(rows.size, ARG, np.uint8), np.zeros(rows.size, np.uint64), np.zeros(rows.size, np.uint64), [], []
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
        key = (r, firsts[k], counts[k], stop)
        if key not in memo:
            s = py_slice(stored_text(st, r), firsts[k], counts[k], stop)
            rc, body = want_encode(st.tab, s)
            assert rc == OK
            memo[key] = (s, np.frombuffer(body, np.uint8))
        s, body = memo[key]
        status[k], nb[k], ln[k], texts[k] = OK, body.size, len(s), s
        pieces.append(body)
    data = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    return SimpleNamespace(status=status, body_index=_index_of(nb), text_index=_index_of(ln), data=data, total=int(nb.sum()), text_total=int(ln.sum()), texts=texts)


# --- the fixtures ----------------------------------------------------------------------------------------------------------------------
MAIN_SIZES = [0, 1, 2, 3, 9, 40, 100, 300, 700, 1000, 1500, 3000, 20000, 40000]


@functools.lru_cache(maxsize=None)
def main_fixture():
    """44 records of text under the table of their own bytes: the sizes above and 30 random ones up to 2 500 -> (store, [texts])."""
    rng = np.random.default_rng(0x511CE001)
    sizes = np.concatenate((MAIN_SIZES, rng.integers(0, 2501, size=30)))
    pool = corpus.text_like(int(sizes.sum()), 0x511CE002)
    cuts = _index_of(sizes)
    texts = [pool[int(cuts[i]) : int(cuts[i + 1])].tobytes() for i in range(sizes.size)]
    return make_store(oracle_table(pool), texts), texts


@functools.lru_cache(maxsize=None)
def phase_rows():
    """900 (row, first, count) over the main fixture, a third of them with few symbols in front of their end (the lane's), a third far
    into the two long records (the workgroup's) -> three arrays."""
    st, texts = main_fixture()
    rng = np.random.default_rng(0x511CE003)
    rows, first, count = [], [], []
    for i in range(900):
        r = int(rng.integers(0, st.n)) if i % 3 else int(rng.integers(12, 14))
        n = len(texts[r])
        f = int(rng.integers(0, min(n, 100) + 1)) if i % 3 == 1 else int(rng.integers(0, n + 1))
        rows.append(r), first.append(f), count.append(int(rng.integers(0, 20)) if i % 3 == 1 else int(rng.integers(0, 400)))
    return np.array(rows), np.array(first), np.array(count)


def bit_at(st, r, i):
    """The bit, from the aligned word record r's body begins in -- as the kernels count --, at which symbol i of its text begins."""
    text = np.frombuffer(stored_text(st, r), np.uint8)
    return (int(st.body_index[r]) % 4) * 8 + int(st.tab[1][text[:i]].astype(np.int64).sum())


@functools.lru_cache(maxsize=None)
def edge_rows():
    """Slices of the main fixture's longest record at the workgroup path's edges -> {case: (row, first, count)}: across a lane edge,
    across several lanes, across the 8 KiB block edge (begin in block 0, end in block 1), ending with the block, beginning with block 1."""
    st, texts = main_fixture()
    r = 13
    starts = bit_at(st, r, 0) + np.concatenate(([0], np.cumsum(st.tab[1][np.frombuffer(texts[r], np.uint8)].astype(np.int64))))
    at_block = int(np.searchsorted(starts, BLOCK_BITS))  # the first symbol that begins at or behind the block edge
    at_lane = int(np.searchsorted(starts, 40 * LANE_BITS))
    return {"lane_edge": (r, at_lane - 1, 2), "lanes": (r, at_lane - 30, 400), "block_edge": (r, at_block - 20, 45), "block_end": (r, at_block - 200, 200),
            "block_begin": (r, at_block, 300), "blocks": (r, 7, len(texts[r]) - 11), "short_of_long": (r, 3, 12)}


def stop_rows(stop=ord(" ")):
    """Rows of the main fixture for the stop byte -> {case: (row, first, count)}, on a lane's record and on a workgroup's: the stop at
    `first` itself, absent from the slice's record part, behind the count only, inside the count."""
    st, texts = main_fixture()
    out = {}
    for tag, r in (("lane", 7), ("long", 13)):
        t = texts[r]
        far = 2000 if tag == "long" else 0  # (far enough in that the slice's end reaches more than a lane takes)
        p = next(i for i in range(far + 30, len(t)) if t[i] == stop and stop not in t[i - 9 : i])
        run = max(range(far, len(t) - 40), key=lambda i: (t.find(bytes([stop]), i) - i) if t.find(bytes([stop]), i) >= 0 else 0)  # the longest stretch without one
        gap = t.find(bytes([stop]), run) - run
        out[tag + "_at_first"] = (r, p, 50)
        out[tag + "_inside"] = (r, p - 9, 50)
        out[tag + "_behind_count"] = (r, run, gap)  # the slice ends right in front of the stop: the count ends it
        out[tag + "_absent"] = (r, run, gap - 1)
    return out


@functools.lru_cache(maxsize=None)
def pad_fixture():
    """Under the 2-bit table (A = 00, C, G, T = 11) -> (store, [texts]): texts without A whose pad bits (zeros) read as A, and -- the
    second half, bodies hand-made -- texts without T whose pad bits are SET and read as T; a short and a long one of each, lengths that
    leave 2, 4 and 6 pad bits."""
    rng = np.random.default_rng(0x511CE010)
    texts = [bytes(rng.choice(np.frombuffer(b"CGT", np.uint8), size=n).tobytes()) for n in (3, 7, 2, 3001, 5002, 2999)]
    texts += [bytes(rng.choice(np.frombuffer(b"ACG", np.uint8), size=n).tobytes()) for n in (3, 7, 2, 3001, 5002, 2999)]
    st = make_store(table_2bit(), texts)
    for r in range(6, 12):
        pad = 8 - 2 * (len(texts[r]) % 4)
        assert 0 < pad < 8
        st.bodies[int(st.body_index[r + 1]) - 1] |= (1 << pad) - 1
    return st, texts


@functools.lru_cache(maxsize=None)
def set_pad_fixture():
    """The main fixture's records with every pad bit of every body SET (hand-made bodies) -> (store, [texts])."""
    st, texts = main_fixture()
    bodies = []
    for r, t in enumerate(texts):
        body = bytearray(st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes())
        pad = len(body) * 8 - int(st.tab[1][np.frombuffer(t, np.uint8)].astype(np.int64).sum())
        if pad:
            body[-1] |= (1 << pad) - 1
        bodies.append(bytes(body))
    return make_store(st.tab, texts, bodies), texts


@functools.lru_cache(maxsize=None)
def cut_fixture():
    """The main fixture's records 6 .. 13 with their bodies cut: by one byte, to a half, to one byte; the lengths kept -> store."""
    st, texts = main_fixture()
    keep, bodies = [], []
    for r in range(6, 14):
        body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes()
        for cut in (body[:-1], body[: len(body) // 2], body[:1]):
            keep.append(texts[r])
            bodies.append(cut)
    return make_store(st.tab, keep, bodies)


@functools.lru_cache(maxsize=None)
def ladder_fixture():
    """Under the ladder table (codewords of 1 .. 32 bits): record 0 = the 33 symbols in order, 40 times (a slice of one symbol has 1 ..
    32 bits, of symbols 0 and 31 together 33); records 1 and 2 = limits.py's `phases` and `uniform` texts of 2 000 and 6 000 symbols,
    the 32-bit codewords at every bit offset -> store."""
    t = limits.ladder32()
    texts = [bytes(range(100, 133)) * 40, limits.phases(t, 2000).tobytes(), limits.uniform(t, 6000).tobytes(), bytes([131, 132]) * 9]
    return make_store(table_ladder(), texts)


@functools.lru_cache(maxsize=None)
def bytes_fixture():
    """Under table_255 (byte 1: 7 bits, every other: 8) -> store: record 0 begins with byte 1, so a slice from first >= 1 is `count` bytes
    that begin at bit 7 of a source byte; record 1 holds no byte 1: slices copy whole bytes."""
    rng = np.random.default_rng(0x511CE020)
    texts = [b"\x01" + rng.integers(2, 256, size=3 * C, dtype=np.uint8).tobytes(), rng.integers(2, 256, size=3 * C, dtype=np.uint8).tobytes()]
    return make_store(table_255(), texts)


# --- one call and its check ------------------------------------------------------------------------------------------------------------


def dev_u32(v):
    return v if np.isscalar(v) else dev_rows(v)


def run_slice(ctx, st, dev, rows, first, count, stop, cap, sizes_only=False, shift=0, tile_off=None):
    """One call, every output full of sentinels first (tests/test_gpu_take.py's run_take).  rows=None: d_rows == NULL."""
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
    torch.cuda.synchronize()
    r.res = ctx.slice_packed_device(st.cb, d_bodies, d_body_index, d_text_index, None if rows is None else dev_rows(rows), dev_u32(first), dev_u32(count),
                                    None if sizes_only else r.d_out, r.d_body_index, r.d_text_index, stop=stop, status=r.d_status)
    torch.cuda.synchronize()
    r.host = r.d_raw.cpu().numpy()
    r.body_index, r.text_index = r.d_body_index.cpu().numpy().view(np.uint64), r.d_text_index.cpu().numpy().view(np.uint64)
    r.status = r.d_status.cpu().numpy()
    return r


def slice_(ctx, st, rows, first, count, stop=None, dev=None, **kw):
    """Run with cap = the need exactly, and check."""
    want = want_slice(st, rows, first, count, stop)
    r = check_take(run_slice(ctx, st, dev or upload(st), rows, first, count, stop, want.total, **kw), want)
    r.want = want
    return r


def triples(cases):
    rows, first, count = (np.array(x) for x in zip(*cases))
    return rows, first, count


# --- 1. slice bounds ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("count", ["0", "1", "7", "len", "to_end"])
def test_first_and_count_at_the_edges_of_the_text(ctx, count):
    st, texts = main_fixture()
    dev, lens = upload(st), np.array([len(t) for t in texts], dtype=np.int64)
    counts = {"0": 0, "1": 1, "7": 7, "len": lens, "to_end": TO_END}[count]
    for first in (0, 1, np.maximum(lens - 1, 0), lens, lens + 1, 0xFFFFFFFF):
        r = slice_(ctx, st, None, first, counts, dev=dev)
        assert r.res.n_failed == 0
        if np.isscalar(first) and np.isscalar(counts):  # the same as device arrays
            as_arrays = slice_(ctx, st, None, np.full(st.n, first), np.full(st.n, counts), dev=dev)
            assert as_arrays.res == r.res
    if count == "to_end":
        whole = slice_(ctx, st, None, 0, TO_END, dev=dev)  # the identity: the store itself
        assert np.array_equal(whole.body_index, st.body_index) and np.array_equal(whole.text_index, st.text_index) and np.array_equal(whole.want.data, st.bodies)


def test_first_plus_count_does_not_wrap(ctx):
    st, texts = main_fixture()
    dev = upload(st)
    for first, count in ((5, 0xFFFFFFFA), (5, 0xFFFFFFFB), (0xFFFFFFFF, 0xFFFFFFFF), (1, 0xFFFFFFFF), (300, 0xFFFFFF00)):
        assert first + count >= 0xFFFFFFFF
        r = slice_(ctx, st, None, first, count, dev=dev)
        assert r.want.texts == [t[first:] for t in texts]
        slice_(ctx, st, None, np.full(st.n, first), np.full(st.n, count), dev=dev)


# --- 2. bit phases, record kinds -----------------------------------------------------------------------------------------------------------


def test_every_begin_bit_and_every_bit_count_on_both_paths(ctx):
    st, _ = main_fixture()
    rows, first, count = phase_rows()
    r = slice_(ctx, st, rows, first, count)
    assert r.res.n_failed == 0 and r.res.text_bytes == sum(len(t) for t in r.want.texts)


def test_lane_block_and_threshold_edges(ctx):
    st, texts = main_fixture()
    rows, first, count = triples(edge_rows().values())
    slice_(ctx, st, rows, first, count)
    # what the slice's end reaches, one symbol to either side of the lane's share: 4 * end + 8 bytes
    ends = [(lane_bytes() - 8) // 4 + d for d in (-1, 0, 1)]
    slice_(ctx, st, [13] * 6 + [10] * 3, [0, 0, 0] + [e - 5 for e in ends] + [e - 1 for e in ends], ends + [5] * 3 + [1] * 3)


@pytest.mark.parametrize("text", ["phases", "uniform", "ordered"])
def test_codewords_of_32_bits(ctx, text):
    st = ladder_fixture()
    dev = upload(st)
    if text == "ordered":  # every bit count 0 .. 33 from every symbol of the ladder
        rows, first, count = triples([(0, 33 * k + i, c) for k in (0, 17, 39) for i in range(33) for c in (0, 1, 2)] + [(3, i, c) for i in range(18) for c in (1, 2, 3)])
    else:
        r = 1 if text == "phases" else 2
        n = int(st.text_index[r + 1] - st.text_index[r])
        rng = np.random.default_rng(0x511CE030 + r)
        first = rng.integers(0, n, size=300)
        rows, count = np.full(300, r), np.where(np.arange(300) % 2 == 0, rng.integers(0, 12, size=300), rng.integers(0, 900, size=300))
    slice_(ctx, st, rows, first, count, dev=dev)
    slice_(ctx, st, None, 1, TO_END, dev=dev)


def test_cut_bodies_end_the_slice_where_the_stored_text_ends(ctx):
    st = cut_fixture()
    dev = upload(st)
    stored = [len(stored_text(st, r)) for r in range(st.n)]
    lens = np.diff(st.text_index).astype(np.int64)
    assert all(s < l for s, l in zip(stored, lens))
    for first, count in ((0, TO_END), (1, lens), (np.maximum(np.array(stored) - 3, 0), 9), (np.array(stored), 5), (np.array(stored) + 1, TO_END), (2, 0xFFFFFFF0)):
        r = slice_(ctx, st, None, first, count, dev=dev)
        assert r.res.n_failed == 0
    assert [int(x) for x in np.diff(slice_(ctx, st, None, 0, TO_END, dev=dev).text_index)] == stored


def test_raw_and_empty_records_slice_to_the_empty_record(ctx):
    texts = [corpus.text_like(n, 0x511CE040 + n).tobytes() for n in (50, 0, 70, 60, 0)]
    tab = oracle_table(np.frombuffer(b"".join(texts), np.uint8))
    bodies = [want_encode(tab, t)[1] for t in texts]
    bodies[2] = b""  # no bytes under a length of 70: kept raw elsewhere
    st = make_store(tab, texts, bodies)
    rows = np.array([2, 0, 2, 1, 4, 2, 3, 1])
    for first, count in ((0, TO_END), (3, 20), (0, 0)):
        r = slice_(ctx, st, rows, first, count)
        got = [int(x) for x in np.diff(r.text_index)]
        assert all(got[k] == 0 for k in (0, 2, 3, 4, 5, 7)) and r.res.n_failed == 0  # (the take call keeps a raw record's length; a slice has the symbols its body holds)
    r = slice_(ctx, st, [2, 1, 4, 2], 0, TO_END)
    assert r.res.out_bytes == 0 and r.res.text_bytes == 0 and bool((r.host == SENTINEL).all())


def test_set_pad_bits_of_hand_made_bodies_are_masked_not_copied(ctx):
    st, texts = set_pad_fixture()
    dev, lens = upload(st), np.array([len(t) for t in texts], dtype=np.int64)
    own, _ = main_fixture()
    assert not np.array_equal(st.bodies, own.bodies)
    for first, count in ((0, TO_END), (1, TO_END), (np.maximum(lens - 3, 0), 3), (np.maximum(lens - 1, 0), 9), (2, lens)):
        r = slice_(ctx, st, None, first, count, dev=dev)
    whole = slice_(ctx, st, None, 0, TO_END, dev=dev)
    assert np.array_equal(whole.want.data, own.bodies)  # the encoder's own bodies: the pad is zero again


# --- 3. the stop byte ----------------------------------------------------------------------------------------------------------------------


def test_the_stop_byte_cuts_in_front_of_its_first_occurrence(ctx):
    st, texts = main_fixture()
    dev = upload(st)
    cases = stop_rows()
    rows, first, count = triples(cases.values())
    r = slice_(ctx, st, rows, first, count, stop=ord(" "), dev=dev)
    got = dict(zip(cases, r.want.texts))
    for tag in ("lane", "long"):
        assert got[tag + "_at_first"] == b"" and 0 < len(got[tag + "_inside"]) < 50
        assert len(got[tag + "_behind_count"]) == cases[tag + "_behind_count"][2] and len(got[tag + "_absent"]) == cases[tag + "_absent"][2]
    for stop in (ord(" "), ord("e"), texts[13][0]):
        slice_(ctx, st, None, 0, TO_END, stop=stop, dev=dev)
        slice_(ctx, st, None, 3, 1000, stop=bytes([stop]), dev=dev)


def test_a_stop_byte_in_the_pad_bits_or_without_a_code_cuts_nothing(ctx):
    st, texts = pad_fixture()
    dev = upload(st)
    for stop in (ord("A"), ord("T")):  # what zero pad bits read as; what set pad bits read as
        r = slice_(ctx, st, None, 0, TO_END, stop=stop, dev=dev)
        absent = [k for k, t in enumerate(texts) if bytes([stop]) not in t]
        assert len(absent) >= 6 and all(r.want.texts[k] == texts[k] for k in absent)
        slice_(ctx, st, None, 1, 0xFFFFFFF0, stop=stop, dev=dev)
    assert int(st.tab[1][ord("x")]) == 0
    r = slice_(ctx, st, None, 0, TO_END, stop=ord("x"), dev=dev)
    assert r.want.texts == list(texts) and r.res.status == OK
    main, main_texts = main_fixture()
    assert int(main.tab[1][0xFF]) == 0
    r = slice_(ctx, main, None, 2, 5000, stop=0xFF)
    assert r.want.texts == [t[2:5002] for t in main_texts]


# --- 4. rows and layout --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", SELECTIONS)
def test_rows_in_every_order_and_with_repeats(ctx, name):
    st, _ = main_fixture()
    rows = selection(name, st.n)
    rng = np.random.default_rng(0x511CE050)
    slice_(ctx, st, rows, rng.integers(0, 50, size=rows.size), rng.integers(0, 3000, size=rows.size), stop=ord("."))
    if name == "identity":
        with_rows = slice_(ctx, st, rows, 4, 100)
        without = slice_(ctx, st, None, 4, 100)
        assert without.res == with_rows.res and np.array_equal(without.host[without.at : without.at + without.cap], with_rows.host[with_rows.at : with_rows.at + with_rows.cap])


def test_slices_of_0_to_33_bits_share_destination_words(ctx):
    st = ladder_fixture()
    rng = np.random.default_rng(0x511CE060)
    first = rng.integers(0, 33 * 40 - 2, size=4000)
    count = rng.integers(0, 3, size=4000)
    two = (first % 33 <= 15) | (first % 33 == 32)  # (up to 33 bits: 16 + 17, 32 + 1 at the ladder's wrap; one long codeword else)
    count[~two] = np.minimum(count[~two], 1)
    want = want_slice(st, np.zeros(4000, np.int64), first, count)
    sizes = np.diff(want.body_index)
    assert sizes.max() <= 5 and set(range(6)) == set(int(x) for x in sizes)
    per_word = np.bincount((want.body_index[:-1][sizes > 0] // 16).astype(np.int64))
    assert per_word.max() >= 6  # many rows begin inside one 16-byte destination word
    slice_(ctx, st, np.zeros(4000, np.int64), first, count)
    slice_(ctx, st, np.zeros(3000, np.int64), np.tile([0, 33, 66], 1000), 1)  # one bit each, a byte per row: 16 rows per destination word


@pytest.mark.parametrize("place", ["between", "start", "end"])
@pytest.mark.parametrize("run", [1, 63, 64, 257, 5000])
def test_runs_of_empty_results(ctx, run, place):
    st, texts = main_fixture()
    kinds = [(5, 0, 0), (0, 0, 9), (6, 100, 9), (8, 701, 1)]  # a count of zero, an empty record, first == len, first == len + 1
    empties = [kinds[i % 4] for i in range(run)]
    full = [(9, 3, 700), (13, 2500, 4000)]
    cases = {"between": full[:1] + empties + full[1:], "start": empties + full, "end": full + empties}[place]
    r = slice_(ctx, st, *triples(cases))
    assert r.res.text_bytes == 4700 and int(np.count_nonzero(np.diff(r.body_index))) == 2


@pytest.mark.parametrize("n_rows", [1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_scan_edges(ctx, n_rows):
    st, _ = main_fixture()
    rng = np.random.default_rng(0x511CE070 + n_rows)
    slice_(ctx, st, rng.integers(5, 12, size=n_rows), rng.integers(0, 40, size=n_rows), rng.integers(0, 6, size=n_rows))


@pytest.mark.parametrize("total", [C - 1, C, C + 1, 2 * C + 1])
@pytest.mark.parametrize("tile_off", [0, 5])
def test_totals_at_the_copy_tile_size(ctx, total, tile_off):
    st = bytes_fixture()
    counts = np.array([997] * (total // 997) + [total % 997])
    for record in (0, 1):  # bytes that begin at bit 7 of a source byte; whole bytes
        r = slice_(ctx, st, np.full(counts.size, record), 1 + np.arange(counts.size) * 13, counts, tile_off=tile_off)
        assert r.res.out_bytes == total and r.d_out.data_ptr() % C == tile_off


def test_a_slice_across_a_copy_tile_boundary_from_every_offset(ctx):
    st = bytes_fixture()
    dev = upload(st)
    for before in range(17):  # the crossing slice begins `before` bytes in front of the boundary
        r = slice_(ctx, st, [0, 0, 1], [1, 50, 7], [C - before, 100, 40], dev=dev, tile_off=0)
        assert int(r.body_index[1]) == C - before
        slice_(ctx, st, [1, 0, 0, 0], [0, 3, 9, 9], [40, C - before, 100, 100], dev=dev, tile_off=C - 40)


@pytest.mark.parametrize("shift", range(16))
def test_every_output_base_and_body_alignment(ctx, shift):
    import torch

    st, _ = main_fixture()
    lead = shift  # d_bodies at every alignment of 16, and with it every body
    d = torch.full((lead + st.bodies.size + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
    d[lead : lead + st.bodies.size] = torch.from_numpy(st.bodies).cuda()
    dev = (d[lead : lead + st.bodies.size], _dev_index(st.body_index), _dev_index(st.text_index))
    assert d.data_ptr() % 16 == 0 and dev[0].data_ptr() % 16 == lead
    rng = np.random.default_rng(0x511CE080 + shift)
    rows = rng.integers(0, st.n, size=300)
    r = slice_(ctx, st, rows, rng.integers(0, 60, size=300), np.where(rng.integers(0, 2, size=300) == 0, rng.integers(0, 9, size=300), rng.integers(0, 2000, size=300)), dev=dev,
               shift=shift)
    assert r.d_out.data_ptr() % 16 == shift
    slice_(ctx, st, [13, 0, 2, 13], [1, 0, 1, 30000], [TO_END, 5, 1, TO_END], dev=dev, shift=shift)


# --- 5. the call's own behaviour ------------------------------------------------------------------------------------------------------------


def test_failures_stay_local(ctx):
    st, bad = failures_store()  # random bytes: under table_255 every byte string is a text
    st.tab = table_255()
    st.cb = _cb(st.tab)
    dev = upload(st, spare=4096)
    rows = np.array([0, 16, 1, 3, 2, 0xFFFFFFFF, 8, 4, 15, 9, 5, 11, 6, 14, 12, 13, 7, 10, 3, 0], dtype=np.uint32)
    want = want_slice(st, rows, 2, 100)
    assert [int(s) for s in want.status] == [bad.get(int(r), OK) if r < 16 else ARG for r in rows]
    r = check_take(run_slice(ctx, st, dev, rows, 2, 100, None, want.total), want)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (9, 1, ARG)
    for k in np.flatnonzero(want.status):  # a failed row is an empty record
        assert r.body_index[k] == r.body_index[k + 1] and r.text_index[k] == r.text_index[k + 1]
    r = slice_(ctx, st, np.array([0, 1, 2, 15, 9, 3], dtype=np.uint32), 0, TO_END, dev=dev)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 3, UNSUPPORTED)
    r = slice_(ctx, st, np.array([13, 0, 1, 2, 4, 5, 6, 7, 10, 12, 13], dtype=np.uint32), 1, 77, stop=9, dev=dev)  # a bad record that no row selects does not matter
    assert r.res.n_failed == 0 and not r.status.any()
    want = want_slice(st, None, 0, 50)  # d_rows == NULL: every record, the bad ones among them
    r = check_take(run_slice(ctx, st, dev, None, 0, 50, None, want.total), want)
    assert r.res.n_failed == len(bad)


def test_capacity_and_sizes_only(ctx):
    st, _ = main_fixture()
    rng = np.random.default_rng(0x511CE090)
    rows = np.concatenate((rng.integers(0, st.n, size=400), [st.n + 5, 0]))  # (one row fails: d_status is complete either way)
    first, count = rng.integers(0, 30, size=402), rng.integers(0, 500, size=402)
    dev = upload(st)
    want = want_slice(st, rows, first, count, ord(","))
    args = (ctx, st, dev, rows, first, count, ord(","))
    exact = check_take(run_slice(*args, want.total), want)
    assert exact.res.n_failed == 1
    check_take(run_slice(*args, want.total - 1), want, call_status=CAP)
    check_take(run_slice(*args, 1), want, call_status=CAP)
    sizes_only = check_take(run_slice(*args, want.total, sizes_only=True), want)
    assert sizes_only.res == exact.res
    check_take(run_slice(*args, want.total + 1000), want)  # the ctx is as good as before; room to spare stays untouched


def _raw_call(ctx, st, dev, n_rows, d_rows, d_out, d_a, d_b, res, cb=None, stop=NO_STOP, **ptr):
    """One call through the C ABI; ptr: p_rows, p_first, p_count, p_out -- addresses (or None) in place of those arrays -- and cap."""
    from entreepy_amd import _native as N

    d_bodies, d_body_index, d_text_index = dev
    return N.lib().et_slice_packed_device(ctx._h, ctypes.byref((cb or st.cb).raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n,
                                          ptr.get("p_rows", d_rows.data_ptr()), n_rows, ptr.get("p_first"), 0, ptr.get("p_count"), TO_END, stop, ptr.get("p_out", d_out.data_ptr()),
                                          ptr.get("cap", d_out.numel()), d_a.data_ptr(), d_b.data_ptr(), None, ctypes.byref(res))


def test_no_rows_an_incomplete_table_and_a_bad_stop_enqueue_nothing(ctx):
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    st, _ = main_fixture()
    dev = upload(st)
    d_rows = dev_rows([1, 2])
    d_out = torch.full((4000,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_a, d_b = (torch.full((3,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    fresh = lambda: N.TakeResult(out_bytes=99, text_bytes=98, n_failed=97, first_failed=96, first_status=95)  # noqa: E731
    res = fresh()
    assert _raw_call(ctx, st, dev, 0, d_rows, d_out, d_a, d_b, res) == OK
    assert (res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (0, 0, 0, 0, 0)
    data, length = (a.copy() for a in st.tab)
    length[int(np.flatnonzero(length)[0])] = 0  # a hole in the tree
    res = fresh()
    assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, cb=E.Codebook.from_tables(data, length)) == UNSUPPORTED
    for stop in (-2, 256, 1 << 20):
        res = fresh()
        assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, stop=stop) == ARG
        assert (res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (99, 98, 97, 96, 95), "*res was touched"
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_a == -1).all()) and bool((d_b == -1).all()), "something was enqueued"
    res = fresh()
    assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res) == OK  # the ctx is as good as before
    torch.cuda.synchronize()
    want = want_slice(st, [1, 2], 0, TO_END)
    assert res.out_bytes == want.total and d_out[: want.total].cpu().numpy().tobytes() == want.data.tobytes() and bool((d_out[want.total :] == SENTINEL).all())


def test_call_level_argument_errors_on_a_live_context(ctx):
    """The checks that come before anything touches a device, with a context that could go on: ET_ERR_ARG, *res untouched, nothing
    enqueued -- every output and the bodies hold what they held."""
    import torch

    from entreepy_amd import _native as N

    st, _ = main_fixture()
    dev = upload(st)
    before = dev[0].clone()
    d_rows, d_u32 = dev_rows([1, 2]), dev_rows([0, 0, 0])
    d_out = torch.full((4000,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_a, d_b = (torch.full((3,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    inside = dev[0].data_ptr() + 8
    cases = {"a misaligned d_first": dict(p_first=d_u32.data_ptr() + 1), "a misaligned d_count": dict(p_count=d_u32.data_ptr() + 2), "misaligned d_rows": dict(p_rows=d_rows.data_ptr() + 3),
             "d_out inside d_bodies": dict(p_out=inside, cap=16), "d_out around d_bodies' end": dict(p_out=dev[0].data_ptr() + dev[0].numel() - 1, cap=64),
             "no d_rows, and n_rows is not n_records": dict(p_rows=None)}
    for what, ptr in cases.items():
        res = N.TakeResult(out_bytes=99, text_bytes=98, n_failed=97, first_failed=96, first_status=95)
        assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, **ptr) == ARG, what
        assert (res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (99, 98, 97, 96, 95), f"{what}: *res was touched"
    res = N.TakeResult(out_bytes=99)
    assert _raw_call(ctx, st, dev, 0x80000000, d_rows, d_out, d_a, d_b, res) == ARG and res.out_bytes == 99
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_a == -1).all()) and bool((d_b == -1).all()) and torch.equal(dev[0], before), "something was enqueued"
    want = want_slice(st, [1, 2], 0, TO_END)  # the same arguments, well-formed: the aligned d_first and d_count are accepted, the ctx is as good as before
    res, d_to_end = N.TakeResult(), dev_rows([TO_END, TO_END])
    assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, p_first=d_u32.data_ptr(), p_count=d_to_end.data_ptr()) == OK
    torch.cuda.synchronize()
    assert res.out_bytes == want.total and d_out[: want.total].cpu().numpy().tobytes() == want.data.tobytes() and bool((d_out[want.total :] == SENTINEL).all())


def test_offsets_above_4_gib(ctx):
    import torch

    page_len, few = 256 << 10, 5
    text = corpus.text_like(page_len, 0x511CE0A0)
    tab = oracle_table(text)
    cb = _cb(tab)
    body = np.frombuffer(want_encode(tab, text)[1], np.uint8)
    first = next(i for i in range(1, 50) if int(tab[1][text[:i]].sum()) % 8)  # the slice begins inside a source byte
    piece = np.frombuffer(want_encode(tab, text[first:])[1], np.uint8)  # what every long row becomes
    small = np.frombuffer(want_encode(tab, text[first : first + 9])[1], np.uint8)
    L, P = body.size, piece.size
    assert page_len <= _small_max()
    d_body, d_piece = torch.from_numpy(body.copy()).cuda(), torch.from_numpy(piece.copy()).cuda()
    # output: the slice of one record n_pages times behind one row of a few bytes, so that a row straddles 2^32
    n_pages = (1 << 32) // P + 3
    total = small.size + n_pages * P
    n_rows = n_pages + 1
    d_count = torch.full((n_rows,), -1, dtype=torch.int32, device="cuda")  # ET_SLICE_TO_END
    d_count[0] = 9
    d_raw = torch.full((LEAD + total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((n_rows + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_status = torch.full((n_rows,), 0xEE, dtype=torch.uint8, device="cuda")
    res = ctx.slice_packed_device(cb, d_body, _dev_index([0, L]), _dev_index([0, page_len]), torch.zeros(n_rows, dtype=torch.int32, device="cuda"), first, d_count,
                                  d_raw[LEAD : LEAD + total], d_bi, d_ti, status=d_status)
    torch.cuda.synchronize()
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed) == (OK, total, 9 + n_pages * (page_len - first), 0)
    steps = torch.arange(n_rows + 1, dtype=torch.int64, device="cuda")
    want_bi, want_ti = steps * P + (small.size - P), steps * (page_len - first) + (9 - (page_len - first))
    want_bi[0] = want_ti[0] = 0
    assert torch.equal(d_bi, want_bi) and torch.equal(d_ti, want_ti) and not bool(d_status.any())
    assert total > 1 << 32
    d_out = d_raw[LEAD : LEAD + total]
    assert d_out[: small.size].cpu().numpy().tobytes() == small.tobytes()
    assert torch.equal(d_out[small.size :].view(n_pages, P), d_piece.unsqueeze(0).expand(n_pages, P)), "a row differs from the oracle's encode of the slice"
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
    res = ctx.slice_packed_device(cb, d_bodies[: far + L], _dev_index([0, L, far, far + L]), _dev_index([0, page_len, page_len, 2 * page_len]), dev_rows([2, 1, 0, 2]), first, TO_END,
                                  d_raw[LEAD : LEAD + 3 * P], d_bi, d_ti, status=d_status)
    torch.cuda.synchronize()
    # (record 1's body of 2^32 + 37 - L zeros is above 4 * small_max: that row fails alone)
    n = page_len - first
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (OK, 3 * P, 3 * n, 1, 1, UNSUPPORTED)
    assert d_bi.tolist() == [0, P, P, 2 * P, 3 * P] and d_ti.tolist() == [0, n, n, 2 * n, 3 * n] and d_status.tolist() == [OK, UNSUPPORTED, OK, OK]
    assert torch.equal(d_raw[LEAD : LEAD + 3 * P].view(3, P), d_piece.unsqueeze(0).expand(3, P))
    assert bool((d_raw[:LEAD] == SENTINEL).all()) and bool((d_raw[LEAD + 3 * P :] == SENTINEL).all())


# --- 6. composition -------------------------------------------------------------------------------------------------------------------------


def test_search_slice_join_gather_on_one_context(ctx):
    """encode_packed of log lines and of a key set -> search(b"user=") -> d_first = d_pos + 5 on the device -> slice up to the next ';'
    -> join against the keys -> gather: nothing is synchronised in between, and text appears at the very end only."""
    import torch

    import entreepy_amd as E

    rng = np.random.default_rng(0x511CE0B0)
    users = [b"u%03d" % i + bytes(rng.choice(np.frombuffer(b"abc", np.uint8), size=int(rng.integers(0, 4))).tobytes()) for i in range(300)]
    lines = []
    for i in range(2000):
        who = users[int(rng.integers(0, 300))]
        kind = i % 5
        lines.append({0: b"ts=%d;user=" % i + who + b";ok", 1: b"user=" + who, 2: b"host=h%d;lvl=3" % i, 3: b"a=1;user=" + who + b";user=zzz;", 4: b"x;user=;y"}[kind])
    keys = users[::3]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(lines + users), np.uint8), minlength=256))
    sides = []
    for column in (keys, lines):
        index = _index_of([len(w) for w in column])
        d_text, d_index = _dev_bytes(np.frombuffer(b"".join(column), np.uint8)), _dev_index(index)
        d_out = torch.empty(cb.body_bound(int(index[-1])) + len(column), dtype=torch.uint8, device="cuda")
        sides.append((d_out, torch.empty(len(column) + 1, dtype=torch.int64, device="cuda"), d_index, d_text))
    n = len(lines)
    d_rows, d_pos, d_hits, d_key = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(4))
    d_raw = torch.full((LEAD + 16 * n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ids, d_bi, d_ti = d_raw[LEAD:], torch.full((n + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_texts = torch.full((16 * n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_texts_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    enc = [ctx.encode_packed_device(cb, s[3], s[2], s[0], s[1]) for s in sides]
    key_store, line_store = ((s[0][: e.out_bytes], s[1], s[2]) for s, e in zip(sides, enc))
    m = ctx.search_packed_device(cb, *line_store, b"user=", E.SEARCH_CONTAINS, rows=d_rows, pos=d_pos)
    d_first = d_pos[: m.n_match] + 5
    s = ctx.slice_packed_device(cb, *line_store, d_rows[: m.n_match], d_first, E.SLICE_TO_END, d_ids[: 16 * n], d_bi[: m.n_match + 1], d_ti[: m.n_match + 1], stop=b";")
    ids = (d_ids[: max(s.out_bytes, 1)], d_bi[: m.n_match + 1], d_ti[: m.n_match + 1])
    j = ctx.join_packed_device(cb, *ids, *key_store, rows=d_hits, key_of_row=d_key)
    g = ctx.decode_packed_gather_device(cb, *ids, d_hits[: j.n_match], d_texts[: 16 * n], d_texts_index[: j.n_match + 1])
    torch.cuda.synchronize()
    # the same pipeline in Python
    found = [(i, l.find(b"user=")) for i, l in enumerate(lines) if b"user=" in l]
    cut = [lines[i][p + 5 :].split(b";")[0] for i, p in found]
    hits = [k for k, c in enumerate(cut) if c in set(keys)]
    assert 0 < len(hits) < len(found) < n and b"" in cut
    assert all(e.status == OK and e.n_failed == 0 for e in enc) and (m.status, m.n_match, m.n_failed) == (OK, len(found), 0)
    assert (s.status, s.n_failed, s.text_bytes) == (OK, 0, sum(len(c) for c in cut)) and _guards_intact(d_ids, s.out_bytes)
    assert np.diff(d_ti[: m.n_match + 1].cpu().numpy()).tolist() == [len(c) for c in cut]
    want_ids = b"".join(want_encode(_tables_of(cb), c)[1] for c in cut)
    assert d_ids[: s.out_bytes].cpu().numpy().tobytes() == want_ids
    assert (j.status, j.n_failed, j.n_keys_failed) == (OK, 0, 0) and d_hits[: j.n_match].tolist() == hits
    assert d_key[: j.n_match].tolist() == [keys.index(cut[k]) for k in hits]
    assert (g.status, g.n_failed, g.n_short) == (OK, 0, 0) and d_texts[: g.out_bytes].cpu().numpy().tobytes() == b"".join(cut[k] for k in hits)


def _tables_of(cb):
    return np.array(cb.raw.data, dtype=np.uint32), np.array(cb.raw.length, dtype=np.uint8)


def test_single_stream_calls_before_and_after_a_slice(ctx):
    """et_encode_device, a slice, et_decode_device on one ctx with no synchronisation in between."""
    import torch

    import entreepy_amd as E

    st, _ = main_fixture()
    rows, first, count = phase_rows()
    want = want_slice(st, rows, first, count)
    big = corpus.text_like(300_000, 0x511CE0C0)
    image = np.frombuffer(_oracle().encode(big), np.uint8)
    d_big = torch.from_numpy(big.copy()).cuda()
    d_image = torch.full((E.encode_bound(big.size) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_back = torch.full((big.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    dev, d_rows, d_first, d_count = upload(st), dev_rows(rows), dev_rows(first), dev_rows(count)
    d_raw = torch.full((LEAD + want.total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((rows.size + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    n_image = ctx.encode_device(d_big, d_image[: d_image.numel() - TAIL])
    res = ctx.slice_packed_device(st.cb, *dev, d_rows, d_first, d_count, d_raw[LEAD : LEAD + want.total], d_bi, d_ti)
    n_back = ctx.decode_device(d_image[:n_image], d_back[: big.size], skip=4)
    torch.cuda.synchronize()
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed) == (OK, want.total, want.text_total, 0)
    host = d_raw.cpu().numpy()
    assert np.array_equal(host[LEAD : LEAD + want.total], want.data) and bool((host[:LEAD] == SENTINEL).all()) and bool((host[LEAD + want.total :] == SENTINEL).all())
    assert np.array_equal(d_bi.cpu().numpy().view(np.uint64), want.body_index) and np.array_equal(d_ti.cpu().numpy().view(np.uint64), want.text_index)
    assert n_image == image.size and d_image[:n_image].cpu().numpy().tobytes() == image.tobytes()
    assert n_back == big.size and d_back[: big.size].cpu().numpy().tobytes() == big.tobytes() and bool((d_back[big.size :] == SENTINEL).all())


def test_list_helper_returns_a_store_of_the_slices(ctx):
    import entreepy_amd as E

    _, texts = main_fixture()
    texts = texts[:30]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(texts), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, texts)
    lengths = [len(t) for t in texts]
    rng = np.random.default_rng(0x511CE0D0)
    rows = np.concatenate((rng.integers(0, 30, size=80), [0, 0, 29, 4]))
    first, count = rng.integers(0, 60, size=rows.size), rng.integers(0, 900, size=rows.size)
    for f, c, stop in ((first, count, None), (2, 40, None), (first, E.SLICE_TO_END, b" "), (0, count, ord("e"))):
        new_blob, new_index, new_lengths = ctx.slice_packed(cb, blob, out_index, lengths, rows, f, c, stop=stop)
        want = [py_slice(texts[r], ff, cc, stop if stop is None or isinstance(stop, int) else stop[0]) for r, ff, cc in zip(rows, per_row(f, rows.size), per_row(c, rows.size))]
        assert [int(x) for x in new_lengths] == [len(w) for w in want]
        assert (new_blob, new_index.tolist()) == (lambda b, i: (b, i.tolist()))(*ctx.encode_packed(cb, want))
        assert ctx.decode_packed(cb, new_blob, new_index, new_lengths) == want
    assert ctx.slice_packed(cb, blob, out_index, lengths, [], 0, 5)[0] == b""
    with pytest.raises(E.EntreepyError, match="row 1") as e:
        ctx.slice_packed(cb, blob, out_index, lengths, [3, 30, 4], 0, 5)
    assert e.value.status == ARG


# --- 7. the state a context keeps between calls ---------------------------------------------------------------------------------------------
# The cells of tests/test_gpu_retained.py for the row `slice` (tests/retained_slice.py): a slice between the call that sets a state and
# the calls that read it leaves the histogram link, the held range and the last codebook as they were.


@pytest.mark.parametrize("reader", ["body", "head", "on_host"])
def test_histogram_link_survives_a_slice(reader):
    from tests import test_gpu_retained as G

    G.test_histogram_link("slice", reader)


@pytest.mark.parametrize("how", ["sync", "maps", "between", "windows"])
def test_held_range_survives_a_slice(how):
    from tests import test_gpu_retained as G

    G.test_held_range("slice", how)


def test_last_codebook_survives_a_slice():
    from tests import test_gpu_retained as G

    G.test_last_codebook("slice")
