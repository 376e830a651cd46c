"""GPU: et_take_packed_device -- a selection of a packed store's records as a new packed store, bodies copied as they are -- against
numpy: row k's bytes are the slice of the source blob its record's pair names, both output indexes are cumulative sums (model()),
and for the round trips the oracle's texts.  d_out lies between sentinel bytes (LEAD in front, TAIL behind the capacity); in every
test the bytes in front of d_out and behind out_body_index[n_rows] must still hold them afterwards."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus
from tests.test_gpu_batch import SENTINEL, _oracle, _small_max
from tests.test_gpu_gather import dev_rows, make_store, upload
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_shared_host import oracle_table

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
SCAN_TILE = 4096  # rows per trip of k_take_scan's one workgroup (csrc/et_batch.h TAKE_SCAN_TILE)
C = 8192  # bytes of output per tile of k_take_copy (csrc/et_batch.h TAKE_TILE_BYTES)
LEAD = 16  # sentinel bytes in front of d_out, at least


# --- the fixtures (tests/test_take_host.py runs model() on them without a GPU) ---------------------------------------------------------


def raw_store(body_sizes, lengths=None, seed=0x7A4E0001):
    """A store whose bodies are random bytes: the call interprets none of them.  lengths: the records' text lengths (default: the body
    sizes, which a table of 8-bit codes would give)."""
    sizes = np.asarray(body_sizes, dtype=np.uint64)
    blob = np.random.default_rng(seed).integers(0, 256, size=int(sizes.sum()), dtype=np.uint8)
    return SimpleNamespace(bodies=blob, body_index=_index_of(sizes), text_index=_index_of(sizes if lengths is None else lengths), n=sizes.size)


def model(st, rows):
    """numpy's take: per row its status by the header's rule, then slice, concatenate, two cumulative sums."""
    small, body_bytes = _small_max(), st.bodies.size
    rows = np.asarray(rows, dtype=np.int64)
    status, nb, ln, pieces = np.full(rows.size, ARG, np.uint8), np.zeros(rows.size, np.uint64), np.zeros(rows.size, np.uint64), []
    for k, r in enumerate(rows):
        if r >= st.n:
            continue
        b0, b1, t0, t1 = (int(x) for x in (st.body_index[r], st.body_index[r + 1], st.text_index[r], st.text_index[r + 1]))
        if not (b0 <= b1 <= body_bytes and t0 <= t1):
            continue
        if t1 - t0 > small or b1 - b0 > 4 * small:
            status[k] = UNSUPPORTED
            continue
        status[k], nb[k], ln[k] = OK, b1 - b0, t1 - t0
        pieces.append(st.bodies[b0:b1])
    data = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    return SimpleNamespace(status=status, body_index=_index_of(nb), text_index=_index_of(ln), data=data, total=int(nb.sum()), text_total=int(ln.sum()))


@functools.lru_cache(maxsize=None)
def mixed_store():
    """About 300 records under the table of their own text, lengths 0 .. 5 000 with 0 and 1 among them -> (store, [texts])."""
    rng = np.random.default_rng(0x7A4E0010)
    sizes = rng.integers(0, 5001, size=300)
    sizes[:6] = [0, 1, 2, 3, 0, 5000]
    pool = corpus.text_like(int(sizes.sum()), 0x7A4E0011)
    cuts = _index_of(sizes)
    texts = [pool[int(cuts[i]) : int(cuts[i + 1])].tobytes() for i in range(300)]
    return make_store(oracle_table(pool), texts), texts


def selection(name, n):
    rng = np.random.default_rng(0x7A4E0012)
    return {"identity": lambda: np.arange(n), "reversed": lambda: np.arange(n)[::-1], "permutation": lambda: rng.permutation(n),
            "random_tenth": lambda: np.sort(rng.choice(n, size=n // 10, replace=False)), "one_record_500_times": lambda: np.full(500, 17),
            "neighbours_doubled": lambda: np.repeat(rng.permutation(n)[:150], 2)}[name]()


SELECTIONS = ["identity", "reversed", "permutation", "random_tenth", "one_record_500_times", "neighbours_doubled"]
SMALL_SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 33]


@functools.lru_cache(maxsize=None)
def small_store():
    """Bodies of 0, 1, 7, 8, 9, 15, 16, 17 and 33 bytes, 40 of each, shuffled; a length that is not the body size."""
    sizes = np.random.default_rng(0x7A4E0020).permutation(np.repeat(SMALL_SIZES, 40))
    return raw_store(sizes, lengths=sizes * 2 + 1, seed=0x7A4E0021)


@functools.lru_cache(maxsize=None)
def empties_store():
    """Record 0: no bytes, length 0; 1 and 2: bodies of 50 and 70 bytes; 3: no bytes under a length of 9 (kept raw elsewhere)."""
    return raw_store([0, 50, 70, 0], lengths=[0, 60, 80, 9], seed=0x7A4E0030)


def empty_run_rows(run, place):
    run_rows = np.where(np.arange(run) % 3 == 2, 3, 0)  # both kinds of empty row
    return {"between": np.concatenate(([1], run_rows, [2])), "start": np.concatenate((run_rows, [1, 2])), "end": np.concatenate(([1, 2], run_rows))}[place]


# --- one call and its check ---------------------------------------------------------------------------------------------------------------


def run_take(ctx, st, dev, rows, cap, sizes_only=False, shift=0, tile_off=None):
    """One call, every output full of sentinels first.  d_out begins `shift` bytes behind a 16-byte aligned address -- or, with
    tile_off, that many bytes behind a multiple of C."""
    import torch

    d_bodies, d_body_index, d_text_index = dev
    n = len(rows)
    r = SimpleNamespace(cap=cap, sizes_only=sizes_only)
    r.d_raw = torch.full((3 * C + LEAD + 16 + cap + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert r.d_raw.data_ptr() % 16 == 0
    r.at = LEAD + shift if tile_off is None else (-r.d_raw.data_ptr()) % C + C + tile_off
    r.d_out = r.d_raw[r.at : r.at + max(cap, 1)]  # (an empty tensor has no address: rows that need no room get a byte)
    r.d_body_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_text_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.res = ctx.take_packed_device(d_bodies, d_body_index, d_text_index, dev_rows(rows), None if sizes_only else r.d_out, r.d_body_index, r.d_text_index, r.d_status)
    torch.cuda.synchronize()
    r.host = r.d_raw.cpu().numpy()
    r.body_index, r.text_index = r.d_body_index.cpu().numpy().view(np.uint64), r.d_text_index.cpu().numpy().view(np.uint64)
    r.status = r.d_status.cpu().numpy()
    return r


def check_take(r, want, call_status=OK):
    assert np.array_equal(r.body_index, want.body_index), f"out_body_index differs from the cumulative sum, first at {int(np.flatnonzero(r.body_index != want.body_index)[0])}"
    assert np.array_equal(r.text_index, want.text_index), f"out_text_index differs from the cumulative sum, first at {int(np.flatnonzero(r.text_index != want.text_index)[0])}"
    assert np.array_equal(r.status, want.status)
    failed = np.flatnonzero(want.status)
    assert (r.res.status, r.res.out_bytes, r.res.text_bytes, r.res.n_failed) == (call_status, want.total, want.text_total, failed.size), r.res
    if failed.size:
        assert (r.res.first_failed, r.res.first_status) == (int(failed[0]), int(want.status[failed[0]])), r.res
    written = not r.sizes_only and call_status == OK
    got = r.host[r.at : r.at + want.total] if written else r.host[:0]
    bad = np.flatnonzero(got != want.data[: got.size])
    assert bad.size == 0, f"the taken bytes differ from the source's, first at {int(bad[0])} of {want.total}"
    assert bool((r.host[: r.at] == SENTINEL).all()), "a byte in front of d_out was written"
    behind = r.at + (want.total if written else 0)
    bad = np.flatnonzero(r.host[behind:] != SENTINEL)
    assert bad.size == 0, f"a byte at or behind d_out + out_body_index[n_rows] was written, the first {int(bad[0])} bytes behind it"
    return r


def take(ctx, st, rows, dev=None, **kw):
    """Run with cap = the need exactly, and check."""
    want = model(st, rows)
    return check_take(run_take(ctx, st, dev or upload(st), rows, want.total, **kw), want)


# --- 1. selections, scan edges ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", SELECTIONS)
def test_selections(ctx, name):
    st, _ = mixed_store()
    r = take(ctx, st, selection(name, st.n))
    assert r.res.n_failed == 0
    if name == "identity":
        assert np.array_equal(r.body_index, st.body_index) and np.array_equal(r.text_index, st.text_index)


@pytest.mark.parametrize("n_rows", [1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_scan_edges(ctx, n_rows):
    st = small_store()
    rows = np.random.default_rng(0x7A4E0040 + n_rows).integers(0, st.n, size=n_rows)
    rows[0] = int(np.flatnonzero(np.diff(st.body_index) == 33)[0])
    take(ctx, st, rows)


# --- 2. copy-tile edges -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("total", [C - 1, C, C + 1, 2 * C + 1])
@pytest.mark.parametrize("tile_off", [0, 5])
def test_totals_at_the_tile_size(ctx, total, tile_off):
    sizes = [997] * (total // 997) + [total % 997]
    st = raw_store(sizes, seed=0x7A4E0050 + total)
    r = take(ctx, st, np.arange(st.n)[::-1], tile_off=tile_off)
    assert r.res.out_bytes == total and r.d_out.data_ptr() % C == tile_off


def test_a_body_across_a_tile_boundary_from_every_offset(ctx):
    for before in range(17):  # the crossing body begins `before` bytes in front of the boundary
        st = raw_store([C - before, 100, 40], seed=0x7A4E0060 + before)
        dev = upload(st)
        r = take(ctx, st, [0, 1, 2], dev=dev, tile_off=0)
        assert int(r.body_index[1]) == C - before
        take(ctx, st, [2, 0, 1, 1], dev=dev, tile_off=C - 40)  # ... and with the tile's start inside a body


def test_a_body_longer_than_two_tiles_and_a_single_byte(ctx):
    st = raw_store([3, 2 * C + 501, 1, 4 * C], lengths=[3, 9000, 1, 70000], seed=0x7A4E0070)
    dev = upload(st)
    take(ctx, st, [0, 1, 0, 3, 1], dev=dev, shift=3)
    take(ctx, st, [1], dev=dev, tile_off=C - 7)
    for shift in (0, 9, 15):  # the smallest total of all
        r = take(ctx, st, [2], dev=dev, shift=shift)
        assert r.res.out_bytes == 1 and r.res.text_bytes == 1


# --- 3. small bodies, empty rows ----------------------------------------------------------------------------------------------------------


def test_small_bodies_share_destination_words(ctx):
    st = small_store()
    rows = np.random.default_rng(0x7A4E0080).integers(0, st.n, size=3000)
    want = model(st, rows)
    per_word = np.bincount((want.body_index[:-1][np.diff(want.body_index) > 0] // 16).astype(np.int64))
    assert per_word.max() >= 4  # several rows begin inside one 16-byte destination word
    take(ctx, st, rows)
    ones = np.flatnonzero(np.diff(st.body_index) == 1)
    take(ctx, st, np.tile(ones, 5))  # 16 rows per word


@pytest.mark.parametrize("place", ["between", "start", "end"])
@pytest.mark.parametrize("run", [1, 63, 64, 257, 5000])
def test_runs_of_empty_rows(ctx, run, place):
    st = empties_store()
    r = take(ctx, st, empty_run_rows(run, place))
    assert r.res.out_bytes == 120 and r.res.text_bytes == 140 + 9 * (run // 3)


def test_a_selection_of_empty_rows_only_writes_nothing(ctx):
    st = empties_store()
    r = take(ctx, st, [0, 3, 0, 0, 3] * 100)
    assert r.res.out_bytes == 0 and r.res.text_bytes == 9 * 200 and bool((r.host == SENTINEL).all())


# --- 4. alignment and write extent --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shift", range(16))
def test_every_output_base_and_body_alignment(ctx, shift):
    import torch

    st = small_store()
    lead = shift % 8  # d_bodies at alignments 0 .. 7
    d = torch.zeros(lead + st.bodies.size + 1, dtype=torch.uint8, device="cuda")
    d[lead : lead + st.bodies.size] = torch.from_numpy(st.bodies).cuda()
    dev = (d[lead : lead + st.bodies.size], _dev_index(st.body_index), _dev_index(st.text_index))
    assert dev[0].data_ptr() % 8 == lead
    r = take(ctx, st, np.random.default_rng(0x7A4E0090 + shift).integers(0, st.n, size=700), dev=dev, shift=shift)
    assert r.d_out.data_ptr() % 16 == shift
    big = raw_store([5000, 1, 9000], seed=0x7A4E0091)
    take(ctx, big, [2, 0, 1, 2], shift=shift)


# --- 5. failures stay local ---------------------------------------------------------------------------------------------------------------


def failures_store():
    """14 records of random bytes, four of them spoilt as tests/test_gpu_gather.py spoils them; record 14: a length above the small-stream
    limit; record 15: a body above 4 * small_max -- over zeros, which nothing reads.  -> (store, the bad records)."""
    small = _small_max()
    st = raw_store([150, 140, 1, 130, 166, 0, 145, 155, 152, 135, 149, 144, 150, 138], seed=0x7A4E00A0)
    good = int(st.bodies.size)
    st.bodies = np.concatenate((st.bodies, np.zeros(10 + 4 * small + 1, np.uint8)))
    st.body_index = np.concatenate((st.body_index, np.array([good + 10, good + 10 + 4 * small + 1], np.uint64)))
    st.text_index = np.concatenate((st.text_index, st.text_index[-1] + np.array([small + 1, small + 101], np.uint64)))
    st.n = 16
    st.body_index[4] = st.body_index[3] - np.uint64(5)  # a decreasing body pair: record 3 fails; record 4's body begins 5 bytes early
    st.body_index[9] = np.uint64(st.bodies.size + 77)  # a body pair beyond body_bytes: records 8 and 9 fail
    st.text_index[12] = st.text_index[11] - np.uint64(3)  # a decreasing text pair: record 11 fails; record 12 is 3 longer
    return st, {3: ARG, 8: ARG, 9: ARG, 11: ARG, 14: UNSUPPORTED, 15: UNSUPPORTED}


def test_failures_stay_local(ctx):
    st, bad = failures_store()
    dev = upload(st, spare=4096)  # (what lies behind body_bytes is mapped: a pair that is followed shows as wrong bytes)
    rows = np.array([0, 16, 1, 3, 2, 0xFFFFFFFF, 8, 4, 15, 9, 5, 11, 6, 14, 12, 13, 7, 10, 3, 0], dtype=np.uint32)
    want = model(st, rows)
    assert [int(s) for s in want.status] == [bad.get(int(r), OK) if r < 16 else ARG for r in rows]
    r = check_take(run_take(ctx, st, dev, rows, want.total), want)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (9, 1, ARG)
    for k in np.flatnonzero(want.status):  # a failed row is an empty record
        assert r.body_index[k] == r.body_index[k + 1] and r.text_index[k] == r.text_index[k + 1]
    r = take(ctx, st, np.array([0, 1, 2, 15, 9, 3], dtype=np.uint32), dev=dev)  # the lowest failing row is not the first failing record
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 3, UNSUPPORTED)
    r = take(ctx, st, np.array([13, 0, 1, 2, 4, 5, 6, 7, 10, 12, 13], dtype=np.uint32), dev=dev)  # a bad record that no row selects does not matter
    assert r.res.n_failed == 0 and not r.status.any()


# --- 6. capacity, sizes only, no rows -----------------------------------------------------------------------------------------------------


def test_capacity_and_sizes_only(ctx):
    st, _ = mixed_store()
    rows = np.concatenate((np.random.default_rng(0x7A4E00B0).integers(0, st.n, size=400), [st.n + 5, 0]))  # (one row fails: d_status is complete either way)
    dev = upload(st)
    want = model(st, rows)
    exact = check_take(run_take(ctx, st, dev, rows, want.total), want)
    assert exact.res.n_failed == 1
    check_take(run_take(ctx, st, dev, rows, want.total - 1), want, call_status=CAP)
    check_take(run_take(ctx, st, dev, rows, 1), want, call_status=CAP)
    sizes_only = check_take(run_take(ctx, st, dev, rows, want.total, sizes_only=True), want)
    assert sizes_only.res == exact.res
    check_take(run_take(ctx, st, dev, rows, want.total + 1000), want)  # the ctx is as good as before; room to spare stays untouched


def test_no_rows_is_ok_and_zeroes_the_result(ctx):
    import torch

    from entreepy_amd import _native as N

    st = small_store()
    d_bodies, d_body_index, d_text_index = upload(st)
    d_rows = dev_rows([1, 2])
    d_out = torch.full((200,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_a, d_b = (torch.full((3,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    res = N.TakeResult(out_bytes=99, text_bytes=98, n_failed=97, first_failed=96, first_status=95)
    rc = N.lib().et_take_packed_device(ctx._h, d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n, d_rows.data_ptr(), 0, d_out.data_ptr(), 200,
                                       d_a.data_ptr(), d_b.data_ptr(), None, ctypes.byref(res))
    assert rc == OK and (res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_a == -1).all()) and bool((d_b == -1).all()), "something was enqueued"


# --- 7. offsets above 2^32 ----------------------------------------------------------------------------------------------------------------


def test_offsets_above_4_gib(ctx):
    import torch

    page_len, few = 256 << 10, 5
    rng = np.random.default_rng(0x7A4E00C0)
    body = rng.integers(0, 256, size=page_len + 3, dtype=np.uint8)  # the body of a 256 KiB text, an odd number of bytes
    L = body.size
    n_pages = (1 << 32) // L + 3
    total = few + n_pages * L
    assert page_len <= _small_max() and total > 1 << 32
    d_body = torch.from_numpy(body).cuda()
    # output: the body selected n_pages times behind one row of 5 bytes, so that a row straddles 2^32
    d_store = torch.cat((d_body, d_body[:few]))
    n_rows = n_pages + 1
    d_rows = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    d_rows[0] = 1
    d_raw = torch.full((LEAD + total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((n_rows + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_status = torch.full((n_rows,), 0xEE, dtype=torch.uint8, device="cuda")
    res = ctx.take_packed_device(d_store, _dev_index([0, L, L + few]), _dev_index([0, page_len, page_len + few]), d_rows, d_raw[LEAD : LEAD + total], d_bi, d_ti, d_status)
    torch.cuda.synchronize()
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed) == (OK, total, few + n_pages * page_len, 0)
    steps = torch.arange(n_rows + 1, dtype=torch.int64, device="cuda")
    want_bi, want_ti = steps * L + (few - L), steps * page_len + (few - page_len)
    want_bi[0] = want_ti[0] = 0
    assert torch.equal(d_bi, want_bi) and torch.equal(d_ti, want_ti) and not bool(d_status.any())
    straddling = 1 + ((1 << 32) - few) // L
    assert few + (straddling - 1) * L < 1 << 32 < few + straddling * L and straddling < n_rows
    d_out = d_raw[LEAD : LEAD + total]
    assert torch.equal(d_out[:few], d_body[:few])
    assert torch.equal(d_out[few:].view(n_pages, L), d_body.unsqueeze(0).expand(n_pages, L)), "a row differs from the body"
    assert bool((d_raw[:LEAD] == SENTINEL).all()) and bool((d_raw[LEAD + total :] == SENTINEL).all())
    del d_out, d_raw
    # input: a body behind offset 2^32 + 37 of a zero-filled buffer, another at 0, a record of length zero that spans what lies between
    far = (1 << 32) + 37
    d_bodies = torch.zeros(far + L + 1, dtype=torch.uint8, device="cuda")
    d_bodies[:L] = d_body
    d_bodies[far : far + L] = d_body
    d_raw = torch.full((LEAD + 3 * L + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((5,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_status = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    res = ctx.take_packed_device(d_bodies[: far + L], _dev_index([0, L, far, far + L]), _dev_index([0, page_len, page_len, 2 * page_len]), dev_rows([2, 1, 0, 2]),
                                 d_raw[LEAD : LEAD + 3 * L], d_bi, d_ti, d_status)
    torch.cuda.synchronize()
    # (record 1's body of 2^32 + 37 - L zeros is above 4 * small_max: that row fails alone)
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (OK, 3 * L, 3 * page_len, 1, 1, UNSUPPORTED)
    assert d_bi.tolist() == [0, L, L, 2 * L, 3 * L] and d_ti.tolist() == [0, page_len, page_len, 2 * page_len, 3 * page_len] and d_status.tolist() == [OK, UNSUPPORTED, OK, OK]
    assert torch.equal(d_raw[LEAD : LEAD + 3 * L].view(3, L), d_body.unsqueeze(0).expand(3, L))
    assert bool((d_raw[:LEAD] == SENTINEL).all()) and bool((d_raw[LEAD + 3 * L :] == SENTINEL).all())


# --- 8. round trips -----------------------------------------------------------------------------------------------------------------------


def _taken(ctx, dev, n_rows, d_rows, room):
    """-> (d_out with LEAD sentinel bytes in front and TAIL behind its room, d_body_index, d_text_index, result) of a take with room to
    spare; nothing is waited for."""
    import torch

    d_raw = torch.full((LEAD + room + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((n_rows + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    return d_raw[LEAD:], d_bi, d_ti, ctx.take_packed_device(*dev, d_rows, d_raw[LEAD : LEAD + room], d_bi, d_ti)


def _guards_intact(d_out, total):
    """_taken's d_out: the sentinels in front of it and behind its first `total` bytes."""
    import torch

    d_raw = torch.as_strided(d_out, (LEAD + d_out.numel(),), (1,), d_out.storage_offset() - LEAD)
    return bool((d_raw[:LEAD] == SENTINEL).all()) and bool((d_out[total:] == SENTINEL).all())


@pytest.mark.parametrize("name", ["permutation", "neighbours_doubled"])
def test_the_taken_store_decodes_to_the_selected_texts(ctx, name):
    import torch

    st, texts = mixed_store()
    rows = selection(name, st.n)
    want = [texts[int(r)] for r in rows]
    dev, d_rows = upload(st), dev_rows(rows)
    text_total = sum(len(t) for t in want)
    d_out, d_bi, d_ti, t = _taken(ctx, dev, rows.size, d_rows, int(st.bodies.size) * 2)
    d_text = torch.full((text_total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = ctx.decode_packed_device(st.cb, d_out[: t.out_bytes], d_bi, d_ti, d_text[:text_total])  # straight from the take
    d_gathered = torch.full((text_total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_gi = torch.full((rows.size + 1,), -1, dtype=torch.int64, device="cuda")
    g = ctx.decode_packed_gather_device(st.cb, *dev, d_rows, d_gathered[:text_total], d_gi)
    torch.cuda.synchronize()
    assert (t.status, t.n_failed, t.text_bytes) == (OK, 0, text_total) and _guards_intact(d_out, t.out_bytes)
    assert (p.status, p.n_failed, p.n_short, p.out_bytes) == (OK, 0, 0, text_total) and (g.status, g.n_failed, g.n_short) == (OK, 0, 0)
    host = d_text.cpu().numpy()
    assert host[:text_total].tobytes() == b"".join(want), "the taken store's texts differ from the oracle's"
    assert bool((host[text_total:] == SENTINEL).all()) and torch.equal(d_text, d_gathered) and torch.equal(d_ti, d_gi)


def test_a_body_kept_raw_elsewhere_keeps_its_length(ctx):
    import torch

    from tests.test_gpu_packed import _join, wants_encode

    texts = [corpus.text_like(n, 0x7A4E00D0 + n).tobytes() for n in (50, 60, 70, 0, 90)]
    tab = oracle_table(np.frombuffer(b"".join(texts), np.uint8))
    bodies = [body for _, body in wants_encode(tab, *_join(texts))]
    bodies[2] = b""  # no bytes under a length of 70
    st = make_store(tab, texts, bodies)
    rows = np.array([2, 0, 2, 3, 4, 2, 1])
    r = take(ctx, st, rows)
    assert [int(x) for x in np.diff(r.text_index)] == [len(texts[i]) for i in rows] and [int(x) for x in np.diff(r.body_index)] == [len(bodies[i]) for i in rows]
    total = int(r.text_index[-1])
    d_text = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = ctx.decode_packed_device(st.cb, r.d_out, r.d_body_index, r.d_text_index, d_text[:total])
    d_gi = torch.full((rows.size + 1,), -1, dtype=torch.int64, device="cuda")
    g = ctx.decode_packed_gather_device(st.cb, *upload(st), dev_rows(rows), d_text.clone()[:total], d_gi)
    torch.cuda.synchronize()
    assert (p.status, p.n_failed, p.n_short) == (OK, 0, 3) and (g.n_failed, g.n_short) == (0, 3)
    host = d_text.cpu().numpy()
    for k, i in enumerate(rows):
        t0, t1 = int(r.text_index[k]), int(r.text_index[k + 1])
        assert host[t0:t1].tobytes() == (texts[i] if i != 2 else bytes([SENTINEL]) * 70)


def test_match_take_join_gather_on_one_context(ctx):
    """encode_packed of a key column -> match(PREFIX) -> take -> join with the taken store as the key set -> gather: nothing is
    synchronised in between, and text appears at the very end only."""
    import torch

    import entreepy_amd as E

    rng = np.random.default_rng(0x7A4E00E0)
    words = [bytes(rng.choice(np.frombuffer(b"abcx", np.uint8), size=int(rng.integers(1, 4))).tobytes()) + b"-%04d" % int(rng.integers(0, 400)) for _ in range(1500)]
    keys, records = words[:600], [words[int(i)] for i in rng.integers(0, 1500, size=2500)]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(words), np.uint8), minlength=256))
    sides = []
    for column in (keys, records):
        index = _index_of([len(w) for w in column])
        d_text, d_index = _dev_bytes(np.frombuffer(b"".join(column), np.uint8)), _dev_index(index)
        d_out = torch.empty(cb.body_bound(int(index[-1])) + len(column), dtype=torch.uint8, device="cuda")
        d_out_index = torch.empty(len(column) + 1, dtype=torch.int64, device="cuda")
        sides.append((d_out, d_out_index, d_index, d_text))
    d_rows, d_hits = torch.full((600,), -1, dtype=torch.int32, device="cuda"), torch.full((2500,), -1, dtype=torch.int32, device="cuda")
    d_texts = torch.full((int(sides[1][3].numel()) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_texts_index = torch.full((2501,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    enc = [ctx.encode_packed_device(cb, s[3], s[2], s[0], s[1]) for s in sides]
    key_store, rec_store = ((s[0][: e.out_bytes], s[1], s[2]) for s, e in zip(sides, enc))
    m = ctx.match_packed_device(cb, *key_store, b"x", E.MATCH_PREFIX, rows=d_rows)
    d_out, d_bi, d_ti, t = _taken(ctx, key_store, m.n_match, d_rows[: m.n_match], int(enc[0].out_bytes))
    j = ctx.join_packed_device(cb, *rec_store, d_out[: max(t.out_bytes, 1)], d_bi, d_ti, rows=d_hits)
    g = ctx.decode_packed_gather_device(cb, *rec_store, d_hits[: j.n_match], d_texts[: d_texts.numel() - TAIL], d_texts_index[: j.n_match + 1])
    torch.cuda.synchronize()
    chosen = {k for k in keys if k.startswith(b"x")}
    want_rows = [i for i, w in enumerate(records) if w in chosen]
    assert 0 < len(chosen) < 600 and 0 < len(want_rows) < 2500
    assert all(e.status == OK and e.n_failed == 0 for e in enc) and (m.status, m.n_failed) == (OK, 0) and (t.status, t.n_failed) == (OK, 0)
    assert d_rows[: m.n_match].tolist() == [i for i, k in enumerate(keys) if k.startswith(b"x")]
    assert (j.status, j.n_failed, j.n_keys_failed) == (OK, 0, 0) and d_hits[: j.n_match].tolist() == want_rows and _guards_intact(d_out, t.out_bytes)
    assert (g.status, g.n_failed, g.n_short) == (OK, 0, 0)
    assert d_texts[: g.out_bytes].cpu().numpy().tobytes() == b"".join(records[i] for i in want_rows)


# --- 9. ordering, the list helper ---------------------------------------------------------------------------------------------------------


def test_single_stream_calls_before_and_after_a_take(ctx):
    """et_encode_device, a take, et_decode_device on one ctx with no synchronisation in between, and one more take of another context
    on a side stream."""
    import torch

    import entreepy_amd as E

    st, _ = mixed_store()
    rows = selection("permutation", st.n)
    want = model(st, rows)
    big = corpus.text_like(300_000, 0x7A4E00F0)
    image = np.frombuffer(_oracle().encode(big), np.uint8)
    d_big = torch.from_numpy(big.copy()).cuda()
    d_image = torch.full((E.encode_bound(big.size) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_back = torch.full((big.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    dev, d_rows = upload(st), dev_rows(rows)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    c = E.Context(0)
    try:
        n_image = ctx.encode_device(d_big, d_image[: d_image.numel() - TAIL])
        a = _taken(ctx, dev, rows.size, d_rows, want.total)
        n_back = ctx.decode_device(d_image[:n_image], d_back[: big.size], skip=4)
        c.use_stream(side.cuda_stream)
        b = _taken(c, dev, rows.size, d_rows, want.total)
        torch.cuda.synchronize()
    finally:
        c.close()
    for d_out, d_bi, d_ti, res in (a, b):
        assert (res.status, res.out_bytes, res.text_bytes, res.n_failed) == (OK, want.total, want.text_total, 0)
        host = d_out.cpu().numpy()
        assert np.array_equal(host[: want.total], want.data) and _guards_intact(d_out, want.total)
        assert np.array_equal(d_bi.cpu().numpy().view(np.uint64), want.body_index) and np.array_equal(d_ti.cpu().numpy().view(np.uint64), want.text_index)
    assert n_image == image.size and d_image[:n_image].cpu().numpy().tobytes() == image.tobytes()
    assert n_back == big.size and d_back[: big.size].cpu().numpy().tobytes() == big.tobytes() and bool((d_back[big.size :] == SENTINEL).all())


def test_list_helper_returns_a_store_of_the_selected_records(ctx):
    import entreepy_amd as E

    _, texts = mixed_store()
    texts = texts[:120]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(texts), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, texts)
    lengths = [len(t) for t in texts]
    rows = np.concatenate((np.random.default_rng(0x7A4E0100).integers(0, 120, size=150), [0, 0, 119, 4]))
    new_blob, new_index, new_lengths = ctx.take_packed(blob, out_index, lengths, rows)
    host = np.frombuffer(blob, np.uint8)
    assert new_blob == b"".join(host[int(out_index[r]) : int(out_index[r + 1])].tobytes() for r in rows)
    assert np.array_equal(new_index, _index_of([int(out_index[r + 1] - out_index[r]) for r in rows])) and [int(x) for x in new_lengths] == [lengths[r] for r in rows]
    assert ctx.decode_packed(cb, new_blob, new_index, new_lengths) == [texts[r] for r in rows]
    assert ctx.take_packed(blob, out_index, lengths, [])[0] == b""
    with pytest.raises(E.EntreepyError, match="row 1") as e:
        ctx.take_packed(blob, out_index, lengths, [3, 120, 4])
    assert e.value.status == ARG
