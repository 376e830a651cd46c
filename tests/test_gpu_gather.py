"""GPU: et_decode_packed_gather_device -- a selection of a packed store's records decoded into a dense output the call lays out --
against the oracle: the text of row k is want_decode(table, body, length) of record rows[k] (tests/test_gpu_shared.py), the offsets
are the cumulative sum of the rows' rooms, computed here in numpy.  d_out (cap + TAIL bytes), d_out_index, d_written and d_status
are filled with sentinels first; afterwards every byte no row's [out_index[k], out_index[k] + written[k]) owns must still hold it."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus
from tests.test_gpu_batch import SENTINEL, _oracle, _small_max
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of, _join, check_result, wants_encode
from tests.test_gpu_shared import _cb, _family, _length_batch, want_decode
from tests.test_shared_host import oracle_table, table_255

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
SCAN_TILE = 4096  # rows per trip of the scan kernel's one workgroup (csrc/et_batch.h PACKED_SCAN_TILE)


def make_store(tab, texts, bodies=None):
    """The host side of a packed store: the bodies of `texts` under `tab` back to back (or `bodies`, where a test cuts them), the two
    offset arrays.  A text the encoder refuses (above small_max) keeps its length and has an empty body."""
    text, text_index = _join(texts)
    if bodies is None:
        bodies = [body for _, body in wants_encode(tab, text, text_index)]
    blob, body_index = _join(bodies)
    return SimpleNamespace(tab=tab, cb=_cb(tab), bodies=blob, body_index=body_index, text_index=text_index, n=len(texts))


def upload(st, spare=0):
    """-> (d_bodies, d_body_index, d_text_index); `spare` more bytes are mapped behind the bodies (a copy of their beginning)."""
    d = _dev_bytes(np.concatenate((st.bodies, st.bodies[:spare])))
    return d[: st.bodies.size], _dev_index(st.body_index), _dev_index(st.text_index)


def want_rows(st, rows):
    """Per row (status, room, text): judged from the record's own two pairs, as the header states it."""
    body_bytes = st.bodies.size
    memo, out = {}, []
    for r in (int(r) for r in rows):
        if r not in memo:
            if r >= st.n:
                memo[r] = (ARG, 0, b"")
            else:
                b0, b1, t0, t1 = (int(x) for x in (st.body_index[r], st.body_index[r + 1], st.text_index[r], st.text_index[r + 1]))
                if not (b0 <= b1 <= body_bytes and t0 <= t1):
                    memo[r] = (ARG, 0, b"")
                elif t1 - t0 > _small_max():
                    memo[r] = (UNSUPPORTED, 0, b"")
                else:
                    memo[r] = (OK, t1 - t0, want_decode(st.tab, st.bodies[b0:b1].tobytes(), t1 - t0)[1])
        out.append(memo[r])
    return out


def dev_rows(rows):
    import torch

    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint32).view(np.int32).copy()).cuda()


def run_gather(ctx, st, dev, rows, cap, sizes_only=False, shift=0):
    """One call, every output full of sentinels first; d_out begins `shift` bytes behind an aligned address."""
    import torch

    d_bodies, d_body_index, d_text_index = dev
    n = len(rows)
    r = SimpleNamespace(cap=cap, sizes_only=sizes_only, shift=shift)
    r.d_raw = torch.full((shift + cap + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert r.d_raw.data_ptr() % 16 == 0
    r.d_out = r.d_raw[shift : shift + max(cap, 1)]  # (an empty tensor has no address: rows that need no room get a byte)
    r.d_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_written = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.res = ctx.decode_packed_gather_device(st.cb, d_bodies, d_body_index, d_text_index, dev_rows(rows), None if sizes_only else r.d_out, r.d_index, r.d_written, r.d_status)
    torch.cuda.synchronize()
    return fetch(r)


def fetch(r):
    r.host, r.index = r.d_raw.cpu().numpy(), r.d_index.cpu().numpy().view(np.uint64)
    r.written, r.status = r.d_written.cpu().numpy(), r.d_status.cpu().numpy()
    return r


def check_gather(r, wants, call_status=OK):
    index = _index_of([room for _, room, _ in wants])
    total = int(index[-1])
    assert np.array_equal(r.index, index), f"out_index differs from the cumulative sum of the rooms, first at {int(np.flatnonzero(r.index != index)[0])}"
    assert list(r.status) == [s for s, _, _ in wants]
    assert r.res.status == call_status and r.res.out_bytes == total, r.res
    decoded = not r.sizes_only and call_status == OK
    short = sum(1 for s, room, data in wants if s == OK and len(data) < room) if decoded else 0
    check_result(r.res, [s for s, _, _ in wants], n_short=short)
    if not decoded:
        assert bool((r.host == SENTINEL).all()), "a byte of d_out was written"
        assert bool((r.written == -1).all()), "d_written was touched"
        return r
    assert list(r.written) == [len(data) for _, _, data in wants]
    out = r.host[r.shift :]
    untouched = np.ones(r.host.size, dtype=bool)
    for k, ((_, _, data), o) in enumerate(zip(wants, index[:-1])):
        assert out[int(o) : int(o) + len(data)].tobytes() == data, f"row {k}: its symbols differ from the oracle's"
        untouched[r.shift + int(o) : r.shift + int(o) + len(data)] = False
    bad = np.flatnonzero(untouched & (r.host != SENTINEL))
    assert bad.size == 0, f"bytes outside every row's [out_index, out_index + written) were written, the first at {int(bad[0]) - r.shift}"
    return r


def gather(ctx, st, rows, dev=None, **kw):
    """Run with cap = the need exactly, and check."""
    wants = want_rows(st, rows)
    return check_gather(run_gather(ctx, st, dev or upload(st), rows, sum(room for _, room, _ in wants), **kw), wants)


@functools.lru_cache(maxsize=None)
def _mixed_store(n=300, seed=0x6A7E4001):
    """n tiny records, 0 .. 200 bytes, the lengths 0 and 1 among them, under the table of their own text."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 201, size=n)
    sizes[:6] = [0, 1, 2, 3, 0, 1]
    pool = corpus.text_like(int(sizes.sum()), seed + 1)
    cuts = _index_of(sizes)
    return make_store(oracle_table(pool), [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(n)])


# --- 1. selections ----------------------------------------------------------------------------------------------------------------


def _selection(name, n):
    rng = np.random.default_rng(0x6A7E4010)
    if name == "identity":
        return np.arange(n)
    if name == "reversed":
        return np.arange(n)[::-1]
    if name == "permutation":
        return rng.permutation(n)
    if name == "random_tenth":
        return np.sort(rng.choice(n, size=n // 10, replace=False))
    if name == "one_record_500_times":
        return np.full(500, 17)
    if name == "neighbours_doubled":
        return np.repeat(rng.permutation(n)[:150], 2)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["identity", "reversed", "permutation", "random_tenth", "one_record_500_times", "neighbours_doubled"])
def test_selections(ctx, name):
    import torch

    st = _mixed_store()
    rows = _selection(name, st.n)
    dev = upload(st)
    r = gather(ctx, st, rows, dev=dev)
    assert r.res.n_failed == 0 and r.res.n_short == 0
    if name == "identity":
        assert {int(o) % 4 for o in r.index[:-1]} == {0, 1, 2, 3}
        total = int(st.text_index[-1])
        d_packed = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
        p = ctx.decode_packed_device(st.cb, dev[0], dev[1], dev[2], d_packed[:total])
        torch.cuda.synchronize()
        assert (p.status, p.n_failed, p.n_short) == (OK, 0, 0) and np.array_equal(r.index, st.text_index)
        assert np.array_equal(r.host[:total], d_packed.cpu().numpy()[:total]), "the identity's bytes differ from et_decode_packed_device's"
    if name == "one_record_500_times":
        assert int(st.text_index[18] - st.text_index[17]) > 0
    if name == "neighbours_doubled":
        assert bool((rows[0::2] == rows[1::2]).all())


# --- 2. scan edges ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_rows", [1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_scan_edges(ctx, n_rows):
    st = _mixed_store(64, 0x6A7E4020)
    rows = np.random.default_rng(0x6A7E4021 + n_rows).integers(0, 64, size=n_rows)
    rows[0] = 7
    gather(ctx, st, rows)


# --- 3. alignment -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_output_base_and_body_alignment(ctx, shift):
    st = _mixed_store(256, 0x6A7E4030)
    dev = upload(st)
    assert dev[0].data_ptr() % 16 == 0
    starts = {int(b) % 16 for b, e in zip(st.body_index[:-1], st.body_index[1:]) if e > b}
    assert starts == set(range(16))
    r = gather(ctx, st, np.random.default_rng(0x6A7E4031).permutation(256), dev=dev, shift=shift)
    assert r.d_out.data_ptr() % 4 == shift and {int(o) % 4 for o in r.index[:-1]} == {0, 1, 2, 3}


# --- 4. long records --------------------------------------------------------------------------------------------------------------


def test_long_records(ctx):
    small_max = _small_max()
    tab, texts = _length_batch()  # 0 .. 8193, small_max, small_max + 1, and the bodies of 8191, 8192 and 8193 bytes
    pool = texts[[len(t) for t in texts].index(small_max)]  # (every byte of it has a code)
    texts = list(texts) + [pool[:15_000], pool[20_000:60_000]]
    st = make_store(tab, texts)
    sizes, body_sizes = np.diff(st.text_index), np.diff(st.body_index)
    at_max, too_long, two_blocks, two_flushes = list(sizes).index(small_max), list(sizes).index(small_max + 1), len(texts) - 2, len(texts) - 1
    assert body_sizes[two_blocks] > 8192 and sizes[two_blocks] < 16384  # more than one 8 KiB block of body
    assert sizes[two_flushes] > 2 * 16384  # more than one flush of the 16 384-symbol stage
    rows = [two_flushes, too_long, at_max, two_blocks, 3, too_long, two_flushes] + list(range(len(texts)))[::-1]
    r = gather(ctx, st, rows)
    assert r.status[1] == UNSUPPORTED and r.index[2] == r.index[1] and r.written[1] == 0
    assert r.status[2] == OK and r.written[2] == small_max
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 1, UNSUPPORTED) and r.res.n_short == 0


# --- 5. code families -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["text", "2bit", "uniform255", "zeros90", "ladder32"])
def test_code_families(ctx, res_files, name):
    tab, draw = _family(name, res_files)
    rng = np.random.default_rng(0x6A7E4050)
    st = make_store(tab, [draw(int(n), 0x6A7E4051 + i) for i, n in enumerate(rng.integers(1, 201, size=60))])
    r = gather(ctx, st, rng.integers(0, 60, size=200))
    assert not r.status.any() and r.res.n_short == 0


# --- 6. failures stay local -------------------------------------------------------------------------------------------------------


def test_failures_stay_local(ctx):
    sizes = [150, 140, 1, 130, 166, 0, 145, 155, 152, 135, 149, 144, 150, 138]
    pool = corpus.text_like(sum(sizes), 0x6A7E4060)
    cuts = _index_of(sizes)
    st = make_store(oracle_table(pool), [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(14)])
    good_text = st.text_index.copy()
    body_bytes = st.bodies.size
    st.body_index[4] = st.body_index[3] - np.uint64(5)  # a decreasing body pair: record 3 fails; record 4's body begins 5 bytes early
    st.body_index[9] = np.uint64(body_bytes + 77)  # a body pair beyond body_bytes: records 8 and 9 fail
    st.text_index[12] = st.text_index[11] - np.uint64(3)  # a decreasing text pair: record 11 fails; record 12 asks for more symbols than its body holds
    bad_records = {3, 8, 9, 11}
    dev = upload(st, spare=body_bytes)  # (what lies behind body_bytes is mapped: a pair that is followed shows as wrong bytes)
    rows = np.array([0, 14, 1, 3, 2, 0xFFFFFFFF, 8, 4, 9, 5, 11, 6, 12, 13, 7, 10, 3, 0], dtype=np.uint32)
    wants = want_rows(st, rows)
    bad_rows = [k for k, r in enumerate(rows) if r >= 14 or int(r) in bad_records]
    assert [k for k, (s, _, _) in enumerate(wants) if s] == bad_rows and all(wants[k][:2] == (ARG, 0) for k in bad_rows)
    for k, r in enumerate(rows):  # the neighbours' texts are the pool's own
        if k not in bad_rows and r not in (4, 12):
            assert wants[k][2] == pool[int(good_text[r]) : int(good_text[r + 1])].tobytes()
    r = check_gather(run_gather(ctx, st, dev, rows, sum(room for _, room, _ in wants)), wants)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (len(bad_rows), 1, ARG)
    # the lowest failing row is not the first failing record
    later = np.array([0, 1, 2, 9, 4, 3], dtype=np.uint32)
    r = gather(ctx, st, later, dev=dev)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (2, 3, ARG)
    # a bad record that no row selects does not matter
    r = gather(ctx, st, np.array([13, 0, 1, 2, 4, 5, 6, 7, 10, 12, 13], dtype=np.uint32), dev=dev)
    assert r.res.n_failed == 0 and not r.status.any()


# --- 7. short and empty bodies ----------------------------------------------------------------------------------------------------


def test_short_and_empty_bodies(ctx):
    rng = np.random.default_rng(0x6A7E4070)
    sizes = rng.integers(50, 201, size=24)
    sizes[3] = 0
    pool = corpus.text_like(int(sizes.sum()), 0x6A7E4071)
    tab = oracle_table(pool)
    cuts = _index_of(sizes)
    texts = [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(24)]
    bodies = [body for _, body in wants_encode(tab, *_join(texts))]
    bodies[5] = bodies[5][:-1]  # cut by a byte: its last codeword, at least, is gone
    bodies[9] = b""  # no body under a length above zero: a record the encoder failed
    st = make_store(tab, texts, bodies)
    rows = np.array([0, 5, 1, 9, 3, 9, 2, 5, 23, 3, 5])
    wants = want_rows(st, rows)
    assert all(0 < len(wants[k][2]) < wants[k][1] for k in (1, 7, 10)) and all(wants[k][1:] == (int(sizes[9]), b"") for k in (3, 5))
    assert all(wants[k] == (OK, 0, b"") for k in (4, 9))  # a length of zero
    r = gather(ctx, st, rows)
    assert r.res.n_short == 5 and r.res.n_failed == 0
    out = r.host[r.shift :]
    for k in (1, 3, 5, 7, 10):  # the room is kept, and what the row did not fill was left alone
        assert int(r.index[k + 1] - r.index[k]) == wants[k][1]
        assert bool((out[int(r.index[k]) + int(r.written[k]) : int(r.index[k + 1])] == SENTINEL).all())


# --- 8. capacity and sizes only ---------------------------------------------------------------------------------------------------


def test_capacity_and_sizes_only(ctx):
    st = _mixed_store()
    rows = np.concatenate((np.random.default_rng(0x6A7E4080).integers(0, st.n, size=400), [st.n + 5, 0]))  # (one row fails: d_status is complete either way)
    dev = upload(st)
    wants = want_rows(st, rows)
    need = sum(room for _, room, _ in wants)
    exact = check_gather(run_gather(ctx, st, dev, rows, need), wants)
    assert exact.host[need] == SENTINEL and exact.res.n_failed == 1
    check_gather(run_gather(ctx, st, dev, rows, need - 1), wants, call_status=CAP)
    check_gather(run_gather(ctx, st, dev, rows, 1), wants, call_status=CAP)
    sizes_only = check_gather(run_gather(ctx, st, dev, rows, need, sizes_only=True), wants)
    assert sizes_only.res == exact.res and np.array_equal(sizes_only.index, exact.index) and np.array_equal(sizes_only.status, exact.status)
    # ... with n_short 0, whatever the writing call counts
    cut = make_store(st.tab, [b"abcdefgh" * 8, b""], [b"", b"\0"])  # (a byte of body under the second record: the blob has an address)
    w = gather(ctx, cut, [0, 0, 0])
    s = check_gather(run_gather(ctx, cut, upload(cut), [0, 0, 0], 192, sizes_only=True), want_rows(cut, [0, 0, 0]))
    assert (w.res.n_short, s.res.n_short) == (3, 0) and np.array_equal(w.index, s.index)
    check_gather(run_gather(ctx, st, dev, rows, need), wants)  # the ctx is as good as before


# --- 9. the table, and no rows ----------------------------------------------------------------------------------------------------


def test_an_incomplete_table_is_refused_with_nothing_enqueued(ctx):
    import torch

    import entreepy_amd as E
    from tests.test_shared_host import table_ladder

    data, length = table_ladder()
    data[110], length[110] = 0, 0  # a hole
    d_bodies, d_index = _dev_bytes(np.full(120, 100, np.uint8)), _dev_index(_index_of([50, 70]))
    d_out = torch.full((200,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_out_index = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    d_written = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    d_status = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EntreepyError) as e:
        ctx.decode_packed_gather_device(_cb((data, length)), d_bodies, d_index, d_index, dev_rows([1, 0]), d_out, d_out_index, d_written, d_status)
    assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_out_index == -1).all()) and bool((d_written == -1).all()) and bool((d_status == 0xEE).all()), "something was enqueued"


def test_no_rows_is_ok_and_zeroes_the_result(ctx):
    import torch

    from entreepy_amd import _native as N

    st = _mixed_store(64, 0x6A7E4020)
    d_bodies, d_body_index, d_text_index = upload(st)
    d_rows = dev_rows([1, 2])
    d_out = torch.full((200,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_out_index = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    res = N.PackedResult(out_bytes=99, n_failed=98, first_failed=97, n_short=96, first_status=95)
    rc = N.lib().et_decode_packed_gather_device(ctx._h, ctypes.byref(st.cb.raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n,
                                                d_rows.data_ptr(), 0, d_out.data_ptr(), 200, d_out_index.data_ptr(), None, None, ctypes.byref(res))
    assert rc == OK and (res.out_bytes, res.n_failed, res.first_failed, res.n_short, res.first_status) == (0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_out_index == -1).all()), "something was enqueued"


# --- 10. offsets above 2^32 -------------------------------------------------------------------------------------------------------


def test_offsets_above_4_gib(ctx):
    import torch

    n_pages, page_len, few = 16_400, 256 << 10, 5
    tab = table_255()
    cb = _cb(tab)
    page = corpus.uniform(page_len, 0x6A7E40A0, 1, 256)
    body, body_few = (np.frombuffer(_oracle().pack_body(tab[0], tab[1], t, 0)[0], np.uint8) for t in (page, page[:few]))
    L = body.size
    total = few + n_pages * page_len
    assert page_len <= _small_max() and total > 1 << 32
    d_page = torch.from_numpy(page).cuda()
    # output: a 256 KiB record selected 16 400 times, behind one row of 5 bytes (2^32 is a multiple of the page: with it a row straddles)
    d_body = torch.from_numpy(body.copy()).cuda()
    d_store = torch.from_numpy(np.concatenate((body, body_few))).cuda()
    n_rows = n_pages + 1
    d_rows = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    d_rows[0] = 1
    d_out = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_index = torch.full((n_rows + 1,), -1, dtype=torch.int64, device="cuda")
    d_written = torch.full((n_rows,), -1, dtype=torch.int32, device="cuda")
    d_status = torch.full((n_rows,), 0xEE, dtype=torch.uint8, device="cuda")
    res = ctx.decode_packed_gather_device(cb, d_store, _dev_index([0, L, L + body_few.size]), _dev_index([0, page_len, page_len + few]), d_rows, d_out[:total], d_index, d_written, d_status)
    torch.cuda.synchronize()
    assert (res.status, res.out_bytes, res.n_failed, res.n_short) == (OK, total, 0, 0)
    want_index = torch.arange(n_rows + 1, dtype=torch.int64, device="cuda") * page_len + (few - page_len)
    want_index[0] = 0
    assert torch.equal(d_index, want_index), "out_index[k] != 5 + (k - 1) * page_len"
    assert int(d_written[0]) == few and bool((d_written[1:] == page_len).all()) and not bool(d_status.any())
    straddling = 1 + ((1 << 32) - few) // page_len
    assert few + (straddling - 1) * page_len < 1 << 32 < few + straddling * page_len
    assert torch.equal(d_out[:few], d_page[:few])
    for k in (1, straddling, n_rows - 1):
        assert torch.equal(d_out[few + (k - 1) * page_len : few + k * page_len], d_page), f"row {k} differs from the page"
    assert torch.equal(d_out[few:total].view(n_pages, page_len), d_page.unsqueeze(0).expand(n_pages, page_len)), "a row differs from the page"
    assert bool((d_out[total:] == SENTINEL).all())
    del d_out
    # input: a body behind offset 2^32, another at 0, a record of length zero that spans what lies between
    far = (1 << 32) + 37
    d_bodies = torch.zeros(far + L + 1, dtype=torch.uint8, device="cuda")
    d_bodies[:L] = d_body
    d_bodies[far : far + L] = d_body
    rows = [2, 1, 0, 2]
    d_out = torch.full((3 * page_len + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_index = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    d_written = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    res = ctx.decode_packed_gather_device(cb, d_bodies[: far + L], _dev_index([0, L, far, far + L]), _dev_index([0, page_len, page_len, 2 * page_len]), dev_rows(rows),
                                          d_out[: 3 * page_len], d_index, d_written)
    torch.cuda.synchronize()
    assert (res.status, res.out_bytes, res.n_failed, res.n_short) == (OK, 3 * page_len, 0, 0)
    assert d_index.tolist() == [0, page_len, page_len, 2 * page_len, 3 * page_len] and d_written.tolist() == [page_len, 0, page_len, page_len]
    assert torch.equal(d_out[: 3 * page_len].view(3, page_len), d_page.unsqueeze(0).expand(3, page_len)) and bool((d_out[3 * page_len :] == SENTINEL).all())


# --- 11. ordering -----------------------------------------------------------------------------------------------------------------


def test_gather_packed_and_single_stream_calls_back_to_back(ctx, res_files):
    """A gather call, a packed decode under another table and et_decode_device on one ctx with no synchronisation in between -- the
    packed calls' table, counters, workspace and report slot are rewritten in stream order -- and one more gather call of another
    context on a side stream."""
    import torch

    import entreepy_amd as E

    a = _mixed_store()
    tab_b, draw = _family("uniform255", res_files)
    b = make_store(tab_b, [draw(n, 0x6A7E40B0 + n) for n in (3000, 1, 9000, 257) * 4])
    big = corpus.text_like(300_000, 0x6A7E40B1)
    d_et = torch.from_numpy(np.frombuffer(_oracle().encode(big), np.uint8).copy()).cuda()
    d_big = torch.full((big.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    rows = np.random.default_rng(0x6A7E40B2).permutation(a.n)
    wants = want_rows(a, rows)
    need = sum(room for _, room, _ in wants)
    dev_a, dev_b = upload(a), upload(b)
    runs = []
    for _ in range(2):
        r = SimpleNamespace(cap=need, sizes_only=False, shift=0, d_raw=torch.full((need + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda"),
                            d_index=torch.full((rows.size + 1,), -1, dtype=torch.int64, device="cuda"), d_written=torch.full((rows.size,), -1, dtype=torch.int32, device="cuda"),
                            d_status=torch.full((rows.size,), 0xEE, dtype=torch.uint8, device="cuda"))
        runs.append(r)
    d_rows = dev_rows(rows)
    b_total = int(b.text_index[-1])
    d_b = torch.full((b_total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    c = E.Context(0)
    try:
        runs[0].res = ctx.decode_packed_gather_device(a.cb, *dev_a, d_rows, runs[0].d_raw[:need], runs[0].d_index, runs[0].d_written, runs[0].d_status)
        p = ctx.decode_packed_device(b.cb, *dev_b, d_b[:b_total])
        m = ctx.decode_device(d_et, d_big[: big.size], skip=4)
        c.use_stream(side.cuda_stream)
        runs[1].res = c.decode_packed_gather_device(a.cb, *dev_a, d_rows, runs[1].d_raw[:need], runs[1].d_index, runs[1].d_written, runs[1].d_status)
        torch.cuda.synchronize()
    finally:
        c.close()
    for r in runs:
        check_gather(fetch(r), wants)
    assert (p.status, p.out_bytes, p.n_failed, p.n_short) == (OK, b_total, 0, 0)
    host = d_b.cpu().numpy()
    want_b = b"".join(want_rows(b, [k])[0][2] for k in range(b.n))
    assert host[:b_total].tobytes() == want_b and bool((host[b_total:] == SENTINEL).all())
    host = d_big.cpu().numpy()
    assert m == big.size and host[: big.size].tobytes() == big.tobytes() and bool((host[big.size :] == SENTINEL).all())


# --- the list helper --------------------------------------------------------------------------------------------------------------


def test_list_helper_returns_the_selected_texts(ctx):
    import entreepy_amd as E

    rng = np.random.default_rng(0x6A7E40C0)
    strings = []
    for _ in range(100):
        alphabet = rng.choice(255, size=int(rng.integers(1, 255)), replace=False).astype(np.uint8)
        strings.append(alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(0, 2000)))].tobytes())
    strings[7] = b""
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(strings), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, strings)
    lengths = [len(s) for s in strings]
    rows = np.concatenate((rng.integers(0, 100, size=150), [7, 7, 99, 0]))
    assert np.unique(rows).size < rows.size
    assert ctx.decode_packed_rows(cb, blob, out_index, lengths, rows) == [strings[int(r)] for r in rows]
    assert ctx.decode_packed_rows(cb, blob, out_index, lengths, []) == []
    with pytest.raises(E.EntreepyError, match="row 1") as e:
        ctx.decode_packed_rows(cb, blob, out_index, lengths, [3, 100, 4])
    assert e.value.status == ARG
