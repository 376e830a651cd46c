"""GPU: et_encode_packed_device / et_decode_packed_device -- dense bodies plus u64 offsets, all on the device -- against the
oracle: the encode's bytes are pack_body's per record, concatenated, and its offsets their cumulative sum; the decode's are the
oracle's decode of write_header + body (tests/test_gpu_shared.py's want_encode / want_decode).  Every output buffer is filled
with the sentinel first, and whatever no record owns -- behind out_index[n] / text_index[n], and the room of a failed or short
record -- must still hold it afterwards."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus
from tests.test_gpu_batch import SENTINEL, _oracle, _small_max, _u8
from tests.test_gpu_shared import Dense, _cb, _family, _length_batch, check, want_decode, want_encode
from tests.test_shared_host import oracle_table, table_255

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
TAIL = 64  # sentinel bytes behind `cap` that no call may touch
SCAN_TILE = 4096  # records per trip of the scan kernel's one workgroup (csrc/et_batch.h PACKED_SCAN_TILE)


def _index_of(sizes):
    return np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.uint64)))).astype(np.uint64)


def _dev_index(index):
    import torch

    return torch.from_numpy(np.ascontiguousarray(index, dtype=np.uint64).view(np.int64)).cuda()


def _dev_bytes(blob):
    """The bytes on the device, in a tensor one byte longer (an empty blob still has an address)."""
    import torch

    blob = _u8(blob)
    d = torch.zeros(blob.size + 1, dtype=torch.uint8, device="cuda")
    d[: blob.size] = torch.from_numpy(blob.copy()).cuda()
    return d[: blob.size]


def _join(texts):
    texts = [_u8(t) for t in texts]
    return (np.concatenate(texts) if texts else np.zeros(0, np.uint8)), _index_of([t.size for t in texts])


def wants_encode(tab, text, index):
    """Per record (status, body), each judged from its own pair of offsets."""
    out = []
    for t0, t1 in zip(index[:-1], index[1:]):
        out.append(want_encode(tab, text[int(t0) : int(t1)]) if t0 <= t1 <= text.size else (ARG, b""))
    return out


def run_encode(ctx, cb, d_text, d_text_index, cap, sizes_only=False):
    import torch

    n = d_text_index.numel() - 1
    r = SimpleNamespace(cap=cap, sizes_only=sizes_only)
    r.d_out = torch.full((cap + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    r.d_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.res = ctx.encode_packed_device(cb, d_text, d_text_index, None if sizes_only else r.d_out[:cap], r.d_index, r.d_status)
    torch.cuda.synchronize()
    r.host, r.index, r.status = r.d_out.cpu().numpy(), r.d_index.cpu().numpy().view(np.uint64), r.d_status.cpu().numpy()
    return r


def check_result(res, statuses, n_short=0):
    failed = np.flatnonzero(np.asarray(statuses))
    assert res.n_failed == failed.size and res.n_short == n_short, (res, failed)
    if failed.size:
        assert (res.first_failed, res.first_status) == (int(failed[0]), int(statuses[failed[0]])), res


def check_encode(r, wants, call_status=OK):
    sizes = [len(body) for _, body in wants]
    index = _index_of(sizes)
    total = int(index[-1])
    assert np.array_equal(r.index, index), f"out_index differs from the cumulative sum of the oracle's sizes, first at {int(np.flatnonzero(r.index != index)[0])}"
    assert list(r.status) == [s for s, _ in wants]
    assert r.res.status == call_status and r.res.out_bytes == total
    check_result(r.res, [s for s, _ in wants])
    if r.sizes_only or call_status != OK:
        assert bool((r.host == SENTINEL).all()), "a byte of d_out was written"
    else:
        assert r.host[:total].tobytes() == b"".join(body for _, body in wants), "the bodies differ from the oracle's concatenation"
        assert bool((r.host[total:] == SENTINEL).all()), "a byte at or behind d_out + out_index[n] was written"
    return r


def wants_decode(tab, bodies, body_index, text_index, cap):
    out = []
    for b0, b1, t0, t1 in zip(body_index[:-1], body_index[1:], text_index[:-1], text_index[1:]):
        if not (b0 <= b1 <= bodies.size and t0 <= t1 <= cap):
            out.append((ARG, b""))
        else:
            out.append(want_decode(tab, bodies[int(b0) : int(b1)].tobytes(), int(t1 - t0)))
    return out


def run_decode(ctx, cb, d_bodies, d_body_index, d_text_index, cap):
    import torch

    n = d_text_index.numel() - 1
    r = SimpleNamespace(cap=cap)
    r.d_out = torch.full((cap + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    r.d_written = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.res = ctx.decode_packed_device(cb, d_bodies, d_body_index, d_text_index, r.d_out[:cap], r.d_written, r.d_status)
    torch.cuda.synchronize()
    r.host, r.written, r.status = r.d_out.cpu().numpy(), r.d_written.cpu().numpy(), r.d_status.cpu().numpy()
    return r


def check_decode(r, wants, text_index):
    assert list(r.status) == [s for s, _ in wants]
    assert list(r.written) == [len(data) for _, data in wants]
    assert r.res.status == OK and r.res.out_bytes == int(text_index[-1])
    short = sum(1 for (s, data), t0, t1 in zip(wants, text_index[:-1], text_index[1:]) if s == OK and len(data) < int(t1) - int(t0))
    check_result(r.res, [s for s, _ in wants], n_short=short)
    untouched = np.ones(r.host.size, dtype=bool)
    for (_, data), t0 in zip(wants, text_index[:-1]):
        assert r.host[int(t0) : int(t0) + len(data)].tobytes() == data, "a record's symbols differ from the oracle's"
        untouched[int(t0) : int(t0) + len(data)] = False
    bad = np.flatnonzero(untouched & (r.host != SENTINEL))
    assert bad.size == 0, f"bytes outside every record's [text_index, text_index + written) were written, the first at {int(bad[0])}"
    return r


def roundtrip(ctx, tab, texts):
    """Encode with cap = the total exactly; decode the encoder's own d_out / d_out_index, handed straight back."""
    cb = _cb(tab)
    text, index = _join(texts)
    wants = wants_encode(tab, text, index)
    total = sum(len(body) for _, body in wants)
    d_text, d_index = _dev_bytes(text), _dev_index(index)
    enc = check_encode(run_encode(ctx, cb, d_text, d_index, total), wants)
    back = wants_decode(tab, enc.host[:total], enc.index, index, text.size)
    dec = check_decode(run_decode(ctx, cb, enc.d_out[:total], enc.d_index, d_index, text.size), back, index)
    for (s, _), (_, data), t in zip(wants, back, texts):
        assert data == (_u8(t).tobytes() if s == OK else b"")
    return enc, dec


# --- 1. lengths -------------------------------------------------------------------------------------------------------------------


def test_lengths(ctx):
    tab, texts = _length_batch()  # 0 .. 8193, small_max, small_max + 1, and the bodies of 8191, 8192 and 8193 bytes
    small_max = _small_max()
    at = [len(t) for t in texts].index(small_max + 1)
    enc, dec = roundtrip(ctx, tab, texts)
    assert enc.status[at] == UNSUPPORTED and int(np.count_nonzero(enc.status)) == 1
    assert enc.index[at] == enc.index[at + 1] and enc.index[at - 1] < enc.index[at] < enc.index[at + 2]  # no bytes; its neighbours are adjacent
    assert list(np.diff(enc.index)[-3:]) == [8191, 8192, 8193]
    # (its empty body under a count above zero decodes to nothing and counts as short)
    assert dec.written[at] == 0 and dec.res.n_short == 1 and dec.written[at - 1] == small_max


# --- 2. alignment -----------------------------------------------------------------------------------------------------------------


def test_every_text_and_body_alignment(ctx):
    rng = np.random.default_rng(0x9AC4ED02)
    sizes = rng.integers(100, 301, size=256)
    pool = corpus.text_like(int(sizes.sum()), 0x9AC4ED03)
    cuts = _index_of(sizes)
    texts = [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(256)]
    enc, dec = roundtrip(ctx, oracle_table(pool), texts)
    assert enc.d_out.data_ptr() % 16 == 0 and dec.d_out.data_ptr() % 16 == 0
    assert {int(o) % 16 for o in enc.index[:-1]} == set(range(16)) and {int(o) % 16 for o in cuts[:-1]} == set(range(16))


# --- 3. scan edges ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 8193] + ([2 * SCAN_TILE + 1] if SCAN_TILE > 4096 else []))
def test_scan_edges(ctx, n):
    rng = np.random.default_rng(0x9AC4ED10 + n)
    sizes = rng.integers(0, 25, size=n)
    sizes[0] = 7  # (n = 1: a batch that is not empty)
    pool = corpus.text_like(int(sizes.sum()) + 1, 0x9AC4ED11)
    cuts = _index_of(sizes)
    roundtrip(ctx, oracle_table(pool), [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(n)])


def test_20000_tiny_records_a_third_of_them_empty(ctx):
    rng = np.random.default_rng(0x9AC4ED12)
    sizes = rng.integers(1, 9, size=20_000)
    sizes[rng.random(20_000) < 1 / 3] = 0
    pool = corpus.text_like(int(sizes.sum()), 0x9AC4ED13)
    cuts = _index_of(sizes)
    enc, _ = roundtrip(ctx, oracle_table(pool), [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(20_000)])
    assert 6000 < int(np.count_nonzero(np.diff(enc.index) == 0)) < 7400


# --- 4. code families -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["text", "2bit", "uniform255", "zeros90", "ladder32"])
def test_code_families(ctx, res_files, name):
    tab, draw = _family(name, res_files)
    rng = np.random.default_rng(0x9AC4ED20)
    texts = [draw(int(n), 0x9AC4ED21 + i) for i, n in enumerate(rng.integers(1, 6000, size=64))]
    enc, dec = roundtrip(ctx, tab, texts)
    assert not enc.status.any() and not dec.status.any() and dec.res.n_short == 0


# --- 5. failures stay local -------------------------------------------------------------------------------------------------------


def test_failures_stay_local(ctx):
    pool = corpus.text_like(24 * 700, 0x9AC4ED30)
    tab = oracle_table(pool)
    uncoded = int(np.flatnonzero(tab[1] == 0)[-1])
    texts = [pool[700 * i : 700 * (i + 1)].copy() for i in range(24)]
    for b, at in ((0, 0), (7, 350), (23, 699)):
        texts[b][at] = uncoded
    enc, dec = roundtrip(ctx, tab, texts)
    assert list(np.flatnonzero(enc.status)) == [0, 7, 23] and set(enc.status[[0, 7, 23]]) == {UNSUPPORTED}
    assert (enc.res.n_failed, enc.res.first_failed, enc.res.first_status) == (3, 0, UNSUPPORTED)
    sizes = np.diff(enc.index)
    assert list(np.flatnonzero(sizes == 0)) == [0, 7, 23] and enc.index[1] == 0 and enc.index[8] == enc.index[7] and enc.index[24] == enc.index[23]
    # a failure that is not the first record's: first_failed names the lowest
    text, index = _join(texts[1:])
    r = check_encode(run_encode(ctx, _cb(tab), _dev_bytes(text), _dev_index(index), int(sizes.sum())), wants_encode(tab, text, index))
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (2, 6, UNSUPPORTED)


# --- 6. capacity ------------------------------------------------------------------------------------------------------------------


def test_capacity(ctx):
    rng = np.random.default_rng(0x9AC4ED40)
    sizes = rng.integers(0, 3000, size=300)
    pool = corpus.text_like(int(sizes.sum()), 0x9AC4ED41)
    tab = oracle_table(pool)
    cb = _cb(tab)
    index = _index_of(sizes)
    wants = wants_encode(tab, pool, index)
    total = sum(len(body) for _, body in wants)
    d_text, d_index = _dev_bytes(pool), _dev_index(index)
    exact = check_encode(run_encode(ctx, cb, d_text, d_index, total), wants)
    assert exact.host[total] == SENTINEL
    check_encode(run_encode(ctx, cb, d_text, d_index, total - 1), wants, call_status=CAP)
    check_encode(run_encode(ctx, cb, d_text, d_index, 1), wants, call_status=CAP)
    sizes_only = check_encode(run_encode(ctx, cb, d_text, d_index, total, sizes_only=True), wants)
    assert sizes_only.res == exact.res and np.array_equal(sizes_only.index, exact.index) and np.array_equal(sizes_only.status, exact.status)
    # decode: a text index that ends one byte beyond cap
    r = run_decode(ctx, cb, exact.d_out[:total], exact.d_index, d_index, pool.size - 1)
    assert r.res.status == CAP and r.res.out_bytes == pool.size
    assert bool((r.host == SENTINEL).all()), "a byte of d_out was written"
    assert bool((r.written == -1).all()) and bool((r.status == 0xEE).all())
    check_decode(run_decode(ctx, cb, exact.d_out[:total], exact.d_index, d_index, pool.size), [(OK, pool[int(a) : int(b)].tobytes()) for a, b in zip(index[:-1], index[1:])], index)


# --- 7. bad offsets are refused, not followed -------------------------------------------------------------------------------------


def _bad_index_batch():
    sizes = [300, 280, 1, 260, 333, 0, 290, 310, 305, 270, 299, 288, 301, 277]
    pool = corpus.text_like(sum(sizes), 0x9AC4ED50)
    return oracle_table(pool), pool, _index_of(sizes)


def test_bad_text_offsets_fail_their_own_records(ctx):
    tab, pool, index = _bad_index_batch()
    d_pool = _dev_bytes(np.concatenate((pool, pool)))  # (what lies behind text_bytes is mapped: a pair that is followed shows as wrong bytes)
    bad = index.copy()
    bad[4] = bad[3] - np.uint64(7)  # a decreasing pair: record 3 fails, record 4 begins 7 bytes early
    bad[9] = np.uint64(pool.size + 1000)  # an entry beyond text_bytes: records 8 and 9 fail
    wants = wants_encode(tab, pool, bad)
    assert [s for s, _ in wants] == [OK, OK, OK, ARG, OK, OK, OK, OK, ARG, ARG, OK, OK, OK, OK] and len(wants[4][1]) > len(wants_encode(tab, pool, index)[4][1])
    total = sum(len(body) for _, body in wants)
    r = check_encode(run_encode(ctx, _cb(tab), d_pool[: pool.size], _dev_index(bad), total), wants)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 3, ARG)
    huge = index.copy()
    huge[6] = np.uint64(1) << np.uint64(63)  # far outside any mapping
    wants = wants_encode(tab, pool, huge)
    assert [b for b, (s, _) in enumerate(wants) if s] == [5, 6]
    check_encode(run_encode(ctx, _cb(tab), d_pool[: pool.size], _dev_index(huge), sum(len(body) for _, body in wants)), wants)


def test_bad_body_and_text_offsets_fail_their_own_records_on_decode(ctx):
    tab, pool, index = _bad_index_batch()
    cb = _cb(tab)
    good = wants_encode(tab, pool, index)
    bodies = np.frombuffer(b"".join(body for _, body in good), np.uint8)
    body_index = _index_of([len(body) for _, body in good])
    d_bodies = _dev_bytes(np.concatenate((bodies, bodies)))
    cap = pool.size
    bad_body = body_index.copy()
    bad_body[4] = bad_body[3] - np.uint64(5)  # decreasing: record 3 fails; record 4's body begins 5 bytes early
    bad_body[9] = np.uint64(bodies.size + 77)  # beyond body_bytes: records 8 and 9 fail
    bad_text = index.copy()
    bad_text[12] = np.uint64(cap + 5)  # beyond cap: records 11 and 12 fail
    wants = wants_decode(tab, bodies, bad_body, bad_text, cap)
    assert [s for s, _ in wants] == [OK, OK, OK, ARG, OK, OK, OK, OK, ARG, ARG, OK, ARG, ARG, OK]
    r = check_decode(run_decode(ctx, cb, d_bodies[: bodies.size], _dev_index(bad_body), _dev_index(bad_text), cap), wants, bad_text)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (5, 3, ARG)
    for b in (0, 1, 2, 5, 6, 7, 10, 13):
        assert wants[b][1] == pool[int(index[b]) : int(index[b + 1])].tobytes()


def test_a_misaligned_offset_array_is_an_argument_error(ctx):
    import torch

    from entreepy_amd import _native as N

    tab, pool, index = _bad_index_batch()
    cb = _cb(tab)
    n = index.size - 1
    d_text = _dev_bytes(pool)
    raw = torch.zeros(8 * (n + 1) + 16, dtype=torch.uint8, device="cuda")
    raw[4 : 4 + 8 * (n + 1)] = torch.from_numpy(index.view(np.uint8).copy()).cuda()
    d_index = _dev_index(index)
    d_out = torch.full((pool.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_out_index = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    res = N.PackedResult()
    L, h, c = N.lib(), ctx._h, ctypes.byref(cb.raw)
    assert L.et_encode_packed_device(h, c, d_text.data_ptr(), pool.size, raw.data_ptr() + 4, n, d_out.data_ptr(), pool.size, d_out_index.data_ptr(), None, ctypes.byref(res)) == ARG
    assert L.et_encode_packed_device(h, c, d_text.data_ptr(), pool.size, d_index.data_ptr(), n, d_out.data_ptr(), pool.size, d_out_index.data_ptr() + 4, None, ctypes.byref(res)) == ARG
    assert L.et_decode_packed_device(h, c, d_text.data_ptr(), pool.size, raw.data_ptr() + 4, d_index.data_ptr(), n, d_out.data_ptr(), pool.size, None, None, ctypes.byref(res)) == ARG
    assert L.et_decode_packed_device(h, c, d_text.data_ptr(), pool.size, d_index.data_ptr(), raw.data_ptr() + 4, n, d_out.data_ptr(), pool.size, None, None, ctypes.byref(res)) == ARG
    # null pointers, too many records, no records
    assert L.et_encode_packed_device(h, c, d_text.data_ptr(), pool.size, d_index.data_ptr(), n, d_out.data_ptr(), pool.size, None, None, ctypes.byref(res)) == ARG
    assert L.et_encode_packed_device(h, c, d_text.data_ptr(), pool.size, d_index.data_ptr(), n, d_out.data_ptr(), pool.size, d_out_index.data_ptr(), None, None) == ARG
    assert L.et_decode_packed_device(h, c, d_text.data_ptr(), pool.size, d_index.data_ptr(), d_index.data_ptr(), n, None, pool.size, None, None, ctypes.byref(res)) == ARG
    assert L.et_encode_packed_device(h, c, d_text.data_ptr(), pool.size, d_index.data_ptr(), 0x80000000, d_out.data_ptr(), pool.size, d_out_index.data_ptr(), None, ctypes.byref(res)) == ARG
    res.out_bytes = 99
    assert L.et_encode_packed_device(h, c, d_text.data_ptr(), pool.size, d_index.data_ptr(), 0, d_out.data_ptr(), pool.size, d_out_index.data_ptr(), None, ctypes.byref(res)) == OK
    assert res.out_bytes == 0
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_out_index == -1).all()), "something was enqueued"


def test_an_incomplete_table_is_refused_with_nothing_enqueued(ctx):
    import torch

    import entreepy_amd as E
    from tests.test_shared_host import table_ladder

    data, length = table_ladder()
    data[110], length[110] = 0, 0  # a hole
    text, index = _join([np.full(50, 100, np.uint8), np.full(70, 101, np.uint8)])
    d_text, d_index = _dev_bytes(text), _dev_index(index)
    d_out = torch.full((200,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_out_index = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    for call in (lambda cb: ctx.encode_packed_device(cb, d_text, d_index, d_out, d_out_index), lambda cb: ctx.decode_packed_device(cb, d_text, d_index, d_index, d_out)):
        with pytest.raises(E.EntreepyError) as e:
            call(_cb((data, length)))
        assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_out_index == -1).all()), "something was enqueued"


# --- 8. short bodies --------------------------------------------------------------------------------------------------------------


def test_bodies_that_end_early(ctx):
    rng = np.random.default_rng(0x9AC4ED60)
    sizes = rng.integers(50, 9000, size=40)
    pool = corpus.text_like(int(sizes.sum()), 0x9AC4ED61)
    tab = oracle_table(pool)
    index = _index_of(sizes)
    bodies = [body for _, body in wants_encode(tab, pool, index)]
    for b in (5, 31):
        bodies[b] = bodies[b][:-1]  # cut by a byte: its last codeword, at least, is gone
    blob, body_index = _join(bodies)
    wants = wants_decode(tab, blob, body_index, index, pool.size)
    assert [b for b, (_, data) in enumerate(wants) if len(data) < sizes[b]] == [5, 31] and all(len(wants[b][1]) > 0 for b in (5, 31))
    r = check_decode(run_decode(ctx, _cb(tab), _dev_bytes(blob), _dev_index(body_index), _dev_index(index), pool.size), wants, index)
    assert r.res.n_short == 2 and r.res.n_failed == 0
    for b in (5, 31):  # the rest of their room was left alone
        assert bool((r.host[int(index[b]) + int(r.written[b]) : int(index[b + 1])] == SENTINEL).all())


# --- 9. offsets above 2^32 --------------------------------------------------------------------------------------------------------


def test_offsets_above_4_gib(ctx):
    import torch

    n, page_len = 17_000, 256 << 10
    tab = table_255()
    cb = _cb(tab)
    page = corpus.uniform(page_len, 0x9AC4ED70, 1, 256)
    body = _oracle().pack_body(tab[0], tab[1], page, 0)[0]
    L = len(body)
    total = n * L
    assert page_len <= _small_max() and total > 1 << 32
    d_text = torch.from_numpy(page).cuda().unsqueeze(0).expand(n, page_len).contiguous().view(-1)
    d_text_index = torch.arange(n + 1, dtype=torch.int64, device="cuda") * page_len
    want_index = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    d_out = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    sizes = ctx.encode_packed_device(cb, d_text, d_text_index, None, d_index)
    assert (sizes.status, sizes.out_bytes, sizes.n_failed) == (OK, total, 0)
    torch.cuda.synchronize()
    assert torch.equal(d_index, want_index) and bool((d_out == SENTINEL).all())
    d_index.fill_(-1)
    res = ctx.encode_packed_device(cb, d_text, d_text_index, d_out[:total], d_index)
    assert res == sizes
    torch.cuda.synchronize()
    assert torch.equal(d_index, want_index), "out_index[b] != b * L"
    straddling = (1 << 32) // L
    assert straddling * L < 1 << 32 < (straddling + 1) * L
    d_body = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).cuda()
    for b in (0, straddling, n - 1):
        assert torch.equal(d_out[b * L : (b + 1) * L], d_body), f"record {b} differs from the oracle's body"
    assert torch.equal(d_out[:total].view(n, L), d_body.unsqueeze(0).expand(n, L)), "a record differs from the oracle's body"
    assert bool((d_out[total:] == SENTINEL).all())
    # random access: a 1-record sub-range of the body offsets, the text laid out afresh ...
    d_page = torch.from_numpy(page).cuda()
    one = torch.tensor([0, page_len], dtype=torch.int64, device="cuda")
    for b in (0, straddling, n - 1):
        d_dec = torch.full((page_len + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_written = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        r = ctx.decode_packed_device(cb, d_out[:total], d_index[b : b + 2], one, d_dec[:page_len], d_written)
        torch.cuda.synchronize()
        assert (r.status, r.out_bytes, r.n_failed, r.n_short) == (OK, page_len, 0, 0) and int(d_written[0]) == page_len
        assert torch.equal(d_dec[:page_len], d_page) and bool((d_dec[page_len:] == SENTINEL).all()), b
    # ... and of both offset arrays: the last record lands at its own place, above 4 GiB, in an output as long as the text
    d_dec = torch.full((n * page_len + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    r = ctx.decode_packed_device(cb, d_out[:total], d_index[n - 1 :], d_text_index[n - 1 :], d_dec[: n * page_len])
    torch.cuda.synchronize()
    assert (r.status, r.out_bytes, r.n_failed, r.n_short) == (OK, n * page_len, 0, 0)
    assert torch.equal(d_dec[(n - 1) * page_len : n * page_len], d_page)
    assert bool((d_dec[: (n - 1) * page_len] == SENTINEL).all()) and bool((d_dec[n * page_len :] == SENTINEL).all())


# --- 10. ordering -----------------------------------------------------------------------------------------------------------------


def _two_batches(res_files):
    out = []
    for name in ("text", "uniform255"):
        tab, draw = _family(name, res_files)
        texts = [draw(n, 0x9AC4ED80 + n) for n in (3000, 1, 9000, 257) * 8]
        text, index = _join(texts)
        wants = wants_encode(tab, text, index)
        out.append(SimpleNamespace(tab=tab, cb=_cb(tab), texts=texts, text=text, index=index, wants=wants, total=sum(len(body) for _, body in wants)))
    return out


def _enqueue_packed(b):
    import torch

    b.d_text, b.d_text_index = _dev_bytes(b.text), _dev_index(b.index)
    b.d_out = torch.full((b.total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    b.d_index = torch.full((len(b.texts) + 1,), -1, dtype=torch.int64, device="cuda")
    b.d_status = torch.full((len(b.texts),), 0xEE, dtype=torch.uint8, device="cuda")
    return b


def _check_enqueued(b):
    r = SimpleNamespace(cap=b.total, sizes_only=False, res=b.res, host=b.d_out.cpu().numpy(), index=b.d_index.cpu().numpy().view(np.uint64), status=b.d_status.cpu().numpy())
    check_encode(r, b.wants)


def test_packed_shared_and_single_stream_calls_back_to_back(ctx, res_files):
    """Two packed encodes under different tables, a shared-table encode and et_encode_device on one ctx with no synchronisation in
    between, then both packed decodes: the packed calls' table, counters and report slot are rewritten in stream order."""
    import torch

    import entreepy_amd as E

    O = _oracle()
    a, b = (_enqueue_packed(x) for x in _two_batches(res_files))
    big = corpus.text_like(300_000, 0x9AC4ED90)
    d_big = torch.from_numpy(big).cuda()
    enc_big = torch.full((E.encode_bound(big.size) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    shared = Dense(a.texts, [a.cb.body_bound(len(t)) for t in a.texts])
    dec = [torch.full((x.text.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda") for x in (a, b)]
    torch.cuda.synchronize()
    a.res = ctx.encode_packed_device(a.cb, a.d_text, a.d_text_index, a.d_out[: a.total], a.d_index, a.d_status)
    b.res = ctx.encode_packed_device(b.cb, b.d_text, b.d_text_index, b.d_out[: b.total], b.d_index, b.d_status)
    shared.out_len, shared.status, shared.path = ctx.encode_shared_device(a.cb, shared.d_in, shared.in_off, shared.in_len, shared.d_out, shared.out_off, shared.caps)
    m = ctx.encode_device(d_big, enc_big)
    back = [ctx.decode_packed_device(x.cb, x.d_out[: x.total], x.d_index, x.d_text_index, d[: x.text.size]) for x, d in zip((b, a), dec[::-1])]
    torch.cuda.synchronize()
    _check_enqueued(a)
    _check_enqueued(b)
    shared.host = shared.d_out.cpu().numpy()
    check(shared, [want_encode(a.tab, t, c) for t, c in zip(a.texts, shared.caps)])
    assert enc_big[:m].cpu().numpy().tobytes() == O.encode(big)
    for x, d, r in zip((a, b), dec, back[::-1]):
        assert (r.status, r.out_bytes, r.n_failed, r.n_short) == (OK, x.text.size, 0, 0)
        host = d.cpu().numpy()
        assert host[: x.text.size].tobytes() == x.text.tobytes() and bool((host[x.text.size :] == SENTINEL).all())


def test_packed_call_on_a_side_stream(res_files):
    """et_ctx_set_stream to a torch side stream, one packed encode there, then -- back on the default stream, nothing in between --
    the packed decode of the bodies the side stream is still writing: the context's stream switches order them."""
    import torch

    import entreepy_amd as E

    pool = corpus.text_like(512 * 30_000, 0x9AC4EDA0)
    tab = oracle_table(pool)
    cb = _cb(tab)
    index = _index_of([30_000] * 512)
    wants = wants_encode(tab, pool, index)
    x = _enqueue_packed(SimpleNamespace(tab=tab, cb=cb, texts=[None] * 512, text=pool, index=index, wants=wants, total=sum(len(body) for _, body in wants)))
    d_dec = torch.full((pool.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    c = E.Context(0)
    try:
        with torch.cuda.stream(side):
            x.res = c.encode_packed_device(cb, x.d_text, x.d_text_index, x.d_out[: x.total], x.d_index, x.d_status)
        r = c.decode_packed_device(cb, x.d_out[: x.total], x.d_index, x.d_text_index, d_dec[: pool.size])
        torch.cuda.synchronize()
    finally:
        c.close()
    _check_enqueued(x)
    assert (r.status, r.out_bytes, r.n_failed, r.n_short) == (OK, pool.size, 0, 0)
    host = d_dec.cpu().numpy()
    assert host[: pool.size].tobytes() == pool.tobytes() and bool((host[pool.size :] == SENTINEL).all())


# --- the list helpers -------------------------------------------------------------------------------------------------------------


def test_list_helpers_round_trip_100_random_byte_strings(ctx):
    import entreepy_amd as E

    O = _oracle()
    rng = np.random.default_rng(0x9AC4EDB0)
    strings = []
    for _ in range(100):
        alphabet = rng.choice(255, size=int(rng.integers(1, 255)), replace=False).astype(np.uint8)
        strings.append(alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(0, 20_000)))].tobytes())
    strings[7] = b""
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(strings), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, strings)
    bodies = [O.pack_body(cb.data, cb.length, s, 0)[0] if s else b"" for s in strings]
    assert blob == b"".join(bodies) and np.array_equal(out_index, _index_of([len(b) for b in bodies])) and out_index.dtype == np.uint64
    assert blob == b"".join(ctx.encode_shared(cb, strings))
    assert ctx.decode_packed(cb, blob, out_index, [len(s) for s in strings]) == strings
    assert ctx.decode_packed(cb, blob, out_index[40:61], [len(s) for s in strings[40:60]]) == strings[40:60]  # a sub-range of the records
    assert ctx.encode_packed(cb, [])[0] == b"" and ctx.decode_packed(cb, b"", np.zeros(1, np.uint64), []) == []
    with pytest.raises(E.EntreepyError, match="item 2") as e:  # (byte 255 is in no string: no code)
        ctx.encode_packed(cb, [strings[0], strings[1], b"ab\xffcd", strings[2], b"\xff"])
    assert e.value.status == UNSUPPORTED
