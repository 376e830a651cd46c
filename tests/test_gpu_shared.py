"""GPU: et_encode_shared_device / et_decode_shared_device -- batched bodies under one code table given by the caller --
against the oracle, record by record: status, out_len, the bytes (pack_body's for the encode; for the decode the oracle's
decode of write_header + body, the only body decoder it has), and the sentinel everywhere else.

Outputs lie at every residue mod 16 with sentinel gaps in front of, between and behind them (Dense below), and every byte outside
a record's [out_off, out_off + out_len) must still be the sentinel afterwards -- for a failed record its whole room."""
import functools

import numpy as np
import pytest

from tests import corpus
from tests.test_gpu_batch import SENTINEL, Batch, _oracle, _small_max, _u8
from tests.test_shared_host import oracle_table, table_255, table_2bit, table_6bit, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
FRONT, GAP = 35, 19  # sentinel bytes in front of the first output and (at least) between two; 64 behind the last


class Dense:
    """The device side of one shared-table call.  Inputs back to back (or input b at address residue in_res[b] mod 16; or the
    outputs of an earlier call, source = (tensor, offsets, lengths)); output b at address residue out_res[b] mod 16 (default
    b % 16) with room for caps[b] bytes."""

    def __init__(self, blobs, caps, in_res=None, out_res=None, source=None):
        import torch

        n = len(caps)
        if source is None:
            blobs = [_u8(b) for b in blobs]
            self.in_len = np.array([b.size for b in blobs], dtype=np.uint64)
            offs, cur = [], 0
            for b, blob in enumerate(blobs):
                if in_res is not None:
                    cur += (in_res[b] - cur) % 16
                offs.append(cur)
                cur += blob.size
            packed = np.zeros(cur + 1, np.uint8)
            for o, blob in zip(offs, blobs):
                packed[o : o + blob.size] = blob
            self.in_off = np.array(offs, dtype=np.uint64)
            self.d_in = torch.from_numpy(packed).cuda()
        else:
            self.d_in, self.in_off, self.in_len = source[0], np.asarray(source[1], np.uint64), np.asarray(source[2], np.uint64)
        self.caps = np.asarray(caps, dtype=np.uint64)
        offs, cur = [], FRONT
        for b in range(n):
            cur += ((b % 16 if out_res is None else out_res[b]) - cur) % 16
            offs.append(cur)
            cur += int(self.caps[b]) + GAP
        self.out_off = np.array(offs, dtype=np.uint64)
        self.d_out = torch.full((cur + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.d_in.data_ptr() % 16 == 0 and self.d_out.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def run(self, fn, sizes_only=False):
        import torch

        self.out_len, self.status, self.path = fn(self.d_in, self.in_off, self.in_len, None if sizes_only else self.d_out, self.out_off, self.caps)
        torch.cuda.synchronize()
        self.host = self.d_out.cpu().numpy()
        return self

    def result(self, b):
        o = int(self.out_off[b])
        return self.host[o : o + int(self.out_len[b])].tobytes()

    def assert_clean(self):
        """Every byte outside the records' [out_off, out_off + out_len) is the sentinel still."""
        mask = np.ones(self.host.size, dtype=bool)
        for o, n in zip(self.out_off, self.out_len):
            mask[int(o) : int(o) + int(n)] = False
        bad = np.flatnonzero(mask & (self.host != SENTINEL))
        assert bad.size == 0, f"bytes outside every record's [out_off, out_off + out_len) were written, the first at {int(bad[0])}"


def _cb(tab):
    import entreepy_amd as E

    return E.Codebook.from_tables(*tab)


def want_encode(tab, text, cap=None):
    """-> (status, body) as the issue states them; cap=None: unlimited (a sizes-only call)."""
    data, length = tab
    t = _u8(text)
    if t.size == 0:
        return OK, b""
    if t.size > _small_max() or bool((length[t] == 0).any()):
        return UNSUPPORTED, b""
    body = _oracle().pack_body(data, length, t, 0)[0]
    return (CAP, b"") if cap is not None and len(body) > cap else (OK, body)


def want_decode(tab, body, count):
    O = _oracle()
    if len(body) == 0 or count == 0:
        return OK, b""
    if count > _small_max():
        return UNSUPPORTED, b""
    return OK, O.decode((O.write_header(tab[0], tab[1], count) + bytes(body))[4:])


def check(run, wants):
    assert len(wants) == run.out_len.size
    for b, (status, data) in enumerate(wants):
        assert run.status[b] == status, (b, int(run.status[b]), status)
        assert run.out_len[b] == len(data), (b, int(run.out_len[b]), len(data))
        assert run.result(b) == data, f"record {b}: the bytes differ from the oracle's"
    assert not run.path.any()
    run.assert_clean()
    return run


def roundtrip(ctx, tab, texts, in_res=None, out_res=None):
    """Encode (caps = et_body_bound), check; decode the encoder's own bodies where they lie (out_cap = the record's length), check."""
    cb = _cb(tab)
    caps = [cb.body_bound(len(t)) for t in texts]
    wants = [want_encode(tab, t, c) for t, c in zip(texts, caps)]
    enc = check(Dense(texts, caps, in_res=in_res, out_res=out_res).run(functools.partial(ctx.encode_shared_device, cb)), wants)
    counts = [len(t) if s == OK else 0 for t, (s, _) in zip(texts, wants)]
    back = [want_decode(tab, body, n) for (_, body), n in zip(wants, counts)]
    dec = check(Dense(None, counts, out_res=out_res, source=(enc.d_out, enc.out_off, enc.out_len)).run(functools.partial(ctx.decode_shared_device, cb)), back)
    for t, (s, _), (_, data) in zip(texts, wants, back):
        if s == OK:
            assert data == _u8(t).tobytes()  # (the oracle's decode inverts its pack)
    return enc, dec


# --- 1. lengths -------------------------------------------------------------------------------------------------------------------

LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193]


@functools.lru_cache(maxsize=None)
def _length_batch():
    """(table, texts): slices of one text-like pool under the pool's own table, so that every byte has a code."""
    small_max = _small_max()
    pool = corpus.text_like(2 * small_max + 200_000, 0x5A4ED01)
    tab = oracle_table(pool)
    texts, cur = [], 0
    for n in LENGTHS + [small_max, small_max + 1]:
        texts.append(pool[cur : cur + n])
        cur += n
    # the three texts whose BODY is 8191, 8192 and 8193 bytes long: the decode's block
    for target in (8191, 8192, 8193):
        for start in range(cur, cur + 4000):
            bits = np.cumsum(tab[1][pool[start : start + 20_000]].astype(np.int64))
            hit = np.flatnonzero((bits + 7) // 8 == target)
            if hit.size:
                texts.append(pool[start : start + int(hit[0]) + 1])
                break
        else:
            raise AssertionError(f"no slice of the pool packs to {target} bytes")
    return tab, texts


def test_lengths(ctx):
    tab, texts = _length_batch()
    small_max = _small_max()
    enc, dec = roundtrip(ctx, tab, texts)
    n = len(LENGTHS)
    assert enc.status[n] == OK and enc.status[n + 1] == UNSUPPORTED and int(np.count_nonzero(enc.status)) == 1
    assert list(enc.out_len[n + 2 :]) == [8191, 8192, 8193]
    assert dec.out_len[n] == small_max and dec.result(n) == texts[n].tobytes()
    # a record of et_batch_small_max() + 1 symbols is not decoded either, and fails alone
    cb = _cb(tab)
    body = enc.result(n)
    d = Dense([body, body, body], [small_max, small_max + 1, 100]).run(functools.partial(ctx.decode_shared_device, cb))
    check(d, [want_decode(tab, body, small_max), (UNSUPPORTED, b""), want_decode(tab, body, 100)])


# --- 2. alignment -----------------------------------------------------------------------------------------------------------------


def test_every_input_and_output_alignment(ctx):
    rng = np.random.default_rng(0x5A4ED02)
    sizes = rng.integers(100, 301, size=256)
    pool = corpus.text_like(int(sizes.sum()), 0x5A4ED03)
    cuts = np.concatenate(([0], np.cumsum(sizes)))
    texts = [pool[cuts[i] : cuts[i + 1]] for i in range(256)]
    in_res, out_res = [i // 16 for i in range(256)], [i % 16 for i in range(256)]
    enc, dec = roundtrip(ctx, oracle_table(pool), texts, in_res=in_res, out_res=out_res)
    base_in, base_out = enc.d_in.data_ptr(), enc.d_out.data_ptr()
    assert {((base_in + int(i)) % 16, (base_out + int(o)) % 16) for i, o in zip(enc.in_off, enc.out_off)} == {(a, b) for a in range(16) for b in range(16)}
    # the decode's inputs are the encode's outputs (residue i % 16); its outputs get the other index
    d = Dense(None, [len(t) for t in texts], out_res=in_res, source=(enc.d_out, enc.out_off, enc.out_len)).run(functools.partial(ctx.decode_shared_device, _cb(oracle_table(pool))))
    check(d, [(OK, t.tobytes()) for t in texts])


# --- 3. code families ---------------------------------------------------------------------------------------------------------------


def _family(name, res_files):
    """-> (table, draw(n, seed))"""
    if name == "text":  # codes beyond the 11 bits of the first-level table
        tab = oracle_table(res_files["a_midsummer_nights_dream.txt"])
        assert int(tab[1].max()) > 11
        return tab, lambda n, seed: corpus.text_like(n, seed)
    if name == "2bit":
        return table_2bit(), lambda n, seed: np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)]
    if name == "6bit":
        return table_6bit(), lambda n, seed: corpus.uniform(n, seed, 32, 96)
    if name == "uniform255":  # 7/8 bits: never self-synchronises, the fixed point does the work
        return table_255(), lambda n, seed: corpus.uniform(n, seed, 1, 256)
    if name == "zeros90":  # a 1-bit codeword: about 200 symbols per lane

        def draw(n, seed):
            rng = np.random.default_rng(seed)
            return np.where(rng.random(n) < 0.9, 0, rng.integers(1, 65, size=n)).astype(np.uint8)

        tab = oracle_table(draw(200_000, 0x5A4ED10))
        assert int(tab[1][0]) == 1
        return tab, draw
    if name == "ladder32":  # lengths 1 .. 31, 32, 32: both 32-bit codewords occur

        def draw(n, seed):
            rng = np.random.default_rng(seed)
            t = (100 + np.minimum(rng.geometric(0.5, size=n) - 1, 32)).astype(np.uint8)
            t[:: max(n // 7, 1)] = 132
            t[n // 2] = 131 if n > 2 else t[n // 2]
            return t

        return table_ladder(), draw
    raise KeyError(name)


@pytest.mark.parametrize("name", ["text", "2bit", "6bit", "uniform255", "zeros90", "ladder32"])
def test_code_families(ctx, res_files, name):
    tab, draw = _family(name, res_files)
    texts = [draw(n, 0x5A4ED20 + n) for n in (1, 257, 5000)]
    if name == "ladder32":
        assert all(132 in t for t in texts) and all(131 in t for t in texts[1:])
    enc, dec = roundtrip(ctx, tab, texts)
    assert not enc.status.any() and [dec.result(b) for b in range(3)] == [t.tobytes() for t in texts]


# --- 4. the tables serve every stream of a workgroup's loop -----------------------------------------------------------------------------


@pytest.mark.parametrize("shape", ["20000_short", "3000_mixed"])
def test_table_reuse_across_the_grid_stride_loop(ctx, shape):
    """More records than any grid holds workgroups, on both sides of a chunk's end."""
    rng = np.random.default_rng(0x5A4ED30)
    if shape == "20000_short":
        sizes = rng.integers(1, 65, size=20_000)
    else:
        sizes = np.exp(rng.uniform(0.0, np.log(9000.0), size=3000)).astype(np.int64).clip(1, 9000)
        sizes[:4] = [1, 9000, 4096, 8193]
    pool = corpus.text_like(int(sizes.sum()), 0x5A4ED31)
    cuts = np.concatenate(([0], np.cumsum(sizes)))
    texts = [pool[cuts[i] : cuts[i + 1]] for i in range(sizes.size)]
    enc, dec = roundtrip(ctx, oracle_table(pool), texts)
    assert not enc.status.any() and not dec.status.any()


# --- 5. failures stay local ---------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _failure_batch():
    """(table, texts, caps): good records, records with one uncoded byte (first, last, offsets 4095 and 4096), one capacity a
    byte short and one exact."""
    pool = corpus.text_like(80_000, 0x5A4ED40)
    tab = oracle_table(pool)
    uncoded = int(np.flatnonzero(tab[1] == 0)[-1])
    sizes = [3000, 6000, 500, 6000, 9000, 9000, 7000, 7000, 1, 4096]
    texts, cur = [], 0
    for n in sizes:
        texts.append(pool[cur : cur + n].copy())
        cur += n
    for b, at in ((1, 0), (3, 5999), (4, 4095), (5, 4096)):
        texts[b][at] = uncoded
    caps = [_cb(tab).body_bound(n) for n in sizes]
    exact = len(_oracle().pack_body(tab[0], tab[1], texts[6], 0)[0])
    caps[6], caps[7] = exact - 1, len(_oracle().pack_body(tab[0], tab[1], texts[7], 0)[0])
    return tab, texts, caps


def test_failures_stay_local(ctx):
    tab, texts, caps = _failure_batch()
    wants = [want_encode(tab, t, c) for t, c in zip(texts, caps)]
    assert [s for s, _ in wants] == [OK, UNSUPPORTED, OK, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, CAP, OK, OK, OK]
    enc = check(Dense(texts, caps).run(functools.partial(ctx.encode_shared_device, _cb(tab))), wants)
    for b in (1, 3, 4, 5, 6):  # nothing was written for the failed ones
        o = int(enc.out_off[b])
        assert enc.out_len[b] == 0 and bool((enc.host[o : o + int(caps[b])] == SENTINEL).all()), b
    assert enc.out_len[7] == caps[7]


# --- 6. sizes only, and the list helpers -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["lengths", "failures"])
def test_sizes_only(ctx, which):
    if which == "lengths":
        tab, texts = _length_batch()
        caps = [_cb(tab).body_bound(len(t)) for t in texts]
    else:
        tab, texts, caps = _failure_batch()
    run = Dense(texts, caps).run(functools.partial(ctx.encode_shared_device, _cb(tab)), sizes_only=True)
    assert bool((run.host == SENTINEL).all())
    wants = [want_encode(tab, t, None) for t in texts]  # (out_cap reads as unlimited)
    assert list(run.status) == [s for s, _ in wants] and list(run.out_len) == [len(d) for _, d in wants]
    writing = Dense(texts, caps).run(functools.partial(ctx.encode_shared_device, _cb(tab)))
    for b, c in enumerate(caps):
        if run.out_len[b] <= c:
            assert (run.status[b], run.out_len[b]) == (writing.status[b], writing.out_len[b]), b
        else:
            assert writing.status[b] == CAP and run.status[b] == OK, b
    # overlapping rooms are no error when nothing is written
    out_len, status, _ = ctx.encode_shared_device(_cb(tab), run.d_in, run.in_off, run.in_len, None, np.zeros(len(texts), np.uint64), run.caps)
    assert list(out_len) == list(run.out_len) and list(status) == list(run.status)


def test_list_helpers_round_trip_100_random_byte_strings(ctx):
    import entreepy_amd as E

    O = _oracle()
    rng = np.random.default_rng(0x5A4ED50)
    strings = []
    for _ in range(100):
        alphabet = rng.choice(255, size=int(rng.integers(1, 255)), replace=False).astype(np.uint8)
        strings.append(alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(0, 20_000)))].tobytes())
    strings[7] = b""
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(strings), np.uint8), minlength=256))
    assert cb.is_complete()
    bodies = ctx.encode_shared(cb, strings)
    assert bodies == [O.pack_body(cb.data, cb.length, s, 0)[0] for s in strings]
    assert ctx.decode_shared(cb, bodies, [len(s) for s in strings]) == strings
    assert ctx.encode_shared(cb, []) == [] and ctx.decode_shared(cb, [], []) == []
    with pytest.raises(E.EntreepyError, match="item 2") as e:  # (byte 255 is in no string: no code)
        ctx.encode_shared(cb, [strings[0], strings[1], b"ab\xffcd", strings[2], b"\xff"])
    assert e.value.status == UNSUPPORTED


# --- 7. decode edges ----------------------------------------------------------------------------------------------------------------------


def test_decode_edges(ctx, res_files):
    O = _oracle()
    tab, draw = _family("zeros90", res_files)
    text_tab = oracle_table(res_files["a_midsummer_nights_dream.txt"])
    for tab, texts in ((tab, [draw(n, 0x5A4ED60 + n) for n in (5000, 30_001, 3, 700)]), (text_tab, [corpus.text_like(n, 0x5A4ED70 + n) for n in (5000, 20_000, 3, 700)])):
        bodies = [O.pack_body(tab[0], tab[1], t, 0)[0] for t in texts]
        blobs, counts = [], []
        for body, t in zip(bodies, texts):
            for cut in (0, 1, 2, 9):  # a body that ends early gives the oracle's shorter result
                if cut < len(body):
                    blobs.append(body[: len(body) - cut])
                    counts.append(len(t))
            blobs.append(body)  # out_cap below the record's length: the first out_cap symbols, nothing behind them
            counts.append(len(t) // 2)
            blobs.append(body)
            counts.append(1)
        blobs += [b"", bodies[0], b""]  # in_len = 0, out_cap = 0, both
        counts += [100, 0, 0]
        wants = [want_decode(tab, body, n) for body, n in zip(blobs, counts)]
        assert wants[0] == (OK, texts[0].tobytes()) and 0 < len(wants[1][1]) < len(texts[0]) and wants[4][1] == texts[0].tobytes()[: len(texts[0]) // 2]
        check(Dense(blobs, counts).run(functools.partial(ctx.decode_shared_device, _cb(tab))), wants)
    # trailing pad bits: records of the 1-bit-code family whose bodies end inside a byte decode to their length and no further
    tab, draw = _family("zeros90", res_files)
    texts = [draw(n, 0x5A4ED80 + n) for n in range(40, 60)]
    assert any(int(tab[1][t].sum()) % 8 for t in texts)
    roundtrip(ctx, tab, texts)


# --- 8. the call -----------------------------------------------------------------------------------------------------------------------------


def test_an_incomplete_table_is_refused_with_nothing_written(ctx):
    import ctypes

    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    data, length = table_ladder()
    data[110], length[110] = 0, 0  # a hole
    cb = _cb((data, length))
    texts = [np.full(50, 100, np.uint8), np.full(70, 101, np.uint8)]
    d = Dense(texts, [64, 64])
    for fn in (N.lib().et_encode_shared_device, N.lib().et_decode_shared_device):
        items = np.zeros(2, dtype=E.Context._ITEM)
        items["in_off"], items["in_len"], items["out_off"], items["out_cap"], items["out_len"] = d.in_off, d.in_len, d.out_off, d.caps, 99
        assert fn(ctx._h, ctypes.byref(cb.raw), d.d_in.data_ptr(), d.d_out.data_ptr(), items.ctypes.data, 2) == UNSUPPORTED
        assert list(items["out_len"]) == [0, 0]
    with pytest.raises(E.EntreepyError) as e:
        ctx.encode_shared_device(cb, d.d_in, d.in_off, d.in_len, None, d.out_off, d.caps)
    assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d.d_out == SENTINEL).all()), "something was enqueued"


def test_overlapping_outputs_and_null_pointers_are_argument_errors(ctx):
    import ctypes

    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    tab = table_6bit()
    cb = _cb(tab)
    texts = [corpus.uniform(2000, 0x5A4ED90 + i, 32, 96) for i in range(3)]
    d = Dense(texts, [1500] * 3)
    d.out_off[2] = d.out_off[0] + np.uint64(1499)  # record 2 begins inside record 0's room
    for fn in (ctx.encode_shared_device, ctx.decode_shared_device):
        with pytest.raises(E.EntreepyError) as e:
            fn(cb, d.d_in, d.in_off, d.in_len, d.d_out, d.out_off, d.caps)
        assert e.value.status == ARG
    torch.cuda.synchronize()
    assert bool((d.d_out == SENTINEL).all()), "something was enqueued"
    items = (N.BatchItem * 1)()
    L = N.lib()
    for fn in (L.et_encode_shared_device, L.et_decode_shared_device):
        assert fn(ctx._h, None, d.d_in.data_ptr(), d.d_out.data_ptr(), items, 1) == ARG
        assert fn(ctx._h, ctypes.byref(cb.raw), None, d.d_out.data_ptr(), items, 1) == ARG
        assert fn(ctx._h, ctypes.byref(cb.raw), d.d_in.data_ptr(), d.d_out.data_ptr(), None, 1) == ARG
        assert fn(ctx._h, ctypes.byref(cb.raw), d.d_in.data_ptr(), d.d_out.data_ptr(), None, 0) == OK  # n_items = 0
    assert L.et_decode_shared_device(ctx._h, ctypes.byref(cb.raw), d.d_in.data_ptr(), None, items, 1) == ARG
    empty = np.zeros(0, np.uint64)
    for fn in (ctx.encode_shared_device, ctx.decode_shared_device):
        out_len, status, path = fn(cb, d.d_in, empty, empty, d.d_out, empty, empty)
        assert out_len.size == status.size == path.size == 0
    torch.cuda.synchronize()
    assert bool((d.d_out == SENTINEL).all())


def test_two_tables_back_to_back_without_synchronisation(ctx, res_files):
    """encode under table A, encode under table B, decode A's bodies, decode B's: four calls on one ctx, nothing between them."""
    import torch

    fams = [_family(name, res_files) for name in ("text", "uniform255")]
    sets = [[draw(n, 0x5A4EDA0 + n) for n in (3000, 1, 9000, 257) * 8] for _, draw in fams]
    cbs = [_cb(tab) for tab, _ in fams]
    encs = [Dense(texts, [cb.body_bound(len(t)) for t in texts]) for texts, cb in zip(sets, cbs)]
    lens = [ctx.encode_shared_device(cb, e.d_in, e.in_off, e.in_len, e.d_out, e.out_off, e.caps) for cb, e in zip(cbs, encs)]
    decs = [Dense(None, [len(t) for t in texts], source=(e.d_out, e.out_off, n[0])) for texts, e, n in zip(sets, encs, lens)]
    outs = [ctx.decode_shared_device(cb, d.d_in, d.in_off, d.in_len, d.d_out, d.out_off, d.caps) for cb, d in zip(cbs, decs)]
    torch.cuda.synchronize()
    for (tab, _), texts, e, n, d, o in zip(fams, sets, encs, lens, decs, outs):
        e.out_len, e.status, e.path = n
        d.out_len, d.status, d.path = o
        e.host, d.host = e.d_out.cpu().numpy(), d.d_out.cpu().numpy()
        check(e, [want_encode(tab, t) for t in texts])
        check(d, [(OK, t.tobytes()) for t in texts])


def test_shared_call_on_a_side_stream_between_default_stream_calls(res_files):
    """A single-stream encode on the default stream, a shared-table encode on a torch side stream, then -- back on the default
    stream -- a shared-table decode of the bodies the side stream is still writing and a single-stream decode, with no
    synchronisation in between: the context's own stream switches order them."""
    import torch

    import entreepy_amd as E

    O = _oracle()
    big = corpus.text_like((8 << 20) + 5, 0x5A4EDB0)
    pool = corpus.text_like(512 * 30_000, 0x5A4EDB1)
    tab = oracle_table(pool)
    cb = _cb(tab)
    texts = [pool[30_000 * i : 30_000 * (i + 1)] for i in range(512)]
    d_big = torch.from_numpy(big).cuda()
    enc_big = torch.full((E.encode_bound(big.size) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    dec_big = torch.full((big.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    e = Dense(texts, [cb.body_bound(30_000)] * 512)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    c = E.Context(0)
    try:
        m = c.encode_device(d_big, enc_big)
        with torch.cuda.stream(side):
            e.out_len, e.status, e.path = c.encode_shared_device(cb, e.d_in, e.in_off, e.in_len, e.d_out, e.out_off, e.caps)
        d = Dense(None, [30_000] * 512, source=(e.d_out, e.out_off, e.out_len))
        d.out_len, d.status, d.path = c.decode_shared_device(cb, d.d_in, d.in_off, d.in_len, d.d_out, d.out_off, d.caps)
        assert c.decode_device(enc_big, dec_big, skip=4, length=m - 4) == big.size
        torch.cuda.synchronize()
    finally:
        c.close()
    assert enc_big[:m].cpu().numpy().tobytes() == O.encode(big)
    assert dec_big[: big.size].cpu().numpy().tobytes() == big.tobytes() and bool((dec_big[big.size :] == SENTINEL).all())
    e.host, d.host = e.d_out.cpu().numpy(), d.d_out.cpu().numpy()
    check(e, [want_encode(tab, t) for t in texts])
    check(d, [(OK, t.tobytes()) for t in texts])


def test_the_ctx_serves_the_other_calls_after_a_shared_call(ctx):
    """A shared-table call, then et_decode_batch_device and et_decode_device on the same ctx: its workspaces stay consistent."""
    O = _oracle()
    pool = corpus.text_like(40 * 5000, 0x5A4EDC0)
    tab = oracle_table(pool)
    texts = [pool[5000 * i : 5000 * (i + 1)] for i in range(40)]
    roundtrip(ctx, tab, texts)
    images = [O.encode(t) for t in texts]
    b = Batch([im[4:] for im in images], [5016] * 40, lead=3).run(ctx.decode_batch_device)
    b.assert_nothing_outside()
    assert not b.status.any() and [b.result(i) for i in range(40)] == [t.tobytes() for t in texts]
    assert ctx.decode(images[0][4:]) == texts[0].tobytes()
    enc, _ = roundtrip(ctx, tab, texts[:5])
    assert enc.result(0) == O.pack_body(tab[0], tab[1], texts[0], 0)[0]
