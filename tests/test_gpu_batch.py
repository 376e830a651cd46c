"""GPU: et_encode_batch_device / et_decode_batch_device -- many small streams in one call -- against the oracle.

Every batch is checked stream by stream: the image is the oracle's image, the decoded bytes the oracle's decoded bytes, out_len
the oracle's lengths, status and path what the test says beforehand.  Output buffers are filled with 0xA5 first, and no byte
outside [out_off, out_off + out_cap) of an item may change.  Where a test also goes through ctx.encode / ctx.decode that is a
second check; the oracle is the first."""
import hashlib

import numpy as np
import pytest

from tests import corpus
from tests.test_gpu_parity import GOLDEN_SHA

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GAP = 48  # bytes between two outputs (a multiple of 16), filled with SENTINEL, that no call may touch


def _oracle():
    from oracle import oracle as O

    return O


def _small_max():
    from entreepy_amd import _native as N

    return N.lib().et_batch_small_max()


def _u8(x):
    return x if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), dtype=np.uint8)


class Batch:
    """The device side of one batch call: inputs packed back to back (so their offsets are unaligned), outputs at multiples of
    16 with GAP sentinel bytes between and behind them."""

    def __init__(self, blobs, caps, lead=0):
        import torch

        blobs = [_u8(b) for b in blobs]
        self.in_len = np.array([b.size for b in blobs], dtype=np.uint64)
        self.in_off = (np.concatenate(([0], np.cumsum(self.in_len)[:-1])) + lead).astype(np.uint64) if blobs else np.zeros(0, np.uint64)
        packed = np.concatenate([np.zeros(lead, np.uint8)] + blobs) if blobs else np.zeros(1, np.uint8)
        self.d_in = torch.from_numpy(packed.copy() if packed.size else np.zeros(1, np.uint8)).cuda()
        self.caps = np.asarray(caps, dtype=np.uint64)
        room = (self.caps + np.uint64(15)) // np.uint64(16) * np.uint64(16) + np.uint64(GAP)
        self.out_off = np.concatenate(([0], np.cumsum(room)[:-1])).astype(np.uint64) if blobs else np.zeros(0, np.uint64)
        self.d_out = torch.full((int(room.sum()) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def run(self, fn):
        import torch

        self.out_len, self.status, self.path = fn(self.d_in, self.in_off, self.in_len, self.d_out, self.out_off, self.caps)
        torch.cuda.synchronize()
        self.host = self.d_out.cpu().numpy()
        return self

    def result(self, b):
        o = int(self.out_off[b])
        return self.host[o : o + int(self.out_len[b])].tobytes()

    def assert_nothing_outside(self):
        """Bytes between and behind the outputs are the sentinel still."""
        mask = np.ones(self.host.size, dtype=bool)
        for o, c in zip(self.out_off, self.caps):
            mask[int(o) : int(o) + int(c)] = False
        assert bool((self.host[mask] == SENTINEL).all()), "a byte outside every item's [out_off, out_off + out_cap) was written"


def _encode_batch(ctx, texts, caps=None):
    import entreepy_amd as E

    caps = [E.encode_bound(len(t)) for t in texts] if caps is None else caps
    b = Batch(texts, caps).run(ctx.encode_batch_device)
    b.assert_nothing_outside()
    return b


def _decode_batch(ctx, comps, caps=None, lead=3):
    if caps is None:
        caps = [int.from_bytes(bytes(c[1:5]), "big") + 16 if len(c) >= 5 else 16 for c in comps]
    b = Batch(comps, caps, lead=lead).run(ctx.decode_batch_device)
    b.assert_nothing_outside()
    return b


def _check_roundtrip(ctx, texts, enc_paths=None, dec_paths=None):
    """texts -> images (the oracle's, byte for byte) -> decoded (the oracle's decode of its own image).  -> (enc, dec) batches."""
    O = _oracle()
    want = [O.encode(t) for t in texts]
    enc = _encode_batch(ctx, texts)
    for b, w in enumerate(want):
        assert enc.status[b] == 0, (b, enc.status[b])
        assert enc.out_len[b] == len(w), (b, len(texts[b]), enc.out_len[b], len(w))
        assert enc.result(b) == w, f"stream {b} (n={len(texts[b])}): image differs from the oracle's"
    if enc_paths is not None:
        assert list(enc.path) == list(enc_paths), (list(enc.path), list(enc_paths))
    back = [O.decode(w[4:]) for w in want]
    dec = _decode_batch(ctx, [w[4:] for w in want])
    for b, w in enumerate(back):
        assert dec.status[b] == 0, (b, dec.status[b])
        assert dec.out_len[b] == len(w), (b, len(texts[b]), dec.out_len[b], len(w))
        assert dec.result(b) == w, f"stream {b} (n={len(texts[b])}): decoded bytes differ from the oracle's"
    if dec_paths is not None:
        assert list(dec.path) == list(dec_paths), (list(dec.path), list(dec_paths))
    return enc, dec


def _expected_decode_path(comp):
    """The rule, from et_parse_header's table alone: the batch kernel takes a stream whose dictionary is a full prefix-free
    tree (Kraft sum exactly 1) and that holds at most et_batch_small_max() symbols; a stream that decodes to nothing (no
    dictionary, no symbols, no body) needs no kernel at all and counts as 0."""
    import entreepy_amd as E

    cb, n_symbols, body_off = E.parse_header(bytes(comp[:8192]))
    lengths = cb.length
    if cb.raw.n_coded == 0 or n_symbols == 0 or body_off >= len(comp):
        return 0
    kraft = sum(1 << (32 - int(l)) for l in lengths if l)
    return 0 if kraft == 1 << 32 and n_symbols <= _small_max() else 1


# --- the reference's own files --------------------------------------------------------------------------------------------------


def test_reference_fixtures_in_one_batch(ctx, res_files):
    names = list(GOLDEN_SHA)
    texts = [res_files[n] for n in names]
    enc, dec = _check_roundtrip(ctx, texts, enc_paths=[0, 0, 0], dec_paths=[0, 0, 0])
    for b, name in enumerate(names):
        assert hashlib.sha256(enc.result(b)).hexdigest() == GOLDEN_SHA[name], name
        assert dec.result(b) == texts[b], name


# --- 1024 text-like streams -----------------------------------------------------------------------------------------------------

EDGES = [1, 2, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 65536]


def test_1024_text_like_streams_of_every_length(ctx):
    """Lengths log-uniform between 1 and et_batch_small_max() (so that short streams are as common as long ones; about 20 MB
    in all), the edge lengths and et_batch_small_max() itself forced in.  All of them by the batch kernels."""
    rng = np.random.default_rng(0xBA7C01)
    small_max = _small_max()
    lengths = np.exp(rng.uniform(0.0, np.log(small_max), size=1024)).astype(np.int64).clip(1, small_max)
    forced = EDGES + [small_max]
    lengths[rng.choice(1024, size=len(forced), replace=False)] = forced
    pool = corpus.text_like(int(lengths.sum()), 0xBA7C02)
    cuts = np.concatenate(([0], np.cumsum(lengths)))
    texts = [pool[cuts[i] : cuts[i + 1]] for i in range(1024)]
    enc, dec = _check_roundtrip(ctx, texts, enc_paths=[0] * 1024, dec_paths=[0] * 1024)
    assert int(np.count_nonzero(enc.in_off % 16)) > 900  # (packed back to back: the inputs are unaligned)
    for b in range(1024):
        if len(set(texts[b].tolist())) > 1:  # (a lone symbol encodes to the bare header, Q2)
            assert dec.result(b) == texts[b].tobytes(), b


# --- the code families ----------------------------------------------------------------------------------------------------------


def _families(res_files):
    n = 50_000
    rng = np.random.default_rng(0xBA7C03)
    zeros97 = np.where(rng.random(n) < 0.97, 0, rng.integers(1, 65, size=n)).astype(np.uint8)
    fam = [("text", corpus.text_like(n, 0xBA7C04)), ("two_symbols", corpus.uniform(n, 0xBA7C05, 65, 67)), ("single_symbol", np.full(1000, 97, np.uint8))]
    for k in (4, 10, 26, 64, 255, 256):
        lo = 1 if k == 255 else 0
        fam.append((f"uniform{k}", corpus.uniform(n, 0xBA7C10 + k, lo, lo + k)))
    fam += [("zeros97", zeros97), ("nul_bytes", corpus.uniform(n, 0xBA7C06, 0, 40)),
            ("midsummer_eee", np.frombuffer(res_files["a_midsummer_nights_dream.txt"] + b"eee", dtype=np.uint8))]
    return fam


def test_every_code_family_in_one_batch(ctx, res_files):
    """Text, two symbols, a lone symbol (bare header, decodes to nothing: Q2), uniform over 4 / 10 / 26 / 64 / 255 / 256 values
    (256: lossy by construction, Q1), 97 % zeros, NUL bytes, Midsummer + 'eee'.  The encode takes all of them itself.  Which
    way the decode goes follows from the dictionary (_expected_decode_path): the batch kernel wherever it is a full tree.
    The 256-value stream's dictionary IS one -- Q1 drops the most frequent symbol BEFORE the tree is built (255 leaves), so
    no leaf is missing from it; its text is short of the dropped symbols, and the decode stops when the bits run out."""
    O = _oracle()
    fam = _families(res_files)
    texts = [t for _, t in fam]
    assert np.unique(dict(fam)["uniform256"]).size == 256
    want = [O.encode(t) for t in texts]
    dec_paths = [_expected_decode_path(w[4:]) for w in want]
    enc, dec = _check_roundtrip(ctx, texts, enc_paths=[0] * len(fam), dec_paths=dec_paths)
    by_name = {name: b for b, (name, _) in enumerate(fam)}
    assert enc.result(by_name["single_symbol"]) == bytes.fromhex("e7c0de0100000003e8") and dec.out_len[by_name["single_symbol"]] == 0
    assert dec.out_len[by_name["uniform256"]] < len(texts[by_name["uniform256"]])  # (lossy: compared with the oracle above)
    for name in ("text", "two_symbols", "uniform4", "uniform10", "uniform26", "uniform64", "uniform255", "zeros97", "nul_bytes", "midsummer_eee"):
        assert dec_paths[by_name[name]] == 0, name
        assert dec.result(by_name[name]) == texts[by_name[name]].tobytes(), name


def test_a_dictionary_that_is_no_full_tree_goes_to_the_single_stream_path(ctx):
    """A hand-made stream whose dictionary lacks a leaf (codes 0, 10, 110; 111 is no code) between two ordinary ones: the
    decode hands it to et_decode_device (path 1) and gives what the oracle gives."""
    import entreepy_amd as E

    O = _oracle()
    data, length = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    for sym, (code, l) in zip(b"abc", [(0b0, 1), (0b10, 2), (0b110, 3)]):
        data[sym], length[sym] = code, l
    rng = np.random.default_rng(0xBA7C07)
    text = np.frombuffer(b"abc", dtype=np.uint8)[rng.integers(0, 3, size=20_000)]
    body, _ = O.pack_body(data, length, text)
    comp = E.Codebook.from_tables(data, length).header(text.size)[4:] + body
    assert _expected_decode_path(comp) == 1
    good = O.encode(corpus.text_like(3000, 0xBA7C08))[4:]
    dec = _decode_batch(ctx, [good, comp, good])
    assert list(dec.status) == [0, 0, 0] and list(dec.path) == [0, 1, 0]
    assert dec.result(1) == O.decode(comp) == text.tobytes()
    assert dec.result(0) == dec.result(2) == O.decode(good)


# --- streams too long for the batch kernels ----------------------------------------------------------------------------------------


def test_long_streams_are_delegated(ctx):
    small_max = _small_max()
    lengths = [5000, small_max + 1, 70_000, 4 << 20, 1, small_max]
    texts = [corpus.text_like(n, 0xBA7C20 + i) for i, n in enumerate(lengths)]
    paths = [1 if n > small_max else 0 for n in lengths]
    assert paths == [0, 1, 0, 1, 0, 0]
    _check_roundtrip(ctx, texts, enc_paths=paths, dec_paths=paths)


# --- failures stay local ------------------------------------------------------------------------------------------------------------


def test_encode_failures_stay_local(ctx):
    import entreepy_amd as E
    from entreepy_amd import _native as N

    O = _oracle()
    texts = [corpus.text_like(n, 0xBA7C30 + i) for i, n in enumerate([7000, 0, 300, 9000, 4096])]
    caps = [E.encode_bound(len(t)) for t in texts]
    caps[1] = 64
    caps[3] -= 1  # one byte short
    with pytest.raises(O.OracleError) as e:
        O.encode(texts[1])
    assert e.value.status == O.QUEUE_EMPTY
    enc = _encode_batch(ctx, texts, caps)
    assert list(enc.status) == [0, N.ET_ERR_EMPTY, 0, N.ET_ERR_CAP, 0]
    assert list(enc.out_len[[1, 3]]) == [0, 0]
    for b in (0, 2, 4):
        assert enc.result(b) == O.encode(texts[b]), b
    for b in (1, 3):  # nothing was written for the failed ones
        o = int(enc.out_off[b])
        assert bool((enc.host[o : o + int(caps[b])] == SENTINEL).all()), b


def test_decode_failures_stay_local(ctx):
    from entreepy_amd import _native as N

    O = _oracle()
    texts = [corpus.text_like(n, 0xBA7C40 + i) for i, n in enumerate([6000, 5000, 100, 5000, 20_000, 30_000, 777, 9000])]
    comps = [bytearray(O.encode(t)[4:]) for t in texts]
    comps[1][6] = 0  # the first dictionary entry's code length: no code has length 0
    comps[3] = comps[3][:20]  # ends inside the dictionary
    body5 = len(comps[5]) - 200
    comps[5] = comps[5][: len(comps[5]) - body5 // 2]  # ends in the middle of the body
    caps = [len(t) + 16 for t in texts]
    caps[7] = len(texts[7]) - 1  # one byte short
    with pytest.raises(O.OracleError) as e:  # (the oracle reads a dictionary that ends early leniently; et_parse_header does not)
        O.decode(bytes(comps[1]))
    assert e.value.status == O.FORMAT
    short = O.decode(bytes(comps[5]))
    assert 0 < len(short) < len(texts[5]) and texts[5].tobytes().startswith(short)
    dec = _decode_batch(ctx, [bytes(c) for c in comps], caps)
    assert list(dec.status) == [0, N.ET_ERR_FORMAT, 0, N.ET_ERR_FORMAT, 0, 0, 0, N.ET_ERR_CAP]
    assert list(dec.path) == [0] * 8
    assert list(dec.out_len[[1, 3, 7]]) == [0, 0, 0]
    assert dec.out_len[5] == len(short) and dec.result(5) == short
    for b in (0, 2, 4, 6):
        assert dec.result(b) == texts[b].tobytes() == O.decode(bytes(comps[b])), b
    for b in (1, 3):
        o = int(dec.out_off[b])
        assert bool((dec.host[o : o + int(caps[b])] == SENTINEL).all()), b


def test_overlapping_outputs_are_refused_before_anything_runs(ctx):
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    texts = [corpus.text_like(2000, 0xBA7C50 + i) for i in range(3)]
    b = Batch(texts, [E.encode_bound(2000)] * 3)
    b.out_off[2] = b.out_off[0] + np.uint64(E.encode_bound(2000) - 16)  # item 2 begins inside item 0's room
    for fn in (ctx.encode_batch_device, ctx.decode_batch_device):
        with pytest.raises(E.EntreepyError) as e:
            fn(b.d_in, b.in_off, b.in_len, b.d_out, b.out_off, b.caps)
        assert e.value.status == N.ET_ERR_ARG
        torch.cuda.synchronize()
        assert bool((b.d_out == SENTINEL).all()), "something was enqueued"


def test_null_items_are_an_argument_error(ctx):
    from entreepy_amd import _native as N

    b = Batch([corpus.text_like(100, 1)], [8000])
    for fn in (N.lib().et_encode_batch_device, N.lib().et_decode_batch_device):
        assert fn(ctx._h, b.d_in.data_ptr(), b.d_out.data_ptr(), None, 1) == N.ET_ERR_ARG
        items = (N.BatchItem * 1)()
        assert fn(ctx._h, None, b.d_out.data_ptr(), items, 1) == N.ET_ERR_ARG
        assert fn(ctx._h, b.d_in.data_ptr(), None, items, 1) == N.ET_ERR_ARG


# --- batch sizes ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_items", [0, 1, 20_000])
def test_batch_sizes(ctx, n_items):
    """0 items (ET_OK, nothing enqueued), 1, and 20 000 streams of 64 bytes: twenty chunks of launches, back to back."""
    pool = corpus.text_like(64 * n_items, 0xBA7C60)
    texts = [pool[64 * i : 64 * i + 64] for i in range(n_items)]
    enc, dec = _check_roundtrip(ctx, texts, enc_paths=[0] * n_items, dec_paths=[0] * n_items)
    assert enc.out_len.size == dec.out_len.size == n_items
    if n_items == 0:
        assert bool((enc.host == SENTINEL).all()) and bool((dec.host == SENTINEL).all())


# --- the two APIs are interchangeable --------------------------------------------------------------------------------------------------


def test_batch_and_single_stream_calls_are_interchangeable(ctx):
    O = _oracle()
    rng = np.random.default_rng(0xBA7C70)
    texts = [corpus.text_like(int(n), 0xBA7C71 + i) for i, n in enumerate(rng.integers(2, 40_000, size=24))]
    singles = [ctx.encode(t) for t in texts]
    dec = _decode_batch(ctx, [s[4:] for s in singles])
    enc = _encode_batch(ctx, texts)
    for b, t in enumerate(texts):
        assert singles[b] == O.encode(t)
        assert dec.status[b] == 0 and dec.result(b) == O.decode(singles[b][4:]) == t.tobytes(), b
        assert enc.status[b] == 0 and enc.result(b) == singles[b], b
        assert ctx.decode(enc.result(b)[4:]) == t.tobytes(), b


def test_list_pair_round_trips_100_random_byte_strings(ctx):
    """Context.encode_batch / decode_batch: random lengths, random alphabets of 2 .. 255 values (so that every string is
    lossless: no lone symbol, Q2, and never all 256 values, Q1)."""
    O = _oracle()
    rng = np.random.default_rng(0xBA7C80)
    strings = []
    for _ in range(100):
        alphabet = rng.choice(256, size=int(rng.integers(2, 256)), replace=False).astype(np.uint8)
        s = alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(2, 20_000)))]
        s[:2] = alphabet[:2]
        strings.append(s.tobytes())
    images = ctx.encode_batch(strings)
    assert images == [O.encode(s) for s in strings]
    assert ctx.decode_batch([im[4:] for im in images]) == strings
    assert ctx.encode_batch([]) == [] and ctx.decode_batch([]) == []


def test_list_pair_names_the_first_failed_item(ctx):
    import entreepy_amd as E

    with pytest.raises(E.EmptyInputError, match="item 2"):
        ctx.encode_batch([b"abc", b"hello", b"", b"x", b""])
    good = _oracle().encode(b"hello world")[4:]
    with pytest.raises(E.EntreepyError, match="item 1") as e:
        ctx.decode_batch([good, good[:7], good])
    assert e.value.status == 4  # ET_ERR_FORMAT


# --- streams ---------------------------------------------------------------------------------------------------------------------------


def test_batch_call_on_a_side_stream_between_default_stream_calls():
    """A single-stream encode on the default stream, a batch encode on a torch side stream, then -- back on the default stream
    -- a batch decode of the images the side stream is still writing and a single-stream decode, with no synchronisation in
    between: the context's own stream switches order them (include/entreepy_hip.h, "STREAM SWITCHES")."""
    import torch

    import entreepy_amd as E

    O = _oracle()
    big = corpus.text_like((8 << 20) + 5, 0xBA7C90)
    pool = corpus.text_like(512 * 30_000, 0xBA7C91)
    texts = [pool[30_000 * i : 30_000 * (i + 1)] for i in range(512)]
    d_big = torch.from_numpy(big).cuda()
    enc_big = torch.full((E.encode_bound(big.size) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    dec_big = torch.full((big.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    b = Batch(texts, [E.encode_bound(30_000)] * 512)
    back = Batch([], [])
    back.d_out = torch.full((512 * 30_016 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    back_off = (np.arange(512) * 30_016).astype(np.uint64)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    c = E.Context(0)
    try:
        m = c.encode_device(d_big, enc_big)
        with torch.cuda.stream(side):
            out_len, status, path = c.encode_batch_device(b.d_in, b.in_off, b.in_len, b.d_out, b.out_off, b.caps)
        assert not status.any() and not path.any()
        dec_len, dec_status, dec_path = c.decode_batch_device(b.d_out, b.out_off + np.uint64(4), out_len - np.uint64(4), back.d_out, back_off,
                                                              np.full(512, 30_000, np.uint64))
        assert c.decode_device(enc_big, dec_big, skip=4, length=m - 4) == big.size
        torch.cuda.synchronize()
    finally:
        c.close()
    assert not dec_status.any() and not dec_path.any() and list(dec_len) == [30_000] * 512
    assert enc_big[:m].cpu().numpy().tobytes() == O.encode(big)
    assert dec_big[: big.size].cpu().numpy().tobytes() == big.tobytes() and bool((dec_big[big.size :] == SENTINEL).all())
    images, decoded = b.d_out.cpu().numpy(), back.d_out.cpu().numpy()
    for i, t in enumerate(texts):
        o = int(b.out_off[i])
        assert images[o : o + int(out_len[i])].tobytes() == O.encode(t), i
        assert decoded[30_016 * i : 30_016 * i + 30_000].tobytes() == t.tobytes(), i
        assert bool((decoded[30_016 * i + 30_000 : 30_016 * (i + 1)] == SENTINEL).all()), i
