"""What a context keeps from one call to the next, and what every other call does to it: ONE table.  A plain module like limits.py
and guards.py, imported by name; neither HIP nor torch is touched before a closure runs.  tests/test_retained_host.py checks
(without a GPU) that the table covers every context call of include/entreepy_hip.h and that its fixtures are what the GPU test takes
them for; tests/test_gpu_retained.py runs it on the device.

Two kinds of state (include/entreepy_hip.h, "STATE A CTX KEEPS BETWEEN CALLS"):
  the HISTOGRAM LINK  set by et_histogram_device(d_text, n): the text it names, the tile geometry, the per-tile histograms, the
                      totals on the device and in pinned host memory.  Read by the shard encodes of the same (d_text, n) and by
                      et_histogram_host / _device_ptr / _on_host.
  the HELD RANGE      set by et_decode_range_sync, or et_decode_range_maps + et_decode_range_resolve: the lanes' states, the
                      blocks' exits, counts and offsets, the flags and the decode tables.  Read by et_decode_range_write (and by
                      et_decode_range_resolve, between the two calls of the second pair).
Let X be any other context call made between the call that set the state and the call that reads it.  Per (state, X) exactly one
of these holds:
  KEEPS     the reader returns ET_OK and its result is the reference's, byte for byte, as if X had not been called;
  DROPS     the reader returns ET_ERR_ARG, enqueues nothing, writes nothing, and et_last_error names the missing first call;
  REPLACED  (the held range under another range call) the reader gives the NEW range's result.
A row that DROPS the histogram link because X is itself a histogram of another text (`names`) leaves a link to THAT text: the
shard encode of the old text is refused, et_histogram_host hands out the new text's counts."""
import functools
import os
import shutil
import tempfile

import numpy as np

KEEPS, DROPS, REPLACED = "keeps", "drops", "replaced"
HISTOGRAM, RANGE = "histogram link", "held range"
ET_OK, ET_ERR_ARG = 0, 6

# the calls that set and that read each kind of state (et_last_codebook: the table of the last whole encode, a third and simpler kind)
SETTERS = {HISTOGRAM: ("et_histogram_device",), RANGE: ("et_decode_range_sync", "et_decode_range_maps", "et_decode_range_resolve")}
READERS = {HISTOGRAM: ("et_encode_body_device", "et_encode_head_shard_device", "et_histogram_host", "et_histogram_device_ptr", "et_histogram_on_host"),
           RANGE: ("et_decode_range_write", "et_decode_range_resolve"), "last codebook": ("et_last_codebook",)}
# et_last_error's text for a reader that finds no first call (csrc/et_api.cpp, csrc/et_decode.cpp)
MISSING = {
    "et_encode_body_device": "shard encode needs et_histogram_device on the same (d_text, n) first",
    "et_encode_head_shard_device": "shard encode needs et_histogram_device on the same (d_text, n) first",
    "et_histogram_host": "no current histogram (et_histogram_device first)",
    "et_histogram_device_ptr": "no current histogram (et_histogram_device first)",
    "et_histogram_on_host": "no current histogram (et_histogram_device first)",
    "et_decode_range_write": "et_decode_range_write needs et_decode_range_sync first",
    "et_decode_range_resolve": "et_decode_range_resolve needs et_decode_range_maps first",
}
# context calls that neither set, read nor can damage the state: (call, why it has no row)
EXCLUDED = {
    "et_ctx_create": "makes the context",
    "et_ctx_destroy": "ends it",
    "et_ctx_stream": "a getter: const et_ctx",
    "et_ctx_device": "a getter: const et_ctx",
    "et_last_error": "a getter: const et_ctx",
    "et_group_create": "a group constructor: keeps the pointer, calls nothing",
    "et_group_create_rccl": "a group constructor: keeps the pointer, calls nothing",
}

# ---- the inputs, made once and shared; read-only --------------------------------------------------------------------------------------

HIST_N, HIST_OFFSET, HIST_START_BIT, HIST_ROUNDS = 70_001, 3, 5, 1  # 18 tiles of one 4 KiB round, a ragged last chunk, the text 3 bytes behind an aligned address
OTHER_N = 5_003
RESERVE_GROWS = 32 << 20
TEXT_RANGE_N, ROWS_RANGE_N = 74_000, 43_000  # bodies of five 8 KiB blocks and a ragged tail
BLOCK = 8192
HELD = (1 * BLOCK, 4 * BLOCK)  # blocks 1..3: the range the cells hold


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def hist_text():
    from tests import corpus

    return _frozen(corpus.text_like(HIST_N, 0x5E7A))


@functools.lru_cache(maxsize=None)
def other_text():
    """X's "another text": another distribution, so another code table."""
    from tests import corpus

    return _frozen(corpus.enwik_like(OTHER_N, 77))


@functools.lru_cache(maxsize=None)
def big_text():
    """One byte above et_batch_small_max(): the batch calls hand it to et_encode_device / et_decode_device."""
    from entreepy_amd import _native as N
    from tests import corpus

    return _frozen(corpus.text_like(N.lib().et_batch_small_max() + 1, 78))


TEXTS = {"hist": hist_text, "other": other_text, "big": big_text}


@functools.lru_cache(maxsize=None)
def image(name):
    """The oracle's .et image of a text, less its first four bytes."""
    from oracle import oracle as O

    return O.encode(TEXTS[name]())[4:]


@functools.lru_cache(maxsize=None)
def table_of(name):
    """(data, length) of the oracle's build_dict for a text."""
    from oracle import oracle as O

    data, length, _ = O.build_dict(np.bincount(TEXTS[name](), minlength=256).astype(np.uint64))
    return data, length


def codebook_of(name):
    import entreepy_amd as E

    return E.Codebook.from_tables(*table_of(name))


@functools.lru_cache(maxsize=None)
def hist_reference():
    """-> (counts, the oracle's body packed from HIST_START_BIT and its end bit, the oracle's whole image): what the histogram link's
    readers must give for hist_text() under its own table."""
    from oracle import oracle as O

    text = hist_text()
    data, length = table_of("hist")
    body, end_bit = O.pack_body(data, length, text, HIST_START_BIT)
    return np.bincount(text, minlength=256).astype(np.uint64), body, end_bit, O.encode(text)


@functools.lru_cache(maxsize=None)
def range_fixture(name):
    """The streams whose ranges are held, as tests/test_syncwork_host.py's Stream: "text", the text-like stream of
    tests/test_gpu_syncwork.py (et_decode_range_sync by tree walk); "rows", the 255-value flat stream of tests/test_gpu_rowsync.py
    (et_decode_range_maps + _resolve by rows)."""
    import entreepy_amd as E
    from oracle import oracle as O
    from tests import corpus
    from tests.test_gpu_rowsync import flat
    from tests.test_syncwork_host import Stream, fixture

    if name == "sparse":  # a third one, whose range lies in the decode tables as well: tests/guards.py's sparse dictionary, by window sweeps
        return fixture("sparse")
    text = corpus.text_like(TEXT_RANGE_N, 61) if name == "text" else flat(255, ROWS_RANGE_N, 7, lo=1)
    comp = O.encode(text)[4:]
    cb, n_symbols, body_off = E.parse_header(comp)
    assert n_symbols == text.size
    return Stream("retained/" + name, cb.data, cb.length, text, comp[body_off & ~3 :], (body_off & 3) * 8, comp=comp, body_off=body_off)


def other_range(name):
    """The range X synchronises in place of the held one: block 4 to the stream's ragged end."""
    return 4 * BLOCK, range_fixture(name).n_bytes


# the packed store of the shared-table and packed rows: five records, one of them empty, under the table of their own bytes
RECORDS = [b"to be", b"or not", b"to be or not to be", b"", b"that is the question"]


@functools.lru_cache(maxsize=None)
def store():
    """-> (data, length, the bodies back to back, their n + 1 offsets, the records' lengths), the bodies by the oracle's pack_body."""
    from oracle import oracle as O

    data, length, _ = O.build_dict(np.bincount(np.frombuffer(b"".join(RECORDS), np.uint8), minlength=256).astype(np.uint64))
    bodies = [O.pack_body(data, length, r)[0] if r else b"" for r in RECORDS]
    index = np.concatenate(([0], np.cumsum([len(b) for b in bodies]))).astype(np.uint64)
    return data, length, b"".join(bodies), index, np.array([len(r) for r in RECORDS], np.uint64)


def reserve_growth():
    """{buffer: (bytes it has after the setter on the small fixture, bytes et_ctx_reserve(RESERVE_GROWS) asks for)}, by the sizes in
    csrc/et_api.cpp (make_geometry, ensure_encode_ws, et_ctx_reserve) and csrc/et_decode.cpp (ensure_dec_ws); ensure() rounds up to
    4096.  The context exposes no capacity, so that the reserve of the "grows" row does grow is arithmetic, held here."""
    page = lambda b: (b + 4095) & ~4095
    tiles_held = (HIST_OFFSET + HIST_N + HIST_ROUNDS * 4096 - 1) // (HIST_ROUNDS * 4096)
    rpt = 1
    while rpt < 128 and (15 + RESERVE_GROWS) // (rpt * 4096) > 2048:
        rpt <<= 1
    tiles_reserved = (15 + RESERVE_GROWS + rpt * 4096 - 1) // (rpt * 4096) + 1
    subs_held = (HELD[1] - HELD[0]) * 8 // 256
    subs_reserved = (RESERVE_GROWS + 8192) * 8 // 256 + 2
    return {"tile_hist": (page(tiles_held * 1024), tiles_reserved * 1024), "sub_state": (page(subs_held * 4), subs_reserved * 4)}


# ---- what a cell's calls work on --------------------------------------------------------------------------------------------------


class Env:
    """One FRESH context (reserve growth starts from a known size) and X's inputs on the device, all made and the device drained
    before the setter runs: nothing of X's preparation lies between the setter and the reader."""

    def __init__(self):
        import torch

        import entreepy_amd as E

        self.torch, self.E = torch, E
        self.ctx = E.Context(0)
        self.ctx.use_torch_stream()
        self.other = self.dev(other_text())
        self.other_image = self.dev(image("other"))
        self.hist = torch.zeros(256, dtype=torch.int64, device="cuda")
        self.scratch = torch.empty(E.encode_bound(OTHER_N) + 64, dtype=torch.uint8, device="cuda")
        self.side = torch.cuda.Stream()
        self.streams = {name: self.upload(range_fixture(name)) for name in ("text", "rows", "sparse")}
        self.tmp = tempfile.mkdtemp(prefix="et_retained_")
        self.new_range = None  # (fixture, begin, end, start): what a REPLACED row put in place of the held range
        torch.cuda.synchronize()

    def close(self):
        self.torch.cuda.synchronize()
        self.ctx.close()
        shutil.rmtree(self.tmp, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def dev(self, a):
        a = np.frombuffer(bytes(a), np.uint8) if not isinstance(a, np.ndarray) else a
        return self.torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()

    def at_offset(self, a, off):
        """The bytes on the device as a view that begins `off` bytes behind a 16-byte aligned address."""
        buf = self.torch.zeros(16 + off + a.size + 16, dtype=self.torch.uint8, device="cuda")
        lo = (-buf.data_ptr()) % 16 + off
        buf[lo : lo + a.size] = self.dev(a)
        assert buf[lo:].data_ptr() % 16 == off
        return buf[lo : lo + a.size]

    def upload(self, fx):
        """A stream as the range calls take it: 16 bytes of zeros in front of its 4-byte aligned base, 64 behind its end."""
        d = self.torch.zeros(16 + fx.n_bytes + 64, dtype=self.torch.uint8, device="cuda")
        d[16 : 16 + fx.n_bytes] = self.dev(fx.stream)
        assert d.data_ptr() % 16 == 0
        return d[16 : 16 + fx.n_bytes]

    def file(self, name, content=None):
        path = os.path.join(self.tmp, name)
        if content is not None:
            with open(path, "wb") as f:
                f.write(bytes(content))
        return path

    def store_cb(self):
        return self.E.Codebook.from_tables(*store()[:2])


# ---- the intervening calls, each at its smallest meaningful size ------------------------------------------------------------------


def _nothing(env):
    pass


def _reserve_same(env):
    env.ctx.reserve(1)


def _reserve_grows(env):
    free = env.torch.cuda.mem_get_info()[0]
    env.ctx.reserve(RESERVE_GROWS)
    print(f"reserve({RESERVE_GROWS}): free device memory {free} -> {env.torch.cuda.mem_get_info()[0]} bytes")


def _tile_rounds(env):
    env.ctx.set_tile_rounds(2 * HIST_ROUNDS)


def _set_stream(env):
    env.ctx.use_stream(env.side.cuda_stream)


def _own_stream(env):
    env.ctx.use_own_stream()


def _timing(env):
    env.ctx.enable_timing(True)
    for which in ("encode", "decode", None):
        env.ctx.timings(which)


def _histogram_other(env):
    env.ctx.histogram_device(env.other, env.hist)


def _encode_device_other(env):
    n = env.ctx.encode_device(env.other, env.scratch)
    assert env.scratch[:n].cpu().numpy().tobytes()[4:] == image("other")


def _encode_other(env):
    assert env.ctx.encode(other_text())[4:] == image("other")


def _encode_fd(env):
    assert env.ctx.encode_file(env.file("other.txt", other_text()), env.file("other.et"))[0] == OTHER_N
    with open(env.file("other.et"), "rb") as f:
        assert f.read()[4:] == image("other")


def _decode_device(env):
    n = env.ctx.decode_device(env.other_image, env.scratch[: (OTHER_N + 15) & ~15])
    assert env.scratch[:n].cpu().numpy().tobytes() == other_text().tobytes()


def _decode(env):
    assert env.ctx.decode(image("other")) == other_text().tobytes()


def _decode_fd(env):
    assert env.ctx.decode_file(env.file("in.et", b"\xe7\xc0\xde\x01" + image("other")), env.file("out.txt"))[1] == OTHER_N
    with open(env.file("out.txt"), "rb") as f:
        assert f.read() == other_text().tobytes()


def _decode_body_device(env):
    cb, n, off = env.E.parse_header(image("other"))
    m = env.ctx.decode_body_device(cb, env.other_image[off:], n, env.scratch[: (OTHER_N + 15) & ~15])
    assert env.scratch[:m].cpu().numpy().tobytes() == other_text().tobytes()


def _range_sync_other(env):
    fx = range_fixture("text")
    begin, end = other_range("text")
    s, x, n, _ = fx.truth(begin, end)
    info = env.ctx.decode_range_sync(fx.codebook(), env.streams["text"], begin, end, s)
    assert (info["start_bit"], info["exit_bit"], info["n_symbols"]) == (s, x, n), info
    env.new_range = ("text", begin, end, s)


def _range_maps_other(env):
    fx = range_fixture("rows")
    begin, end = other_range("rows")
    s, x, n, _ = fx.truth(begin, end)
    m, k = env.ctx.decode_range_maps(fx.codebook(), env.streams["rows"], begin, end, -1)
    assert k == 8 and m[s] == x, (list(m), s, x)
    info = env.ctx.decode_range_resolve(s)
    assert (info["start_bit"], info["exit_bit"], info["n_symbols"]) == (s, x, n), info
    env.new_range = ("rows", begin, end, s)


def _small_texts():
    return [other_text()[:100].tobytes(), other_text()[:1000].tobytes()]


def _small_images():
    from oracle import oracle as O

    return [O.encode(t)[4:] for t in _small_texts()]


def _batch_encode_small(env):
    assert [e[4:] for e in env.ctx.encode_batch(_small_texts())] == _small_images()


def _batch_encode_delegated(env):
    big = env.ctx.encode_batch(_small_texts()[:1] + [big_text().tobytes()])[1]
    assert big[4:] == image("big")


def _batch_decode_small(env):
    assert env.ctx.decode_batch(_small_images()) == _small_texts()


def _batch_decode_delegated(env):
    assert env.ctx.decode_batch(_small_images()[:1] + [image("big")])[1] == big_text().tobytes()


def _encode_shared(env):
    _, _, blob, index, _ = store()
    assert b"".join(env.ctx.encode_shared(env.store_cb(), RECORDS)) == blob


def _decode_shared(env):
    _, _, blob, index, lengths = store()
    bodies = [blob[int(a) : int(b)] for a, b in zip(index[:-1], index[1:])]
    assert env.ctx.decode_shared(env.store_cb(), bodies, [int(l) for l in lengths]) == RECORDS


def _encode_packed(env):
    _, _, blob, index, _ = store()
    got, got_index = env.ctx.encode_packed(env.store_cb(), RECORDS)
    assert got == blob and np.array_equal(got_index, index)


def _decode_packed(env):
    _, _, blob, index, lengths = store()
    assert env.ctx.decode_packed(env.store_cb(), blob, index, lengths) == RECORDS


def _gather(env):
    _, _, blob, index, lengths = store()
    assert env.ctx.decode_packed_rows(env.store_cb(), blob, index, lengths, [2, 0, 2]) == [RECORDS[2], RECORDS[0], RECORDS[2]]


def _match(env):
    _, _, blob, index, lengths = store()
    assert env.ctx.match_packed(env.store_cb(), blob, index, lengths, b"to be", env.E.MATCH_PREFIX) == [0, 2]


def _search(env):
    _, _, blob, index, lengths = store()
    assert env.ctx.search_packed(env.store_cb(), blob, index, lengths, b"not", env.E.SEARCH_CONTAINS) == ([1, 2], [3, 9])


def _join(env):
    _, _, blob, index, lengths = store()
    assert env.ctx.join_packed(env.store_cb(), blob, index, lengths, blob[: int(index[2])], index[:3], lengths[:2]) == [0, 1]


def _take(env):
    _, _, blob, index, lengths = store()
    got, got_index, got_lengths = env.ctx.take_packed(blob, index, lengths, [1, 1, 4])
    bodies = [blob[int(index[r]) : int(index[r + 1])] for r in (1, 1, 4)]
    assert got == b"".join(bodies) and got_lengths.tolist() == [6, 6, 20] and int(got_index[-1]) == len(got)


def _selftest_decode_tables(env):
    import ctypes

    from entreepy_amd import _native as N

    where = ctypes.c_int(-1)
    assert N.lib().et_selftest_decode_tables(env.ctx._h, ctypes.byref(codebook_of("other").raw), ctypes.byref(where)) == ET_OK, where.value


def _selftest_treewalk_table(env):
    import ctypes

    from entreepy_amd import _native as N

    diff = ctypes.c_uint32(99)
    assert N.lib().et_selftest_treewalk_table(env.ctx._h, ctypes.byref(codebook_of("other").raw), ctypes.byref(diff)) == ET_OK, diff.value


def _selftest_join_hash(env):
    from entreepy_amd import _native as N

    _, _, blob, index, lengths = store()
    d_blob, d_index = env.ctx._packed_upload(np.frombuffer(blob, np.uint8).copy(), index)
    d_text_index = env.torch.from_numpy(np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)).cuda()
    d_hash = env.torch.zeros(len(RECORDS), dtype=env.torch.int64, device="cuda")
    env.ctx._bind()
    assert N.lib().et_selftest_join_hash(env.ctx._h, d_blob.data_ptr(), d_blob.numel(), d_index.data_ptr(), d_text_index.data_ptr(), len(RECORDS), d_hash.data_ptr()) == ET_OK
    body = np.frombuffer(blob[: int(index[1])], np.uint8).copy()
    assert int(d_hash.cpu().numpy().view(np.uint64)[0]) == N.lib().et_join_hash(body.ctypes.data, body.size, int(lengths[0]))


def _fd_copies(env):
    """et_device_to_fd and et_fd_to_device: 4 KiB of the other text through a file and back."""
    from entreepy_amd import _native as N

    back = env.torch.zeros(4096, dtype=env.torch.uint8, device="cuda")
    env.ctx._bind()
    fd = os.open(env.file("copy.bin"), os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        assert N.lib().et_device_to_fd(env.ctx._h, env.other.data_ptr(), 4096, fd, 0) == ET_OK
        assert N.lib().et_fd_to_device(env.ctx._h, fd, 0, 4096, back.data_ptr()) == ET_OK
    finally:
        os.close(fd)
    env.torch.cuda.synchronize()
    assert back.cpu().numpy().tobytes() == other_text()[:4096].tobytes()


class Row:
    """One intervening call X.  calls: the context functions it makes; hist, held: what becomes of the histogram link and of the
    held range; names: the text the histogram link names after a row that drops it by taking another histogram; encodes: the
    text whose table et_last_codebook holds after X (None: X is no whole encode); why: for a row that drops, the buffer it touches."""

    def __init__(self, name, calls, run, hist=KEEPS, held=KEEPS, names=None, encodes=None, why=None):
        self.name, self.calls, self.run, self.hist, self.held, self.names, self.encodes, self.why = name, tuple(calls), run, hist, held, names, encodes, why

    def outcome(self, state):
        return {HISTOGRAM: self.hist, RANGE: self.held}[state]


_ENCODES = dict(hist=DROPS, why="K1 refills ctx->tile_hist and ctx->hist for its own text: the link names that text now")
_DECODES = dict(held=DROPS, why="the decode's stages refill ctx->sub_state, blk_*, flag and the tables: et_decode_body_device clears the range")
ROWS = [
    Row("nothing", (), _nothing),
    Row("reserve_same", ("et_ctx_reserve",), _reserve_same),
    Row("reserve_grows", ("et_ctx_reserve",), _reserve_grows, hist=DROPS, held=DROPS, why="ensure() replaces ctx->tile_hist / ctx->sub_state, blk_*: what they held is gone"),
    Row("set_tile_rounds", ("et_ctx_set_tile_rounds",), _tile_rounds, hist=DROPS, why="the tile histograms in ctx->tile_hist are of another geometry"),
    Row("set_stream", ("et_ctx_set_stream",), _set_stream),
    Row("use_own_stream", ("et_ctx_use_own_stream",), _own_stream),
    Row("timing", ("et_ctx_enable_timing", "et_last_timings_of", "et_last_timings"), _timing),
    Row("histogram_other", ("et_histogram_device",), _histogram_other, names="other", **_ENCODES),
    Row("encode_device_other", ("et_encode_device",), _encode_device_other, names="other", encodes="other", **_ENCODES),
    Row("encode_other", ("et_encode",), _encode_other, names="other", encodes="other", **_ENCODES),
    Row("encode_fd", ("et_encode_fd",), _encode_fd, names="other", encodes="other", **_ENCODES),
    Row("decode_device", ("et_decode_device",), _decode_device, **_DECODES),
    Row("decode", ("et_decode",), _decode, **_DECODES),
    Row("decode_fd", ("et_decode_fd",), _decode_fd, **_DECODES),
    Row("decode_body_device", ("et_decode_body_device",), _decode_body_device, **_DECODES),
    Row("range_sync_other", ("et_decode_range_sync",), _range_sync_other, held=REPLACED),
    Row("range_maps_other", ("et_decode_range_maps", "et_decode_range_resolve"), _range_maps_other, held=REPLACED),
    Row("batch_encode_small", ("et_encode_batch_device",), _batch_encode_small),
    Row("batch_encode_delegated", ("et_encode_batch_device",), _batch_encode_delegated, names="big", encodes="big", **_ENCODES),
    Row("batch_decode_small", ("et_decode_batch_device",), _batch_decode_small),
    Row("batch_decode_delegated", ("et_decode_batch_device",), _batch_decode_delegated, **_DECODES),
    Row("encode_shared", ("et_encode_shared_device",), _encode_shared),
    Row("decode_shared", ("et_decode_shared_device",), _decode_shared),
    Row("encode_packed", ("et_encode_packed_device",), _encode_packed),
    Row("decode_packed", ("et_decode_packed_device",), _decode_packed),
    Row("gather", ("et_decode_packed_gather_device",), _gather),
    Row("match", ("et_match_packed_device",), _match),
    Row("search", ("et_search_packed_device",), _search),
    Row("join", ("et_join_packed_device",), _join),
    Row("take", ("et_take_packed_device",), _take),
    Row("selftest_decode_tables", ("et_selftest_decode_tables",), _selftest_decode_tables, held=DROPS, why="rebuilds ctx->lut for the caller's table"),
    Row("selftest_treewalk_table", ("et_selftest_treewalk_table",), _selftest_treewalk_table, held=DROPS, why="rebuilds ctx->tw_table and ctx->chain_table for the caller's table"),
    Row("selftest_join_hash", ("et_selftest_join_hash",), _selftest_join_hash),
    Row("fd_copies", ("et_device_to_fd", "et_fd_to_device"), _fd_copies),
]
NAMES = [r.name for r in ROWS]
# the rows that may drop, as the issue names them: nothing else does
DROPS_HISTOGRAM = {"reserve_grows", "set_tile_rounds", "histogram_other", "encode_device_other", "encode_other", "encode_fd", "batch_encode_delegated"}
DROPS_RANGE = {"reserve_grows", "decode_device", "decode", "decode_fd", "decode_body_device", "batch_decode_delegated", "selftest_decode_tables", "selftest_treewalk_table"}


def row(name):
    return ROWS[NAMES.index(name)]
