"""GPU: one Context driven across stream switches with its calls still in flight.

A device call returns before its last kernels finish (a decode's write pass, an encode's K4, a whole histogram), and the next
call rewrites the workspaces those kernels read (sub_state, blk_off, chain_table, tile_off, enc_table ...).  A switch of the
context's stream -- a torch.cuda.stream block, use_stream, use_own_stream, et_ctx_set_stream -- must therefore order the new
stream after everything the context enqueued on the old one (include/entreepy_hip.h, "STREAM SWITCHES").

test_a_switch_orders_the_new_stream_after_the_old is the deterministic probe of that ordering: its calls only write bounded
indices, so it is safe against a library without it.  The others drive every decode family, the encode, the range calls, close()
and the host/file calls across switches at sizes where the previous call's write kernel is still running when the next call's
host work ends; without the ordering they may read stale offsets, so they are only meant for a library that has it.

Every test makes its own Context; no torch.cuda.synchronize() between the calls under test, only before comparing."""
import ctypes
import time

import numpy as np
import pytest

from tests import corpus
from tests.guards import _sparse_dictionary
from tests.test_gpu_rowsync import flat
from tests.test_gpu_strips import sparse

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SENTINEL = 0xA5
SLACK = 64  # bytes past the end of every output, filled with SENTINEL, that no call may touch


def _oracle():
    from oracle import oracle as O

    return O


def _expected_image(text):
    """The .et image the oracle makes of `text` (host uint8): the restatement up to 16 MiB, its chunk-parallel twin above
    (held equal to it by tests/test_oracle.py)."""
    if text.size <= 16 * MiB:
        return _oracle().encode(text)
    from oracle import cpu_fast

    return cpu_fast.encode(text, 16)


def _text(n, seed):
    """n bytes of Midsummer-like text, sampled on the device (fast at these sizes), on the host."""
    import torch

    return corpus.text_like_torch(n, seed, torch.device("cuda", 0)).cpu().numpy()


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def _out(n):
    """An output tensor of n + SLACK bytes, all SENTINEL."""
    import torch

    return torch.full((n + SLACK,), SENTINEL, dtype=torch.uint8, device="cuda")


def _assert_output(out, text_dev, n, what):
    """out[:n] is the text, the SLACK bytes behind it are untouched (call after a synchronize)."""
    import torch

    assert torch.equal(out[:n], text_dev[:n]), f"{what}: wrong bytes"
    assert bool((out[n:] == SENTINEL).all()), f"{what}: bytes past the end were written"


def _path(cb):
    from entreepy_amd import _native as N

    p = ctypes.c_uint32(99)
    assert N.lib().et_decode_path(ctypes.byref(cb.raw), ctypes.byref(p)) == N.ET_OK
    return p.value


# --- a. the probe -------------------------------------------------------------------------------------------------------------


def _busy(stream, junk, iters):
    """Harmless element-wise kernels on an unrelated tensor, enqueued on `stream`."""
    import torch

    with torch.cuda.stream(stream):
        for _ in range(iters):
            junk.mul_(1.0000001)


def _overtakes(A, B, junk, iters):
    """Whether a kernel enqueued on B finishes while A still runs `iters` busy kernels enqueued before it, with no context
    involved: HIP may put two streams on one hardware queue, and there B can never overtake A, whatever the library does."""
    import torch

    _busy(A, junk, iters)
    ea, eb = torch.cuda.Event(), torch.cuda.Event()
    ea.record(A)
    with torch.cuda.stream(B):
        torch.zeros(1024, device="cuda").add_(1)
    eb.record(B)
    overtook = False
    while not ea.query():
        if eb.query():
            overtook = True
            break
    torch.cuda.synchronize()
    return overtook


@pytest.mark.parametrize("how", ["torch_stream_block", "use_stream", "use_own_stream", "et_ctx_set_stream"])
def test_a_switch_orders_the_new_stream_after_the_old(how):
    """Stream A is held busy for ~30 ms by unrelated kernels, then the context enqueues a histogram on it (the call returns at
    once) and switches to B, where it enqueues another.  B's histogram may not finish before A's: an event behind each is polled,
    and B's completing while A's has not is the failure.  Both histograms then equal np.bincount.  A is a stream that B is first
    seen to overtake without the context, so that the probe can fail."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    n_a, n_b = 32 * MiB, 8 * MiB
    host_a = corpus.uniform(n_a, 101)
    host_b = corpus.text_like(n_b, 102)
    text_a, text_b = _dev(host_a), _dev(host_b)
    hist_a = torch.zeros(256, dtype=torch.int64, device="cuda")
    hist_b = torch.zeros(256, dtype=torch.int64, device="cuda")
    junk = torch.ones(64 * MiB, dtype=torch.float32, device="cuda")
    c = E.Context(0)
    try:
        c.reserve(n_a)
        B = torch.cuda.ExternalStream(N.lib().et_ctx_stream(c._h)) if how == "use_own_stream" else torch.cuda.Stream()
        # size the busy work (the first launch of the kernel loads it: not part of what is timed), then pick A
        S = torch.cuda.Stream()
        _busy(S, junk, 2)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(S)
        _busy(S, junk, 20)
        t1.record(S)
        t1.synchronize()
        iters = min(4000, max(100, int(20 * 30.0 / max(t0.elapsed_time(t1), 1e-3)) + 1))
        A = next((s for s in (torch.cuda.Stream() for _ in range(8)) if _overtakes(s, B, junk, iters // 3)), None)
        assert A is not None, "no stream that B overtakes: the probe could not fail"

        def on_a(fn):
            if how == "torch_stream_block":
                with torch.cuda.stream(A):
                    fn()
            else:
                c.use_stream(A.cuda_stream)
                fn()

        def on_b(fn):
            """Switches the context to B the way under test and runs fn there."""
            if how == "torch_stream_block":
                with torch.cuda.stream(B):
                    fn()
                return
            if how == "use_stream":
                c.use_stream(B.cuda_stream)
            elif how == "use_own_stream":
                c.use_own_stream()
            else:
                assert N.lib().et_ctx_set_stream(c._h, ctypes.c_void_p(B.cuda_stream)) == N.ET_OK
            fn()

        # warm both streams: no workspace is allocated or freed inside the probe
        on_a(lambda: c.histogram_device(text_a, hist_a))
        torch.cuda.synchronize()
        on_b(lambda: c.histogram_device(text_b, hist_b))
        torch.cuda.synchronize()
        hist_a.zero_()
        hist_b.zero_()
        torch.cuda.synchronize()

        # the probe
        _busy(A, junk, iters)
        ea, eb = torch.cuda.Event(), torch.cuda.Event()
        on_a(lambda: c.histogram_device(text_a, hist_a))
        ea.record(A)
        on_b(lambda: c.histogram_device(text_b, hist_b))
        eb.record(B)
        assert not ea.query(), "the busy work on A was over before the switch: the probe proves nothing"
        deadline = time.monotonic() + 30.0
        while True:
            b_done = eb.query()  # (B first: B done and then A not yet done means B finished first)
            a_done = ea.query()
            assert not (b_done and not a_done), f"{how}: the call on B finished before the call the context had enqueued on A"
            if a_done:
                break
            assert time.monotonic() < deadline, "A never finished"
        torch.cuda.synchronize()
        assert np.array_equal(hist_a.cpu().numpy(), np.bincount(host_a, minlength=256))
        assert np.array_equal(hist_b.cpu().numpy(), np.bincount(host_b, minlength=256))
    finally:
        torch.cuda.synchronize()  # (a library without the ordering would free the workspaces under A's histogram)
        c.close()


# --- b. every decode family, round-robin over streams ------------------------------------------------------------------------


@pytest.fixture(scope="module")
def family_images():
    """One image per decode family, made and checked synchronously on a context of their own:
    [(name, kind, payload, n, text on the device)], kind "image" (payload: .et minus 4 bytes, on the device) or "body"
    (payload: (Codebook, packed body on the device)).  What each decode runs is asserted here, so the set is known to be covered."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    O = _oracle()
    dev = torch.device("cuda", 0)
    texts = [
        ("text", corpus.text_like_torch(256 * MiB, 0x57AE01, dev), N.ET_PATH_TREE_WALK, {"tree_walk_sync": True, "strips_write": False}),
        ("uniform255", _dev(flat(255, 96 * MiB, 0x57AE02, lo=1)), N.ET_PATH_ROWS, {"row_sync": True}),
        ("flat16", _dev(flat(16, 64 * MiB + 3, 0x57AE03)), N.ET_PATH_FIXED, {"fixed_sync": True}),
        ("zeros97", _dev(sparse(128 * MiB + 5, 0.97, 0x57AE04)), N.ET_PATH_TREE_WALK, {"strips_write": True, "tree_walk_sync": True}),
        ("nearflat31", _dev(flat(31, 32 * MiB + 7, 0x57AE05)), N.ET_PATH_EXIT_MAPS, {"exhaustive_sync": True, "row_sync": False, "fixed_sync": False}),
    ]
    prep = E.Context(0)
    prep.enable_timing(E.Context.TIMING_DECODE_BODY)
    out = []
    try:
        for name, text, path, flags in texts:
            n = text.numel()
            enc = torch.zeros(E.encode_bound(n) + 64, dtype=torch.uint8, device="cuda")
            m = prep.encode_device(text, enc)
            image = enc[4:m].clone()
            del enc
            cb, n_sym, _ = E.parse_header(image[:8192].cpu().numpy().tobytes())
            assert n_sym == n and _path(cb) == path, name
            dec = _out(n)
            assert prep.decode_device(image, dec[: n + SLACK]) == n
            t = prep.timings("decode")
            torch.cuda.synchronize()
            _assert_output(dec, text, n, name)
            for k, v in flags.items():
                assert t[k] == v, (name, t)
            out.append((name, "image", image, n, text))
        # a dictionary no encoder makes, outside the tree walk's domain: the round-1 window kernels
        data_t, len_t, syms = _sparse_dictionary()
        cb = E.Codebook.from_tables(data_t, len_t)
        assert _path(cb) == N.ET_PATH_WINDOWS
        rng = np.random.default_rng(0x57AE06)
        n = 8 * MiB + 9
        host = syms[rng.integers(0, syms.size, size=n)].astype(np.uint8)
        host[rng.random(n) < 0.5] = 32
        body, _ = O.pack_body(data_t, len_t, host)
        d_body = _dev(np.frombuffer(body, dtype=np.uint8))
        text = _dev(host)
        dec = _out(n)
        assert prep.decode_body_device(cb, d_body, n, dec) == n
        torch.cuda.synchronize()
        _assert_output(dec, text, n, "sparse_dictionary")
        out.append(("sparse_dictionary", "body", (cb, d_body), n, text))
    finally:
        prep.close()
    return out


def _decode(c, item, out):
    name, kind, payload, n, _ = item
    if kind == "image":
        return c.decode_device(payload, out)
    cb, body = payload
    return c.decode_body_device(cb, body, n, out)


@pytest.mark.parametrize("n_streams", [1, 2, 3])
def test_alternating_streams_decode_every_family(family_images, n_streams):
    """Every family's image decoded round-robin over n_streams torch streams (1: back to back on one stream), no synchronize in
    between, into separate outputs: once on a context reserved for the largest, once on a fresh one with the images in ascending
    size, so that ensure() reallocates workspaces in the middle of the sequence while earlier writes still run."""
    import torch

    import entreepy_amd as E

    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    by_size = sorted(family_images, key=lambda it: it[3])
    for order, reserve in ((family_images, True), (by_size, False)):
        c = E.Context(0)
        try:
            if reserve:
                c.reserve(max(it[3] for it in order))
            outs = [_out(it[3]) for it in order]
            torch.cuda.synchronize()
            for i, item in enumerate(order):
                with torch.cuda.stream(streams[i % n_streams]):
                    assert _decode(c, item, outs[i]) == item[3], item[0]
            torch.cuda.synchronize()
            for item, out in zip(order, outs):
                _assert_output(out, item[4], item[3], f"{item[0]} (reserved={reserve}, streams={n_streams})")
        finally:
            c.close()


# --- c. the encode ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_streams", [2, 3])
def test_alternating_streams_encode(n_streams):
    """Five texts with different code tables encoded round-robin over the streams without a synchronize (the fifth with codes
    longer than 32 bits: histogram + encode_body_device, k_encode_tiles_long), then every decodable image decoded on a stream
    other than the one that encoded it (the context's own switch is the only thing ordering the decode after the encode).
    Images are the oracle's bytes, decodes the texts.  (Codes beyond 32 bits pack the reference's deterministic garbage,
    test_gpu_parity.py::test_long_codes_beyond_32_bits: that body is compared, not decoded.)"""
    import torch

    import entreepy_amd as E

    O = _oracle()
    hosts = [("text", _text(128 * MiB + 1, 0x57AE11)), ("enwik_like", corpus.enwik_like(48 * MiB + 3, 0x57AE12)),
             ("uniform255", corpus.uniform(64 * MiB + 5, 0x57AE13, 1, 256)), ("zeros97", sparse(64 * MiB + 7, 0.97, 0x57AE14))]
    wants = [_expected_image(h) for _, h in hosts]
    texts = [_dev(h) for _, h in hosts]
    rng = np.random.default_rng(0x57AE15)
    data_t, len_t = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    for s in range(40):
        data_t[s] = rng.integers(0, 1 << 32, dtype=np.uint64)
        len_t[s] = [1, 5, 31, 32, 33, 40, 64, 65, 100, 255][s % 10]
    long_cb = E.Codebook.from_tables(data_t, len_t)
    long_host = rng.integers(0, 40, size=MiB + 1, dtype=np.uint8)
    long_want, long_end = O.pack_body(data_t, len_t, long_host)
    long_text = _dev(long_host)
    long_hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    long_out = torch.zeros(len(long_want) + 64, dtype=torch.uint8, device="cuda")
    encs = [torch.zeros(E.encode_bound(t.numel()) + 64, dtype=torch.uint8, device="cuda") for t in texts]
    decs = [_out(t.numel()) for t in texts]
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    c = E.Context(0)
    try:
        torch.cuda.synchronize()
        ms = []
        for i, (t, enc) in enumerate(zip(texts, encs)):
            with torch.cuda.stream(streams[i % n_streams]):
                ms.append(c.encode_device(t, enc))
        with torch.cuda.stream(streams[len(texts) % n_streams]):
            c.histogram_device(long_text, long_hist)
            end = c.encode_body_device(long_cb, long_text, long_out)
        for i, (enc, m, dec) in enumerate(zip(encs, ms, decs)):
            with torch.cuda.stream(streams[(i + 1) % n_streams]):
                assert c.decode_device(enc, dec, skip=4, length=m - 4) == texts[i].numel()
        torch.cuda.synchronize()
        for (name, _), t, enc, m, want, dec in zip(hosts, texts, encs, ms, wants, decs):
            assert m == len(want) and enc[:m].cpu().numpy().tobytes() == want, name
            _assert_output(dec, t, t.numel(), name)
        assert end == long_end
        assert long_out[: len(long_want)].cpu().numpy().tobytes() == long_want
        assert np.array_equal(long_hist.cpu().numpy(), np.bincount(long_host, minlength=256))
    finally:
        c.close()


# --- d. the range calls ------------------------------------------------------------------------------------------------------


def _split(et, ranks):
    """(Codebook, n_symbols, the body from its 4-byte aligned base on the device, first bit, [(begin, end)] of `ranks` block ranges)."""
    import entreepy_amd as E

    comp = _dev(np.frombuffer(et[4:], dtype=np.uint8))
    cb, n_symbols, body_off = E.parse_header(et[4 : 4 + 8192])
    ptr = comp.data_ptr() + body_off
    base_off, first_bit = body_off - (ptr & 3), (ptr & 3) * 8
    stream = comp[base_off:]
    n_blocks = (stream.numel() + 8191) // 8192
    spans = [(r * n_blocks // ranks * 8192, min((r + 1) * n_blocks // ranks * 8192, stream.numel())) for r in range(ranks)]
    return cb, n_symbols, stream, first_bit, spans


def test_range_calls_across_a_switch():
    """A cold decode over virtual ranks (a context each, as test_cold_decode_virtual_ranks / test_ranges_of_a_stream_split_over_ranks),
    each rank's synchronisation on one stream and its write on another, no synchronize between them: a text through
    decode_range_sync (one rank forced to a wrong start and repaired), uniform bytes through decode_range_maps + _resolve."""
    import torch

    import entreepy_amd as E

    S = [torch.cuda.Stream(), torch.cuda.Stream()]
    ranks = 3
    # text: decode_range_sync / _write
    host = _text(96 * MiB + 11, 0x57AE21)
    cb, n_symbols, stream, first_bit, spans = _split(_expected_image(host), ranks)
    text = _dev(host)
    ctxs = [E.Context(0) for _ in range(ranks)]
    try:
        infos = []
        for r, (c, (begin, end)) in enumerate(zip(ctxs, spans)):
            start = first_bit if r == 0 else (5 if r == 1 else -1)  # rank 1: a wrong start, repaired below
            with torch.cuda.stream(S[r % 2]):
                infos.append(c.decode_range_sync(cb, stream, begin, end, start))
        for _ in range(ranks + 2):
            prev, wrong = first_bit, []
            for i, inf in enumerate(infos):
                if inf["start_bit"] != prev:
                    wrong.append((i, prev))
                prev = inf["exit_bit"]
            if not wrong:
                break
            for i, w in wrong:
                with torch.cuda.stream(S[i % 2]):
                    infos[i] = ctxs[i].decode_range_sync(cb, stream, spans[i][0], spans[i][1], w)
        else:
            raise AssertionError("did not settle")
        outs, firsts, first = [], [], 0
        for r, (c, inf) in enumerate(zip(ctxs, infos)):
            take = max(0, min(inf["n_symbols"], n_symbols - first))
            buf = _out(take)
            with torch.cuda.stream(S[(r + 1) % 2]):
                assert c.decode_range_write(take, buf[: take + SLACK]) == take
            outs.append((buf, take, first))
            first += inf["n_symbols"]
        torch.cuda.synchronize()
        assert first >= n_symbols
        for buf, take, f in outs:
            _assert_output(buf, text[f:], take, f"text range at {f}")
    finally:
        for c in ctxs:
            c.close()

    # uniform bytes: decode_range_maps on one stream, _resolve and _write on the other
    host = flat(255, 64 * MiB + 13, 0x57AE22, lo=1)
    cb, n_symbols, stream, first_bit, spans = _split(_expected_image(host), ranks)
    text = _dev(host)
    ctxs = [E.Context(0) for _ in range(ranks)]
    try:
        maps = []
        for r, (c, (begin, end)) in enumerate(zip(ctxs, spans)):
            with torch.cuda.stream(S[r % 2]):
                m, n_starts = c.decode_range_maps(cb, stream, begin, end, first_bit if r == 0 else -1)
            assert n_starts == 8
            maps.append(m)
        outs, first, s_in = [], 0, first_bit
        for r, (c, m) in enumerate(zip(ctxs, maps)):
            with torch.cuda.stream(S[(r + 1) % 2]):
                inf = c.decode_range_resolve(s_in)
                assert inf["row_walk"] and inf["start_bit"] == s_in and inf["exit_bit"] == m[s_in], (inf, m[:8], s_in)
                take = max(0, min(inf["n_symbols"], n_symbols - first))
                buf = _out(take)
                assert c.decode_range_write(take, buf[: take + SLACK]) == take
            s_in = m[s_in]
            outs.append((buf, take, first))
            first += inf["n_symbols"]
        torch.cuda.synchronize()
        assert first >= n_symbols
        for buf, take, f in outs:
            _assert_output(buf, text[f:], take, f"uniform range at {f}")
    finally:
        for c in ctxs:
            c.close()


# --- e. close() --------------------------------------------------------------------------------------------------------------


def test_close_right_after_a_switch():
    """A large decode on A, a tiny call on B, close() at once: the context's teardown waits for A's write kernel too (it frees
    the workspaces that kernel reads).  A's output is the text."""
    import torch

    import entreepy_amd as E

    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    host = _text(128 * MiB + 17, 0x57AE31)
    image = _dev(np.frombuffer(_expected_image(host), dtype=np.uint8))
    text = _dev(host)
    small = _dev(corpus.text_like(4096, 0x57AE32))
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    out = _out(host.size)
    torch.cuda.synchronize()
    c = E.Context(0)
    try:
        with torch.cuda.stream(A):
            assert c.decode_device(image, out, skip=4) == host.size
        with torch.cuda.stream(B):
            c.histogram_device(small, hist)
    finally:
        c.close()
    torch.cuda.synchronize()
    _assert_output(out, text, host.size, "the decode on A")
    assert np.array_equal(hist.cpu().numpy(), np.bincount(small.cpu().numpy(), minlength=256))


# --- f. host and file calls ---------------------------------------------------------------------------------------------------


def test_host_and_file_calls_after_device_calls_elsewhere(tmp_path):
    """A device decode on a torch stream; use_own_stream(); host-memory decode / encode and a file decode on the same context
    (their staging and workspaces are rewritten while the device decode may still run); use_torch_stream() and one more device
    call.  Every result is the oracle's."""
    import torch

    import entreepy_amd as E

    O = _oracle()
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    big = _text(128 * MiB + 19, 0x57AE41)
    big_image = _dev(np.frombuffer(_expected_image(big), dtype=np.uint8))
    big_text = _dev(big)
    small = corpus.enwik_like(6 * MiB + 1, 0x57AE42)
    small_et = O.encode(small)
    path = tmp_path / "small.et"
    path.write_bytes(small_et)
    last = corpus.uniform(24 * MiB + 3, 0x57AE43, 1, 256)
    last_want = _expected_image(last)
    last_text = _dev(last)
    last_enc = torch.zeros(E.encode_bound(last.size) + 64, dtype=torch.uint8, device="cuda")
    out = _out(big.size)
    torch.cuda.synchronize()
    c = E.Context(0)
    try:
        with torch.cuda.stream(S1):
            assert c.decode_device(big_image, out, skip=4) == big.size
        c.use_own_stream()
        assert c.decode(small_et[4:]) == small.tobytes()
        assert c.encode(small) == small_et
        assert c.decode_file(str(path), str(tmp_path / "small.out")) == (len(small_et) - 4, small.size)
        assert (tmp_path / "small.out").read_bytes() == small.tobytes()
        with torch.cuda.stream(S2):
            c.use_torch_stream()
            m = c.encode_device(last_text, last_enc)
        torch.cuda.synchronize()
        _assert_output(out, big_text, big.size, "the device decode on S1")
        assert m == len(last_want) and last_enc[:m].cpu().numpy().tobytes() == last_want
    finally:
        c.close()
