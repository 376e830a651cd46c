"""GPU: the state a context keeps between calls survives another call, or the call that would read it is refused -- never a third
thing.  tests/retained.py holds the table: the two kinds of state (the link between et_histogram_device and the shard encode; the
range held between et_decode_range_sync / _maps + _resolve and et_decode_range_write), every other context call X at its
smallest size, and per (state, X) the ONE outcome expected.  Here every cell runs on a fresh context: the setter, X, the readers.

  keeps     the readers return ET_OK and give the reference's bytes (np.bincount, the oracle's packed body and image, the slice of
            the text that the serial walk of tests/bitwalk.py says begins in the range), nothing written outside them;
  drops     the readers return ET_ERR_ARG with the existing message about the missing first call, and every byte of their
            outputs still holds its sentinel;
  replaced  (a range call of another range) the write gives the NEW range's symbols.

tests/test_retained_host.py checks the table's completeness and the references without a GPU.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

from tests import retained as R
from tests.guards import Guarded

pytestmark = pytest.mark.gpu

ROWS = pytest.mark.parametrize("x", R.NAMES)


def _refused(call, reader):
    """The reader finds no first call: ET_ERR_ARG, and et_last_error says which call is missing."""
    import entreepy_amd as E

    with pytest.raises(E.EntreepyError) as e:
        call()
    assert e.value.status == R.ET_ERR_ARG and R.MISSING[reader] in str(e.value), f"{reader}: {e.value}"


def _untouched(*outs):
    for g in outs:
        dirty = g.check().first_dirty(0)
        assert dirty is None, f"a refused call wrote the byte at offset {dirty} of its output"


def _device_ptr(ctx):
    """et_histogram_device_ptr -> (status, the pointer, et_last_error)."""
    from entreepy_amd import _native as N

    p = ctypes.c_void_p()
    rc = N.lib().et_histogram_device_ptr(ctx._h, ctypes.byref(p))
    return rc, p.value, N.lib().et_last_error(ctx._h).decode()


def _read_counts(env, ptr):
    """256 x u64 at a device address that is no tensor's: one hipMemcpy of the runtime already in the process, the device drained."""
    env.torch.cuda.synchronize()
    hip = ctypes.CDLL(None)
    if not hasattr(hip, "hipMemcpy"):
        hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.restype, hip.hipMemcpy.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    counts = np.zeros(256, np.uint64)
    assert hip.hipMemcpy(counts.ctypes.data, ptr, 2048, 2) == 0  # hipMemcpyDeviceToHost
    return counts


def _words(image):
    """bytes -> the same, zero-padded to whole 32-bit words (a shard encode overwrites every word it touches)."""
    a = np.zeros((len(image) + 3) // 4 * 4, np.uint8)
    a[: len(image)] = np.frombuffer(image, np.uint8)
    return a


def _same_bytes(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: byte {int(bad[0])} of {want.size} is {int(got[bad[0]]):02x}, the reference has {int(want[bad[0]]):02x} ({bad.size} bytes differ)"


# ---- the histogram link ----------------------------------------------------------------------------------------------------------------


@ROWS
@pytest.mark.parametrize("reader", ["body", "head", "on_host"])
def test_histogram_link(x, reader):
    """et_histogram_device of 70 001 text-like bytes 3 bytes behind an aligned address, tiles of one round; X; then
      body     et_histogram_host, et_histogram_device_ptr, et_encode_body_device at start bit 5;
      head     et_encode_head_shard_device under the header of et_write_header;
      on_host  et_histogram_on_host with the true counts BEFORE X, the body encode after it.
    The outputs are 0xFF between guard bytes."""
    row = R.row(x)
    text = R.hist_text()
    counts, body, end_bit, image = R.hist_reference()
    cb = R.codebook_of("hist")
    header = cb.header(R.HIST_N)
    want_body, want_head = _words(body), _words(image)
    head_end = 8 * len(header) + end_bit - R.HIST_START_BIT
    with R.Env() as env:
        ctx, torch = env.ctx, env.torch
        d_text = env.at_offset(text, R.HIST_OFFSET)
        d_hist = torch.zeros(256, dtype=torch.int64, device="cuda")
        out_body, out_head = Guarded(want_body.size, fill=0xFF), Guarded(want_head.size, fill=0xFF)
        torch.cuda.synchronize()
        ctx.set_tile_rounds(R.HIST_ROUNDS)
        ctx.histogram_device(d_text, d_hist)
        if reader == "on_host":
            ctx.histogram_on_host(counts)
        row.run(env)
        body_call = lambda: ctx.encode_body_device(cb, d_text, out_body.room, R.HIST_START_BIT)
        head_call = lambda: ctx.encode_head_shard_device(cb, d_text, out_head.room, header)
        if row.hist == R.KEEPS:
            if reader == "head":
                assert head_call() == head_end
                _same_bytes(out_head.check().data(), want_head, "et_encode_head_shard_device against the oracle's image")
                out_head.assert_extent(want_head.size, "et_encode_head_shard_device")
            else:
                if reader == "body":
                    assert np.array_equal(ctx.histogram_host(), counts)
                    rc, ptr, _ = _device_ptr(ctx)
                    assert rc == R.ET_OK and np.array_equal(_read_counts(env, ptr), counts)
                assert body_call() == end_bit
                _same_bytes(out_body.check().data(), want_body, "et_encode_body_device against the oracle's pack_body")
                out_body.assert_extent(want_body.size, "et_encode_body_device")
            _untouched(out_body if reader == "head" else out_head)
        else:
            assert row.hist == R.DROPS
            if row.names:  # X took a histogram of its own: the link names THAT text, and the counts are that text's
                theirs = np.bincount(R.TEXTS[row.names](), minlength=256).astype(np.uint64)
                assert np.array_equal(ctx.histogram_host(), theirs)
                rc, ptr, _ = _device_ptr(ctx)
                assert rc == R.ET_OK and np.array_equal(_read_counts(env, ptr), theirs)
            else:
                _refused(ctx.histogram_host, "et_histogram_host")
                _refused(lambda: ctx.histogram_on_host(counts), "et_histogram_on_host")
                rc, _, err = _device_ptr(ctx)
                assert rc == R.ET_ERR_ARG and err == R.MISSING["et_histogram_device_ptr"]
            _refused(body_call, "et_encode_body_device")
            _refused(head_call, "et_encode_head_shard_device")
            _untouched(out_body, out_head)
        torch.cuda.synchronize()
        assert np.array_equal(d_hist.cpu().numpy().view(np.uint64), counts)  # what the setter itself gave stays what it was


# ---- the held range ----------------------------------------------------------------------------------------------------------------------

REPLACES = {"range_sync_other": "text", "range_maps_other": "rows"}  # the fixture whose other range such a row puts in place


def _triple(info):
    return info["start_bit"], info["exit_bit"], info["n_symbols"]


@ROWS
@pytest.mark.parametrize("how", ["sync", "maps", "between", "windows"])
def test_held_range(x, how):
    """Blocks 1..3 of a body of five 8 KiB blocks (the sparse stream: eight) and a ragged tail.
      sync     the text-like stream: et_decode_range_sync from an unknown start; X; et_decode_range_write;
      maps     the 255-value flat stream: et_decode_range_maps, et_decode_range_resolve; X; et_decode_range_write;
      between  the same, X between _maps and _resolve: "drops" means that _resolve is refused (and the write behind it);
      windows  the sparse dictionary's stream (tests/guards.py), whose range lies in the decode tables too: et_decode_range_sync by
               window sweeps from the true start; X; et_decode_range_write.
    What the setter reported is the walk's (start, exit, count); for "keeps" the resolve behind X reports it unchanged, and the
    write stores exactly that many symbols: the walk's."""
    row = R.row(x)
    name = {"sync": "text", "windows": "sparse"}.get(how, "rows")
    fx = R.range_fixture(name)
    begin, end = R.HELD
    s, exit_, n, syms = fx.truth(begin, end)
    want_n, want = n, syms
    if row.held == R.REPLACED:
        new = R.range_fixture(REPLACES[x])
        new_s, new_exit, want_n, want = new.truth(*R.other_range(REPLACES[x]))
    with R.Env() as env:
        ctx, torch = env.ctx, env.torch
        cb, d = fx.codebook(), env.streams[name]
        out = Guarded(want_n)
        torch.cuda.synchronize()
        if how == "sync":
            info = ctx.decode_range_sync(cb, d, begin, end, -1)
            assert _triple(info) == (s, exit_, n) and info["tree_walk"], info
        elif how == "windows":
            info = ctx.decode_range_sync(cb, d, begin, end, s)
            assert _triple(info) == (s, exit_, n) and not info["tree_walk"], info
        else:
            m, k = ctx.decode_range_maps(cb, d, begin, end, -1)
            assert k == 8 and m[s] == exit_, (list(m), s, exit_)
            if how == "maps":
                info = ctx.decode_range_resolve(s)
                assert _triple(info) == (s, exit_, n) and info["row_walk"], info
        row.run(env)
        write = lambda: ctx.decode_range_write(want_n, out.room)
        if row.held == R.DROPS:
            if how == "between":
                _refused(lambda: ctx.decode_range_resolve(s), "et_decode_range_resolve")
            _refused(write, "et_decode_range_write")
            _untouched(out)
            return
        if how == "between":
            if row.held == R.KEEPS:
                info = ctx.decode_range_resolve(s)
                assert _triple(info) == (s, exit_, n) and info["row_walk"], info
            elif REPLACES[x] == "rows":  # the new range came by the maps as well: it resolves again, to itself
                assert env.new_range == ("rows", *R.other_range("rows"), new_s)
                assert _triple(ctx.decode_range_resolve(new_s)) == (new_s, new_exit, want_n)
            else:  # the new range came by et_decode_range_sync: there are no maps to resolve
                _refused(lambda: ctx.decode_range_resolve(s), "et_decode_range_resolve")
        assert write() == want_n
        _same_bytes(out.check().data(), want, f"et_decode_range_write against the walk of the {'new' if row.held == R.REPLACED else 'held'} range")
        out.assert_extent(want_n, "et_decode_range_write")


# ---- the last codebook -------------------------------------------------------------------------------------------------------------------


@ROWS
def test_last_codebook(x):
    """et_last_codebook behind et_encode_device(text A) and X: the oracle's build_dict of A, unless X is itself a whole encode --
    then of X's text."""
    row = R.row(x)
    data, length = R.table_of(row.encodes or "hist")
    with R.Env() as env:
        ctx, torch = env.ctx, env.torch
        d_text = env.dev(R.hist_text())
        out = torch.empty(env.E.encode_bound(R.HIST_N), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n = ctx.encode_device(d_text, out)
        row.run(env)
        cb = ctx.last_codebook()
        assert np.array_equal(cb.length, length) and np.array_equal(cb.data[length > 0], data[length > 0])
        torch.cuda.synchronize()
        assert out[:n].cpu().numpy().tobytes() == R.hist_reference()[3]


# ---- both kinds of state at once -----------------------------------------------------------------------------------------------------


def test_the_two_kinds_of_state_do_not_disturb_each_other():
    """histogram -> range sync -> packed decode -> body encode -> range write on one context, nothing between them from this side:
    the body is the oracle's, the symbols are the walk's, the records are the store's."""
    text = R.hist_text()
    counts, body, end_bit, _ = R.hist_reference()
    fx = R.range_fixture("text")
    s, exit_, n, syms = fx.truth(*R.HELD)
    _, _, blob, index, lengths = R.store()
    text_index = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    with R.Env() as env:
        ctx, torch = env.ctx, env.torch
        d_text = env.at_offset(text, R.HIST_OFFSET)
        d_hist = torch.zeros(256, dtype=torch.int64, device="cuda")
        d_blob, d_body_index = ctx._packed_upload(np.frombuffer(blob, np.uint8).copy(), index)
        d_text_index = torch.from_numpy(text_index.view(np.int64)).cuda()
        want_body = _words(body)
        out_body, out_syms, out_records = Guarded(want_body.size, fill=0xFF), Guarded(n), Guarded(int(text_index[-1]))
        cb, store_cb, range_cb = R.codebook_of("hist"), env.store_cb(), fx.codebook()
        torch.cuda.synchronize()
        ctx.histogram_device(d_text, d_hist)
        info = ctx.decode_range_sync(range_cb, env.streams["text"], *R.HELD, -1)
        res = ctx.decode_packed_device(store_cb, d_blob, d_body_index, d_text_index, out_records.room)
        end = ctx.encode_body_device(cb, d_text, out_body.room, R.HIST_START_BIT)
        m = ctx.decode_range_write(n, out_syms.room)
        assert _triple(info) == (s, exit_, n) and (res.status, res.n_failed, res.n_short) == (R.ET_OK, 0, 0) and end == end_bit and m == n
        _same_bytes(out_body.check().data(), want_body, "et_encode_body_device")
        _same_bytes(out_syms.check().data(), syms, "et_decode_range_write")
        assert out_records.check().data().tobytes() == b"".join(R.RECORDS)
        for g, size in ((out_body, want_body.size), (out_syms, n), (out_records, int(text_index[-1]))):
            g.assert_extent(size, "a call of the sequence")
        assert np.array_equal(ctx.histogram_host(), counts)
