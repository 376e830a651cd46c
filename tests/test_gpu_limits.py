"""GPU: the kernels at the worst cases their buffers, loop bounds and branches are sized for (tests/limits.py; that the inputs
reach those cases is checked on the host, tests/test_limits_host.py).  Bit-exact against the oracle (pack_body, encode, decode)
or the text itself, through the C ABI.

  K4's three append paths (whole quads, pairs, single symbols), each at its edge, chosen on purpose rather than by chance;
  K4's rings with every symbol of a round at the longest code (4096 words for codes up to 31 bits, 8192 for 32, the long kernel's);
  the single-stream decode's chained write with 32-bit codewords in full trees, through plans of 2, 3 and 8 index bits;
  the same streams through the whole-stream, batched, shared-table and range calls;
  trees of 31, 32 and 33 levels behind the host's own code construction."""
import functools

import numpy as np
import pytest

from tests import limits as L
from tests.guards import Guarded
from tests.test_gpu_batch import Batch, _small_max
from tests.test_gpu_shared import roundtrip

pytestmark = pytest.mark.gpu

UNSUPPORTED = 7  # et_status


def _oracle():
    from oracle import oracle as O

    return O


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).copy()).cuda()


def _at_offset(a, off):
    """The bytes on the device as a view that begins `off` bytes behind an aligned address."""
    import torch

    a = np.frombuffer(bytes(a), np.uint8) if not isinstance(a, np.ndarray) else a
    buf = torch.zeros(off + a.size + 16, dtype=torch.uint8, device="cuda")
    buf[off : off + a.size] = torch.from_numpy(a.copy()).cuda()
    view = buf[off : off + a.size]
    assert view.data_ptr() % 16 == off % 16
    return view


def _encode_body(ctx, t, cb, d_text, text, start_bit, what, fill=0xFF):
    """et_encode_body_device into a buffer of `fill` against pack_body into a zeroed one: end bit, every byte from the word of
    start_bit to the last word, and the fill behind the last word."""
    import torch

    want, want_end = _oracle().pack_body(t.data, t.length, text, start_bit)
    n_words = (want_end + 31) // 32
    out = torch.full((n_words * 4 + 64,), fill, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    ctx.histogram_device(d_text, hist)
    end = ctx.encode_body_device(cb, d_text, out, start_bit)
    torch.cuda.synchronize()
    assert end == want_end, (what, end, want_end)
    got = out.cpu().numpy()
    image = np.zeros(n_words * 4, np.uint8)
    image[: len(want)] = np.frombuffer(want, np.uint8)
    first = start_bit // 32
    gw, ww = got[: n_words * 4].view(">u4")[first:], image.view(">u4")[first:]
    bad = np.flatnonzero(gw != ww)
    assert bad.size == 0, (f"{what}: word {first + int(bad[0])} of {n_words} is {int(gw[bad[0]]):08x}, the oracle's pack_body has {int(ww[bad[0]]):08x} "
                           f"({bad.size} words differ, the last of them word {first + int(bad[-1])})")
    assert bool((got[n_words * 4 :] == fill).all()), f"{what}: a byte behind the body's last word was written"


# --- part 3: K4's three paths -------------------------------------------------------------------------------------------------------

START_BITS = (0, 1, 31)  # 32-bit appends with fill == 0 and with fill != 0


@pytest.mark.parametrize("path,quad", L.K4_PATTERNS, ids=[f"{p}-{L.pattern_id(q)}" for p, q in L.K4_PATTERNS])
def test_k4_append_paths_at_their_edges(ctx, path, quad):
    """One quad pattern of code lengths (ladder32, Z = a byte without a code) filling whole rounds, and as ONE chunk among chunks
    of 1-bit symbols at lanes 0, 31, 63 and 255 and in each quad position -- one lane's ballot then sends its whole wavefront
    down the rarer path.  Two rounds and 17 bytes, start bits 0, 1 and 31, the text once as a view 3 bytes behind an aligned
    address."""
    t = L.ladder32()
    cb = t.codebook()
    texts = [("whole rounds", L.k4_whole_rounds(t, quad, L.K4_N))]
    texts += [(f"one chunk at lane {lane}, quad {pos}", L.k4_one_chunk(t, quad, L.K4_N, lane, pos)) for lane in L.K4_LANES for pos in range(4)]
    for placement, text in texts:
        d_text = _dev(text)
        for start_bit in START_BITS:
            _encode_body(ctx, t, cb, d_text, text, start_bit, f"pattern {list(quad)} ({path} path), {placement}, start bit {start_bit}")
    for placement, text in texts[:2]:
        _encode_body(ctx, t, cb, _at_offset(text, 3), text, 1, f"pattern {list(quad)} ({path} path), {placement}, text at byte offset 3, start bit 1")


# --- part 4: ring saturation -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,text_name", L.RING_PAIRS, ids=[f"{a}-{b}" for a, b in L.RING_PAIRS])
def test_rounds_of_longest_codes_fill_the_ring(ctx, name, text_name):
    """Every symbol of a round at the table's longest code: 4096 x 31 bits into the 4096-word ring, 4096 x 32 into the 8192-word
    ring, steps of 256 x 255 bits into the long kernel's; and such rounds alternating with rounds of 4096 bits.  Five rounds
    and 17 bytes as tiles of 1, 2 and 8 rounds, start bits 0, 1 and 31, into a buffer of 0xFF."""
    t = L.table(name)
    cb = t.codebook()
    text = L.text_of(name, text_name, L.RING_N)
    d_text = _dev(text)
    try:
        for rounds in (1, 2, 8):
            ctx.set_tile_rounds(rounds)
            for start_bit in START_BITS:
                _encode_body(ctx, t, cb, d_text, text, start_bit, f"{text_name}({name}), tiles of {rounds} rounds, start bit {start_bit}")
    finally:
        ctx.set_tile_rounds(0)


# --- part 5: decode at the limit -------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _packed(name, text_name, n, start_bit=0):
    """-> (text, header, body): body = pack_body at start_bit, header = Codebook.header."""
    t = L.table(name)
    text = L.text_of(name, text_name, n)
    return text, t.codebook().header(n), _oracle().pack_body(t.data, t.length, text, start_bit)[0]


def _decode_body(ctx, cb, body, n_symbols, start_bit, out):
    """et_decode_body_device of the body one byte behind an aligned address -> (symbols, the decode's timing flags)."""
    import torch

    m = ctx.decode_body_device(cb, _at_offset(body, 1), n_symbols, out, start_bit)
    torch.cuda.synchronize()
    return m, ctx.timings("decode")


@pytest.mark.parametrize("name,text_name", L.DECODE_PAIRS, ids=[f"{a}-{b}" for a, b in L.DECODE_PAIRS])
def test_body_decode_of_32_bit_codes_in_full_trees(ctx, name, text_name):
    """et_decode_body_device: the chained write (k_dec_write_wave) with codewords of 31 and 32 bits at every bit offset, through
    sub-tables of 8 (ladders, broom), 3 (comb8) and 2 (comb11) index bits; start bits 0 and 5, the body at a pointer offset of 1."""
    import torch

    t = L.table(name)
    cb = t.codebook()
    guarded = (name, text_name) in (("ladder32", "dense"), ("comb11", "uniform"))
    ctx.enable_timing(True)
    try:
        for start_bit in (0, 5):
            text, _, body = _packed(name, text_name, L.DECODE_N, start_bit)
            g = Guarded(text.size) if guarded else None
            out = g.room if guarded else torch.full((text.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            m, flags = _decode_body(ctx, cb, body, text.size, start_bit, out)
            what = f"{text_name}({name}), start bit {start_bit}"
            assert m == text.size, (what, m)
            got = out[:m].cpu().numpy()
            bad = np.flatnonzero(got != text)
            assert bad.size == 0, f"{what}: symbol {int(bad[0])} is {int(got[bad[0]])}, the text has {int(text[bad[0]])} ({bad.size} of {m} differ)"
            assert flags["chained_write"], (what, flags)
            if guarded:
                g.check().assert_extent(m, what)
            else:
                assert bool((out[m:] == 0xA5).all()), f"{what}: a byte behind the last symbol was written"
    finally:
        ctx.enable_timing(False)


@pytest.mark.parametrize("name,text_name", L.COLD_PAIRS, ids=[f"{a}-{b}" for a, b in L.COLD_PAIRS])
def test_short_declarations_and_truncated_bodies(ctx, name, text_name):
    """A declared length one short, and the image cut by 1, 2, 3, 4, 5 and 33 bytes: what the oracle's decode gives, through
    et_decode_body_device and et_decode_device."""
    import torch

    O = _oracle()
    t = L.table(name)
    cb = t.codebook()
    text, header, body = _packed(name, text_name, L.DECODE_N)
    n = text.size
    cases = [("declared length one short", cb.header(n - 1), body, n - 1)]
    cases += [(f"cut by {cut} bytes", header, body[: len(body) - cut], n) for cut in (1, 2, 3, 4, 5, 33)]
    for what, head, part, declared in cases:
        want = O.decode((head + part)[4:])
        assert 0 < len(want) <= declared and want == text[: len(want)].tobytes() and (len(want) < n)
        out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        m, _ = _decode_body(ctx, cb, part, declared, 0, out)
        assert m == len(want) and out[:m].cpu().numpy().tobytes() == want, (name, text_name, what, "et_decode_body_device", m, len(want))
        assert bool((out[m:] == 0xA5).all()), (what, "et_decode_body_device wrote behind its last symbol")
        out.fill_(0xA5)
        m = ctx.decode_device(_dev(np.frombuffer((head + part)[4:], np.uint8)), out)
        torch.cuda.synchronize()
        assert m == len(want) and out[:m].cpu().numpy().tobytes() == want, (name, text_name, what, "et_decode_device", m, len(want))
        assert bool((out[m:] == 0xA5).all()), (what, "et_decode_device wrote behind its last symbol")


@pytest.mark.parametrize("name", L.DECODE_TABLES)
def test_whole_stream_and_batched_decode_of_the_same_images(ctx, name):
    """header + body through et_decode_device, and all of a table's images through et_decode_batch_device in one batch (the
    batch kernels: path 0)."""
    import torch

    packed = [_packed(name, text_name, L.DECODE_N) for text_name in L.DECODE_TEXTS]
    for text_name, (text, header, body) in zip(L.DECODE_TEXTS, packed):
        out = torch.full((text.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        m = ctx.decode_device(_dev(np.frombuffer((header + body)[4:], np.uint8)), out)
        torch.cuda.synchronize()
        assert m == text.size and out[:m].cpu().numpy().tobytes() == text.tobytes(), (name, text_name, m)
        assert bool((out[m:] == 0xA5).all()), (name, text_name)
    b = Batch([(header + body)[4:] for _, header, body in packed], [text.size for text, _, _ in packed], lead=3).run(ctx.decode_batch_device)
    b.assert_nothing_outside()
    assert not b.status.any() and not b.path.any(), (list(b.status), list(b.path))
    for i, (text, _, _) in enumerate(packed):
        assert b.out_len[i] == text.size and b.result(i) == text.tobytes(), (name, L.DECODE_TEXTS[i])


@pytest.mark.parametrize("name", L.DECODE_TABLES)
def test_shared_table_calls_on_the_same_texts(ctx, name):
    """et_encode_shared_device against pack_body, et_decode_shared_device of its bodies against the oracle's decode and the
    texts; the outputs at address residues 0 .. 3 between sentinels."""
    t = L.table(name)
    texts = [L.text_of(name, text_name, L.DECODE_N) for text_name in L.DECODE_TEXTS]
    texts.append(texts[1][: L.DECODE_N // 2 + 1])
    enc, dec = roundtrip(ctx, t.tab, texts, out_res=[0, 1, 2, 3])
    assert not enc.status.any() and not dec.status.any()
    assert {(enc.d_out.data_ptr() + int(o)) % 4 for o in enc.out_off} == {0, 1, 2, 3}
    assert [dec.result(b) for b in range(4)] == [x.tobytes() for x in texts]


def test_the_longest_record_a_batched_stream_can_have(ctx):
    """et_batch_small_max() symbols of 32 bits each: a body of 1 MiB, 128 blocks, through the shared encode, the shared decode
    and the batched decode."""
    t = L.broom32()
    n = _small_max()
    text = L.dense(t, n, seed=0x11A179)
    enc, dec = roundtrip(ctx, t.tab, [text])
    assert enc.out_len[0] == n * 4 == 1 << 20 and dec.out_len[0] == n and dec.result(0) == text.tobytes()
    image = t.codebook().header(n) + enc.result(0)
    b = Batch([image[4:]], [n], lead=3).run(ctx.decode_batch_device)
    b.assert_nothing_outside()
    assert list(b.status) == [0] and list(b.path) == [0] and b.out_len[0] == n
    assert b.result(0) == text.tobytes()


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("name,text_name", L.COLD_PAIRS, ids=[f"{a}-{b}" for a, b in L.COLD_PAIRS])
def test_cold_ranges_cut_through_32_bit_codewords(name, text_name, ranks):
    """et_decode_range_sync / _write over block ranges of one stream, one et_ctx per range, the exchange by hand as
    test_gpu_cli_dist.py's test_cold_decode_virtual_ranks does it (a forced wrong start included): every range's symbols are
    its slice of the text, and a 32-bit codeword lies across a range boundary."""
    import torch

    import entreepy_amd as E

    t = L.table(name)
    text, header, body = _packed(name, text_name, L.COLD_N)
    image = (header + body)[4:]
    comp = _dev(np.frombuffer(image, np.uint8))
    cb, n_symbols, body_off = E.parse_header(image)
    assert n_symbols == text.size and np.array_equal(cb.length, t.length) and np.array_equal(cb.data, t.data)
    ptr = comp.data_ptr() + body_off
    base_off, first_bit = body_off - (ptr & 3), (ptr & 3) * 8
    stream = comp[base_off:]
    n_blocks = (stream.numel() + 8191) // 8192
    assert n_blocks >= 4
    bits = t.bits(text)
    begins = L.starts(t, text, first_bit)
    ctxs, infos, spans = [], [], []
    try:
        for r in range(ranks):
            lo, hi = r * n_blocks // ranks, (r + 1) * n_blocks // ranks
            c = E.Context(0)
            c.use_torch_stream()
            ctxs.append(c)
            begin, end = lo * 8192, min(hi * 8192, stream.numel())
            start = first_bit if lo == 0 else (5 if r == 1 else -1)  # (rank 1: a wrong start, repaired below)
            infos.append(c.decode_range_sync(cb, stream, begin, end, start))
            spans.append((begin, end))
        cut = [b * 8 for b, _ in spans[1:]]
        assert any(bool(((begins < at) & (begins + bits > at) & (bits == 32)).any()) for at in cut), "no 32-bit codeword across a range boundary"
        for _ in range(ranks + 2):
            prev, wrong = first_bit, []
            for i, inf in enumerate(infos):
                if inf["start_bit"] != prev:
                    wrong.append((i, prev))
                prev = inf["exit_bit"]
            if not wrong:
                break
            for i, w in wrong:
                infos[i] = ctxs[i].decode_range_sync(cb, stream, spans[i][0], spans[i][1], w)
        else:
            raise AssertionError("did not settle")
        first = 0
        for r, (c, inf) in enumerate(zip(ctxs, infos)):
            take = max(0, min(inf["n_symbols"], n_symbols - first))
            buf = torch.full((inf["n_symbols"] + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            m = c.decode_range_write(take, buf)
            torch.cuda.synchronize()
            assert m == take and buf[:m].cpu().numpy().tobytes() == text[first : first + m].tobytes(), (name, text_name, ranks, r, first, m)
            first += inf["n_symbols"]
        assert first >= n_symbols
    finally:
        for c in ctxs:
            c.close()


# --- part 6: 31, 32 and 33 levels behind the host's own code construction ------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _fibonacci(max_len):
    text = L.fibonacci_text(max_len)
    text.setflags(write=False)
    return text, _oracle().encode(text)


def _max_length(image):
    import entreepy_amd as E

    return int(E.parse_header(image[4 : 4 + 8192])[0].raw.max_length)


def _encode_whole(ctx, text, image):
    import torch

    import entreepy_amd as E

    out = torch.full((E.encode_bound(text.size),), 0xFF, dtype=torch.uint8, device="cuda")
    n = ctx.encode_device(_dev(text), out)
    torch.cuda.synchronize()
    got = out[:n].cpu().numpy().tobytes()
    assert n == len(image) and got == image, f"encode of {text.size} bytes: {n} bytes against the oracle's {len(image)}, the first difference at byte {next((i for i, (a, b) in enumerate(zip(got, image)) if a != b), min(n, len(image)))}"
    return out, n


def _decode_whole(ctx, d_image, n_image, text, image):
    import torch

    out = torch.full((text.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    m = ctx.decode_device(d_image, out, skip=4, length=n_image - 4)
    torch.cuda.synchronize()
    want = _oracle().decode(image[4:])
    assert want == text.tobytes()
    assert m == text.size and out[:m].cpu().numpy().tobytes() == want
    assert bool((out[m:] == 0xA5).all())


@pytest.mark.parametrize("max_len", [31, 32])
def test_whole_calls_on_trees_of_31_and_32_levels(ctx, max_len):
    """et_encode_device (the 4096- and the 8192-word ring behind et_build_codebook) and et_decode_device against the oracle."""
    text, image = _fibonacci(max_len)
    assert _max_length(image) == max_len
    d_image, n = _encode_whole(ctx, text, image)
    _decode_whole(ctx, d_image, n, text, image)


def test_a_tree_of_33_levels_encodes_and_is_declined_by_the_decode(ctx):
    """The long kernel behind et_build_codebook: the image is the oracle's; the decode declines it (ET_ERR_UNSUPPORTED) and the
    same context then decodes the 32-level stream."""
    import torch

    import entreepy_amd as E

    text, image = _fibonacci(33)
    d_image, n = _encode_whole(ctx, text, image)
    assert int(ctx.last_codebook().raw.max_length) == 33
    out = torch.full((text.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EntreepyError) as e:
        ctx.decode_device(d_image, out, skip=4, length=n - 4)
    assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()), "a declined decode wrote something"
    text32, image32 = _fibonacci(32)
    _decode_whole(ctx, _dev(np.frombuffer(image32, np.uint8)), len(image32), text32, image32)
