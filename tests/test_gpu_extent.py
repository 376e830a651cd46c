"""GPU: what every single-stream device call may WRITE, and what it answers when the output is too small.

Output buffers belong to the caller.  Every output here is a tests/guards.py Guarded buffer: 64 bytes of 0xA5 on either side
of the usable part, which begins on a 16-byte boundary.  After a torch.cuda.synchronize() the bytes a call produced are compared
with the oracle's, and the bytes it had no business with must still be 0xA5 -- in front of d_out, from *out_len on, at and past
d_out + cap.

  A. decode extent, one family per write kernel, at ragged lengths and at declared lengths shorter than the body;
  B. ET_ERR_CAP of every single-stream call (nothing written, *out_len == 0, the context sound afterwards), exact capacities,
     truncated bodies (the write that is not speculative), the range write, the shard encode's words;
  C. the write kernels behind ET_NO_STRIPS / ET_NO_ROW_WRITE / ET_NO_FIXED_WRITE / ET_NO_ROW_SYNC, and the window tables'
     families behind ET_DEC_TABLES_HOST, one child process each.

Every family decodes with ONE code table -- the reference builder's for the family's byte distribution, or a hand-made one --
and a body the oracle packs from the first n bytes of the family's text, so that every length, n = 1 included, reaches the
family's kernel.  Families whose table fits a header are decoded as an image (the oracle's header in front: decode_device),
the hand-made ones through decode_body_device.  What ran is asserted from Context.timings("decode") in a second, timed call
of the same input; the untimed call is the one whose extent is checked.

MEASURED on an MI355X: no decode write kernel uses slack behind *out_len -- k_dec_write_wave and its strips instantiation,
k_row_write, k_fixed_write and the round-1 k_dec_write / k_dec_write_reg keep to [d_out, d_out + *out_len) at every length
here -- so every assertion below is the strict one (slack=0), and include/entreepy_hip.h and DESIGN.md §2 promise it.
That the guards see an over-store is shown once, for the chained write, in DESIGN.md §2."""
import ctypes
import functools
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

from tests import corpus
from tests.conftest import ROOT
from tests.guards import Guarded, _random_prefix_code, _sparse_dictionary
from tests.test_gpu_rowsync import flat
from tests.test_gpu_strips import sparse

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 15, 16, 17, 31, 33, 4095, 4096, 4097, 65_537)
OWN = 200_003  # every family's own length
UNSET = 0x5EED  # what *out_len holds before a call: a refused call must store 0 itself
FLAG_KEYS = ("exhaustive_sync", "tree_walk_sync", "chained_write", "row_sync", "fixed_sync", "strips_write")

# kind: "image" (decode_device of header + body) or "body" (decode_body_device); base: the family's text; path: et_decode_path;
# flags: what timings("decode") must say; lengths: the n of part A; fulls: the body lengths of the declared-length matrix
Family = namedtuple("Family", "name kind cb base path flags lengths fulls")


def _oracle():
    from oracle import oracle as O

    return O


def _dev(b):
    import torch

    return torch.frombuffer(bytearray(b) if len(b) else bytearray(1), dtype=torch.uint8)[: len(b)].cuda()


@functools.lru_cache(maxsize=None)
def _family(name):
    import entreepy_amd as E
    from entreepy_amd import _native as N

    def hist_code(h):
        return E.Codebook.from_histogram(np.asarray(h, dtype=np.uint64))

    def flat_hist(lo, k, w):
        h = np.zeros(256, dtype=np.uint64)
        h[lo : lo + k] = w
        return h

    all_lengths = LENGTHS + (OWN,)
    if name == "chained":  # k_dec_write_wave<8>: the chained-table windows
        base = corpus.text_like(OWN, 0xE701)
        return Family(name, "image", hist_code(np.bincount(base, minlength=256)), base, N.ET_PATH_TREE_WALK,
                      dict(tree_walk_sync=True, chained_write=True, strips_write=False, row_sync=False, fixed_sync=False, exhaustive_sync=False), all_lengths, (OWN,))
    if name == "strips":  # k_dec_write_wave<8, true>: n_symbols / 128 > n_subs, which no shorter stream of this code reaches
        base = sparse(OWN, 0.97, 0xE702)
        return Family(name, "image", hist_code(np.bincount(base, minlength=256)), base, N.ET_PATH_TREE_WALK,
                      dict(tree_walk_sync=True, chained_write=True, row_sync=False, fixed_sync=False), (4095, 4096, 4097, 65_537, OWN), (OWN,))
    if name == "rows":  # k_row_write
        return Family(name, "image", hist_code(flat_hist(1, 255, 100)), flat(255, OWN, 0xE703, lo=1), N.ET_PATH_ROWS,
                      dict(row_sync=True, exhaustive_sync=True, fixed_sync=False, tree_walk_sync=False), all_lengths, (OWN,))
    if name.startswith("fixed") and name != "fixed256":  # k_fixed_write, L = 1, 2, 4, 6
        k = int(name[5:])
        return Family(name, "image", hist_code(flat_hist(10, k, 50)), flat(k, OWN, 0xE704 + k, lo=10), N.ET_PATH_FIXED,
                      dict(fixed_sync=True, exhaustive_sync=True, row_sync=False), all_lengths, (OWN,))
    if name == "fixed256":  # k_fixed_write, L = 8: a code no encoder makes (tests/test_gpu_fixedsync.py)
        rng = np.random.default_rng(8)
        cb = E.Codebook.from_tables(rng.permutation(256).astype(np.uint32), np.full(256, 8, dtype=np.uint8))
        return Family(name, "body", cb, rng.integers(0, 256, size=OWN).astype(np.uint8), N.ET_PATH_FIXED,
                      dict(fixed_sync=True, exhaustive_sync=True, row_sync=False), all_lengths, (OWN,))
    if name == "exitmaps":  # the exit maps with the chained write behind them: 31 symbols of equal weight (tests/test_host_logic.py: 'M')
        return Family(name, "image", hist_code(flat_hist(0, 31, 1000)), flat(31, OWN, 0xE705, lo=0), N.ET_PATH_EXIT_MAPS,
                      dict(exhaustive_sync=True, chained_write=True, row_sync=False, fixed_sync=False, tree_walk_sync=False), all_lengths, (OWN,))
    if name == "round1":  # k_dec_write alone (<= 3 blocks: 4 000), k_dec_write_reg (60 000), behind k_dec_sync_reg2 (2 000 000)
        # (et_timings has no flag for the round-1 kernels: all that the flags below say is "none of the later paths".  Which of the
        # three kernels a size reaches follows from the thresholds in et_kernels_fallback.hip alone; if the planner moved a size
        # to another of them, this matrix would not notice.)
        data_t, len_t, syms = _sparse_dictionary()
        n = 2_000_000
        rng = np.random.default_rng(n)
        base = syms[np.minimum(rng.integers(0, 300, size=n), syms.size - 1) % syms.size].astype(np.uint8)
        base[rng.random(n) < 0.5] = 32  # half of it the 2-bit code: the stream re-synchronises
        return Family(name, "body", E.Codebook.from_tables(data_t, len_t), base, N.ET_PATH_WINDOWS,
                      dict(tree_walk_sync=False, chained_write=False, exhaustive_sync=False, row_sync=False, fixed_sync=False), all_lengths + (4_000, 60_000, n), (4_000, OWN))
    raise KeyError(name)


FAMILIES = ("chained", "strips", "rows", "fixed2", "fixed4", "fixed16", "fixed64", "fixed256", "exitmaps", "round1")


def _path(cb):
    from entreepy_amd import _native as N

    p = ctypes.c_uint32(99)
    assert N.lib().et_decode_path(ctypes.byref(cb.raw), ctypes.byref(p)) == N.ET_OK
    return p.value


def _stream(fam, n, declared=None):
    """(what the decode reads, host bytes; byte offset of the body in it): the first n bytes of the family's text packed by the
    oracle, behind the oracle's header for an image -- whose length field says `declared` (default: n)."""
    O = _oracle()
    body, _ = O.pack_body(fam.cb.data, fam.cb.length, fam.base[:n], 0)
    if fam.kind == "body":
        return body, 0
    head = O.write_header(fam.cb.data, fam.cb.length, n if declared is None else declared)[4:]
    return head + body, len(head)


def _timed_flags(ctx, call):
    ctx.enable_timing(True)
    try:
        call()
        return ctx.timings("decode")
    finally:
        ctx.enable_timing(False)


def _n_subs(d_stream, body_off):
    a = d_stream.data_ptr() + body_off
    return ((a & 3) + d_stream.numel() - body_off) * 8 // 256 + (1 if ((a & 3) + d_stream.numel() - body_off) * 8 % 256 else 0)


def _check_extent(ctx, fam, n, declared=None, flags=None):
    """Part A for one stream: n symbols in the body, `declared` of them asked for (default: all).  The output has room for the
    whole body and 32 bytes more, all inside cap, so a kernel that used slack behind *out_len would be allowed to and is seen."""
    import torch

    O = _oracle()
    take = n if declared is None else declared
    what = f"{fam.name} n={n} declared={take}"
    assert _path(fam.cb) == fam.path, what
    stream, body_off = _stream(fam, n, declared)
    want = fam.base[:take].tobytes()
    if fam.kind == "image":
        assert O.decode(stream) == want, what  # (the oracle's intended decode is the text)
    d_stream = _dev(stream)
    g = Guarded(n + 32)

    def decode(out):
        if fam.kind == "image":
            return ctx.decode_device(d_stream, out)
        return ctx.decode_body_device(fam.cb, d_stream, take, out)

    m = decode(g.room)
    g.check()
    assert m == take, what
    assert g.data(m).tobytes() == want, f"{what}: wrong bytes"
    g.assert_extent(m, what)
    t = _timed_flags(ctx, lambda: decode(torch.empty(n + 32, dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    expect = dict(fam.flags if flags is None else flags)
    if fam.name == "strips" and "strips_write" not in expect:
        expect["strips_write"] = take // 128 > _n_subs(d_stream, body_off)
        if declared is None:
            assert expect["strips_write"], f"{what}: too short for the strips"
    for k, v in expect.items():
        assert t[k] == v, (what, k, {f: t[f] for f in FLAG_KEYS})


# --- A. decode extent ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", FAMILIES)
def test_decode_writes_its_symbols_and_nothing_else(ctx, name):
    """out[:n] is the text; the 64 bytes in front of d_out and every byte from *out_len on -- 32 of them inside cap -- keep their
    0xA5, at every ragged length of the family's list."""
    fam = _family(name)
    for n in fam.lengths:
        _check_extent(ctx, fam, n)


@pytest.mark.parametrize("name", FAMILIES)
def test_declared_length_shorter_than_the_body_clamps_the_write(ctx, name):
    """The same with a declared length shorter than the body (the header's length field, bytes 1..4 of the stream; n_symbols for
    the hand-made tables): the bytes between `declared` and the body's full length stay 0xA5.  (Through ctx.decode the
    library's own workspace hides this.)  The strips take a clamped quarter by windows, and a declared count too small for
    the planner's rule picks the windows' instantiation: the flag is asserted to follow n_symbols / 128 > n_subs."""
    fam = _family(name)
    for full in fam.fulls:
        for declared in (1, 15, 16, 17, 4096, 4097, full - 17, full - 1):
            if declared < full:  # (the 4 000-symbol body of round1 has no 4096)
                _check_extent(ctx, fam, full, declared)


# --- B. capacity ----------------------------------------------------------------------------------------------------------------


def _last_error(c):
    from entreepy_amd import _native as N

    return N.lib().et_last_error(c._h).decode()


def _raw_decode(c, fam, d_stream, n_symbols, ptr, cap, body_call):
    """et_decode_device, or et_decode_body_device on the same stream's body (body_call; always for the hand-made tables)."""
    import entreepy_amd as E
    from entreepy_amd import _native as N

    c._bind()
    got = ctypes.c_size_t(UNSET)
    if fam.kind == "image" and not body_call:
        rc = N.lib().et_decode_device(c._h, d_stream.data_ptr(), d_stream.numel(), ptr, cap, ctypes.byref(got))
    else:
        cb, off = fam.cb, 0
        if fam.kind == "image":
            cb, n_symbols, off = E.parse_header(d_stream[:8192].cpu().numpy().tobytes())
        rc = N.lib().et_decode_body_device(c._h, ctypes.byref(cb.raw), d_stream.data_ptr() + off, d_stream.numel() - off, 0, n_symbols, ptr, cap, ctypes.byref(got))
    return rc, got.value


def _assert_sound(c, other, seed):
    """The next calls on the same context: a decode of another family and an encode, both the oracle's bytes."""
    import entreepy_amd as E

    O = _oracle()
    fam = _family(other)
    n = 70_001
    stream, _ = _stream(fam, n)
    d_stream = _dev(stream)
    g = Guarded(n)
    m = c.decode_device(d_stream, g.room) if fam.kind == "image" else c.decode_body_device(fam.cb, d_stream, n, g.room)
    text = corpus.text_like(50_001, seed)
    e = Guarded(E.encode_bound(text.size))
    k = c.encode_device(_dev(text.tobytes()), e.room)
    g.check()
    e.check()
    assert m == n and g.data(m).tobytes() == fam.base[:n].tobytes(), f"the decode of {other} after a refused call"
    g.assert_extent(m, f"the decode of {other} after a refused call")
    want = O.encode(text)
    assert k == len(want) and e.data(k).tobytes() == want, "the encode after a refused call"
    e.assert_extent(e.n, "the encode after a refused call")


CAP_FAMILIES = (("chained", "rows"), ("rows", "fixed16"), ("fixed16", "exitmaps"), ("exitmaps", "chained"))  # (family, the other family decoded afterwards)


@pytest.mark.parametrize("body_call", [False, True], ids=["et_decode_device", "et_decode_body_device"])
@pytest.mark.parametrize("name,other", CAP_FAMILIES)
def test_decode_refuses_a_small_output_and_writes_nothing(name, other, body_call):
    """cap = n_out - 1 and cap = 0: ET_ERR_CAP from the check behind the synchronisation (et_decode.cpp, "output buffer too
    small": with cap < n_symbols no speculative write was launched, so it stands in front of the only write), *out_len == 0, not
    one byte of the buffer or its guards touched.  Then cap = n_out exactly: ET_OK under part A's assertions -- the refused
    calls left the pinned blocks' turn, the report epoch and the write's ticket as the next decode needs them -- and a decode
    of another family and an encode on the same context."""
    import entreepy_amd as E
    from entreepy_amd import _native as N

    fam = _family(name)
    n = 70_001
    stream, _ = _stream(fam, n)
    d_stream = _dev(stream)
    c = E.Context(0)
    try:
        g = Guarded(n)
        for cap in (n - 1, 0):
            rc, got = _raw_decode(c, fam, d_stream, n, g.ptr, cap, body_call)
            g.check()
            assert rc == N.ET_ERR_CAP and got == 0, (name, cap, rc, got)
            assert _last_error(c) == "output buffer too small", (name, cap, _last_error(c))
            assert g.front_clean() and g.back_clean(0), f"{name} cap={cap}: a refused decode wrote the byte at offset {g.first_dirty(0)}"
        rc, got = _raw_decode(c, fam, d_stream, n, g.ptr, n, body_call)
        g.check()
        assert rc == N.ET_OK and got == n, (name, rc, got)
        assert g.data(n).tobytes() == fam.base[:n].tobytes(), f"{name} cap = n_out: wrong bytes"
        g.assert_extent(n, f"{name} cap = n_out")
        _assert_sound(c, other, 7)
    finally:
        c.close()


@pytest.mark.parametrize("where", ["late_block", "first_block"])
def test_truncated_body_is_written_after_the_report(where):
    """The header declares N symbols, the body is cut so that the oracle decodes M < N.  With M <= cap < N the speculative write
    is not launched (body_first_sweep: cap >= n_symbols) and the symbols leave through write_symbols(d, n_out, false) behind
    wait_report: ET_OK, *out_len == M, the oracle's bytes, nothing past M -- by the same write kernel as the whole stream's
    decode (timings).  cap = M - 1: ET_ERR_CAP, nothing written."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    O = _oracle()
    fam = _family("chained")
    N_decl = OWN
    stream, body_off = _stream(fam, N_decl)
    cut = body_off + (1_000 if where == "first_block" else 8192 * 12 + 3_001)  # (the body is ~115 KiB: 15 blocks)
    assert cut < len(stream) - 8192
    part = stream[:cut]
    want = O.decode(part)
    M = len(want)
    assert 0 < M < N_decl - 64 and want == fam.base[:M].tobytes()
    d_part, d_whole = _dev(part), _dev(stream)
    c = E.Context(0)
    try:
        whole = _timed_flags(c, lambda: c.decode_device(d_whole, torch.empty(N_decl, dtype=torch.uint8, device="cuda")))
        g = Guarded(N_decl)
        for cap in (M, (M + N_decl) // 2, N_decl - 1):
            g.refill()
            rc, got = _raw_decode(c, fam, d_part, N_decl, g.ptr, cap, False)
            g.check()
            assert rc == N.ET_OK and got == M, (where, cap, rc, got, M)
            assert g.data(M).tobytes() == want, f"{where} cap={cap}: not the oracle's bytes"
            g.assert_extent(M, f"truncated body, {where}, cap={cap}")
        g.refill()
        rc, got = _raw_decode(c, fam, d_part, N_decl, g.ptr, M - 1, False)
        g.check()
        assert rc == N.ET_ERR_CAP and got == 0 and _last_error(c) == "output buffer too small", (where, rc, got)
        assert g.front_clean() and g.back_clean(0), f"{where}: a refused decode wrote the byte at offset {g.first_dirty(0)}"
        t = _timed_flags(c, lambda: _raw_decode(c, fam, d_part, N_decl, g.ptr, M, False))
        torch.cuda.synchronize()
        assert {k: t[k] for k in FLAG_KEYS} == {k: whole[k] for k in FLAG_KEYS} and t["chained_write"] and t["tree_walk_sync"], (t, whole)
        _assert_sound(c, "rows", 8)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["chained", "rows"])
def test_range_write_extent_and_capacity(name):
    """et_decode_range_write behind et_decode_range_sync (a tree-walk range) and behind et_decode_range_maps + _resolve (a row
    code's), set up as tests/test_gpu_cli_dist.py::test_cold_decode_virtual_ranks does: the first blocks of a stream, its start
    known.  max_symbols of 1, 17, total - 1 and total into a buffer of exactly that size; cap = n_out - 1 is ET_ERR_CAP with
    nothing written, and the same call with room succeeds: the range stays valid after a refused write."""
    import entreepy_amd as E
    from entreepy_amd import _native as N

    fam = _family(name)
    n = 70_001
    stream, body_off = _stream(fam, n)
    comp = _dev(stream)
    ptr = comp.data_ptr() + body_off
    base_off, first_bit = body_off - (ptr & 3), (ptr & 3) * 8
    body = comp[base_off:]
    n_blocks = (body.numel() + 8191) // 8192
    assert n_blocks >= 4
    end = (n_blocks // 2) * 8192
    c = E.Context(0)
    try:
        if name == "chained":
            info = c.decode_range_sync(fam.cb, body, 0, end, first_bit)
            assert info["tree_walk"] and info["start_bit"] == first_bit
        else:
            _, n_starts = c.decode_range_maps(fam.cb, body, 0, end, first_bit)
            info = c.decode_range_resolve(first_bit)
            assert n_starts == 8 and info["row_walk"]
        total = info["n_symbols"]
        assert 8192 < total < n
        for max_symbols in (1, 17, total - 1, total):
            g = Guarded(max_symbols)
            got = ctypes.c_size_t(UNSET)
            c._bind()
            rc = N.lib().et_decode_range_write(c._h, max_symbols, g.ptr, max_symbols - 1, ctypes.byref(got))
            g.check()
            assert rc == N.ET_ERR_CAP and got.value == 0 and _last_error(c) == "output buffer too small", (name, max_symbols, rc, got.value)
            assert g.front_clean() and g.back_clean(0), f"{name} max_symbols={max_symbols}: a refused write wrote the byte at offset {g.first_dirty(0)}"
            m = c.decode_range_write(max_symbols, g.room)
            g.check()
            assert m == max_symbols and g.data(m).tobytes() == fam.base[:m].tobytes(), (name, max_symbols)
            g.assert_extent(m, f"range write, {name}, max_symbols={max_symbols}")
        _assert_sound(c, "fixed16" if name == "chained" else "chained", 9)
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 17, 4097, 300_000])
def test_encode_device_capacity(n):
    """cap = et_encode_bound(n) - 1: ET_ERR_CAP before anything is enqueued ("cap < et_encode_bound(n)"), *out_len == 0, the
    output untouched.  cap = et_encode_bound(n) exactly: the oracle's image, nothing in front of d_out and nothing at or past
    d_out + cap.  (n = 1: a lone symbol, the bare header.)"""
    import entreepy_amd as E
    from entreepy_amd import _native as N

    O = _oracle()
    text = corpus.text_like(n, 0xE7B0 + n)
    d_text = _dev(text.tobytes())
    bound = E.encode_bound(n)
    c = E.Context(0)
    try:
        g = Guarded(bound)
        c._bind()
        got = ctypes.c_size_t(UNSET)
        rc = N.lib().et_encode_device(c._h, d_text.data_ptr(), n, g.ptr, bound - 1, ctypes.byref(got))
        g.check()
        assert rc == N.ET_ERR_CAP and got.value == 0 and _last_error(c) == "cap < et_encode_bound(n)", (n, rc, got.value)
        assert g.front_clean() and g.back_clean(0), f"n={n}: a refused encode wrote the byte at offset {g.first_dirty(0)}"
        got = ctypes.c_size_t(UNSET)
        rc = N.lib().et_encode_device(c._h, d_text.data_ptr(), n, g.ptr, bound, ctypes.byref(got))
        g.check()
        want = O.encode(text)
        assert rc == N.ET_OK and got.value == len(want) and g.data(len(want)).tobytes() == want, (n, rc, got.value)
        g.assert_extent(bound, f"encode_device n={n}")
        _assert_sound(c, "chained", 10)
    finally:
        c.close()


def _shard_code(max_len):
    import entreepy_amd as E

    rng = np.random.default_rng(max_len)
    n_sym = 60
    lens, codes = _random_prefix_code(rng, n_sym, max_len)
    syms = rng.choice(256, size=n_sym, replace=False)
    data_t, len_t = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    for s, l, code in zip(syms, lens, codes):
        data_t[s], len_t[s] = code & 0xFFFFFFFF, l
    absent = np.setdiff1d(np.arange(256), syms)[:3].astype(np.uint8)  # symbols of length 0
    return E.Codebook.from_tables(data_t, len_t), data_t, len_t, syms[rng.integers(0, n_sym, size=20_001)].astype(np.uint8), absent


def _shard_call(c, cb, d_text, n, ptr, cap_bytes, start_bit, header):
    from entreepy_amd import _native as N

    c._bind()
    end = ctypes.c_uint64(UNSET)
    if header is None:
        rc = N.lib().et_encode_body_device(c._h, ctypes.byref(cb.raw), d_text.data_ptr() if n else None, n, ptr, cap_bytes, start_bit, ctypes.byref(end))
    else:
        hb = np.frombuffer(header, dtype=np.uint8)
        rc = N.lib().et_encode_head_shard_device(c._h, ctypes.byref(cb.raw), d_text.data_ptr() if n else None, n, ptr, cap_bytes, hb.ctypes.data, hb.size, ctypes.byref(end))
    return rc, end.value


@pytest.mark.parametrize("max_len", [12, 32])
def test_shard_encode_overwrites_exactly_its_words(max_len):
    """et_encode_body_device at start bits 0, 1, 31, 32, 45 and et_encode_head_shard_device, into a buffer of 0xFF whose usable
    part is exactly ((end + 31) / 32) * 4 bytes: the words in front of start_bit / 32 keep their 0xFF; from there to the last
    word the bytes are the oracle's pack_body into a ZEROED buffer -- so the bits of the first word before start_bit and the
    bits of the last word from `end` on are 0, what the OR of a concatenation relies on -- and nothing behind the last word is
    touched.  One word less: ET_ERR_CAP ("body does not fit d_out"), nothing written."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    O = _oracle()
    cb, data_t, len_t, text, _ = _shard_code(max_len)
    d_text = _dev(text.tobytes())
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    header = O.write_header(data_t, len_t, text.size)
    c = E.Context(0)
    try:
        for start_bit, head in [(s, None) for s in (0, 1, 31, 32, 45)] + [(8 * len(header), header)]:
            what = f"max_len={max_len} start_bit={start_bit}{' (head shard)' if head else ''}"
            want, want_end = O.pack_body(data_t, len_t, text, start_bit)
            cap = (want_end + 31) // 32 * 4
            image = np.zeros(cap, dtype=np.uint8)
            image[: len(want)] = np.frombuffer(want, dtype=np.uint8)
            first = 0 if head else start_bit // 32 * 4
            if head:
                image[: len(head)] |= np.frombuffer(head, dtype=np.uint8)
            g = Guarded(cap, fill=0xFF)
            c.histogram_device(d_text, hist)
            rc, end = _shard_call(c, cb, d_text, text.size, g.ptr, cap - 4, start_bit, head)
            g.check()
            assert rc == N.ET_ERR_CAP and _last_error(c) == "body does not fit d_out", (what, rc)
            assert g.front_clean() and g.back_clean(0), f"{what}: a refused shard encode wrote the byte at offset {g.first_dirty(0)}"
            c.histogram_device(d_text, hist)
            rc, end = _shard_call(c, cb, d_text, text.size, g.ptr, cap, start_bit, head)
            g.check()
            assert rc == N.ET_OK and end == want_end, (what, rc, end, want_end)
            assert (g.data(first) == 0xFF).all(), f"{what}: a word in front of the shard's first was written"
            got = g.data()[first:]
            bad = np.flatnonzero(got != image[first:])
            assert bad.size == 0, f"{what}: byte {first + int(bad[:1].sum())} of {cap} differs from the oracle's pack_body into a zeroed buffer"
            g.assert_extent(cap, what)
        _assert_sound(c, "chained", 11)
    finally:
        c.close()


@pytest.mark.parametrize("empty", ["no_text", "zero_length_symbols"])
def test_empty_shard_writes_one_zero_word(empty):
    """A shard without text (n = 0), or of symbols whose codewords have length 0, still owns the word its start bit lies in:
    exactly that word becomes 0 (include/entreepy_hip.h: every word a shard touches is fully overwritten) -- for the head shard
    the header padded with zeros to a word -- *end_bit == start_bit, and nothing else of a 0xFF buffer changes.  A buffer that
    ends in front of that word: ET_ERR_CAP."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    O = _oracle()
    cb, data_t, len_t, _, absent = _shard_code(12)
    text = absent[np.arange(1_000) % absent.size] if empty == "zero_length_symbols" else np.zeros(0, dtype=np.uint8)
    d_text = _dev(text.tobytes())
    hist = torch.zeros(256, dtype=torch.int64, device="cuda")
    header = O.write_header(data_t, len_t, text.size)
    c = E.Context(0)
    try:
        for start_bit, head in [(s, None) for s in (0, 1, 31, 32, 45)] + [(8 * len(header), header)]:
            what = f"{empty} start_bit={start_bit}{' (head shard)' if head else ''}"
            first = 0 if head else start_bit // 32 * 4
            cap = (len(head) + 3) // 4 * 4 if head else first + 4
            image = np.zeros(cap - first, dtype=np.uint8)
            if head:
                image[: len(head)] = np.frombuffer(head, dtype=np.uint8)
            g = Guarded(cap + 8, fill=0xFF)  # (8 bytes of the usable part lie behind cap: at or past d_out + cap)
            c.histogram_device(d_text, hist)
            rc, end = _shard_call(c, cb, d_text, text.size, g.ptr, cap - 4, start_bit, head)
            g.check()
            assert rc == N.ET_ERR_CAP and _last_error(c) == "body does not fit d_out", (what, rc)
            assert g.front_clean() and g.back_clean(0), f"{what}: a refused shard encode wrote the byte at offset {g.first_dirty(0)}"
            c.histogram_device(d_text, hist)
            rc, end = _shard_call(c, cb, d_text, text.size, g.ptr, cap, start_bit, head)
            g.check()
            assert rc == N.ET_OK and end == start_bit, (what, rc, end)
            assert (g.data(first) == 0xFF).all(), f"{what}: a word in front of the shard's own was written"
            assert g.data(cap)[first:].tobytes() == image.tobytes(), f"{what}: {g.data(cap)[first:].tobytes().hex()} for {image.tobytes().hex()}"
            g.assert_extent(cap, what)
        _assert_sound(c, "rows", 13)
    finally:
        c.close()


def test_host_memory_calls_capacity():
    """et_encode / et_decode on numpy buffers with guard bytes on both sides: cap = len - 1 is ET_ERR_CAP with *out_len == 0 and
    nothing written; cap = len is ET_OK with the oracle's bytes; the guards are intact either way."""
    import entreepy_amd as E
    from entreepy_amd import _native as N

    O = _oracle()
    text = corpus.text_like(4_097, 0xE7C0)
    et = O.encode(text)
    comp = np.frombuffer(et[4:], dtype=np.uint8)
    c = E.Context(0)
    try:
        for call, src, want, message in ((N.lib().et_encode, text, et, "output buffer too small"), (N.lib().et_decode, comp, text.tobytes(), "output buffer too small")):
            g = Guarded(len(want), device=None)
            got = ctypes.c_size_t(UNSET)
            rc = call(c._h, src.ctypes.data, src.size, g.ptr, len(want) - 1, ctypes.byref(got))
            g.check()
            assert rc == N.ET_ERR_CAP and got.value == 0 and _last_error(c) == message, (rc, got.value, _last_error(c))
            assert g.front_clean() and g.back_clean(0), f"a refused host call wrote the byte at offset {g.first_dirty(0)}"
            got = ctypes.c_size_t(UNSET)
            rc = call(c._h, src.ctypes.data, src.size, g.ptr, len(want), ctypes.byref(got))
            g.check()
            assert rc == N.ET_OK and got.value == len(want) and g.data().tobytes() == want, (rc, got.value)
            g.assert_extent(len(want), "host call at cap = len")
        _assert_sound(c, "rows", 12)
    finally:
        c.close()


# --- C. the same kernels behind their switches --------------------------------------------------------------------------------

# switch -> (families it affects, the flags their decodes then report; None: what they report without it)
SWITCHES = {
    "ET_NO_STRIPS": (("strips",), dict(tree_walk_sync=True, chained_write=True, strips_write=False)),
    "ET_NO_ROW_WRITE": (("rows",), dict(row_sync=True, exhaustive_sync=True, chained_write=True)),
    "ET_NO_FIXED_WRITE": (("fixed2", "fixed4", "fixed16", "fixed64", "fixed256"), dict(fixed_sync=True, exhaustive_sync=True)),
    "ET_NO_ROW_SYNC": (("rows",), dict(row_sync=False, exhaustive_sync=True, chained_write=True)),
    # the families that run on the window tables, those built by the host: the flags are the families' own (None)
    "ET_DEC_TABLES_HOST": (("exitmaps", "round1"), None),
}
SWITCH_LENGTHS = (17, 4097, 65_537, OWN)


def _child(switch):
    """(In the child process, the switch set: they are read once per process.)  Part A for the families the switch affects."""
    import entreepy_amd as E

    assert os.environ.get(switch) == "1"
    families, flags = SWITCHES[switch]
    c = E.Context(0)
    try:
        for name in families:
            for n in SWITCH_LENGTHS:
                _check_extent(c, _family(name), n, flags=flags)
    finally:
        c.close()
    print("ok")


def test_extent_behind_the_switches():
    """One child process per switch, one after the other, each under its own time limit; the first child that fails ends the
    test, so the ones behind it are not started."""
    for switch in SWITCHES:
        try:
            r = subprocess.run([sys.executable, "-m", "tests.test_gpu_extent", switch], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **{switch: "1"}), timeout=120)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{switch}: the child ran into its time limit; the switches behind it were not started\n{e.stderr!r}")
        assert r.returncode == 0 and "ok" in r.stdout, f"{switch}: exit status {r.returncode}; the switches behind it were not started\n{r.stderr[-3000:]}"


if __name__ == "__main__":
    _child(sys.argv[1])
