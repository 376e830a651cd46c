"""Host-side mirror of the reference's codec interface over the C ABI.

    reference                                   here
    encode(allocator, text, out_writer,         encode(text, flags) -> bytes
           std_out, flags) !usize  (encode.zig:25)
    decode(allocator, compressed_text, ...)     decode(compressed_text, flags) -> bytes
           !usize                   (decode.zig:13)
    EncodeFlags / DecodeFlags (encode.zig:9-14, decode.zig:7-11)
    error.QueueEmpty on empty input             EmptyInputError

`compressed_text` keeps the reference's convention: the .et file minus its first four
bytes (main.zig:204, test.zig:26).  Everything numeric happens in libentreepy_hip.so;
torch appears only as the owner of device memory and streams in the *_device calls.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _native as N


class EntreepyError(RuntimeError):
    def __init__(self, status, detail=""):
        msg = N.lib().et_strerror(status).decode()
        super().__init__(f"{msg}{': ' + detail if detail else ''} (et_status {status})")
        self.status = status


class EmptyInputError(EntreepyError):
    """The reference's error.QueueEmpty (queue.zig:28-30 reached from encode.zig:137-138)."""


@dataclass
class EncodeFlags:  # encode.zig:9-14
    write_output: bool = False
    print_output: bool = False
    debug: bool = False


@dataclass
class DecodeFlags:  # decode.zig:7-11
    write_output: bool = False
    print_output: bool = False
    debug: bool = False


@dataclass
class PackedResult:  # struct et_packed_result, and the call's own status in front
    status: int
    out_bytes: int
    n_failed: int
    first_failed: int
    n_short: int
    first_status: int


@dataclass
class MatchResult:  # struct et_match_result, and the call's own status in front
    status: int
    n_match: int
    n_failed: int
    first_failed: int
    first_status: int
    pattern_bits: int


@dataclass
class JoinResult:  # struct et_join_result, and the call's own status in front
    status: int
    n_match: int
    n_failed: int
    first_failed: int
    n_keys_failed: int
    first_key_failed: int
    first_status: int
    first_key_status: int


@dataclass
class GroupResult:  # struct et_group_result, and the call's own status in front
    status: int
    n_groups: int
    n_failed: int
    first_failed: int
    first_status: int


GROUP_NONE = N.ET_GROUP_NONE  # group_packed_device: group_of of a failed record


@dataclass
class NumberResult:  # struct et_number_result, and the call's own status in front
    status: int
    n_ok: int
    n_empty: int
    n_bad: int
    n_range: int
    n_failed: int
    first_failed: int
    first_status: int


NUMBER_OK, NUMBER_EMPTY, NUMBER_BAD, NUMBER_RANGE = N.ET_NUMBER_OK, N.ET_NUMBER_EMPTY, N.ET_NUMBER_BAD, N.ET_NUMBER_RANGE  # number_packed_device: a row's kind


@dataclass
class TakeResult:  # struct et_take_result, and the call's own status in front
    status: int
    out_bytes: int
    text_bytes: int
    n_failed: int
    first_failed: int
    first_status: int


MATCH_EQUAL, MATCH_PREFIX, MATCH_NOT =N.ET_MATCH_EQUAL, N.ET_MATCH_PREFIX, N.ET_MATCH_NOT  # match_packed_device's mode
MATCH_LESS, MATCH_LESS_EQUAL = N.ET_MATCH_LESS, N.ET_MATCH_LESS_EQUAL  # ... its order modes: text < needle, text <= needle (with MATCH_NOT: >=, >)
SEARCH_CONTAINS, SEARCH_SUFFIX = N.ET_SEARCH_CONTAINS, N.ET_SEARCH_SUFFIX  # search_packed_device's mode; MATCH_NOT may be or-ed in
SLICE_TO_END, SLICE_NO_STOP = N.ET_SLICE_TO_END, N.ET_SLICE_NO_STOP  # slice_packed_device: a count "to the end"; no stop byte
RECODE_DROP = N.ET_RECODE_DROP  # recode_packed_device: the map entry of a byte that is deleted


def byte_map(frm=b"", to=b"", delete=b""):
    """bytes.maketrans(frm, to) plus deletions, as recode_packed_device takes a map: 256 int16 values, entry c the byte that c becomes,
    RECODE_DROP for the bytes of `delete` -- text.translate(bytes.maketrans(frm, to), delete), one byte to one byte or to none."""
    m = np.frombuffer(bytes.maketrans(bytes(frm), bytes(to)), dtype=np.uint8).astype(np.int16)
    m[np.frombuffer(bytes(delete), dtype=np.uint8)] = RECODE_DROP
    return m


ASCII_UPPER = byte_map(bytes(range(ord("a"), ord("z") + 1)), bytes(range(ord("A"), ord("Z") + 1)))  # bytes.upper(): a-z alone
ASCII_LOWER = byte_map(bytes(range(ord("A"), ord("Z") + 1)), bytes(range(ord("a"), ord("z") + 1)))  # bytes.lower(): A-Z alone
for _m in (ASCII_UPPER, ASCII_LOWER):
    _m.setflags(write=False)
FIELD_TO_END, FIELD_ABSENT = N.ET_FIELD_TO_END, N.ET_FIELD_ABSENT  # field_packed_device: "every field from here on"; pos of a field that is not there


def _check(status, ctx=None):
    if status == N.ET_OK:
        return
    detail = N.lib().et_last_error(ctx).decode() if ctx else ""
    if status == N.ET_ERR_EMPTY:
        raise EmptyInputError(status, detail)
    raise EntreepyError(status, detail)


def _host_u8(buf):
    a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, dtype=np.uint8)
    return a, (a.ctypes.data if a.size else None)


class Codebook:
    """The code table (reference `dictionary`), host side."""

    def __init__(self, raw=None):
        self.raw = raw if raw is not None else N.Codebook()

    @classmethod
    def from_histogram(cls, hist):
        """encode.zig:54-214 via et_build_codebook."""
        h = np.ascontiguousarray(hist, dtype=np.uint64)
        assert h.size == 256
        cb = cls()
        _check(N.lib().et_build_codebook(h.ctypes.data, ctypes.byref(cb.raw)))
        return cb

    @classmethod
    def from_tables(cls, data, length):
        """An arbitrary table (tests of the long-code path)."""
        cb = cls()
        d = np.ascontiguousarray(data, dtype=np.uint32)
        l = np.ascontiguousarray(length, dtype=np.uint8)
        ctypes.memmove(cb.raw.data, d.ctypes.data, 1024)
        ctypes.memmove(cb.raw.length, l.ctypes.data, 256)
        nz = l[l > 0]
        cb.raw.n_coded = int(nz.size)
        cb.raw.min_length = int(nz.min()) if nz.size else 0
        cb.raw.max_length = int(nz.max()) if nz.size else 0
        return cb

    @property
    def data(self):
        return np.frombuffer(self.raw.data, dtype=np.uint32).copy()

    @property
    def length(self):
        return np.frombuffer(self.raw.length, dtype=np.uint8).copy()

    @property
    def dfs_order(self):
        # a lone symbol is a leaf-root with length 0 (encode.zig:137-138): still one dump line
        n = int(self.raw.n_coded) or 1
        return np.frombuffer(self.raw.dfs_order, dtype=np.uint8)[:n].copy()

    def header(self, text_len):
        """encode.zig:259-299 via et_write_header."""
        out = np.zeros(8192, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        _check(N.lib().et_write_header(ctypes.byref(self.raw), int(text_len), out.ctypes.data, out.size, ctypes.byref(n)))
        return out[: n.value].tobytes()

    def bits(self, hist):
        h = np.ascontiguousarray(hist, dtype=np.uint64)
        b = ctypes.c_uint64(0)
        _check(N.lib().et_codebook_bits(ctypes.byref(self.raw), h.ctypes.data, ctypes.byref(b)))
        return b.value

    def is_complete(self):
        """A full prefix-free tree of codes up to 32 bits (et_codebook_is_complete): what the shared-table calls ask for."""
        return N.lib().et_codebook_is_complete(ctypes.byref(self.raw)) == N.ET_OK

    def body_bound(self, n):
        """Bytes that always hold the body of n symbols (et_body_bound)."""
        return N.lib().et_body_bound(ctypes.byref(self.raw), int(n))

    def encode_pattern(self, text):
        """text -> (its body under this table as bytes, the number of bits): what match_packed_device compares the records' bodies
        with (et_encode_pattern, on the host).  Raises EntreepyError(ET_ERR_UNSUPPORTED) for a byte without a code."""
        a, p = _host_u8(bytes(text))
        out = np.zeros(max(4 * a.size, 1), dtype=np.uint8)
        bits = ctypes.c_uint64(0)
        _check(N.lib().et_encode_pattern(ctypes.byref(self.raw), p, a.size, out.ctypes.data, out.size, ctypes.byref(bits)))
        return out[: (bits.value + 7) // 8].tobytes(), bits.value


def parse_header(compressed_text):
    """decode.zig:34-141 via et_parse_header -> (Codebook, n_symbols, body_offset)."""
    a, p = _host_u8(compressed_text)
    cb = Codebook()
    n = ctypes.c_uint64(0)
    off = ctypes.c_size_t(0)
    _check(N.lib().et_parse_header(p, a.size, ctypes.byref(cb.raw), ctypes.byref(n), ctypes.byref(off)))
    return cb, n.value, off.value


def encode_bound(n):
    return N.lib().et_encode_bound(n)


class Context:
    """One et_ctx: a GPU's stream, workspaces and pinned staging.

    The *_device calls (and a Group's) take torch tensors, which torch's CURRENT stream produced and will consume, so by
    default they run on that stream: whatever stream is current when the call is made (torch.cuda.stream(...) included) is
    the one the call is ordered on.  (Until round 4 a new context ran on a non-blocking stream of its own unless told
    otherwise, and a caller who forgot use_torch_stream() raced with the kernels that made its tensors: tests/soak/soak_sharded.py
    found that the hard way.)  use_own_stream() / use_stream(ptr) opt out: the caller then orders those streams against the ones
    its tensors live on.  The C ABI is unchanged: an et_ctx starts on its own stream (et_ctx_set_stream).

    Calls return before their kernels finish.  Whichever way the context moves to another stream (a torch.cuda.stream block,
    use_stream, use_own_stream, use_torch_stream), the new stream is first ordered after all the work the context enqueued on
    the old one (include/entreepy_hip.h, "STREAM SWITCHES"), and the old stream must still exist at that moment.  So a tensor
    this context wrote on stream A and a later call of it reads on stream B needs no synchronisation; ordering against work
    that is not this context's stays the caller's job (torch's usual rules across streams)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        self.device = device
        self._groups = []  # weak references to the Groups made on this context: closed before it
        self._follow_torch = True  # device calls bind the ctx to torch's current stream first
        self._bound = None
        _check(N.lib().et_ctx_create(device, ctypes.byref(self._h)))

    def close(self):
        for ref in self._groups:
            g = ref()
            if g is not None:
                g.close()
        self._groups = []
        if self._h:
            N.lib().et_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- plumbing ---------------------------------------------------------------
    def use_stream(self, hip_stream):
        """Run on a caller-owned stream (a raw hipStream_t); the caller orders it against the streams its tensors live on."""
        self._follow_torch = False
        self._bound = None
        _check(N.lib().et_ctx_set_stream(self._h, ctypes.c_void_p(hip_stream)), self._h)

    def use_own_stream(self):
        """Run on the context's own non-blocking stream; the caller orders it against the streams its tensors live on."""
        self._follow_torch = False
        self._bound = None
        _check(N.lib().et_ctx_use_own_stream(self._h), self._h)

    def use_torch_stream(self):
        """(The default.)  Every device call runs on the stream that is torch's current one when the call is made."""
        self._follow_torch = True
        self._bind()

    def _bind(self):
        """Before a call that takes device tensors: the ctx onto torch's current stream (a pointer compare when nothing changed)."""
        if not self._follow_torch:
            return
        import torch

        ptr = torch.cuda.current_stream(self.device).cuda_stream
        if ptr != self._bound:
            _check(N.lib().et_ctx_set_stream(self._h, ctypes.c_void_p(ptr)), self._h)
            self._bound = ptr

    def reserve(self, max_text_bytes):
        _check(N.lib().et_ctx_reserve(self._h, int(max_text_bytes)), self._h)

    def set_tile_rounds(self, rounds):
        """Force the encode tile to rounds x 4 KiB (0 = size-based).  Test/tuning knob."""
        _check(N.lib().et_ctx_set_tile_rounds(self._h, int(rounds)), self._h)

    TIMING_DECODE_BODY = 2  # et_ctx_enable_timing's ET_TIMING_DECODE_BODY: only the decode's write kernel carries events

    def enable_timing(self, on=True):
        """True / False: every phase / nothing carries HIP events; Context.TIMING_DECODE_BODY: the decode's write kernel alone
        (timings("decode") then holds body_ms, host_ms and the path flags only)."""
        _check(N.lib().et_ctx_enable_timing(self._h, 2 if (on is not True and on == self.TIMING_DECODE_BODY) else int(bool(on))), self._h)

    def timings(self, which=None):
        """Phase timings of the last call (which=None), the last encode-side call ("encode")
        or the last decode ("decode"); waits for that call's last event."""
        t = N.Timings()
        if which is None:
            _check(N.lib().et_last_timings(self._h, ctypes.byref(t)), self._h)
        else:
            _check(N.lib().et_last_timings_of(self._h, {"encode": 0, "decode": 1}[which], ctypes.byref(t)), self._h)
        d = {k: getattr(t, k) for k, _ in N.Timings._fields_ if k not in ("reserved", "pad_")}
        d["exhaustive_sync"] = bool(t.reserved & 1)
        d["tree_walk_sync"] = bool(t.reserved & 2)
        d["chained_write"] = bool(t.reserved & 4)
        d["row_sync"] = bool(t.reserved & 8)
        d["fixed_sync"] = bool(t.reserved & 16)
        d["strips_write"] = bool(t.reserved & 32)
        return d

    def last_codebook(self):
        """Code table of the most recent encode of this context (et_last_codebook)."""
        cb = Codebook()
        _check(N.lib().et_last_codebook(self._h, ctypes.byref(cb.raw)), self._h)
        return cb

    # -- whole calls, files (chunked pinned-buffer pipeline) -------------------------
    def encode_file(self, in_path, out_path=None):
        """c: in_path -> out_path (.et image); out_path None = code only (main.zig -t).
        Returns (bytes read, bytes of .et produced)."""
        return self._file_call(N.lib().et_encode_fd, in_path, out_path, ())

    def decode_file(self, in_path, out_path=None, skip=4):
        """d: in_path (a .et file; its first `skip` bytes are passed over as main.zig:204
        does) -> out_path.  Returns (bytes consumed after the skip, bytes decoded)."""
        return self._file_call(N.lib().et_decode_fd, in_path, out_path, (skip,))

    def _file_call(self, fn, in_path, out_path, extra):
        import os

        fin = os.open(in_path, os.O_RDONLY)
        fout = os.open(out_path, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) if out_path is not None else -1
        try:
            a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
            _check(fn(self._h, fin, *extra, fout, ctypes.byref(a), ctypes.byref(b)), self._h)
            return a.value, b.value
        finally:
            os.close(fin)
            if fout >= 0:
                os.close(fout)

    # -- whole calls, host memory --------------------------------------------------
    def encode(self, text):
        a, p = _host_u8(text)
        out = np.empty(encode_bound(a.size), dtype=np.uint8)
        n = ctypes.c_size_t(0)
        _check(N.lib().et_encode(self._h, p, a.size, out.ctypes.data, out.size, ctypes.byref(n)), self._h)
        return out[: n.value].tobytes()

    def decode(self, compressed_text):
        a, p = _host_u8(compressed_text)
        want = ctypes.c_size_t(0)
        _check(N.lib().et_decoded_size(p, a.size, ctypes.byref(want)), self._h)
        out = np.empty(want.value + 64, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        _check(N.lib().et_decode(self._h, p, a.size, out.ctypes.data, out.size, ctypes.byref(n)), self._h)
        return out[: n.value].tobytes()

    # -- whole calls, device memory (torch uint8 tensors) ------------------------------
    def encode_device(self, text, out):
        """text, out: 1-D uint8 CUDA tensors; out.numel() >= encode_bound(text.numel()).
        Stream-ordered: returns the .et byte count without waiting for the kernels."""
        self._bind()
        n = ctypes.c_size_t(0)
        _check(N.lib().et_encode_device(self._h, text.data_ptr(), text.numel(), out.data_ptr(), out.numel(), ctypes.byref(n)), self._h)
        return n.value

    def decode_device(self, compressed_text, out, skip=0, length=None):
        """compressed_text[skip : skip + length] (default: to its end) -> out; the offsets spare the caller a tensor view."""
        self._bind()
        n = ctypes.c_size_t(0)
        length = compressed_text.numel() - skip if length is None else length
        _check(N.lib().et_decode_device(self._h, compressed_text.data_ptr() + skip, length, out.data_ptr(), out.numel(), ctypes.byref(n)), self._h)
        return n.value

    # -- batches of small streams (et_encode_batch_device / et_decode_batch_device) ------------
    _ITEM = np.dtype([("in_off", "<u8"), ("in_len", "<u8"), ("out_off", "<u8"), ("out_cap", "<u8"), ("out_len", "<u8"), ("status", "<i4"), ("path", "<u4")])

    def _batch_device(self, fn, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps):
        assert self._ITEM.itemsize == ctypes.sizeof(N.BatchItem) == N.lib().et_batch_item_size()
        items = np.zeros(len(in_offsets), dtype=self._ITEM)
        items["in_off"], items["in_len"], items["out_off"], items["out_cap"] = in_offsets, in_lens, out_offsets, out_caps
        self._bind()
        _check(fn(self._h, in_tensor.data_ptr(), out_tensor.data_ptr(), items.ctypes.data if items.size else None, items.size), self._h)
        return items["out_len"].copy(), items["status"].copy(), items["path"].copy()

    def encode_batch_device(self, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps):
        """Stream b: the text in_tensor[in_offsets[b] : + in_lens[b]] -> its .et image at out_tensor[out_offsets[b] : + out_caps[b]]
        (uint8 CUDA tensors; out_caps[b] >= encode_bound(in_lens[b]), the output address a multiple of 16; outputs disjoint).
        One call for all of them.  -> (out_lens, statuses, paths) as numpy arrays: a stream that fails (statuses[b] != 0)
        fails alone; paths[b] = 0 by the batch kernels, 1 by the single-stream path.  Stream-ordered like encode_device."""
        return self._batch_device(N.lib().et_encode_batch_device, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps)

    def decode_batch_device(self, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps):
        """Stream b: the .et file minus its first four bytes at in_tensor[in_offsets[b] : + in_lens[b]] -> its symbols at
        out_tensor[out_offsets[b] : + out_caps[b]].  Returns as encode_batch_device."""
        return self._batch_device(N.lib().et_decode_batch_device, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps)

    def _batch_host(self, call, blobs, caps, what):
        """One upload, one batch call, one download."""
        import torch

        blobs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blobs]
        if not blobs:
            return []
        lens = np.array([b.size for b in blobs], dtype=np.uint64)
        in_off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
        caps = (np.asarray(caps, dtype=np.uint64) + 15) & ~np.uint64(15)
        out_off = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        dev = torch.device("cuda", self.device)
        packed = np.concatenate(blobs) if int(lens.sum()) else np.zeros(0, dtype=np.uint8)
        d_in = torch.empty(max(packed.size, 1), dtype=torch.uint8, device=dev)
        d_in[: packed.size] = torch.from_numpy(packed).to(dev)
        d_out = torch.empty(max(int(caps.sum()), 16), dtype=torch.uint8, device=dev)
        out_lens, statuses, _ = call(d_in, in_off, lens, d_out, out_off, caps)
        bad = np.flatnonzero(statuses)
        if bad.size:
            cls = EmptyInputError if statuses[bad[0]] == N.ET_ERR_EMPTY else EntreepyError
            raise cls(int(statuses[bad[0]]), f"{what}: item {int(bad[0])}")
        host = d_out.cpu().numpy()  # (the copy runs on torch's current stream, behind the batch's kernels)
        return [host[int(o) : int(o) + int(n)].tobytes() for o, n in zip(out_off, out_lens)]

    def encode_batch(self, texts):
        """[bytes] -> [their .et images], through one encode_batch_device call.  Raises EntreepyError naming the first
        item that failed (EmptyInputError for an empty text)."""
        return self._batch_host(self.encode_batch_device, texts, [encode_bound(len(t)) for t in texts], "encode_batch")

    def decode_batch(self, compressed_texts):
        """[.et files minus their first four bytes] -> [their texts], through one decode_batch_device call."""
        caps = [int.from_bytes(bytes(c[1:5]), "big") + 16 if len(c) >= 5 else 16 for c in compressed_texts]
        return self._batch_host(self.decode_batch_device, compressed_texts, caps, "decode_batch")

    # -- batched bodies under one shared code table (et_encode_shared_device / et_decode_shared_device) ------------
    def _shared_device(self, fn, codebook, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps):
        items = np.zeros(len(in_offsets), dtype=self._ITEM)
        items["in_off"], items["in_len"], items["out_off"], items["out_cap"] = in_offsets, in_lens, out_offsets, out_caps
        self._bind()
        _check(fn(self._h, ctypes.byref(codebook.raw), in_tensor.data_ptr(), self._opt_ptr(out_tensor), items.ctypes.data if items.size else None, items.size), self._h)
        return items["out_len"].copy(), items["status"].copy(), items["path"].copy()

    def encode_shared_device(self, codebook, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps):
        """Record b: the text in_tensor[in_offsets[b] : + in_lens[b]] -> its body alone under `codebook` (a complete table:
        Codebook.is_complete) at out_tensor[out_offsets[b] : + out_lens[b]], any alignment, not a byte beyond it;
        out_caps[b] >= codebook.body_bound(in_lens[b]) always suffices.  out_tensor=None: sizes only -- nothing is written,
        out_lens and statuses are the writing call's.  -> (out_lens, statuses, paths) as encode_batch_device; paths are 0."""
        return self._shared_device(N.lib().et_encode_shared_device, codebook, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps)

    def decode_shared_device(self, codebook, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps):
        """Record b: the body in_tensor[in_offsets[b] : + in_lens[b]] -> out_caps[b] symbols (the record's length, which the
        caller keeps; fewer when the body ends early) at out_tensor[out_offsets[b] : ...].  Returns as encode_shared_device."""
        return self._shared_device(N.lib().et_decode_shared_device, codebook, in_tensor, in_offsets, in_lens, out_tensor, out_offsets, out_caps)

    def _shared_host(self, call, codebook, blobs, what, out_lens=None):
        """One upload, the call(s), one download; the outputs lie back to back.  out_lens=None: a sizes-only call finds them."""
        import torch

        blobs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blobs]
        if not blobs:
            return []
        lens = np.array([b.size for b in blobs], dtype=np.uint64)
        in_off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
        dev = torch.device("cuda", self.device)
        packed = np.concatenate(blobs)
        d_in = torch.empty(max(packed.size, 1), dtype=torch.uint8, device=dev)
        d_in[: packed.size] = torch.from_numpy(packed).to(dev)

        def first_failure(statuses):
            bad = np.flatnonzero(statuses)
            if bad.size:
                raise EntreepyError(int(statuses[bad[0]]), f"{what}: item {int(bad[0])}")

        if out_lens is None:
            out_lens, statuses, _ = call(codebook, d_in, in_off, lens, None, np.zeros(lens.size, np.uint64), np.zeros(lens.size, np.uint64))
            first_failure(statuses)
        caps = np.asarray(out_lens, dtype=np.uint64)
        out_off = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        d_out = torch.empty(max(int(caps.sum()), 1), dtype=torch.uint8, device=dev)
        out_lens, statuses, _ = call(codebook, d_in, in_off, lens, d_out, out_off, caps)
        first_failure(statuses)
        host = d_out.cpu().numpy()  # (the copy runs on torch's current stream, behind the call's kernels)
        return [host[int(o) : int(o) + int(n)].tobytes() for o, n in zip(out_off, out_lens)]

    def encode_shared(self, codebook, texts):
        """[bytes] -> [their bodies under `codebook`]: a sizes-only call, a prefix sum, then one call that packs the bodies
        back to back.  Raises EntreepyError naming the first item that failed (a byte the table has no code for)."""
        return self._shared_host(self.encode_shared_device, codebook, texts, "encode_shared")

    def decode_shared(self, codebook, bodies, lengths):
        """[bodies], [the records' lengths] -> [their texts], through one decode_shared_device call."""
        assert len(bodies) == len(lengths)
        return self._shared_host(self.decode_shared_device, codebook, bodies, "decode_shared", out_lens=lengths)

    # -- packed record batches (et_encode_packed_device / et_decode_packed_device) ------------
    @staticmethod
    def _index_ptr(t, n=None):
        """A device offsets array: a 1-D CUDA tensor of 8-byte integers (torch.int64 holds the u64 values), n + 1 entries."""
        assert t.is_cuda and t.dim() == 1 and t.element_size() == 8 and t.is_contiguous() and not t.is_floating_point(), "an offsets array is a 1-D CUDA tensor of 64-bit integers"
        assert t.numel() >= 1 and (n is None or t.numel() == n + 1), "an offsets array holds one entry more than there are records"
        return t.data_ptr()

    @staticmethod
    def _rows_ptr(t, what="rows is a 1-D CUDA tensor of 32-bit integers"):
        """Record or key numbers on the device: a 1-D CUDA tensor of 4-byte integers."""
        assert t.is_cuda and t.dim() == 1 and t.element_size() == 4 and t.is_contiguous() and not t.is_floating_point(), what
        return t.data_ptr()

    @staticmethod
    def _opt_ptr(t):
        return None if t is None else t.data_ptr()

    def _store_args(self, bodies, body_index, text_index):
        """A store as the selecting calls' C functions take it: its five arguments, the record count last."""
        n = text_index.numel() - 1
        return bodies.data_ptr(), bodies.numel(), self._index_ptr(body_index, n), self._index_ptr(text_index), n

    def _out32(self, t, what="rows is a 1-D CUDA tensor of 32-bit integers"):
        """An optional output of 32-bit entries: (its pointer, how many it holds), (None, 0) without one."""
        return (None, 0) if t is None else (self._rows_ptr(t, what), t.numel())

    def _cap_or_raise(self, rc):
        if rc != N.ET_ERR_CAP:  # (a capacity error still carries the room needed: the caller reads it and comes back)
            _check(rc, self._h)
        return rc

    def _packed_result(self, status, res):
        return PackedResult(self._cap_or_raise(status), res.out_bytes, res.n_failed, res.first_failed, res.n_short, res.first_status)

    def _take_result(self, status, res):
        return TakeResult(self._cap_or_raise(status), res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status)

    def encode_packed_device(self, codebook, text, text_index, out, out_index, status=None):
        """Record b: text[text_index[b] : text_index[b + 1]] -> its body under `codebook` at out[out_index[b] : out_index[b + 1]],
        the bodies back to back from out_index[0] = 0; the scan that lays them out runs on the GPU.  text, out: uint8 CUDA tensors;
        text_index (given), out_index (written): CUDA tensors of n + 1 64-bit integers; status: optional uint8 CUDA tensor of n
        et_status bytes.  A failed record (a byte without a code, a record above batch small_max, a bad pair of offsets) takes no
        bytes.  out=None: sizes only.  -> PackedResult; .status is ET_OK or ET_ERR_CAP (nothing written, .out_bytes = the room
        needed); any other failure of the call raises.  Stream-ordered: the result is final, the tensors once the stream drained."""
        n = text_index.numel() - 1
        res = N.PackedResult()
        self._bind()
        rc = N.lib().et_encode_packed_device(self._h, ctypes.byref(codebook.raw), text.data_ptr(), text.numel(), self._index_ptr(text_index), n,
                                             self._opt_ptr(out), 0 if out is None else out.numel(), self._index_ptr(out_index, n), self._opt_ptr(status), ctypes.byref(res))
        return self._packed_result(rc, res)

    def decode_packed_device(self, codebook, bodies, body_index, text_index, out, written=None, status=None):
        """Record b: text_index[b + 1] - text_index[b] symbols from bodies[body_index[b] : body_index[b + 1]] -> out[text_index[b] : ...].
        The three arrays may be the encoder's own (bodies = its out, body_index = its out_index), or sub-ranges of the two
        offsets arrays: records [i, j) are body_index[i : j + 1] and text_index[i : j + 1].  written: optional int32/uint32 CUDA
        tensor of n counts; status as encode_packed_device.  -> PackedResult (.n_short: bodies that ended early)."""
        n = text_index.numel() - 1
        res = N.PackedResult()
        self._bind()
        rc = N.lib().et_decode_packed_device(self._h, ctypes.byref(codebook.raw), bodies.data_ptr(), bodies.numel(), self._index_ptr(body_index, n), self._index_ptr(text_index), n,
                                             out.data_ptr(), out.numel(), self._opt_ptr(written), self._opt_ptr(status), ctypes.byref(res))
        return self._packed_result(rc, res)

    def decode_packed_gather_device(self, codebook, bodies, body_index, text_index, rows, out, out_index, written=None, status=None):
        """Row k of the result is record rows[k] of the store (bodies, body_index, text_index: decode_packed_device's, the text offsets
        serving as record lengths only), in any order, with repeats: its symbols go to out[out_index[k] : out_index[k + 1]], the rows
        back to back from out_index[0] = 0 -- the layout is computed on the GPU.  rows: int32/uint32 CUDA tensor of record numbers;
        out_index (written): CUDA tensor of len(rows) + 1 64-bit integers; written, status: optional, one entry per ROW.  A row that
        fails (a record number beyond the store, a bad pair of offsets, a record above batch small_max) takes no bytes; the result's
        first_failed is a row.  out=None: sizes only.  -> PackedResult; .status is ET_OK or ET_ERR_CAP (nothing written, .out_bytes =
        the room needed); any other failure of the call raises.  Stream-ordered like decode_packed_device."""
        n = text_index.numel() - 1
        rows_p = self._rows_ptr(rows)
        res = N.PackedResult()
        self._bind()
        rc = N.lib().et_decode_packed_gather_device(self._h, ctypes.byref(codebook.raw), bodies.data_ptr(), bodies.numel(), self._index_ptr(body_index, n), self._index_ptr(text_index), n,
                                                    rows_p, rows.numel(), self._opt_ptr(out), 0 if out is None else out.numel(), self._index_ptr(out_index, rows.numel()),
                                                    self._opt_ptr(written), self._opt_ptr(status), ctypes.byref(res))
        return self._packed_result(rc, res)

    def match_packed_device(self, codebook, bodies, body_index, text_index, needle, mode, rows=None, status=None):
        """The records of the store (bodies, body_index, text_index: decode_packed_gather_device's) whose text equals `needle`
        (MATCH_EQUAL), begins with it (MATCH_PREFIX), or lies below it as bytes compare (MATCH_LESS: text < needle, MATCH_LESS_EQUAL:
        text <= needle) -- with MATCH_NOT or-ed in, the valid records that do not: >= and > for the order modes -- found on the
        compressed bytes, nothing decoded.  needle: bytes on the host.  rows: int32/uint32 CUDA tensor that takes the selected record
        numbers, ascending (decode_packed_gather_device's rows); None: count only.  status: optional uint8 CUDA tensor of one et_status
        byte per record; a failed record is never selected.  -> MatchResult; .status is ET_OK or ET_ERR_CAP (no row written, .n_match =
        the room needed); any other failure of the call raises.  Stream-ordered like decode_packed_device."""
        a, p = _host_u8(bytes(needle))
        res = N.MatchResult()
        self._bind()
        rc = N.lib().et_match_packed_device(self._h, ctypes.byref(codebook.raw), *self._store_args(bodies, body_index, text_index), p, a.size, int(mode), *self._out32(rows),
                                            self._opt_ptr(status), ctypes.byref(res))
        return MatchResult(self._cap_or_raise(rc), res.n_match, res.n_failed, res.first_failed, res.first_status, res.pattern_bits)

    def search_packed_device(self, codebook, bodies, body_index, text_index, needle, mode, rows=None, pos=None, status=None):
        """The records of the store (bodies, body_index, text_index: match_packed_device's) whose text contains `needle`
        (SEARCH_CONTAINS) or ends with it (SEARCH_SUFFIX) -- with MATCH_NOT or-ed in, the valid records that do not -- found on the
        compressed bytes by a walk over the codeword boundaries, nothing decoded.  needle: bytes on the host, at most 256.  rows:
        int32/uint32 CUDA tensor that takes the selected record numbers, ascending; None: count only.  pos: optional tensor like rows
        (not with MATCH_NOT): where in each selected record the needle lies -- the first occurrence, or length - len(needle).
        status: optional uint8 CUDA tensor of one et_status byte per record; a failed record is never selected.  -> MatchResult;
        .status is ET_OK or ET_ERR_CAP (no row written, .n_match = the room needed); any other failure of the call raises.
        Stream-ordered like decode_packed_device."""
        a, p = _host_u8(bytes(needle))
        what = "rows and pos are 1-D CUDA tensors of 32-bit integers"
        assert pos is None or (rows is not None and pos.numel() >= rows.numel()), "pos is as large as rows"
        res = N.MatchResult()
        self._bind()
        rc = N.lib().et_search_packed_device(self._h, ctypes.byref(codebook.raw), *self._store_args(bodies, body_index, text_index), p, a.size, int(mode), *self._out32(rows, what),
                                             self._out32(pos, what)[0], self._opt_ptr(status), ctypes.byref(res))
        return MatchResult(self._cap_or_raise(rc), res.n_match, res.n_failed, res.first_failed, res.first_status, res.pattern_bits)

    def join_packed_device(self, codebook, bodies, body_index, text_index, key_bodies, key_body_index, key_text_index, mode=0, rows=None, key_of_row=None, status=None,
                           key_status=None):
        """The records of the store (bodies, body_index, text_index: match_packed_device's) that equal SOME key of the key set
        (key_bodies, key_body_index, key_text_index: a packed store under the same codebook, on the device) -- with mode=MATCH_NOT the
        valid records that equal none -- decided on the compressed bytes through a hash table, nothing decoded and no key brought to
        the host.  rows: int32/uint32 CUDA tensor that takes the selected record numbers, ascending; None: count only.  key_of_row:
        optional tensor like rows (not with MATCH_NOT): the lowest key number equal to each selected record.  status, key_status:
        optional uint8 CUDA tensors of one et_status byte per record / per key; a failed record is never selected, a failed key
        equals nothing.  An empty key set (key_body_index of one entry) selects nothing.  -> JoinResult; .status is ET_OK or
        ET_ERR_CAP (no row written, .n_match = the room needed); any other failure of the call raises.  Stream-ordered like
        decode_packed_device."""
        what = "rows and key_of_row are 1-D CUDA tensors of 32-bit integers"
        assert key_of_row is None or (rows is not None and key_of_row.numel() >= rows.numel()), "key_of_row is as large as rows"
        res = N.JoinResult()
        self._bind()
        rc = N.lib().et_join_packed_device(self._h, ctypes.byref(codebook.raw), *self._store_args(bodies, body_index, text_index),
                                           *self._store_args(key_bodies, key_body_index, key_text_index), int(mode), *self._out32(rows, what), self._out32(key_of_row, what)[0],
                                           self._opt_ptr(status), self._opt_ptr(key_status), ctypes.byref(res))
        return JoinResult(self._cap_or_raise(rc), res.n_match, res.n_failed, res.first_failed, res.n_keys_failed, res.first_key_failed, res.first_status, res.first_key_status)

    def group_packed_device(self, codebook, bodies, body_index, text_index, first_rows=None, count=None, group_of=None, status=None):
        """The groups of equal records of the store (bodies, body_index, text_index: join_packed_device's) -- DISTINCT, GROUP BY and
        COUNT(*) -- decided on the compressed bytes by a join of the store with itself, nothing decoded.  Groups are numbered in order
        of first appearance.  first_rows: int32/uint32 CUDA tensor that takes each group's lowest record number, ascending
        (take_packed_device's rows: the store of the distinct texts); None: count only.  count: optional tensor like first_rows: the
        members of each group.  group_of: optional tensor of one 32-bit entry per record: its group, GROUP_NONE for a failed record.
        count and group_of need first_rows.  status: optional uint8 CUDA tensor of one et_status byte per record; a failed record
        belongs to no group.  -> GroupResult; .status is ET_OK or ET_ERR_CAP (nothing written, .n_groups = the room needed); any
        other failure of the call raises.  Stream-ordered like decode_packed_device."""
        what = "first_rows, count and group_of are 1-D CUDA tensors of 32-bit integers"
        assert count is None or (first_rows is not None and count.numel() >= first_rows.numel()), "count is as large as first_rows"
        assert group_of is None or group_of.numel() >= text_index.numel() - 1, "group_of holds an entry per record"
        res = N.GroupResult()
        self._bind()
        rc = N.lib().et_group_packed_device(self._h, ctypes.byref(codebook.raw), *self._store_args(bodies, body_index, text_index), *self._out32(first_rows, what),
                                            self._out32(count, what)[0], self._out32(group_of, what)[0], self._opt_ptr(status), ctypes.byref(res))
        return GroupResult(self._cap_or_raise(rc), res.n_groups, res.n_failed, res.first_failed, res.first_status)

    def take_packed_device(self, bodies, body_index, text_index, rows, out, out_body_index, out_text_index, status=None):
        """Row k of the NEW store is record rows[k] of the store (bodies, body_index, text_index: decode_packed_gather_device's), in any
        order, with repeats: its body goes as it is to out[out_body_index[k] : out_body_index[k + 1]], the bodies back to back from 0,
        and out_text_index[k + 1] - out_text_index[k] is its length -- nothing decoded, no codebook.  rows: int32/uint32 CUDA tensor of
        record numbers (match_packed_device's or join_packed_device's); out_body_index, out_text_index (written): CUDA tensors of
        len(rows) + 1 64-bit integers; status: optional uint8 CUDA tensor of one et_status byte per ROW.  A row that fails (a record
        number beyond the store, a bad pair of offsets, a record above the limits) becomes an empty record.  out=None: sizes only.  out
        may not overlap bodies.  -> TakeResult; .status is ET_OK or ET_ERR_CAP (nothing written, .out_bytes = the room needed); any
        other failure of the call raises.  Stream-ordered like decode_packed_device: the three outputs may go straight into
        join_packed_device (as the key set), decode_packed_device or decode_packed_gather_device."""
        n = text_index.numel() - 1
        rows_p = self._rows_ptr(rows)
        res = N.TakeResult()
        self._bind()
        rc = N.lib().et_take_packed_device(self._h, bodies.data_ptr(), bodies.numel(), self._index_ptr(body_index, n), self._index_ptr(text_index), n, rows_p, rows.numel(),
                                           self._opt_ptr(out), 0 if out is None else out.numel(), self._index_ptr(out_body_index, rows.numel()),
                                           self._index_ptr(out_text_index, rows.numel()), self._opt_ptr(status), ctypes.byref(res))
        return self._take_result(rc, res)

    def slice_packed_device(self, codebook, bodies, body_index, text_index, rows, first, count, out, out_body_index, out_text_index, stop=None, status=None):
        """Row k of the NEW store is text[first : first + count] of record rows[k] of the store (bodies, body_index, text_index:
        take_packed_device's; rows=None: row k is record k), cut in front of the first byte `stop` in it -- found and copied on the
        compressed bytes, nothing decoded: its body, as encode_packed_device would write it under `codebook`, goes to
        out[out_body_index[k] : out_body_index[k + 1]], and out_text_index[k + 1] - out_text_index[k] is its length.  first, count:
        an int for every row, or an int32/uint32 CUDA tensor of one value per row (first may be search_packed_device's pos, or that
        plus the needle's length); count=SLICE_TO_END: to the end.  stop: None, an int 0 .. 255, or one byte.  status: optional uint8
        CUDA tensor of one et_status byte per ROW; a row that fails becomes an empty record.  out=None: sizes only.  out may not
        overlap bodies.  -> TakeResult; .status is ET_OK or ET_ERR_CAP (nothing written, .out_bytes = the room needed); any other
        failure of the call raises.  Stream-ordered like take_packed_device."""
        n = text_index.numel() - 1
        n_rows = n if rows is None else rows.numel()
        what = "rows, first and count are ints or 1-D CUDA tensors of 32-bit integers"
        first_p, first_v = (None, int(first)) if isinstance(first, (int, np.integer)) else (self._rows_ptr(first, what), 0)
        count_p, count_v = (None, int(count)) if isinstance(count, (int, np.integer)) else (self._rows_ptr(count, what), 0)
        assert all(p is None or t.numel() >= n_rows for p, t in ((first_p, first), (count_p, count))), "first and count hold a value per row"
        if stop is None:
            stop = SLICE_NO_STOP
        elif not isinstance(stop, (int, np.integer)):
            (stop,) = bytes(stop)
        res = N.TakeResult()
        self._bind()
        rc = N.lib().et_slice_packed_device(self._h, ctypes.byref(codebook.raw), bodies.data_ptr(), bodies.numel(), self._index_ptr(body_index, n), self._index_ptr(text_index), n,
                                            None if rows is None else self._rows_ptr(rows, what), n_rows, first_p, first_v, count_p, count_v, int(stop),
                                            self._opt_ptr(out), 0 if out is None else out.numel(), self._index_ptr(out_body_index, n_rows),
                                            self._index_ptr(out_text_index, n_rows), self._opt_ptr(status), ctypes.byref(res))
        return self._take_result(rc, res)

    def number_packed_device(self, codebook, bodies, body_index, text_index, rows, first, count, stop=None, values=None, kind=None, group_of=None, n_groups=None, sum=None,
                             n=None, min=None, max=None, status=None):
        """text[first : first + count] of record rows[k] of the store (slice_packed_device's store, rows, first, count and stop, word
        for word), cut in front of the first byte `stop`, READ as an integer of the grammar [+-]?[0-9]+ on the compressed bytes, nothing
        decoded.  values: optional int64 CUDA tensor of one entry per row: the value, 0 unless the row is NUMBER_OK.  kind: optional
        uint8 CUDA tensor of one entry per row: NUMBER_OK, NUMBER_EMPTY (the empty text: SQL's NULL; also a failed row), NUMBER_BAD (not
        of the grammar, or more than 32 symbols), NUMBER_RANGE (outside int64).  sum, n, min, max: optional int64 CUDA tensors of
        n_groups entries each (n holds u64 counts): the aggregates over the NUMBER_OK rows of each group, initialised by the call --
        0, 0, INT64_MAX, INT64_MIN --, the sum modulo 2^64.  group_of: int32/uint32 CUDA tensor of one group number per ROW
        (group_packed_device's group_of when rows is None; GROUP_NONE skips the row, any other number >= n_groups fails it); None:
        every row is in group 0 and n_groups is 1.  status: optional uint8 CUDA tensor of one et_status byte per ROW.  With no output
        the call only counts.  -> NumberResult; any failure of the call raises.  Stream-ordered like slice_packed_device."""
        n_records = text_index.numel() - 1
        n_rows = n_records if rows is None else rows.numel()
        what = "rows, first, count and group_of are ints or 1-D CUDA tensors of 32-bit integers"
        first_p, first_v = (None, int(first)) if isinstance(first, (int, np.integer)) else (self._rows_ptr(first, what), 0)
        count_p, count_v = (None, int(count)) if isinstance(count, (int, np.integer)) else (self._rows_ptr(count, what), 0)
        assert all(p is None or t.numel() >= n_rows for p, t in ((first_p, first), (count_p, count))), "first and count hold a value per row"
        if stop is None:
            stop = SLICE_NO_STOP
        elif not isinstance(stop, (int, np.integer)):
            (stop,) = bytes(stop)
        aggregates = [t for t in (sum, n, min, max) if t is not None]
        if n_groups is None:
            n_groups = 1 if aggregates and group_of is None else aggregates[0].numel() if aggregates else 0
        for t in aggregates + ([] if values is None else [values]):
            assert t.is_cuda and t.dim() == 1 and t.element_size() == 8 and t.is_contiguous() and not t.is_floating_point(), "values and the aggregates are 1-D CUDA tensors of 64-bit integers"
        assert all(t.numel() >= n_groups for t in aggregates), "an aggregate holds an entry per group"
        assert values is None or values.numel() >= n_rows, "values holds an entry per row"
        assert kind is None or (kind.is_cuda and kind.element_size() == 1 and kind.is_contiguous() and kind.numel() >= n_rows), "kind is a CUDA tensor of one byte per row"
        assert group_of is None or group_of.numel() >= n_rows, "group_of holds an entry per row"
        res = N.NumberResult()
        self._bind()
        rc = N.lib().et_number_packed_device(self._h, ctypes.byref(codebook.raw), bodies.data_ptr(), bodies.numel(), self._index_ptr(body_index, n_records),
                                             self._index_ptr(text_index), n_records, None if rows is None else self._rows_ptr(rows, what), n_rows, first_p, first_v, count_p,
                                             count_v, int(stop), self._opt_ptr(values), self._opt_ptr(kind), None if group_of is None else self._rows_ptr(group_of, what),
                                             int(n_groups), self._opt_ptr(sum), self._opt_ptr(n), self._opt_ptr(min), self._opt_ptr(max), self._opt_ptr(status), ctypes.byref(res))
        _check(rc, self._h)
        return NumberResult(rc, res.n_ok, res.n_empty, res.n_bad, res.n_range, res.n_failed, res.first_failed, res.first_status)

    def field_packed_device(self, codebook, bodies, body_index, text_index, rows, field, n_fields, delim, out, out_body_index, out_text_index, pos=None, status=None):
        """Row k of the NEW store is delim.join(text.split(delim)[field : field + n_fields]) of record rows[k] of the store (bodies,
        body_index, text_index: take_packed_device's; rows=None: row k is record k) -- SPLIT_PART, found and copied on the compressed
        bytes, nothing decoded: its body, as encode_packed_device would write it under `codebook`, goes to
        out[out_body_index[k] : out_body_index[k + 1]], and out_text_index[k + 1] - out_text_index[k] is its length.  field (from 0),
        n_fields: an int for every row, or an int32/uint32 CUDA tensor of one value per row; n_fields=FIELD_TO_END: every field from
        `field` on.  delim: an int 0 .. 255, or one byte.  pos: optional int32/uint32 CUDA tensor of one value per row: the symbol at
        which the field begins, FIELD_ABSENT when the record has no such field (the row is then the empty record, its status ET_OK)
        and for a failed row.  status: optional uint8 CUDA tensor of one et_status byte per ROW; a row that fails becomes an empty
        record.  out=None: sizes only (pos is written).  out may not overlap bodies.  -> TakeResult; .status is ET_OK or ET_ERR_CAP
        (nothing written, .out_bytes = the room needed); any other failure of the call raises.  Stream-ordered like
        take_packed_device."""
        n = text_index.numel() - 1
        n_rows = n if rows is None else rows.numel()
        what = "rows, field, n_fields and pos are ints or 1-D CUDA tensors of 32-bit integers"
        field_p, field_v = (None, int(field)) if isinstance(field, (int, np.integer)) else (self._rows_ptr(field, what), 0)
        count_p, count_v = (None, int(n_fields)) if isinstance(n_fields, (int, np.integer)) else (self._rows_ptr(n_fields, what), 0)
        assert all(p is None or t.numel() >= n_rows for p, t in ((field_p, field), (count_p, n_fields))), "field and n_fields hold a value per row"
        assert pos is None or pos.numel() >= n_rows, "pos holds a value per row"
        if not isinstance(delim, (int, np.integer)):
            (delim,) = bytes(delim)
        res = N.TakeResult()
        self._bind()
        rc = N.lib().et_field_packed_device(self._h, ctypes.byref(codebook.raw), bodies.data_ptr(), bodies.numel(), self._index_ptr(body_index, n), self._index_ptr(text_index), n,
                                            None if rows is None else self._rows_ptr(rows, what), n_rows, field_p, field_v, count_p, count_v, int(delim),
                                            self._opt_ptr(out), 0 if out is None else out.numel(), self._index_ptr(out_body_index, n_rows),
                                            self._index_ptr(out_text_index, n_rows), None if pos is None else self._rows_ptr(pos, what), self._opt_ptr(status),
                                            ctypes.byref(res))
        return self._take_result(rc, res)

    def concat_packed_device(self, codebook, a, sep, b, out, out_body_index, out_text_index, rows_a=None, rows_b=None, status=None):
        """Row k of the NEW store is text(A[rows_a[k]]) + sep + text(B[rows_b[k]]), text() the record's stored text -- row-wise string
        concatenation on the compressed bytes, nothing decoded: the left stored text's bits, sep's bits under `codebook` and the right
        stored text's bits laid end to end.  Both sides are walked to the end of their stored text, as slice_packed_device walks: the
        pad bits of either body are masked, not copied, a record kept raw (no bytes under a length) is the empty text on either side,
        and out_text_index advances by the SYMBOLS of the three -- not by the right record's length where its body ends before it.
        For every input the row is exactly what encode_packed_device writes for the concatenated stored texts.  a, b: (bodies, body_index, text_index) as
        take_packed_device takes a store, or None for an absent side (prefix or suffix every record; not both); they may be the same
        store.  sep: bytes, at most concat_sep_max() of them.  rows_a, rows_b: int32/uint32 CUDA tensors of one record number per row
        (any order, repeats allowed), or None: row k is record k of that side.  A row fails -- the empty record -- with the left
        record's status if that is not OK, else the right's, else ET_ERR_UNSUPPORTED for a new length above batch small_max.
        out=None: sizes only.  out may not overlap either side's bodies.  -> TakeResult; .status is ET_OK or ET_ERR_CAP (nothing
        written, .out_bytes = the room needed); any other failure of the call raises.  Stream-ordered like take_packed_device."""
        sep_a, sep_p = _host_u8(bytes(sep))
        what = "rows_a and rows_b are 1-D CUDA tensors of 32-bit integers"
        sides, counts = [], []
        for store, rows in ((a, rows_a), (b, rows_b)):
            if store is None:
                sides += [None, 0, None, None, 0, None]
                continue
            bodies, body_index, text_index = store
            n = text_index.numel() - 1
            sides += [bodies.data_ptr(), bodies.numel(), self._index_ptr(body_index, n), self._index_ptr(text_index), n, None if rows is None else self._rows_ptr(rows, what)]
            counts.append(n if rows is None else rows.numel())
        assert counts and min(counts) == max(counts), "at least one side, and both sides give the same number of rows"
        n_rows = counts[0]
        res = N.TakeResult()
        self._bind()
        rc = N.lib().et_concat_packed_device(self._h, ctypes.byref(codebook.raw), *sides[:6], sep_p, sep_a.size, *sides[6:], n_rows, self._opt_ptr(out),
                                             0 if out is None else out.numel(), self._index_ptr(out_body_index, n_rows), self._index_ptr(out_text_index, n_rows),
                                             self._opt_ptr(status), ctypes.byref(res))
        return self._take_result(rc, res)

    def recode_packed_device(self, codebook_in, codebook_out, bodies, body_index, text_index, rows, out, out_body_index, out_text_index, byte_map=None, status=None):
        """Row k of the NEW store is the stored text of record rows[k] of the store (bodies, body_index, text_index:
        take_packed_device's, written under `codebook_in`; rows=None: row k is record k) sent through `byte_map` and written under
        `codebook_out` -- text.translate(table, delete) and a change of table in one pass over the compressed bytes, no text in
        between: its body, as encode_packed_device would write it under codebook_out, goes to
        out[out_body_index[k] : out_body_index[k + 1]], and out_text_index[k + 1] - out_text_index[k] is its length.  byte_map: None
        (the identity), or 256 integers (byte_map(), ASCII_UPPER, ASCII_LOWER): entry c is the byte c becomes, RECODE_DROP deletes it.
        codebook_out may be codebook_in; the identity under one table normalises the store (pad bits cleared, lengths cut to what the
        bodies hold).  A row fails -- the empty record -- as slice_packed_device's rows do, or with ET_ERR_UNSUPPORTED where a kept byte
        of its stored text has no code under codebook_out.  status: optional uint8 CUDA tensor of one et_status byte per ROW.
        out=None: sizes only.  out may not overlap bodies.  -> TakeResult; .status is ET_OK or ET_ERR_CAP (nothing written,
        .out_bytes = the room needed); any other failure of the call raises.  Stream-ordered like take_packed_device."""
        n = text_index.numel() - 1
        n_rows = n if rows is None else rows.numel()
        map_p = None
        if byte_map is not None:
            wide = np.asarray(byte_map)
            assert wide.shape == (256,) and wide.dtype.kind in "iu", "byte_map holds 256 integers"
            assert ((wide >= -32768) & (wide <= 32767)).all(), "a map entry is a byte, or RECODE_DROP"  # (what does not fit 16 bits is no byte either)
            map_a = np.ascontiguousarray(wide, dtype=np.int16)
            map_p = map_a.ctypes.data_as(ctypes.c_void_p)
        res = N.TakeResult()
        self._bind()
        rc = N.lib().et_recode_packed_device(self._h, ctypes.byref(codebook_in.raw), ctypes.byref(codebook_out.raw), map_p, bodies.data_ptr(), bodies.numel(),
                                             self._index_ptr(body_index, n), self._index_ptr(text_index), n, None if rows is None else self._rows_ptr(rows), n_rows,
                                             self._opt_ptr(out), 0 if out is None else out.numel(), self._index_ptr(out_body_index, n_rows),
                                             self._index_ptr(out_text_index, n_rows), self._opt_ptr(status), ctypes.byref(res))
        return self._take_result(rc, res)

    def _packed_upload(self, blob, index):
        """-> (the bytes on the device, in a tensor that is never empty: one spare byte behind an empty blob; the offsets)."""
        import torch

        dev = torch.device("cuda", self.device)
        d = torch.empty(max(blob.size, 1), dtype=torch.uint8, device=dev)
        d[: blob.size] = torch.from_numpy(blob).to(dev)
        return d, torch.from_numpy(np.ascontiguousarray(index, dtype=np.uint64).view(np.int64)).to(dev)

    def encode_packed(self, codebook, texts):
        """[bytes] -> (the bodies back to back as bytes, out_index as a numpy u64 array of len(texts) + 1): ONE encode_packed_device
        call.  Raises EntreepyError naming the first item that failed (a byte the table has no code for)."""
        import torch

        texts = [np.frombuffer(bytes(t), dtype=np.uint8) for t in texts]
        if not texts:
            return b"", np.zeros(1, np.uint64)
        index = np.concatenate(([0], np.cumsum([t.size for t in texts]))).astype(np.uint64)
        d_text, d_index = self._packed_upload(np.concatenate(texts), index)
        d_out = torch.empty(max(codebook.body_bound(int(index[-1])) + len(texts), 1), dtype=torch.uint8, device=d_text.device)  # (each body rounds up to a byte)
        d_out_index = torch.empty(len(texts) + 1, dtype=torch.int64, device=d_text.device)
        res = self.encode_packed_device(codebook, d_text, d_index, d_out, d_out_index)
        _check(res.status, self._h)
        if res.n_failed:
            raise EntreepyError(res.first_status, f"encode_packed: item {res.first_failed}")
        return d_out[: res.out_bytes].cpu().numpy().tobytes(), d_out_index.cpu().numpy().view(np.uint64)  # (the copies run behind the call's kernels)

    def decode_packed(self, codebook, blob, out_index, lengths):
        """The bodies back to back, their offsets (encode_packed's pair) and the records' lengths -> [their texts] (shorter where a
        body ends early)."""
        import torch

        out_index = np.asarray(out_index, dtype=np.uint64)
        assert out_index.size == len(lengths) + 1
        if not len(lengths):
            return []
        text_index = np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.uint64)))).astype(np.uint64)
        d_blob, d_body_index = self._packed_upload(np.array(np.frombuffer(bytes(blob), dtype=np.uint8)), out_index)
        d_text_index = torch.from_numpy(text_index.view(np.int64)).to(d_blob.device)
        d_out = torch.empty(max(int(text_index[-1]), 1), dtype=torch.uint8, device=d_blob.device)
        d_written = torch.empty(len(lengths), dtype=torch.int32, device=d_blob.device)
        res = self.decode_packed_device(codebook, d_blob, d_body_index, d_text_index, d_out, written=d_written)
        _check(res.status, self._h)
        if res.n_failed:
            raise EntreepyError(res.first_status, f"decode_packed: item {res.first_failed}")
        host, written = d_out.cpu().numpy(), d_written.cpu().numpy()  # (a body that ends early gives the shorter text, as decode_shared)
        return [host[int(a) : int(a) + int(w)].tobytes() for a, w in zip(text_index[:-1], written)]

    def decode_packed_rows(self, codebook, blob, out_index, lengths, rows):
        """decode_packed's store and a list of record numbers (any order, repeats allowed) -> [the texts of those records], through
        one decode_packed_gather_device call."""
        import torch

        out_index = np.asarray(out_index, dtype=np.uint64)
        lengths = np.asarray(lengths, dtype=np.uint64)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        assert out_index.size == lengths.size + 1
        if not rows.size:
            return []
        text_index = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
        d_blob, d_body_index = self._packed_upload(np.array(np.frombuffer(bytes(blob), dtype=np.uint8)), out_index)
        d_text_index = torch.from_numpy(text_index.view(np.int64)).to(d_blob.device)
        d_rows = torch.from_numpy(rows.view(np.int32)).to(d_blob.device)
        room = int(lengths[rows[rows < lengths.size]].sum())  # (a row beyond the store fails below, and takes none)
        d_out = torch.empty(max(room, 1), dtype=torch.uint8, device=d_blob.device)
        d_rows_index = torch.empty(rows.size + 1, dtype=torch.int64, device=d_blob.device)
        d_written = torch.empty(rows.size, dtype=torch.int32, device=d_blob.device)
        res = self.decode_packed_gather_device(codebook, d_blob, d_body_index, d_text_index, d_rows, d_out, d_rows_index, written=d_written)
        _check(res.status, self._h)
        if res.n_failed:
            raise EntreepyError(res.first_status, f"decode_packed_rows: row {res.first_failed}")
        host, at, written = d_out.cpu().numpy(), d_rows_index.cpu().numpy(), d_written.cpu().numpy()  # (the copies run behind the call's kernels)
        return [host[int(a) : int(a) + int(w)].tobytes() for a, w in zip(at[:-1], written)]

    def match_packed(self, codebook, blob, out_index, lengths, needle, mode):
        """decode_packed's store, a needle and a mode -> [the numbers of the records that match], ascending, through one
        match_packed_device call: what decode_packed_rows takes."""
        import torch

        out_index, lengths = self._store_arrays(out_index, lengths)
        if not lengths.size:
            return []
        store = self._store_upload(blob, out_index, lengths)
        d_rows = torch.empty(lengths.size, dtype=torch.int32, device=store[0].device)
        res = self.match_packed_device(codebook, *store, needle, mode, rows=d_rows)
        _check(res.status, self._h)
        self._raise_failed(res, "match_packed")
        return d_rows[: res.n_match].cpu().numpy().view(np.uint32).tolist()  # (the copy runs behind the call's kernels)

    def search_packed(self, codebook, blob, out_index, lengths, needle, mode):
        """decode_packed's store, a needle and a mode -> ([the numbers of the records that contain the needle, or end with it],
        ascending, [where in each]) through one search_packed_device call; with MATCH_NOT the records that do not, and no positions."""
        import torch

        out_index, lengths = self._store_arrays(out_index, lengths)
        if not lengths.size:
            return [], []
        store = self._store_upload(blob, out_index, lengths)
        d_rows = torch.empty(lengths.size, dtype=torch.int32, device=store[0].device)
        d_pos = None if mode & MATCH_NOT else torch.empty_like(d_rows)
        res = self.search_packed_device(codebook, *store, needle, mode, rows=d_rows, pos=d_pos)
        _check(res.status, self._h)
        self._raise_failed(res, "search_packed")
        rows = d_rows[: res.n_match].cpu().numpy().view(np.uint32).tolist()  # (the copies run behind the call's kernels)
        return rows, [] if d_pos is None else d_pos[: res.n_match].cpu().numpy().view(np.uint32).tolist()

    def join_packed(self, codebook, blob, out_index, lengths, key_blob, key_index, key_lengths, mode=0):
        """decode_packed's store and a key set of the same form (e.g. encode_packed's of the keys) -> [the numbers of the records that
        equal some key] -- with MATCH_NOT those that equal none --, ascending, through one join_packed_device call."""
        import torch

        (out_index, lengths), (key_index, key_lengths) = self._store_arrays(out_index, lengths), self._store_arrays(key_index, key_lengths)
        if not lengths.size:
            return []
        store, keys = self._store_upload(blob, out_index, lengths), self._store_upload(key_blob, key_index, key_lengths)
        d_rows = torch.empty(lengths.size, dtype=torch.int32, device=store[0].device)
        res = self.join_packed_device(codebook, *store, *keys, mode=mode, rows=d_rows)
        _check(res.status, self._h)
        self._raise_failed(res, "join_packed")
        if res.n_keys_failed:
            raise EntreepyError(res.first_key_status, f"join_packed: key {res.first_key_failed}")
        return d_rows[: res.n_match].cpu().numpy().view(np.uint32).tolist()  # (the copy runs behind the call's kernels)

    def group_packed(self, codebook, blob, out_index, lengths):
        """decode_packed's store -> (first_rows, counts, group_of) as numpy u32 arrays: each distinct text's first record, ascending,
        how many records hold it, and every record's group -- through a count-only group_packed_device call, then the writing one."""
        import torch

        out_index, lengths = self._store_arrays(out_index, lengths)
        if not lengths.size:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        store = self._store_upload(blob, out_index, lengths)
        dev = store[0].device
        res = self.group_packed_device(codebook, *store)
        self._raise_failed(res, "group_packed")
        d_first, d_count = (torch.empty(max(res.n_groups, 1), dtype=torch.int32, device=dev) for _ in range(2))
        d_group_of = torch.empty(lengths.size, dtype=torch.int32, device=dev)
        res = self.group_packed_device(codebook, *store, first_rows=d_first, count=d_count, group_of=d_group_of)
        _check(res.status, self._h)
        host = lambda t, k: t[:k].cpu().numpy().view(np.uint32)  # (the copies run behind the call's kernels)
        return host(d_first, res.n_groups), host(d_count, res.n_groups), host(d_group_of, lengths.size)

    # What the list helpers of the selecting and the store-deriving calls share.
    @staticmethod
    def _raise_failed(res, what):
        """The first failed record of a call, as an EntreepyError."""
        if res.n_failed:
            raise EntreepyError(res.first_status, f"{what}: record {res.first_failed}")

    @staticmethod
    def _store_arrays(out_index, lengths):
        """decode_packed's offsets and lengths as numpy u64 arrays."""
        out_index = np.asarray(out_index, dtype=np.uint64)
        lengths = np.asarray(lengths, dtype=np.uint64)
        assert out_index.size == lengths.size + 1
        return out_index, lengths

    def _store_upload(self, blob, out_index, lengths):
        """-> (bodies, body_index, text_index) on the device, as take_packed_device takes a store; text_index from the lengths."""
        import torch

        text_index = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
        d_blob, d_body_index = self._packed_upload(np.array(np.frombuffer(bytes(blob), dtype=np.uint8)), out_index)
        return d_blob, d_body_index, torch.from_numpy(text_index.view(np.int64)).to(d_blob.device)

    @staticmethod
    def _per_row(v, n_rows, dev):
        """A per-row argument: an int for every row as it is, a list of one value per row as a device tensor."""
        import torch

        if isinstance(v, (int, np.integer)):
            return int(v)
        v = np.ascontiguousarray(v, dtype=np.uint32)
        assert v.size == n_rows
        return torch.from_numpy(v.view(np.int32)).to(dev)

    @staticmethod
    def _bodies_room(out_index, lengths, rows):
        """The bytes of the rows' bodies: room for a result that is no longer than they are.  (A row beyond the store fails in the
        call, and takes none.)"""
        good = rows[rows < lengths.size]
        return int((out_index[good + 1] - out_index[good]).sum())

    @staticmethod
    def _new_store(room, n_rows, dev):
        """-> (out, out_body_index, out_text_index) for a call: `room` bytes, or None for sizes only, and the new index pair."""
        import torch

        d_out = None if room is None else torch.empty(max(room, 1), dtype=torch.uint8, device=dev)
        return d_out, torch.empty(n_rows + 1, dtype=torch.int64, device=dev), torch.empty(n_rows + 1, dtype=torch.int64, device=dev)

    def _store_download(self, what, res, d_out, d_new_index, d_new_text):
        """The end of a list helper: raises for the call or its first failed row, then -> (bodies, offsets, lengths) on the host."""
        _check(res.status, self._h)
        if res.n_failed:
            raise EntreepyError(res.first_status, f"{what}: row {res.first_failed}")
        new_text = d_new_text.cpu().numpy().view(np.uint64)  # (the copies run behind the call's kernels)
        return d_out[: res.out_bytes].cpu().numpy().tobytes(), d_new_index.cpu().numpy().view(np.uint64), np.diff(new_text)

    def take_packed(self, blob, out_index, lengths, rows):
        """decode_packed's store and a list of record numbers (any order, repeats allowed) -> (the bodies of those records back to back
        as bytes, their offsets as a numpy u64 array of len(rows) + 1, their lengths as a numpy u64 array): a store of the same form,
        as encode_packed of those records' texts gives it, through one take_packed_device call."""
        out_index, lengths = self._store_arrays(out_index, lengths)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if not rows.size:
            return b"", np.zeros(1, np.uint64), np.zeros(0, np.uint64)
        store = self._store_upload(blob, out_index, lengths)
        dev = store[0].device
        new = self._new_store(self._bodies_room(out_index, lengths, rows), rows.size, dev)
        res = self.take_packed_device(*store, self._per_row(rows, rows.size, dev), *new)
        return self._store_download("take_packed", res, *new)

    def slice_packed(self, codebook, blob, out_index, lengths, rows, first, count, stop=None):
        """decode_packed's store, a list of record numbers (any order, repeats allowed) and where each row's slice begins and how long
        it is at most (an int for every row, or a list of one per row) -> a store like take_packed's: (the bodies of
        text[first : first + count], cut in front of `stop`, back to back as bytes, their offsets, their lengths), as encode_packed
        of those pieces gives it, through one slice_packed_device call."""
        out_index, lengths = self._store_arrays(out_index, lengths)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if not rows.size:
            return b"", np.zeros(1, np.uint64), np.zeros(0, np.uint64)
        store = self._store_upload(blob, out_index, lengths)
        dev = store[0].device
        first, count, d_rows = (self._per_row(v, rows.size, dev) for v in (first, count, rows))
        new = self._new_store(self._bodies_room(out_index, lengths, rows), rows.size, dev)  # (a slice is no longer than its record's body)
        res = self.slice_packed_device(codebook, *store, d_rows, first, count, *new, stop=stop)
        return self._store_download("slice_packed", res, *new)

    def number_packed(self, codebook, blob, out_index, lengths, rows, first, count, stop=None, group_of=None, n_groups=None):
        """decode_packed's store, a list of record numbers (any order, repeats allowed) and slice_packed's first, count and stop ->
        (values as a numpy int64 array, kinds as a numpy u8 array) of text[first : first + count] read as integers, through one
        number_packed_device call.  With n_groups (and group_of: a list of one group number per row; None: one group) also the four
        aggregates: -> (values, kinds, sums, counts, minima, maxima), int64 arrays but the u64 counts.  Raises for a failed row."""
        import torch

        out_index, lengths = self._store_arrays(out_index, lengths)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if n_groups is None and group_of is not None:
            raise ValueError("group_of needs n_groups")
        if not rows.size:
            empty = (np.zeros(0, np.int64), np.zeros(0, np.uint8))
            if n_groups is None:
                return empty
            g = int(n_groups)
            return empty + (np.zeros(g, np.int64), np.zeros(g, np.uint64), np.full(g, np.iinfo(np.int64).max), np.full(g, np.iinfo(np.int64).min))
        store = self._store_upload(blob, out_index, lengths)
        dev = store[0].device
        first, count, d_rows = (self._per_row(v, rows.size, dev) for v in (first, count, rows))
        d_values, d_kind = torch.empty(rows.size, dtype=torch.int64, device=dev), torch.empty(rows.size, dtype=torch.uint8, device=dev)
        agg = {} if n_groups is None else {k: torch.empty(int(n_groups), dtype=torch.int64, device=dev) for k in ("sum", "n", "min", "max")}
        d_group_of = None if group_of is None else self._per_row(list(group_of), rows.size, dev)
        res = self.number_packed_device(codebook, *store, d_rows, first, count, stop=stop, values=d_values, kind=d_kind, group_of=d_group_of,
                                        n_groups=None if n_groups is None else int(n_groups), **agg)
        if res.n_failed:
            raise EntreepyError(res.first_status, f"number_packed: row {res.first_failed}")
        out = (d_values.cpu().numpy(), d_kind.cpu().numpy())  # (the copies run behind the call's kernels)
        if n_groups is None:
            return out
        return out + (agg["sum"].cpu().numpy(), agg["n"].cpu().numpy().view(np.uint64), agg["min"].cpu().numpy(), agg["max"].cpu().numpy())

    def field_packed(self, codebook, blob, out_index, lengths, rows, field, n_fields=1, delim=b","):
        """decode_packed's store, a list of record numbers (any order, repeats allowed), each row's first field (from 0) and how many
        fields it takes (an int for every row, or a list of one per row) -> a store like take_packed's and the fields' positions:
        (the bodies of delim.join(text.split(delim)[field : field + n_fields]) back to back as bytes, their offsets, their lengths,
        pos as a numpy u32 array: the symbol at which each field begins, FIELD_ABSENT where the record has no such field -- that row
        is the empty record), through one field_packed_device call."""
        import torch

        out_index, lengths = self._store_arrays(out_index, lengths)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if not rows.size:
            return b"", np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        store = self._store_upload(blob, out_index, lengths)
        dev = store[0].device
        field, n_fields, d_rows = (self._per_row(v, rows.size, dev) for v in (field, n_fields, rows))
        new = self._new_store(self._bodies_room(out_index, lengths, rows), rows.size, dev)  # (a field is no longer than its record's body)
        d_pos = torch.empty(rows.size, dtype=torch.int32, device=dev)
        res = self.field_packed_device(codebook, *store, d_rows, field, n_fields, delim, *new, pos=d_pos)
        return (*self._store_download("field_packed", res, *new), d_pos.cpu().numpy().view(np.uint32))

    def concat_packed(self, codebook, a, sep, b, rows_a=None, rows_b=None):
        """Two stores as decode_packed takes them -- a, b: (blob, out_index, lengths), or None for an absent side -- a literal and a
        list of record numbers per side (None: row k is record k) -> a store like take_packed's: (the bodies of
        text(a[rows_a[k]]) + sep + text(b[rows_b[k]]) back to back as bytes, their offsets, their lengths), as encode_packed of the
        concatenated texts gives it, through one concat_packed_device call."""
        import torch

        dev = torch.device("cuda", self.device)
        stores, d_rows, counts, room = [], [], [], 0
        for store, rows in ((a, rows_a), (b, rows_b)):
            if store is None:
                stores.append(None)
                d_rows.append(None)
                continue
            blob, out_index, lengths = store
            out_index, lengths = self._store_arrays(out_index, lengths)
            stores.append(self._store_upload(blob, out_index, lengths))
            rows = np.arange(lengths.size, dtype=np.uint32) if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
            d_rows.append(self._per_row(rows, rows.size, dev))
            counts.append(rows.size)
            room += self._bodies_room(out_index, lengths, rows)  # (a run is no longer than its record's body)
        assert counts and min(counts) == max(counts), "at least one side, and both sides give the same number of rows"
        n_rows = counts[0]
        if not n_rows:
            return b"", np.zeros(1, np.uint64), np.zeros(0, np.uint64)
        room += n_rows * (codebook.body_bound(len(bytes(sep))) + 1)  # (the literal's bits per row, and the byte a row rounds up to)
        new = self._new_store(room, n_rows, dev)
        res = self.concat_packed_device(codebook, stores[0], sep, stores[1], *new, rows_a=d_rows[0], rows_b=d_rows[1])
        return self._store_download("concat_packed", res, *new)

    def recode_packed(self, codebook_in, codebook_out, blob, out_index, lengths, rows=None, byte_map=None):
        """decode_packed's store under `codebook_in`, a list of record numbers (None: row k is record k) and a map -> a store like
        take_packed's under `codebook_out`: (the bodies of the rows' texts sent through the map, back to back as bytes, their
        offsets, their lengths), as encode_packed of the translated texts gives it, through two recode_packed_device calls: the
        sizes, then the bytes."""
        import torch

        out_index, lengths = self._store_arrays(out_index, lengths)
        rows = np.arange(lengths.size, dtype=np.uint32) if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
        if not rows.size:
            return b"", np.zeros(1, np.uint64), np.zeros(0, np.uint64)
        store = self._store_upload(blob, out_index, lengths)
        dev = store[0].device
        args = (codebook_in, codebook_out, *store, self._per_row(rows, rows.size, dev))
        new = self._new_store(None, rows.size, dev)
        sizes = self.recode_packed_device(*args, *new, byte_map=byte_map)  # (a new body may be longer than the old: ask)
        new = (torch.empty(max(sizes.out_bytes, 1), dtype=torch.uint8, device=dev), *new[1:])
        res = self.recode_packed_device(*args, *new, byte_map=byte_map)
        return self._store_download("recode_packed", res, *new)


    # -- staged calls (sharded encode) ----------------------------------------------
    def histogram_device(self, text, hist):
        """text: uint8 CUDA tensor; hist: int64/uint64 CUDA tensor of 256 counters."""
        self._bind()
        assert hist.numel() == 256 and hist.element_size() == 8
        _check(N.lib().et_histogram_device(self._h, text.data_ptr(), text.numel(), hist.data_ptr()), self._h)

    def histogram_host(self):
        """The counts of the last histogram_device call on the host (uint64[256]): waits for them, no copy command."""
        c = np.zeros(256, dtype=np.uint64)
        _check(N.lib().et_histogram_host(self._h, c.ctypes.data), self._h)
        return c

    def histogram_on_host(self, counts):
        """The counts of the last histogram_device call, already on the host (uint64[256])."""
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        assert c.size == 256
        _check(N.lib().et_histogram_on_host(self._h, c.ctypes.data), self._h)

    def encode_body_device(self, codebook, text, out, start_bit=0):
        self._bind()
        end = ctypes.c_uint64(0)
        _check(N.lib().et_encode_body_device(self._h, ctypes.byref(codebook.raw), text.data_ptr(), text.numel(), out.data_ptr(),
                                             out.numel() * out.element_size(), int(start_bit), ctypes.byref(end)), self._h)
        return end.value

    def encode_head_shard_device(self, codebook, text, out, header):
        """Shard 0 of a sharded encode: file header followed by the shard's body."""
        self._bind()
        end = ctypes.c_uint64(0)
        hb = np.frombuffer(header, dtype=np.uint8)
        _check(N.lib().et_encode_head_shard_device(self._h, ctypes.byref(codebook.raw), text.data_ptr(), text.numel(), out.data_ptr(),
                                                   out.numel() * out.element_size(), hb.ctypes.data, hb.size, ctypes.byref(end)), self._h)
        return end.value

    def decode_body_device(self, codebook, body, n_symbols, out, start_bit=0):
        self._bind()
        n = ctypes.c_size_t(0)
        _check(N.lib().et_decode_body_device(self._h, ctypes.byref(codebook.raw), body.data_ptr(), body.numel(), int(start_bit),
                                             int(n_symbols), out.data_ptr(), out.numel(), ctypes.byref(n)), self._h)
        return n.value


    def decode_range_sync(self, codebook, stream, begin, end, in_start_bit=-1):
        """One rank's part of a cold multi-GPU decode: synchronise the codewords that begin
        in stream[begin:end] (uint8 device tensor of the body from its 4-byte aligned base;
        begin a multiple of 8192, end too unless it is the stream's end).  Call again with
        the predecessor's exit as in_start_bit to repair.  -> dict(start_bit, exit_bit,
        n_symbols, sweeps)."""
        self._bind()
        info = N.RangeInfo()
        tail = stream.numel() - end
        _check(N.lib().et_decode_range_sync(self._h, ctypes.byref(codebook.raw), stream.data_ptr() + begin, end - begin, tail,
                                            int(begin >= 16), int(in_start_bit), ctypes.byref(info)), self._h)
        return {"start_bit": info.start_bit, "exit_bit": info.exit_bit, "n_symbols": info.n_symbols, "sweeps": info.sweeps,
                "tree_walk": info.reserved == 2}

    def decode_range_maps(self, codebook, stream, begin, end, in_start_bit=-1):
        """Exhaustive variant of decode_range_sync for codes that do not self-synchronise:
        -> (map, n_starts), map[p] = exit bit of the range when its first codeword begins
        p bits in (p < n_starts; constant when in_start_bit >= 0).  Follow with
        decode_range_resolve(start) once the start is known."""
        self._bind()
        m = (ctypes.c_uint8 * 32)()
        k = ctypes.c_uint32(0)
        tail = stream.numel() - end
        _check(N.lib().et_decode_range_maps(self._h, ctypes.byref(codebook.raw), stream.data_ptr() + begin, end - begin, tail, int(in_start_bit),
                                            ctypes.byref(m), ctypes.byref(k)), self._h)
        return bytes(m), k.value

    def decode_range_resolve(self, in_start_bit):
        self._bind()
        info = N.RangeInfo()
        _check(N.lib().et_decode_range_resolve(self._h, int(in_start_bit), ctypes.byref(info)), self._h)
        return {"start_bit": info.start_bit, "exit_bit": info.exit_bit, "n_symbols": info.n_symbols, "sweeps": info.sweeps, "row_walk": info.reserved == 3}

    def decode_range_write(self, max_symbols, out):
        self._bind()
        n = ctypes.c_size_t(0)
        _check(N.lib().et_decode_range_write(self._h, int(max_symbols), out.data_ptr(), out.numel(), ctypes.byref(n)), self._h)
        return n.value


class Group:
    """One rank's et_group: a Context plus how the ranks exchange small host buffers.

    allgather: callable(bytes of this rank) -> bytes of all ranks in rank order (any transport:
    torch.distributed over gloo, MPI, threads ...), or rccl_id: the 128-byte id rank 0 got from
    Group.rccl_unique_id(), for an RCCL communicator of the library's own over xGMI.

    All ranks make the same calls in the same order.  A call in which any rank fails raises on EVERY rank
    (the rows of each exchange carry the ranks' statuses; include/entreepy_hip.h, "FAILURES").

    lib: the loaded library whose group entry points are called (default: libentreepy_hip.so).  The CPU tests
    pass a build of the same sequence (csrc/et_shard_seq.cpp) over a stand-in for the GPU."""

    def __init__(self, ctx, rank, world, allgather=None, rccl_id=None, lib=None):
        import weakref

        self.ctx, self.rank, self.world = ctx, rank, world
        self._lib = lib if lib is not None else N.lib()
        self._h = ctypes.c_void_p()
        self._py_gather = allgather
        self._cb = N.ALLGATHER_FN(self._gather)  # kept alive with the group
        ctx_h = getattr(ctx, "_h", None)
        if rccl_id is not None:
            ident = (ctypes.c_uint8 * N.ET_RCCL_ID_BYTES).from_buffer_copy(bytes(rccl_id))
            _check(self._lib.et_group_create_rccl(ctx_h, rank, world, ctypes.byref(ident), ctypes.byref(self._h)), ctx_h)
        else:
            _check(self._lib.et_group_create(ctx_h, rank, world, self._cb if allgather else ctypes.cast(None, N.ALLGATHER_FN), None, ctypes.byref(self._h)),
                   ctx_h if lib is None else None)
        if hasattr(ctx, "_groups"):
            ctx._groups.append(weakref.ref(self))

    @staticmethod
    def rccl_unique_id():
        ident = (ctypes.c_uint8 * N.ET_RCCL_ID_BYTES)()
        _check(N.lib().et_rccl_unique_id(ctypes.byref(ident)))
        return bytes(ident)

    def _gather(self, user, send, recv, nbytes):
        try:
            got = self._py_gather(ctypes.string_at(send, nbytes))
            if len(got) != nbytes * self.world:
                return 1
            ctypes.memmove(recv, got, len(got))
            return 0
        except Exception:  # noqa: BLE001 -- reported to the C caller as a failed exchange
            return 1

    def _bind_ctx(self):
        """The group's context onto torch's current stream (Context._bind); the CPU stand-in's contexts have no stream."""
        b = getattr(self.ctx, "_bind", None)
        if b is not None:
            b()

    def _ck(self, status):
        if status == N.ET_OK:
            return
        detail = self._lib.et_group_last_error(self._h).decode()
        if status == N.ET_ERR_EMPTY:
            raise EmptyInputError(status, detail)
        raise EntreepyError(status, detail)

    def close(self):
        if self._h:
            self._lib.et_group_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def force_collectives(self, on=True):
        """A group of one takes the transport's path all the same (one-GPU tests of the N > 1 path)."""
        self._ck(self._lib.et_group_set_option(self._h, N.ET_GROUP_FORCE_COLLECTIVES, int(bool(on))))

    def set_timeout_ms(self, ms):
        self._ck(self._lib.et_group_set_option(self._h, N.ET_GROUP_TIMEOUT_MS, int(ms)))

    @staticmethod
    def _info(i):
        return {k: getattr(i, k) for k, _ in N.ShardInfo._fields_}

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t is not None and t.numel() else None

    def encode_sharded(self, text, out):
        """et_encode_sharded: this rank's chunk (uint8 tensor, may be empty) -> its piece of the image in `out`."""
        self._bind_ctx()
        i = N.ShardInfo()
        self._ck(self._lib.et_encode_sharded(self._h, self._ptr(text), text.numel(), out.data_ptr() if out is not None else None,
                                             out.numel() if out is not None else 0, ctypes.byref(i)))
        return self._info(i)

    def merge_seams(self, out):
        self._bind_ctx()
        self._ck(self._lib.et_shard_merge_seams(self._h, out.data_ptr() if out is not None else None))

    def write_fd(self, out, fd):
        self._bind_ctx()
        self._ck(self._lib.et_shard_write_fd(self._h, out.data_ptr(), fd))

    def place(self, out, image):
        self._bind_ctx()
        self._ck(self._lib.et_shard_place(self._h, out.data_ptr(), image.data_ptr(), image.numel()))

    def gather(self, out, image, root=0):
        self._bind_ctx()
        self._ck(self._lib.et_shard_gather(self._h, out.data_ptr(), image.data_ptr() if image is not None else None,
                                           image.numel() if image is not None else 0, root))

    def info(self):
        i = N.ShardInfo()
        self._ck(self._lib.et_group_last_info(self._h, ctypes.byref(i)))
        return self._info(i)

    def codebook(self):
        cb = Codebook()
        self._ck(self._lib.et_group_codebook(self._h, ctypes.byref(cb.raw)))
        return cb

    def start_bits(self):
        a = np.zeros(self.world + 1, dtype=np.uint64)
        self._ck(self._lib.et_group_start_bits(self._h, a.ctypes.data))
        return [int(x) for x in a]

    def decode_sharded(self, compressed_text, out):
        """et_decode_sharded: this rank's block range of one cold stream -> (symbols written, index of the first)."""
        self._bind_ctx()
        n = ctypes.c_size_t(0)
        first = ctypes.c_uint64(0)
        self._ck(self._lib.et_decode_sharded(self._h, self._ptr(compressed_text), compressed_text.numel() if compressed_text is not None else 0,
                                             out.data_ptr() if out is not None else None, out.numel() if out is not None else 0, ctypes.byref(n), ctypes.byref(first)))
        return n.value, first.value

    def decode_window(self, head, length):
        """et_decode_shard_window: (offset, bytes) of `compressed` this rank needs besides the dictionary (head =
        the first min(length, 8192) bytes of it, host bytes)."""
        a, p = _host_u8(head)
        off, ln = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(self._lib.et_decode_shard_window(p, a.size, int(length), self.rank, self.world, ctypes.byref(off), ctypes.byref(ln)))
        return off.value, ln.value

    def decode_begin(self, head, length, window, window_off, cap=None):
        """et_decode_sharded_begin (collective): window = uint8 tensor holding bytes [window_off, ...) of `compressed`
        -> (symbols this rank writes, index of the first)."""
        self._bind_ctx()
        a, p = _host_u8(head) if head is not None else (np.zeros(0, dtype=np.uint8), None)
        n, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(self._lib.et_decode_sharded_begin(self._h, p, a.size, int(length), self._ptr(window), int(window_off), window.numel() if window is not None else 0,
                                                   (1 << 64) - 1 if cap is None else int(cap), ctypes.byref(n), ctypes.byref(first)))
        return n.value, first.value

    def decode_write(self, out):
        self._bind_ctx()
        n = ctypes.c_size_t(0)
        self._ck(self._lib.et_decode_sharded_write(self._h, out.data_ptr() if out is not None else None, out.numel() if out is not None else 0, ctypes.byref(n)))
        return n.value


def shard_words(starts, world, rank):
    """et_shard_words: (piece_lo, piece_hi, owned_lo, owned_hi) of `rank`, in 4-byte words of the image."""
    a = np.ascontiguousarray(starts, dtype=np.uint64)
    w = np.zeros(4, dtype=np.uint64)
    _check(N.lib().et_shard_words(a.ctypes.data, world, rank, w.ctypes.data))
    return tuple(int(x) for x in w)


def seam_word(starts, world, rank, first_last):
    """et_seam_word: the word closing `rank`'s owned range merged with the later shards that begin in it, or None."""
    a = np.ascontiguousarray(starts, dtype=np.uint64)
    fl = np.ascontiguousarray(first_last, dtype=np.uint32)
    merged, has = ctypes.c_uint32(0), ctypes.c_int(0)
    _check(N.lib().et_seam_word(a.ctypes.data, world, rank, fl.ctypes.data, ctypes.byref(merged), ctypes.byref(has)))
    return merged.value if has.value else None


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def encode(text, flags=None, device=0):
    """encode.zig:25.  Returns the .et file image (the bytes the reference hands to
    out_writer.writeAll, encode.zig:319).  Raises EmptyInputError on b''."""
    return default_context(device).encode(text)


def decode(compressed_text, flags=None, device=0):
    """decode.zig:13.  `compressed_text` = .et file minus its first 4 bytes."""
    return default_context(device).decode(compressed_text)
