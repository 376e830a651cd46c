"""Many small streams: the batched calls against a loop over the single-stream calls (bench.py is untouched by this).

For each shape (1 024 x 64 KiB and 4 096 x 4 KiB of text-like data, resident in HBM) three legs are timed, each in a child
process of its own so that every leg loads exactly one build of the library:
  single_parent   et_encode_device / et_decode_device, one call per stream -- on the library named by --parent-lib (a build of
                  the commit before the batched calls; it does not export them).  Left out when no such build is given.
  single          the same loop on this tree's library (ET_LIB_PATH, or entreepy_amd/libentreepy_hip.so): shows that the
                  single-stream calls did not move.
  batch           et_encode_batch_device / et_decode_batch_device, one call per shape, on this tree's library -- or on the one
                  named by --batch-lib (a build of the commit before the shared-table calls, to set `shared` against).
  shared          et_encode_shared_device / et_decode_shared_device, one call per shape, on this tree's library: the bodies alone
                  under ONE table built from the histogram of the whole shape's text, each body in a slot of et_body_bound bytes.
                  Also reports what the records take: body_bytes (all bodies), header_bytes (the one header that stores the
                  table) -- against the batch leg's image_bytes (all per-stream .et images).
  packed          et_encode_packed_device / et_decode_packed_device, one call per shape, on this tree's library: text and bodies
                  dense, u64 offsets on the device, under the shared leg's table.  With it runs packed_baseline, what the packed
                  encode replaces -- a sizes-only et_encode_shared_device, a prefix sum on the host, the writing call into the dense
                  layout -- and et_decode_shared_device out of that layout, on this tree's library or on the one named by
                  --batch-lib (a build of the commit before the packed calls).
  gather          et_decode_packed_gather_device, one call per shape and selection, on this tree's library: a selection of the packed
                  leg's records -- every row in order, a random 10 % (ascending, as a filter leaves them), a random permutation of
                  all rows -- decoded into a dense output.  Beside the writing call it times the sizes-only call on the same rows and,
                  for the identity, et_decode_packed_device of the same batch.  With it runs gather_baseline, what the call replaces
                  -- both offset arrays copied to the host, the items and their prefix sum built there, et_decode_shared_device on
                  those items -- on this tree's library or on the one named by --batch-lib (a build of the commit before the call).
  match           et_match_packed_device, one call per shape, selectivity and mode, on this tree's library: the records of a packed
                  store that begin with a 12-byte needle (PREFIX) or equal a whole record of at most 4 096 bytes (EQUAL), at about 0.1 %,
                  10 % and 100 % of the records, with d_rows and count only.  Beside the two shapes it runs on 262 144 key-like records
                  of 16 .. 48 bytes.  With it runs match_baseline, what the call replaces -- et_decode_packed_device of the whole store,
                  then the first L bytes of every record gathered, compared, the lengths tested and nonzero, in torch on the device -- on
                  this tree's library or on the one named by --batch-lib (a build of the commit before the call).  --shapes picks shapes.
  join            et_join_packed_device, one call per key set and selectivity, on this tree's library: the 262 144 key-like records of
                  16 .. 48 bytes against key sets of 16, 1 024 and 65 536 keys (packed stores on the device themselves), about 0.1 % and
                  10 % of the records equal to some key, with d_rows and d_key_of_row, and count only.  With it runs join_baseline, what
                  the call replaces -- one et_match_packed_device(ET_MATCH_EQUAL) per key, the keys' texts on the host, then the union of
                  their rows sorted in torch -- on this tree's library or on the one named by --batch-lib (a build of the commit before
                  the call).  Both check their rows against set membership over the plain texts first.
  take            et_take_packed_device, one call per shape and selection, on this tree's library: a selection of a packed store's
                  records as a new packed store -- the two shapes with every row in order, a random 10 % and a random permutation, and the
                  262 144 key-like records with a random 0.1 % and 10 %.  Beside the writing call it times the sizes-only call and, as
                  the floor, a plain device-to-device copy (torch.Tensor.copy_) of as many bytes in the same process; vs_copy_floor is
                  the call's time over that copy's.  With it runs take_baseline, what the call replaces -- et_decode_packed_gather_device
                  of the rows, then et_encode_packed_device of that text -- on this tree's library or on the one named by --batch-lib (a
                  build of the commit before the call).  Both check their bodies against slices of the store's first.
  search          the match leg's three stores with a 12-byte needle planted at a random position in 0.1 % and in 10 % of the records (and at
                  the end of every second of those): et_search_packed_device under CONTAINS -- with positions, and count only -- and under
                  SUFFIX, its rows and positions checked against the plain texts first.
  search_baseline the first step of anything that searches by decoding, and the only part of it this library has:
                  et_decode_packed_device of the same store -- on this tree's library or on the one named by --batch-lib (a build of the
                  commit before the call).
  order           the match leg's three stores, a tenth of the records copies of record 0: et_match_packed_device(ET_MATCH_LESS) with needles at
                  the 0.1 %, 10 % and 50 % quantiles of the stored texts and, on the two page shapes, a needle that shares 1 KiB with that
                  tenth (the wavefront path) -- with rows, and count only, the rows checked against Python's `<` over the plain texts first --
                  and in the same process ET_MATCH_PREFIX with a 12-byte needle, the floor of a filter that reads one line per record.
  order_baseline  what the call replaces, as far as this library has it: et_decode_packed_device of the whole store -- on this tree's
                  library or on the one named by --batch-lib (a build of the commit before the modes); the comparison in torch that a
                  caller would still have to run behind it is NOT in the figure.
  search_sweep    (only when named) stores of 16 MiB of text in records of 32 .. 4096 bytes, CONTAINS: the times from which
                  SEARCH_LANE_BYTES is chosen -- run it on builds with -DET_SEARCH_LANE_BYTES=0 and =8192 (ET_LIB_PATH names the library)
                  for the two paths at every size.
  slice           et_slice_packed_device (LEFT 12, 64 symbols from the middle, behind a needle up to a stop byte) against what it replaces:
                  a decode (or gather) of the rows' records and et_encode_packed_device of the cut text; the search's walk and the take's
                  copy on the same rows as floors
  field           et_field_packed_device (field k of the pages split at spaces, of 10 % of the rows; fields 0, 3 and 7 of 262 144 CSV lines, of
                  all rows and of 10 %) against what it replaces: a decode (or gather) of the rows' records and et_encode_packed_device of
                  the cut text; the slice up to the delimiter on the same rows and the search's walk over the store as floors
  recode          (only when named) et_recode_packed_device (every row re-tabled, ASCII UPPER of every row under one table, 10 % of the
                  rows re-tabled; the two shapes and the 262 144 CSV lines) against what it replaces, in the same process: a decode (or
                  gather), a torch gather through the map's table, et_encode_packed_device under the other table; the sizes-only call
                  and the slice [0, TO_END) of the same rows as floors
  recode_sweep    (only when named) the search sweep's stores, every row re-tabled: run it on builds with -DET_RECODE_LANE_BYTES=0 and =8192
  group           (only when named) et_group_packed_device (262 144 key-like records drawn from pools of 16, 1 024 and 65 536 values, all
                  different, and 1 024 values with one on 90 % of the records; 4 096 x 4 KiB pages from a pool of 512) with all three
                  outputs and count only, against what it replaces, in the same process: et_decode_packed_device, the texts padded into
                  a matrix with their lengths, torch.unique(dim=0) with inverse and counts; the two partitions and counts compared first
  number          (only when named) et_number_packed_device (field 3 of 262 144 CSV lines read as integers: every line, 10 % of them, the
                  whole column's SUM / COUNT / MIN / MAX, SUM per key for pools of 16 and 65 536 keys; 4 096 x 4 KiB pages with a number
                  behind a 12-byte needle) against what it replaces, in the same process: the field call (or search and slice) of the
                  column as a store, et_decode_packed_device, a torch parse of the padded matrix, scatter_add_; values and aggregates
                  checked against Python's first; the slice call on the same ask and the field call as floors
--legs picks the legs (default: all but the sweeps, concat, recode, group and number).
Timing: HIP events on the stream round the whole sequence of calls (all encodes; all decodes), WARMUP untimed repetitions, then
REPS timed ones; the median is the figure, min and max the run-to-run spread.  Every leg checks its decoded bytes against the
text once before timing.  One JSON line on stdout (and into --out).

    python tools/batch_bench.py --parent-lib /path/to/parent/libentreepy_hip.so --out profiles/batch_bench.json
    python tools/batch_bench.py --legs batch,shared --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/shared_bench.json
    python tools/batch_bench.py --legs packed --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/packed_bench.json
    python tools/batch_bench.py --legs gather --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/gather_bench.json
    python tools/batch_bench.py --legs match --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/match_bench.json
    python tools/batch_bench.py --legs join --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/join_bench.json
    python tools/batch_bench.py --legs take --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/take_bench.json
    python tools/batch_bench.py --legs search --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/search_bench.json
    python tools/batch_bench.py --legs order --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/order_bench.json
    python tools/batch_bench.py --legs slice --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/slice_bench.json
    python tools/batch_bench.py --legs field --batch-lib /path/to/parent/libentreepy_hip.so --out profiles/field_bench.json
    python tools/batch_bench.py --legs concat --out profiles/concat_bench.json
    python tools/batch_bench.py --legs recode --out profiles/recode_bench.json
    python tools/batch_bench.py --legs group --out profiles/group_bench.json
    python tools/batch_bench.py --legs number --out profiles/number_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 64 * 1024), (4096, 4 * 1024)]
REPS, WARMUP = 20, 3
TABLE = ["et_build_codebook", "et_body_bound", "et_codebook_is_complete"]
STORE = TABLE + ["et_encode_packed_device"]


def _open(lib_path, names):
    """-> (L, h, the device): the library at lib_path with the named entry points (and the context's own) declared, and a context on
    torch's current stream."""
    import torch

    from entreepy_amd import _native as N

    names = ["et_ctx_create", "et_ctx_destroy", "et_ctx_set_stream", "et_last_error"] + names
    L = N.declare(ctypes.CDLL(lib_path, mode=ctypes.RTLD_GLOBAL), names)  # (torch is imported: the process-wide HIP runtime is loaded)
    h = ctypes.c_void_p()
    assert L.et_ctx_create(0, ctypes.byref(h)) == 0
    assert L.et_ctx_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)) == 0
    return L, h, torch.device("cuda", 0)


def _timed(fn):
    """WARMUP untimed calls, then REPS between HIP events on the stream: the median, and the spread."""
    import torch

    ms = []
    for rep in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if rep >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _codebook(L, text):
    """-> the complete table built from the histogram of `text` (a tensor on the device, or numpy arrays on the host)"""
    import numpy as np
    import torch

    from entreepy_amd import _native as N

    if isinstance(text, torch.Tensor):
        hist = torch.bincount(text.to(torch.int32), minlength=256).cpu().numpy().astype(np.uint64)
    else:
        hist = sum(np.bincount(t, minlength=256) for t in text).astype(np.uint64)
    cb = N.Codebook()
    assert L.et_build_codebook(hist.ctypes.data, ctypes.byref(cb)) == 0 and L.et_codebook_is_complete(ctypes.byref(cb)) == 0
    return cb


def _packed_store(L, h, text, index, cb=None):
    """-> (cb, bodies, body bytes, body_index, text_index), the tensors on the device: the records text[index[j] : index[j + 1]] (text a
    tensor on the device, index numpy u64) as a packed store (et_encode_packed_device) under cb, or under a table from the text's histogram."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N

    if cb is None:
        cb = _codebook(L, text)
    n, total = index.size - 1, int(index[-1])
    cap = L.et_body_bound(ctypes.byref(cb), total) + n
    bodies = torch.zeros(cap + 64, dtype=torch.uint8, device=text.device)
    text_index = torch.from_numpy(index.view(np.int64)).to(text.device)
    body_index = torch.zeros(n + 1, dtype=torch.int64, device=text.device)
    res = N.PackedResult()
    assert L.et_encode_packed_device(h, ctypes.byref(cb), text.data_ptr(), total, text_index.data_ptr(), n, bodies.data_ptr(), cap, body_index.data_ptr(), None,
                                     ctypes.byref(res)) == 0 and res.n_failed == 0, L.et_last_error(h)
    torch.cuda.synchronize()
    return cb, bodies, int(res.out_bytes), body_index, text_index


def _leg(leg, lib_path):
    import numpy as np
    import torch

    from entreepy_amd import _native as N
    from tests import corpus

    names = ["et_encode_bound", "et_encode_device", "et_decode_device"]
    if leg == "batch":
        names += ["et_encode_batch_device", "et_decode_batch_device"]
    if leg == "packed":
        names += ["et_encode_packed_device", "et_decode_packed_device"]
    if leg in ("shared", "packed", "dense"):
        names += ["et_encode_shared_device", "et_decode_shared_device", "et_write_header"] + TABLE
    L, h, dev = _open(lib_path, names)
    results = {}
    for count, size in SHAPES:
        text = corpus.text_like_torch(count * size, 0xB47C4 + size, dev)
        bound = L.et_encode_bound(size)
        if leg in ("shared", "packed", "dense"):  # one table for the whole shape, from the histogram of all of its text
            cb = _codebook(L, text)
            bound = (L.et_body_bound(ctypes.byref(cb), size) + 15) // 16 * 16
            head, head_len = np.zeros(8192, np.uint8), ctypes.c_size_t(0)
            assert L.et_write_header(ctypes.byref(cb), count * size, head.ctypes.data, head.size, ctypes.byref(head_len)) == 0
        enc = torch.zeros(count * bound + 64, dtype=torch.uint8, device=dev)
        dec = torch.zeros(count * (size + 16) + 64, dtype=torch.uint8, device=dev)
        enc_len = np.zeros(count, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        item = np.dtype([(name, {ctypes.c_uint64: "<u8", ctypes.c_int32: "<i4", ctypes.c_uint32: "<u4"}[t]) for name, t in N.BatchItem._fields_])
        idx = np.arange(count, dtype=np.uint64)
        items_e, items_d = np.zeros(count, dtype=item), np.zeros(count, dtype=item)
        items_e["in_off"], items_e["in_len"], items_e["out_off"], items_e["out_cap"] = idx * size, size, idx * bound, bound
        items_d["in_off"], items_d["out_off"], items_d["out_cap"] = idx * bound + 4, idx * (size + 16), size + 16

        if leg == "shared":  # (bodies: nothing to skip in front of them, and out_cap is the record's length)
            items_d["in_off"], items_d["out_cap"] = idx * bound, size
        if leg == "dense":  # (text and symbols dense; where the bodies lie comes out of encode_all's prefix sum)
            items_d["out_off"], items_d["out_cap"] = idx * size, size
        if leg == "packed":
            text_index = torch.arange(count + 1, dtype=torch.int64, device=dev) * size
            out_index = torch.zeros(count + 1, dtype=torch.int64, device=dev)
            res = N.PackedResult()

        def encode_all():
            if leg == "packed":
                assert L.et_encode_packed_device(h, ctypes.byref(cb), text.data_ptr(), count * size, text_index.data_ptr(), count, enc.data_ptr(), count * bound,
                                                 out_index.data_ptr(), None, ctypes.byref(res)) == 0, L.et_last_error(h)
                assert res.n_failed == 0
                enc_len[0] = res.out_bytes
            elif leg == "dense":  # sizes only, the prefix sum, the writing call
                assert L.et_encode_shared_device(h, ctypes.byref(cb), text.data_ptr(), None, items_e.ctypes.data, count) == 0, L.et_last_error(h)
                items_e["out_cap"] = items_e["out_len"]
                items_e["out_off"][1:] = np.cumsum(items_e["out_len"][:-1])
                assert L.et_encode_shared_device(h, ctypes.byref(cb), text.data_ptr(), enc.data_ptr(), items_e.ctypes.data, count) == 0, L.et_last_error(h)
                enc_len[:] = items_e["out_len"]
            elif leg == "shared":
                assert L.et_encode_shared_device(h, ctypes.byref(cb), text.data_ptr(), enc.data_ptr(), items_e.ctypes.data, count) == 0, L.et_last_error(h)
                enc_len[:] = items_e["out_len"]
            elif leg == "batch":
                assert L.et_encode_batch_device(h, text.data_ptr(), enc.data_ptr(), items_e.ctypes.data, count) == 0, L.et_last_error(h)
                enc_len[:] = items_e["out_len"]
            else:
                for i in range(count):
                    assert L.et_encode_device(h, text.data_ptr() + i * size, size, enc.data_ptr() + i * bound, bound, ctypes.byref(n)) == 0, L.et_last_error(h)
                    enc_len[i] = n.value

        def decode_all():
            if leg == "packed":
                assert L.et_decode_packed_device(h, ctypes.byref(cb), enc.data_ptr(), count * bound, out_index.data_ptr(), text_index.data_ptr(), count, dec.data_ptr(),
                                                 count * size, None, None, ctypes.byref(res)) == 0, L.et_last_error(h)
                assert res.n_failed == 0 and res.n_short == 0
            elif leg == "dense":
                items_d["in_off"], items_d["in_len"] = items_e["out_off"], enc_len
                assert L.et_decode_shared_device(h, ctypes.byref(cb), enc.data_ptr(), dec.data_ptr(), items_d.ctypes.data, count) == 0, L.et_last_error(h)
                assert not items_d["status"].any() and (items_d["out_len"] == size).all()
            elif leg == "shared":
                items_d["in_len"] = enc_len
                assert L.et_decode_shared_device(h, ctypes.byref(cb), enc.data_ptr(), dec.data_ptr(), items_d.ctypes.data, count) == 0, L.et_last_error(h)
                assert not items_d["status"].any() and (items_d["out_len"] == size).all()
            elif leg == "batch":
                items_d["in_len"] = enc_len - np.uint64(4)
                assert L.et_decode_batch_device(h, enc.data_ptr(), dec.data_ptr(), items_d.ctypes.data, count) == 0, L.et_last_error(h)
                assert not items_d["status"].any() and (items_d["out_len"] == size).all()
            else:
                for i in range(count):
                    assert L.et_decode_device(h, enc.data_ptr() + i * bound + 4, int(enc_len[i]) - 4, dec.data_ptr() + i * (size + 16), size + 16, ctypes.byref(n)) == 0, L.et_last_error(h)

        encode_all()
        decode_all()
        torch.cuda.synchronize()
        if leg in ("packed", "dense"):
            assert torch.equal(dec[: count * size], text), "decoded bytes differ from the text"
        else:
            assert torch.equal(dec[: count * (size + 16)].view(count, size + 16)[:, :size].reshape(-1), text), "decoded bytes differ from the text"
        if leg in ("batch", "shared", "dense"):
            assert not items_e["status"].any() and not items_e["path"].any() and not items_d["path"].any()
        sizes = {"image_bytes": int(enc_len.sum())} if leg in ("single", "batch") else {"body_bytes": int(enc_len.sum()), "header_bytes": int(head_len.value)}
        enc_ms, dec_ms = [], []
        for rep in range(WARMUP + REPS):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            encode_all()
            e1.record()
            decode_all()
            e2.record()
            e2.synchronize()
            if rep >= WARMUP:
                enc_ms.append(e0.elapsed_time(e1))
                dec_ms.append(e1.elapsed_time(e2))
        both = [a + b for a, b in zip(enc_ms, dec_ms)]
        results[f"{count}x{size}"] = {
            "encode_ms": round(statistics.median(enc_ms), 4), "decode_ms": round(statistics.median(dec_ms), 4),
            "encode_min_ms": round(min(enc_ms), 4), "encode_max_ms": round(max(enc_ms), 4), "decode_min_ms": round(min(dec_ms), 4), "decode_max_ms": round(max(dec_ms), 4),
            "roundtrip_ms": round(statistics.median(both), 4), "roundtrip_min_ms": round(min(both), 4), "roundtrip_max_ms": round(max(both), 4),
            "text_gb_per_s": round(2 * count * size / statistics.median(both) / 1e6, 2), **sizes,
        }
        del text, enc, dec
    L.et_ctx_destroy(h)
    print(json.dumps(results))


SELECTIONS = ("identity", "random_tenth", "permutation")


def _selection(name, count):
    import numpy as np

    rng = np.random.default_rng(0x6A7E4 + count)
    if name == "identity":
        return np.arange(count, dtype=np.uint32)
    if name == "random_tenth":
        return np.sort(rng.choice(count, size=count // 10, replace=False)).astype(np.uint32)
    return rng.permutation(count).astype(np.uint32)


def _gather_leg(leg, lib_path):
    """gather / gather_baseline: per shape a packed store (et_encode_packed_device, untimed), then per selection the timed decode."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N
    from tests import corpus

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device", "et_decode_shared_device"] + (["et_decode_packed_gather_device"] if leg == "gather" else []))
    item = np.dtype([(name, {ctypes.c_uint64: "<u8", ctypes.c_int32: "<i4", ctypes.c_uint32: "<u4"}[t]) for name, t in N.BatchItem._fields_])
    results = {}
    for count, size in SHAPES:
        text = corpus.text_like_torch(count * size, 0xB47C4 + size, dev)
        cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, text, np.arange(count + 1, dtype=np.uint64) * np.uint64(size))
        res = N.PackedResult()
        shape = {"body_bytes": body_bytes}
        for name in SELECTIONS:
            rows = _selection(name, count)
            d_rows = torch.from_numpy(rows.view(np.int32)).to(dev)
            need = rows.size * size
            dec = torch.zeros(need + 64, dtype=torch.uint8, device=dev)
            out_index = torch.zeros(rows.size + 1, dtype=torch.int64, device=dev)
            want = text.view(count, size)[d_rows.long()].reshape(-1)

            def gather(d_out=dec):
                assert L.et_decode_packed_gather_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, d_rows.data_ptr(),
                                                        rows.size, None if d_out is None else d_out.data_ptr(), need, out_index.data_ptr(), None, None, ctypes.byref(res)) == 0, L.et_last_error(h)
                assert res.out_bytes == need and res.n_failed == 0 and res.n_short == 0

            def baseline():
                bi, ti = (t.cpu().numpy().view(np.uint64) for t in (body_index, text_index))  # both offset arrays, to the host
                at = rows.astype(np.int64)
                items = np.zeros(rows.size, dtype=item)
                items["in_off"], items["in_len"], items["out_cap"] = bi[at], bi[at + 1] - bi[at], ti[at + 1] - ti[at]
                items["out_off"][1:] = np.cumsum(items["out_cap"][:-1])
                assert L.et_decode_shared_device(h, ctypes.byref(cb), bodies.data_ptr(), dec.data_ptr(), items.ctypes.data, rows.size) == 0, L.et_last_error(h)
                assert not items["status"].any() and (items["out_len"] == items["out_cap"]).all()

            def packed():
                assert L.et_decode_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, dec.data_ptr(), need, None, None,
                                                 ctypes.byref(res)) == 0, L.et_last_error(h)
                assert res.n_failed == 0 and res.n_short == 0

            run = gather if leg == "gather" else baseline
            run()
            torch.cuda.synchronize()
            assert torch.equal(dec[:need], want), "decoded rows differ from the text"
            shape[name] = {"rows": int(rows.size), **_timed(run)}
            if leg == "gather":
                shape[name]["sizes_only"] = _timed(lambda: gather(None))
                if name == "identity":
                    shape[name]["packed_decode"] = _timed(packed)
            del dec, want
        results[f"{count}x{size}"] = shape
        del text, bodies
    L.et_ctx_destroy(h)
    print(json.dumps(results))


KEY_SHAPE = (262144, (16, 48))  # the match legs' third shape: key-like records of 16 .. 48 bytes
SELECTIVITIES = (("0.1%", 0.001), ("10%", 0.1), ("100%", 1.0))
MATCH_PREFIX_LEN = 12


def _match_store(count, size, fraction, dev):
    """-> (text on the device, text_index as numpy u64, the chosen records ascending, record 0's text): `fraction` of the records, record
    0 among them, are copies of record 0; the others are text-like and as long as `size` says (a number, or a range)."""
    import numpy as np
    import torch

    from tests import corpus

    rng = np.random.default_rng(0x3A7C4 + count + int(fraction * 1000))
    chosen = np.arange(count) if fraction >= 1.0 else np.union1d([0], rng.choice(count, size=max(int(count * fraction), 1), replace=False))
    if isinstance(size, int):
        text = corpus.text_like_torch(count * size, 0xB47C4 + size, dev)
        rec = text.view(count, size)
        rec[torch.from_numpy(chosen).to(dev)] = rec[0].clone()
        return text, np.arange(count + 1, dtype=np.uint64) * np.uint64(size), chosen, rec[0].cpu().numpy().tobytes()
    lengths = rng.integers(size[0], size[1] + 1, size=count)
    lengths[chosen] = lengths[0]
    index = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    host = corpus.text_like(int(index[-1]), 0xB47C4 + count).copy()
    key = host[: lengths[0]].copy()
    at = (index[chosen].astype(np.int64)[:, None] + np.arange(lengths[0])[None, :]).reshape(-1)
    host[at] = np.tile(key, chosen.size)
    return torch.from_numpy(host).to(dev), index, chosen, key.tobytes()


def _match_leg(leg, lib_path, shapes):
    """match / match_baseline: per shape and selectivity a packed store (et_encode_packed_device, untimed), then the timed filter: the
    call under PREFIX and EQUAL (and count only) -- or what it replaces: et_decode_packed_device of the whole store, then the first L
    bytes of every record gathered, compared, the lengths tested and nonzero, in torch on the device."""
    import torch

    from entreepy_amd import _native as N

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device"] + (["et_match_packed_device"] if leg == "match" else []))
    results = {}
    for count, size in SHAPES + [KEY_SHAPE]:
        shape_name = f"{count}x{size}" if isinstance(size, int) else f"{count}x{size[0]}-{size[1]}"
        if shapes and shape_name not in shapes:
            continue
        shape = {}
        for sel_name, fraction in SELECTIVITIES:
            text, index, chosen, key = _match_store(count, size, fraction, dev)
            cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, text, index)
            total = int(index[-1])
            res = N.PackedResult()
            lengths = text_index[1:] - text_index[:-1]

            def torch_filter(buf, needle, equal):  # the first len(needle) bytes of every record gathered and compared, the lengths tested, nonzero
                d_needle = torch.frombuffer(bytearray(needle), dtype=torch.uint8).to(dev)
                at = (text_index[:-1].unsqueeze(1) + torch.arange(len(needle), device=dev).unsqueeze(0)).clamp_(max=total - 1)
                same = (buf[at] == d_needle.unsqueeze(0)).all(dim=1) & ((lengths == len(needle)) if equal else (lengths >= len(needle)))
                return same.nonzero().squeeze(1)

            needles = {"prefix": (key[:MATCH_PREFIX_LEN], N.ET_MATCH_PREFIX), "equal": (key[:4096], N.ET_MATCH_EQUAL)}
            needles = {name: (needle, mode, torch_filter(text, needle, name == "equal")) for name, (needle, mode) in needles.items()}
            assert needles["prefix"][2].numel() >= chosen.size and needles["equal"][2].numel() == (chosen.size if len(key) <= 4096 else 0)
            entry = {"records": count, "chosen": int(chosen.size), "text_bytes": total, "body_bytes": body_bytes}
            if leg == "match":
                d_rows = torch.zeros(count, dtype=torch.int32, device=dev)
                mres = N.MatchResult()

                def call(needle, mode, rows=d_rows):
                    assert L.et_match_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, needle, len(needle), mode,
                                                    None if rows is None else rows.data_ptr(), count, None, ctypes.byref(mres)) == 0, L.et_last_error(h)
                    assert mres.n_failed == 0

                for name, (needle, mode, want) in needles.items():
                    call(needle, mode)
                    torch.cuda.synchronize()
                    assert mres.n_match == want.numel() and torch.equal(d_rows[: mres.n_match].long(), want), "the rows differ from the records chosen"
                    entry[name] = {"needle_bytes": len(needle), "rows": int(mres.n_match), **_timed(lambda: call(needle, mode))}
                    entry[name]["count_only"] = _timed(lambda: call(needle, mode, None))
            else:
                dec = torch.zeros(total + 64, dtype=torch.uint8, device=dev)

                def baseline(needle, equal):
                    assert L.et_decode_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, dec.data_ptr(), total, None,
                                                     None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    assert res.n_failed == 0 and res.n_short == 0
                    return torch_filter(dec, needle, equal)

                for name, (needle, mode, want) in needles.items():
                    assert torch.equal(baseline(needle, name == "equal"), want), "the rows differ from the records chosen"
                    entry[name] = {"needle_bytes": len(needle), "rows": int(want.numel()), **_timed(lambda: baseline(needle, name == "equal"))}
                del dec
            shape[sel_name] = entry
            del text, bodies
        results[shape_name] = shape
    L.et_ctx_destroy(h)
    print(json.dumps(results))


ORDER_QUANTILES = (("0.1%", 0.001), ("10%", 0.1), ("50%", 0.5))
ORDER_SHARED_PREFIX = 1024  # bytes the wavefront-path needle shares with a tenth of the records


def _order_leg(leg, lib_path, shapes):
    """order / order_baseline: per shape a packed store with a tenth of its records copies of record 0 (et_encode_packed_device, untimed),
    then the timed filter: ET_MATCH_LESS with needles at three quantiles of the stored texts and one that shares 1 KiB with that tenth,
    with rows and count only, and ET_MATCH_PREFIX with a 12-byte needle beside it -- or what the call replaces: et_decode_packed_device
    of the whole store (the comparison behind it is left out)."""
    import torch

    from entreepy_amd import _native as N

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device"] + (["et_match_packed_device"] if leg == "order" else []))
    results = {}
    for count, size in SHAPES + [KEY_SHAPE]:
        shape_name = f"{count}x{size}" if isinstance(size, int) else f"{count}x{size[0]}-{size[1]}"
        if shapes and shape_name not in shapes:
            continue
        text, index, chosen, key = _match_store(count, size, 0.1, dev)
        cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, text, index)
        total = int(index[-1])
        entry = {"records": count, "sharing": int(chosen.size), "text_bytes": total, "body_bytes": body_bytes}
        if leg == "order":
            host = text.cpu().numpy()
            texts = [host[int(index[j]) : int(index[j + 1])].tobytes() for j in range(count)]
            ranked = sorted(texts)
            needles = {name: ranked[int(q * count)][:4096] for name, q in ORDER_QUANTILES}  # (et_match_pattern_max())
            if len(key) > ORDER_SHARED_PREFIX:
                needles["shares_1KiB"] = key[:ORDER_SHARED_PREFIX] + bytes([key[ORDER_SHARED_PREFIX] ^ 1])
            d_rows = torch.zeros(count, dtype=torch.int32, device=dev)
            mres = N.MatchResult()

            def call(needle, mode, rows=d_rows):
                assert L.et_match_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, needle, len(needle), mode,
                                                None if rows is None else rows.data_ptr(), count, None, ctypes.byref(mres)) == 0, L.et_last_error(h)
                assert mres.n_failed == 0

            for name, needle in needles.items():
                want = [j for j, t in enumerate(texts) if t < needle]
                call(needle, N.ET_MATCH_LESS)
                torch.cuda.synchronize()
                assert mres.n_match == len(want) and d_rows[: mres.n_match].tolist() == want, "the rows differ from Python's `<` over the plain texts"
                entry[name] = {"needle_bytes": len(needle), "rows": len(want), **_timed(lambda: call(needle, N.ET_MATCH_LESS))}
                entry[name]["count_only"] = _timed(lambda: call(needle, N.ET_MATCH_LESS, None))
            floor = key[:MATCH_PREFIX_LEN]
            call(floor, N.ET_MATCH_PREFIX)
            torch.cuda.synchronize()
            assert mres.n_match == sum(t.startswith(floor) for t in texts)
            entry["prefix_floor"] = {"needle_bytes": len(floor), "rows": int(mres.n_match), **_timed(lambda: call(floor, N.ET_MATCH_PREFIX))}
            del host, texts, ranked
        else:
            dec = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
            res = N.PackedResult()

            def decode():
                assert L.et_decode_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, dec.data_ptr(), total, None,
                                                 None, ctypes.byref(res)) == 0, L.et_last_error(h)
                assert res.n_failed == 0 and res.n_short == 0

            decode()
            torch.cuda.synchronize()
            assert torch.equal(dec[:total], text[:total]), "the decoded store differs from the text"
            entry["decode"] = {"comparison_included": False, **_timed(decode)}
            del dec
        results[shape_name] = entry
        del text, bodies
    L.et_ctx_destroy(h)
    print(json.dumps(results))


SEARCH_NEEDLE_LEN = 12
SEARCH_SELECTIVITIES = (("0.1%", 0.001), ("10%", 0.1))
SWEEP_SIZES = (32, 64, 96, 128, 192, 256, 384, 512, 1024, 4096)  # bytes of text per record of the sweep's stores ...
SWEEP_BYTES = 16 << 20                                            # ... of this much text each


def _search_store(count, size, fraction):
    """-> (text, text_index, needle, (rows that contain it, where, rows that end with it)): `count` text-like records, as long as
    `size` says (a number, or a range); a 12-byte needle planted at a random position in `fraction` of them, and at the end of every
    second of those as well.  The expected rows are Python's find and endswith over the plain texts."""
    import numpy as np

    from tests import corpus

    rng = np.random.default_rng(0x5EA2C4 + count + int(fraction * 1000))
    lengths = np.full(count, size) if isinstance(size, int) else rng.integers(size[0], size[1] + 1, size=count)
    index = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    host = corpus.text_like(int(index[-1]), 0xB47C4 + count).copy()
    needle = corpus.text_like(4096, 0x5EA2C4)[-SEARCH_NEEDLE_LEN:].copy()
    for j, b in enumerate(rng.choice(count, size=max(int(count * fraction), 1), replace=False)):
        at = int(index[b]) + int(rng.integers(0, int(lengths[b]) - SEARCH_NEEDLE_LEN + 1))
        host[at : at + SEARCH_NEEDLE_LEN] = needle
        if j % 2:
            host[int(index[b + 1]) - SEARCH_NEEDLE_LEN : int(index[b + 1])] = needle
    blob, nd = host.tobytes(), needle.tobytes()
    rows, pos, ends = [], [], []
    for b in range(count):
        t = blob[int(index[b]) : int(index[b + 1])]
        p = t.find(nd)
        if p >= 0:
            rows.append(b)
            pos.append(p)
            if t.endswith(nd):
                ends.append(b)
    return host, index, nd, (rows, pos, ends)


def _search_leg(leg, lib_path, shapes):
    """search / search_baseline / search_sweep: per shape and selectivity a packed store (et_encode_packed_device, untimed), then the
    timed call: et_search_packed_device under CONTAINS (with positions, and count only) and SUFFIX, its rows and positions checked
    against the plain texts first -- or the first step of anything that searches by decoding: et_decode_packed_device of the whole
    store.  search_sweep: stores of SWEEP_BYTES of text in records of one size each, 10 % of them with the needle, under CONTAINS;
    which path a size takes is the library's et_search_lane_bytes(), reported beside the times."""
    import torch

    from entreepy_amd import _native as N

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device"] + ([] if leg == "search_baseline" else ["et_search_packed_device", "et_search_lane_bytes"]))
    sweep = leg == "search_sweep"
    results = {"lane_bytes": int(L.et_search_lane_bytes())} if sweep else {}
    for count, size in [(SWEEP_BYTES // s, s) for s in SWEEP_SIZES] if sweep else SHAPES + [KEY_SHAPE]:
        shape_name = f"{count}x{size}" if isinstance(size, int) else f"{count}x{size[0]}-{size[1]}"
        if shapes and shape_name not in shapes:
            continue
        shape = {}
        for sel_name, fraction in SEARCH_SELECTIVITIES[1:] if sweep else SEARCH_SELECTIVITIES:
            host, index, needle, (rows, pos, ends) = _search_store(count, size, fraction)
            text = torch.from_numpy(host).to(dev)
            cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, text, index, _codebook(L, [host]))
            total = int(index[-1])
            res = N.PackedResult()
            entry = {"records": count, "text_bytes": total, "body_bytes": body_bytes, "needle_bytes": len(needle), "contain": len(rows), "end_with": len(ends)}
            if leg == "search_baseline":
                dec = torch.zeros(total + 64, dtype=torch.uint8, device=dev)

                def decode():
                    assert L.et_decode_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, dec.data_ptr(), total, None,
                                                     None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    assert res.n_failed == 0 and res.n_short == 0

                decode()
                torch.cuda.synchronize()
                assert torch.equal(dec[:total], text), "decoded bytes differ from the text"
                entry["decode"] = _timed(decode)
                del dec
            else:
                d_rows, d_pos = torch.zeros(count, dtype=torch.int32, device=dev), torch.zeros(count, dtype=torch.int32, device=dev)
                mres = N.MatchResult()

                def call(mode, rows_t=d_rows, pos_t=d_pos):
                    assert L.et_search_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, needle, len(needle), mode,
                                                     None if rows_t is None else rows_t.data_ptr(), count, None if pos_t is None else pos_t.data_ptr(), None, ctypes.byref(mres)) == 0, L.et_last_error(h)
                    assert mres.n_failed == 0

                for name, mode, want in (("contains", N.ET_SEARCH_CONTAINS, rows), ("suffix", N.ET_SEARCH_SUFFIX, ends)):
                    call(mode)
                    torch.cuda.synchronize()
                    assert mres.n_match == len(want) and d_rows[: mres.n_match].tolist() == want, "the rows differ from the plain texts'"
                    if name == "contains":
                        assert d_pos[: mres.n_match].tolist() == pos, "the positions differ from the plain texts'"
                    if sweep and name == "suffix":
                        continue
                    entry[name] = {"rows": int(mres.n_match), **_timed(lambda: call(mode))}
                entry["contains"]["count_only"] = _timed(lambda: call(N.ET_SEARCH_CONTAINS, None, None))
            shape[sel_name] = entry
            del text, bodies
        results[shape_name] = shape
    L.et_ctx_destroy(h)
    print(json.dumps(results))


JOIN_KEYS = (16, 1024, 65536)
JOIN_SELECTIVITIES = (("0.1%", 0.001), ("10%", 0.1))


def _join_store(count, size, n_keys, fraction):
    """-> (text, text_index, key text, key text_index) as numpy arrays: `count` text-like records of size[0] .. size[1] bytes, `fraction` of
    them copies of one of n_keys text-like keys (the chosen records take the keys in turn; keys beyond their number equal no record)."""
    import numpy as np

    from tests import corpus

    rng = np.random.default_rng(0x10A5E + count + n_keys + int(fraction * 1000))
    key_lengths = rng.integers(size[0], size[1] + 1, size=n_keys)
    key_index = np.concatenate(([0], np.cumsum(key_lengths))).astype(np.uint64)
    key_text = corpus.text_like(int(key_index[-1]), 0x10A5E + n_keys).copy()
    chosen = np.sort(rng.choice(count, size=max(int(count * fraction), 1), replace=False))
    which = np.arange(chosen.size) % n_keys
    lengths = rng.integers(size[0], size[1] + 1, size=count)
    lengths[chosen] = key_lengths[which]
    index = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    text = corpus.text_like(int(index[-1]), 0xB47C4 + count).copy()
    for r, k in zip(chosen, which):
        text[int(index[r]) : int(index[r + 1])] = key_text[int(key_index[k]) : int(key_index[k + 1])]
    return text, index, key_text, key_index


def _join_leg(leg, lib_path):
    """join / join_baseline: per key set and selectivity two packed stores (et_encode_packed_device, untimed), then the timed join: the
    call with d_rows and d_key_of_row (and count only) -- or what it replaces: one et_match_packed_device(ET_MATCH_EQUAL) per key, then
    the union of their rows sorted in torch."""
    import torch

    from entreepy_amd import _native as N

    L, h, dev = _open(lib_path, STORE + ["et_match_packed_device"] + (["et_join_packed_device"] if leg == "join" else []))
    count, size = KEY_SHAPE
    shape = {}
    for n_keys in JOIN_KEYS:
        per_keys = {}
        for sel_name, fraction in JOIN_SELECTIVITIES:
            text, index, key_text, key_index = _join_store(count, size, n_keys, fraction)
            cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, torch.from_numpy(text).to(dev), index, _codebook(L, [text, key_text]))  # (one table for both stores)
            # the expected rows: set membership over the plain texts; the key of a row: the first index of its text among the keys
            blob, key_blob = text.tobytes(), key_text.tobytes()
            keys = [key_blob[int(a) : int(b)] for a, b in zip(key_index[:-1], key_index[1:])]
            first = {}
            for k, t in enumerate(keys):
                first.setdefault(t, k)
            found = [(r, first.get(blob[int(a) : int(b)])) for r, (a, b) in enumerate(zip(index[:-1], index[1:]))]
            want_rows = [r for r, k in found if k is not None]
            want_keys = [k for r, k in found if k is not None]
            entry = {"records": count, "keys": n_keys, "rows": len(want_rows), "body_bytes": body_bytes}
            d_rows = torch.zeros(count, dtype=torch.int32, device=dev)
            if leg == "join":
                _, key_bodies, key_body_bytes, key_body_index, key_text_index = _packed_store(L, h, torch.from_numpy(key_text).to(dev), key_index, cb)
                d_key_of_row = torch.zeros(count, dtype=torch.int32, device=dev)
                jres = N.JoinResult()

                def call(rows=d_rows):
                    assert L.et_join_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, key_bodies.data_ptr(),
                                                   key_body_bytes, key_body_index.data_ptr(), key_text_index.data_ptr(), n_keys, 0, None if rows is None else rows.data_ptr(), count,
                                                   None if rows is None else d_key_of_row.data_ptr(), None, None, ctypes.byref(jres)) == 0, L.et_last_error(h)
                    assert jres.n_failed == 0 and jres.n_keys_failed == 0

                call()
                torch.cuda.synchronize()
                assert jres.n_match == len(want_rows) and d_rows[: jres.n_match].tolist() == want_rows, "the rows differ from set membership over the texts"
                assert d_key_of_row[: jres.n_match].tolist() == want_keys, "a key number is not the first index of the row's text"
                entry.update(_timed(call))
                entry["count_only"] = _timed(lambda: call(None))
            else:
                mres = N.MatchResult()

                def baseline():
                    at = 0
                    for t in keys:
                        assert L.et_match_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, t, len(t),
                                                        N.ET_MATCH_EQUAL, d_rows.data_ptr() + 4 * at, count - at, None, ctypes.byref(mres)) == 0, L.et_last_error(h)
                        at += mres.n_match
                    return torch.sort(d_rows[:at])[0]

                got = baseline()
                torch.cuda.synchronize()
                assert got.tolist() == want_rows, "the rows differ from set membership over the texts"
                entry.update(_timed(baseline))
            per_keys[sel_name] = entry
            del bodies
        shape[f"{n_keys}_keys"] = per_keys
    L.et_ctx_destroy(h)
    print(json.dumps({f"{count}x{size[0]}-{size[1]}": shape}))


def _take_leg(leg, lib_path):
    """take / take_baseline: per shape a packed store (et_encode_packed_device, untimed), then per selection the timed call: the take
    with d_out -- beside it the sizes-only call and a plain device-to-device copy of as many bytes (torch.Tensor.copy_, the floor) -- or
    what it replaces: et_decode_packed_gather_device of the rows, then et_encode_packed_device of that text."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N
    from tests import corpus

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_gather_device"] + (["et_take_packed_device"] if leg == "take" else []))
    rng = np.random.default_rng(0x7A4E5)
    count, size = KEY_SHAPE
    key_lengths = rng.integers(size[0], size[1] + 1, size=count)
    stores = [(f"{c}x{s}", c, np.arange(c + 1, dtype=np.uint64) * np.uint64(s), SELECTIONS) for c, s in SHAPES]
    stores.append((f"{count}x{size[0]}-{size[1]}", count, np.concatenate(([0], np.cumsum(key_lengths))).astype(np.uint64), ("random_0.1%", "random_tenth")))
    results = {}
    for shape_name, count, index, selections in stores:
        total = int(index[-1])
        text = corpus.text_like_torch(total, 0xB47C4 + count, dev)
        cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, text, index)
        res = N.PackedResult()
        host_bodies, bi = bodies[:body_bytes].cpu().numpy(), body_index.cpu().numpy().view(np.uint64)
        shape = {"body_bytes": body_bytes}
        for name in selections:
            rows = np.sort(rng.choice(count, size=max(count // 1000, 1), replace=False)).astype(np.uint32) if name == "random_0.1%" else _selection(name, count)
            d_rows = torch.from_numpy(rows.view(np.int32)).to(dev)
            at = rows.astype(np.int64)
            need, text_need = int((bi[at + 1] - bi[at]).sum()), int((index[at + 1] - index[at]).sum())
            want = np.concatenate([host_bodies[int(bi[r]) : int(bi[r + 1])] for r in at])
            out = torch.zeros(need + 64, dtype=torch.uint8, device=dev)
            out_body_index = torch.zeros(rows.size + 1, dtype=torch.int64, device=dev)
            out_text_index = torch.zeros(rows.size + 1, dtype=torch.int64, device=dev)
            entry = {"rows": int(rows.size), "bytes": need}
            if leg == "take":
                tres = N.TakeResult()

                def take(d_out=out):
                    assert L.et_take_packed_device(h, bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, d_rows.data_ptr(), rows.size,
                                                   None if d_out is None else d_out.data_ptr(), need, out_body_index.data_ptr(), out_text_index.data_ptr(), None,
                                                   ctypes.byref(tres)) == 0, L.et_last_error(h)
                    assert tres.out_bytes == need and tres.text_bytes == text_need and tres.n_failed == 0

                take()
                torch.cuda.synchronize()
                assert np.array_equal(out[:need].cpu().numpy(), want), "the taken bodies differ from the store's"
                assert np.array_equal(np.diff(out_body_index.cpu().numpy()), (bi[at + 1] - bi[at]).astype(np.int64)) and int(out_text_index[-1]) == text_need
                entry.update(_timed(take))
                entry["sizes_only"] = _timed(lambda: take(None))
                src = bodies[:need] if need <= body_bytes else torch.zeros(need, dtype=torch.uint8, device=dev)
                entry["copy_floor"] = _timed(lambda: out[:need].copy_(src))
                entry["vs_copy_floor"] = round(entry["ms"] / entry["copy_floor"]["ms"], 2)
            else:
                dec = torch.zeros(text_need + 64, dtype=torch.uint8, device=dev)

                def baseline():
                    assert L.et_decode_packed_gather_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, d_rows.data_ptr(),
                                                            rows.size, dec.data_ptr(), text_need, out_text_index.data_ptr(), None, None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    assert res.out_bytes == text_need and res.n_failed == 0 and res.n_short == 0
                    assert L.et_encode_packed_device(h, ctypes.byref(cb), dec.data_ptr(), text_need, out_text_index.data_ptr(), rows.size, out.data_ptr(), need,
                                                     out_body_index.data_ptr(), None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    assert res.out_bytes == need and res.n_failed == 0

                baseline()
                torch.cuda.synchronize()
                assert np.array_equal(out[:need].cpu().numpy(), want), "the re-encoded bodies differ from the store's"
                entry.update(_timed(baseline))
                del dec
            shape[name] = entry
            del out, want
        results[shape_name] = shape
        del text, bodies
    L.et_ctx_destroy(h)
    print(json.dumps(results))


SLICE_CASES = ("left12", "middle64", "after_needle")


def _slice_leg(leg, lib_path, shapes):
    """slice / slice_baseline: per shape a packed store with a 12-byte needle in 10 % of its records (_search_store; encoded untimed), then
    per case -- LEFT 12 of every record; 64 symbols from the middle of every record; behind the needle up to the next space, of the records
    that hold it (rows and positions from an untimed search) -- the timed call: et_slice_packed_device, its bytes and offsets checked
    against et_encode_packed_device of Python's slices first, beside it the sizes-only call and the two floors on the same store and rows
    (et_search_packed_device CONTAINS: the walk with nothing written; et_take_packed_device: the copy alone) -- or what it replaces:
    et_decode_packed_device of the store (et_decode_packed_gather_device where the rows are a selection), then et_encode_packed_device
    of the sliced text; the cutting in between is not timed."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N

    base = leg == "slice_baseline"
    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device", "et_decode_packed_gather_device"]
                      + ([] if base else ["et_slice_packed_device", "et_slice_lane_bytes", "et_search_packed_device", "et_take_packed_device"]))
    results = {} if base else {"lane_bytes": int(L.et_slice_lane_bytes())}
    for count, size in SHAPES + [KEY_SHAPE]:
        shape_name = f"{count}x{size}" if isinstance(size, int) else f"{count}x{size[0]}-{size[1]}"
        if shapes and shape_name not in shapes:
            continue
        host, index, needle, (found, pos, _) = _search_store(count, size, 0.1)
        blob, lengths = host.tobytes(), np.diff(index).astype(np.int64)
        text = torch.from_numpy(host).to(dev)
        cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, text, index, _codebook(L, [host]))
        res, shape = N.PackedResult(), {"records": count, "body_bytes": body_bytes}
        everyone = np.arange(count, dtype=np.uint32)
        cases = {"left12": (None, np.zeros(count, np.int64), np.full(count, 12), None), "middle64": (None, lengths // 2, np.full(count, 64), None),
                 "after_needle": (np.array(found, dtype=np.uint32), np.array(pos, dtype=np.int64) + len(needle), np.full(len(found), 0xFFFFFFFF), ord(" "))}
        for name in SLICE_CASES:
            rows, first, cnt, stop = cases[name]
            at = everyone if rows is None else rows
            pieces = []
            for r, f, c in zip(at.tolist(), first.tolist(), cnt.tolist()):
                piece = blob[int(index[r]) + f : min(int(index[r]) + f + c, int(index[r + 1]))] if f < lengths[r] else b""
                pieces.append(piece if stop is None or bytes([stop]) not in piece else piece[: piece.index(bytes([stop]))])
            cut_index = np.concatenate(([0], np.cumsum([len(x) for x in pieces]))).astype(np.uint64)
            cut_total = int(cut_index[-1])
            cut_text = torch.from_numpy(np.frombuffer(b"".join(pieces) + b"\0", np.uint8).copy()).to(dev)
            _, want, need, want_index, cut_text_index = _packed_store(L, h, cut_text, cut_index, cb)  # what the slices must be: the encoder's bodies of Python's slices
            n_rows = at.size
            d_rows = torch.from_numpy(at.view(np.int32).copy()).to(dev)
            out = torch.zeros(need + 64, dtype=torch.uint8, device=dev)
            out_body_index, out_text_index = (torch.zeros(n_rows + 1, dtype=torch.int64, device=dev) for _ in range(2))
            entry = {"rows": int(n_rows), "bytes": need, "text_bytes": cut_total}
            if base:
                room = int(index[-1]) if rows is None else int(lengths[at.astype(np.int64)].sum())
                dec = torch.zeros(room + 64, dtype=torch.uint8, device=dev)

                def baseline():
                    if rows is None:
                        assert L.et_decode_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, dec.data_ptr(), room, None,
                                                         None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    else:
                        assert L.et_decode_packed_gather_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, d_rows.data_ptr(),
                                                                n_rows, dec.data_ptr(), room, out_text_index.data_ptr(), None, None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    assert res.out_bytes == room and res.n_failed == 0 and res.n_short == 0
                    assert L.et_encode_packed_device(h, ctypes.byref(cb), cut_text.data_ptr(), cut_total, cut_text_index.data_ptr(), n_rows, out.data_ptr(), need, out_body_index.data_ptr(),
                                                     None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    assert res.out_bytes == need and res.n_failed == 0

                baseline()
                torch.cuda.synchronize()
                assert torch.equal(out[:need], want[:need]) and torch.equal(out_body_index, want_index)
                entry.update(_timed(baseline))
                del dec
            else:
                tres, mres = N.TakeResult(), N.MatchResult()
                d_first, d_count = (torch.from_numpy(v.astype(np.uint32).view(np.int32).copy()).to(dev) for v in (first, cnt))
                scalars = name == "left12"  # (the scalars where every row has the same; device arrays else)

                def call(d_out=out):
                    assert L.et_slice_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count,
                                                    None if rows is None else d_rows.data_ptr(), n_rows, None if scalars else d_first.data_ptr(), 0, None if scalars else d_count.data_ptr(),
                                                    12, -1 if stop is None else stop, None if d_out is None else d_out.data_ptr(), need, out_body_index.data_ptr(),
                                                    out_text_index.data_ptr(), None, ctypes.byref(tres)) == 0, L.et_last_error(h)
                    assert tres.out_bytes == need and tres.text_bytes == cut_total and tres.n_failed == 0

                call()
                torch.cuda.synchronize()
                assert torch.equal(out[:need], want[:need]), "the slices differ from the encoder's bodies of Python's slices"
                assert torch.equal(out_body_index, want_index) and torch.equal(out_text_index, cut_text_index)
                entry.update(_timed(call))
                entry["sizes_only"] = _timed(lambda: call(None))
                d_hits, d_pos = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(2))

                def search():
                    assert L.et_search_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, needle, len(needle),
                                                     N.ET_SEARCH_CONTAINS, d_hits.data_ptr(), count, d_pos.data_ptr(), None, ctypes.byref(mres)) == 0, L.et_last_error(h)

                taken = torch.zeros(body_bytes + 64, dtype=torch.uint8, device=dev)

                def take():
                    assert L.et_take_packed_device(h, bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, d_rows.data_ptr(), n_rows, taken.data_ptr(),
                                                   body_bytes, out_body_index.data_ptr(), out_text_index.data_ptr(), None, ctypes.byref(tres)) == 0, L.et_last_error(h)

                entry["search_floor"] = _timed(search)
                entry["take_floor"] = _timed(take)
                entry["vs_search_floor"] = round(entry["ms"] / entry["search_floor"]["ms"], 2)
                entry["vs_take_floor"] = round(entry["ms"] / entry["take_floor"]["ms"], 2)
                if name == "after_needle":  # the pair as it runs: the search's rows and positions straight into the slice, first = pos + 12 by a torch add

                    def pair():
                        search()
                        d_after = d_pos[: mres.n_match] + len(needle)
                        assert L.et_slice_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, d_hits.data_ptr(),
                                                        mres.n_match, d_after.data_ptr(), 0, None, 0xFFFFFFFF, stop, out.data_ptr(), need, out_body_index.data_ptr(),
                                                        out_text_index.data_ptr(), None, ctypes.byref(tres)) == 0, L.et_last_error(h)

                    pair()
                    torch.cuda.synchronize()
                    assert torch.equal(out[:need], want[:need]) and mres.n_match == n_rows
                    entry["search_then_slice"] = _timed(pair)
                del taken
            shape[name] = entry
            del out, want, cut_text
        results[shape_name] = shape
        del text, bodies
    L.et_ctx_destroy(h)
    print(json.dumps(results))


CSV_SHAPE = (262144, "csv")  # the field legs' third shape: generated lines of 8 comma-separated fields of 4 .. 16 bytes
FIELD_CASES = {"pages": [(3, "tenth"), (100, "tenth")], "csv": [(0, "all"), (3, "all"), (7, "all"), (0, "tenth"), (3, "tenth"), (7, "tenth")]}


def _csv_store(count):
    """-> (text, text_index): `count` lines of 8 comma-separated fields of 4 .. 16 text-like bytes each (a comma or a line end in
    the source text becomes a space)."""
    import numpy as np

    from tests import corpus

    rng = np.random.default_rng(0xF1E1DB + count)
    widths = rng.integers(4, 17, size=(count, 8))
    lengths = widths.sum(axis=1) + 7
    index = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    host = corpus.text_like(int(index[-1]), 0xF1E1DC + count).copy()
    host[(host == ord(",")) | (host == 10)] = ord(" ")
    commas = (index[:-1, None].astype(np.int64) + np.cumsum(widths + 1, axis=1)[:, :7] - 1).ravel()  # behind each of a line's first seven fields
    host[commas] = ord(",")
    return host, index


def _field_leg(leg, lib_path, shapes):
    """field / field_baseline: per shape a packed store (encoded untimed) -- the two page shapes with the space as the delimiter, fields 3
    and 100 of 10 % of the records; 262 144 CSV lines (_csv_store), fields 0, 3 and 7 of every record and of 10 % -- then the timed call:
    et_field_packed_device, its bytes, offsets and positions checked against et_encode_packed_device of Python's split over the plain
    texts first, beside it the sizes-only call and two floors on the same store (et_slice_packed_device(0, TO_END, stop=delim) on the
    same rows: field 0 does the same work; et_search_packed_device CONTAINS over the whole store: the walk with nothing written) -- or
    what it replaces: et_decode_packed_device of the store (et_decode_packed_gather_device where the rows are a selection), then
    et_encode_packed_device of the cut text; the cutting in between is not timed."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N

    base = leg == "field_baseline"
    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device", "et_decode_packed_gather_device"]
                      + ([] if base else ["et_field_packed_device", "et_field_lane_bytes", "et_slice_packed_device", "et_search_packed_device"]))
    results = {} if base else {"lane_bytes": int(L.et_field_lane_bytes())}
    for count, size in SHAPES + [CSV_SHAPE]:
        shape_name = f"{count}x{size}"
        if shapes and shape_name not in shapes:
            continue
        csv = size == "csv"
        if csv:
            host, index = _csv_store(count)
        else:
            host, index, _, _ = _search_store(count, size, 0.1)
        delim = ord(",") if csv else ord(" ")
        needle = host[-SEARCH_NEEDLE_LEN:].tobytes()  # (the floor's walk: what it finds does not matter)
        blob, d = host.tobytes(), bytes([delim])
        text = torch.from_numpy(host).to(dev)
        cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, text, index, _codebook(L, [host]))
        res, shape = N.PackedResult(), {"records": count, "body_bytes": body_bytes}
        tenth = np.sort(np.random.default_rng(0xF1E1DD + count).choice(count, size=count // 10, replace=False)).astype(np.uint32)
        parts_of = {}
        for field, sel in FIELD_CASES["csv" if csv else "pages"]:
            name = f"field{field}_{sel}"
            rows = None if sel == "all" else tenth
            at = np.arange(count, dtype=np.uint32) if rows is None else rows
            pieces, where = [], []
            for r in at.tolist():
                if r not in parts_of:
                    parts_of[r] = blob[int(index[r]) : int(index[r + 1])].split(d)
                parts = parts_of[r]
                pieces.append(parts[field] if field < len(parts) else b"")
                where.append(sum(len(x) + 1 for x in parts[:field]) if field < len(parts) else 0xFFFFFFFF)
            cut_index = np.concatenate(([0], np.cumsum([len(x) for x in pieces]))).astype(np.uint64)
            cut_total = int(cut_index[-1])
            cut_text = torch.from_numpy(np.frombuffer(b"".join(pieces) + b"\0", np.uint8).copy()).to(dev)
            _, want, need, want_index, cut_text_index = _packed_store(L, h, cut_text, cut_index, cb)  # what the fields must be: the encoder's bodies of Python's split
            n_rows = at.size
            d_rows = torch.from_numpy(at.view(np.int32).copy()).to(dev)
            out = torch.zeros(need + 64, dtype=torch.uint8, device=dev)
            out_body_index, out_text_index = (torch.zeros(n_rows + 1, dtype=torch.int64, device=dev) for _ in range(2))
            entry = {"rows": int(n_rows), "bytes": need, "text_bytes": cut_total, "absent": int(sum(w == 0xFFFFFFFF for w in where))}
            if base:
                room = int(index[-1]) if rows is None else int(np.diff(index).astype(np.int64)[at.astype(np.int64)].sum())
                dec = torch.zeros(room + 64, dtype=torch.uint8, device=dev)

                def baseline():
                    if rows is None:
                        assert L.et_decode_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, dec.data_ptr(), room, None,
                                                         None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    else:
                        assert L.et_decode_packed_gather_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, d_rows.data_ptr(),
                                                                n_rows, dec.data_ptr(), room, out_text_index.data_ptr(), None, None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    assert res.out_bytes == room and res.n_failed == 0 and res.n_short == 0
                    assert L.et_encode_packed_device(h, ctypes.byref(cb), cut_text.data_ptr(), cut_total, cut_text_index.data_ptr(), n_rows, out.data_ptr(), need, out_body_index.data_ptr(),
                                                     None, ctypes.byref(res)) == 0, L.et_last_error(h)
                    assert res.out_bytes == need and res.n_failed == 0

                baseline()
                torch.cuda.synchronize()
                assert torch.equal(out[:need], want[:need]) and torch.equal(out_body_index, want_index)
                entry.update(_timed(baseline))
                del dec
            else:
                tres, mres = N.TakeResult(), N.MatchResult()
                d_pos = torch.zeros(n_rows, dtype=torch.int32, device=dev)
                rows_p = None if rows is None else d_rows.data_ptr()

                def call(d_out=out):
                    assert L.et_field_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, rows_p, n_rows, None, field,
                                                    None, 1, delim, None if d_out is None else d_out.data_ptr(), need, out_body_index.data_ptr(), out_text_index.data_ptr(),
                                                    d_pos.data_ptr(), None, ctypes.byref(tres)) == 0, L.et_last_error(h)
                    assert tres.out_bytes == need and tres.text_bytes == cut_total and tres.n_failed == 0

                call()
                torch.cuda.synchronize()
                assert torch.equal(out[:need], want[:need]), "the fields differ from the encoder's bodies of Python's split"
                assert torch.equal(out_body_index, want_index) and torch.equal(out_text_index, cut_text_index)
                assert d_pos.cpu().numpy().view(np.uint32).tolist() == where, "the positions differ from Python's"
                entry.update(_timed(call))
                entry["sizes_only"] = _timed(lambda: call(None))
                sliced = torch.zeros(body_bytes + 64, dtype=torch.uint8, device=dev)
                d_hits, d_found = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(2))

                def slice0():
                    assert L.et_slice_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, rows_p, n_rows, None, 0,
                                                    None, 0xFFFFFFFF, delim, sliced.data_ptr(), body_bytes, out_body_index.data_ptr(), out_text_index.data_ptr(), None,
                                                    ctypes.byref(tres)) == 0, L.et_last_error(h)

                def search():
                    assert L.et_search_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), count, needle, len(needle),
                                                     N.ET_SEARCH_CONTAINS, d_hits.data_ptr(), count, d_found.data_ptr(), None, ctypes.byref(mres)) == 0, L.et_last_error(h)

                entry["slice0_floor"] = _timed(slice0)
                entry["search_floor"] = _timed(search)
                entry["vs_slice0_floor"] = round(entry["ms"] / entry["slice0_floor"]["ms"], 2)
                entry["vs_search_floor"] = round(entry["ms"] / entry["search_floor"]["ms"], 2)
                del sliced
            shape[name] = entry
            del out, want, cut_text
        results[shape_name] = shape
        del text, bodies
    L.et_ctx_destroy(h)
    print(json.dumps(results))


def _concat_leg(lib_path, shapes):
    """concat: on the 262 144 CSV lines the stores of field 0 and of field 3 (et_field_packed_device, untimed), then field0 + "," +
    field3 of every row and of 10 % of the rows, and "user=" + field0 of every row (no left side); on 4 096 x 4 KiB two selections of
    10 % of the records with nothing between them (the workgroup's walk on both sides).  Per case et_concat_packed_device, its bytes
    and offsets checked against the other route's, beside it the sizes-only call -- and, in the same process, the route it replaces:
    et_decode_packed_device (et_decode_packed_gather_device where the rows are a selection) of both sides, the concatenated text and
    its offsets built with torch on the device, et_encode_packed_device."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device", "et_decode_packed_gather_device", "et_field_packed_device", "et_concat_packed_device", "et_concat_lane_bytes"])
    results = {"lane_bytes": int(L.et_concat_lane_bytes())}
    res, tres = N.PackedResult(), N.TakeResult()

    def store_of(text, index, cb=None):
        cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, text, index, cb)
        return cb, (bodies, body_bytes, body_index, text_index, index.size - 1)

    def field_of(cb, st, field):  # -> the store of one field of every record
        bodies, body_bytes, body_index, text_index, n = st
        out = torch.zeros(body_bytes + 64, dtype=torch.uint8, device=dev)
        bi, ti = (torch.zeros(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
        assert L.et_field_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n, None, n, None, field, None, 1, ord(","),
                                        out.data_ptr(), body_bytes, bi.data_ptr(), ti.data_ptr(), None, None, ctypes.byref(tres)) == 0 and tres.n_failed == 0, L.et_last_error(h)
        torch.cuda.synchronize()
        return out, int(tres.out_bytes), bi, ti, n

    def lengths_of(st, d_rows):
        text_index = st[3]
        if d_rows is None:
            return text_index[1:] - text_index[:-1]
        rows = d_rows.to(torch.int64)
        return text_index[rows + 1] - text_index[rows]

    def decode(cb, st, d_rows, n_rows, room):  # -> the rows' texts back to back, on the device
        bodies, body_bytes, body_index, text_index, n = st
        dec = torch.empty(room + 64, dtype=torch.uint8, device=dev)
        if d_rows is None:
            assert L.et_decode_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n, dec.data_ptr(), room, None, None,
                                             ctypes.byref(res)) == 0, L.et_last_error(h)
        else:
            at = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
            assert L.et_decode_packed_gather_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n, d_rows.data_ptr(), n_rows,
                                                    dec.data_ptr(), room, at.data_ptr(), None, None, ctypes.byref(res)) == 0, L.et_last_error(h)
        assert res.out_bytes == room and res.n_failed == 0 and res.n_short == 0
        return dec

    def case(cb, A, B, rows_a, rows_b, sep, n_rows):
        d_rows = [None if r is None else torch.from_numpy(r.view(np.int32).copy()).to(dev) for r in (rows_a, rows_b)]
        sep_t = torch.from_numpy(np.frombuffer(sep, np.uint8).copy()).to(dev)
        room_out = sum(st[1] for st in (A, B) if st is not None) + n_rows * (len(sep) * 4 + 1)  # (a bound: whole stores, a literal of 32-bit codes)
        outs = [torch.zeros(room_out + 64, dtype=torch.uint8, device=dev) for _ in range(2)]
        idx = [[torch.zeros(n_rows + 1, dtype=torch.int64, device=dev) for _ in range(2)] for _ in range(2)]
        side = lambda st, r: ([None, 0, None, None, 0, None] if st is None else [st[0].data_ptr(), st[1], st[2].data_ptr(), st[3].data_ptr(), st[4], None if r is None else r.data_ptr()])  # noqa: E731

        def call(d_out=outs[0]):
            assert L.et_concat_packed_device(h, ctypes.byref(cb), *side(A, d_rows[0]), sep, len(sep), *side(B, d_rows[1]), n_rows, None if d_out is None else d_out.data_ptr(), room_out,
                                             idx[0][0].data_ptr(), idx[0][1].data_ptr(), None, ctypes.byref(tres)) == 0, L.et_last_error(h)
            assert tres.n_failed == 0

        rooms = [0 if st is None else int(lengths_of(st, r).sum()) for st, r in ((A, d_rows[0]), (B, d_rows[1]))]  # (known to the caller: not part of the route)
        total = sum(rooms) + n_rows * len(sep)

        def baseline():
            zero = torch.zeros(n_rows, dtype=torch.int64, device=dev)
            len_a, len_b = (zero if st is None else lengths_of(st, r) for st, r in ((A, d_rows[0]), (B, d_rows[1])))
            new_index = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
            torch.cumsum(len_a + len(sep) + len_b, 0, out=new_index[1:])
            text = torch.empty(total + 64, dtype=torch.uint8, device=dev)
            for st, r, room, lengths, shift in ((A, d_rows[0], rooms[0], len_a, new_index[:-1]), (B, d_rows[1], rooms[1], len_b, new_index[:-1] + len_a + len(sep))):
                if st is not None:  # byte i of the decoded side belongs to row[i]: it moves by where that row's part begins now less where it began
                    dec = decode(cb, st, r, n_rows, room)
                    row = torch.repeat_interleave(torch.arange(n_rows, device=dev), lengths, output_size=room)
                    text[torch.arange(room, device=dev) + (shift - (torch.cumsum(lengths, 0) - lengths))[row]] = dec[:room]
            if len(sep):
                text[((new_index[:-1] + len_a)[:, None] + torch.arange(len(sep), device=dev)[None, :]).reshape(-1)] = sep_t.repeat(n_rows)
            assert L.et_encode_packed_device(h, ctypes.byref(cb), text.data_ptr(), total, new_index.data_ptr(), n_rows, outs[1].data_ptr(), room_out, idx[1][0].data_ptr(), None,
                                             ctypes.byref(res)) == 0 and res.n_failed == 0, L.et_last_error(h)

        call()
        baseline()
        torch.cuda.synchronize()
        need = int(tres.out_bytes)
        assert need == int(res.out_bytes) and torch.equal(outs[0][:need], outs[1][:need]) and torch.equal(idx[0][0], idx[1][0]), "the two routes differ"
        entry = {"rows": int(n_rows), "bytes": need, "text_bytes": int(tres.text_bytes)}
        entry.update(_timed(call))
        entry["sizes_only"] = _timed(lambda: call(None))
        entry["baseline"] = _timed(baseline)
        gap, spreads = entry["baseline"]["ms"] - entry["ms"], (entry["baseline"]["max_ms"] - entry["baseline"]["min_ms"]) + (entry["max_ms"] - entry["min_ms"])
        entry["baseline_over_concat"], entry["beyond_both_spreads"] = round(entry["baseline"]["ms"] / entry["ms"], 2), bool(gap > spreads)
        return entry

    count = CSV_SHAPE[0]
    if not shapes or f"{count}xcsv" in shapes:
        host, index = _csv_store(count)
        cb, lines = store_of(torch.from_numpy(host).to(dev), index, _codebook(L, [host, np.frombuffer(b"user=", np.uint8)]))
        f0, f3 = field_of(cb, lines, 0), field_of(cb, lines, 3)
        tenth = np.sort(np.random.default_rng(0xC07CA7 + count).choice(count, size=count // 10, replace=False)).astype(np.uint32)
        results[f"{count}xcsv"] = {"records": count, "field0_comma_field3_all": case(cb, f0, f3, None, None, b",", count),
                                   "field0_comma_field3_tenth": case(cb, f0, f3, tenth, tenth, b",", tenth.size), "user_prefix_field0_all": case(cb, None, f0, None, None, b"user=", count)}
        del lines, f0, f3
    count, size = SHAPES[1]
    if not shapes or f"{count}x{size}" in shapes:
        host, index, _, _ = _search_store(count, size, 0.1)
        cb, pages = store_of(torch.from_numpy(host).to(dev), index, _codebook(L, [host]))
        rng = np.random.default_rng(0xC07CA8 + count)
        rows_a, rows_b = (np.sort(rng.choice(count, size=count // 10, replace=False)).astype(np.uint32) for _ in range(2))
        results[f"{count}x{size}"] = {"records": count, "two_selections_tenth": case(cb, pages, pages, rows_a, rows_b, b"", rows_a.size)}
    L.et_ctx_destroy(h)
    print(json.dumps(results))


RECODE_SWEEP_SIZES = (128, 512, 1024, 2048, 4096, 8192, 12288)  # bytes of text per record of the recode sweep's stores (bodies of about 0.6 of that)


def _recode_leg(lib_path, shapes, sweep=False):
    """recode_sweep (only when named): stores of SWEEP_BYTES of text in records of one size each, every row re-tabled: the times from
    which RECODE_LANE_BYTES would be chosen -- run it on builds with -DET_RECODE_LANE_BYTES=0 and =8192 (ET_LIB_PATH names the library).
    recode: on 1 024 x 64 KiB, 4 096 x 4 KiB and the 262 144 CSV lines three cells -- every row re-tabled (table OUT from the
    histogram turned upside down over the same symbols), ASCII UPPER of every row under one table (of the text and its upper-cased
    self), a random 10 % of the rows re-tabled.  Per cell et_recode_packed_device, its bytes and offsets checked against the other
    route's, beside it the sizes-only call (what the plan costs without the write) and the slice [0, TO_END) of the same rows (a walk
    and a copy: the floor) -- and, in the same process, the route it replaces: et_decode_packed_device (et_decode_packed_gather_device
    for a selection), a torch gather through the 256-entry table where there is a map, et_encode_packed_device under table OUT."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device", "et_decode_packed_gather_device", "et_slice_packed_device", "et_recode_packed_device", "et_recode_lane_bytes"])
    results = {"lane_bytes": int(L.et_recode_lane_bytes())}
    res, tres = N.PackedResult(), N.TakeResult()
    upper = np.arange(256, dtype=np.int16)
    upper[97:123] -= 32

    def table_of(hist):
        cb = N.Codebook()
        hist = np.ascontiguousarray(hist, dtype=np.uint64)
        assert L.et_build_codebook(hist.ctypes.data, ctypes.byref(cb)) == 0 and L.et_codebook_is_complete(ctypes.byref(cb)) == 0
        return cb

    def case(cb_in, cb_out, st, rows, bmap):
        bodies, body_bytes, body_index, text_index, n = st
        n_rows = n if rows is None else rows.size
        d_rows = None if rows is None else torch.from_numpy(rows.view(np.int32).copy()).to(dev)
        rows_p = None if d_rows is None else d_rows.data_ptr()
        map_p = None if bmap is None else bmap.ctypes.data
        lut = None if bmap is None else torch.from_numpy(bmap.astype(np.uint8)).to(dev)
        idx = [[torch.zeros(n_rows + 1, dtype=torch.int64, device=dev) for _ in range(2)] for _ in range(3)]

        def call(d_out, cap):
            assert L.et_recode_packed_device(h, ctypes.byref(cb_in), ctypes.byref(cb_out), map_p, bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n,
                                             rows_p, n_rows, None if d_out is None else d_out.data_ptr(), cap, idx[0][0].data_ptr(), idx[0][1].data_ptr(), None,
                                             ctypes.byref(tres)) == 0, L.et_last_error(h)
            assert tres.n_failed == 0

        call(None, 0)
        need, room = int(tres.out_bytes), int(tres.text_bytes)  # (no drops: the rows' text bytes are the old ones)
        outs = [torch.zeros(need + 64, dtype=torch.uint8, device=dev) for _ in range(2)]
        sliced = torch.zeros(body_bytes + 64, dtype=torch.uint8, device=dev)
        at = text_index if d_rows is None else torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)

        def baseline():
            dec = torch.empty(room + 64, dtype=torch.uint8, device=dev)
            if d_rows is None:
                assert L.et_decode_packed_device(h, ctypes.byref(cb_in), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n, dec.data_ptr(), room, None,
                                                 None, ctypes.byref(res)) == 0, L.et_last_error(h)
            else:
                assert L.et_decode_packed_gather_device(h, ctypes.byref(cb_in), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n, rows_p, n_rows,
                                                        dec.data_ptr(), room, at.data_ptr(), None, None, ctypes.byref(res)) == 0, L.et_last_error(h)
            assert res.out_bytes == room and res.n_failed == 0 and res.n_short == 0
            text = dec if lut is None else lut[dec[:room].to(torch.int64)]
            assert L.et_encode_packed_device(h, ctypes.byref(cb_out), text.data_ptr(), room, at.data_ptr(), n_rows, outs[1].data_ptr(), need, idx[1][0].data_ptr(), None,
                                             ctypes.byref(res)) == 0 and res.n_failed == 0, L.et_last_error(h)

        def slice0():
            assert L.et_slice_packed_device(h, ctypes.byref(cb_in), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n, rows_p, n_rows, None, 0, None,
                                            0xFFFFFFFF, -1, sliced.data_ptr(), body_bytes, idx[2][0].data_ptr(), idx[2][1].data_ptr(), None, ctypes.byref(tres)) == 0, L.et_last_error(h)

        call(outs[0], need)
        baseline()
        torch.cuda.synchronize()
        assert need == int(res.out_bytes) and torch.equal(outs[0][:need], outs[1][:need]) and torch.equal(idx[0][0], idx[1][0]), "the two routes differ"
        entry = {"rows": int(n_rows), "bytes": need, "text_bytes": room}
        entry.update(_timed(lambda: call(outs[0], need)))
        entry["sizes_only"] = _timed(lambda: call(None, 0))
        entry["slice0_floor"] = _timed(slice0)
        entry["baseline"] = _timed(baseline)
        gap, spreads = entry["baseline"]["ms"] - entry["ms"], (entry["baseline"]["max_ms"] - entry["baseline"]["min_ms"]) + (entry["max_ms"] - entry["min_ms"])
        entry["baseline_over_recode"], entry["beyond_both_spreads"] = round(entry["baseline"]["ms"] / entry["ms"], 2), bool(gap > spreads)
        entry["vs_slice0_floor"] = round(entry["ms"] / entry["slice0_floor"]["ms"], 2)
        return entry

    todo = [(f"{count}x{size}", lambda count=count, size=size: _search_store(count, size, 0.1)[:2]) for count, size in SHAPES] + [(f"{CSV_SHAPE[0]}xcsv", lambda: _csv_store(CSV_SHAPE[0]))]
    if sweep:
        todo = [(f"{SWEEP_BYTES // size}x{size}", lambda size=size: _search_store(SWEEP_BYTES // size, size, 0.1)[:2]) for size in RECODE_SWEEP_SIZES]
    for name, make in todo:
        if shapes and name not in shapes:
            continue
        host, index = make()
        n = index.size - 1
        hist = np.bincount(host, minlength=256).astype(np.uint64)
        turned = np.where(hist > 0, hist.max() + 1 - hist, 0)  # the same symbols, what was frequent is rare
        hist_up = hist + np.bincount(np.frombuffer(host.tobytes().upper(), np.uint8), minlength=256).astype(np.uint64)
        text = torch.from_numpy(host).to(dev)
        cb1, cb2, cbu = table_of(hist), table_of(turned), table_of(hist_up)
        _, *plain = _packed_store(L, h, text, index, cb1)
        cased = None if sweep else _packed_store(L, h, text, index, cbu)[1:]
        if sweep:
            results[name] = {"records": n, "retable_all": case(cb1, cb2, (*plain, n), None, None)}
            continue
        tenth = np.sort(np.random.default_rng(0x4EC0DE + n).choice(n, size=n // 10, replace=False)).astype(np.uint32)
        results[name] = {"records": n, "retable_all": case(cb1, cb2, (*plain, n), None, None), "upper_all": case(cbu, cbu, (*cased, n), None, upper),
                         "retable_tenth": case(cb1, cb2, (*plain, n), tenth, None)}
        del text, plain, cased
    L.et_ctx_destroy(h)
    print(json.dumps(results))


GROUP_POOLS = [("pool_16", 16, 0.0), ("pool_1024", 1024, 0.0), ("pool_65536", 65536, 0.0), ("all_distinct", None, 0.0), ("pool_1024_one_value_90pct", 1024, 0.9)]


def _group_store(count, size, pool, hot):
    """-> (text, text_index) as numpy arrays: `count` records drawn from `pool` different text-like values (None: every record its own),
    as long as `size` says (a number, or a range); `hot` of the records hold value 0.  A value's first four bytes spell its number, so
    that no two values are the same text."""
    import numpy as np

    from tests import corpus

    n_values = count if pool is None else pool
    rng = np.random.default_rng(0x6E0A9 + count + n_values + int(hot * 1000))
    value_lengths = np.full(n_values, size) if isinstance(size, int) else rng.integers(size[0], size[1] + 1, size=n_values)
    value_index = np.concatenate(([0], np.cumsum(value_lengths))).astype(np.int64)
    values = corpus.text_like(int(value_index[-1]), 0x6E0A9 + n_values).copy()
    for k in range(4):
        values[value_index[:-1] + k] = 48 + ((np.arange(n_values) >> (6 * k)) & 63)
    pick = np.arange(count) if pool is None else rng.integers(0, n_values, size=count)
    if hot:
        pick[rng.random(count) < hot] = 0
    lengths = value_lengths[pick]
    index = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    src = np.repeat(value_index[pick] - index[:-1], lengths) + np.arange(int(index[-1]))
    return values[src], index.astype(np.uint64)


def _group_leg(lib_path, shapes):
    """group: on the 262 144 key-like records texts drawn from pools of 16, 1 024 and 65 536 values, all different, and 1 024 values with
    one of them on 90 % of the records; on 4 096 x 4 KiB pages drawn from a pool of 512 (the wavefront's path).  Per case
    et_group_packed_device with all three outputs, beside it the count-only call -- and, in the same process, the route it replaces:
    et_decode_packed_device, the texts padded into an [n, longest + 4] matrix on the device with the length in the last four columns (no
    padding makes two texts equal), torch.unique(dim=0, return_inverse=True, return_counts=True).  The two routes' answers are compared
    first: the partition d_group_of induces is the one `inverse` induces, and the counts agree class by class."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device", "et_group_packed_device"])
    results = {}
    res, gres = N.PackedResult(), N.GroupResult()

    def case(host, index):
        n, total = index.size - 1, int(index[-1])
        cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, torch.from_numpy(host).to(dev), index)
        first, count, group_of = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        lengths = text_index[1:] - text_index[:-1]
        longest = int(lengths.max())
        found = {}

        def call(write=True):
            assert L.et_group_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n, first.data_ptr() if write else None, n,
                                            count.data_ptr() if write else None, group_of.data_ptr() if write else None, None, ctypes.byref(gres)) == 0, L.et_last_error(h)
            assert gres.n_failed == 0

        def baseline():
            dec = torch.empty(total + 64, dtype=torch.uint8, device=dev)
            assert L.et_decode_packed_device(h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n, dec.data_ptr(), total, None, None,
                                             ctypes.byref(res)) == 0 and res.n_failed == 0 and res.n_short == 0, L.et_last_error(h)
            padded = torch.zeros((n, longest + 4), dtype=torch.uint8, device=dev)
            row = torch.repeat_interleave(torch.arange(n, device=dev), lengths, output_size=total)
            padded[row, torch.arange(total, device=dev) - text_index[:-1][row]] = dec[:total]
            padded[:, longest:] = lengths.to(torch.int32).view(torch.uint8).reshape(n, 4)
            found["values"], found["inverse"], found["counts"] = torch.unique(padded, dim=0, return_inverse=True, return_counts=True)

        call()
        baseline()
        torch.cuda.synchronize()
        g = int(gres.n_groups)
        of, inverse = group_of.to(torch.int64), found["inverse"].reshape(-1).to(torch.int64)
        assert g == found["counts"].numel() and torch.unique(of * g + inverse).numel() == g, "the two routes' partitions differ"
        assert torch.equal(count[:g].to(torch.int64), found["counts"][inverse[first[:g].to(torch.int64)]].to(torch.int64)), "the two routes' counts differ"
        assert int(count[:g].sum()) == n and bool((first[1:g] > first[: g - 1]).all())
        entry = {"records": int(n), "groups": g, "largest_group": int(count[:g].max()), "text_bytes": total, "body_bytes": body_bytes}
        entry.update(_timed(call))
        entry["count_only"] = _timed(lambda: call(False))
        entry["baseline"] = _timed(baseline)
        gap, spreads = entry["baseline"]["ms"] - entry["ms"], (entry["baseline"]["max_ms"] - entry["baseline"]["min_ms"]) + (entry["max_ms"] - entry["min_ms"])
        entry["baseline_over_group"], entry["beyond_both_spreads"] = round(entry["baseline"]["ms"] / entry["ms"], 2), bool(gap > spreads)
        found.clear()
        return entry

    count, size = KEY_SHAPE
    name = f"{count}x{size[0]}-{size[1]}"
    if not shapes or name in shapes:
        results[name] = {case_name: case(*_group_store(count, size, pool, hot)) for case_name, pool, hot in GROUP_POOLS}
    count, size = SHAPES[1]
    if not shapes or f"{count}x{size}" in shapes:
        results[f"{count}x{size}"] = {"pool_512": case(*_group_store(count, size, 512, 0.0))}
    L.et_ctx_destroy(h)
    print(json.dumps(results))


NUMBER_POOLS = (16, 65536)          # the number leg's key pools: field 0 of its CSV lines
NUMBER_NEEDLE = b"page-amount="     # ... and what stands in front of the number in its pages: 12 bytes
NUMBER_WIDTH = 20                   # columns of the baseline's padded matrix: a sign and 19 digits


def _number_lines(count, pool):
    """-> (text, text_index, keys, amounts): `count` CSV lines of 8 fields -- field 0 a key out of `pool`, field 3 an integer of either
    sign with 1 .. 12 digits, the others 4 .. 16 text-like bytes (a comma or a line end in the source text becomes a space)."""
    import numpy as np

    from tests import corpus

    rng = np.random.default_rng(0x4E0B + count + pool)
    widths = rng.integers(4, 17, size=(count, 6))
    offs = np.concatenate(([0], np.cumsum(widths.ravel()))).astype(np.int64)
    filler = corpus.text_like(int(offs[-1]), 0x4E0C + count).copy()
    filler[(filler == ord(",")) | (filler == 10)] = ord(" ")
    blob = filler.tobytes()
    keys = rng.integers(0, pool, size=count)
    amounts = (rng.random(count) * 10.0 ** rng.integers(1, 13, size=count)).astype(np.int64) * rng.choice([-1, 1], size=count)
    lines = []
    for i in range(count):
        f = [blob[offs[6 * i + j] : offs[6 * i + j + 1]] for j in range(6)]
        lines.append(b"k%07d,%s,%s,%d,%s,%s,%s,%s" % (keys[i], f[0], f[1], amounts[i], f[2], f[3], f[4], f[5]))
    index = np.concatenate(([0], np.cumsum([len(x) for x in lines]))).astype(np.uint64)
    return np.frombuffer(b"".join(lines), np.uint8).copy(), index, keys, amounts


def _number_pages(count, size):
    """-> (text, text_index, amounts): `count` text-like pages of `size` bytes, in each NUMBER_NEEDLE, an integer and ";" at a random place."""
    import numpy as np

    from tests import corpus

    rng = np.random.default_rng(0x4E0D + count)
    host = corpus.text_like(count * size, 0x4E0E + count).copy()
    host[host == ord(";")] = ord(",")
    amounts = (rng.random(count) * 10.0 ** rng.integers(1, 13, size=count)).astype(np.int64) * rng.choice([-1, 1], size=count)
    for b in range(count):
        piece = NUMBER_NEEDLE + b"%d;" % amounts[b]
        at = b * size + int(rng.integers(0, size - len(piece)))
        host[at : at + len(piece)] = np.frombuffer(piece, np.uint8)
    assert all(host[b * size : (b + 1) * size].tobytes().count(NUMBER_NEEDLE) == 1 for b in range(0, count, 97))
    return host, (np.arange(count + 1) * size).astype(np.uint64), amounts


def _number_leg(lib_path, shapes):
    """number: on 262 144 CSV lines of 8 fields (field 0 a key out of a pool of 16 or 65 536, field 3 an integer) -- (a) the values of
    field 3 of every line through the field call's positions and stop=",", (b) of a random 10 %, (c) the whole column's SUM, COUNT, MIN
    and MAX, (d) SUM per key with et_group_packed_device's group numbers over field 0 -- and on 4 096 x 4 KiB pages (e) the number behind
    a 12-byte needle (search -> number).  Per case et_number_packed_device alone on positions that are already there (`ms`), the whole
    new route (`route`: the sizes-only field call, or the search, that finds the positions, then the number call) and, in the same
    process, the route it replaces (`baseline`): et_field_packed_device (or search and slice) of the column as a store,
    et_decode_packed_device of it, the text padded into an [n, 20] matrix and parsed in torch, scatter_add_ / scatter_reduce_ for the
    aggregates.  Values and aggregates are checked against Python's first.  The verdict compares `route` with `baseline`: HIT when the
    gap exceeds both spreads, MISS when it does not or the call is slower.  Floors: the slice call on the same ask, the field call."""
    import numpy as np
    import torch

    from entreepy_amd import _native as N

    L, h, dev = _open(lib_path, STORE + ["et_decode_packed_device", "et_field_packed_device", "et_slice_packed_device", "et_search_packed_device", "et_group_packed_device",
                                         "et_number_packed_device", "et_number_lane_bytes"])
    results = {"lane_bytes": int(L.et_number_lane_bytes())}
    res, tres, mres, gres, nres = N.PackedResult(), N.TakeResult(), N.MatchResult(), N.GroupResult(), N.NumberResult()
    pow10 = torch.tensor([10**k for k in range(19)], dtype=torch.int64, device=dev)
    cols = torch.arange(NUMBER_WIDTH, device=dev)[None, :]
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def parse(dec, text_index, n, total):
        """The torch parse of the baseline: the column's text padded into a matrix, sign and digits to int64."""
        lengths = text_index[1:] - text_index[:-1]
        row = torch.repeat_interleave(torch.arange(n, device=dev), lengths, output_size=total)
        padded = torch.zeros((n, NUMBER_WIDTH), dtype=torch.uint8, device=dev)
        padded[row, torch.arange(total, device=dev) - text_index[:-1][row]] = dec[:total]
        digit = padded.to(torch.int64) - 48
        mine = (digit >= 0) & (digit <= 9) & (cols < lengths[:, None])
        values = (torch.where(mine, digit, 0) * pow10[(lengths[:, None] - 1 - cols).clamp(0, 18)]).sum(dim=1)
        return torch.where(padded[:, 0] == 45, -values, values)

    def verdict(entry):
        new, old = entry["route"], entry["baseline"]
        gap, spreads = old["ms"] - new["ms"], (old["max_ms"] - old["min_ms"]) + (new["max_ms"] - new["min_ms"])
        entry["baseline_over_route"], entry["beyond_both_spreads"] = round(old["ms"] / new["ms"], 2), bool(gap > spreads)
        entry["verdict"] = "HIT" if gap > spreads else "MISS"
        return entry

    def store_of(host, index):
        n = index.size - 1
        cb, bodies, body_bytes, body_index, text_index = _packed_store(L, h, torch.from_numpy(host).to(dev), index, _codebook(L, [host]))
        return SimpleNamespace(cb=cb, bodies=bodies, body_bytes=body_bytes, body_index=body_index, text_index=text_index, n=n,
                               args=lambda: (h, ctypes.byref(cb), bodies.data_ptr(), body_bytes, body_index.data_ptr(), text_index.data_ptr(), n))

    def decode(st_args, n, total, dec):
        assert L.et_decode_packed_device(*st_args, dec.data_ptr(), total, None, None, ctypes.byref(res)) == 0 and res.n_failed == 0 and res.n_short == 0, L.et_last_error(h)

    def number(st, rows, n_rows, d_first, stop, values=None, group_of=None, n_groups=0, agg=None):
        agg = agg or {}
        assert L.et_number_packed_device(*st.args(), ptr(rows), n_rows, d_first.data_ptr(), 0, None, 0xFFFFFFFF, stop, ptr(values), None, ptr(group_of), n_groups, ptr(agg.get("sum")),
                                         ptr(agg.get("n")), ptr(agg.get("min")), ptr(agg.get("max")), None, ctypes.byref(nres)) == 0, L.et_last_error(h)
        assert nres.n_ok == n_rows and nres.n_failed == 0

    count, _ = CSV_SHAPE
    for pool in NUMBER_POOLS:
        name = f"{count}xcsv_pool_{pool}"
        if shapes and name not in shapes:
            continue
        host, index, keys, amounts = _number_lines(count, pool)
        st = store_of(host, index)
        shape = {"records": count, "body_bytes": st.body_bytes}
        tenth = np.sort(np.random.default_rng(0x4E0F + count).choice(count, size=count // 10, replace=False)).astype(np.uint32)
        d_tenth = torch.from_numpy(tenth.view(np.int32).copy()).to(dev)
        out = torch.zeros(st.body_bytes + 64, dtype=torch.uint8, device=dev)
        obi, oti = (torch.zeros(count + 1, dtype=torch.int64, device=dev) for _ in range(2))
        d_pos, values = torch.zeros(count, dtype=torch.int32, device=dev), torch.zeros(count, dtype=torch.int64, device=dev)
        dec = torch.zeros(count * NUMBER_WIDTH + 64, dtype=torch.uint8, device=dev)

        def field(k, rows, n_rows, write):
            assert L.et_field_packed_device(*st.args(), ptr(rows), n_rows, None, k, None, 1, ord(","), out.data_ptr() if write else None, st.body_bytes, obi.data_ptr(), oti.data_ptr(),
                                            d_pos.data_ptr(), None, ctypes.byref(tres)) == 0 and tres.n_failed == 0, L.et_last_error(h)

        # the group numbers of (d), untimed: both routes are given them
        field(0, None, count, True)
        g_first, g_of = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(2))
        assert L.et_group_packed_device(h, ctypes.byref(st.cb), out.data_ptr(), int(tres.out_bytes), obi.data_ptr(), oti.data_ptr(), count, g_first.data_ptr(), count, None, g_of.data_ptr(),
                                        None, ctypes.byref(gres)) == 0 and gres.n_failed == 0, L.et_last_error(h)
        torch.cuda.synchronize()
        n_groups = int(gres.n_groups)
        assert n_groups == len(set(keys.tolist()))
        g_of64 = g_of.to(torch.int64)
        first_rows = g_first[:n_groups].cpu().numpy()
        want_sums = np.zeros(pool, np.int64)
        np.add.at(want_sums, keys, amounts)
        found = {}

        def case(rows, n_rows, want_values, groups):
            """groups: None (values alone), 1 (the whole column), or n_groups (per key)."""
            entry = {"rows": int(n_rows)}
            agg = None
            if groups:
                agg = {k: torch.zeros(groups, dtype=torch.int64, device=dev) for k in (("sum", "n", "min", "max") if groups == 1 else ("sum",))}
            of = g_of if groups and groups > 1 else None

            def call():
                number(st, rows, n_rows, d_pos, ord(","), None if groups else values, of, groups or 0, agg)

            def route():
                field(3, rows, n_rows, False)
                call()

            def baseline():
                field(3, rows, n_rows, True)
                total = int(tres.text_bytes)
                decode((h, ctypes.byref(st.cb), out.data_ptr(), int(tres.out_bytes), obi.data_ptr(), oti.data_ptr(), n_rows), n_rows, total, dec)
                v = parse(dec, oti[: n_rows + 1], n_rows, total)
                found["values"] = v
                if groups == 1:
                    found["agg"] = (v.sum(), v.min(), v.max())
                elif groups:
                    found["agg"] = (torch.zeros(groups, dtype=torch.int64, device=dev).scatter_add_(0, g_of64, v),)

            route()
            baseline()
            torch.cuda.synchronize()
            assert found["values"].cpu().numpy().tolist() == want_values.tolist(), "the baseline's values differ from Python's"
            if not groups:
                assert values[:n_rows].cpu().numpy().tolist() == want_values.tolist(), "the values differ from Python's"
            elif groups == 1:
                got = [int(agg[k][0]) for k in ("sum", "n", "min", "max")]
                assert got == [int(want_values.sum()), n_rows, int(want_values.min()), int(want_values.max())] and [int(x) for x in found["agg"]] == [got[0], got[2], got[3]]
            else:
                assert torch.equal(agg["sum"], found["agg"][0]) and agg["sum"].cpu().numpy().tolist() == want_sums[keys[first_rows]].tolist(), "the sums per key differ from Python's"
            entry.update(_timed(call))
            entry["route"], entry["baseline"] = _timed(route), _timed(baseline)
            field(3, rows, n_rows, False)  # (the floors' positions)

            def slice_floor():
                assert L.et_slice_packed_device(*st.args(), ptr(rows), n_rows, d_pos.data_ptr(), 0, None, 0xFFFFFFFF, ord(","), out.data_ptr(), st.body_bytes, obi.data_ptr(),
                                                oti.data_ptr(), None, ctypes.byref(tres)) == 0, L.et_last_error(h)

            entry["slice_floor"], entry["field_floor"] = _timed(slice_floor), _timed(lambda: field(3, rows, n_rows, False))
            found.clear()
            return verdict(entry)

        shape["a_values_all"] = case(None, count, amounts, None)
        shape["b_values_tenth"] = case(d_tenth, tenth.size, amounts[tenth.astype(np.int64)], None)
        shape["c_column_sum_n_min_max"] = case(None, count, amounts, 1)
        shape["d_sum_per_key"] = dict(case(None, count, amounts, n_groups), groups=n_groups)
        results[name] = shape
        del st, out, dec

    count, size = SHAPES[1]
    name = f"{count}x{size}"
    if not shapes or name in shapes:
        host, index, amounts = _number_pages(count, size)
        st = store_of(host, index)
        d_rows, d_pos = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(2))
        values = torch.zeros(count, dtype=torch.int64, device=dev)
        out = torch.zeros(st.body_bytes + 64, dtype=torch.uint8, device=dev)
        obi, oti = (torch.zeros(count + 1, dtype=torch.int64, device=dev) for _ in range(2))
        dec = torch.zeros(count * NUMBER_WIDTH + 64, dtype=torch.uint8, device=dev)
        found = {}

        def search():
            assert L.et_search_packed_device(*st.args(), NUMBER_NEEDLE, len(NUMBER_NEEDLE), N.ET_SEARCH_CONTAINS, d_rows.data_ptr(), count, d_pos.data_ptr(), None,
                                             ctypes.byref(mres)) == 0 and mres.n_match == count, L.et_last_error(h)
            return d_pos + len(NUMBER_NEEDLE)

        d_first = search()

        def call():
            number(st, d_rows, count, d_first, ord(";"), values)

        def route():
            number(st, d_rows, count, search(), ord(";"), values)

        def baseline():
            first = search()
            assert L.et_slice_packed_device(*st.args(), d_rows.data_ptr(), count, first.data_ptr(), 0, None, 0xFFFFFFFF, ord(";"), out.data_ptr(), st.body_bytes, obi.data_ptr(),
                                            oti.data_ptr(), None, ctypes.byref(tres)) == 0 and tres.n_failed == 0, L.et_last_error(h)
            total = int(tres.text_bytes)
            decode((h, ctypes.byref(st.cb), out.data_ptr(), int(tres.out_bytes), obi.data_ptr(), oti.data_ptr(), count), count, total, dec)
            found["values"] = parse(dec, oti, count, total)

        route()
        baseline()
        torch.cuda.synchronize()
        assert values.cpu().numpy().tolist() == amounts.tolist() == found["values"].cpu().numpy().tolist(), "the values differ from Python's"
        entry = {"rows": count, "body_bytes": st.body_bytes}
        entry.update(_timed(call))
        entry["route"], entry["baseline"] = _timed(route), _timed(baseline)

        def slice_floor():
            assert L.et_slice_packed_device(*st.args(), d_rows.data_ptr(), count, d_first.data_ptr(), 0, None, 0xFFFFFFFF, ord(";"), out.data_ptr(), st.body_bytes, obi.data_ptr(),
                                            oti.data_ptr(), None, ctypes.byref(tres)) == 0, L.et_last_error(h)

        entry["slice_floor"], entry["search_floor"] = _timed(slice_floor), _timed(search)
        results[name] = {"e_number_behind_a_needle": verdict(entry)}
    L.et_ctx_destroy(h)
    print(json.dumps(results))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.environ.get("ET_PARENT_LIB_PATH"))
    ap.add_argument("--batch-lib", default=os.environ.get("ET_BATCH_LIB_PATH"))
    ap.add_argument("--legs", default="single_parent,single,batch,shared,packed,gather,match,join,take,search,order,slice,field")
    ap.add_argument("--shapes", default="")  # (the match legs: a comma list of shape names, e.g. 262144x16-48; default: all)
    ap.add_argument("--out")
    ap.add_argument("--leg")  # (internal: the child processes)
    ap.add_argument("--lib")
    a = ap.parse_args()
    if a.leg and a.leg.startswith("match"):
        return _match_leg(a.leg, a.lib, [s for s in a.shapes.split(",") if s])
    if a.leg and a.leg.startswith("order"):
        return _order_leg(a.leg, a.lib, [s for s in a.shapes.split(",") if s])
    if a.leg and a.leg.startswith("search"):
        return _search_leg(a.leg, a.lib, [s for s in a.shapes.split(",") if s])
    if a.leg and a.leg.startswith("join"):
        return _join_leg(a.leg, a.lib)
    if a.leg and a.leg.startswith("take"):
        return _take_leg(a.leg, a.lib)
    if a.leg and a.leg.startswith("slice"):
        return _slice_leg(a.leg, a.lib, [s for s in a.shapes.split(",") if s])
    if a.leg and a.leg.startswith("field"):
        return _field_leg(a.leg, a.lib, [s for s in a.shapes.split(",") if s])
    if a.leg == "concat":
        return _concat_leg(a.lib, [s for s in a.shapes.split(",") if s])
    if a.leg in ("recode", "recode_sweep"):
        return _recode_leg(a.lib, [s for s in a.shapes.split(",") if s], sweep=a.leg == "recode_sweep")
    if a.leg == "group":
        return _group_leg(a.lib, [s for s in a.shapes.split(",") if s])
    if a.leg == "number":
        return _number_leg(a.lib, [s for s in a.shapes.split(",") if s])
    if a.leg:
        return (_gather_leg if a.leg.startswith("gather") else _leg)(a.leg, a.lib)
    here = os.environ.get("ET_LIB_PATH") or os.path.join(ROOT, "entreepy_amd", "libentreepy_hip.so")
    legs = ([("single_parent", "single", a.parent_lib)] if a.parent_lib else []) + [("single", "single", here), ("batch", "batch", a.batch_lib or here), ("shared", "shared", here)]
    legs = [leg for leg in legs if leg[0] in a.legs.split(",")]
    if "packed" in a.legs.split(","):
        legs += [("packed_baseline", "dense", a.batch_lib or here), ("packed", "packed", here)]
    if "gather" in a.legs.split(","):
        legs += [("gather_baseline", "gather_baseline", a.batch_lib or here), ("gather", "gather", here)]
    if "match" in a.legs.split(","):
        legs += [("match_baseline", "match_baseline", a.batch_lib or here), ("match", "match", here)]
    if "join" in a.legs.split(","):
        legs += [("join_baseline", "join_baseline", a.batch_lib or here), ("join", "join", here)]
    if "take" in a.legs.split(","):
        legs += [("take_baseline", "take_baseline", a.batch_lib or here), ("take", "take", here)]
    if "search" in a.legs.split(","):
        legs += [("search_baseline", "search_baseline", a.batch_lib or here), ("search", "search", here)]
    if "order" in a.legs.split(","):
        legs += [("order_baseline", "order_baseline", a.batch_lib or here), ("order", "order", here)]
    if "slice" in a.legs.split(","):
        legs += [("slice_baseline", "slice_baseline", a.batch_lib or here), ("slice", "slice", here)]
    if "field" in a.legs.split(","):
        legs += [("field_baseline", "field_baseline", a.batch_lib or here), ("field", "field", here)]
    if "concat" in a.legs.split(","):  # (the baseline runs in the leg's own process, on this build)
        legs += [("concat", "concat", here)]
    if "recode" in a.legs.split(","):  # (likewise)
        legs += [("recode", "recode", here)]
    if "group" in a.legs.split(","):  # (likewise)
        legs += [("group", "group", here)]
    if "number" in a.legs.split(","):  # (likewise)
        legs += [("number", "number", here)]
    if "recode_sweep" in a.legs.split(","):
        legs += [("recode_sweep", "recode_sweep", here)]
    if "search_sweep" in a.legs.split(","):
        legs += [("search_sweep", "search_sweep", here)]
    out = {"tool": "batch_bench", "reps": REPS, "warmup": WARMUP, "batch_on_another_build": bool(a.batch_lib)}
    for name, leg, lib in legs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--lib", lib, "--shapes", a.shapes], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"leg {name} failed ({r.returncode})")
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    base = out.get("single_parent", out.get("single"))
    if base and "batch" in out:
        out["speedup_vs_" + ("parent" if a.parent_lib else "single")] = {k: round(base[k]["roundtrip_ms"] / out["batch"][k]["roundtrip_ms"], 1) for k in out["batch"]}
    if "batch" in out and "shared" in out:
        out["shared_vs_batch"] = {k: {w: round(out["batch"][k][w] / out["shared"][k][w], 2) for w in ("encode_ms", "decode_ms")} for k in out["shared"]}
    if "packed" in out:  # > 1: the packed call is the faster one
        out["packed_vs_baseline"] = {k: {w: round(out["packed_baseline"][k][w] / out["packed"][k][w], 2) for w in ("encode_ms", "decode_ms")} for k in out["packed"]}
    if "gather" in out:  # > 1: the gather call is the faster one; identity_extra_ms: what the identity takes beyond a packed decode plus a sizes-only gather
        out["gather_vs_baseline"] = {k: {n: round(out["gather_baseline"][k][n]["ms"] / out["gather"][k][n]["ms"], 2) for n in SELECTIONS} for k in out["gather"]}
        out["gather_identity_extra_ms"] = {k: round(v["identity"]["ms"] - v["identity"]["packed_decode"]["ms"] - v["identity"]["sizes_only"]["ms"], 4) for k, v in out["gather"].items()}
    if "match" in out:  # > 1: the match call is the faster one
        out["match_vs_baseline"] = {k: {sel: {m: round(out["match_baseline"][k][sel][m]["ms"] / e[m]["ms"], 2) for m in ("prefix", "equal")} for sel, e in v.items()} for k, v in out["match"].items()}
    if "search" in out:  # > 1: the search is faster than the decode of the whole store, the first step of a search by decoding
        out["search_vs_decode"] = {k: {sel: {m: round(out["search_baseline"][k][sel]["decode"]["ms"] / e[m]["ms"], 2) for m in ("contains", "suffix")} for sel, e in v.items()}
                                   for k, v in out["search"].items()}
    if "order" in out:  # per shape and needle: the decode's time over LESS's (> 1: LESS is faster), whether the medians lie further apart than the two spreads together, LESS over the PREFIX floor
        out["order_vs_decode"] = {}
        for k, v in out["order"].items():
            dec, floor = out["order_baseline"][k]["decode"], v["prefix_floor"]
            out["order_vs_decode"][k] = {name: {"decode_over_less": round(dec["ms"] / e["ms"], 2),
                                                "beyond_both_spreads": dec["ms"] - e["ms"] > (dec["max_ms"] - dec["min_ms"]) + (e["max_ms"] - e["min_ms"]),
                                                "less_over_prefix_floor": round(e["ms"] / floor["ms"], 2)} for name, e in v.items() if isinstance(e, dict) and name != "prefix_floor"}
    if "join" in out:  # > 1: the join call is the faster one
        out["join_vs_baseline"] = {k: {keys: {sel: round(out["join_baseline"][k][keys][sel]["ms"] / e["ms"], 2) for sel, e in v.items()} for keys, v in shape.items()}
                                   for k, shape in out["join"].items()}
    if "take" in out:  # > 1: the take call is the faster one; vs_copy_floor (in the take leg): its time over a plain copy of as many bytes
        out["take_vs_baseline"] = {k: {n: round(out["take_baseline"][k][n]["ms"] / e["ms"], 2) for n, e in v.items() if isinstance(e, dict)} for k, v in out["take"].items()}
    if "slice" in out:  # per shape and case: the pair's time over the slice's (> 1: the slice is faster), and whether the medians lie further apart than the two spreads together
        out["slice_vs_baseline"] = {}
        for k, v in out["slice"].items():
            if not isinstance(v, dict):
                continue
            out["slice_vs_baseline"][k] = {}
            for name in SLICE_CASES:
                old, new = out["slice_baseline"][k][name], v[name]
                out["slice_vs_baseline"][k][name] = {"baseline_over_slice": round(old["ms"] / new["ms"], 2),
                                                     "beyond_both_spreads": old["ms"] - new["ms"] > (old["max_ms"] - old["min_ms"]) + (new["max_ms"] - new["min_ms"])}
        out["slice_condition_met"] = all(e["beyond_both_spreads"] for v in out["slice_vs_baseline"].values() for e in v.values())
    if "field" in out:  # per shape and case: the pair's time over the field call's (> 1: the field call is faster), and whether the medians lie further apart than the two spreads together
        out["field_vs_baseline"] = {}
        for k, v in out["field"].items():
            if not isinstance(v, dict):
                continue
            out["field_vs_baseline"][k] = {}
            for name, new in v.items():
                if not isinstance(new, dict):
                    continue
                old = out["field_baseline"][k][name]
                out["field_vs_baseline"][k][name] = {"baseline_over_field": round(old["ms"] / new["ms"], 2),
                                                     "beyond_both_spreads": old["ms"] - new["ms"] > (old["max_ms"] - old["min_ms"]) + (new["max_ms"] - new["min_ms"])}
        out["field_condition_met"] = all(e["beyond_both_spreads"] for v in out["field_vs_baseline"].values() for e in v.values())
    if "concat" in out:
        out["concat_condition_met"] = all(e["beyond_both_spreads"] for v in out["concat"].values() if isinstance(v, dict) for e in v.values() if isinstance(e, dict))
    if "recode" in out:
        out["recode_condition_met"] = all(e["beyond_both_spreads"] for v in out["recode"].values() if isinstance(v, dict) for e in v.values() if isinstance(e, dict))
    if "group" in out:
        out["group_condition_met"] = {k: {name: e["beyond_both_spreads"] for name, e in v.items()} for k, v in out["group"].items()}
    if "number" in out:
        out["number_verdicts"] = {k: {name: e["verdict"] for name, e in v.items() if isinstance(e, dict)} for k, v in out["number"].items() if isinstance(v, dict)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
