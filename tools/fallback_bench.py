"""The round-1 decode kernels (et_kernels_fallback.hip), which bench.py no longer reaches: decode_body_device with the context's
timing on, on the library named by ET_LIB_PATH (or entreepy_amd/libentreepy_hip.so), one process per run.

Four legs:
  sparse_256m   the sparse dictionary of tests/guards.py, the recipe of test_fallback_sweeps_and_write_are_what_a_sparse_dictionary_runs,
                256 MiB of text: k_dec_sync_reg2, k_dec_write_reg and the special launches beside them
  flat_256m     the hand-made table of 200 codes of 8 bits, 256 MiB: k_dec_maps_reg, the chains, k_dec_resolve_reg, k_dec_write_reg
  sparse_60k    the sparse recipe at 60 000 symbols: k_dec_sync_reg<true, true>, no superblocks
  sparse_3blk   the sparse recipe at a body of 3 * 8192 bytes: the LDS-window kernels alone -- a latency figure, call_ms is its number
Per leg: the decoded bytes checked against the text once, WARMUP untimed calls, then REPS timed ones; every figure is the median
over them (min and max beside the total).  total_ms and the phases are timings("decode")'s; call_ms is the host's clock round the
call and the wait for its last kernel.  One JSON line on stdout (and appended to --out).

    python tools/fallback_bench.py --label new --out profiles/fallback_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 20, 3
PHASES = ("host_ms", "sync_ms", "scan_ms", "body_ms")


def _sparse_case(n, seed, body_bytes=None):
    """-> (code table, packed body, text): n symbols of the sparse recipe, or (body_bytes) their first prefix that packs to that many."""
    import numpy as np

    from oracle import oracle as O
    from tests.guards import _sparse_dictionary

    data_t, len_t, syms = _sparse_dictionary()
    rng = np.random.default_rng(seed)
    text = syms[np.minimum(rng.integers(0, 300, size=n), syms.size - 1) % syms.size].astype(np.uint8)
    text[rng.random(n) < 0.5] = 32
    if body_bytes is not None:
        text = text[: int(np.searchsorted(np.cumsum(len_t[text].astype(np.int64)), 8 * body_bytes - 7)) + 1]
    body, _ = O.pack_body(data_t, len_t, text)
    return (data_t, len_t), np.frombuffer(body, dtype=np.uint8).copy(), text


def _flat_case(n, seed):
    import numpy as np

    data_t, len_t = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    data_t[:200], len_t[:200] = np.arange(200), 8
    text = np.random.default_rng(seed).integers(0, 200, size=n, dtype=np.uint8)
    return (data_t, len_t), text, text  # (the code of symbol s is the byte s)


LEGS = {
    "sparse_256m": lambda: _sparse_case(256 << 20, 256),
    "flat_256m": lambda: _flat_case(256 << 20, 256),
    "sparse_60k": lambda: _sparse_case(60_000, 60_000),
    "sparse_3blk": lambda: _sparse_case(400_000, 17, 3 * 8192),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch

    import entreepy_amd as E

    ctx = E.Context(0)
    out = {"tool": "fallback_bench", "label": a.label, "lib": os.environ.get("ET_LIB_PATH", ""), "reps": REPS, "warmup": WARMUP}
    for leg in a.legs.split(","):
        (data_t, len_t), body, text = LEGS[leg]()
        cb = E.Codebook.from_tables(data_t, len_t)
        d_body = torch.from_numpy(body).cuda()
        d_text = torch.from_numpy(text).cuda()
        dec = torch.empty(text.size + 64, dtype=torch.uint8, device="cuda")
        ctx.enable_timing(True)
        assert ctx.decode_body_device(cb, d_body, text.size, dec) == text.size
        tm = ctx.timings("decode")
        assert torch.equal(dec[: text.size], d_text), "decoded bytes differ from the text"
        runs = []
        for rep in range(WARMUP + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.decode_body_device(cb, d_body, text.size, dec)
            torch.cuda.synchronize()
            call_ms = (time.perf_counter() - t0) * 1e3
            if rep >= WARMUP:
                runs.append(dict(ctx.timings("decode"), call_ms=call_ms))
        ctx.enable_timing(False)
        totals = [r["total_ms"] for r in runs]
        out[leg] = {
            "symbols": int(text.size), "body_bytes": int(body.size), "exhaustive_sync": tm["exhaustive_sync"], "chained_write": tm["chained_write"],
            "sync_iters": tm["sync_iters"], "total_ms": round(statistics.median(totals), 4), "total_min_ms": round(min(totals), 4), "total_max_ms": round(max(totals), 4),
            "call_ms": round(statistics.median(r["call_ms"] for r in runs), 4), **{p: round(statistics.median(r[p] for r in runs), 4) for p in PHASES},
        }
        del d_body, d_text, dec
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
