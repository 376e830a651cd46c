#!/usr/bin/env python3
"""bench.py -- the hot path's headline metric on MI355X.

A "step" is one pass of the hot path over one batch: encode the rank's text stream
to a .et image (K1 histogram -> host code construction -> K2 scan -> K4 scatter) and
decode that image back (header to the host -> tables -> D1 synchronisation by tree walk -> D2
scan -> D3 write over chained tables), inputs resident in HBM.  Workload at N=1 (BASELINE.json metric): "text-1G", 2^30 bytes of order-0
samples of res/a_midsummer_nights_dream.txt's byte distribution (no benchmark corpus
exists offline).  N>1: every rank holds its own 2^30-byte shard of one
N-GiB stream (weak scaling); the shards share one code table through an RCCL
all-gather of the local histograms and land at their global bit offsets.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

Invoked plainly with --gpus N > 1 (no WORLD_SIZE in the environment) it starts the N ranks itself -- torch.distributed.run
as a CHILD process, before this process has imported torch or touched a GPU -- relays rank 0's line and exits with the
children's status.  Prints ONE JSON line on rank 0.

A plain run measures the headline alone: set-up, W warm-up steps, SETTLE_STEPS more untimed ones, K timed steps, the line.
--full adds everything else the line has carried: the as-asked region right behind the warm-up (value_cold), the instrumented
steps behind phase_ms / kernels / roofline, at N = 1 the extra workloads and the CPU baselines, at N > 1 the concatenation,
the one-GPU comparison step and the cold sharded decode.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
SETTLE_STEPS = 200       # untimed steps between the warm-up (--full: the as-asked value_cold region) and the steady-state region (value); see main
HBM_COPY_GBPS = 6290.0  # same guide: what a float4 copy reaches (report against both, headline against spec)


def cpu_baseline(sample_u8, what, budget_s=14.0):
    """Oracle (kind "port": the Zig reference cannot be built here) on one host core,
    on a prefix of the same stream sized to ~budget_s of CPU work."""
    from oracle import oracle as O

    probe = sample_u8[: 4 << 20]
    t = time.perf_counter()
    et = O.encode(probe)
    O.decode(et[4:])
    per_byte = (time.perf_counter() - t) / probe.size
    n = int(min(sample_u8.size, max(probe.size, budget_s / per_byte)))
    n -= n % 4096
    data = sample_u8[:n]
    t0 = time.perf_counter()
    et = O.encode(data)
    t1 = time.perf_counter()
    back = O.decode(et[4:])
    t2 = time.perf_counter()
    assert back == data.tobytes()
    return {
        "value": round(n / (t2 - t0) / 1e9, 5),
        "unit": "GB/s",
        "cores": 1,
        "kind": "port",
        "sample": f"first {n >> 20} MiB of rank 0's {what} stream, oracle encode+decode round trip "
                  f"(encode {n / (t1 - t0) / 1e6:.1f} MB/s, decode {n / (t2 - t1) / 1e6:.1f} MB/s), 1 thread",
    }


def cpu_baseline_parallel(sample_u8, what, threads, budget_s=8.0):
    """SURVEY.md 8d's second CPU figure: the fast chunk-parallel CPU variant
    (oracle/et_cpu_fast.c, one chunk per thread).  Default thread count: this process's
    CPU share of the GPU box (16 host cores per GPU on the pool), not the whole host."""
    from oracle import cpu_fast as F

    cores = threads or min(len(os.sched_getaffinity(0)), 16)
    probe = sample_u8[: 32 << 20]
    t = time.perf_counter()
    F.decode(F.encode(probe, cores)[4:], cores)
    per_byte = (time.perf_counter() - t) / probe.size
    n = int(min(sample_u8.size, max(probe.size, budget_s / per_byte)))
    n -= n % 4096
    data = sample_u8[:n]
    t0 = time.perf_counter()
    et = F.encode(data, cores)
    t1 = time.perf_counter()
    back = F.decode(et[4:], cores)
    t2 = time.perf_counter()
    assert back == data.tobytes()
    return {
        "value": round(n / (t2 - t0) / 1e9, 4),
        "unit": "GB/s",
        "cores": cores,
        "kind": "port-fast",
        "sample": f"first {n >> 20} MiB of rank 0's {what} stream, chunk-parallel lookup-table CPU variant, encode+decode "
                  f"round trip (encode {n / (t1 - t0) / 1e6:.0f} MB/s, decode {n / (t2 - t1) / 1e6:.0f} MB/s), {cores} threads",
    }


def load_pmc_traffic(kernel, bytes_per_gpu):
    """(HBM bytes per launch, where the figure comes from) from the committed rocprofv3 --pmc passes
    (profiles/pmc_latest.json: FETCH_SIZE x 2 + WRITE_SIZE, separate passes of this same command on another box) -- NOT
    measured by the run that prints the line -- or (None, why) when there are none or they were taken at another size."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_latest.json")) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None, "no profiles/pmc_latest.json"
    meta = d.get("_meta", {})
    if meta.get("bytes_per_gpu", 1 << 30) != bytes_per_gpu:
        return None, f"profiles/pmc_latest.json was collected at {meta.get('bytes_per_gpu', 1 << 30)} B per GPU, this run has {bytes_per_gpu}"
    v = d.get(kernel, {}).get("hbm_bytes_per_launch")
    return v, f"profiles/pmc_latest.json (tag {meta.get('tag', 'r03')}; rocprofv3 --pmc passes of this command, not this run)"


DUMP_SAMPLE = 1 << 22   # values per dumped array: two float32 arrays of 16 MiB, under the 64 MB a dump may take
DUMP_SEED = 0x5EED0D0D


def dump_positions(length):
    """Where an array of `length` values is sampled for --dump-outputs: the first 4096 (the .et header and dictionary) and
    DUMP_SAMPLE - 4096 seeded draws, sorted -- a function of the length alone, so two builds are compared position for position."""
    import numpy as np

    if length <= DUMP_SAMPLE:
        return np.arange(length, dtype=np.int64)
    head = np.arange(4096, dtype=np.int64)
    rest = np.sort(np.random.default_rng(DUMP_SEED).integers(4096, length, DUMP_SAMPLE - 4096, dtype=np.int64))
    return np.concatenate([head, rest])


def dump_outputs(directory, torch, image, decoded, n):
    """What the last timed step handed its caller, as float32 .npy files: `encoded` (the .et image, or this rank's part
    of it), `decoded` (the text decoded back), each sampled at dump_positions(); `sizes` (float64: input bytes, image
    bytes, decoded symbols)."""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    for name, t in (("encoded", image), ("decoded", decoded)):
        pos = torch.from_numpy(dump_positions(t.numel())).to(t.device)
        np.save(os.path.join(directory, name + ".npy"), t[pos].cpu().numpy().astype(np.float32))
    np.save(os.path.join(directory, "sizes.npy"), np.array([n, image.numel(), decoded.numel()], dtype=np.float64))


def fail(msg):
    """A failed check ends the run without a line (not an assert: python -O strips those)."""
    sys.stderr.write(f"bench.py: {msg}\n")
    sys.stderr.flush()
    sys.exit(3)


def uniform_bytes_torch(n, lo, hi, seed, dev):
    """n uniform bytes in [lo, hi), generated on the device (BASELINE config 5: 16 GiB does not cross PCIe quickly)."""
    import torch

    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    step = 1 << 28
    for s in range(0, n, step):
        m = min(step, n - s)
        out[s : s + m] = torch.randint(lo, hi, (m,), generator=g, device=dev, dtype=torch.int16).to(torch.uint8)
    return out


def measure_stream(torch, ctx, pipe, text, enc, dec, reps, lead, decode=True, verify=True):
    """`lead` untimed + `reps` measured steps (encode to .et, cold decode back) of one HBM-resident stream, every phase carrying
    HIP events (ctx.enable_timing(True)).  -> dict: n, packed_bytes, GB/s figures, phase_ms, which decode kernels ran.
    decode=False: the stream has no inverse (all 256 byte values: the reference drops a symbol) -- encode only."""
    n = text.numel()
    ph = {"hist": 0.0, "enc_scan": 0.0, "enc_body": 0.0, "enc_total": 0.0, "dec_sync": 0.0, "dec_sync_first": 0.0, "dec_scan": 0.0, "dec_body": 0.0, "dec_total": 0.0}
    m = n
    td = None
    # 1. the step as a caller pays it: no events, nothing read back between steps (host clock over `reps` steps)
    torch.cuda.synchronize()
    ctx.enable_timing(False)
    for i in range(reps + lead):
        if i == lead:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        r = pipe.encode_shard(text, enc, timings=False)
        if decode:
            m = pipe.decode_shard(enc, r, dec)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps * 1e3
    # 2. the same steps with every phase carrying HIP events, read back after every step -> phase_ms
    ctx.enable_timing(True)
    for i in range(reps + 4):
        r = pipe.encode_shard(text, enc, timings=False)
        if decode:
            m = pipe.decode_shard(enc, r, dec)
        te = pipe.encode_timings()
        if decode:
            td = ctx.timings("decode")
        if i >= 4:
            for k in ("hist", "enc_scan", "enc_body", "enc_total"):
                ph[k] += te[k]
            if decode:
                ph["dec_sync"] += td["sync_ms"]
                ph["dec_sync_first"] += td["sync_first_ms"]
                ph["dec_scan"] += td["scan_ms"]
                ph["dec_body"] += td["body_ms"]
                ph["dec_total"] += td["total_ms"]
    torch.cuda.synchronize()
    ok = None
    if verify and decode:
        ok = bool(m == n and torch.equal(dec[:n], text))
        if not ok:
            fail("round trip of an extra workload is not the identity")
    cb = ctx.last_codebook()
    p = {k: v / reps for k, v in ph.items()}
    packed = r["body_bytes"]
    out = {
        "bytes": n, "packed_bytes": packed, "symbols": int(cb.raw.n_coded), "code_lengths": [int(cb.raw.min_length), int(cb.raw.max_length)],
        "steps": reps, "lead_steps": lead,
        "ms_per_step": round(wall, 4),  # host clock over `steps` uninstrumented steps behind `lead_steps` untimed ones
        ("round_trip_GBps" if decode else "encode_only_GBps"): round(n / (wall * 1e-3) / 1e9, 2),  # n / ms_per_step
        "encode_GBps": round(n / (p["enc_total"] * 1e-3) / 1e9, 2),
        "encode_hbm_frac": round((2 * n + packed) / ((p["hist"] + p["enc_scan"] + p["enc_body"]) * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
        "phase_ms": {k: round(v, 4) for k, v in p.items() if decode or not k.startswith("dec_")},
    }
    if decode:
        out["decode_GBps"] = round(n / (p["dec_total"] * 1e-3) / 1e9, 2)
        out["decode_hbm_frac"] = round((n + packed) / (p["dec_total"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
        out["kernels_only_round_trip_GBps"] = round(n / ((p["enc_total"] + p["dec_total"]) * 1e-3) / 1e9, 2)  # n / (enc_total + dec_total): begin of K1 .. end of K4 plus begin of D1 .. end of D3, instrumented steps
        if td.get("row_sync"):
            out["decode_path"] = "k_row_sync + k_row_write" if os.environ.get("ET_NO_ROW_WRITE") != "1" else "k_row_sync + k_dec_write_wave"
        elif td.get("fixed_sync"):
            out["decode_path"] = "k_fixed_write" if os.environ.get("ET_NO_FIXED_WRITE") != "1" else "k_fixed_sync + k_dec_write_wave"
        else:
            out["decode_path"] = ("exhaustive maps (k_dec_maps_reg / k_dec_compose / k_dec_chain / k_dec_resolve_reg)" if td["exhaustive_sync"]
                                  else ("k_tw_sync" if td["tree_walk_sync"] else "k_dec_sync_reg2")) + " + " + ("k_dec_write_wave" if td["chained_write"] else "k_dec_write_reg")
        out["verified"] = ok
    return out


EXTRA_WORKLOADS = ("enwik-like", "text-100M", "text-5M", "flat4-1G", "flat10-1G", "flat26-1G", "zeros97-1G", "uniform255-4G", "uniform256-16G")


def run_extra_workload(name, torch, E, corpus, ctx, pipe, dev, n_headline, verify=True, reps=None):
    """One of BASELINE.json's other configurations (or the enwik-like stream) at N = 1, beside the headline: -> dict."""
    free, _ = torch.cuda.mem_get_info(dev)
    if name == "enwik-like":
        n = n_headline
        text = corpus.enwik_like_torch(n, 0x5EED0009, dev)
        what = f"enwik-like: {n} B, 206 symbols (96 Zipf-like + 110 with probabilities 2^-12 .. 2^-24), seed 0x5EED0009"
        reps, lead, decode = reps or 10, 30, True
    elif name == "text-100M":  # BASELINE configs[2] (enwik8's size; the corpus does not exist offline)
        n = 100_000_000
        real = corpus.from_env("ET_CORPUS_ENWIK8", n)
        text = torch.from_numpy(real).to(dev) if real is not None else corpus.text_like_torch(n, 0x5EED0003, dev)
        n = text.numel()
        what = f"text-100M: {n} B, " + ("enwik8 ($ET_CORPUS_ENWIK8)" if real is not None else "order-0 samples of Midsummer's byte distribution, seed 0x5EED0003") + " (BASELINE configs[2])"
        reps, lead, decode = reps or 40, 60, True
    elif name == "text-5M":  # BASELINE configs[1] (the Complete Works' size)
        n = 5_458_199
        real = corpus.from_env("ET_CORPUS_SHAKESPEARE")
        host = real if real is not None else corpus.tiled_midsummer(n)
        text = torch.from_numpy(host).to(dev)
        n = text.numel()
        what = f"text-5M: {n} B, " + ("$ET_CORPUS_SHAKESPEARE" if real is not None else "a_midsummer_nights_dream.txt tiled") + " (BASELINE configs[1])"
        reps, lead, decode = reps or 100, 100, True
    elif name == "uniform255-4G":  # BASELINE configs[4]'s decode half: the largest lossless stream of the format
        n = (4 << 30) - (1 << 20)
        if free < 3 * n + (3 << 30):
            return {"skipped": f"needs ~{(3 * n) >> 30} GiB of free HBM, {free >> 30} GiB are free"}
        text = uniform_bytes_torch(n, 1, 256, 0x5EED0055, dev)
        what = (f"uniform255-4G: {n} B uniform over byte values 1..255, seed 0x5EED0055 (BASELINE configs[4] where the format is lossless: 255 symbols, "
                f"just under 4 GiB -- the reference drops one of 256 symbols, Q1, and wraps the length at 4 GiB, Q4); codes of 7-8 bits do not self-synchronise")
        reps, lead, decode = reps or 5, 3, True
    elif name == "uniform256-16G":  # BASELINE configs[4], encode
        n = 16 << 30
        if free < 2 * n + (4 << 30):
            return {"skipped": f"needs ~{(2 * n) >> 30} GiB of free HBM, {free >> 30} GiB are free"}
        text = uniform_bytes_torch(n, 0, 256, 0x5EED0005, dev)
        what = (f"uniform256-16G: {n} B uniform over all 256 byte values, seed 0x5EED0005 (BASELINE configs[4]), encode only: with 256 distinct "
                f"values the reference's encoder drops a symbol (Q1) and the stream has no inverse")
        reps, lead, decode = reps or 5, 2, False
    elif name in ("flat4-1G", "flat10-1G", "flat26-1G"):  # not BASELINE configurations: the small flat alphabets next to its worst case (DNA-, digit-, letter-like)
        k = int(name[4 : name.index("-")])
        n = n_headline
        text = uniform_bytes_torch(n, 48, 48 + k, 0x5EED0F00 + k, dev)
        what = (f"{name}: {n} B uniform over {k} byte values, seed {0x5EED0F00 + k:#x} (not a BASELINE configuration: the small flat alphabets beside configs[4]); "
                + ("2-bit codewords only: decoded by arithmetic, no synchronisation" if k == 4 else "codes of two neighbouring lengths that settle quickly: the tree walk"))
        reps, lead, decode = reps or 10, 10, True
    elif name == "zeros97-1G":  # not a BASELINE configuration: a stream with one dominant value (a 1-bit codeword, ~200 symbols per 256-bit subsequence)
        n = n_headline
        text = uniform_bytes_torch(n, 1, 255, 0x5EED0097, dev)
        g = torch.Generator(device=dev)
        g.manual_seed(0x5EED0097)
        step = 1 << 26
        for s0 in range(0, n, step):
            m = min(step, n - s0)
            text[s0 : s0 + m][torch.rand(m, generator=g, device=dev) < 0.97] = 0
        what = (f"zeros97-1G: {n} B, 97 % zero bytes, the rest uniform over 254 other values, seed 0x5EED0097 (not a BASELINE configuration: "
                "~200 symbols per 256-bit subsequence -- the write pass's instantiation that walks a quarter once, into strips)")
        reps, lead, decode = reps or 10, 10, True
    else:
        return {"error": f"unknown workload {name}"}
    n = text.numel()
    ctx.reserve(n)
    enc = torch.zeros(E.encode_bound(n) + 64, dtype=torch.uint8, device=dev)
    dec = torch.empty(n + 64, dtype=torch.uint8, device=dev) if decode else None
    out = {"workload": what}
    out.update(measure_stream(torch, ctx, pipe, text, enc, dec, reps, lead, decode, verify))
    return out


def main():
    # Libraries chat on stdout (RCCL prints a version banner at communicator creation):
    # keep the real stdout for the ONE JSON line and send everything else to stderr.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bytes", type=int, default=int(os.environ.get("ET_BENCH_BYTES", 1 << 30)), help="text bytes per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the chunk-parallel CPU baseline (0: min(cores, 16))")
    ap.add_argument("--no-second-workload", "--no-extra-workloads", dest="no_second_workload", action="store_true",
                    help="skip the streams measured after the headline at N=1 (enwik-like and BASELINE's other configurations)")
    ap.add_argument("--workloads", default=os.environ.get("ET_BENCH_WORKLOADS", ",".join(EXTRA_WORKLOADS)),
                    help="which of them, comma-separated: " + ", ".join(EXTRA_WORKLOADS))
    ap.add_argument("--ref-value", type=float, default=None, help="the 1-GPU value (GB/s) a N > 1 line's scaling_efficiency is computed against (default: value_n1_same_step, measured in the same run)")
    ap.add_argument("--decode", choices=("cold", "shard"), default="cold",
                    help="N = 1 only: 'shard' decodes the image the way the ranks of an N > 1 step decode their shards (the encode's code table and "
                         "start bit, no header hand-over) -- the N = 1 step an N > 1 value is comparable with; the headline is 'cold'")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline too: value_cold, phase / kernel / roofline figures, at N = 1 the extra "
                         "workloads and CPU baselines (--no-extra-workloads / --no-cpu-baseline leave them out), at N > 1 the "
                         "concatenation, the one-GPU comparison step and the cold sharded decode")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rank 0's image and decoded text, sampled) as DIR/<name>.npy")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # Launch the ranks: a child process per GPU through torch.distributed.run.  Nothing here has imported torch or
        # initialised a GPU (a process that has must never be replaced by another program on this pool; a child is fine).
        import socket
        import subprocess

        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.abspath(__file__)] + sys.argv[1:]
        child = subprocess.run(cmd, stdout=subprocess.PIPE, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))
        lines = [ln for ln in child.stdout.decode("utf-8", "replace").splitlines() if ln.startswith("{") and '"metric"' in ln]
        if lines:
            os.write(real_stdout, (lines[-1] + "\n").encode())
        sys.exit(child.returncode if child.returncode or lines else 1)

    import torch
    import torch.distributed as dist

    import entreepy_amd as E
    from entreepy_amd import _native as N
    from entreepy_amd import sharded
    from tests import corpus

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run"
    # ET_BENCH_DEVICE / ET_DIST_BACKEND exist only to rehearse the N > 1 flow on a
    # one-GPU box (all ranks on cuda:0 over gloo); the driver's runs use neither.
    local = int(os.environ.get("ET_BENCH_DEVICE", local))
    backend = os.environ.get("ET_DIST_BACKEND", "nccl")
    if local >= torch.cuda.device_count():
        sys.exit(f"bench.py: rank {rank} wants cuda:{local} but the node shows {torch.cuda.device_count()} GPU(s) "
                 "(ET_BENCH_DEVICE=0 ET_DIST_BACKEND=gloo rehearses N ranks on one GPU)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    force_group = world == 1 and os.environ.get("ET_BENCH_FORCE_GROUP") == "1"  # rehearsal: N>1 code path at N=1
    if force_group:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    n = args.bytes
    # The metric's stream: a real corpus when the environment names one ($ET_CORPUS_ENWIK9, BASELINE config 4;
    # rank r takes the r-th n-byte slice), else the synthetic text-1G.
    real = corpus.from_env("ET_CORPUS_ENWIK9")
    if real is not None and real.size >= (rank + 1) * min(n, real.size // world):
        n = min(n, real.size // world)
        text = torch.from_numpy(real[rank * n : (rank + 1) * n].copy()).to(dev)
        workload_name = f"enwik9 from $ET_CORPUS_ENWIK9: {n} B per GPU"
        real_sample = real[rank * n : rank * n + min(n, 1 << 30)].copy()  # (the CPU baselines' sample, below)
    else:
        real_sample = None
        text = corpus.text_like_torch(n, 0x5EED0004 + rank, dev)
        workload_name = (f"text-1G: {n} B per GPU, order-0 samples of a_midsummer_nights_dream.txt's byte distribution, "
                         f"seed 0x5EED0004+rank")  # (no parentheses: the driver's parser cuts config.workload at the first one)
    del real
    ctx = E.Context(local)
    ctx.use_torch_stream()
    ctx.reserve(n)
    ctx.enable_timing(True)  # (every phase, for the instrumented steps; the timed regions switch to the write kernel's pair alone, see main)
    enc = torch.zeros(E.encode_bound(n) + 64, dtype=torch.uint8, device=dev)
    dec = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    pipe = sharded.ShardedCodec(ctx, dist.group.WORLD if (world > 1 or force_group) else None, dev)

    n1_as_shard = world == 1 and not force_group and args.decode == "shard"
    phases = {"hist": 0.0, "enc_host": 0.0, "enc_scan": 0.0, "enc_body": 0.0, "dec_sync": 0.0, "dec_sync_first": 0.0, "dec_scan": 0.0, "dec_body": 0.0,
              "enc_total": 0.0, "dec_total": 0.0, "sync_launches": 0, "exchange": 0.0}
    state = {}

    def add_decode_timings():
        t = ctx.timings("decode")
        phases["dec_sync"] += t["sync_ms"]
        phases["dec_sync_first"] += t["sync_first_ms"]
        phases["dec_scan"] += t["scan_ms"]
        phases["dec_body"] += t["body_ms"]
        phases["dec_total"] += t["total_ms"]
        phases["sync_launches"] += t["sync_iters"]
        state["sync_kernel"] = "k_tw_sync" if t["tree_walk_sync"] else "k_dec_sync_reg2"
        state["write_kernel"] = "k_dec_write_wave" if t["chained_write"] else "k_dec_write_reg"

    # The HIP events of every call are recorded inside the timed region; their elapsed
    # times are READ where reading cannot stall the stream: the decode's after the next
    # step's encode has been handed over (its histogram read-back waits for everything
    # before it anyway), the encode's after the decode that follows it.
    def step(record, first):
        r = pipe.encode_shard(text, enc, timings=False)
        if record and not first:
            add_decode_timings()  # of the step before
        m = pipe.decode_shard(enc, r, dec, as_shard=n1_as_shard)
        if record and state["all_phases"]:
            te = pipe.encode_timings()
            for k in ("hist", "enc_host", "enc_scan", "enc_body", "enc_total", "exchange"):
                phases[k] += te[k]
        state["layout"] = r
        state["decoded"] = m

    def timing_mode(all_phases):
        """all_phases: the four large kernels and the phases between them carry HIP events (the instrumented steps); else the
        decode's write kernel alone -- the dominant kernel, whose events the roofline needs INSIDE the timed region.  A dispatch that
        carries events costs ~5 us of queue time on either side (rocprofv3 timeline: 4.8 us gaps around K1, K4, D1, D3 against 0
        between two plain dispatches): ~35 us of a 1.39 ms step that no production call pays."""
        all_phases = all_phases or os.environ.get("ET_BENCH_TIME_ALL") == "1"  # (A/B switch: every phase timed in the timed regions too, as before round 3)
        torch.cuda.synchronize()
        ctx.enable_timing(True if all_phases else ctx.TIMING_DECODE_BODY)
        state["all_phases"] = all_phases

    def zero_phases():
        for k in phases:
            phases[k] = 0.0 if isinstance(phases[k], float) else 0

    def barrier():
        if world > 1:
            dist.barrier(device_ids=[local]) if backend == "nccl" else dist.barrier()

    def timed_region():
        """EXACTLY K steps between barrier + synchronize on both sides; the MAX over ranks."""
        zero_phases()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(True, i == 0)
        torch.cuda.synchronize()
        barrier()
        dt = time.perf_counter() - t0
        add_decode_timings()  # the last step's
        if world > 1:
            tmax = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax.item())
        return dt

    # The round trip is verified once; then, AS ASKED: W warm-up steps and K timed steps -> value_cold.  Then the same K
    # steps again behind SETTLE_STEPS more untimed ones -> value: a step hands over to the host twice (the histogram for
    # the code construction, the header for the decode's tables) and the host answers in ~20 us once its clocks and caches
    # are up -- on a box that has just been leased the first hundred steps see 2-3 x that -- and the GPU's clocks take ~15
    # steps to come back after an idle stretch such as the verification's 0.1 s (the write kernel: 0.59 ms falling to 0.49,
    # rocprofv3 trace).  Both figures are in the line; `value` is the steady state, value_cold the run as the contract
    # words it (same code, same K, only the number of untimed steps before it differs).
    # A plain run (no --full) leaves out the value_cold region and the instrumented steps: W warm-up steps, SETTLE_STEPS untimed
    # ones, the K timed steps of `value`.
    # (the harness's own comparison kernels are loaded before the pipeline first runs: the verification below then costs a
    # fraction of a millisecond instead of ~0.1 s of module loading with the GPU idle and its clocks falling)
    torch.equal(dec[:n], text)
    timing_mode(all_phases=False)
    for _ in range(2):
        step(False, True)
    torch.cuda.synchronize()
    verify = os.environ.get("ET_BENCH_NO_VERIFY") != "1"  # (timing probes: builds whose kernels give wrong results on purpose; the line then says "verified": false and carries value_unverified instead of value)
    if verify and not (state["decoded"] == n and torch.equal(dec[:n], text)):
        fail("round trip is not the identity")
    for _ in range(args.warmup):
        step(False, True)
    if args.full:
        elapsed_cold = timed_region()
        # the untimed set-up steps: the last K of them carry every phase's events -> phase_ms and the four kernels' figures
        for _ in range(max(SETTLE_STEPS - args.steps - 8, 0)):
            step(False, True)
        timing_mode(all_phases=True)
        for _ in range(4):
            step(False, True)
        zero_phases()
        for i in range(args.steps):
            step(True, i == 0)
        torch.cuda.synchronize()
        add_decode_timings()
        instrumented = dict(phases)
        timing_mode(all_phases=False)
        for _ in range(4):
            step(False, True)
    else:
        for _ in range(SETTLE_STEPS):  # (the untimed set-up steps alone: `value` is the same steady state as --full's)
            step(False, True)
    elapsed = timed_region()
    body_ms_timed = phases["dec_body"] / args.steps  # the write kernel's own events, every step of the timed region
    m_bytes = state["layout"]["body_bytes"]  # packed body bytes of this rank's shard (worked out here, off the timed path)
    if verify and not (state["decoded"] == n and torch.equal(dec[:n], text)):
        fail("round trip of the last timed step is not the identity")
    if args.dump_outputs and rank == 0:
        r = state["layout"]
        image = enc[: r["et_len"]] if r["single"] else enc[: (r["end_bit"] + 7) // 8]
        dump_outputs(args.dump_outputs, torch, image, dec[: state["decoded"]], n)
    if args.full:
        timing_mode(all_phases=True)  # (the second workload below reports its phases)

    # N > 1: the bit-offset-adjusted concatenation of the shards into ONE image on rank 0 (seam merge + owned
    # words over xGMI), timed on its own after the headline region -- it is not part of `value`.
    concat_ms = seam_ms = None
    if world > 1 and args.full:
        best = None
        for _ in range(3):
            r = pipe.encode_shard(text, enc, timings=False)
            torch.cuda.synchronize()
            barrier()
            tc0 = time.perf_counter()
            image = pipe.concat_on_rank0(enc, r)
            torch.cuda.synchronize()
            barrier()
            dt = (time.perf_counter() - tc0) * 1e3
            best = dt if best is None else min(best, dt)
            del image
        tmax = torch.tensor([best], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        concat_ms = float(tmax.item())
        seam_ms = pipe.lib_group.info()["seam_ms"] if pipe.lib_group is not None else None

    # N > 1: what the N-GPU value is to be held against, measured in THIS run: every rank alone on its own shard (no group, no
    # exchange), the same step -- encode, then the body decoded with the encode's code table -- all ranks at once (each GPU as
    # busy as in the N-GPU step), K steps between barriers, the max over ranks.  scaling_efficiency = value / (N x this).
    n1_same_ms = cold_sharded_ms = None
    if (world > 1 or force_group) and args.full:
        solo = sharded.ShardedCodec(ctx, None, dev)
        torch.cuda.synchronize()
        ctx.enable_timing(False)

        def solo_step():
            r1 = solo.encode_shard(text, enc, timings=False)
            return solo.decode_shard(enc, r1, dec, as_shard=True)

        for _ in range(max(args.warmup, 10)):
            solo_step()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m1 = solo_step()
        torch.cuda.synchronize()
        barrier()
        dt = time.perf_counter() - t0
        if verify and not (m1 == n and torch.equal(dec[:n], text)):
            fail("round trip of the one-GPU comparison step is not the identity")
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        if world > 1:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        n1_same_ms = float(tmax.item()) / args.steps * 1e3
        # ... and the COLD decode of the whole image by the N ranks (et_decode_sharded: every rank synchronises its range of
        # 8 KiB blocks, one exchange of (start, exit, symbols) rows, repairs if a rank began wrong, writes its share): rank 0's
        # concatenated image goes to every rank first (not timed), then best of 3 between barriers.
        try:
            if os.environ.get("ET_BENCH_NO_COLD_SHARDED") == "1":
                raise RuntimeError("skipped (ET_BENCH_NO_COLD_SHARDED=1)")
            if pipe.lib_group is not None:
                pipe.lib_group.set_timeout_ms(30_000)  # (beside the headline: an exchange a peer never joins ends in 30 s with an error on every rank, not in 10 minutes)
            r = pipe.encode_shard(text, enc, timings=False)
            image = pipe.concat_on_rank0(enc, r)
            file_bytes = (r["starts"][-1] + 7) // 8 if not r["single"] else r["et_len"]
            whole = torch.empty((file_bytes + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
            if rank == 0:
                whole[:file_bytes] = image[:file_bytes]
            if world > 1:
                if backend == "nccl":
                    dist.broadcast(whole, src=0)
                else:
                    host_img = whole.cpu()
                    dist.broadcast(host_img, src=0)
                    whole.copy_(host_img)
            dec_cold = torch.empty(int(n * 1.02) + 16384, dtype=torch.uint8, device=dev)  # (a rank's share follows the 8 KiB blocks of the packed stream, not the text)
            best = None
            for _ in range(3):
                torch.cuda.synchronize()
                barrier()
                tc0 = time.perf_counter()
                got, first = pipe.decode_cold(whole[4:file_bytes], dec_cold)
                torch.cuda.synchronize()
                barrier()
                dtc = (time.perf_counter() - tc0) * 1e3
                best = dtc if best is None else min(best, dtc)
            tmax = torch.tensor([best], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            if world > 1:
                dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            cold_sharded_ms = float(tmax.item())
            del whole, image, dec_cold
        except Exception as e:  # noqa: BLE001 -- beside the headline: reported in its place
            cold_sharded_ms = repr(e)
            torch.cuda.synchronize()
        ctx.enable_timing(True)

    # N = 1: the other streams -- enwik-like (206 symbols, code lengths up to 24: the long codes the text stream never shows) and
    # BASELINE.json's other configurations (5.4 MB and 10^8 B of text, 4 GiB of 255 uniform byte values through the exhaustive
    # decode, 16 GiB of 256 for the encode) -- same step, a few repetitions each, reported beside the headline, never instead of it.
    extras = None
    if world == 1 and not force_group and not args.no_second_workload and args.full:
        extras = {}
        del text, enc, dec
        text = None
        for name in [w for w in args.workloads.split(",") if w]:
            torch.cuda.empty_cache()
            try:  # (beside the headline: whatever goes wrong here is reported in its place and does not cost the line)
                extras[name] = run_extra_workload(name, torch, E, corpus, ctx, pipe, dev, n, verify)
            except SystemExit:
                raise
            except Exception as e:  # noqa: BLE001
                extras[name] = {"error": repr(e)}
                torch.cuda.synchronize()
        torch.cuda.empty_cache()

    if rank == 0:
        K = args.steps
        out = {
            "metric": "GB/s encode+decode on 1 GiB text at 1/2/4/8 MI355X; % of HBM read peak",
            ("value" if verify else "value_unverified"): round(world * n / elapsed * K / 1e9, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": K,
            "warmup": args.warmup,
            "setup_steps": SETTLE_STEPS,  # untimed steps between the warm-up (--full: the value_cold region) and the `value` region (host clocks and caches; see main)
            "ms_per_step": round(elapsed / K * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic" if real_sample is None else "enwik9 ($ET_CORPUS_ENWIK9)",
            "verified": bool(verify),  # both round trips (before the warm-up, after the last timed step) compared with the input on the device
            "library": N.LIB_PATH,     # the shared object the step ran in ($ET_LIB_PATH swaps in another build)
            "config": {
                "workload": workload_name + ", one step = encode to .et + decode back, HBM-resident",
                "bytes_per_gpu": n,
                "packed_bytes_per_gpu": m_bytes,
                "sharding": "1 stream" if world == 1 else f"{world} contiguous shards of one stream, one RCCL all-gather of the local histograms per step (sum = global histogram, rows = shard bit counts)",
                "value_definition": "text bytes taken through encode+decode per second, all GPUs",
                "decode": pipe.DECODE_SHARD if (world > 1 or force_group or n1_as_shard) else pipe.DECODE_SINGLE,
            },
        }
        if args.full:
            ms = {k: v / K for k, v in instrumented.items()}  # per step, over the K instrumented set-up steps
            kernels = {
                # name: (ms per launch, algorithmic bytes per launch).  Each of the four kernels carries
                # its own pair of HIP events on the ctx stream (hipExtLaunchKernelGGL: begin and end of
                # that dispatch, no marker packets), recorded in every step of the timed region.
                "k_hist_tiles": (ms["hist"], n),
                "k_encode_tiles": (ms["enc_body"], n + m_bytes),
                state["sync_kernel"]: (ms["dec_sync_first"], m_bytes),
                state["write_kernel"]: (ms["dec_body"], m_bytes + n),
            }
            dominant = max(kernels, key=lambda k: kernels[k][0])
            d_ms, d_bytes = kernels[dominant]
            in_timed_region = dominant == state["write_kernel"]
            if in_timed_region:  # (the kernel that carries its events through the timed region; any other: the instrumented steps' figure)
                d_ms = body_ms_timed
            achieved = d_bytes / (d_ms * 1e-3) / 1e9
            traffic, traffic_source = load_pmc_traffic(dominant.split("<")[0], n)
            # whole encode on the GPU's clock, begin of K1 to end of K4 (enc_scan = everything between the
            # two: histogram reduce, the host's code construction, tile scan, uploads)
            enc_kernel_ms = ms["hist"] + ms["enc_scan"] + ms["enc_body"]
            out.update({
                "value_cold": round(world * n / elapsed_cold * K / 1e9, 3),  # the same K steps right behind the W warm-up steps (no further untimed steps)
                "ms_per_step_cold": round(elapsed_cold / K * 1e3, 4),
                "encode_GBps": round(world * n / (ms["enc_total"] * 1e-3) / 1e9, 2),
                "decode_GBps": round(world * n / (ms["dec_total"] * 1e-3) / 1e9, 2),
                "encode_hbm_frac": round((2 * n + m_bytes) / (enc_kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                "phase_ms": {k: round(v, 4) for k, v in ms.items()},
                "roofline": {
                    "kernel": dominant,
                    "bound": "hbm",
                    "achieved": round(achieved, 1),
                    "peak": HBM_PEAK_GBPS,
                    "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBPS, 4),
                    "frac_of_measured_copy": round(achieved / HBM_COPY_GBPS, 4),
                    "traffic": traffic,
                    "traffic_source": traffic_source,
                    "ms_per_launch": round(d_ms, 4),
                    "algorithmic_bytes_per_launch": d_bytes,
                    "measured": ("HIP events carried by the dispatch, every step of the timed region" if in_timed_region
                                 else f"HIP events carried by the dispatch, the {K} instrumented set-up steps"),
                },
                "phase_ms_measured": (f"the last {K} of the {SETTLE_STEPS} untimed set-up steps, every phase carrying HIP events; in the timed regions only "
                                      f"{state['write_kernel']} does (a dispatch with events costs ~5 us of queue time on either side: ~35 us per step)"),
                "kernels": {k: {"ms_per_launch": round(v[0], 4), "GBps": round(v[1] / (v[0] * 1e-3) / 1e9, 1) if v[0] else None,
                                "frac": round(v[1] / (v[0] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if v[0] else None} for k, v in kernels.items()},
            })
        if concat_ms is not None:
            out["concat_ms"] = round(concat_ms, 4)     # seams merged + every rank's owned words on rank 0's GPU, max over ranks, best of 3
            out["seam_ms"] = None if seam_ms is None else round(seam_ms, 4)
            out["exchange_ms"] = round(ms["exchange"], 4)  # the histogram all-gather of every step (host clock, incl. the wait for K1)
            out["exchange"] = "RCCL ncclAllGather of the 2 KiB histogram rows from device memory" if backend == "nccl" else f"{backend} all-gather through the exchange callback"
        if n1_same_ms is not None:
            # the N = 1 figure of the SAME step (every rank alone on its shard, shard-style decode), this run; the headline N = 1 line
            # of a separate run decodes cold (header hand-over and parse: ~35 us more per step) and is not the same step
            out["value_n1_same_step"] = round(n / (n1_same_ms * 1e-3) / 1e9, 3)
            out["ms_per_step_n1_same_step"] = round(n1_same_ms, 4)
            out["decode_cold_sharded_ms"] = cold_sharded_ms if isinstance(cold_sharded_ms, str) or cold_sharded_ms is None else round(cold_sharded_ms, 4)
            ref = args.ref_value or out["value_n1_same_step"]
            key = "value" if verify else "value_unverified"
            out["scaling_efficiency"] = round(out[key] / (world * ref), 4)  # value(N) / (N x value(1))
            out["scaling_efficiency_against"] = ("--ref-value" if args.ref_value else "value_n1_same_step: the same step on one GPU per rank, no group, measured in this run")
            if args.ref_value:
                out["ref_value"] = args.ref_value
        if extras is not None:
            out["workloads"] = extras
        if world == 1 and not args.no_cpu_baseline and args.full:
            if real_sample is not None:
                host_text = real_sample
            else:
                text = corpus.text_like_torch(n, 0x5EED0004 + rank, dev) if text is None else text  # the headline stream again
                host_text = text[: min(n, 1 << 30)].cpu().numpy()
            what = "enwik9" if real_sample is not None else "text-1G"
            out["cpu_baseline"] = cpu_baseline(host_text[: 768 << 20], what)
            out["cpu_baseline_parallel"] = cpu_baseline_parallel(host_text, what, args.cpu_threads)
        os.write(real_stdout, (json.dumps(out) + "\n").encode())

    if world > 1 or force_group:
        barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
