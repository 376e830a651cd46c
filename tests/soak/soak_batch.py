"""Soak of the batched calls against the oracle: random batches (1 .. 300 streams) of random sources (text, uniform
alphabets of 1 .. 256 values, a dominant symbol, geometric -> long codes, Fibonacci-like counts -> codes beyond 32 bits, empty
texts), random lengths up to a little over et_batch_small_max(), inputs packed back to back.  Every image must be
oracle.encode's and every decode oracle.decode's, stream by stream, with the status the oracle implies; bytes outside the
items' outputs must stay untouched.  Bounded: stops after TRIALS batches or MAX_SECONDS, whichever is first.
Usage: python tests/soak/soak_batch.py SEED TRIALS [MAX_SECONDS]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import entreepy_amd as E
from entreepy_amd import _native as N
from oracle import oracle as O
from tests import corpus

SENTINEL = 0xA5


def source(rng, n, seed):
    src = int(rng.integers(0, 5))
    if src == 0:
        return corpus.text_like(n, seed)
    if src == 1:
        return corpus.uniform(n, seed, 0, int(rng.integers(1, 257)))
    if src == 2:
        p = float(rng.choice([0.5, 0.9, 0.999]))
        return np.where(rng.random(n) < p, int(rng.integers(0, 256)), corpus.text_like(n, seed)).astype(np.uint8)
    if src == 3:
        return np.minimum(rng.geometric(0.5, size=n) - 1, int(rng.integers(8, 40))).astype(np.uint8)
    k = int(rng.integers(20, 42))  # Fibonacci-like counts: codes of up to ~40 bits (quirk Q3: the encode delegates, the decode declines)
    fib = [1, 1]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    reps = np.array(fib, dtype=np.float64)
    reps = np.maximum(1, (reps * min(1.0, n / reps.sum())).astype(np.int64))
    return rng.permutation(np.repeat(np.arange(k, dtype=np.uint8), reps))


def run(ctx, fn, blobs, caps, lead):
    lens = np.array([b.size for b in blobs], dtype=np.uint64)
    in_off = (np.concatenate(([0], np.cumsum(lens)[:-1])) + lead).astype(np.uint64)
    d_in = torch.from_numpy(np.concatenate([np.zeros(lead + 1, np.uint8)] + blobs)).cuda()
    caps = np.asarray(caps, dtype=np.uint64)
    room = (caps + np.uint64(15)) // np.uint64(16) * np.uint64(16) + np.uint64(32)
    out_off = np.concatenate(([0], np.cumsum(room)[:-1])).astype(np.uint64)
    d_out = torch.full((int(room.sum()) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    out_len, status, path = fn(d_in, in_off, lens, d_out, out_off, caps)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    mask = np.ones(host.size, dtype=bool)
    for o, c in zip(out_off, caps):
        mask[int(o) : int(o) + int(c)] = False
    clean = bool((host[mask] == SENTINEL).all())
    return [host[int(o) : int(o) + int(n)].tobytes() for o, n in zip(out_off, out_len)], status, path, clean


def main():
    seed, trials = int(sys.argv[1]), int(sys.argv[2])
    max_seconds = float(sys.argv[3]) if len(sys.argv) > 3 else 240.0
    rng = np.random.default_rng(seed)
    small_max = N.lib().et_batch_small_max()
    ctx = E.Context(0)
    t0 = time.time()
    bad = streams = done = 0
    for trial in range(trials):
        if time.time() - t0 > max_seconds:
            break
        texts = []
        for b in range(int(rng.integers(1, 301))):
            r = rng.random()
            n = 0 if r < 0.02 else int(rng.integers(1, 3000)) if r < 0.6 else int(rng.integers(1, 80_000)) if r < 0.97 else int(rng.integers(small_max - 2, small_max + 3000))
            texts.append(source(rng, n, seed * 1_000_000 + trial * 1000 + b) if n else np.zeros(0, np.uint8))
        want = [O.encode(t) if t.size else None for t in texts]
        images, status, path, clean = run(ctx, ctx.encode_batch_device, texts, [E.encode_bound(t.size) for t in texts], int(rng.integers(0, 16)))
        ok = clean
        long_codes = [int(O.build_dict(O.histogram(t))[1].max()) > 32 if t.size else False for t in texts]
        for b, w in enumerate(want):
            if w is None:
                ok = ok and status[b] == N.ET_ERR_EMPTY
            else:
                ok = ok and status[b] == 0 and images[b] == w and path[b] == int(texts[b].size > small_max or long_codes[b])
        comps = [np.frombuffer(w[4:], dtype=np.uint8) for w in want if w is not None]
        if comps:
            caps = [int.from_bytes(c[1:5].tobytes(), "big") + 16 for c in comps]
            decoded, status, path, clean = run(ctx, ctx.decode_batch_device, comps, caps, int(rng.integers(0, 16)))
            ok = ok and clean
            longs = [l for l, w in zip(long_codes, want) if w is not None]
            for b, c in enumerate(comps):
                if longs[b]:  # (a code beyond 32 bits: the decoder declines, as documented)
                    ok = ok and status[b] == N.ET_ERR_UNSUPPORTED
                else:
                    ok = ok and status[b] == 0 and decoded[b] == O.decode(c)
        streams += len(texts)
        done += 1
        if not ok:
            bad += 1
            print("trial", trial, "MISMATCH", [t.size for t in texts][:20], flush=True)
        if trial % 10 == 0:
            print(f"trial {trial} ok ({time.time() - t0:.0f} s)", flush=True)
    ctx.close()
    print(f"done: {done} batches, {streams} streams, bad = {bad}, {time.time() - t0:.0f} s", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
