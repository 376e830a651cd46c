"""Soak of one context moved between streams with its calls in flight (tests/test_gpu_streams.py holds the short, fixed-seed
versions): every round makes a few texts of random families and sizes, then encodes and decodes them on one context, each call on
a stream picked at random -- torch streams through torch.cuda.stream blocks, the context's own stream, a raw use_stream -- with no
synchronise until the round ends.  Every decode must equal its text and leave the 64 bytes behind it untouched.  No reserve(): the
workspaces grow inside rounds.  Progress goes to stdout once per 10 rounds.
Usage: python tests/soak/soak_streams.py SEED ROUNDS [MAX_BYTES]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import torch

import entreepy_amd as E
from tests import corpus

SLACK, SENTINEL = 64, 0xA5


def make_text(rng, n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(int(rng.integers(0, 1 << 62)))
    fam = int(rng.integers(0, 6))
    if fam == 0:
        return "text", corpus.text_like_torch(n, int(rng.integers(0, 1 << 31)), dev)
    if fam == 1:
        return "enwik", corpus.enwik_like_torch(n, int(rng.integers(0, 1 << 31)), dev)
    if fam == 2:  # uniform over 255 values: the row walk
        return "uniform255", torch.randint(1, 256, (n,), generator=g, device=dev, dtype=torch.uint8)
    if fam == 3:  # 16 values of (almost) equal weight: a fixed-length code
        return "flat16", torch.randint(0, 16, (n,), generator=g, device=dev, dtype=torch.uint8) + 100
    if fam == 4:  # 97 % zeros: the strips
        t = torch.randint(1, 255, (n,), generator=g, device=dev, dtype=torch.uint8)
        return "zeros97", t.masked_fill_(torch.rand(n, generator=g, device=dev) < 0.97, 0)
    return "flat31", torch.randint(0, 31, (n,), generator=g, device=dev, dtype=torch.uint8)  # the exit maps


def main():
    seed, rounds = int(sys.argv[1]), int(sys.argv[2])
    max_bytes = int(sys.argv[3]) if len(sys.argv) > 3 else 64 << 20
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    ctx = E.Context(0)
    streams = [torch.cuda.Stream() for _ in range(3)]
    t0 = time.time()
    bad = calls = 0

    def on_random_stream(fn):
        k = int(rng.integers(0, 5))
        if k < 3:
            ctx.use_torch_stream()
            with torch.cuda.stream(streams[k]):
                return fn()
        if k == 3:
            ctx.use_own_stream()
        else:
            ctx.use_stream(streams[int(rng.integers(0, 3))].cuda_stream)
        return fn()

    for r in range(rounds):
        jobs = []
        for _ in range(int(rng.integers(2, 7))):
            n = int(rng.integers(1 << 20, max_bytes)) if rng.random() < 0.7 else int(rng.integers(4096, 1 << 20))
            name, text = make_text(rng, n, dev)
            if bool((text == text[0]).all()):
                continue  # (a lone symbol encodes to the bare header: nothing to decode)
            enc = torch.zeros(E.encode_bound(n) + 64, dtype=torch.uint8, device=dev)
            out = torch.full((n + SLACK,), SENTINEL, dtype=torch.uint8, device=dev)
            jobs.append((name, n, text, enc, out))
        torch.cuda.synchronize()  # (inputs and outputs are made on the default stream; the calls below order only among themselves)
        ms = [on_random_stream(lambda j=j: ctx.encode_device(j[2], j[3])) for j in jobs]
        got = {}
        for i in rng.permutation(len(jobs)):
            name, n, text, enc, out = jobs[i]
            got[i] = on_random_stream(lambda: ctx.decode_device(enc, out, skip=4, length=ms[i] - 4))
        calls += 2 * len(jobs)
        torch.cuda.synchronize()
        for i, (name, n, text, enc, out) in enumerate(jobs):
            if got[i] != n or not torch.equal(out[:n], text) or not bool((out[n:] == SENTINEL).all()):
                bad += 1
                print("round", r, "job", i, name, n, "MISMATCH", got[i], flush=True)
        if r % 10 == 0:
            print(f"round {r} ok ({calls} calls, {time.time() - t0:.0f} s)", flush=True)
    ctx.close()
    print(f"done: {rounds} rounds, {calls} calls, bad = {bad}, {time.time() - t0:.0f} s", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
