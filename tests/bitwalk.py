"""The serial decoder as a table: for every bit of a stream, the codeword that begins there; walks over that table give where a
range is left, how many codewords begin in it and which -- what the synchronisation kernels compute in parallel, here one step
at a time.  Plain numpy, a module like limits.py and guards.py, imported by name; it knows nothing about the library.
tests/test_syncwork_host.py checks it against the oracle, tests/test_gpu_syncwork.py holds the kernels against it.

Bit q of a stream is bit 7 - q % 8 of its byte q // 8; the streams handed in begin at the 4-byte aligned word their body starts
in, which is how the range calls count.

Bit patterns that are no symbol's codeword (hand-made tables) -- two rules, both the library's:

  unmatched="stop", the default: nothing says how to go on.  L is 0 there, walk() raises Unmatched, Jumps.walk answers -1,
  merge_distances answers NEVER.

  unmatched="skip", the rule of the window kernels (csrc/et_kernels_fallback.hip; include/entreepy_hip.h at
  et_decode_body_device: "passed over one bit at a time"): where no codeword matches at bit q -- the bits behind the stream's end
  read as zeros -- the step is ONE bit and carries no symbol; next_table returns a third array C, "a codeword begins here", and
  every walk that is handed C counts and collects the codewords only and steps over the rest.  The last max_length bits of a
  stream: a pattern without a codeword is passed over as anywhere else, bit by bit, up to the last bit (walk_subsequence: its
  step of 1 never has pos + 1 > lim while pos < lim); a codeword that MATCHES (against the zeros behind the end) and reaches
  beyond the last bit is cut -- the walk ends at the end, the codeword uncounted (walk_subsequence: `CHECK_LIM && pos + len_ >
  lim`, off_stream).  The walks over registers (walk_steps, walk_write) serve interior blocks only and never see the end.

  holes as leaves, the rule of the tree walk (csrc/et_treewalk_host.cpp tw_build_tree(complete = true)): every child a tree
  node lacks is a leaf that decodes as byte 0.  leaves_for_holes() gives those leaves as pseudo-codewords; next_table takes
  them as `extra`, and the walks are the plain ones (the table is then a full tree: nothing is unmatched)."""
import numpy as np

# The tree walk's geometry, as csrc/et_treewalk.hip has it: k_tw_sync's lane (q[u]: "512-bit lane = subsequences 2q, 2q + 1") and
# its run-in (tw_walk<0, 4 * TW_RUN, ...>: "from the root, 128 bits before the lane's own"; TW_RUN = 4 words, also DEC_WARMUP_BITS).
LANE_BITS = 512
RUN_IN_BITS = 128
BLOCK_BYTES = 8192  # what the ranges of a split stream are multiples of
BLOCK_BITS = BLOCK_BYTES * 8
NEVER = np.iinfo(np.int64).max  # merge_distances: the walk met a bit pattern without a codeword


class Unmatched(ValueError):
    """A walk stands on a bit pattern that is no codeword's (hand-made tables): nothing says how to go on."""


def windows32(stream_bytes):
    """The 32 bits that begin at every bit of the stream (zeros behind its end), as uint32."""
    b = np.frombuffer(bytes(stream_bytes), dtype=np.uint8) if not isinstance(stream_bytes, np.ndarray) else stream_bytes
    n = b.size
    b = np.concatenate([b, np.zeros(8, np.uint8)]).astype(np.uint64)
    v = (b[0:n] << np.uint64(32)) | (b[1 : n + 1] << np.uint64(24)) | (b[2 : n + 2] << np.uint64(16)) | (b[3 : n + 3] << np.uint64(8)) | b[4 : n + 4]
    shifts = (8 - np.arange(8)).astype(np.uint64)
    return ((v[:, None] >> shifts[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(-1)


def next_table(stream_bytes, data, length, unmatched="stop", extra=()):
    """-> (L, S), one entry per bit of the stream: the length of the codeword that begins at bit q and its symbol; L[q] = 0
    where no codeword matches.  (The bits behind the stream's end count as zeros: a codeword with q + L[q] beyond the last bit
    is cut by the end -- walk() knows.)  One shift per code length, one compare per coded symbol (a lookup for the lengths up
    to 16 bits, which is the same compare for all symbols of a length at once).
    unmatched="skip" -> (L, S, C): L[q] = 1 where no codeword matches, C[q] says where one does (the module's docstring).
    extra: further codewords (code, length, symbol) beside the table's -- leaves_for_holes()."""
    assert unmatched in ("stop", "skip")
    data, length = np.asarray(data, np.uint32), np.asarray(length, np.uint8)
    coded = np.flatnonzero(length > 0)
    codes = np.concatenate([data[coded], np.array([c for c, _, _ in extra], np.uint32)]).astype(np.uint32)
    lens = np.concatenate([length[coded], np.array([l for _, l, _ in extra], np.uint8)]).astype(np.uint8)
    symbols = np.concatenate([coded, np.array([s for _, _, s in extra], np.int64)]).astype(np.uint8)
    win = windows32(stream_bytes)
    L, S = np.zeros(win.size, np.uint8), np.zeros(win.size, np.uint8)
    for l in sorted(set(lens.tolist())):
        w = win >> np.uint32(32 - l)
        which = np.flatnonzero(lens == l)
        if l <= 16:
            lut = np.zeros(1 << l, np.uint16)
            lut[codes[which]] = which + 1
            hit = lut[w]
            m = hit > 0
            L[m], S[m] = l, symbols[hit[m] - 1]
        else:
            for i in which:
                m = w == codes[i]
                L[m], S[m] = l, symbols[i]
    if unmatched == "stop":
        return L, S
    C = L > 0
    L[~C] = 1
    return L, S, C


def leaves_for_holes(data, length):
    """The tree walk's rule for a table that leaves bit patterns without a symbol: every child that a node of the codewords'
    tree lacks is a leaf, and it decodes as byte 0 -> [(code, length, 0)], one pseudo-codeword per maximal missing subtree,
    for next_table's `extra`.  (The tree's nodes are the proper prefixes of the codewords, the empty one included.)"""
    data, length = np.asarray(data, np.uint32), np.asarray(length, np.uint8)
    words = {(int(data[s]), int(length[s])) for s in np.flatnonzero(length > 0)}
    nodes = {(c >> (l - k), k) for c, l in words for k in range(l)}
    assert not (nodes & words), "a codeword is a prefix of another"
    return sorted(((c << 1) | bit, k + 1, 0) for c, k in nodes for bit in (0, 1) if ((c << 1) | bit, k + 1) not in nodes | words)


def decode_by_rule(stream_bytes, data, length, rule, first_bit=0):
    """The symbols of the whole stream from first_bit under a table that leaves bit patterns without a codeword -- rule "skip":
    passed over bit by bit (the window kernels); "leaves": every hole of the tree a leaf that decodes as byte 0 (the tree walk)."""
    if rule == "leaves":
        L, S = next_table(stream_bytes, data, length, extra=leaves_for_holes(data, length))
        return walk_symbols(L, S, first_bit, L.size)[1]
    assert rule == "skip"
    L, S, C = next_table(stream_bytes, data, length, "skip")
    return walk_symbols(L, S, first_bit, L.size, C)[1]


def boundaries(first_bit, length, text):
    """The true codeword boundaries of a text packed from first_bit: entry i is where codeword i begins, the last entry where
    the last one ends."""
    bits = np.asarray(length, np.uint8)[np.asarray(text, np.uint8)].astype(np.int64)
    return first_bit + np.concatenate([[0], np.cumsum(bits)])


def _cut(Lb, p):
    """The codeword at p is cut by the stream's end (it is nobody's); a pattern without a codeword further in raises."""
    l = Lb[p]
    if l and p + l <= len(Lb):
        return False
    if p + 32 > len(Lb):
        return True
    raise Unmatched(f"no codeword begins at bit {p}")


def _as_bytes(a, dtype=np.uint8):
    return a if isinstance(a, bytes) else np.asarray(a, dtype).tobytes()


def walk(L, p, end, C=None):
    """Follow L from bit p until the position is at or past bit `end` -> (exit, count): the first boundary at or past `end`
    and the codewords that began in front of it.  A codeword cut by the stream's end ends the walk at `end`, uncounted.
    C (next_table's, unmatched="skip"): the steps that are no codeword's are taken and not counted."""
    Lb = _as_bytes(L)
    n, size = 0, len(Lb)
    if C is not None:
        Cb = _as_bytes(C)
        while p < end:
            l = Lb[p]
            if Cb[p]:
                if p + l > size:
                    return end, n
                n += 1
            p += l
        return p, n
    while p < end:
        l = Lb[p]
        if l == 0 or p + l > size:
            if _cut(Lb, p):
                return end, n
        p += l
        n += 1
    return p, n


def walk_positions(L, p, end, C=None):
    """walk() that keeps where it stood -> (exit, the bits at which the counted codewords begin, as int64)."""
    Lb = _as_bytes(L)
    at, size = [], len(Lb)
    if C is not None:
        Cb = _as_bytes(C)
        while p < end:
            l = Lb[p]
            if Cb[p]:
                if p + l > size:
                    p = end
                    break
                at.append(p)
            p += l
        return p, np.asarray(at, np.int64)
    while p < end:
        l = Lb[p]
        if l == 0 or p + l > size:
            if _cut(Lb, p):
                p = end
                break
        at.append(p)
        p += l
    return p, np.asarray(at, np.int64)


def walk_symbols(L, S, p, end, C=None):
    """walk() that also returns the symbols -> (exit, symbols as uint8): what a write of the walked range produces."""
    exit_, at = walk_positions(L, p, end, C)
    return exit_, np.asarray(S)[at].astype(np.uint8)


class Jumps:
    """walk() for many (start, end) pairs at once -- all start offsets of a map, every cut of a stream: J[k][q] is where 2^k
    steps from bit q lead (pointer doubling; 4 bytes per bit and level, so for streams of a megabit, not of sixteen).  With C
    (unmatched="skip") a step need not be a codeword: N[k][q] counts the codewords among those 2^k steps, as much again."""

    def __init__(self, L, C=None):
        L = np.asarray(L, np.uint8)
        self.n = n = L.size
        self.L = L
        self.dead = dead = n + 64  # where the codewords the stream's end cuts and the patterns without a codeword lead; absorbing
        nxt = np.full(dead + 1, dead, np.int32)
        q = np.arange(n, dtype=np.int64)
        to = q + L
        ok = (L > 0) & (to <= n)
        if C is not None:
            C = np.asarray(C, bool)
            ok |= ~C  # one bit on: never beyond the end
        nxt[:n][ok] = to[ok]
        self.J = [nxt]
        self.N = None
        if C is not None:
            cnt = np.zeros(dead + 1, np.int32)
            cnt[:n][ok & C] = 1
            self.N = [cnt]
        while (1 << len(self.J)) < n + 1:
            j = self.J[-1]
            if self.N is not None:
                c = self.N[-1]
                self.N.append(c + c[j])
            self.J.append(j[j])

    def walk(self, starts, ends):
        """-> (exits, counts) as int64 arrays; starts below ends.  An exit of -1: the walk met a pattern without a codeword
        (never with C)."""
        pos = np.array(starts, dtype=np.int64, ndmin=1)
        ends = np.broadcast_to(np.asarray(ends, np.int64), pos.shape)
        assert (pos < ends).all() and (ends <= self.n).all()
        count = np.zeros(pos.shape, np.int64)
        for k in range(len(self.J) - 1, -1, -1):
            to = self.J[k][pos].astype(np.int64)
            go = to < ends
            count += np.where(go, self.N[k][pos], 0) if self.N is not None else go.astype(np.int64) << k
            pos = np.where(go, to, pos)
        last = self.J[0][pos].astype(np.int64)  # at or past the end, or dead
        cut = last == self.dead
        exits = np.where(cut, ends, last)
        if self.N is not None:
            return exits, count + self.N[0][pos]
        unmatched = cut & (pos + 32 <= self.n)
        exits[unmatched] = -1
        return exits, count + (~cut).astype(np.int64)


def chain(L, first_bit, at=None, C=None):
    """is_boundary, one flag per bit and one for the stream's end: the bits at which the whole codewords of the walk from
    first_bit begin (the text's, and those in the pad bits behind it; `at`: walk_positions' answer, if the caller has it), and
    the end itself.  With C the bits that the walk only steps over are no boundaries."""
    n = len(L)
    if at is None:
        _, at = walk_positions(L, first_bit, n, C)
    on = np.zeros(n + 1, bool)
    on[at] = True
    on[n] = True
    return on


def unsettled_runs(dist, lanes_per_block=BLOCK_BITS // LANE_BITS, settled_below=LANE_BITS + RUN_IN_BITS):
    """Per block of lanes: the longest run of consecutive lanes whose blind walk (merge_distances) is NOT on the true chain
    before the lane's own bits end.  Such a lane leaves its bits wrongly until the lane before it hands it its true start,
    one lane per trip of the block's fixed point: a run of r lanes takes r trips behind the first, and a block whose run
    reaches the trip cap gives up.  A lane whose walk met a pattern without a codeword (NEVER) is nobody's to judge: it ends
    a run.  NEVER is the default rule's answer (unmatched="stop": the tree walk's tables, whose holes are leaves, are not the
    reference's to follow); distances made under unmatched="skip", the window kernels' rule, hold no NEVER, and every lane is
    judged."""
    dist = np.asarray(dist)
    bad = (dist >= settled_below) & (dist != NEVER)
    runs = np.zeros((bad.size + lanes_per_block - 1) // lanes_per_block, np.int64)
    cur = 0
    for i, b in enumerate(bad.tolist()):
        if i % lanes_per_block == 0:  # (a block's first lane gets its start from the block before, not from a lane)
            cur = 0
        cur = cur + 1 if b else 0
        runs[i // lanes_per_block] = max(runs[i // lanes_per_block], cur)
    return runs


def longest_unsettled_run(stream_bytes, first_bit, data, length, lane_bits=LANE_BITS, run_in_bits=RUN_IN_BITS, unmatched="stop"):
    """A whole stream under the reference: over all 8 KiB blocks, the longest run of consecutive lanes that leave their own
    bits off the true chain (unsettled_runs of merge_distances).  unmatched: next_table's."""
    return int(unsettled_block_runs(stream_bytes, first_bit, data, length, lane_bits, run_in_bits, unmatched).max())


def unsettled_block_runs(stream_bytes, first_bit, data, length, lane_bits=LANE_BITS, run_in_bits=RUN_IN_BITS, unmatched="stop", extra=()):
    """longest_unsettled_run's figure for every 8 KiB block of the stream (unsettled_runs), as int64.  extra: next_table's."""
    L, _, *C = next_table(stream_bytes, data, length, unmatched, extra)
    C = C[0] if C else None
    dist = merge_distances(L, chain(L, first_bit, C=C), lane_bits, run_in_bits, enough=lane_bits + run_in_bits, C=C)
    assert C is None or int(dist.max()) < NEVER
    return unsettled_runs(dist, BLOCK_BITS // lane_bits, lane_bits + run_in_bits)


def merge_distances(L, is_boundary, lane_bits=LANE_BITS, run_in_bits=RUN_IN_BITS, enough=None, C=None):
    """For every lane of lane_bits bits: the distance from `lane start - run_in_bits` to the first true boundary that a walk
    begun at that bit (as if a codeword began there) reaches -- how far a lane that runs in blind is from the truth.  Lane 0
    has nothing in front of it: 0.  NEVER: the walk met a pattern without a codeword -- under the default rule; with C
    (next_table's, unmatched="skip") such a pattern is stepped over, every lane has a distance, and NEVER does not occur.
    A walk that leaves the stream has met everybody (the lanes behind the end stand at the root).  enough: a walk that has
    gone that many bits without meeting the truth stops there, and where it stands is its answer (at least `enough`: all that
    a caller with a threshold needs)."""
    L = np.asarray(L, np.uint8)
    n = L.size
    n_lanes = (n + lane_bits - 1) // lane_bits
    p0 = np.arange(n_lanes, dtype=np.int64) * lane_bits - run_in_bits
    dist = np.zeros(n_lanes, np.int64)
    live = np.flatnonzero(p0 >= 0)
    pos = p0[live].copy()
    while live.size:
        done = (pos >= n) | is_boundary[np.minimum(pos, n)]
        if enough is not None:
            done |= pos - p0[live] >= enough
        dist[live[done]] = np.minimum(pos[done], n) - p0[live[done]]
        live, pos = live[~done], pos[~done]
        step = L[pos].astype(np.int64)
        stuck = (step == 0) | (pos + step > n)  # (with C no step is 0, and a step beyond the end is a codeword's: cut)
        cut = stuck & (pos + 32 > n) if C is None else stuck
        dist[live[stuck & ~cut]] = NEVER
        dist[live[cut]] = n - p0[live[cut]]
        live, pos = live[~stuck], (pos + step)[~stuck]
    return dist


# ---- streams too long to hold bit by bit: the true chain from the text's code lengths, the walks in pieces ----------------------


class TextBounds:
    """The true codeword boundaries of a text packed from first_bit (boundaries()) without an entry per symbol: the sums of
    every `every` code lengths are kept, a stretch of boundaries is worked out when asked for."""

    def __init__(self, first_bit, length, text, every=4096):
        self.lens = np.asarray(length, np.uint8)[np.asarray(text, np.uint8)]
        self.every = every
        whole = self.lens.size // every * every
        sums = self.lens[:whole].reshape(-1, every).sum(axis=1, dtype=np.int64)
        self.coarse = first_bit + np.concatenate([[0], np.cumsum(sums)])  # where symbol k * every begins
        self.end = int(self.coarse[-1]) + int(self.lens[whole:].sum(dtype=np.int64))  # where the last codeword ends

    def between(self, lo, hi):
        """The boundaries p with lo <= p < hi, as int64: where the codewords begin, and where the last one ends."""
        k0 = max(int(np.searchsorted(self.coarse, lo, side="right")) - 1, 0)
        k1 = int(np.searchsorted(self.coarse, hi, side="left"))
        lens = self.lens[k0 * self.every : k1 * self.every]
        p = int(self.coarse[k0]) + np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        return p[(p >= lo) & (p < hi)]


def _lengths16(piece, data, length):
    """next_table's L for a table whose longest codeword has 16 bits or fewer, by ONE lookup of the 16 bits that begin at every
    bit (the table is prefix-free: at most one codeword is a prefix of them); the last two bytes of `piece` are only read."""
    lut = np.zeros(1 << 16, np.uint8)
    for s in np.flatnonzero(length).tolist():
        l, c = int(length[s]), int(data[s])
        lut[c << (16 - l) : (c + 1) << (16 - l)] = l
    b = piece.astype(np.uint32)
    v = (b[:-2] << np.uint32(16)) | (b[1:-1] << np.uint32(8)) | b[2:]
    w = (v[:, None] >> (8 - np.arange(8, dtype=np.uint32))[None, :]) & np.uint32(0xFFFF)
    return lut[w.reshape(-1)]


def _piece(stream, lo_bit, hi_bit, data, length, bounds, unmatched):
    """next_table's L (and C) and the true chain's flags for the bits [lo_bit, hi_bit) of a stream (lo_bit a multiple of 8),
    four more bytes read behind them for the codewords that reach over -> (L, C or None, on_chain with one more entry, for
    hi_bit)."""
    stream = np.frombuffer(bytes(stream), dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream
    data, length = np.asarray(data, np.uint32), np.asarray(length, np.uint8)
    n = (hi_bit - lo_bit + 7) // 8
    piece = np.zeros(n + 4, np.uint8)
    got = stream[lo_bit // 8 : lo_bit // 8 + n + 4]
    piece[: got.size] = got
    if int(length.max()) <= 16:
        L = _lengths16(piece, data, length)[: hi_bit - lo_bit]
    else:
        L = next_table(piece, data, length)[0][: hi_bit - lo_bit]
    C = None
    if unmatched == "skip":
        C = L > 0
        L[~C] = 1
    on = np.zeros(hi_bit - lo_bit + 1, bool)
    on[bounds.between(lo_bit, hi_bit + 1) - lo_bit] = True
    return L, C, on


def seam_walks(stream, first_bit, data, length, text, run_in_bits=RUN_IN_BITS, reach=1024, unmatched="skip", bounds=None):
    """What the first lane of every block b >= 1 makes of its blind run-in, walked at the seams only: from run_in_bits in front
    of the block's first bit, as if a codeword began there, to the first position at or behind that bit -> (blind, true,
    merged), one entry per block from block 1 on, in bits behind the block's first bit: where the blind walk stands, where the
    true chain's first codeword of the block begins, and where the blind walk first stands on the true chain (-1: not within
    `reach` bits).  A sweep's first lane of a block that nobody hands a start begins at `blind`; the block before it ends on
    `true`."""
    n_bits = len(stream) * 8
    bounds = bounds or TextBounds(first_bit, length, text)
    seams = np.arange(1, (n_bits + BLOCK_BITS - 1) // BLOCK_BITS, dtype=np.int64) * BLOCK_BITS
    blind, true, merged = (np.full(seams.size, -1, np.int64) for _ in range(3))
    for i, seam in enumerate(seams.tolist()):
        lo, hi = seam - run_in_bits, min(seam + reach, n_bits)
        assert lo % 8 == 0
        L, _, on = _piece(stream, lo, hi, data, length, bounds, unmatched)
        ahead = np.flatnonzero(on[run_in_bits:])
        true[i] = ahead[0] if ahead.size else -1
        p = 0
        while p < hi - lo:
            if p >= run_in_bits:
                if blind[i] < 0:
                    blind[i] = p - run_in_bits
                if on[p]:
                    merged[i] = p - run_in_bits
                    break
            if not L[p]:
                break  # (unmatched="stop": nothing says how to go on)
            p += int(L[p])
    return blind, true, merged


def listed_after_first_sweep(stream, first_bit, data, length, text, **kw):
    """-> (the blocks b >= 1 whose first lane's blind run-in leaves it another start than the true one -- what a check of
    every block's start against the exit of the block before it lists, where nothing has settled the block's first lane --,
    seam_walks' merged for them)."""
    blind, true, merged = seam_walks(stream, first_bit, data, length, text, **kw)
    wrong = np.flatnonzero(blind != true)
    return wrong + 1, merged[wrong]


def unsettled_block_runs_by_text(stream, first_bit, data, length, text, lanes=((LANE_BITS, RUN_IN_BITS),), unmatched="skip", piece_blocks=64, bounds=None):
    """unsettled_block_runs for a stream of many megabytes whose text is at hand, for several lane geometries (lane_bits,
    run_in_bits) at once -> one array per geometry: the true chain from the text's code lengths (TextBounds) instead of a walk,
    the table and the lanes' blind walks in pieces of piece_blocks blocks -- a piece begins a lane early, so that its first lane
    has its run-in, and ends a lane and a run-in late, so that no walk of its lanes leaves it.  The same figures as
    unsettled_block_runs (tests/test_repairs_host.py holds the two against each other)."""
    stream = np.frombuffer(bytes(stream), dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream
    n_bits = stream.size * 8
    bounds = bounds or TextBounds(first_bit, length, text)
    n_blocks = (n_bits + BLOCK_BITS - 1) // BLOCK_BITS
    widest = max(l for l, _ in lanes)
    dist = [np.zeros((n_bits + l - 1) // l, np.int64) for l, _ in lanes]
    for b0 in range(0, n_blocks, piece_blocks):
        b1 = min(b0 + piece_blocks, n_blocks)
        lo = max(b0 * BLOCK_BITS - widest, 0)
        hi = min(b1 * BLOCK_BITS + widest + max(r for _, r in lanes) + 64, n_bits)
        L, C, on = _piece(stream, lo, hi, data, length, bounds, unmatched)
        if hi == n_bits:
            on[hi - lo] = True  # chain(): the stream's end
        for (lane_bits, run_in_bits), out in zip(lanes, dist):
            lead = (b0 * BLOCK_BITS - lo) // lane_bits  # whole lanes in front of the piece's own (lo is a multiple of every lane)
            assert lo % lane_bits == 0
            l0, l1 = b0 * BLOCK_BITS // lane_bits, min(b1 * BLOCK_BITS // lane_bits, out.size)
            d = merge_distances(L, on, lane_bits, run_in_bits, enough=lane_bits + run_in_bits, C=C)
            out[l0:l1] = d[lead : lead + l1 - l0]
    assert C is None or max(int(d.max()) for d in dist) < NEVER
    return [unsettled_runs(d, BLOCK_BITS // l, l + r) for d, (l, r) in zip(dist, lanes)]
