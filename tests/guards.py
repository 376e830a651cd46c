"""Helpers the GPU test modules share: output buffers with guard bytes on both sides (what may a call write?) and hand-made
code tables.  A plain module, imported by name; nothing here is a fixture."""
import numpy as np

FILL = 0xA5
FRONT = BACK = 64


class Guarded:
    """FRONT + room + BACK bytes, all `fill`; the usable part -- .room, a view of `room` bytes, at address .ptr -- begins on a
    16-byte boundary.  device=None: host memory (numpy), else a torch device.  After the calls under test, check() takes a
    snapshot (after a torch.cuda.synchronize() for device memory); front_clean / back_clean / first_dirty / data read it."""

    def __init__(self, room, fill=FILL, device="cuda"):
        self.n, self.fill, self.on_device = int(room), fill, device is not None
        total = FRONT + self.n + BACK + 16
        if self.on_device:
            import torch

            self.buf = torch.full((total,), fill, dtype=torch.uint8, device=device)
            base = self.buf.data_ptr()
        else:
            self.buf = np.full(total, fill, dtype=np.uint8)
            base = self.buf.ctypes.data
        self.lo = FRONT + (-(base + FRONT)) % 16
        self.ptr = base + self.lo
        assert self.ptr % 16 == 0 and self.lo >= FRONT
        self.room = self.buf[self.lo : self.lo + self.n]
        self.snap = None

    def refill(self):
        if self.on_device:
            self.buf.fill_(self.fill)
        else:
            self.buf[:] = self.fill
        self.snap = None

    def check(self):
        if self.on_device:
            import torch

            torch.cuda.synchronize()
            self.snap = self.buf.cpu().numpy()
        else:
            self.snap = self.buf.copy()
        return self

    def data(self, n=None):
        """The first n bytes of the usable part (default: all of it), as the snapshot holds them."""
        return self.snap[self.lo : self.lo + (self.n if n is None else n)]

    def front_clean(self):
        return bool((self.snap[: self.lo] == self.fill).all())

    def back_clean(self, from_byte):
        """Every byte from offset from_byte of the usable part to the end of the back guard still holds the fill."""
        return bool((self.snap[self.lo + from_byte :] == self.fill).all())

    def first_dirty(self, from_byte=None):
        """Offset, relative to the usable part's first byte (negative: in the front guard), of the first byte that no longer
        holds the fill: in the front guard, or at or behind from_byte (default: the end of the usable part).  None: clean."""
        from_byte = self.n if from_byte is None else from_byte
        watched = np.ones(self.snap.size, dtype=bool)
        watched[self.lo : self.lo + from_byte] = False
        bad = np.flatnonzero(watched & (self.snap != self.fill))
        return int(bad[0]) - self.lo if bad.size else None

    def assert_extent(self, out_len, what, slack=0):
        """Nothing in front of the usable part and nothing from out_len + slack on was written."""
        dirty = self.first_dirty(out_len + slack)
        assert dirty is None, f"{what}: byte at offset {dirty} written, outside [0, {out_len}{' + %d' % slack if slack else ''}) of a buffer of {self.n}"


def _random_prefix_code(rng, n_sym, max_len):
    """A prefix-free table with random lengths up to max_len (Kraft-feasible), codes
    assigned canonically; not optimal, only a legal input for the body kernels."""
    lens = np.sort(rng.integers(2, max_len + 1, size=n_sym))
    while sum(2.0 ** -int(l) for l in lens) > 1.0:
        lens[np.argmin(lens)] += 1
        lens = np.sort(lens)
    code, prev, codes = 0, int(lens[0]), []
    for l in lens:
        code <<= int(l) - prev
        prev = int(l)
        codes.append(code)
        code += 1
    return lens, codes


def _sparse_dictionary():
    """A prefix-free table no encoder makes: two 2-bit codes and a hundred 16-bit codes 1iiiiiii00000000 -- completed with a
    leaf for every bit pattern nobody has, its tree has ~900 internal nodes, beyond the tree walk's table (255)."""
    data_t, len_t = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    data_t[32], len_t[32] = 0b00, 2
    data_t[101], len_t[101] = 0b01, 2
    for i in range(100):
        data_t[120 + i], len_t[120 + i] = 0x8000 | (i << 8), 16
    return data_t, len_t, np.array([32, 101] + list(range(120, 220)))


def _flat200_dictionary():
    """200 symbols with the 8-bit codes 0 .. 199 (the code of symbol s is the byte s): the bytes 200 .. 255 are bit patterns
    nobody has.  A tree the walk can hold, but nearly fixed-length: the exit maps, and -- the tree not being full -- the
    window kernels' write behind them."""
    data_t, len_t = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    data_t[:200], len_t[:200] = np.arange(200), 8
    return data_t, len_t


def _small_holed_dictionary():
    """0, 10, 110 and the sixteen 8-bit codewords 1110xxxx: a small tree with one hole, the pattern 1111.  The tree walk takes
    it (the hole becomes a leaf that decodes as byte 0); if its sweep gives up, the exit maps pass the hole over bit by bit.
    -> (data, length, the symbols)."""
    data_t, len_t = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    data_t[65], len_t[65] = 0b0, 1
    data_t[66], len_t[66] = 0b10, 2
    data_t[67], len_t[67] = 0b110, 3
    for i in range(16):
        data_t[100 + i], len_t[100 + i] = (0b1110 << 4) | i, 8
    return data_t, len_t, np.array([65, 66, 67] + list(range(100, 116)))


def sparse_text(n, seed):
    """The text recipe of the sparse fixtures under _sparse_dictionary: half of it the 2-bit code of byte 32, so that the
    stream re-synchronises."""
    _, _, syms = _sparse_dictionary()
    rng = np.random.default_rng(seed)
    text = syms[np.minimum(rng.integers(0, 300, size=n), syms.size - 1) % syms.size].astype(np.uint8)
    text[rng.random(n) < 0.5] = 32
    return text


def ones_longest(lengths):
    """{symbol: length} -> (data, length) of the canonical code of those lengths (tests/test_shared_host.py): the shortest
    codeword all zeros, the LONGEST all ones -- a run of 0xff bytes is that codeword over and over, from whatever bit."""
    from tests.test_shared_host import canonical

    data, length = canonical(lengths)
    longest = int(length.max())
    assert int(data[length == longest].max()) == (1 << longest) - 1
    return data, length


def image_under(data, length, text):
    """The .et image (less its first four bytes) of a text under a hand-made table: the library's header, the oracle's body."""
    import entreepy_amd as E
    from oracle import oracle as O

    return (E.Codebook.from_tables(data, length).header(len(text)) + O.pack_body(data, length, text)[0])[4:]


def _skewed_flat_dictionary():
    """A spread-length code with a flat class that never re-synchronises, in a table the tree walk cannot hold:
      skewed  00, 010, 0110, 01110, 011110, 011111                           (the bytes 1 .. 6: 2 to 6 bits, complete under 0)
      flat    1x1x1x1x, the sixteen 8-bit codewords with ones at their even bits  (the bytes 16 .. 31)
      filler  100 iiiiiii 000000 for i < 100, 16 bits, in no text            (the bytes 120 .. 219: with a leaf for every bit
              pattern nobody has, ~700 internal nodes, beyond the tree walk's 255 -- as _sparse_dictionary)
    Two bits into a flat codeword another flat codeword begins, whatever the x: a walk that stands at an even offset inside
    the flat codewords reads flat codewords for good and meets the true boundaries only if its offset is 0 mod 8.
    -> (data, length, the skewed symbols, the flat symbols)."""
    data_t, len_t = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    for s, (c, l) in enumerate([(0b00, 2), (0b010, 3), (0b0110, 4), (0b01110, 5), (0b011110, 6), (0b011111, 6)], start=1):
        data_t[s], len_t[s] = c, l
    for j in range(16):
        x = [(j >> k) & 1 for k in (3, 2, 1, 0)]
        data_t[16 + j], len_t[16 + j] = int("".join("1%d" % b for b in x), 2), 8
    for i in range(100):
        data_t[120 + i], len_t[120 + i] = (0b100 << 13) | (i << 6), 16
    return data_t, len_t, np.arange(1, 7, dtype=np.uint8), np.arange(16, 32, dtype=np.uint8)


def _skewed_run(rng, n, flat_follows):
    """n skewed symbols of _skewed_flat_dictionary (the short ones the likelier); flat_follows: padded with one or two more so
    that what follows begins 2, 4 or 6 bits behind a byte boundary, if the run itself begins at one."""
    _, len_t, skewed, _ = _skewed_flat_dictionary()
    run = skewed[np.minimum(rng.geometric(0.5, size=n) - 1, skewed.size - 1)]
    if not flat_follows:
        return run
    bits = int(len_t[run].astype(np.int64).sum())
    pad = []
    if bits % 2:
        pad.append(2)  # the 3-bit codeword
    if (bits + 3 * len(pad)) % 8 == 0:
        pad.append(1)  # the 2-bit codeword
    run = np.concatenate([run, np.array(pad, np.uint8)])
    assert int(len_t[run].astype(np.int64).sum()) % 8 in (2, 4, 6)
    return run


# island(where): (skewed symbols in front, flat symbols, skewed symbols behind) -- 144 blocks of 8 KiB each, the island in the
# first, a middle and the last one
ISLANDS = {"first": (3_000, 1_500, 3_200_000), "middle": (1_600_000, 1_500, 1_600_000), "last": (3_200_000, 1_500, 3_000)}


def island(where, seed=7):
    """-> (data, length, text): ONE stretch that does not settle in a long stream that does, under _skewed_flat_dictionary --
    skewed symbols, 1 500 flat ones laid 2, 4 or 6 bits behind a byte boundary as in skewed_then_flat (12 000 bits: some 46
    subsequences of 256 bits whose blind run-in stands in a phase that never meets the truth), skewed symbols again.  One
    block gives up in the window family's first sweep and stays unsettled through the second; everything else is clean: few
    enough blocks for the listed repair sweeps, not for the fallback (tests/test_syncwork_host.py checks all of that on the
    input)."""
    n_head, n_flat, n_tail = ISLANDS[where]
    data_t, len_t, _, flat = _skewed_flat_dictionary()
    rng = np.random.default_rng(seed)
    head = _skewed_run(rng, n_head, True)
    middle = flat[rng.integers(0, flat.size, size=n_flat)]
    return data_t, len_t, np.concatenate([head, middle, _skewed_run(rng, n_tail, False)]).astype(np.uint8)


def skewed_then_flat(n_head=40_000, n_flat=60_000, seed=5):
    """-> (data, length, text): skewed symbols (the short ones the likelier), then flat symbols only, then a thousand skewed
    ones again, under _skewed_flat_dictionary.  The skewed part is padded with one or two symbols so that the flat part begins
    2, 4 or 6 bits behind a byte boundary: every blind run-in, which begins at a byte boundary, then stands at an even offset
    that is not 0 mod 8 -- in the phase that never meets the truth."""
    data_t, len_t, skewed, flat = _skewed_flat_dictionary()
    rng = np.random.default_rng(seed)
    head = skewed[np.minimum(rng.geometric(0.5, size=n_head) - 1, skewed.size - 1)]
    bits = int(len_t[head].astype(np.int64).sum())
    pad = []
    if bits % 2:
        pad.append(2)  # the 3-bit codeword
    if (bits + 3 * len(pad)) % 8 == 0:
        pad.append(1)  # the 2-bit codeword
    head = np.concatenate([head, np.array(pad, np.uint8)])
    assert int(len_t[head].astype(np.int64).sum()) % 8 in (2, 4, 6)
    text = np.concatenate([head, flat[rng.integers(0, flat.size, size=n_flat)], head[:1000]]).astype(np.uint8)
    return data_t, len_t, text


def _skewed_flat_tree_dictionary():
    """_skewed_flat_dictionary's relative that the TREE WALK plans for: the same skewed and flat codewords, no filler, and every
    bit pattern under prefix 1 that is no flat codeword's given to a short codeword of its own -- 1x0, 1x1x0, 1x1x1x0 (the bytes
    40 .. 53: in no text, and a walk that stands at an even offset inside flat codewords, which reads flat codewords only,
    never reads one).  The table is complete: 35 internal nodes, nothing unmatched, no hole for the walk to make a leaf of.
    -> (data, length, the skewed symbols, the flat symbols)."""
    data_t, len_t, skewed, flat = _skewed_flat_dictionary()
    data_t, len_t = data_t.copy(), len_t.copy()
    data_t[120:220], len_t[120:220] = 0, 0
    s = 40
    for k in (1, 2, 3):  # 1x 0, 1x1x 0, 1x1x1x 0
        for j in range(1 << k):
            x = [(j >> i) & 1 for i in range(k - 1, -1, -1)]
            data_t[s], len_t[s] = int("".join("1%d" % b for b in x) + "0", 2), 2 * k + 1
            s += 1
    assert s == 54 and sum(2.0 ** -int(l) for l in len_t if l) == 1.0
    return data_t, len_t, skewed, flat


PERIOD_DICTIONARIES = {"windows": _skewed_flat_dictionary, "tree_walk": _skewed_flat_tree_dictionary}
PERIOD_BLOCK_BITS = 65_536  # the decode's 8 KiB blocks
ISLAND_FLAT, ISLAND_AT_BIT = 1_500, 20_000  # island()'s stretch; where in its block it begins (about: 2, 4 or 6 bits behind a byte boundary)


def _skewed_up_to(rng, bits):
    """Random skewed symbols of _skewed_flat_dictionary, as many of the draw as fit into `bits` bits -> (symbols, their bits)."""
    _, len_t, skewed, _ = _skewed_flat_dictionary()
    run = skewed[np.minimum(rng.geometric(0.5, size=bits // 2 + 1) - 1, skewed.size - 1)]
    cum = np.cumsum(len_t[run].astype(np.int64))
    n = int(np.searchsorted(cum, bits, side="right"))
    return run[:n], int(cum[n - 1]) if n else 0


def _skewed_fill(rng, bits, flat_follows=False, begins_at=0):
    """Skewed symbols that fill EXACTLY `bits` bits: a random run, its tail the 2- and 3-bit codewords.  flat_follows: not
    exactly -- up to 13 bits fewer, padded as _skewed_run pads so that a run which begins at bit begins_at ends 2, 4 or 6 bits
    behind a byte boundary."""
    run, used = _skewed_up_to(rng, bits - 8)
    if flat_follows:
        pad, end = [], begins_at + used
        if end % 2:
            pad.append(2)  # the 3-bit codeword
        if (end + 3 * len(pad)) % 8 == 0:
            pad.append(1)  # the 2-bit codeword
        return np.concatenate([run, np.array(pad, np.uint8)])
    left = bits - used
    assert left >= 8
    tail = [2] * (left % 2) + [1] * ((left - 3 * (left % 2)) // 2)
    return np.concatenate([run, np.array(tail, np.uint8)])


def periodic_islands(dictionary, period_blocks, island_block=None, seed=11):
    """-> (data, length, period_text, period_body): ONE period of a stream that is tiled on the device -- skewed symbols, one
    stretch that cannot settle (island()'s: ISLAND_FLAT flat symbols laid 2, 4 or 6 bits behind a byte boundary), skewed
    symbols, EXACTLY period_blocks * 65 536 bits, the tail trimmed with the 2- and 3-bit codewords.  So the oracle's pack of the
    period is whole 8 KiB blocks without a pad bit, N copies of those bytes are the body of N copies of the text, and every
    copy lies on the block grid as the first does.  The stretch lies inside block island_block of the period (default: the
    middle one), from about bit ISLAND_AT_BIT of it.  dictionary: "windows" (_skewed_flat_dictionary) or "tree_walk"
    (_skewed_flat_tree_dictionary).  tests/test_repairs_host.py checks all of that, and which blocks give up, on the host."""
    from oracle import oracle as O

    data_t, len_t, _, flat = PERIOD_DICTIONARIES[dictionary]()
    island_block = period_blocks // 2 if island_block is None else island_block
    assert 0 <= island_block < period_blocks and ISLAND_AT_BIT + 8 * ISLAND_FLAT + 4_096 < PERIOD_BLOCK_BITS
    rng = np.random.default_rng(seed)
    head = _skewed_fill(rng, island_block * PERIOD_BLOCK_BITS + ISLAND_AT_BIT, True)
    middle = flat[rng.integers(0, flat.size, size=ISLAND_FLAT)]
    used = int(len_t[head].astype(np.int64).sum()) + 8 * ISLAND_FLAT
    assert used % 8 in (2, 4, 6)
    text = np.concatenate([head, middle, _skewed_fill(rng, period_blocks * PERIOD_BLOCK_BITS - used)]).astype(np.uint8)
    body, end_bit = O.pack_body(data_t, len_t, text)
    assert end_bit == period_blocks * PERIOD_BLOCK_BITS and len(body) * 8 == end_bit
    return data_t, len_t, text, body


def failed_run_ins(n_blocks, flat_symbols=40, lead_bits=200, seed=13):
    """-> (data, length, text): a stream of n_blocks 8 KiB blocks (and a few bytes) under _skewed_flat_dictionary in which
    EVERY block seam lies inside a SHORT flat stretch: skewed symbols up to some lead_bits in front of the seam, flat_symbols
    flat ones 2, 4 or 6 bits behind a byte boundary (320 bits: the 128-bit blind run-in of the block's first lane begins inside
    them, in a phase that never meets the truth, and is still inside them at the seam -- the lane begins where no codeword
    does), skewed symbols again.  The stretch ends inside the lane it misleads, and the skewed symbols behind it bring that
    lane's walk to the true chain within a few lanes (tests/test_repairs_host.py: within 1 024 bits): nobody gives up, no
    block's exit moves, and every seam that no workgroup of the first sweep settles within itself goes on the worklist of the
    second.  The same holds with the block grid 8 or 24 bits off (a body 1 or 3 bytes behind an aligned address)."""
    data_t, len_t, _, flat = _skewed_flat_dictionary()
    rng = np.random.default_rng(seed)
    parts, used = [], 0
    for b in range(1, n_blocks):
        run = _skewed_fill(rng, b * PERIOD_BLOCK_BITS - lead_bits - used, True, used)
        parts += [run, flat[rng.integers(0, flat.size, size=flat_symbols)]]
        used += int(len_t[run].astype(np.int64).sum()) + 8 * flat_symbols
        assert used % 8 in (2, 4, 6) and b * PERIOD_BLOCK_BITS + 64 < used < b * PERIOD_BLOCK_BITS + 8 * flat_symbols - 128
    parts.append(_skewed_up_to(rng, n_blocks * PERIOD_BLOCK_BITS + 1_000 - used)[0])
    return data_t, len_t, np.concatenate(parts).astype(np.uint8)
