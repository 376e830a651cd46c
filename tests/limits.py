"""Code tables and texts that reach the worst cases the kernels are sized for: 32-bit codewords in full trees, chained decode
tables narrowed to two index bits, encode rounds in which every symbol has the longest code, and the 16-byte chunks that send
K4's append down each of its three paths.  A plain module like guards.py, imported by name; tests/test_limits_host.py checks
(without a GPU) that every input here still reaches its limit, tests/test_gpu_limits.py runs them on the device."""
import functools

import numpy as np

from tests.test_shared_host import canonical, table_ladder

ROUND = 4096  # bytes of text per K4 round: 256 lanes x one 16-byte chunk
CHUNK = 16
Z = "Z"  # in a chunk pattern: a byte the table has no code for (length 0); et_encode_body_device alone accepts it


class Table:
    """data[256] u32, length[256] u8 and the symbols by length.  complete: a full prefix-free tree of codes up to 32 bits."""

    def __init__(self, name, data, length, complete=True):
        self.name, self.data, self.length, self.complete = name, np.asarray(data, np.uint32), np.asarray(length, np.uint8), complete
        self.max_len = int(self.length.max())
        self.coded = np.flatnonzero(self.length).astype(np.uint8)
        self.uncoded = int(np.flatnonzero(self.length == 0)[0]) if (self.length == 0).any() else None

    @property
    def tab(self):
        return self.data, self.length

    def of_len(self, l):
        """The table's symbols of length l, in symbol order."""
        return np.flatnonzero(self.length == l).astype(np.uint8)

    def sym(self, l):
        """The table's (first) symbol of length l; Z: a byte without a code."""
        if l == Z:
            assert self.uncoded is not None
            return self.uncoded
        s = self.of_len(l)
        assert s.size, f"{self.name} has no code of {l} bits"
        return int(s[0])

    def codebook(self):
        import entreepy_amd as E

        return E.Codebook.from_tables(self.data, self.length)

    def bits(self, text):
        return self.length[np.asarray(text, np.uint8)].astype(np.int64)


def _from_codes(name, codes, first_symbol=1):
    """[(code, length)] -> Table; symbols first_symbol, first_symbol + 1, ... in the order given."""
    data, length = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    assert first_symbol + len(codes) <= 256
    for i, (c, l) in enumerate(codes):
        assert 1 <= l <= 32 and 0 <= c < 1 << l
        data[first_symbol + i], length[first_symbol + i] = c, l
    return Table(name, data, length)


def _ladder_codes(prefix, depth, first, last):
    """Under the node `prefix` (depth bits): leaves of lengths first, first + 1, ..., last - 1, last, last -- a run of ones with
    a zero at its end, and the run of ones itself."""
    codes = []
    for l in range(first, last):
        k = l - depth  # k - 1 ones and a zero
        codes.append((((prefix << k) | ((1 << (k - 1)) - 1) << 1), l))
    k = last - depth
    codes.append(((prefix << k) | (((1 << (k - 1)) - 1) << 1), last))
    codes.append(((prefix << k) | ((1 << k) - 1), last))
    return codes


@functools.lru_cache(maxsize=None)
def ladder32():
    """Lengths 1 .. 31, 32, 32 (the bytes 100 .. 132): tests/test_shared_host.py's table_ladder."""
    return Table("ladder32", *table_ladder())


@functools.lru_cache(maxsize=None)
def ladder31():
    """Lengths 1 .. 30, 31, 31 (the bytes 100 .. 131)."""
    return Table("ladder31", *canonical({100 + i: min(i + 1, 31) for i in range(32)}))


@functools.lru_cache(maxsize=None)
def broom32():
    """A ladder 1 .. 27 (the bytes 100 .. 126) and a complete 5-level subtree under its last node: 32 codewords of 32 bits
    (the bytes 127 .. 158), the 27 ones followed by every 5-bit value."""
    t = Table("broom32", *canonical({**{100 + i: i + 1 for i in range(27)}, **{127 + j: 32 for j in range(32)}}))
    assert [int(c) for c in t.data[127:159]] == [0xFFFFFFE0 + j for j in range(32)]
    return t


def _comb(name, n_ladders):
    """A ladder 1 .. 7; under 1111111 a 4-bit split into 16 nodes at depth 11; the first n_ladders of them carry a ladder down
    to depth 32 (lengths 12 .. 31, 32, 32), the others are leaves of 11 bits."""
    codes = [(((1 << (l - 1)) - 1) << 1, l) for l in range(1, 8)]
    for j in range(16):
        node = (0x7F << 4) | j
        codes += _ladder_codes(node, 11, 12, 32) if j < n_ladders else [(node, 11)]
    return _from_codes(name, codes)


@functools.lru_cache(maxsize=None)
def comb8():
    return _comb("comb8", 8)


@functools.lru_cache(maxsize=None)
def comb11():
    """254 symbols, 253 internal nodes: the most ladders that fit a table of 256 byte values less one uncoded."""
    return _comb("comb11", 11)


def mirror(t):
    """Every code of t complemented within its length: the same shape, not canonical, its long codes runs of zeros."""
    l = t.length.astype(np.uint64)
    mask = np.where(l > 0, (np.uint64(1) << l) - np.uint64(1), np.uint64(0))
    return Table("mirror_" + t.name, ((~t.data.astype(np.uint64)) & mask).astype(np.uint32), t.length)


@functools.lru_cache(maxsize=None)
def long255():
    """Not a prefix code, for the encode alone: the lengths of test_gpu_parity.py's test_long_codes_beyond_32_bits under random
    code words; the symbols 9, 19, 29 and 39 have 255 bits."""
    rng = np.random.default_rng(9)
    data, length = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    for s in range(40):
        data[s] = rng.integers(0, 1 << 32, dtype=np.uint64)
        length[s] = [1, 5, 31, 32, 33, 40, 64, 65, 100, 255][s % 10]
    return Table("long255", data, length, complete=False)


def complete_tables():
    return [ladder32(), ladder31(), broom32(), comb8(), comb11(), mirror(ladder32()), mirror(comb11())]


def all_tables():
    return complete_tables() + [long255()]


def table(name):
    return {t.name: t for t in all_tables()}[name]


# --- texts ------------------------------------------------------------------------------------------------------------------------


def dense(t, n, seed=0x11A175):
    """Every byte a longest-code symbol, drawn among the table's."""
    longest = t.of_len(t.max_len)
    return longest[np.random.default_rng(seed).integers(0, longest.size, size=n)]


def alternating(t, n, seed=0x11A176):
    """Rounds of 4096 longest-code symbols alternating with rounds of the shortest-code (1-bit) symbol."""
    text = dense(t, n, seed)
    short = t.sym(int(t.length[t.length > 0].min()))
    odd = (np.arange(n) // ROUND) % 2 == 1
    text[odd] = short
    return text


def phases(t, n):
    """[S(max), S(k)] for k cycling through the table's lengths below max, repeated: the longest codeword begins at every bit
    offset.  The longest-code symbols take turns."""
    longest = t.of_len(t.max_len)
    ks = [l for l in range(1, t.max_len) if t.of_len(l).size]
    pairs = (n + 1) // 2
    text = np.empty(2 * pairs, np.uint8)
    text[0::2] = longest[np.arange(pairs) % longest.size]
    text[1::2] = np.array([t.sym(k) for k in ks], np.uint8)[np.arange(pairs) % len(ks)]
    return text[:n]


def uniform(t, n, seed=0x11A177):
    """Uniform over the table's symbols."""
    return t.coded[np.random.default_rng(seed).integers(0, t.coded.size, size=n)]


TEXTS = {"dense": dense, "alternating": alternating, "phases": phases, "uniform": uniform}


def starts(t, text, first_bit=0):
    """Bit offset at which every codeword of the text begins."""
    b = t.bits(text)
    return first_bit + np.cumsum(b) - b


def straddles(t, text, every_bits, first_bit=0):
    """How many longest codewords begin in front of a multiple of every_bits and end behind it."""
    s = starts(t, text, first_bit)
    b = t.bits(text)
    return int(np.count_nonzero((s // every_bits != (s + b - 1) // every_bits) & (b == t.max_len)))


# --- K4's three append paths (part 3 of the issue) ------------------------------------------------------------------------------------

QUAD, PAIR, SINGLE = "quad", "pair", "single"
K4_PATTERNS = [
    (QUAD, (8, 8, 8, 8)), (QUAD, (1, 1, 1, 29)), (QUAD, (29, 1, 1, 1)), (QUAD, (16, 16, Z, Z)), (QUAD, (Z, Z, 16, 16)), (QUAD, (32, Z, Z, Z)), (QUAD, (Z, Z, Z, 32)),
    (PAIR, (8, 8, 8, 9)), (PAIR, (1, 31, 31, 1)), (PAIR, (16, 16, 16, 16)), (PAIR, (32, Z, Z, 32)), (PAIR, (Z, 32, 32, Z)),
    (SINGLE, (32, 1, 1, 1)), (SINGLE, (1, 32, 1, 1)), (SINGLE, (2, 31, 1, 1)), (SINGLE, (32, 32, 32, 32)),
]
K4_LANES = (0, 31, 63, 255)


def pattern_id(quad):
    return "-".join(str(x) for x in quad)


def k4_path(lengths16):
    """The append path K4 takes for a full chunk of these 16 code lengths, were every lane of the wavefront like it: whole quads
    when every quad is at most 32 bits, pairs when a quad is wider but no pair of a wide quad is, single symbols otherwise."""
    l = [0 if x == Z else int(x) for x in lengths16]
    assert len(l) == CHUNK
    quads = [sum(l[4 * q : 4 * q + 4]) for q in range(4)]
    if max(quads) <= 32:
        return QUAD
    wide_pair = any(quads[q] > 32 and (l[4 * q] + l[4 * q + 1] > 32 or l[4 * q + 2] + l[4 * q + 3] > 32) for q in range(4))
    return SINGLE if wide_pair else PAIR


def chunk_of(t, lengths16):
    return np.array([t.sym(x) for x in lengths16], np.uint8)


def k4_whole_rounds(t, quad, n):
    """The quad in every quad position of every chunk."""
    return np.resize(chunk_of(t, tuple(quad) * 4), n)


def k4_chunk_lengths(quad, position):
    """The 16 lengths of a chunk of 1-bit symbols with `quad` in quad position `position`."""
    l = [1] * CHUNK
    l[4 * position : 4 * position + 4] = quad
    return tuple(l)


def k4_one_chunk(t, quad, n, lane, position):
    """1-bit symbols throughout, but for the chunk of lane `lane` in every full round, whose quad `position` is the quad."""
    text = np.full(n, t.sym(1), np.uint8)
    special = chunk_of(t, k4_chunk_lengths(quad, position))
    for r in range(n // ROUND):
        at = r * ROUND + lane * CHUNK
        text[at : at + CHUNK] = special
    return text


# --- the 31 / 32 / 33-bit boundary behind the host's own code construction (part 6) -------------------------------------------------


def fibonacci_histogram(max_len):
    """The lightest counts whose code tree (oracle build_dict, and so et_build_codebook) is max_len levels deep: 1, 1, 1, 3, 4,
    7, 11, 18, ... -- every count one more than the sum of all counts but the one in front of it.  The builder keeps leaves and
    merged nodes in two queues and takes the LEAF when the two fronts weigh the same, so the merged node so far goes into the
    next merge only if the leaf after next is strictly heavier than it; Fibonacci's own 1, 1, 2, 3, 5, ... satisfy that too
    but weigh a fifth more, and 1, 1, 1, 2, 3, 5, ... tie and give two chains of half the depth.  tests/test_limits_host.py
    pins the depths."""
    counts = [1, 1, 1]
    while len(counts) < max_len + 1:
        counts.append(1 + sum(counts[:-1]))
    hist = np.zeros(256, np.uint64)
    hist[40 : 40 + len(counts)] = counts
    return hist


def fibonacci_text(max_len, seed=0x11A178):
    hist = fibonacci_histogram(max_len)
    text = np.repeat(np.arange(256, dtype=np.uint8), hist.astype(np.int64))
    np.random.default_rng(seed).shuffle(text)
    return text


# --- which (table, text) pairs the GPU tests run (tests/test_limits_host.py round-trips the same ones through the oracle) -----------

K4_N = 2 * ROUND + 17    # part 3: two rounds and a partial chunk
RING_N = 5 * ROUND + 17  # part 4
DECODE_N = 24_000        # part 5: three to twelve 8 KiB blocks
COLD_N = 16_000          # part 5, cold ranges: at least four 8 KiB blocks
RING_PAIRS = [(name, text) for name in ("ladder31", "ladder32", "broom32") for text in ("dense", "alternating")] + [("long255", "dense")]
DECODE_TABLES = ["ladder32", "ladder31", "broom32", "comb8", "comb11", "mirror_ladder32", "mirror_comb11"]
DECODE_TEXTS = ["dense", "phases", "uniform"]
DECODE_PAIRS = [(name, text) for name in DECODE_TABLES for text in DECODE_TEXTS]
COLD_PAIRS = [("ladder32", "phases"), ("comb11", "uniform")]
# a seed other than the text's default: the first after 0x11A180 that puts a 32-bit codeword of uniform(comb11) across a boundary
# between the block ranges of 2 ranks AND of 3 (one codeword in twelve has 32 bits; tests/test_limits_host.py pins it)
SEEDS = {("comb11", "uniform", COLD_N): 0x11A22C}


@functools.lru_cache(maxsize=None)
def text_of(table_name, text_name, n):
    """The text of a pair, made once and shared; read-only."""
    seed = SEEDS.get((table_name, text_name, n))
    x = TEXTS[text_name](table(table_name), n) if seed is None else TEXTS[text_name](table(table_name), n, seed)
    x.setflags(write=False)
    return x
