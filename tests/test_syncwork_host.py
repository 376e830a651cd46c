"""The serial reference of tests/bitwalk.py against the oracle, and the inputs of tests/test_gpu_syncwork.py against what that
file says of them -- checked on the host, so that a fixture which stops being what the GPU tests take it for fails HERE: the
walk from the true start decodes what the oracle decodes, the planner sends every fixture to the family its test expects, the
streams declared clean for the tree walk satisfy the condition that makes them so, and a start that is one bit off is visible
to the reference on every fixture.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from oracle import oracle as O
from tests import bitwalk as W
from tests import corpus
from tests.guards import _flat200_dictionary, _skewed_flat_dictionary, _small_holed_dictionary, _sparse_dictionary, image_under, island, skewed_then_flat, sparse_text
from tests.test_gpu_rowsync import flat

# name -> (the family a whole-stream decode starts on, as et_decode_path names it; declared clean for the tree walk)
FIXTURES = {
    "text": (N.ET_PATH_TREE_WALK, True),
    "midsummer": (N.ET_PATH_TREE_WALK, True),
    "enwik": (N.ET_PATH_TREE_WALK, True),
    "two_len_quick": (N.ET_PATH_TREE_WALK, False),  # 6 and 7 bits: the quick rule lets the tree walk try; three lanes are far from the truth
    "two_len_slow": (N.ET_PATH_EXIT_MAPS, False),   # 120 symbols of equal weight, 6 and 7 bits (tests/test_gpu_fixedsync.py: quick=False)
    "rows": (N.ET_PATH_ROWS, False),                # 255 symbols: one 7-bit codeword, 254 of 8 bits
    "fixed": (N.ET_PATH_FIXED, False),              # 16 codewords of 4 bits
    "sparse": (N.ET_PATH_WINDOWS, False),           # tests/guards.py: no tree the walk can hold
}
# the fixtures of tests/test_gpu_windows.py, all under hand-made tables with bit patterns that are nobody's codeword (the reference
# follows them by the window kernels' rule, Stream(skip=True)): name -> the family a whole-stream decode starts on
WINDOW_FIXTURES = {
    "sparse_big": N.ET_PATH_WINDOWS,    # the sparse recipe over 36 blocks and more: ranges of 16 blocks and beyond
    "holes200": N.ET_PATH_EXIT_MAPS,    # 200 codes of 8 bits, 5 blocks + 17 bytes
    "skewed_flat": N.ET_PATH_WINDOWS,   # tests/guards.py skewed_then_flat: the even phases of its flat half never merge
    "island_first": N.ET_PATH_WINDOWS,  # tests/guards.py island: ONE block that does not settle among 144
    "island_middle": N.ET_PATH_WINDOWS,
    "island_last": N.ET_PATH_WINDOWS,
}
SPARSE_BIG_SYMBOLS = 265_000
CLEAN_BELOW = W.LANE_BITS + W.RUN_IN_BITS  # a lane that is on the true chain before it leaves its own bits
BODY_LAYOUTS = [(shift, start_bit) for shift in range(4) for start_bit in (0, 5)]  # decode_body_device: the pointer's low bits, the start bit
BIG_SLOW_SYMBOLS = 2_460_000  # two_len_slow over more than 256 blocks: more than one group of exit maps


def _text_of(name):
    if name == "text":
        return corpus.text_like(200_000, 61)
    if name == "midsummer":
        return np.frombuffer(corpus.midsummer(), dtype=np.uint8)
    if name == "enwik":
        return corpus.enwik_like(200_000, 5)
    if name == "two_len_quick":
        return corpus.uniform(150_000, 32, 10, 110)
    if name == "two_len_slow":
        return flat(120, 150_000, 420)
    if name == "two_len_slow_big":
        return flat(120, BIG_SLOW_SYMBOLS, 421)
    if name == "rows":
        return corpus.uniform(150_000, 9, 1, 256)
    if name == "fixed":
        return flat(16, 150_000, 76)
    raise KeyError(name)


class Stream:
    """A stream as the range calls see it: `stream`, its bytes from the 4-byte aligned word the body starts in; first_bit, where
    the first codeword begins in it; the code table; the text.  And the reference's view of it, worked out once and read-only:
    L, S (bitwalk.next_table), `at` (the bit every whole codeword of the true chain begins at, those in the pad bits included),
    on_chain (one flag per bit).  skip: the reference follows the window kernels' rule for bit patterns without a codeword
    (bitwalk: unmatched="skip") -- L is 1 there, C says where a codeword begins, and every walk over L is handed C; else C is
    None."""

    def __init__(self, name, data, length, text, stream, first_bit, comp=None, body_off=None, skip=False):
        self.name, self.data, self.length, self.text = name, np.asarray(data, np.uint32), np.asarray(length, np.uint8), np.asarray(text, np.uint8)
        self.stream, self.first_bit, self.comp, self.body_off = np.frombuffer(bytes(stream), dtype=np.uint8), first_bit, comp, body_off
        self.n_bytes, self.n_bits = self.stream.size, self.stream.size * 8
        self.shift, self.start_bit = first_bit // 8, first_bit % 8  # the body lies `shift` bytes into the stream and begins at bit start_bit of that byte
        self.n_blocks = (self.n_bytes + W.BLOCK_BYTES - 1) // W.BLOCK_BYTES
        self.L, self.S, self.C = W.next_table(self.stream, self.data, self.length, "skip") if skip else (*W.next_table(self.stream, self.data, self.length), None)
        _, self.at = W.walk_positions(self.L, first_bit, self.n_bits, self.C)
        self.on_chain = W.chain(self.L, first_bit, self.at)
        for a in (self.L, self.S, self.at, self.on_chain) + ((self.C,) if skip else ()):
            a.setflags(write=False)
        self._Lb, self._Cb, self._walks = self.L.tobytes(), self.C.tobytes() if skip else None, {}

    def codebook(self):
        return E.Codebook.from_tables(self.data, self.length)

    def true_start(self, begin):
        """Where the first codeword of the range that begins at byte `begin` begins, bits from there."""
        i = np.searchsorted(self.at, begin * 8)
        return int(self.at[i]) - begin * 8 if i < self.at.size else 0

    def truth(self, begin, end):
        """-> (start_bit, exit_bit, n_symbols, symbols) of the range [begin, end) bytes, from the true chain."""
        i, j = np.searchsorted(self.at, begin * 8), np.searchsorted(self.at, end * 8)
        exit_bit = int(self.at[j]) - end * 8 if j < self.at.size else 0  # (a codeword the stream's end cuts: nobody's, the walk ends there)
        return self.true_start(begin), exit_bit, int(j - i), self.S[self.at[i:j]]

    def block_walk(self, b, off):
        """The serial walk of block b from its bit `off` to its end (the stream's, for the last block) -> (exit, in bits behind
        that end; the bits at which the counted codewords begin).  Kept: walks from different starts soon are the same walk."""
        if (b, off) not in self._walks:
            end = min((b + 1) * W.BLOCK_BYTES, self.n_bytes) * 8
            exit_, at = W.walk_positions(self._Lb, b * W.BLOCK_BITS + off, end, self._Cb)
            at.setflags(write=False)
            self._walks[b, off] = (exit_ - end, at)
        return self._walks[b, off]

    def range_walk(self, begin, end, start):
        """-> (exit_bit, at): the serial walk from bit `start` of the range [begin, end) bytes, a range of whole blocks or one
        that ends with the stream, block by block."""
        assert begin % W.BLOCK_BYTES == 0 and (end % W.BLOCK_BYTES == 0 or end == self.n_bytes) and begin < end
        off, ats = start, []
        for b in range(begin // W.BLOCK_BYTES, (end + W.BLOCK_BYTES - 1) // W.BLOCK_BYTES):
            off, at = self.block_walk(b, off)
            ats.append(at)
        return off, np.concatenate(ats)

    def range_count(self, begin, end, start):
        """range_walk's (exit_bit, number of codewords)."""
        exit_bit, at = self.range_walk(begin, end, start)
        return exit_bit, at.size

    def cuts(self, widths=(1, 2, 5)):
        """Ranges of 1, 2 and 5 blocks at every block boundary, as (begin, end) in bytes; those that reach the stream's end
        end with it (ragged, no tail)."""
        out = []
        for w in widths:
            for b in range(self.n_blocks):
                r = (b * W.BLOCK_BYTES, min((b + w) * W.BLOCK_BYTES, self.n_bytes))
                if r not in out:
                    out.append(r)
        return out


@functools.lru_cache(maxsize=None)
def fixture(name):
    """The fixture `name`, made once and shared; read-only."""
    if name in ("sparse", "sparse_big"):  # the dictionary and text of test_fallback_sweeps_and_write_are_what_a_sparse_dictionary_runs, n = 60 000
        data_t, len_t, _ = _sparse_dictionary()
        n = {"sparse": 60_000, "sparse_big": SPARSE_BIG_SYMBOLS}[name]
        text = sparse_text(n, n)
        body, _ = O.pack_body(data_t, len_t, text)
        return Stream(name, data_t, len_t, text, body, 0, comp=body, body_off=0, skip=True)
    if name.startswith("junk/"):  # the first 6 blocks and 100 bytes of junk_stream: ranges whose INTERIOR blocks hold patterns that are nobody's
        whole = junk_stream(name[len("junk/") :])
        body = whole.stream[: 6 * W.BLOCK_BYTES + 100].tobytes()
        return Stream(name, whole.data, whole.length, np.zeros(0, np.uint8), body, 0, comp=body, body_off=0, skip=True)
    if name == "holes200":  # the flat table of test_fallback_block_bookkeeping_flat_table: the text is its own body
        data_t, len_t = _flat200_dictionary()
        text = np.random.default_rng(17).integers(0, 200, size=5 * W.BLOCK_BYTES + 17).astype(np.uint8)
        return Stream(name, data_t, len_t, text, text.tobytes(), 0, comp=text.tobytes(), body_off=0, skip=True)
    if name == "skewed_flat" or name.startswith("island_"):
        data_t, len_t, text = skewed_then_flat() if name == "skewed_flat" else island(name[len("island_") :])
        comp = image_under(data_t, len_t, text)
        _, n_symbols, body_off = E.parse_header(comp)
        assert n_symbols == text.size
        return Stream(name, data_t, len_t, text, comp[body_off & ~3 :], (body_off & 3) * 8, comp=comp, body_off=body_off, skip=True)
    text = _text_of(name)
    comp = O.encode(text)[4:]
    cb, n_symbols, body_off = E.parse_header(comp)
    assert n_symbols == text.size
    return Stream(name, cb.data, cb.length, text, comp[body_off & ~3 :], (body_off & 3) * 8, comp=comp, body_off=body_off)  # (device tensors are 4-byte aligned)


@functools.lru_cache(maxsize=None)
def body_layout(name, shift, start_bit):
    """The fixture's text packed from start_bit into a body that lies `shift` bytes behind a 4-byte aligned address: what
    decode_body_device sees, as a Stream (its body is stream[shift:])."""
    fx = fixture(name)
    body, end_bit = O.pack_body(fx.data, fx.length, fx.text, start_bit)
    body = body[: (end_bit + 7) // 8]
    return Stream(f"{name}+{shift}.{start_bit}", fx.data, fx.length, fx.text, bytes(shift) + body, shift * 8 + start_bit, comp=body)


def decode_path(cb):
    p = ctypes.c_uint32(99)
    assert N.lib().et_decode_path(ctypes.byref(cb.raw), ctypes.byref(p)) == N.ET_OK
    return p.value


@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_walk_from_the_true_start_is_the_oracles_decode(name):
    fx = fixture(name)
    n = fx.text.size
    exit_, syms = W.walk_symbols(fx.L, fx.S, fx.first_bit, fx.n_bits, fx.C)
    assert fx.n_bits <= exit_ < fx.n_bits + 32 and n <= syms.size <= n + 7  # (whole codewords in the pad bits are decoded too)
    image = fx.comp if name != "sparse" else fx.codebook().header(n)[4:] + fx.comp
    assert syms[:n].tobytes() == O.decode(image) == fx.text.tobytes()
    bounds = W.boundaries(fx.first_bit, fx.length, fx.text)
    assert np.array_equal(fx.at[:n], bounds[:-1]) and (fx.at.size == n or fx.at[n] == bounds[-1])
    assert np.array_equal(fx.L[bounds[:-1]], fx.length[fx.text]) and np.array_equal(fx.S[bounds[:-1]], fx.text)
    assert W.walk(fx.L, fx.first_bit, fx.n_bits, fx.C) == (exit_, syms.size)
    # the same through the pointer-doubling variant, for the whole stream and for every cut of it
    jumps = W.Jumps(fx.L, fx.C)
    assert [int(x[0]) for x in jumps.walk([fx.first_bit], [fx.n_bits])] == [exit_, syms.size]
    cuts = fx.cuts()
    assert len(cuts) >= 3 * fx.n_blocks - 5 and sum(1 for _, e in cuts if e == fx.n_bytes) >= 1
    starts = np.array([b * 8 + fx.true_start(b) for b, _ in cuts])
    ends = np.array([e * 8 for _, e in cuts])
    exits, counts = jumps.walk(starts, ends)
    for (b, e), x, c in zip(cuts, exits, counts):
        s, exit_bit, n_sym, syms = fx.truth(b, e)
        assert (int(x) - e * 8, int(c)) == (exit_bit, n_sym) == (W.walk(fx.L, b * 8 + s, e * 8, fx.C)[0] - e * 8, syms.size), (b, e)
        assert (exit_bit, n_sym) == fx.range_count(b, e, s), (b, e)
        assert s < 32 and exit_bit < 32


@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_planner_sends_every_fixture_where_its_gpu_test_expects(name):
    fx = fixture(name)
    cb = fx.codebook()
    assert decode_path(cb) == FIXTURES[name][0]
    t = ctypes.c_uint32(999)
    rc = N.lib().et_row_code(ctypes.byref(cb.raw), ctypes.byref(t))
    if name == "rows":  # 255 symbols: 256 - 255 seven-bit codewords; the range calls' maps have 8 entries
        assert rc == N.ET_OK and t.value == 1 and cb.raw.max_length == 8 and cb.raw.min_length == 7
    elif name != "fixed":  # (16 codewords of 4 bits are no row code either; the planner asks about fixed lengths first)
        assert rc == N.ET_ERR_UNSUPPORTED
    lens = sorted(set(fx.length[fx.length > 0].tolist()))
    want = {"two_len_quick": [6, 7], "two_len_slow": [6, 7], "rows": [7, 8], "fixed": [4], "sparse": [2, 16]}.get(name)
    assert want is None or lens == want
    if name == "enwik":
        assert lens[-1] >= 18  # codes a 12-bit lookup misses
    if name != "sparse":
        assert cb.is_complete()
    assert 8 <= fx.n_blocks <= 19 and fx.n_bytes % W.BLOCK_BYTES  # inner blocks, a ragged last one, several ranges


def test_the_big_two_length_stream_has_more_than_one_group_of_blocks():
    n_bits = int(fixture("two_len_slow").length[_text_of("two_len_slow_big")].astype(np.int64).sum())
    assert n_bits // 8 > 258 * W.BLOCK_BYTES  # a range of 257 blocks and at least a block behind it


@pytest.mark.parametrize("name", [k for k, v in FIXTURES.items() if v[1]])
def test_clean_fixtures_meet_the_tree_walks_condition(name):
    """Every lane's blind run-in (128 bits in front of its own 512) is on the true chain before the lane's own bits end: the
    largest merge distance is below 640.  Then every lane leaves its bits on the true chain at its first attempt, one more trip
    hands every lane its true start, no block gives up, and the verification passes: sync_iters is the family's base."""
    fx = fixture(name)
    d = W.merge_distances(fx.L, fx.on_chain)
    print(f"{name}: max merge distance {int(d.max())} bits over {d.size} lanes")
    assert d.size == (fx.n_bits + 511) // 512 and int(d.max()) < CLEAN_BELOW


def test_clean_condition_of_the_body_layouts_and_not_of_the_two_length_stream():
    for shift, start_bit in BODY_LAYOUTS:
        fx = body_layout("text", shift, start_bit)
        assert int(W.merge_distances(fx.L, fx.on_chain).max()) < CLEAN_BELOW, (shift, start_bit)
    fx = fixture("two_len_quick")  # NOT declared clean: tests/test_gpu_syncwork.py asserts only "at least the base" for it
    d = W.merge_distances(fx.L, fx.on_chain)
    assert int(np.count_nonzero(d >= CLEAN_BELOW)) >= 1 and int(d.max()) < W.NEVER


def test_merge_distances_on_a_stream_small_enough_to_follow():
    """Codewords 0, 10, 11 under the text 10 x 40, 0, 11 x 23: true boundaries at the even bits up to 80, at the odd ones from
    81 on; one pad bit, a zero, which is a whole codeword of its own."""
    data, length = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    data[1], length[1] = 0b0, 1
    data[2], length[2] = 0b10, 2
    data[3], length[3] = 0b11, 2
    text = np.array([2] * 40 + [1] + [3] * 23, np.uint8)  # 128 bits: boundaries at even bits up to 80, at odd ones from 81 on
    body, end = O.pack_body(data, length, text)
    assert end == 127
    L, S = W.next_table(body, data, length)
    on = W.chain(L, 0)
    assert W.walk(L, 0, 127) == (127, 64) and W.walk_symbols(L, S, 0, 127)[1].tobytes() == text.tobytes()
    assert W.walk(L, 0, 128) == (128, 65) and W.walk(L, 0, 81) == (81, 41) and W.walk(L, 0, 82) == (83, 42)
    # lanes of 32 bits with a run-in of 7: the walks begin at bits 25, 57, 89.  From 25, an odd bit of 1010...: "0", and the
    # walk stands on 26, a true boundary; from 57 likewise; 89 is a true boundary itself.
    assert W.merge_distances(L, on, lane_bits=32, run_in_bits=7).tolist() == [0, 1, 1, 0]
    # from bit 82, an even bit behind the phase change, the walk reads 11 from even bits, then 10 over the pad bit, and never
    # stands on an odd bit: it leaves the stream, 46 bits on
    assert W.merge_distances(L, on, lane_bits=96, run_in_bits=14).tolist() == [0, 46]
    assert W.walk(L, 82, 127) == (128, 23)
    # runs of lanes that leave their own bits off the chain, per block of lanes: a block's first lane begins a run anew
    assert W.unsettled_runs([0, 700, 640, 0, 639, 700, 700, 700, 700], lanes_per_block=4).tolist() == [2, 3, 1]
    # a codeword the stream's end cuts is nobody's: without the pad bit, 11 from bit 125 is whole and 1 at bit 127 is cut
    assert W.walk(L[:127], 81, 127) == (127, 23) and W.walk(L[:127], 82, 127) == (127, 22)
    with pytest.raises(W.Unmatched):  # a table without the codeword 0: nothing begins at bit 80
        W.walk(W.next_table(body + bytes(8), data[:3].tolist() + [3] + [0] * 252, [0, 0, 2, 2] + [0] * 252)[0], 0, 128)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_a_start_one_bit_off_is_visible_to_the_reference(name):
    """The inputs of every range (its true start) in a copy, one start shifted by one bit: (exit, count) of the walk from it
    differ from the truth on at least one range -- a reference that could not tell would pin nothing.  One bit LATE is, by
    construction, invisible under a code of two lengths l and l + 1: the late walk reads l bits where the truth reads l + 1
    and stands on the truth's boundary, or it reads on one bit behind the truth, codeword for codeword, until that happens
    -- the same count, the same exit.  So both directions are tried; what each shows is printed."""
    fx = fixture(name)
    jumps = W.Jumps(fx.L, fx.C)
    cuts = [(b, e) for b, e in fx.cuts((1,)) if e - b == W.BLOCK_BYTES]
    starts = np.array([b * 8 + fx.true_start(b) for b, _ in cuts])
    ends = np.array([e * 8 for _, e in cuts])
    true_exits, true_counts = jumps.walk(starts, ends)
    visible = {+1: 0, -1: 0}
    for off in visible:
        for i in range(len(cuts)):
            if starts[i] + off < 0:
                continue
            bad = starts.copy()
            bad[i] += off
            exits, counts = jumps.walk(bad, ends)
            others = np.arange(len(cuts)) != i
            assert np.array_equal(exits[others], true_exits[others]) and np.array_equal(counts[others], true_counts[others])
            visible[off] += (exits[i], counts[i]) != (true_exits[i], true_counts[i])
    print(f"{name}: of {len(cuts)} one-block ranges, a start one bit late changes (exit, count) on {visible[1]}, one bit early on {visible[-1]}")
    assert visible[+1] + visible[-1] >= 1, name


def test_the_skewed_then_flat_dictionary_is_the_window_sweeps_and_never_settles():
    """tests/guards.py skewed_then_flat, which test_skewed_then_flat_stream_hits_the_sync_cap decodes: no tree the walk can
    hold, so the planner starts on the window sweeps; the oracle decodes it; and in whole blocks of the flat half every
    256-bit subsequence's blind run-in (128 bits) is off the true chain when its own bits end."""
    from tests.guards import image_under, skewed_then_flat

    data_t, len_t, text = skewed_then_flat()
    comp = image_under(data_t, len_t, text)
    cb, n, off = E.parse_header(comp)
    assert decode_path(cb) == N.ET_PATH_WINDOWS and O.decode(comp) == text.tobytes()
    k = ctypes.c_uint32(0)
    assert N.lib().et_treewalk_table(ctypes.byref(cb.raw), None, 0, ctypes.byref(k)) != N.ET_OK
    assert W.longest_unsettled_run(comp[off & ~3 :], (off & 3) * 8, cb.data, cb.length, 256, 128) == 256


# ---- hand-made tables: bit patterns that are nobody's codeword (tests/test_gpu_windows.py, and the range tests of test_gpu_syncwork.py) ----

JUNK_DICTIONARIES = {"sparse": lambda: _sparse_dictionary()[:2], "holes200": _flat200_dictionary, "skewed_flat": lambda: _skewed_flat_dictionary()[:2]}
JUNK_BYTES = [8191, 8192, 3 * 8192 + 17, 4 * 8192, 16 * 8192 + 1, 17 * 8192 + 1]  # of test_gpu_parity's _FALLBACK_EDGE_BYTES
JUNK_LANES_ENDING_IN_ONES = range(5, max(JUNK_BYTES) // 32, 41)  # six or seven subsequences of every block, the first one's too
LONG_RANGES = [(0, 16), (1, 17), (3, 20), (16, None), (0, None)]  # of sparse_big, in blocks; None: the stream's end


@functools.lru_cache(maxsize=None)
def junk_stream(dictionary):
    """Random bytes, every value, as a body under one of the hand-made tables: the longest of JUNK_BYTES, of which the others
    are prefixes.  The last three bytes of every 41st subsequence of 256 bits are 0xff: under the sparse table and the 200
    codes that is 24 bits passed over up to the subsequence's end, more than the kernels' tables index -- the lane's walk ends
    in steps without a symbol, and the next symbol is the next lane's (JUNK_LANES_ENDING_IN_ONES, checked on the host)."""
    data_t, len_t = JUNK_DICTIONARIES[dictionary]()
    body = np.random.default_rng(20_241).integers(0, 256, size=max(JUNK_BYTES), dtype=np.uint8)
    for lane in JUNK_LANES_ENDING_IN_ONES:
        body[32 * lane + 29 : 32 * lane + 32] = 0xFF
    return Stream(f"junk/{dictionary}/whole", data_t, len_t, np.zeros(0, np.uint8), body.tobytes(), 0, comp=body.tobytes(), body_off=0, skip=True)


def junk_truth(dictionary, n_bytes, start_bit):
    """What the first n_bytes of the junk decode to from bit start_bit, under the rule "a bit pattern without a codeword is
    passed over one bit at a time" -> (the symbols, the bits passed over).  The blocks that end four bytes or more in front of
    the prefix's end are the whole junk's (kept walks: no codeword that begins in them sees the end); the rest is walked over
    a table of the prefix's own, whose end cuts what reaches beyond it."""
    fx = junk_stream(dictionary)
    whole = max(0, (n_bytes - 4) // W.BLOCK_BYTES)
    off, ats = start_bit, []
    for b in range(whole):
        off, at = fx.block_walk(b, off)
        ats.append(at)
    rest = fx.stream[whole * W.BLOCK_BYTES : n_bytes]
    L, _, C = W.next_table(rest, fx.data, fx.length, "skip")
    _, at = W.walk_positions(L, off, rest.size * 8, C)
    ats.append(at + whole * W.BLOCK_BITS)
    at = np.concatenate(ats)
    passed = n_bytes * 8 - start_bit - int(fx.L[at].astype(np.int64).sum())  # (less the bits of a codeword the end cuts: at most 31)
    return fx.S[at], passed


def _passed_over(fx, begin, end, start):
    """The bits that the walk of the range [begin, end) bytes from its bit `start` steps over without a codeword."""
    exit_bit, at = fx.range_walk(begin, end, start)
    q = int(at[-1]) + int(fx.L[at[-1]]) if at.size else begin * 8 + start  # behind the last counted codeword ...
    while q < end * 8 and not fx.C[q]:
        q += 1  # ... single steps, up to the range's end or to a codeword that the stream's end cuts
    return q - (begin * 8 + start) - int(fx.L[at].astype(np.int64).sum())


@pytest.mark.parametrize("name", list(FIXTURES))
def test_the_skip_walk_from_the_true_start_is_the_plain_walk(name):
    """A stream of its table's own codewords holds no pattern for the rule to act on: under unmatched="skip" the true chain,
    the symbols, every cut's (exit, count) -- by the serial walk and by pointer doubling -- are those of the default rule."""
    fx = fixture(name)
    L0, S0 = W.next_table(fx.stream, fx.data, fx.length)
    L, S, C = W.next_table(fx.stream, fx.data, fx.length, "skip")
    assert np.array_equal(C, L0 > 0) and np.array_equal(L[C], L0[C]) and (L[~C] == 1).all() and np.array_equal(S, S0)
    exit_, at = W.walk_positions(L, fx.first_bit, fx.n_bits, C)
    assert (exit_, at.tolist()) == (W.walk_positions(L0, fx.first_bit, fx.n_bits)[0], fx.at.tolist()) and C[at].all()
    assert W.walk(L, fx.first_bit, fx.n_bits, C) == W.walk(L0, fx.first_bit, fx.n_bits) == (exit_, at.size)
    assert np.array_equal(W.chain(L, fx.first_bit, C=C), fx.on_chain)
    assert np.array_equal(W.walk_symbols(L, S, fx.first_bit, fx.n_bits, C)[1], S0[fx.at])
    cuts = fx.cuts()
    starts, ends = np.array([b * 8 + fx.true_start(b) for b, _ in cuts]), np.array([e * 8 for _, e in cuts])
    for a, b in zip(W.Jumps(L, C).walk(starts, ends), W.Jumps(L0).walk(starts, ends)):
        assert np.array_equal(a, b)
    if FIXTURES[name][1]:  # (the fixtures NOT declared clean may hold lanes that the default rule cannot judge)
        d = W.merge_distances(L, fx.on_chain, C=C)
        assert np.array_equal(d, W.merge_distances(L0, fx.on_chain)) and int(d.max()) < W.NEVER


def test_the_skip_rule_on_a_stream_small_enough_to_follow():
    """Codewords 10 and 11 only, nobody has 0: in 10 0 0 11 0 1|, sixteen bits with the pad, the walk from bit 0 counts 10, 11
    and -- bits 7 and 8 -- 10 (not the 10 at bits 5 and 6, where it never stands), steps over the zeros one at a time, and ends at the end; the one bit left at bit 15 is the
    codeword 10 against the zeros behind the end: cut, uncounted, and the walk ends where the stream does."""
    data, length = [0, 0b10, 0b11] + [0] * 253, [0, 2, 2] + [0] * 253
    body = bytes([0b10001101, 0b00000001])
    L, S, C = W.next_table(body, data, length, "skip")
    assert L.tolist() == [2, 1, 1, 1, 2, 2, 1, 2, 1, 1, 1, 1, 1, 1, 1, 2] and C.tolist() == [l == 2 for l in L.tolist()]
    assert W.walk(L, 0, 16, C) == (16, 3) and W.walk_positions(L, 0, 16, C)[1].tolist() == [0, 4, 7]
    assert W.walk_symbols(L, S, 0, 16, C)[1].tolist() == [1, 2, 1]
    assert W.walk(L, 0, 8, C) == (9, 3) and W.walk(L, 1, 8, C) == (9, 2) and W.walk(L, 5, 7, C) == (7, 1) and W.walk(L, 6, 7, C) == (7, 0)
    jumps = W.Jumps(L, C)
    exits, counts = jumps.walk([0, 0, 1, 6, 9, 15], [16, 8, 8, 7, 16, 16])
    assert exits.tolist() == [16, 9, 9, 7, 16, 16] and counts.tolist() == [3, 3, 2, 0, 0, 0]
    assert W.chain(L, 0, C=C).nonzero()[0].tolist() == [0, 4, 7, 16]
    # lanes of 4 bits with a run-in of 1: from bits 3, 7, 11 -- a step over a zero onto bit 4, a boundary itself, a walk of steps to the end
    assert W.merge_distances(L, W.chain(L, 0, C=C), lane_bits=4, run_in_bits=1, C=C).tolist() == [0, 1, 0, 5]
    with pytest.raises(W.Unmatched):
        W.walk(W.next_table(body + bytes(8), data, length)[0], 0, 16)


def test_the_new_fixtures_are_what_their_gpu_tests_take_them_for():
    """The planner agrees; the sizes; and every walk that a GPU test compares under the rule DOES meet patterns without a
    codeword -- a fixture that stops reaching the rule fails here."""
    for name, path in WINDOW_FIXTURES.items():
        fx = fixture(name)
        assert decode_path(fx.codebook()) == path and fx.C is not None and not fx.C.all(), name
        n = fx.text.size
        assert W.walk_symbols(fx.L, fx.S, fx.first_bit, fx.n_bits, fx.C)[1][:n].tobytes() == fx.text.tobytes()
        assert fx.C[fx.at].all()  # the true chain itself holds codewords only
    big, holes, sf = fixture("sparse_big"), fixture("holes200"), fixture("skewed_flat")
    assert big.n_blocks >= 36 and big.n_bytes % W.BLOCK_BYTES and big.n_bytes <= 1_200_000
    assert holes.n_bytes == 5 * W.BLOCK_BYTES + 17 and holes.stream.tobytes() == holes.text.tobytes()
    assert [int(fixture(n).length.max()) for n in ("sparse", "holes200", "skewed_flat")] == [16, 8, 16]  # the maps' n_starts
    # the exit maps: the walks from every start offset
    for fx in (fixture("sparse"), holes, sf):
        k = int(fx.length.max())
        met = [sum(_passed_over(fx, b, e, p) for p in range(k)) for b, e in fx.cuts()]
        print(f"{fx.name}: bits passed over by the {k} walks of each of {len(met)} ranges: {min(met)} .. {max(met)}")
        assert min(met) > 0
    # ... and under a stream of the table's own codewords those walks are on the true chain after a block: what the INTERIOR blocks
    # of a range see of the rule comes from the junk ranges, where the walks from every start pass bits over in every block
    for d in ("sparse", "holes200"):
        fx = fixture("junk/" + d)
        k = int(fx.length.max())
        assert fx.n_blocks == 7 and fx.text.size == 0
        for b in range(fx.n_blocks):
            for p in range(k):
                assert _passed_over(fx, b * W.BLOCK_BYTES, min((b + 1) * W.BLOCK_BYTES, fx.n_bytes), p) > (100 if b < 6 else 0), (d, b, p)
    # the exits of the even start offsets never merge inside the flat half: a map there has truly different entries
    b = sf.n_blocks // 2
    exits = [sf.range_walk(b * W.BLOCK_BYTES, (b + 1) * W.BLOCK_BYTES, p)[0] for p in range(0, 8, 2)]
    assert len(set(e % 8 for e in exits)) == 4 and sf.text[sf.truth(b * W.BLOCK_BYTES, (b + 1) * W.BLOCK_BYTES)[3].size * b] >= 16, exits
    # the wrong known starts, true start + 1
    for fx in (fixture("sparse"), sf):
        met = [_passed_over(fx, b, e, fx.true_start(b) + 1) for b, e in fx.cuts()]
        assert sum(m > 0 for m in met) >= len(met) // 2, (fx.name, met)
    for b0, b1 in LONG_RANGES:
        begin, end = b0 * W.BLOCK_BYTES, big.n_bytes if b1 is None else b1 * W.BLOCK_BYTES
        assert _passed_over(big, begin, end, big.true_start(begin) + 1) > 0, (b0, b1)
    # the junk
    for d in JUNK_DICTIONARIES:
        for n_bytes in JUNK_BYTES:
            for start_bit in (0, 5):
                syms, passed = junk_truth(d, n_bytes, start_bit)
                assert passed > n_bytes // 4 and syms.size > n_bytes // 2, (d, n_bytes, start_bit, syms.size, passed)  # (a third of the steps or more)
        print(f"junk under {d}: {syms.size} symbols, {passed} bits passed over in {n_bytes} bytes")
    # subsequences whose last codeword ends 16 bits or more in front of their end, a codeword beginning within 32 bits behind it
    for d in ("sparse", "holes200"):
        fx = junk_stream(d)
        ends = fx.at + fx.L[fx.at]
        gap_over_a_lane_end = (fx.at[1:] // 256 > ends[:-1] // 256) & ((ends[:-1] // 256 + 1) * 256 - ends[:-1] >= 16) & (fx.at[1:] % 256 < 32)
        blocks = set((fx.at[1:][gap_over_a_lane_end] // W.BLOCK_BITS).tolist())
        assert {0, 1, 4, 16} <= blocks and len(blocks) >= 12, (d, sorted(blocks))  # the first block, interior ones, one behind the superblocks


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_the_islands_reach_the_listed_repair_and_nothing_else(where):
    """tests/guards.py island under the rule, every lane judged (no NEVER): k >= 1 blocks hold a run of unsettled 256-bit lanes
    that outlasts the first sweep's trips AND the second's; k * 64 <= n_blocks, the rule of dec_state_final and body_first_sweep
    for "repair sweeps, not the fallback"; every other block stays below the first sweep's trips, so that it does not give up.
    From 16 blocks on the first sweep walks 512-bit lanes over superblocks: the same three conditions in that geometry.
    Conditions on the input, not measurements.  And under the default rule most lanes of such a stream are nobody's to judge."""
    from tests.test_gpu_syncwork import CERTAIN_FROM, FIRST_SWEEP_TRIPS

    fx = fixture("island_" + where)
    assert fx.n_blocks == 144
    for lane_bits in (256, 512):
        runs = W.unsettled_block_runs(fx.stream, fx.first_bit, fx.data, fx.length, lane_bits, 128, "skip")
        certain = np.flatnonzero(runs >= CERTAIN_FROM["windows"])
        print(f"island {where}, lanes of {lane_bits} bits: blocks {certain.tolist()} hold runs of {runs[certain].tolist()} unsettled lanes, the others at most {int(np.delete(runs, certain).max())}")
        assert certain.tolist() == [{"first": 0, "middle": 71, "last": 143}[where]]
        assert certain.size * 64 <= fx.n_blocks
        assert int(np.delete(runs, certain).max()) < FIRST_SWEEP_TRIPS
    L0, _ = W.next_table(fx.stream, fx.data, fx.length)
    d0 = W.merge_distances(L0, fx.on_chain, 256, 128, enough=384)
    assert int(np.count_nonzero(d0 == W.NEVER)) > d0.size // 2


def test_holes_as_leaves_is_the_tree_walks_completed_tree():
    """The second rule, the tree walk's (tw_build_tree(complete = true)): every child that a node of the codewords' tree lacks
    becomes a leaf that decodes as byte 0.  bitwalk.leaves_for_holes gives those leaves as pseudo-codewords.  For the small
    holed table of tests/guards.py: ONE leaf, 1111, four bits deep.  et_treewalk_table itself turns a holed table away (it
    builds with complete = false), so the model is held against it through a FULL table: the codewords and, under symbols
    behind every coded one (so that the nodes are numbered as they are without them), the pseudo-codewords -- accepted only
    if prefix-free and full, with the holed tree's own nodes and not one more (every hole a child of a node that is there:
    maximal), and its table is the brute-force table of tests/test_host_logic.py for those codes."""
    from tests.test_host_logic import _brute_treewalk_table

    data_t, len_t, syms = _small_holed_dictionary()
    leaves = W.leaves_for_holes(data_t, len_t)
    assert leaves == [(0b1111, 4, 0)]
    n_int = ctypes.c_uint32(0)
    holed = E.Codebook.from_tables(data_t, len_t)
    assert N.lib().et_treewalk_table(ctypes.byref(holed.raw), None, 0, ctypes.byref(n_int)) == N.ET_ERR_UNSUPPORTED
    assert decode_path(holed) == N.ET_PATH_TREE_WALK  # (the decode completes the tree)
    for d, l in ((data_t, len_t), _flat200_dictionary()):  # the flat table too: 56 missing bytes in a handful of subtrees
        leaves = W.leaves_for_holes(d, l)
        nodes = {(int(d[s]) >> (int(l[s]) - k), k) for s in np.flatnonzero(l) for k in range(int(l[s]))}
        full_d, full_l = d.copy(), l.copy()
        free = [s for s in range(int(np.flatnonzero(l).max()) + 1, 256)]
        assert len(leaves) <= len(free)
        for s, (code, length, byte) in zip(free, leaves):
            full_d[s], full_l[s] = code, length
            assert byte == 0
        full = E.Codebook.from_tables(full_d, full_l)
        cap = (256 + 7) * 256
        table = np.zeros(cap, dtype=np.uint16)
        assert N.lib().et_treewalk_table(ctypes.byref(full.raw), table.ctypes.data, cap, ctypes.byref(n_int)) == N.ET_OK
        assert n_int.value == len(nodes) == full.raw.n_coded - 1
        want_n, want = _brute_treewalk_table(full_d, full_l)
        assert want_n == n_int.value and np.array_equal(table[: want.size], want)
    assert W.leaves_for_holes(*_flat200_dictionary()) == [(0b111, 3, 0), (0b1101, 4, 0), (0b11001, 5, 0)]  # the bytes 224 .., 208 .., 200 ..
    # the model as a table: under it nothing is unmatched, and 0xff reads 1111 1111 -- two leaves, byte 0 twice
    stream = bytes([0xFF, 0b11100101, 0b01101111]) + bytes(4)
    L, S = W.next_table(stream, data_t, len_t, extra=W.leaves_for_holes(data_t, len_t))
    assert (L[:24] > 0).all() and W.walk_symbols(L, S, 0, 24)[1].tolist() == [0, 0, 105, 65, 67, 0]
    Lk, Sk, Ck = W.next_table(stream, data_t, len_t, "skip")
    assert W.walk_symbols(Lk, Sk, 0, 24, Ck)[1].tolist() == [105, 65, 67, 100]  # bit by bit: eight ones passed over, 1110 0101, 0, 110, one more one passed over, 1110 0000 (begun in front of bit 24)
