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
from tests.guards import _sparse_dictionary
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
    on_chain (one flag per bit)."""

    def __init__(self, name, data, length, text, stream, first_bit, comp=None, body_off=None):
        self.name, self.data, self.length, self.text = name, np.asarray(data, np.uint32), np.asarray(length, np.uint8), np.asarray(text, np.uint8)
        self.stream, self.first_bit, self.comp, self.body_off = np.frombuffer(bytes(stream), dtype=np.uint8), first_bit, comp, body_off
        self.n_bytes, self.n_bits = self.stream.size, self.stream.size * 8
        self.shift, self.start_bit = first_bit // 8, first_bit % 8  # the body lies `shift` bytes into the stream and begins at bit start_bit of that byte
        self.n_blocks = (self.n_bytes + W.BLOCK_BYTES - 1) // W.BLOCK_BYTES
        self.L, self.S = W.next_table(self.stream, self.data, self.length)
        _, self.at = W.walk_positions(self.L, first_bit, self.n_bits)
        self.on_chain = W.chain(self.L, first_bit, self.at)
        for a in (self.L, self.S, self.at, self.on_chain):
            a.setflags(write=False)

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
    if name == "sparse":  # the dictionary and text of test_fallback_sweeps_and_write_are_what_a_sparse_dictionary_runs, n = 60 000
        data_t, len_t, syms = _sparse_dictionary()
        n = 60_000
        rng = np.random.default_rng(n)
        text = syms[np.minimum(rng.integers(0, 300, size=n), syms.size - 1) % syms.size].astype(np.uint8)
        text[rng.random(n) < 0.5] = 32
        body, _ = O.pack_body(data_t, len_t, text)
        return Stream(name, data_t, len_t, text, body, 0, comp=body, body_off=0)
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
    exit_, syms = W.walk_symbols(fx.L, fx.S, fx.first_bit, fx.n_bits)
    assert fx.n_bits <= exit_ < fx.n_bits + 32 and n <= syms.size <= n + 7  # (whole codewords in the pad bits are decoded too)
    image = fx.comp if name != "sparse" else fx.codebook().header(n)[4:] + fx.comp
    assert syms[:n].tobytes() == O.decode(image) == fx.text.tobytes()
    bounds = W.boundaries(fx.first_bit, fx.length, fx.text)
    assert np.array_equal(fx.at[:n], bounds[:-1]) and (fx.at.size == n or fx.at[n] == bounds[-1])
    assert np.array_equal(fx.L[bounds[:-1]], fx.length[fx.text]) and np.array_equal(fx.S[bounds[:-1]], fx.text)
    assert W.walk(fx.L, fx.first_bit, fx.n_bits) == (exit_, syms.size)
    # the same through the pointer-doubling variant, for the whole stream and for every cut of it
    jumps = W.Jumps(fx.L)
    assert [int(x[0]) for x in jumps.walk([fx.first_bit], [fx.n_bits])] == [exit_, syms.size]
    cuts = fx.cuts()
    assert len(cuts) >= 3 * fx.n_blocks - 5 and sum(1 for _, e in cuts if e == fx.n_bytes) >= 1
    starts = np.array([b * 8 + fx.true_start(b) for b, _ in cuts])
    ends = np.array([e * 8 for _, e in cuts])
    exits, counts = jumps.walk(starts, ends)
    for (b, e), x, c in zip(cuts, exits, counts):
        s, exit_bit, n_sym, syms = fx.truth(b, e)
        assert (int(x) - e * 8, int(c)) == (exit_bit, n_sym) == (W.walk(fx.L, b * 8 + s, e * 8)[0] - e * 8, syms.size), (b, e)
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
    jumps = W.Jumps(fx.L)
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
