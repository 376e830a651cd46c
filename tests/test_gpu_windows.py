"""GPU: the window family (csrc/et_kernels_fallback.hip) where it is not easy -- the decoder of every dictionary the tree walk
cannot hold, of the range calls under such a dictionary, and of .et files whose dictionary is damaged.

Three walks implement "a bit pattern that is no symbol's codeword is passed over one bit at a time, and yields no symbol": the
LDS windows (walk_subsequence), the step tables of the synchronisation over registers (walk_steps), and the write over registers
(walk_write).  If the synchronisation and the write count such a stretch differently the output is shifted -- bounded, no
fault, no error.  Here they are held, byte for byte and entry for entry, against the serial reference under the same rule
(tests/bitwalk.py, unmatched="skip"): junk bodies, ranges of 16 blocks and more from true, unknown and wrong starts, streams
with ONE block that does not settle (the listed repair sweeps and the second, non-speculative write), and every way through the
family on one context.  The exit maps under these tables are in tests/test_gpu_syncwork.py (RANGE_MAPS, RANGE_SYNC).  For a
SMALL tree with holes the tree walk's own rule applies (a hole is a leaf that decodes as byte 0) until its sweep gives up: both
are pinned, by what the timing says ran.  tests/test_syncwork_host.py checks the reference and these inputs without a GPU.
Every comparison is exact."""
import numpy as np
import pytest

from tests import bitwalk as W
from tests.guards import Guarded, _small_holed_dictionary, image_under, skewed_then_flat, sparse_text
from tests.test_gpu_syncwork import BITS, CERTAIN_FROM, FAMILY, GAVE_UP, _Range, _timed, _triple, check_repair_reach
from tests.test_syncwork_host import JUNK_BYTES, JUNK_DICTIONARIES, LONG_RANGES, fixture, junk_stream, junk_truth

pytestmark = pytest.mark.gpu

NO_BITS = {b: False for b in BITS}


def _behind_0xff(body):
    """The body on the device with 64 bytes of 0xff behind it (the bits behind a stream's end count as ZEROS: a kernel that
    reads on sees ones) -> the tensor's view of the body alone, 256-byte aligned."""
    import torch

    d = torch.full((len(body) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    d[: len(body)] = torch.from_numpy(np.frombuffer(bytes(body), dtype=np.uint8).copy()).cuda()
    assert d.data_ptr() % 16 == 0
    return d[: len(body)]


# ---- whole streams of junk --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dictionary", list(JUNK_DICTIONARIES))
def test_junk_decodes_to_the_walk_that_passes_over_bit_by_bit(ctx, dictionary):
    """et_decode_body_device of random bytes under the sparse table (window sweeps and write), the 200 codes of 8 bits (exit
    maps, then the window write: the tree is not full) and the skewed-and-flat table (window sweeps whose flat stretches may
    give up), at body sizes on both sides of the kernels' block bookkeeping (LDS windows alone, interior blocks, superblocks,
    an odd block behind them), ascending and then descending on one context, from bit 0 and from bit 5, the declared symbol
    count above what the body holds: the count returned and every byte are the serial walk's, and nothing outside
    [0, out_len) is written.  About every second or third step of these walks is the rule under test."""
    fx = junk_stream(dictionary)
    cb = fx.codebook()
    bodies = [_behind_0xff(fx.stream[:t]) for t in JUNK_BYTES]
    out = Guarded(4 * max(JUNK_BYTES) + 64)  # (the shortest codeword of the three tables has 2 bits)
    for start_bit in (0, 5):
        truths = [junk_truth(dictionary, t, start_bit) for t in JUNK_BYTES]
        order = list(range(len(JUNK_BYTES)))
        for i in order + order[::-1]:
            t, (want, passed) = JUNK_BYTES[i], truths[i]
            out.refill()
            declared = 4 * t + 64
            m, iters, bits = _timed(ctx, lambda: ctx.decode_body_device(cb, bodies[i], declared, out.room[:declared], start_bit))
            out.check()
            what = f"{dictionary}, {t} bytes from bit {start_bit}"
            print(f"{what}: {m} symbols ({want.size} by the walk, {passed} bits passed over), sync_iters {iters}, bits {[b for b in BITS if bits[b]]}")
            assert 0 <= m <= declared
            out.assert_extent(m, what)
            assert m == want.size, what
            got = out.data(m)
            if not np.array_equal(got, want):
                at = int(np.flatnonzero(got != want)[0])
                raise AssertionError(f"{what}: symbol {at} of {m} is {int(got[at])}, the walk's is {int(want[at])}; {int((got != want).sum())} differ")
            assert not bits["tree_walk_sync"] or dictionary == "holes200"
            assert not bits["chained_write"]


# ---- the small tree with a hole -----------------------------------------------------------------------------------------------------

HOLED_JUNK_BYTES = 18 * W.BLOCK_BYTES + 1234


def _holed_bodies():
    """-> {name: body}: random bytes; the same with a run of 12 000 bytes of 0xff laid into them.  Under the tree walk's rule
    the run reads 1111, the hole's leaf, from any phase: the four phases never merge, and the lanes it covers do not settle."""
    junk = np.random.default_rng(321).integers(0, 256, size=HOLED_JUNK_BYTES, dtype=np.uint8)
    ones = junk.copy()
    ones[5 * W.BLOCK_BYTES + 100 : 5 * W.BLOCK_BYTES + 12_100] = 0xFF
    return {"junk": junk.tobytes(), "junk with a run of ones": ones.tobytes()}


@pytest.mark.parametrize("name", ["junk", "junk with a run of ones"])
def test_a_small_tree_with_a_hole_decodes_by_the_rule_of_what_ran(ctx, name):
    """The table 0, 10, 110, 1110xxxx: under the tree walk the pattern 1111 is a leaf that decodes as byte 0; if its sweep
    gives up, the exit maps and the window write take over, and they pass the pattern over bit by bit.  Which of the two ran
    is in the timing; the bytes are the ones THAT rule gives (tests/bitwalk.py: leaves_for_holes; unmatched="skip").  The run
    of ones is certain to give up: the reference, following the leaf rule over lanes of 512 bits, finds FIRST_SWEEP_TRIPS
    (CERTAIN_FROM["tree_walk"]) unsettled lanes in a row in more than n_blocks / 64 blocks."""
    data_t, len_t, _ = _small_holed_dictionary()
    import entreepy_amd as E

    cb = E.Codebook.from_tables(data_t, len_t)
    body = _holed_bodies()[name]
    n_blocks = (len(body) + W.BLOCK_BYTES - 1) // W.BLOCK_BYTES
    leaves = W.leaves_for_holes(data_t, len_t)
    out = Guarded(8 * len(body) + 64)  # (the shortest codeword has one bit)
    d_body = _behind_0xff(body)
    for start_bit in (0, 5):
        runs = W.unsettled_block_runs(body, start_bit, data_t, len_t, extra=leaves)
        stuck = int(np.count_nonzero(runs >= CERTAIN_FROM["tree_walk"]))
        certain = stuck * 64 > n_blocks
        assert certain or name == "junk", runs.tolist()
        m, iters, bits = _timed(ctx, lambda: ctx.decode_body_device(cb, d_body, out.n, out.room, start_bit))
        out.check()
        by_leaves = bits["tree_walk_sync"] and bits["chained_write"] and not bits["exhaustive_sync"]
        by_steps = bits["exhaustive_sync"]
        print(f"{name} from bit {start_bit}: unsettled runs per block up to {int(runs.max())}, {'holes as leaves' if by_leaves else 'bit by bit'}; sync_iters {iters}, {m} symbols")
        assert by_leaves != by_steps, bits
        if certain:
            assert by_steps, f"{stuck} of {n_blocks} blocks cannot settle, yet the tree walk's result was kept"
        assert by_leaves or not bits["chained_write"]
        want = W.decode_by_rule(body, data_t, len_t, "leaves" if by_leaves else "skip", start_bit)
        out.assert_extent(m, name)
        assert m == want.size and np.array_equal(out.data(m), want), (name, start_bit, m, want.size)
        out.refill()


# ---- long ranges --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("blocks", LONG_RANGES, ids=lambda r: f"{r[0]}-{'end' if r[1] is None else r[1]}")
def test_long_ranges_under_a_window_dictionary(ctx, blocks):
    """et_decode_range_sync over 16 blocks and more of the sparse dictionary's stream: [0, 16), [1, 17), [3, 20) (17 blocks), [16,
    end) (ragged, no tail) and the whole stream -- the first sweep over superblocks (k_dec_sync_reg2) and its eight special
    workgroups with the bytes in front readable and the start unknown, the repair sweeps over every block.  From the true
    start, from an unknown one, and from the true one + 1: (start, exit, count) and every symbol are the serial walk's from the
    start the call reports; then the call with the true start gives the truth (the repair of the states that stand)."""
    fx = fixture("sparse_big")
    r = _Range(ctx, fx)
    begin, end = blocks[0] * W.BLOCK_BYTES, fx.n_bytes if blocks[1] is None else blocks[1] * W.BLOCK_BYTES
    s, x, n, syms = fx.truth(begin, end)
    assert (s, x, n) == r.walk(begin, end, s) and (end - begin + W.BLOCK_BYTES - 1) // W.BLOCK_BYTES >= 16

    def truth_from_the_true_start():
        info = r.sync(begin, end, s)  # (asserts info["tree_walk"] is False)
        assert _triple(info) == (s, x, n), (begin, end, info)
        assert np.array_equal(r.written(n), syms), (begin, end)

    truth_from_the_true_start()
    starts = ([-1] if begin else []) + [s + 1]
    for start in starts:
        info = r.sync(begin, end, start)
        got = info["start_bit"]
        print(f"blocks {blocks}: start {start} -> {info}")
        assert got < 32 and (start < 0 or got == start) and _triple(info) == r.walk(begin, end, got), (begin, end, start, info)
        assert np.array_equal(r.written(info["n_symbols"]), r.symbols(begin, end, got)), (begin, end, start)
        truth_from_the_true_start()


# ---- one block that does not settle ------------------------------------------------------------------------------------------------


def _island_image(where):
    fx = fixture("island_" + where)
    return fx.comp, fx.text.tobytes()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_unsettled_block_takes_the_listed_repair_sweeps(ctx, where):
    """tests/guards.py island: 144 blocks of which ONE holds a run of 45 or 46 unsettled subsequences (the reference says so of
    the input: tests/test_syncwork_host.py) -- it gives up in the first sweep and fails the verification, too few blocks for
    the fallback: the listed repair sweeps (k_dec_check, then k_dec_sync_reg over the worklist) and a second, non-speculative
    write.  The text, twice; and the timing says that the repair sweeps ran and the fallback did not."""
    comp, want = _island_image(where)
    for _ in range(2):
        assert ctx.decode(comp) == want
    planned, iters, bits = check_repair_reach(ctx, comp, want, certain=True)
    assert planned == "windows"
    assert "exhaustive_sync" not in bits and iters > FAMILY["windows"][0], (planned, iters, bits)
    assert bits == []


# ---- every way through the family, on one context -----------------------------------------------------------------------------------


def test_one_context_every_way_through_the_window_family(ctx):
    """With nothing in between: island("middle") (listed repair, second write), skewed_then_flat (every block gives up: exit
    maps, the round-1 write), the sparse fixture (clean), a 3-block sparse body (the LDS-window kernels alone: draws no ticket
    and leaves both ticket words as they are), island("last") -- and back.  A ticket or flag word that one way leaves behind
    is met by the next.  The bytes, the guards, and the family's row of launches and bits for each."""
    import torch

    import entreepy_amd as E

    def image(comp, text):
        d = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).cuda()
        return lambda out: ctx.decode_device(d, out), text

    def body(fx_or_pair):
        data_t, len_t, text, packed = fx_or_pair
        d, cb = _behind_0xff(packed), E.Codebook.from_tables(data_t, len_t)
        return lambda out: ctx.decode_body_device(cb, d, text.size, out), text.tobytes()

    from oracle import oracle as O

    sparse = fixture("sparse")
    small = sparse_text(18_500, 11)
    small_body = O.pack_body(sparse.data, sparse.length, small)[0]
    assert 2 * W.BLOCK_BYTES < len(small_body) <= 3 * W.BLOCK_BYTES
    sf = skewed_then_flat()
    repaired = lambda iters, bits: iters > FAMILY["windows"][0] and bits == NO_BITS
    ways = [
        ("island middle", image(*_island_image("middle")), repaired),
        ("skewed then flat", image(image_under(*sf), sf[2].tobytes()), lambda iters, bits: (iters, bits) == GAVE_UP["windows", "exit_maps"]),
        ("sparse", body((sparse.data, sparse.length, sparse.text, sparse.comp)), lambda iters, bits: (iters, bits) == FAMILY["windows"]),
        ("sparse, 3 blocks", body((sparse.data, sparse.length, small, small_body)), lambda iters, bits: (iters, bits) == FAMILY["windows"]),
        ("island last", image(*_island_image("last")), repaired),
    ]
    out = Guarded(max(len(text) for _, (_, text), _ in ways) + 64)
    for name, (call, text), row_ok in ways + ways[::-1]:
        out.refill()
        m, iters, bits = _timed(ctx, lambda: call(out.room[: len(text) + 64]))
        out.check()
        print(f"{name}: {m} symbols, sync_iters {iters}, bits {[b for b in BITS if bits[b]]}")
        out.assert_extent(m, name)
        assert m == len(text) and out.data(m).tobytes() == text, name
        assert row_ok(iters, bits), (name, iters, bits)
