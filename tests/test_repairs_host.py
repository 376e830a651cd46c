"""The inputs of tests/test_gpu_repairs.py against what that file takes them for, on the host: the periodic fixture (ONE period
checked here, tiled on the device), how many give-ups each family COUNTS for it, how many blocks its listed repair sweeps meet
and by what margin that is more than one grid of them, and the stream whose every block seam misleads a blind run-in without
anybody giving up.  Conditions on the inputs, read off the serial reference (tests/bitwalk.py); a fixture that stops being what
its GPU test relies on fails HERE.  No GPU.

How a give-up is counted (FLAG_GAVE_UP, which body_first_sweep and dec_state_final hold against n_blocks / 64):
  windows    from 16 blocks on, sweep 0 walks superblocks of two blocks (k_dec_sync_reg2): a pair that is unsettled at its trip
             cap adds 2 and marks BOTH blocks.  Sweep 1 (listed, its cap DEC_REPAIR_SWEEP_TRIPS) settles the innocent one --
             the block before it ends where it always did -- and adds nothing; the guilty one stays marked, fails the
             verification and is the ONE block per stretch that repair_sweeps' worklist holds.
  tree walk  k_tw_sync adds 1 per ATTEMPT that ends at the trip cap, and a block that gave up is done again within the same
             sweep, from the node the block before it published ("a block that gave up is done again whatever the block before
             it says"): a stretch of CERTAIN_FROM or more unsettled lanes ends that attempt at the cap too.  2 per block."""
import ctypes
import functools

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from oracle import oracle as O
from tests import bitwalk as W
from tests.guards import ISLAND_AT_BIT, ISLAND_FLAT, failed_run_ins, periodic_islands
from tests.test_gpu_syncwork import CERTAIN_FROM, FIRST_SWEEP_TRIPS, LANES
from tests.test_syncwork_host import decode_path

FAMILIES = ("windows", "tree_walk")
PATH = {"windows": N.ET_PATH_WINDOWS, "tree_walk": N.ET_PATH_TREE_WALK}
G = {"windows": 2, "tree_walk": 2}  # give-ups per period AS THE DEVICE COUNTS THEM (the module's docstring); one stretch per period
PERIOD_BLOCKS = {f: 64 * G[f] for f in FAMILIES}  # the smallest period with 64 * g <= period_blocks: equality
LISTED_PER_PERIOD = 1  # what repair_sweeps' worklist holds of a period: the block the stretch lies in
WINDOW_LISTED_GRID = 512  # launch_dec_sync, listed: min(n_blocks, 512) workgroups, one listed block each per stride
MANY_PERIODS = 2 * 512 + 64  # part 2: 1 088 listed blocks, two whole strides of 512 and 64 blocks of a third
RUN_IN_BLOCKS, RUN_IN_SHIFTS = 2_304, (0, 1, 3)  # part 3: the stream's blocks; the body's byte offsets behind an aligned address


def tw_listed_blocks_per_stride(n_int):
    """launch_tw_sync's arithmetic for a listed sweep: the table's (n_int + 7) * 256 entries of 2 bytes, at most 3 workgroups
    per CU of what 160 KiB hold, 24 wavefronts shared out among them (16 at the most), a grid of 64 workgroups, one listed
    block per wavefront and stride."""
    per_cu = min(max((160 * 1024) // ((n_int + 7) * 256 * 2), 1), 3)
    waves = (24 + per_cu - 1) // per_cu
    waves -= waves * per_cu > 24
    return 64 * min(waves, 16)


@functools.lru_cache(maxsize=None)
def period(family):
    """-> (data, length, text, body, island_block) of the family's one period; read-only."""
    data_t, len_t, text, body = periodic_islands(family, PERIOD_BLOCKS[family])
    text.setflags(write=False)
    return data_t, len_t, text, body, PERIOD_BLOCKS[family] // 2


def _runs(stream, text, data_t, len_t, family, lane_bits):
    """bitwalk.unsettled_block_runs by way of its variant in pieces (held against it below): a tenth of the time."""
    return W.unsettled_block_runs_by_text(stream, 0, data_t, len_t, text, ((lane_bits, 128),), "skip" if family == "windows" else "stop")[0]


@pytest.mark.parametrize("family", FAMILIES)
def test_one_period_is_whole_blocks_and_tiles(family):
    """The period's bit count; the tiled body is the oracle's pack of the tiled text (three periods, so that the middle one has
    true neighbours); the planner starts it on the family its GPU tests expect; the tree walk's table is complete."""
    data_t, len_t, text, body, _ = period(family)
    n_bits = int(len_t[text].astype(np.int64).sum())
    print(f"{family}: one period is {text.size} symbols in {n_bits} bits = {PERIOD_BLOCKS[family]} blocks")
    assert n_bits == PERIOD_BLOCKS[family] * W.BLOCK_BITS == len(body) * 8
    packed, end_bit = O.pack_body(data_t, len_t, np.tile(text, 3))
    assert end_bit == 3 * n_bits and packed == body * 3
    cb = E.Codebook.from_tables(data_t, len_t)
    assert decode_path(cb) == PATH[family]
    n_int = ctypes.c_uint32(0)
    rc = N.lib().et_treewalk_table(ctypes.byref(cb.raw), None, 0, ctypes.byref(n_int))
    if family == "tree_walk":  # (a table of its own codewords only: the walk makes no leaf, the reference needs no rule)
        assert cb.is_complete() and rc == N.ET_OK and n_int.value == cb.raw.n_coded - 1 == 35
        assert tw_listed_blocks_per_stride(n_int.value) == 512
        assert set(text.tolist()) <= set(range(1, 7)) | set(range(16, 32))  # no text uses the codewords that complete the table
    else:
        assert rc != N.ET_OK


@pytest.mark.parametrize("family", FAMILIES)
def test_which_blocks_of_a_period_give_up_and_how_that_is_counted(family):
    """Three periods in a row under the reference: in every geometry the family walks (the windows: sweep 0's 512-bit lanes, the
    repair sweeps' 256-bit ones; the tree walk: 512), exactly ONE block per period -- the same one -- holds a run of unsettled
    lanes that outlasts every trip cap in the family's base count; every other block holds NO run at the first sweep's cap, and
    all but a few none at all; every block's first lane included, so it starts where the block before it ends.  From that: g,
    the equality 64 * g == period_blocks, the blocks the repair sweeps list and their distances."""
    data_t, len_t, text, body, island_block = period(family)
    pb = PERIOD_BLOCKS[family]
    for lane_bits in sorted({LANES[family][0], 512}):
        runs = _runs(body * 3, np.tile(text, 3), data_t, len_t, family, lane_bits)
        certain = np.flatnonzero(runs >= CERTAIN_FROM[family])
        others = np.delete(runs, certain)
        print(f"{family}, lanes of {lane_bits} bits: blocks {certain.tolist()} of {runs.size} hold runs of {runs[certain].tolist()} unsettled lanes; the others at most {int(others.max())}, {int(np.count_nonzero(others))} of them any")
        assert runs.size == 3 * pb and certain.tolist() == [island_block, pb + island_block, 2 * pb + island_block]
        assert int(others.max()) < FIRST_SWEEP_TRIPS
        assert np.array_equal(runs[:pb][1:], runs[pb : 2 * pb][1:]) and np.array_equal(runs[pb : 2 * pb], runs[2 * pb :])  # every copy lies on the grid alike
    # the stretch lies inside its block, clear of the blocks in front and behind: it re-synchronises before the block ends
    # (the block's exit never moves), and neither it nor its superblock's other half is the block that part 4 (b) cuts off
    a = island_block * W.BLOCK_BITS + ISLAND_AT_BIT
    assert 2 <= island_block and island_block + 1 < pb - 6  # an interior superblock of sweep 0, at every number of periods
    assert a // W.BLOCK_BITS == (a + 8 * ISLAND_FLAT + 2_048) // W.BLOCK_BITS == island_block
    assert island_block + 1 < pb - 1
    g = G[family]
    print(f"{family}: g = {g} give-ups counted per period of {pb} blocks; the repair sweeps list block {island_block} of each period, {pb} blocks apart")
    assert 64 * g == pb and LISTED_PER_PERIOD == 1 and pb > 1  # listed blocks are never neighbours
    # part 2: more listed blocks than two grids of the family's listed sweep hold, and still no more give-ups than n_blocks / 64
    grid = WINDOW_LISTED_GRID if family == "windows" else tw_listed_blocks_per_stride(35)
    listed = MANY_PERIODS * LISTED_PER_PERIOD
    print(f"{family}: {MANY_PERIODS} periods list {listed} blocks, {listed - 2 * grid} more than two strides of {grid}")
    assert listed >= 2 * grid + 64 and 64 * g * MANY_PERIODS <= MANY_PERIODS * pb
    for n in (1, 2):
        assert 64 * g * n <= n * pb and n * LISTED_PER_PERIOD <= grid and n * pb >= 16  # one stride; sweep 0 over superblocks


@pytest.mark.parametrize("family", FAMILIES)
def test_the_reference_in_pieces_is_the_reference(family):
    """unsettled_block_runs_by_text (the true chain from the text's code lengths, the table in pieces) and seam_walks against
    the whole-stream functions: three periods of 16 blocks, in both geometries, with pieces that do not divide the stream."""
    data_t, len_t, text, body = periodic_islands(family, 16)
    stream, text3, rule = body * 3, np.tile(text, 3), "skip" if family == "windows" else "stop"
    L, _, *C = W.next_table(stream, data_t, len_t, rule)
    C = C[0] if C else None
    on = W.chain(L, 0, C=C)
    bounds = W.TextBounds(0, len_t, text3, every=1000)
    assert np.array_equal(np.flatnonzero(on), bounds.between(0, len(stream) * 8 + 1)) and bounds.end == len(stream) * 8
    for lane_bits, piece_blocks in ((256, 5), (512, 7)):
        want = W.unsettled_block_runs(stream, 0, data_t, len_t, lane_bits, 128, rule)
        assert want.max() >= CERTAIN_FROM[family]
        assert np.array_equal(W.unsettled_block_runs_by_text(stream, 0, data_t, len_t, text3, ((lane_bits, 128),), rule, piece_blocks=piece_blocks, bounds=bounds)[0], want)
    blind, true, merged = W.seam_walks(stream, 0, data_t, len_t, text3, unmatched=rule)
    for b in range(1, 48):
        seam = b * W.BLOCK_BITS
        p, _ = W.walk(L, seam - 128, seam, C)
        assert (blind[b - 1], true[b - 1]) == (p - seam, int(np.flatnonzero(on[seam:])[0]))
        while not on[p]:
            p += int(L[p])
        assert merged[b - 1] == p - seam


# ---- part 3: every seam misleads its blind run-in, nobody gives up --------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def run_in_stream():
    """-> (data, length, text, body) of failed_run_ins(RUN_IN_BLOCKS); read-only."""
    data_t, len_t, text = failed_run_ins(RUN_IN_BLOCKS)
    text.setflags(write=False)
    body, end_bit = O.pack_body(data_t, len_t, text)
    return data_t, len_t, text, body[: (end_bit + 7) // 8]


def first_sweep_stretches(n_bytes):
    """The blocks at which a workgroup of the window family's sweep 0 BEGINS a stretch that it settles within itself, so that
    nobody hands their first lane a start: from 16 blocks on the even blocks of the interior superblocks (k_dec_sync_reg2; the
    odd ones' first lane is lane 128 of its workgroup) and every block of the superblocks that are not interior -- those with
    the stream's first block, or with one whose staged words reach the stream's end (block_limit) -- which k_dec_sync takes one
    by one; below 16 blocks, every block."""
    n_blocks = (n_bytes + W.BLOCK_BYTES - 1) // W.BLOCK_BYTES
    special = lambda b: b == 0 or n_bytes * 8 - b * W.BLOCK_BITS + 128 < (4 + 2048 + 4) * 32 + 64
    interior = lambda s: 2 * s + 1 < n_blocks and not special(2 * s) and not special(2 * s + 1)
    return np.array([b for b in range(n_blocks) if n_blocks < 16 or not (b % 2 and interior(b // 2))])


@functools.lru_cache(maxsize=None)
def listed_in_sweep_1(shift):
    """-> (the blocks that the window family's sweep 1 lists for the part 3 stream `shift` bytes behind an aligned address,
    how far into each its blind first lane is on the true chain, the seams that mislead a run-in in all)."""
    data_t, len_t, text, body = run_in_stream()
    stream = bytes(shift) + body
    wrong, merged = W.listed_after_first_sweep(stream, 8 * shift, data_t, len_t, text)
    keep = np.isin(wrong, first_sweep_stretches(len(stream)))
    return wrong[keep], merged[keep], wrong.size


def test_first_sweep_stretches_on_streams_small_enough_to_follow():
    assert first_sweep_stretches(15 * 8192).tolist() == list(range(15))
    assert first_sweep_stretches(20 * 8192).tolist() == [0, 1] + list(range(2, 18, 2)) + [18, 19]  # the last block is the stream's end
    assert first_sweep_stretches(20 * 8192 + 1).tolist() == [0, 1] + list(range(2, 18, 2)) + [18, 19, 20]  # 21 blocks: 19 ends 1 byte short of the end
    assert first_sweep_stretches(20 * 8192 + 100).tolist() == [0, 1] + list(range(2, 20, 2)) + [20]


@pytest.mark.parametrize("shift", RUN_IN_SHIFTS)
def test_every_seam_misleads_its_run_in_and_nobody_gives_up(shift):
    """Part 3's stream at the three placements of the block grid: sweep 1 lists more than two grids and 64 blocks; no two of
    them are neighbours, except among the first two and the last six blocks, which sweep 0 takes one by one; every listed block's first lane is on the
    true chain within 1 024 bits -- four lanes of the block's 256, four of sweep 1's eight trips --, so no exit moves and ONE
    listed sweep settles them all; and no block holds a run of unsettled lanes at the first sweep's trip cap, let alone at
    CERTAIN_FROM: nobody gives up."""
    data_t, len_t, text, body = run_in_stream()
    listed, merged, misled = listed_in_sweep_1(shift)
    n_blocks = (shift + len(body) + W.BLOCK_BYTES - 1) // W.BLOCK_BYTES
    print(f"grid + {shift} bytes: {n_blocks} blocks, {misled} seams mislead a run-in, sweep 1 lists {listed.size} blocks: {listed.size - 2 * WINDOW_LISTED_GRID} more than two strides of {WINDOW_LISTED_GRID}; on the true chain after at most {int(merged.max())} bits")
    assert decode_path(E.Codebook.from_tables(data_t, len_t)) == N.ET_PATH_WINDOWS
    assert n_blocks >= RUN_IN_BLOCKS and misled >= RUN_IN_BLOCKS - 1  # every seam with a stretch laid over it
    assert listed.size >= 2 * WINDOW_LISTED_GRID + 64
    assert (np.diff(listed[(listed >= 2) & (listed < n_blocks - 6)]) >= 2).all()
    assert int(merged.min()) >= 0 and int(merged.max()) < 1024 < W.BLOCK_BITS  # (-1: not within seam_walks' reach)
    bounds = W.TextBounds(8 * shift, len_t, text)
    for lane_bits, runs in zip((256, 512), W.unsettled_block_runs_by_text(bytes(shift) + body, 8 * shift, data_t, len_t, text, ((256, 128), (512, 128)), bounds=bounds)):
        print(f"  lanes of {lane_bits} bits: the longest run of unsettled lanes in a block is {int(runs.max())}")
        assert runs.size == n_blocks and int(runs.max()) < FIRST_SWEEP_TRIPS < CERTAIN_FROM["windows"]
