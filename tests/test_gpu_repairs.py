"""GPU: the listed repair sweeps past ONE grid of listed blocks, and the give-up rule at its edge.

The sweep families end by repairing the blocks whose start contradicts the exit of the block before: those go on a worklist, and a
listed sweep walks it with a capped grid and a stride -- k_dec_sync_reg<false, false> with min(n_blocks, 512) workgroups stepping
wi += gridDim.x (also sweep 1 of every whole-stream window decode), k_tw_sync with at most 64 workgroups of 8 wavefronts stepping
it += gridDim.x * waves_per_group.  A stride that skipped blocks would not show in the bytes: repair_sweeps sweeps until nothing
changes, and the skipped blocks are picked up a grid at a time by the sweeps that follow.  Only the NUMBER of sweeps tells, so
that is what is pinned here: sync_iters with more than two grids of listed blocks equals sync_iters with one listed block.

Beside it, the rule that host and device apply alike -- n_gave_up * 64 > n_blocks sends the decode to the plan's fallback
(body_first_sweep), and the speculative write declines by dec_state_final -- at equality and one block short of it.

The streams are tiled on the device from ONE period that tests/test_repairs_host.py checks on the host (which blocks give up,
how each family counts them, how many blocks are listed and that they are no neighbours); the reference of the bytes is the
oracle's packer and the tiling.  Every comparison is exact and made on the device, between guard bytes."""
import functools
import time

import numpy as np
import pytest

from tests import bitwalk as W
from tests.test_gpu_syncwork import BITS, CERTAIN_FROM, FAMILY, GAVE_UP, LANES, _timed, check_what_ran
from tests.test_repairs_host import FAMILIES, G, MANY_PERIODS, PERIOD_BLOCKS, RUN_IN_SHIFTS, listed_in_sweep_1, period, run_in_stream

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 64
# one stretch that cannot settle: the first sweep (and the windows' second), the verification that fails, ONE repair sweep that
# settles every listed block -- their exits do not move, nobody else is touched -- and the one that finds nothing to do
REPAIRED = {f: (FAMILY[f][0] + 2, FAMILY[f][1]) for f in FAMILIES}


class _Out:
    """GUARD bytes of FILL, `room` bytes, GUARD bytes of FILL on the device; .room begins on a 16-byte boundary.  Looked at on the
    device (a snapshot of gigabytes on the host is what tests/guards.py Guarded would take)."""

    def __init__(self, room):
        import torch

        self.buf = torch.full((GUARD + room + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.room = self.buf[GUARD : GUARD + room]
        assert self.room.data_ptr() % 16 == 0

    def refill(self):
        self.buf.fill_(FILL)

    def assert_holds(self, want, m, what):
        """The first m bytes are want[:m]; nothing in front of the room and nothing from byte m on was written."""
        import torch

        assert m == want.numel(), f"{what}: {m} symbols for {want.numel()}"
        assert bool((self.buf[:GUARD] == FILL).all()), f"{what}: the front guard was written"
        assert bool((self.buf[GUARD + m :] == FILL).all()), f"{what}: bytes behind out_len = {m} were written"
        if not torch.equal(self.room[:m], want):
            at = int(torch.nonzero(self.room[:m] != want)[0])
            raise AssertionError(f"{what}: symbol {at} of {m} is {int(self.room[at])} for {int(want[at])}")


def _codebook(family):
    import entreepy_amd as E

    data_t, len_t = period(family)[:2]
    return E.Codebook.from_tables(data_t, len_t)


def _upload(a):
    import torch

    d = torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy() if not isinstance(a, np.ndarray) else np.array(a)).cuda()
    assert d.data_ptr() % 256 == 0  # the block grid is the body's
    return d


def _decode(ctx, cb, body, declared, out, what):
    out.refill()
    t0 = time.perf_counter()
    m, iters, bits = _timed(ctx, lambda: ctx.decode_body_device(cb, body, declared, out.room, 0))
    print(f"{what}: {body.numel() // W.BLOCK_BYTES} blocks, {m} symbols, sync_iters {iters}, bits {[b for b in BITS if bits[b]]}, {time.perf_counter() - t0:.3f} s")
    return m, iters, bits


# ---- part 2: more listed blocks than two grids ----------------------------------------------------------------------------------


@pytest.mark.parametrize("family", FAMILIES)
def test_listed_sweeps_reach_every_block_beyond_two_grids(ctx, family):
    """MANY_PERIODS = 1 088 copies of the period on the device (139 264 blocks, 1.06 GiB of body, 2.9 GiB of text; about 8 GB of
    device memory with the expected text and the workspaces): every copy lists ONE block for repair_sweeps, 128 blocks from the
    next -- 1 088 listed blocks, two whole strides and 64 blocks of a third for both families (windows: a grid of 512 workgroups;
    tree walk: 64 workgroups of 8 wavefronts for this table's 42 rows, 64 * 8 = 512 blocks per stride, launch_tw_sync's
    arithmetic in tests/test_repairs_host.py) -- and gives up g = 2 times in 128 blocks, so the sweeps stay.  The smallest
    stream that reaches a third stride: one listed block costs 128 blocks by the 1/64 rule.

    sync_iters EQUALS that of ONE copy on the same context, and that is the reasoned count: the family's base, one repair sweep
    that settles every listed block, one that finds none.  1 088 independent stretches need no more sweeps than one if and only
    if the stride reaches all of them in one launch; a workgroup that left after its first listed block would add two sweeps.
    Twice: the second decode runs on the workspaces the first left.  Beside it the count, every byte, the guards, the planned
    family's bits and no exhaustive_sync."""
    import torch

    data_t, len_t, text, body, _ = period(family)
    cb = _codebook(family)
    need = MANY_PERIODS * (len(body) + 2 * text.size) + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{need >> 20} MiB of device memory needed, {free >> 20} MiB free")
    d_body, d_text = _upload(body), _upload(text)
    out = _Out(text.size)
    m, iters, bits = _decode(ctx, cb, d_body, text.size, out, f"{family}, 1 period")
    out.assert_holds(d_text, m, "one period")
    assert (iters, bits) == REPAIRED[family], (iters, bits)
    del out
    t0 = time.perf_counter()
    many_body, many_text = d_body.repeat(MANY_PERIODS), d_text.repeat(MANY_PERIODS)
    assert many_body.data_ptr() % 256 == 0
    out = _Out(many_text.numel())
    torch.cuda.synchronize()
    print(f"{family}: {MANY_PERIODS} periods tiled in {time.perf_counter() - t0:.3f} s, {(many_body.numel() + 2 * many_text.numel()) >> 20} MiB on the device")
    for turn in range(2):
        m, many_iters, many_bits = _decode(ctx, cb, many_body, many_text.numel(), out, f"{family}, {MANY_PERIODS} periods (turn {turn})")
        out.assert_holds(many_text, m, f"{MANY_PERIODS} periods")
        assert many_iters == iters, f"{many_iters} synchronisation launches for {MANY_PERIODS} listed blocks, {iters} for one: a listed sweep did not reach every block"
        assert many_bits == bits and not many_bits["exhaustive_sync"]
        assert many_bits["tree_walk_sync"] == (family == "tree_walk")


# ---- part 3: window sweep 1 over more than two grids of failed run-ins, nobody gives up -------------------------------------------


@pytest.fixture(scope="module")
def run_ins_on_device():
    """Part 3's body with 4 bytes of room in front (0xff around it: the bits behind a stream's end count as zeros) and its text."""
    import torch

    _, _, text, body = run_in_stream()
    d = torch.full((4 + len(body) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    assert d.data_ptr() % 256 == 0
    return d, _upload(np.frombuffer(body, dtype=np.uint8)), _upload(text)


@pytest.mark.parametrize("shift", RUN_IN_SHIFTS)
def test_sweep_1_settles_more_than_two_grids_of_failed_run_ins(ctx, run_ins_on_device, shift):
    """tests/guards.py failed_run_ins: 2 304 blocks (18 MiB) whose every seam lies in a short flat stretch -- the first lane of
    every block runs in blind on the wrong phase and begins where no codeword does.  Sweep 0 settles the odd seams inside its
    superblocks; the even ones, 1 152 by the reference (tests/test_repairs_host.py: more than two grids of 512 and 64 blocks, no
    neighbours, no exit moves, nobody gives up), are what sweep 1 lists and walks with its stride.  The family's row of launches
    EXACTLY: sweep 0, the one listed sweep, the verification -- and the speculative write kept (a block the stride skipped
    fails the verification: repair_sweeps, a second write).  Twice; with the body at an aligned address and 1 and 3 bytes behind
    one, which moves every seam 8 and 24 bits along the body."""
    import entreepy_amd as E

    data_t, len_t, _, _ = run_in_stream()
    room, d_body, d_text = run_ins_on_device
    listed, _, _ = listed_in_sweep_1(shift)
    room.fill_(0xFF)
    room[shift : shift + d_body.numel()] = d_body
    body = room[shift : shift + d_body.numel()]
    cb = E.Codebook.from_tables(data_t, len_t)
    out = _Out(d_text.numel())
    for turn in range(2):
        m, iters, bits = _decode(ctx, cb, body, d_text.numel(), out, f"windows, grid + {shift} bytes, {listed.size} blocks listed by the reference (turn {turn})")
        out.assert_holds(d_text, m, f"grid + {shift}")
        assert (iters, bits) == FAMILY["windows"], (iters, bits)


# ---- part 4: the give-up rule at equality and one block short --------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _longest_run(family):
    """The reference's longest run of unsettled lanes in a block of the tiled period (three copies), in the family's geometry."""
    data_t, len_t, text, body, _ = period(family)
    return int(W.unsettled_block_runs_by_text(body * 3, 0, data_t, len_t, np.tile(text, 3), (LANES[family],), "skip" if family == "windows" else "stop")[0].max())


class _Edge:
    """Two periods of 64 * g blocks: n_gave_up * 64 == n_blocks.  whole(): the body as it is; short(): less its last 8 KiB block,
    as many symbols declared as codewords END inside it (the text's cumulative code lengths)."""

    def __init__(self, ctx, family):
        data_t, len_t, text, body, island_block = period(family)
        self.ctx, self.family, self.cb = ctx, family, _codebook(family)
        self.body, self.text = _upload(body).repeat(2), _upload(text).repeat(2)
        assert self.body.data_ptr() % 256 == 0 and self.body.numel() == 2 * PERIOD_BLOCKS[family] * W.BLOCK_BYTES
        self.n_blocks = 2 * PERIOD_BLOCKS[family]
        assert 2 * G[family] * 64 == self.n_blocks and island_block + 1 < PERIOD_BLOCKS[family] - 1
        ends = np.cumsum(len_t[np.tile(text, 2)].astype(np.int64))
        self.short_symbols = int(np.searchsorted(ends, (self.n_blocks - 1) * W.BLOCK_BITS, side="right"))
        assert 0 < 2 * text.size - self.short_symbols < W.BLOCK_BITS // 2
        self.run = _longest_run(family)
        assert self.run >= CERTAIN_FROM[family]
        self.out = _Out(self.text.numel())

    def whole(self):
        """(a) equality: the sweeps stay -- the listed repair, a second, non-speculative write -- and the fallback does not run."""
        m, iters, bits = _decode(self.ctx, self.cb, self.body, self.text.numel(), self.out, f"{self.family}, gave up * 64 == {self.n_blocks} blocks")
        self.out.assert_holds(self.text, m, "at equality")
        check_what_ran(self.family, self.run, True, iters, bits)
        assert not bits["exhaustive_sync"] and (iters, bits) == REPAIRED[self.family], (iters, bits)

    def short(self):
        """(b) one block short: the same give-ups in n_blocks - 1 blocks, and the plan's fallback runs."""
        m, iters, bits = _decode(self.ctx, self.cb, self.body[: -W.BLOCK_BYTES], self.short_symbols, self.out, f"{self.family}, gave up * 64 > {self.n_blocks - 1} blocks")
        self.out.assert_holds(self.text[: self.short_symbols], m, "one block short")
        check_what_ran(self.family, self.run, True, iters, bits)
        assert (iters, {**bits, "strips_write": False}) == GAVE_UP[self.family, "exit_maps"], (iters, bits)


@pytest.mark.parametrize("family", FAMILIES)
def test_give_ups_at_exactly_a_64th_of_the_blocks_keep_the_sweeps(ctx, family):
    _Edge(ctx, family).whole()


@pytest.mark.parametrize("family", FAMILIES)
def test_give_ups_one_block_beyond_a_64th_take_the_fallback(ctx, family):
    _Edge(ctx, family).short()


@pytest.mark.parametrize("family", FAMILIES)
def test_both_sides_of_the_give_up_rule_on_one_context(ctx, family):
    """(a) and (b) alternating with nothing in between, in either order: a flag or ticket word that one leaves behind is met by
    the other -- a `>` turned `>=` on the host's side or the device's alone leaves an output unwritten or written from a state
    that is not final."""
    e = _Edge(ctx, family)
    for step in (e.whole, e.short, e.whole, e.short, e.short, e.whole):
        step()
