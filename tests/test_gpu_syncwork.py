"""GPU: what the decode's synchronisation RAN and what it RETURNED, not only the bytes behind it.

The decode repairs itself (csrc/et_decode.cpp: a first sweep guesses, a scan verifies, repair sweeps and fallback families
redo what failed), so a synchronisation kernel that is subtly wrong still gives the right bytes -- at the price of launches a
clean stream never needs, or of a family its code table should never see.  Here the launches are counted and the families named
for every kind of stream, and the range calls' (start, exit, count), their maps and their symbols are compared, entry for
entry, with the serial walk of tests/bitwalk.py.  tests/test_syncwork_host.py checks the reference and the fixtures without a GPU.
Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bitwalk as W
from tests.conftest import ROOT
from tests.test_syncwork_host import BODY_LAYOUTS, FIXTURES, body_layout, decode_path, fixture

pytestmark = pytest.mark.gpu

# ---- ONE table: what a whole-stream decode of each family launches and reports ----------------------------------------------------
# sync_iters as csrc/et_decode.cpp counts it -- body_first_sweep (the tree walk: sweep + verification = 2; the windows: sweep,
# repair sweep, verification = 3), body_exhaustive (the row walk + 1, k_fixed_sync + 1, the exit maps + 5, k_fixed_write nothing:
# d.iters stays where BodyDecode{} put it), repair_sweeps (+ 1 per sweep) -- and the path bits of body_timings.
BITS = ("exhaustive_sync", "tree_walk_sync", "chained_write", "row_sync", "fixed_sync", "strips_write")


def _row(sync_iters, *bits_set):
    assert set(bits_set) <= set(BITS)
    return sync_iters, {b: b in bits_set for b in BITS}


FAMILY = {
    "tree_walk": _row(2, "tree_walk_sync", "chained_write"),
    "windows": _row(3),
    "rows": _row(1, "exhaustive_sync", "row_sync", "chained_write"),
    "fixed_write": _row(0, "exhaustive_sync", "fixed_sync"),
    "fixed_sync": _row(1, "exhaustive_sync", "fixed_sync", "chained_write"),
    "exit_maps": _row(5, "exhaustive_sync", "chained_write"),
}
# a first sweep whose blocks give up hands the stream on: the sweep's count plus the fallback's share, the fallback's bits beside the sweep's
# (the window sweeps start only where the code is no tree: the row walk is not theirs to fall back on, and the exit maps behind them
# write over the window tables, there being no chained ones)
GAVE_UP = {("tree_walk", fb): (FAMILY["tree_walk"][0] + FAMILY[fb][0], {b: FAMILY["tree_walk"][1][b] or FAMILY[fb][1][b] for b in BITS}) for fb in ("rows", "exit_maps")}
GAVE_UP[("windows", "exit_maps")] = (FAMILY["windows"][0] + FAMILY["exit_maps"][0], _row(0, "exhaustive_sync")[1])
WHOLE = {"text": "tree_walk", "midsummer": "tree_walk", "enwik": "tree_walk", "two_len_quick": "tree_walk", "two_len_slow": "exit_maps",
         "rows": "rows", "fixed": "fixed_write", "sparse": "windows"}  # the family a whole-stream decode of each fixture runs
RANGE_SYNC = {"text": "tree_walk", "midsummer": "tree_walk", "enwik": "tree_walk", "sparse": "windows", "skewed_flat": "windows"}  # ... and et_decode_range_sync
# ... and et_decode_range_maps; the last three under hand-made tables with bit patterns that are nobody's codeword, which the
# reference passes over as the window kernels do (tests/bitwalk.py, unmatched="skip")
RANGE_MAPS = {"two_len_quick": "exit_maps", "two_len_slow": "exit_maps", "rows": "rows", "sparse": "exit_maps", "holes200": "exit_maps", "skewed_flat": "exit_maps",
              "junk/sparse": "exit_maps", "junk/holes200": "exit_maps"}  # (random bytes: the rule in every block of a range, the interior ones too)
# the switches, each on the fixture whose family it takes away, and where the table says the work goes
SWITCHES = [("ET_NO_ROW_SYNC", "rows", "exit_maps"), ("ET_NO_FIXED_SYNC", "fixed", "exit_maps"), ("ET_NO_QUICK_SYNC", "two_len_quick", "exit_maps"),
            ("ET_NO_FIXED_WRITE", "fixed", "fixed_sync")]


def _path_name(path):
    from entreepy_amd import _native as N

    return {N.ET_PATH_TREE_WALK: "tree_walk", N.ET_PATH_WINDOWS: "windows", N.ET_PATH_ROWS: "rows", N.ET_PATH_FIXED: "fixed_write", N.ET_PATH_EXIT_MAPS: "exit_maps"}[path]


def test_the_table_and_the_planner_agree_on_every_fixture():
    assert {k: _path_name(v[0]) for k, v in FIXTURES.items()} == WHOLE


# ---- decodes with the timing on ----------------------------------------------------------------------------------------------------


def _timed(ctx, call):
    ctx.enable_timing(True)
    try:
        m = call()
        t = ctx.timings("decode")
    finally:
        ctx.enable_timing(False)
    return m, int(t["sync_iters"]), {b: bool(t[b]) for b in BITS}


def _upload(fx):
    """The stream on the device, 16 bytes of zeros in front of its 4-byte aligned base and 64 behind its end -> (tensor, the stream's view)."""
    import torch

    d = torch.zeros(16 + fx.n_bytes + 64, dtype=torch.uint8, device="cuda")
    d[16 : 16 + fx.n_bytes] = torch.from_numpy(fx.stream.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    return d, d[16 : 16 + fx.n_bytes]


def _decode_image(ctx, fx):
    """decode_device of the fixture's .et image -> (bytes, sync_iters, bits)."""
    import torch

    comp = torch.from_numpy(np.frombuffer(fx.comp, dtype=np.uint8).copy()).cuda()
    out = torch.empty(fx.text.size + 64, dtype=torch.uint8, device="cuda")
    m, iters, bits = _timed(ctx, lambda: ctx.decode_device(comp, out))
    return out[:m].cpu().numpy().tobytes(), iters, bits


def _decode_body(ctx, fx):
    """decode_body_device of the fixture's body where it lies: fx.shift bytes behind an aligned address, from bit fx.start_bit."""
    import torch

    _, stream = _upload(fx)
    out = torch.empty(fx.text.size + 64, dtype=torch.uint8, device="cuda")
    cb = fx.codebook()
    m, iters, bits = _timed(ctx, lambda: ctx.decode_body_device(cb, stream[fx.shift :], fx.text.size, out, fx.start_bit))
    return out[:m].cpu().numpy().tobytes(), iters, bits


def _decode(ctx, fx):
    return _decode_body(ctx, fx) if fx.name == "sparse" else _decode_image(ctx, fx)  # (the hand-made dictionary has no image)


def _clean(name):
    return FIXTURES.get(name.split("+")[0], (None, False))[1]


def _check_whole(ctx, fx, family, clean):
    """Twice on one context: the oracle's bytes, the family's launches, the family's bits."""
    want_iters, want_bits = FAMILY[family]
    for turn in range(2):
        got, iters, bits = _decode(ctx, fx) if "+" not in fx.name else _decode_body(ctx, fx)
        print(f"{fx.name} (turn {turn}): family {family}, sync_iters {iters}, bits {[b for b in BITS if bits[b]]}")
        assert got == fx.text.tobytes(), fx.name
        assert bits == want_bits, (fx.name, bits)
        if clean or family != "tree_walk":
            assert iters == want_iters, f"{fx.name}: {iters} synchronisation launches, the {family} family's count is {want_iters}"
        else:  # lanes far from the truth (tests/test_syncwork_host.py): repair sweeps are in order, fewer launches than the base are not
            assert iters >= want_iters, (fx.name, iters)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_what_a_whole_stream_decode_ran(ctx, name):
    """(a) On a clean fixture, sync_iters above the base means a repair sweep ran on a stream that needs none."""
    _check_whole(ctx, fixture(name), WHOLE[name], _clean(name))


@pytest.mark.parametrize("name", ["text", "rows"])
def test_what_a_body_decode_ran_at_every_alignment(ctx, name):
    """(a) through decode_body_device: the body 0 to 3 bytes behind an aligned address, from bit 0 and bit 5 -- the first
    lane's known start (k_tw_sync's known_bit, the row walk's first_bit) at every value it takes."""
    for shift, start_bit in BODY_LAYOUTS:
        fx = body_layout(name, shift, start_bit)
        assert (fx.shift, fx.start_bit) == (shift, start_bit)
        _check_whole(ctx, fx, WHOLE[name], _clean(name))


def child_main(name, family):
    """(b), in the child process: the fixture under the switch the parent has set."""
    import entreepy_amd as E

    with E.Context(0) as c:
        _check_whole(c, fixture(name), family, False)
    print("ok")


@pytest.mark.parametrize("switch,name,family", SWITCHES)
def test_the_switches_move_the_work_where_the_table_says(switch, name, family):
    """(b) ET_NO_ROW_SYNC, ET_NO_FIXED_SYNC, ET_NO_QUICK_SYNC (and ET_NO_FIXED_WRITE, for the table's k_fixed_sync row) in a
    child process each (the switches are read once): the bytes unchanged, the launches and bits the fallback's row -- so (a)
    does notice a change of path."""
    code = f"from tests import test_gpu_syncwork as T; T.child_main({name!r}, {family!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **{switch: "1"}), timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


# csrc/et_kernels.h: a block still unsettled at trip DEC_FIRST_SWEEP_TRIPS of the first sweep gives up; the window sweeps'
# second sweep, which is part of their base count, has DEC_REPAIR_SWEEP_TRIPS more
FIRST_SWEEP_TRIPS, REPAIR_SWEEP_TRIPS = 6, 8
# what a lane is to each sweep family: (bits of its own, bits it runs in over); a block is 8 KiB of them
LANES = {"tree_walk": (W.LANE_BITS, W.RUN_IN_BITS), "windows": (256, 128)}  # k_tw_sync; k_dec_sync: SUB_BITS, DEC_WARMUP_BITS
# the unsettled lanes in a row that make "not clean" certain: the tree walk's block gives up and nothing in its base count
# repairs it; a window block that gave up is taken up again by the second sweep, so the run must outlast that one too
CERTAIN_FROM = {"tree_walk": FIRST_SWEEP_TRIPS, "windows": FIRST_SWEEP_TRIPS + REPAIR_SWEEP_TRIPS}


def check_repair_reach(ctx, comp, want, certain):
    """(c) A stream written to reach the give-up and repair code: the oracle's bytes; what the decode ran, printed; and whether
    it still REACHES that code, as far as that follows from the input alone.  A lane whose blind run-in is not on the true
    chain before the lane's own bits end leaves them wrongly until the lane before hands it its true start, one lane per trip
    of the block's fixed point; a block with CERTAIN_FROM or more such lanes in a row cannot settle within the trips its
    family's base count holds: it gives up (its start marked), and the verification sends the stream to repair sweeps or, if
    enough blocks gave up, to the fallback family.  certain: what the test says of its input -- the reference is certain of
    that; held against the reference here, and, where True, against the timing: more synchronisation launches than the base
    of the family the planner starts the stream on, or the exhaustive bit ("not clean").  Where NO lane is unsettled the
    stream meets the clean condition, and the timing must show the tree walk's base and nothing else.  In between the
    reference does not decide (a lane that is right by accident can be talked out of it by its neighbour), and only the bytes
    are checked.  A lane whose blind walk meets a bit pattern without a codeword: where the planner starts on the window sweeps
    the reference steps over it as they do, and the lane is judged like any other; where it starts on the tree walk, whose
    table makes a leaf of such a pattern, the lane's distance is NEVER -- nobody's to judge, it ends a run."""
    import entreepy_amd as E

    cb, _, off = E.parse_header(comp)
    planned = _path_name(decode_path(cb))
    assert planned in LANES, planned
    # (the image as a 4-byte aligned upload holds it: lanes count from the aligned word the body starts in)
    # (the window kernels pass a bit pattern without a codeword over bit by bit, and so does the reference for them: every lane is
    # judged; under the tree walk such a pattern is a leaf, which the reference does not follow: NEVER, and the lane ends a run)
    run = W.longest_unsettled_run(comp[off & ~3 :], (off & 3) * 8, cb.data, cb.length, *LANES[planned], unmatched="skip" if planned == "windows" else "stop")
    assert (run >= CERTAIN_FROM[planned]) == certain, f"the longest run of unsettled lanes in a block is {run}"
    back, iters, bits = _timed(ctx, lambda: ctx.decode(comp))
    assert back == want
    return check_what_ran(planned, run, certain, iters, bits)


def check_what_ran(planned, run, certain, iters, bits):
    """check_repair_reach's judgement of the timing, for a decode the caller has made (tests/test_gpu_repairs.py: a body on
    the device): planned, the family the planner starts the stream on; run, the reference's longest run of unsettled lanes in a
    block; certain, as there."""
    ran = (planned, iters, [b for b in BITS if bits[b]])
    print(f"longest unsettled run {run} lanes; planned family, sync_iters, bits: {ran}")
    if certain:
        assert iters > FAMILY[planned][0] or bits["exhaustive_sync"], f"the stream decoded like a clean one: {ran}"
    elif run == 0 and planned == "tree_walk":
        assert iters == FAMILY[planned][0] and not bits["exhaustive_sync"], f"a clean stream took a repair: {ran}"
    if bits["exhaustive_sync"]:  # given up: the sweep's launches and the fallback's, whichever the fallback is
        assert (iters, {**bits, "strips_write": False}) in [GAVE_UP[k] for k in GAVE_UP if k[0] == planned], ran
    return ran


# ---- the range calls against the walk ----------------------------------------------------------------------------------------------------


class _Range:
    """One context's range calls on one uploaded stream, and the reference's answers to compare them with."""

    def __init__(self, ctx, fx):
        import torch

        self.ctx, self.fx, self.cb = ctx, fx, fx.codebook()
        self.keep, self.d = _upload(fx)
        self.buf = torch.empty(fx.at.size + 64, dtype=torch.uint8, device="cuda")
        self.jumps = W.Jumps(fx.L, fx.C) if fx.n_bits < (1 << 21) else None

    def walk(self, begin, end, start):
        """-> (start_bit, exit_bit, n_symbols) of the serial walk from bit `start` of the range."""
        exit_bit, at = self.fx.range_walk(begin, end, start)
        if self.jumps is not None:  # (the same by pointer doubling, where the stream is small enough for it)
            exits, counts = self.jumps.walk([begin * 8 + start], [end * 8])
            assert (int(exits[0]) - end * 8, int(counts[0])) == (exit_bit, at.size)
        return start, exit_bit, at.size

    def symbols(self, begin, end, start):
        return self.fx.S[self.fx.range_walk(begin, end, start)[1]]

    def sync(self, begin, end, start):
        info = self.ctx.decode_range_sync(self.cb, self.d, begin, end, start)
        assert info["tree_walk"] == (RANGE_SYNC.get(self.fx.name, "windows") == "tree_walk")
        return info

    def written(self, count):
        m = self.ctx.decode_range_write(count, self.buf)
        assert m == count
        return self.buf[:m].cpu().numpy()


def _triple(info):
    return info["start_bit"], info["exit_bit"], info["n_symbols"]


@pytest.mark.parametrize("name", list(RANGE_SYNC))
def test_range_sync_is_the_serial_walk(ctx, name):
    """(d) Ranges of 1, 2 and 5 blocks at every block boundary, the last ones ending with the stream.  From the TRUE start:
    (start, exit, count) and the symbols are the walk's, and a clean stream takes the tree walk one sweep.  From an UNKNOWN
    start: whatever start the range reports, exit, count and symbols are the walk's from THAT bit; a range whose blind run-in
    (bitwalk.merge_distances: 128 bits in front of it) is on the true chain before the range begins reports the true start;
    where the start is not the true one, ONE call with the true start gives the truth.  From a WRONG known start (the true
    one + 1; under the hand-made dictionaries that bit may begin no codeword: the reference steps over such bits as the window
    kernels do): the walk from that bit; the call with the true start that follows gives the truth again (for the window
    sweeps the repair of the states that stand, same_range_again; for the tree walk a fresh sweep)."""
    fx = fixture(name)
    r = _Range(ctx, fx)
    tree, clean = RANGE_SYNC[name] == "tree_walk", _clean(name)
    dist = W.merge_distances(fx.L, fx.on_chain, C=fx.C)
    unknown = repaired = 0
    for begin, end in fx.cuts():
        s, x, n, syms = fx.truth(begin, end)
        assert (s, x, n) == r.walk(begin, end, s)

        def truth_from_the_true_start():
            info = r.sync(begin, end, s)
            assert _triple(info) == (s, x, n), (begin, end, info)
            assert np.array_equal(r.written(n), syms), (begin, end)
            return info

        info = truth_from_the_true_start()
        if tree and clean:
            assert info["sweeps"] == 1, (begin, end, info)
        if begin:  # an inner range: its start unknown
            unknown += 1
            info = r.sync(begin, end, -1)
            got = info["start_bit"]
            assert got < 32 and _triple(info) == r.walk(begin, end, got), (begin, end, info)
            assert np.array_equal(r.written(info["n_symbols"]), syms if got == s else r.symbols(begin, end, got)), (begin, end)
            if got != s:
                assert dist[begin * 8 // W.LANE_BITS] > W.RUN_IN_BITS, f"range at byte {begin}: its run-in is on the true chain {dist[begin * 8 // W.LANE_BITS]} bits on, yet it reports start {got} for {s}"
                repaired += 1
                truth_from_the_true_start()
        wrong = s + 1
        assert wrong < 32
        info = r.sync(begin, end, wrong)
        assert _triple(info) == r.walk(begin, end, wrong), (begin, end, wrong, info)
        assert np.array_equal(r.written(info["n_symbols"]), r.symbols(begin, end, wrong)), (begin, end, wrong)
        truth_from_the_true_start()
    print(f"{name}: {repaired} of {unknown} ranges with an unknown start reported another start than the true one and took the repair call")


def _check_maps(r, begin, end, by_rows, n_starts):
    """(e) for one range: every entry of the map, the resolve and the write for every start offset, the map of a known start."""
    fx, ctx = r.fx, r.ctx
    m, k = ctx.decode_range_maps(r.cb, r.d, begin, end, -1)
    assert k == n_starts
    walks = [fx.range_walk(begin, end, p) for p in range(k)]  # (exit bit, where the codewords begin)
    assert list(m[:k]) == [e for e, _ in walks], (begin, end, list(m))
    assert list(m[k:]) == list(range(k, 32)), (begin, end, list(m))
    for p, (exit_, at) in enumerate(walks):  # every start, on the one context, one resolve after the other
        info = ctx.decode_range_resolve(p)
        assert _triple(info) == (p, exit_, at.size) and info["row_walk"] == by_rows, (begin, end, p, info)
        assert np.array_equal(r.written(at.size), fx.S[at]), (begin, end, p)
    s, x, n, syms = fx.truth(begin, end)
    if fx.text.size == 0:  # junk: no text and no chain of codewords alone; "the true start" is the walk's from bit 0, what follows the walk from there
        x, at = fx.range_walk(begin, end, s)
        n, syms = at.size, fx.S[at]
    else:
        assert (x, n) == fx.range_count(begin, end, s)
    if s < k:  # (the stream's first range begins up to 3 bytes in: its true start need not be one of the map's)
        assert (x, n) == (walks[s][0], walks[s][1].size)
    known, k = ctx.decode_range_maps(r.cb, r.d, begin, end, s)
    assert k == n_starts and list(known) == [x] * 32, (begin, end, s, list(known))
    info = ctx.decode_range_resolve(s)
    assert _triple(info) == (s, x, n), (begin, end, info)
    assert np.array_equal(r.written(n), syms), (begin, end)


@pytest.mark.parametrize("name", list(RANGE_MAPS))
def test_exit_maps_every_entry(ctx, name):
    """(e) et_decode_range_maps over ranges of 1, 2 and 5 blocks and the ragged last ones: map[p] is where the walk from bit p
    of the range leaves it, for EVERY p below n_starts (the longest codeword; 8 for a row code), p itself behind that; with the
    start known every entry is that start's exit.  et_decode_range_resolve(p) and the write that follows give the walk from p
    -- its start, exit, count and symbols -- for every p, not only the true one."""
    fx = fixture(name)
    r = _Range(ctx, fx)
    by_rows = RANGE_MAPS[name] == "rows"
    n_starts = 8 if by_rows else int(fx.length.max())
    for begin, end in fx.cuts():
        _check_maps(r, begin, end, by_rows, n_starts)


def test_exit_maps_composed_over_more_than_one_group(ctx):
    """(e) 257 blocks of the slow two-length code in ONE range (a group of exit maps is 256 blocks, the groups' maps are
    composed on the host), two more blocks of stream behind it."""
    fx = fixture("two_len_slow_big")
    assert fx.n_blocks >= 259
    _check_maps(_Range(ctx, fx), 0, 257 * W.BLOCK_BYTES, False, int(fx.length.max()))
