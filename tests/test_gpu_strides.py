"""GPU: the stride loops of csrc/et_batch.hip that no other test takes through a second trip -- the join's KEY side (k_join_build past
JOIN_GRID tiles of keys, and k_join_hash likewise), the take's and the gather's plan (k_take_plan, k_gather_plan past PLAN_GRID * LANES
rows) with several copy tiles per workgroup behind it (k_take_copy's `per` >= 2, staged and in place), and the number call (k_number_plan,
k_number_long, k_number_fold past one grid of rows, k_number_fill past one grid of GROUPS).  tests/test_gpu_select.py does this for the
record side of the selecting calls and tests/test_gpu_derived.py for the derived stores; the style is theirs: fixtures are made with
numpy or tiled from a small cycle, the answer for one cycle (or for the distinct texts) is each family's own Python reference -- a dict
for the join, model() for the take, want_rows() for the gather, want_number() for the number call -- and numpy spreads it over the whole
store; every output is compared exactly.  Every test asserts its own reach: the count against the cap, and the place of each special
item behind it, so that a fixture that shrinks below a cap fails its test.  tests/test_strides_host.py checks the builders without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus
from tests.test_gpu_derived import tiled
from tests.test_gpu_gather import check_gather, make_store, run_gather, upload, want_rows
from tests.test_gpu_join import LANE_BYTES, NONE as JOIN_NONE, NOT, device_hashes, host_hash, run_join
from tests.test_gpu_match import ROW_SENTINEL, TILE, _pack, _store
from tests.test_gpu_number import I64_MAX, I64_MIN, N_BAD, N_EMPTY, N_OK, N_RANGE, NONE as GROUP_NONE, TO_END, check_number, lane_bytes as number_lane_bytes, reach, run_number, \
    want_number, wrap64
from tests.test_gpu_order import WRAP_NEEDLE
from tests.test_gpu_packed import _index_of
from tests.test_gpu_select import BAD as REC_BAD, JOIN_LONG as REC_LONG, N as N_WRAPPED, check_rows, device_store, raw_class, select_store
from tests.test_gpu_take import C, check_take, model, raw_store, run_take
from tests.test_shared_host import oracle_table, table_2bit

pytestmark = pytest.mark.gpu

OK, ARG = 0, 6  # et_status
JOIN_GRID, TAKE_GRID = 2048, 2048  # csrc/et_batch.h JOIN_GRID, TAKE_GRID
PLAN_GRID, LANES, LONG_GRID = 1024, 256, 1024  # csrc/et_batch.h GATHER_PLAN_GRID, csrc/et_batch.hip BB, csrc/et_batch.h SHARED_DEC_GRID
STAGE_ROWS = 1024  # entries of out_body_index k_take_copy keeps in LDS for a tile (csrc/et_batch.h TAKE_STAGE_ROWS); C is TAKE_TILE_BYTES
KEY_TRIP = JOIN_GRID * TILE  # the first key of k_join_build's second trip
N_KEYS = KEY_TRIP + 300  # a second trip of two tiles, the last one partial
ROW_TRIP = PLAN_GRID * LANES  # the first row, and the first group, of a plan kernel's second trip
N_ROWS = ROW_TRIP + 65  # a second trip of 65 rows: one whole wavefront and one row of the next
N_GROUPS = ROW_TRIP + 65


# --- 1. the join's key side ------------------------------------------------------------------------------------------------------------
SYMBOLS = 10  # of a numbered key: 20 bits under the 2-bit table, 3 bytes of body
ODD = 0x9E375  # i -> i * ODD modulo 4^10 is one-to-one: key i's number, so that neighbours in the store are no neighbours in the text
STRANGERS = KEY_TRIP + 1000  # numbers from number_of(STRANGERS) on are the text of no key
KEY_BAD = N_KEYS - 1  # the key whose pair of body offsets decreases


def number_of(i):
    return (np.asarray(i, np.uint64) * np.uint64(ODD)) & np.uint64(4**SYMBOLS - 1)


def spell(v):
    """The numbers v as texts: their SYMBOLS base-4 digits over ACGT, the highest first -> uint8[n, SYMBOLS]."""
    shifts = np.arange(SYMBOLS - 1, -1, -1, dtype=np.uint64) * np.uint64(2)
    return np.frombuffer(b"ACGT", np.uint8)[((np.asarray(v, np.uint64)[:, None] >> shifts) & np.uint64(3)).astype(np.intp)]


def bodies_of(v):
    """What the encoder writes for spell(v) under table_2bit() (A, C, G, T = 00, 01, 10, 11, the first symbol at the top of the first
    byte): the 20 bits and 4 pad bits -> uint8[n, 3]."""
    w = np.asarray(v, np.uint64) << np.uint64(4)
    return np.stack(((w >> np.uint64(16)) & np.uint64(0xFF), (w >> np.uint64(8)) & np.uint64(0xFF), w & np.uint64(0xFF)), axis=1).astype(np.uint8)


def as_texts(letters):
    """uint8[n, SYMBOLS] -> n bytes objects."""
    return np.ascontiguousarray(letters).view("S%d" % SYMBOLS).ravel().tolist()


@functools.lru_cache(maxsize=None)
def key_fixture():
    """N_KEYS keys under table_2bit(), made with numpy.  Key i < KEY_TRIP spells number_of(i): all different, all of 3 body bytes.  The
    300 keys of the second trip, at shuffled places: 100 copies of first-trip keys (.dup: (place, the first-trip key)), 100 texts no
    first-trip key holds (.own) and a second copy of one of them (.again: its two places), fillers of that kind, and five texts of other
    sizes (.special): the wavefront's record of tests/test_gpu_select.py (159 bytes: the largest body), the empty text (no bytes: the
    smallest), GC and A (a byte) and GATTA (two); the last key, KEY_BAD, ends in front of where it begins.
    -> .st the store, .texts key k's text (None: KEY_BAD), .first {text: its lowest key number}."""
    rng = np.random.default_rng(0x57D1DE01)
    tab = table_2bit()
    special = {"long": select_store()[1][16][2], "empty": b"", "needle": WRAP_NEEDLE, "one": b"A", "five": b"GATTA"}
    places = KEY_TRIP + rng.permutation(299)
    places[[150, 200]] = np.sort(places[[150, 200]])  # (the text that is there twice: .own names its first place)
    src = np.sort(rng.choice(KEY_TRIP, size=100, replace=False))
    f = SimpleNamespace(dup=list(zip(places[:100].tolist(), src.tolist())), own=places[100:200].tolist(), again=(int(places[150]), int(places[200])),
                        special=dict(zip(special, places[201:206].tolist())), filler=places[206:].tolist())
    origin = np.arange(N_KEYS)  # key k spells number_of(origin[k])
    origin[places[:100]] = src
    origin[places[200]] = places[150]
    v = number_of(origin)
    numbered = np.ones(N_KEYS, bool)
    numbered[list(f.special.values()) + [KEY_BAD]] = False
    packed = {name: np.frombuffer(bytes(_pack(tab, t)), np.uint8) for name, t in special.items()}
    sizes, lengths = np.where(numbered, 3, 0).astype(np.uint64), np.where(numbered, SYMBOLS, 0).astype(np.uint64)
    for name, k in f.special.items():
        sizes[k], lengths[k] = packed[name].size, len(special[name])
    lengths[KEY_BAD] = 1
    body_index = _index_of(sizes)
    blob = np.zeros(int(body_index[-1]), np.uint8)
    blob[body_index[:-1][numbered].astype(np.intp)[:, None] + np.arange(3)] = bodies_of(v[numbered])
    for name, k in f.special.items():
        blob[int(body_index[k]) : int(body_index[k + 1])] = packed[name]
    body_index[N_KEYS] -= np.uint64(1)  # KEY_BAD ends in front of where it begins
    f.st = SimpleNamespace(tab=tab, cb=_store(tab, [b"A"]).cb, n=N_KEYS, bodies=blob, body_index=body_index, text_index=_index_of(lengths))
    f.texts = as_texts(spell(v))
    for name, k in f.special.items():
        f.texts[k] = special[name]
    f.texts[KEY_BAD] = None
    f.first = {}
    for k, t in enumerate(f.texts):
        if t is not None:
            f.first.setdefault(t, k)
    return f


def check_key_reach(f):
    """The key set is past one grid of tiles, and everything the second trip is there for lies in it."""
    sizes = np.diff(f.st.body_index[:N_KEYS]).astype(np.int64)  # (of the keys in front of KEY_BAD)
    assert f.st.n == N_KEYS > KEY_TRIP == JOIN_GRID * TILE and len(f.first) == KEY_TRIP + 100 + len(f.filler) + len(f.special)
    assert bool((sizes[:KEY_TRIP] == 3).all()) and len(set(f.texts[:KEY_TRIP])) == KEY_TRIP  # the first trip: 3 bytes each, no text twice
    assert all(src < KEY_TRIP <= k and f.texts[k] == f.texts[src] and f.first[f.texts[k]] == src for k, src in f.dup) and len(f.dup) == 100
    assert all(k >= KEY_TRIP and f.first[f.texts[k]] == k for k in f.own) and len(f.own) == 100
    assert KEY_TRIP <= min(f.again) and f.texts[f.again[0]] == f.texts[f.again[1]] and f.first[f.texts[f.again[0]]] == min(f.again) != max(f.again)
    assert all(k >= KEY_TRIP and f.first[f.texts[k]] == k for k in f.special.values())
    assert int(sizes[f.special["long"]]) == int(sizes.max()) > LANE_BYTES and int(sizes[f.special["empty"]]) == int(sizes.min()) == 0 == len(f.texts[f.special["empty"]])
    assert sorted(int(sizes[f.special[name]]) for name in ("needle", "one", "five")) == [1, 1, 2]  # sizes the first trip does not have
    assert KEY_BAD >= KEY_TRIP and f.st.body_index[KEY_BAD + 1] < f.st.body_index[KEY_BAD]
    assert {k // TILE for k in f.special.values()} | {KEY_BAD // TILE} == {JOIN_GRID, JOIN_GRID + 1}  # both workgroups that come back hold some


@functools.lru_cache(maxsize=None)
def record_fixture():
    """About 3 000 records, shuffled, encoded one by one by the oracle: texts of first-trip keys, of second-trip keys of every kind,
    and texts that are no key -- numbers no key spells, a key's text with another last symbol, a long record that differs from the long
    key in its last symbol, texts of the special keys' sizes -> (store, key_of: the lowest key number of record b's text, or JOIN_NONE)."""
    f = key_fixture()
    rng = np.random.default_rng(0x57D1DE02)
    texts = [f.texts[int(i)] for i in rng.integers(0, KEY_TRIP, size=1500)]
    texts += [f.texts[k] for k in f.own] * 3 + [f.texts[k] for k, _ in f.dup] * 3 + [f.texts[f.again[1]]] * 5 + [f.texts[k] for k in f.special.values()] * 3
    strangers = as_texts(spell(number_of(STRANGERS + np.arange(800))))
    long_text = f.texts[f.special["long"]]
    stem, near = next((t, t[:-1] + s) for t in (f.texts[src] for _, src in f.dup) for s in (b"A", b"C", b"G", b"T") if t[:-1] + s not in f.first)
    strangers += [near, long_text[:-1] + (b"C" if long_text[-1:] != b"C" else b"G"), b"GATTC", b"C", b"G" * (SYMBOLS + 1), b"T" * (SYMBOLS - 1)]
    texts += strangers
    texts = [texts[int(i)] for i in rng.permutation(len(texts))]
    key_of = np.array([f.first.get(t, JOIN_NONE) for t in texts], np.uint32)
    assert not any(t in f.first for t in strangers) and stem in f.first and near[:-1] == stem[:-1] and near[-1:] != stem[-1:]
    return _store(f.st.tab, texts), key_of, texts


@functools.lru_cache(maxsize=None)
def device_keys():
    return upload(key_fixture().st)


def check_join_run(r, n, want, key_of, count_only, failed):
    """One run against the dict's answer: every field of the result, both status arrays, the rows and their key numbers."""
    n_failed, first_failed, first_status = failed
    assert (r.res.status, r.res.n_match, r.res.n_failed, r.res.first_failed, r.res.first_status) == (OK, want.size, n_failed, first_failed, first_status), r.res
    assert (r.res.n_keys_failed, r.res.first_key_failed, r.res.first_key_status) == (1, KEY_BAD, ARG), r.res
    assert r.status.size == n and np.flatnonzero(r.status).tolist() == ([first_failed] if n_failed else [])
    assert r.key_status.size == N_KEYS and np.flatnonzero(r.key_status).tolist() == [KEY_BAD] and int(r.key_status[KEY_BAD]) == ARG
    check_rows(r.rows, want, count_only)
    if r.key_rows:
        check_rows(r.keys, key_of[want], False)
    else:
        assert bool((r.keys == ROW_SENTINEL).all())


@pytest.mark.parametrize("count_only", [False, True], ids=["rows", "count_only"])
def test_join_against_a_key_set_past_one_grid_of_key_tiles(ctx, count_only):
    """Both modes, three times each with identical arrays: the build races by design, the answer must not."""
    f = key_fixture()
    check_key_reach(f)
    st, key_of, texts = record_fixture()
    found = set(key_of.tolist())
    assert {src for _, src in f.dup} | set(f.own) | {min(f.again)} | set(f.special.values()) | {JOIN_NONE} <= found and not {k for k, _ in f.dup} & found and max(f.again) not in found
    assert int((key_of < KEY_TRIP).sum()) > 1000 and int((key_of == JOIN_NONE).sum()) > 800 and st.n > 8 * TILE
    dev = upload(st)
    for mode in (0, NOT):
        want = np.flatnonzero((key_of != JOIN_NONE) != bool(mode))
        runs = [run_join(ctx, st.cb, dev, st.n, device_keys(), N_KEYS, mode, want.size, count_only=count_only) for _ in range(3)]
        for r in runs:
            check_join_run(r, st.n, want, key_of, count_only, (0, 0, 0))
            assert r.res == runs[0].res and np.array_equal(r.rows, runs[0].rows) and np.array_equal(r.keys, runs[0].keys)


def test_join_with_records_and_keys_both_past_one_grid_of_tiles(ctx):
    """tests/test_gpu_select.py's store, which wraps the flag kernel's grid, against the key set that wraps the build's."""
    f = key_fixture()
    rec, classes, cls = select_store()
    key_of_class = np.array([JOIN_NONE if status or raw_class(c) else f.first.get(text, JOIN_NONE) for c, (status, length, text) in enumerate(classes)], np.uint32)
    assert sorted(set(key_of_class.tolist())) == sorted(f.special[name] for name in ("needle", "one", "long")) + [JOIN_NONE]
    assert N_WRAPPED > JOIN_GRID * TILE < REC_LONG and N_KEYS > KEY_TRIP <= min(f.special.values())
    key_of = key_of_class[cls]
    for mode, count_only in ((0, False), (NOT, False), (0, True)):
        want = np.flatnonzero((cls != 17) & ((key_of != JOIN_NONE) != bool(mode)))  # (class 17 is the record that fails)
        assert 0 < want.size < N_WRAPPED and (REC_LONG in want) == (mode == 0) and int(want[-1]) >= JOIN_GRID * TILE
        r = run_join(ctx, rec.cb, device_store(), N_WRAPPED, device_keys(), N_KEYS, mode, want.size, count_only=count_only)
        check_join_run(r, N_WRAPPED, want, key_of, count_only, (1, REC_BAD, ARG))


def test_device_hash_past_one_grid_of_tiles(ctx):
    """k_join_hash's second trip: every key of it, and a sample of the first, against et_join_hash on the host."""
    f = key_fixture()
    st = f.st
    got = device_hashes(ctx, st)
    sample = np.concatenate((np.random.default_rng(0x57D1DE03).integers(0, KEY_TRIP, size=200), np.arange(KEY_TRIP, N_KEYS)))
    assert st.n > JOIN_GRID * TILE and int((sample >= KEY_TRIP).sum()) == 300
    lengths = np.diff(st.text_index)
    for k in sample.tolist():
        want = 0xFFFFFFFFFFFFFFFF if k == KEY_BAD else host_hash(st.bodies[int(st.body_index[k]) : int(st.body_index[k + 1])], int(lengths[k]))
        assert got[k] == want, k


# --- 2. take and gather ----------------------------------------------------------------------------------------------------------------
CYCLE = np.array([5, 0, 1, 7, 2, 8, 3, 6, 4])  # records of a store of eight, and a row number beyond it
TAKE_SIZES = [0, 1, 7, 16, 33, 560, 0, 0]  # body bytes of the take's records; the long one carries the output past TAKE_GRID tiles
TAKE_LENGTHS = [0, 1, 14, 30, 70, 1000, 0, 9]  # (record 7 is kept raw elsewhere: no bytes under a length)
GATHER_LENGTHS = [0, 1, 7, 16, 33, 300, 0, 2]  # symbols of the gather's records
TINY = np.array([0, 1, 2, 3, 1, 0, 5, 1, 2])  # the second take's cycle: bodies of a byte and of none, and a row number beyond the store
TINY_SIZES, TINY_LENGTHS = [1, 0, 1, 0, (64 << 10) + 3], [2, 0, 1, 9, 64 << 10]  # record 4 is the padding: 64 KiB + 3 bytes
PAD_ROWS, TAIL_ROWS = 130, 40  # rows of the padding in front of and behind the tiny rows; tiny rows behind the last padding


def cycled(cycle, n):
    return np.tile(cycle, n // cycle.size + 1)[:n]


def joined(parts):
    """The wants of several stretches of rows, one behind the other."""
    nb, ln = (np.concatenate([np.diff(getattr(p, name)) for p in parts]) for name in ("body_index", "text_index"))
    out = SimpleNamespace(status=np.concatenate([p.status for p in parts]), body_index=_index_of(nb), text_index=_index_of(ln), data=np.concatenate([p.data for p in parts]))
    out.total, out.text_total = int(out.body_index[-1]), int(out.text_index[-1])
    assert out.total == out.data.size
    return out


def check_failures_in_both_trips(rows, beyond, status, res):
    """The rows that fail are those the test placed: the first of them in the first trip, one at least in the second; the result counts
    both trips and still names the first."""
    failed = np.flatnonzero(rows == beyond)
    assert rows.size == N_ROWS > ROW_TRIP == PLAN_GRID * LANES and np.array_equal(np.flatnonzero(status), failed)
    assert failed[0] < ROW_TRIP <= failed[-1] and int((failed >= ROW_TRIP).sum()) >= 4
    assert (res.n_failed, res.first_failed, res.first_status) == (failed.size, int(failed[0]), ARG), res


def tiles_of_output(body_index, total, skew):
    """k_take_copy's cut of an output that begins `skew` bytes behind a multiple of C -> (tiles, workgroups, tiles per workgroup, entries of
    out_body_index per tile: those of the rows that own the tile's first and last byte and all between, and one)."""
    n_tiles = (skew + total + C - 1) // C
    grid = min(total // C + 2, TAKE_GRID)  # (the test's capacity is the need)
    t = np.arange(n_tiles, dtype=np.int64)
    o0, o1 = np.maximum(t * C - skew, 0), np.minimum((t + 1) * C - skew, total)
    index = body_index.astype(np.int64)
    row_lo, row_end = np.searchsorted(index, o0, side="right") - 1, np.searchsorted(index, o1 - 1, side="right")
    return n_tiles, grid, -(-n_tiles // grid), row_end - row_lo + 1


@functools.lru_cache(maxsize=None)
def take_fixture(which):
    """-> (store, rows, the want, the row number beyond the store).  "mixed": N_ROWS rows cycling over CYCLE.  "tiny": rows of a byte and of
    none -- thousands to a copy tile -- between two stretches of the 64 KiB padding, and TAIL_ROWS more behind it."""
    if which == "mixed":
        st = raw_store(TAKE_SIZES, lengths=TAKE_LENGTHS, seed=0x57D1DE10)
        return st, cycled(CYCLE, N_ROWS), tiled(model(st, CYCLE), N_ROWS), 8
    st = raw_store(TINY_SIZES, lengths=TINY_LENGTHS, seed=0x57D1DE11)
    n_tiny = N_ROWS - 2 * PAD_ROWS - TAIL_ROWS
    pad, tiny = model(st, [4]), model(st, TINY)
    rows = np.concatenate((np.full(PAD_ROWS, 4), cycled(TINY, n_tiny), np.full(PAD_ROWS, 4), cycled(TINY, TAIL_ROWS)))
    return st, rows, joined([tiled(pad, PAD_ROWS), tiled(tiny, n_tiny), tiled(pad, PAD_ROWS), tiled(tiny, TAIL_ROWS)]), 5


@pytest.mark.parametrize("tile_off", [0, 5])
@pytest.mark.parametrize("which", ["mixed", "tiny"])
def test_take_past_one_plan_grid_with_several_copy_tiles_per_workgroup(ctx, which, tile_off):
    st, rows, want, beyond = take_fixture(which)
    assert rows.size == N_ROWS == want.status.size and want.total > TAKE_GRID * C  # more tiles than workgroups ...
    n_tiles, grid, per, entries = tiles_of_output(want.body_index, want.total, tile_off)
    assert grid == TAKE_GRID and per >= 2 and n_tiles > TAKE_GRID  # ... so a workgroup copies a run of them, carrying `hint`
    in_place = np.flatnonzero(entries > STAGE_ROWS)
    if which == "mixed":
        assert N_ROWS / n_tiles < STAGE_ROWS and in_place.size == 0 and int(entries[:-1].min()) > 8  # every tile staged, and none inside one row
    else:
        assert int(entries.max()) > 4 * STAGE_ROWS and bool((in_place % per != 0).any()) and bool((in_place % per == 0).any())  # read in place, in a workgroup's first tile and in a later one
    r = check_take(run_take(ctx, st, upload(st), rows, want.total, tile_off=tile_off), want)
    assert r.d_out.data_ptr() % C == tile_off
    check_failures_in_both_trips(rows, beyond, r.status, r.res)
    if tile_off == 0:
        s = check_take(run_take(ctx, st, upload(st), rows, want.total, sizes_only=True), want)
        assert s.res == r.res


@functools.lru_cache(maxsize=None)
def gather_fixture():
    """Eight records of text under the table of their own bytes, the oracle's encodes -> (store, rows, per row (status, room, text))."""
    pool = corpus.text_like(sum(GATHER_LENGTHS), 0x57D1DE20)
    cuts = _index_of(GATHER_LENGTHS)
    st = make_store(oracle_table(pool), [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(len(GATHER_LENGTHS))])
    cycle_wants = want_rows(st, CYCLE)
    assert [s for s, _, _ in cycle_wants] == [ARG if r == 8 else OK for r in CYCLE] and [len(t) for _, _, t in cycle_wants] == [0 if r == 8 else GATHER_LENGTHS[r] for r in CYCLE]
    return st, cycled(CYCLE, N_ROWS), (cycle_wants * (N_ROWS // CYCLE.size + 1))[:N_ROWS]


def test_gather_past_one_plan_grid(ctx):
    st, rows, wants = gather_fixture()
    need = sum(room for _, room, _ in wants)
    dev = upload(st)
    r = check_gather(run_gather(ctx, st, dev, rows, need), wants)
    check_failures_in_both_trips(rows, 8, r.status, r.res)
    s = check_gather(run_gather(ctx, st, dev, rows, need, sizes_only=True), wants)
    assert (s.res.out_bytes, s.res.n_failed, s.res.first_failed, s.res.first_status) == (r.res.out_bytes, r.res.n_failed, r.res.first_failed, r.res.first_status)


# --- 3. the number call ----------------------------------------------------------------------------------------------------------------
DEEP = 1500  # symbols in front of the number of the record a workgroup reads
BIG = 1 << 62  # the number there: the heavy group's sum wraps
NUMBER_ROWS, NUMBER_FIRST = np.arange(7), np.array([2, 2, DEEP + 1, 2, 2, 2, 2])  # the cycle: six records and a row number beyond them; where each ask begins
HEAVY = 7  # the group of every even row


@functools.lru_cache(maxsize=None)
def number_store():
    filler = corpus.text_like(DEEP + 40, 0x57D1DE30).tobytes().replace(b";", b",").replace(b"=", b"-")
    texts = [b"v=12345;ok", b"v=-987;", filler[:DEEP] + b"=%d;x9" % BIG + filler[DEEP:], b"v=;", b"v=12x;", b"v=99999999999999999999;"]
    return make_store(oracle_table(np.frombuffer(b"".join(texts) + b" a+-0123456789", np.uint8)), texts)


def group_numbers():
    """Every even row in HEAVY; of the odd rows every fourth in no group, the others alone in the group of their own number."""
    k = np.arange(N_ROWS)
    return np.where(k % 2 == 0, HEAVY, np.where(k % 8 == 3, GROUP_NONE, k)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def number_fixture(grouped):
    """-> (rows, first, group_of, the want): want_number() answers for the cycle, numpy spreads it and folds the aggregates; the sums are
    taken modulo 2^64, the heavy group's (the whole column's) with Python's integers as well."""
    st = number_store()
    one = want_number(st, NUMBER_ROWS, NUMBER_FIRST, TO_END, b";")
    assert one.status.tolist() == [OK] * 6 + [ARG] and one.kind.tolist() == [N_OK, N_OK, N_OK, N_EMPTY, N_BAD, N_RANGE, N_EMPTY] and one.values.tolist() == [12345, -987, BIG, 0, 0, 0, 0]
    spread = lambda a: cycled(np.asarray(a), N_ROWS)  # noqa: E731
    group_of, n_groups = (group_numbers(), N_GROUPS) if grouped else (None, 1)
    w = SimpleNamespace(status=spread(one.status), kind=spread(one.kind), values=spread(one.values), texts=(one.texts * (N_ROWS // 7 + 1))[:N_ROWS])
    valid = w.status == OK
    w.counts = {"n_ok": int((valid & (w.kind == N_OK)).sum()), "n_empty": int((valid & (w.kind == N_EMPTY)).sum()), "n_bad": int((w.kind == N_BAD).sum()),
                "n_range": int((w.kind == N_RANGE).sum()), "n_failed": int((~valid).sum())}
    w.first = (int(np.flatnonzero(~valid)[0]), ARG)
    g = group_of.astype(np.int64) if grouped else np.zeros(N_ROWS, np.int64)
    folded = valid & (w.kind == N_OK) & (g != GROUP_NONE)
    gf, vf = g[folded], w.values[folded]
    total, w.min, w.max = np.zeros(n_groups, np.uint64), np.full(n_groups, I64_MAX, np.int64), np.full(n_groups, I64_MIN, np.int64)
    np.add.at(total, gf, vf.astype(np.uint64))  # (modulo 2^64)
    np.minimum.at(w.min, gf, vf)
    np.maximum.at(w.max, gf, vf)
    w.sum, w.n = total.view(np.int64), np.bincount(gf, minlength=n_groups)
    heavy = HEAVY if grouped else 0
    true_sum = sum(int(x) for x in vf[gf == heavy])
    assert true_sum > I64_MAX and int(w.sum[heavy]) == wrap64(true_sum) != true_sum  # the sum wraps
    return cycled(NUMBER_ROWS, N_ROWS), cycled(NUMBER_FIRST, N_ROWS), group_of, w


def check_number_reach(rows, first, group_of, w):
    st = number_store()
    assert rows.size == N_ROWS > ROW_TRIP == PLAN_GRID * LANES
    assert reach(st, 2, DEEP + 1, TO_END) > number_lane_bytes() and all(reach(st, r, 2, TO_END) <= number_lane_bytes() for r in (0, 1, 3, 4, 5))
    assert int((rows == 2).sum()) > LONG_GRID  # more listed rows than k_number_long has workgroups
    failed = np.flatnonzero(w.status)
    assert failed[0] < ROW_TRIP <= failed[-1] and np.array_equal(failed, np.flatnonzero(rows == 6))
    assert {N_OK, N_EMPTY, N_BAD, N_RANGE} <= set(w.kind[ROW_TRIP:].tolist())  # the second trip tallies every kind
    if group_of is None:
        return
    assert N_GROUPS > ROW_TRIP and w.n[HEAVY] > N_ROWS // 6 and int((group_of == GROUP_NONE).sum()) > N_ROWS // 10
    far = np.arange(ROW_TRIP, N_GROUPS)
    reached = far[w.n[far] > 0]
    assert reached.size and bool((np.flatnonzero(np.isin(group_of, reached)) >= ROW_TRIP).all())  # groups of the second trip, reached by rows of the second trip alone
    unused = far[~np.isin(far, group_of)]
    assert unused.size and bool((w.sum[unused] == 0).all() and (w.n[unused] == 0).all() and (w.min[unused] == I64_MAX).all() and (w.max[unused] == I64_MIN).all())


@pytest.mark.parametrize("outputs", [("values", "kind", "sum", "n", "min", "max", "status"), ("sum",), ("n",), ("min",), ("max",), ()], ids=["all", "sum", "n", "min", "max", "count_only"])
def test_number_past_one_grid_of_rows_and_of_groups(ctx, outputs):
    rows, first, group_of, w = number_fixture(True)
    check_number_reach(rows, first, group_of, w)
    st = number_store()
    groups = dict(group_of=group_of, n_groups=N_GROUPS) if outputs else {}  # (group numbers without an aggregate output are an argument error)
    check_number(run_number(ctx, st, upload(st), rows, first, TO_END, stop=b";", outputs=outputs, **groups), w)


def test_number_whole_column_past_one_grid_of_rows(ctx):
    rows, first, group_of, w = number_fixture(False)
    check_number_reach(rows, first, group_of, w)
    st = number_store()
    r = check_number(run_number(ctx, st, upload(st), rows, first, TO_END, stop=b";", n_groups=1), w)
    assert r.res.n_ok == int(w.n[0]) > N_ROWS // 3
