"""GPU: what the match, the search, the join and the group call share -- the tiles of their flag kernels in csrc/et_batch.hip -- past one
grid: a store of more tiles than the capped grid has workgroups, so a workgroup's second trip through its tile loop, the second set of
its tile counts, a failure tallied in that trip and a long record listed from it are all reached.  (The order modes have
tests/test_gpu_order.py::test_a_store_that_wraps_the_tile_grid.)  The store is the order test's wrap_store() with three records
behind it, all in the second trip; a record is one of 18 texts, so each family's own Python reference (select, dict membership, order of
first appearance) answers for the 18 and numpy spreads the answers over the half million; every output is compared exactly, with rows
and count-only.  The group case has about 105 000 groups, not a dozen: a record kept raw (a fifth of the store) is a group of its own."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_gpu_gather import upload
from tests.test_gpu_group import NONE as GROUP_NONE, run_group
from tests.test_gpu_join import LANE_BYTES, NONE as JOIN_NONE, run_join
from tests.test_gpu_match import EQUAL, NOT, PREFIX, ROW_SENTINEL, TILE, _pack, _store, run_match, select as select_match
from tests.test_gpu_order import GRID, WRAP_N, WRAP_NEEDLE, WRAP_RAW, WRAP_TEXTS, wrap_store
from tests.test_gpu_packed import _index_of
from tests.test_gpu_search import CONTAINS, SUFFIX, lane_bytes as search_lane_bytes, run_search, select as select_search
from tests.test_shared_host import table_2bit

pytestmark = pytest.mark.gpu

OK, ARG = 0, 6  # et_status
SEARCH_NEEDLE = b"C"
SEARCH_LONG_SPARE = 40  # bytes of body above et_search_lane_bytes() of the record the search lists as long
JOIN_LONG_SYMBOLS = 4 * (LANE_BYTES + 30) + 1  # of the record the join and the group take by wavefront: 159 bytes of body
N = WRAP_N + 3
SEARCH_LONG, JOIN_LONG, BAD = WRAP_N, WRAP_N + 1, WRAP_N + 2  # the three records behind wrap_store()'s


@functools.lru_cache(maxsize=None)
def select_store():
    """-> (store, classes, cls): wrap_store()'s records, then a run of A that ends in the search's needle, a text of JOIN_LONG_SYMBOLS
    random symbols, and a record whose pair of body offsets decreases.  classes[c] = (status, length, stored text) as the families'
    references take them, cls[b] = the class of record b."""
    tab = table_2bit()
    bodies, body_index, lengths, kind, which = wrap_store()
    long_search = b"A" * (4 * (search_lane_bytes() + SEARCH_LONG_SPARE) - 1) + SEARCH_NEEDLE
    long_join = np.random.default_rng(0x5E1EC700).choice(np.frombuffer(b"ACGT", np.uint8), size=JOIN_LONG_SYMBOLS).tobytes()
    extra = [np.frombuffer(bytes(_pack(tab, t)), np.uint8) for t in (long_search, long_join)]
    assert extra[0].size > search_lane_bytes() and extra[1].size > LANE_BYTES and GRID * TILE < SEARCH_LONG
    st = SimpleNamespace(tab=tab, cb=_store(tab, [b"A"]).cb, n=N, bodies=np.concatenate([bodies] + extra))
    st.body_index = _index_of(np.concatenate((np.diff(body_index), np.array([extra[0].size, extra[1].size, 0], np.uint64))))
    st.body_index[N] -= np.uint64(1)  # record BAD ends in front of where it begins
    st.text_index = _index_of(np.concatenate((lengths, np.array([len(long_search), len(long_join), 1], np.uint64))))
    classes = [(OK, len(t), b"" if k == WRAP_RAW else t) for k, row in enumerate(WRAP_TEXTS) for t in row]
    classes += [(OK, len(long_search), long_search), (OK, len(long_join), long_join), (ARG, 0, b"")]
    cls = np.concatenate((kind * 3 + which, [15, 16, 17]))
    return st, classes, cls


@functools.lru_cache(maxsize=None)
def device_store():
    return upload(select_store()[0])


def raw_class(c):
    return c // 3 == WRAP_RAW


def check_common(r, res_count, want_count):
    st = select_store()[0]
    assert (r.res.status, res_count, r.res.n_failed, r.res.first_failed, r.res.first_status) == (OK, want_count, 1, BAD, ARG), r.res
    assert BAD > GRID * TILE and np.flatnonzero(r.status).tolist() == [BAD] and int(r.status[BAD]) == ARG
    assert r.status.size == st.n


def check_rows(got, want, count_only):
    if count_only:
        assert bool((got == ROW_SENTINEL).all())
    else:
        assert np.array_equal(got[: want.size], want.astype(np.uint32)) and bool((got[want.size :] == ROW_SENTINEL).all())


@pytest.mark.parametrize("count_only", [False, True], ids=["rows", "count_only"])
def test_match_past_one_grid_of_tiles(ctx, count_only):
    st, classes, cls = select_store()
    for mode in (EQUAL, PREFIX | NOT):
        want = np.flatnonzero(np.isin(cls, select_match(classes, WRAP_NEEDLE, mode)))
        assert 0 < want.size < N and int(want[-1]) >= GRID * TILE
        r = run_match(ctx, st.cb, device_store(), N, WRAP_NEEDLE, mode, want.size, count_only=count_only)
        check_common(r, r.res.n_match, want.size)
        check_rows(r.rows, want, count_only)


@pytest.mark.parametrize("count_only", [False, True], ids=["rows", "count_only"])
def test_search_past_one_grid_of_tiles(ctx, count_only):
    st, classes, cls = select_store()
    for mode in (CONTAINS, SUFFIX | NOT):
        sel, pos = select_search(classes, SEARCH_NEEDLE, mode)
        want = np.flatnonzero(np.isin(cls, sel))
        assert 0 < want.size < N and (SEARCH_LONG in want) == (mode == CONTAINS)  # (the long record contains the needle, at its end)
        r = run_search(ctx, st.cb, device_store(), N, SEARCH_NEEDLE, mode, want.size, count_only=count_only)
        check_common(r, r.res.n_match, want.size)
        check_rows(r.rows, want, count_only)
        if r.with_pos:
            pos_of_class = np.zeros(len(classes), np.uint32)
            pos_of_class[sel] = pos
            assert int(pos_of_class[15]) == classes[15][1] - 1
            check_rows(r.pos, pos_of_class[cls[want]], False)
        else:
            assert bool((r.pos == ROW_SENTINEL).all())


@pytest.mark.parametrize("count_only", [False, True], ids=["rows", "count_only"])
def test_join_past_one_grid_of_tiles(ctx, count_only):
    st, classes, cls = select_store()
    keys = [WRAP_NEEDLE, b"A", classes[16][2]]
    ks = _store(st.tab, keys)
    first = {}
    for k, text in enumerate(keys):
        first.setdefault((len(text), text), k)
    key_of_class = np.array([JOIN_NONE if status or raw_class(c) else first.get((length, text), JOIN_NONE) for c, (status, length, text) in enumerate(classes)], np.uint32)
    assert sorted(set(key_of_class.tolist())) == [0, 1, 2, JOIN_NONE]
    want = np.flatnonzero(key_of_class[cls] != JOIN_NONE)
    assert JOIN_LONG in want
    r = run_join(ctx, st.cb, device_store(), N, upload(ks), ks.n, 0, want.size, count_only=count_only)
    check_common(r, r.res.n_match, want.size)
    assert r.res.n_keys_failed == 0 and not r.key_status.any()
    check_rows(r.rows, want, count_only)
    check_rows(r.keys, key_of_class[cls[want]], count_only)


@pytest.mark.parametrize("count_only", [False, True], ids=["rows", "count_only"])
def test_group_past_one_grid_of_tiles(ctx, count_only):
    st, classes, cls = select_store()
    seen = {}
    first_of_class = np.array([int(np.flatnonzero(cls == c)[0]) for c in range(len(classes))])
    for c, (status, length, text) in enumerate(classes):  # the first record of a text: the lowest over the classes that hold it
        if not status and not raw_class(c):
            seen[(length, text)] = min(seen.get((length, text), N), int(first_of_class[c]))
    rep_of_class = np.array([0 if status or raw_class(c) else seen[(length, text)] for c, (status, length, text) in enumerate(classes)])
    rep = np.where(raw_class(cls), np.arange(N), rep_of_class[cls])  # (a record kept raw equals nothing: a group of its own)
    valid = cls != 17
    first = np.unique(rep[valid])  # ascending: the order of first appearance
    group_of = np.where(valid, np.searchsorted(first, rep), GROUP_NONE).astype(np.uint32)
    counts = np.bincount(group_of[valid], minlength=first.size)
    assert len(seen) == 10 and first.size == len(seen) + int(raw_class(cls).sum()) and JOIN_LONG in first
    r = run_group(ctx, st.cb, device_store(), N, first.size, count_only=count_only)
    check_common(r, r.res.n_groups, first.size)
    check_rows(r.first, first, count_only)
    check_rows(r.count, counts, count_only)
    check_rows(r.group_of, group_of, count_only)
