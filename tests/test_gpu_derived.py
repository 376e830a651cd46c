"""GPU: what the slice, the field, the concat and the recode share -- the plan frame and the long-row frame of csrc/et_batch.hip --
past one grid: more rows than the plan kernel's capped grid covers in one trip (row PLAN_GRID * LANES onward is reached by the
frame's stride alone) and more listed rows than the long kernel's capped grid has workgroups (listed row LONG_GRID onward likewise).
The rows cycle over a handful of records, so what one cycle gives is computed once by each family's own reference (want_slice,
want_field, want_concat, want_recode: the oracle's texts, Python's answer, the oracle's encode) and tiled; every output is compared
exactly, with d_out and sizes-only."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_gpu_concat import lane_bytes as concat_lane_bytes, run_concat, want_concat
from tests.test_gpu_field import check_field, lane_bytes as field_lane_bytes, run_field, want_field
from tests.test_gpu_gather import make_store, upload
from tests.test_gpu_packed import _index_of
from tests.test_gpu_recode import UPPER, lane_bytes as recode_lane_bytes, main_tables, run_recode, want_recode
from tests.test_gpu_shared import want_encode
from tests.test_gpu_slice import lane_bytes as slice_lane_bytes, main_fixture, run_slice, want_slice
from tests.test_gpu_take import check_take

pytestmark = pytest.mark.gpu

PLAN_GRID, LANES, LONG_GRID = 1024, 256, 1024  # csrc/et_batch.h GATHER_PLAN_GRID, csrc/et_batch.hip BB, csrc/et_batch.h SHARED_DEC_GRID
N_ROWS = PLAN_GRID * LANES + 65  # a second trip of 65 rows: one whole wavefront and one row of the next
TAKE_GRID, TAKE_TILE_BYTES = 2048, 8192  # csrc/et_batch.h: workgroups of k_take_copy<BITS> and k_concat_copy at most, bytes of output per tile
SPACE = ord(" ")


@functools.lru_cache(maxsize=None)
def cycle_fixture():
    """Under the main fixture's table -> (store, the cycle): 0 a text its lane walks, 1 one whose body exceeds every family's
    lane_bytes(), 2 the empty record, 3 kept raw (no bytes, length 9); the cycle is those four and a row number beyond the store."""
    st, texts = main_fixture()
    keep = [texts[5], texts[10], b"", b"nine char"]
    bodies = [want_encode(st.tab, t)[1] for t in keep]
    bodies[3] = b""
    assert 0 < len(bodies[0]) <= min(slice_lane_bytes(), field_lane_bytes(), concat_lane_bytes(), recode_lane_bytes())
    assert len(bodies[1]) > max(slice_lane_bytes(), field_lane_bytes(), concat_lane_bytes(), recode_lane_bytes()) and 4 * len(keep[1]) + 8 >= len(bodies[1])
    assert keep[1].count(b" ") > 40
    return make_store(st.tab, keep, bodies), np.array([0, 1, 2, 3, len(keep)])


def tiled(want, n):
    """What want_*() gave for one cycle of rows, for the first n rows of the cycle repeated."""
    c = want.status.size
    nb, ln = np.diff(want.body_index), np.diff(want.text_index)
    rep = lambda a: np.tile(a, n // c + 1)[:n]  # noqa: E731
    out = SimpleNamespace(status=rep(want.status), body_index=_index_of(rep(nb)), text_index=_index_of(rep(ln)))
    out.data = np.concatenate((np.tile(want.data, n // c), want.data[: int(nb[: n % c].sum())]))
    out.total, out.text_total = int(out.body_index[-1]), int(out.text_index[-1])
    assert out.total == out.data.size
    if hasattr(want, "pos"):
        out.pos = rep(want.pos)
    return out


def calls(st, dev, cycle, rows):
    """-> {family: (what one cycle gives, run(ctx, cap, sizes_only), check)}; the asks reach into record 1's body."""
    TU = main_tables()["TU"]
    field_of = lambda r: np.where(r == 1, 30, 2)  # noqa: E731  (fields 2 .. 4 of the short text, 30 .. 32 of the long one)
    return {
        "slice": (lambda: want_slice(st, cycle, 2, 1000), lambda ctx, cap, so: run_slice(ctx, st, dev, rows, 2, 1000, None, cap, sizes_only=so), check_take),
        "field": (lambda: want_field(st, cycle, field_of(cycle), 3, SPACE), lambda ctx, cap, so: run_field(ctx, st, dev, rows, field_of(rows), 3, SPACE, cap, sizes_only=so),
                  check_field),
        "concat": (lambda: want_concat(st, st, cycle, cycle, b", "), lambda ctx, cap, so: run_concat(ctx, st, st, rows, rows, b", ", cap, dev_a=dev, dev_b=dev, sizes_only=so),
                   check_take),
        "recode": (lambda: want_recode(st, TU, cycle, UPPER), lambda ctx, cap, so: run_recode(ctx, st, TU, dev, rows, UPPER, cap, sizes_only=so), check_take),
    }


@pytest.mark.parametrize("family", ["slice", "field", "concat", "recode"])
def test_rows_past_one_plan_grid_and_listed_rows_past_one_long_grid(ctx, family):
    st, cycle = cycle_fixture()
    rows = np.tile(cycle, N_ROWS // cycle.size + 1)[:N_ROWS]
    assert rows.size > PLAN_GRID * LANES and int((rows == 1).sum()) > LONG_GRID
    one, run, check = calls(st, upload(st), cycle, rows)[family]
    cycle_want = one()
    assert cycle_want.status.tolist() == [0, 0, 0, 0, 6] and int(np.diff(cycle_want.text_index)[1]) > 0  # (the long row gives something; ET_ERR_ARG beyond the store)
    want = tiled(cycle_want, N_ROWS)
    # What the copy behind the plan reaches here: more tiles of output than it has workgroups, so that a workgroup copies a run of them
    # (`per` >= 2, `hint` and the staged index carried from tile to tile) -- but for the field, whose rows are a few bytes each and
    # whose output stays within one tile per workgroup (k_take_copy<true> past its grid is the slice's case; tests/test_gpu_strides.py has <false>).
    assert (want.total > TAKE_GRID * TAKE_TILE_BYTES) == (family != "field")
    for sizes_only in (False, True):
        r = check(run(ctx, want.total, sizes_only), want)
        assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (int((rows == cycle[-1]).sum()), 4, 6)
