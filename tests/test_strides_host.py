"""The fixtures of tests/test_gpu_strides.py as far as they can be checked without a GPU: the numpy builder of the half million numbered
keys against the oracle's encode (_pack) and the library's hash (et_join_hash against tests/hashcraft.py's restatement), the key set's
dict against a plain loop over a sample, that every special key lies in the build's second trip, and that the take's, the gather's and
the number call's rows cross the caps the GPU tests name -- with the wants that numpy spreads compared, on a short stretch, with the
references run row by row."""
import numpy as np

from tests import hashcraft
from tests.test_gpu_join import NONE as JOIN_NONE, host_hash
from tests.test_gpu_match import _pack
from tests.test_gpu_strides import C, CYCLE, GROUP_NONE, KEY_BAD, KEY_TRIP, N_KEYS, N_ROWS, ROW_TRIP, STAGE_ROWS, STRANGERS, SYMBOLS, TAKE_GRID, TINY, TO_END, as_texts, bodies_of, \
    check_key_reach, check_number_reach, cycled, gather_fixture, joined, key_fixture, number_fixture, number_of, number_store, record_fixture, spell, take_fixture, tiled, tiles_of_output
from tests.test_gpu_number import want_number
from tests.test_gpu_take import model
from tests.test_shared_host import table_2bit


def test_the_numbered_keys_are_the_oracles_encodes_and_all_different():
    tab = table_2bit()
    every = number_of(np.arange(4**SYMBOLS))
    assert np.unique(every).size == 4**SYMBOLS  # one-to-one: numbers of different origins are different texts
    sample = np.concatenate(([0, 1, 4**SYMBOLS - 1], np.random.default_rng(0x57D1DE40).integers(0, 4**SYMBOLS, size=50)))
    for v, text, body in zip(sample.tolist(), as_texts(spell(sample)), bodies_of(sample)):
        assert len(text) == SYMBOLS and int(text.translate(bytes.maketrans(b"ACGT", b"0123")), 4) == v
        assert bytes(_pack(tab, text)) == body.tobytes()


def test_the_key_store_holds_what_its_texts_say_and_hashes_as_the_library_does():
    f = key_fixture()
    check_key_reach(f)
    st, tab = f.st, table_2bit()
    sample = np.concatenate((np.random.default_rng(0x57D1DE41).integers(0, KEY_TRIP, size=50), np.arange(KEY_TRIP, KEY_BAD)))
    lengths = np.diff(st.text_index)
    for k in sample.tolist():
        body = st.bodies[int(st.body_index[k]) : int(st.body_index[k + 1])].tobytes()
        assert body == bytes(_pack(tab, f.texts[k])) and int(lengths[k]) == len(f.texts[k]), k
        assert host_hash(body, len(f.texts[k])) == hashcraft.hash_of(body, len(f.texts[k])), k
    assert int(lengths[KEY_BAD]) == 1 and f.texts[KEY_BAD] is None and st.n == N_KEYS
    lowest = {}
    for k in range(KEY_BAD - 1, -1, -1):  # the dict against a loop from the other end: the last one written is the lowest
        lowest[f.texts[k]] = k
    assert lowest == f.first and all(f.first[f.texts[k]] == src < KEY_TRIP for k, src in f.dup)


def test_the_records_reach_every_kind_of_key_and_texts_that_are_none():
    f = key_fixture()
    st, key_of, texts = record_fixture()
    assert st.n == len(texts) == key_of.size and [f.texts[k] if k != JOIN_NONE else None for k in key_of[:200].tolist()] == [t if t in f.first else None for t in texts[:200]]
    found = set(key_of.tolist())
    assert set(f.own) | {src for _, src in f.dup} | set(f.special.values()) | {JOIN_NONE} <= found and not any(k in found for k, _ in f.dup)
    strangers = set(as_texts(spell(number_of(STRANGERS + np.arange(800)))))
    assert len(strangers) == 800 and not strangers & set(f.first) and strangers <= set(texts)


def test_the_takes_rows_cross_the_plan_grid_and_its_output_the_copy_grid():
    for which, beyond in (("mixed", 8), ("tiny", 5)):
        st, rows, want, b = take_fixture(which)
        assert b == beyond == st.n and rows.size == N_ROWS > ROW_TRIP and want.total > TAKE_GRID * C
        failed = np.flatnonzero(rows == beyond)
        assert failed[0] < ROW_TRIP <= failed[-1] and np.array_equal(np.flatnonzero(want.status), failed)
        for stretch in (slice(0, 700), slice(N_ROWS - 700, N_ROWS)):  # what numpy spread against model() run row by row
            direct = model(st, rows[stretch])
            k0, k1, _ = stretch.indices(N_ROWS)
            o0, o1 = int(want.body_index[k0]), int(want.body_index[k1])
            assert np.array_equal(direct.status, want.status[stretch]) and np.array_equal(direct.body_index, want.body_index[k0 : k1 + 1] - want.body_index[k0])
            assert np.array_equal(direct.text_index, want.text_index[k0 : k1 + 1] - want.text_index[k0]) and np.array_equal(direct.data, want.data[o0:o1])
        for skew in (0, 5):
            n_tiles, grid, per, entries = tiles_of_output(want.body_index, want.total, skew)
            assert per >= 2 and grid == TAKE_GRID and bool((entries > STAGE_ROWS).any()) == (which == "tiny")
    assert set(CYCLE.tolist()) == set(range(9)) and 5 in TINY


def test_joined_and_tiled_agree_with_model_on_a_short_mixture():
    st, _, _, _ = take_fixture("tiny")
    rows = np.concatenate((np.full(3, 4), cycled(TINY, 31), np.full(2, 4), cycled(TINY, 11)))
    got = joined([tiled(model(st, [4]), 3), tiled(model(st, TINY), 31), tiled(model(st, [4]), 2), tiled(model(st, TINY), 11)])
    want = model(st, rows)
    assert all(np.array_equal(getattr(got, name), getattr(want, name)) for name in ("status", "body_index", "text_index", "data")) and got.total == want.total


def test_the_gathers_rows_cross_the_plan_grid():
    st, rows, wants = gather_fixture()
    assert rows.size == len(wants) == N_ROWS > ROW_TRIP and st.n == 8
    failed = [k for k, (s, _, _) in enumerate(wants) if s]
    assert failed == np.flatnonzero(rows == 8).tolist() and failed[0] < ROW_TRIP <= failed[-1]


def test_the_number_calls_rows_and_groups_cross_their_grids():
    st = number_store()
    for grouped in (True, False):
        rows, first, group_of, w = number_fixture(grouped)
        check_number_reach(rows, first, group_of, w)
        tail = slice(N_ROWS - 300, N_ROWS)  # what numpy spread and folded against want_number() run row by row
        direct = want_number(st, rows[tail], first[tail], TO_END, b";")
        assert np.array_equal(direct.status, w.status[tail]) and np.array_equal(direct.kind, w.kind[tail]) and np.array_equal(direct.values, w.values[tail])
    rows, first, group_of, w = number_fixture(True)
    few = np.flatnonzero(group_of != 7)[-200:]  # rows of small groups and of none, the second trip's among them
    direct = want_number(st, rows[few], first[few], TO_END, b";", group_of=group_of[few], n_groups=int(group_of[group_of != GROUP_NONE].max()) + 1)
    for g in set(group_of[few].tolist()) - {GROUP_NONE}:
        assert (direct.sum[g], direct.n[g], direct.min[g], direct.max[g]) == (int(w.sum[g]), int(w.n[g]), int(w.min[g]), int(w.max[g])), g
