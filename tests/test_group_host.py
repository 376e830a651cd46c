"""et_group_packed_device as far as it can be checked without a GPU: declared, bound, exported, the result struct's size; and, in pure
Python with the oracle, that on the stores of tests/test_gpu_group.py the byte rule the kernels implement gives the partition that dict
membership over the oracle's texts gives, and that those fixtures reach the cases the GPU tests name.  For the stores whose hash tags
collide by construction (tests/hashcraft.py): that they collide under the group's own table, and that a model of the table which confirms
a tag hit by less than length, byte count and all bytes gives another partition -- tests/test_join_host.py's model, over the store itself."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from tests.test_gpu_gather import make_store, upload, want_rows  # noqa: F401  (the helpers the fixtures are made with)
from tests import hashcraft
from tests.test_gpu_group import COLLIDERS, EDGE_SIZES, NONE, STORES, chain_fixture, collide_store, counting_fixture, csv_fixture, edges_fixture, failures_fixture, long_store, near_stores, want_group
from tests.test_gpu_join import CRAFT_RECORDS, CRAFTED, LANE_BYTES, LOW_BITS, TILE, _raw, handmade_fixture, host_hash, table_slots
from tests.test_join_host import CATCHES, CONFIRM, TableModel, items_of, orders
from tests.test_gpu_match import judged
from tests.test_gpu_shared import want_decode  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "et_group_packed_device"
NAMES = (NAME, "et_group_result_size", "et_group_records_max")
OK, ARG, UNSUPPORTED = 0, 6, 7  # et_status

assert NAME in N.SIGNATURES, f"{NAME} is not bound: every test of this file is about that call, its fixtures and its model"


def test_group_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared and name in N.SIGNATURES and name in exported, name
    assert len(N.SIGNATURES[NAME][1]) == 13  # (the argument list of the header's declaration)
    assert re.search(r"#define\s+ET_GROUP_NONE\s+0xffffffffu", header) and N.ET_GROUP_NONE == E.GROUP_NONE == NONE


def test_the_struct_has_the_size_the_headers_layout_implies():
    """uint64_t n_groups, n_failed, first_failed; int32_t first_status; uint32_t pad: 3 * 8 + 4 + 4 bytes, no padding of the compiler's."""
    assert [(name, ctypes.sizeof(t)) for name, t in N.GroupResult._fields_] == [("n_groups", 8), ("n_failed", 8), ("first_failed", 8), ("first_status", 4), ("pad", 4)]
    assert N.lib().et_group_result_size() == ctypes.sizeof(N.GroupResult) == 32
    assert N.lib().et_group_records_max() == N.lib().et_join_keys_max() == 1 << 24


def test_the_python_layer_exposes_the_calls():
    assert callable(E.Context.group_packed_device) and callable(E.Context.group_packed)
    assert [f.name for f in E.GroupResult.__dataclass_fields__.values()] == ["status", "n_groups", "n_failed", "first_failed", "first_status"]


def test_a_null_context_is_an_argument_error():
    assert N.lib().et_group_packed_device(None, None, None, 0, None, None, 0, None, 0, None, None, None, None) == ARG


# --- the fixtures of the GPU tests -----------------------------------------------------------------------------------------------------


def rule_groups(st):
    """The groups the kernels' rule gives, no decoding anywhere: both valid, equal lengths, equal byte counts, identical bytes; a body
    of no bytes under a length above zero equals nothing.  -> (first rows, counts, group_of)."""
    blob = st.bodies.tobytes()
    seen, first, counts, group_of = {}, [], [], []
    for b, (status, _, _) in enumerate(judged(st)):
        if status:
            group_of.append(NONE)
            continue
        length, body = int(st.text_index[b + 1]) - int(st.text_index[b]), blob[int(st.body_index[b]) : int(st.body_index[b + 1])]
        key = (b,) if length > 0 and not body else (length, len(body), body)
        if key not in seen:
            seen[key] = len(first)
            first.append(b)
            counts.append(0)
        counts[seen[key]] += 1
        group_of.append(seen[key])
    return first, counts, group_of


@pytest.mark.parametrize("name", sorted(STORES))
def test_the_byte_rule_gives_the_partition_that_membership_over_the_texts_gives(name):
    st = STORES[name]()
    first, counts, group_of = want_group(st)
    assert rule_groups(st) == (first, counts, group_of)
    valid = sum(1 for s, _, _ in judged(st) if not s)
    assert sum(counts) == valid and first == sorted(first) and all(group_of[b] == g for g, b in enumerate(first))


def test_on_a_hand_made_body_the_two_differ_as_the_header_says():
    st, _ = handmade_fixture()
    assert rule_groups(st) == ([0, 1, 2], [1, 1, 1], [0, 1, 2]) and want_group(st) == ([0, 2], [2, 1], [0, 0, 1])


def test_the_fixtures_reach_the_cases_the_gpu_tests_name():
    # edges: every size named, groups whose members lie in different wavefronts, and (from 257 on) different tiles
    assert EDGE_SIZES == [1, 63, 64, 65, 255, 256, 257, 513]
    for n in EDGE_SIZES:
        st = edges_fixture(n)
        first, counts, group_of = want_group(st)
        assert st.n == n and len(first) <= max(1, n // 3)
        members = {}
        for b, g in enumerate(group_of):
            members.setdefault(g, []).append(b)
        if n >= 65:
            assert any(len({b // 64 for b in m}) > 1 for m in members.values())
        if n > TILE:
            assert any(len({b // TILE for b in m}) > 1 for m in members.values()), "no group spans two tiles"
    # counting: one group over three tiles; none of two; one text on 90 %
    assert want_group(counting_fixture("one"))[:2] == ([0], [513])
    assert want_group(counting_fixture("distinct"))[1] == [1] * 513
    skewed = want_group(counting_fixture("skewed"))[1]
    assert max(skewed) > 0.85 * 513 and sum(skewed) == 513
    # the chain: 32 different records with one home slot in the table the call builds, over its last slot into its first, each twice
    st, info = chain_fixture()
    assert info.slots == table_slots(st.n) and 2 * st.n <= info.slots and info.home + COLLIDERS > info.slots
    texts = [t for _, _, t in judged(st)]
    assert len(set(info.colliders)) == COLLIDERS and all(texts.count(t) == 2 for t in info.colliders)
    assert all(host_hash(t, len(t)) & (info.slots - 1) == info.home for t in info.colliders)
    assert want_group(st)[1] == [2] * (st.n // 2)
    # near-equal: the last byte, the last bit, the length with one more byte; the length only; the byte count only
    near, trap, counts_only = near_stores()
    blob = trap.bodies.tobytes()
    same_bytes = {}
    for b, (_, length, _) in enumerate(judged(trap)):
        same_bytes.setdefault(blob[int(trap.body_index[b]) : int(trap.body_index[b + 1])], set()).add(length)
    assert any(len(v) >= 3 for v in same_bytes.values())
    sizes, lengths = np.diff(counts_only.body_index).astype(int), np.diff(counts_only.text_index).astype(int)
    assert lengths[0] == lengths[1] and sizes[0] != sizes[1]
    # long bodies: both sides of JOIN_LANE_BYTES in one tile, a pair that differs in its last 8-byte word only, a pair at the limit
    st = long_store()
    sizes = np.diff(st.body_index).astype(int)
    assert st.n <= TILE and int(sizes.min()) <= LANE_BYTES < 4096 <= int(sizes.max()) == N.lib().et_batch_small_max() // 4
    a, b = (st.bodies[int(st.body_index[i]) : int(st.body_index[i + 1])] for i in (1, 3))
    assert a.size == b.size == 4096 and np.array_equal(a[:-8], b[:-8]) and not np.array_equal(a[-8:], b[-8:])
    assert np.diff(st.text_index).astype(int).tolist().count(N.lib().et_batch_small_max()) >= 2
    # failures: a decreasing pair, a pair beyond the buffer, a length above the limit; two raw records of one length; two empty ones
    st = failures_fixture()
    statuses = [s for s, _, _ in judged(st)]
    assert statuses.count(ARG) == 4 and statuses.count(UNSUPPORTED) == 1 and int(st.body_index[9]) > st.bodies.size
    assert _raw(st, 5) and _raw(st, 10) and judged(st)[5][:2] == judged(st)[10][:2]
    assert [judged(st)[b][:2] for b in (2, 14)] == [(OK, 0)] * 2 and int(st.body_index[3]) == int(st.body_index[2])
    first, counts, group_of = want_group(st)
    assert group_of[5] != group_of[10] and group_of[2] == group_of[14] and counts[group_of[2]] == 2
    # the pipeline's store: 41 keys, the empty one among them
    _, lines = csv_fixture()
    assert len({line.split(b",")[1] for line in lines}) == 41


def test_the_group_call_has_a_row_that_keeps_both_states():
    from tests import retained as R
    from tests import retained_group as S

    assert R.NAMES.count("group") == 1 and R.row("group") is S.ROW and [r.name for r in R.ROWS] == R.NAMES
    row = R.row("group")
    assert NAME in row.calls and NAME in N.SIGNATURES and (row.hist, row.held, row.names, row.encodes) == (R.KEEPS, R.KEEPS, None, None)
    assert "group" not in R.DROPS_HISTOGRAM | R.DROPS_RANGE
    assert len(set(R.RECORDS)) == len(R.RECORDS) == 5  # (the row's store is RECORDS twice: five groups of two)


# --- hash tags that collide by construction (tests/hashcraft.py) ----------------------------------------------------------------------


def model_group(st, order, confirm):
    """want_group(st) as the hash table gives it (tests/test_join_host.py's TableModel over the store itself): a record's representative
    is the number in the first confirmed slot of its probe sequence, a group's number the rank of its representative."""
    items = items_of(st)
    table = TableModel(items, order, CONFIRM[confirm])
    reps = []
    for b, (status, _, _) in enumerate(judged(st)):
        reps.append(NONE if status else b if items[b] is None else table.find(items[b], own=b))
    first = [b for b, r in enumerate(reps) if r == b]
    rank = {b: g for g, b in enumerate(first)}
    return first, [reps.count(b) for b in first], [NONE if r == NONE else rank.get(r, NONE) for r in reps]


def test_the_crafted_stores_collide_under_the_groups_own_table():
    low = (1 << LOW_BITS) - 1
    for name in CRAFTED:
        st, info = collide_store(name)
        slots = table_slots(st.n)
        assert st.n == CRAFT_RECORDS and 256 < slots <= 1 << LOW_BITS, "the crafted homes are equal under the group's mask too"
        texts, statuses = [t for _, _, t in judged(st)], [s for s, _, _ in judged(st)]
        assert info.crafted == list(info.craft.keys) + list(info.craft.strangers) and len(set(info.crafted)) == len(info.crafted)
        for t in info.crafted:
            places = [b for b, u in enumerate(texts) if u == t]
            assert len(places) == info.copies[t] in (2, 3) and len({b // TILE for b in places}) == len(places), "every copy in another tile"
            assert all(host_hash(st.bodies[int(st.body_index[b]) : int(st.body_index[b + 1])], len(t)) == info.craft.hashes[t] for b in places)
        assert {2, 3} == set(info.copies.values())
        assert [b for b, s in enumerate(statuses) if s] == [info.failed] and statuses[info.failed] == ARG and TILE < info.failed < 2 * TILE
        assert [b for b in range(st.n) if _raw(st, b)] == [info.raw] and info.raw >= 2 * TILE
        first, counts, group_of = want_group(st)
        assert len(first) == len(info.crafted) + info.others and sorted(counts) == [1] * info.others + sorted(info.copies.values())
        for b, item in enumerate(items_of(st)):
            if item is not None:
                assert hashcraft.hash_of(item[1], item[0]) == host_hash(item[1], item[0])
    hashes = list(collide_store("one_tag")[1].craft.hashes.values())
    mask = table_slots(CRAFT_RECORDS) - 1
    assert len({h >> 32 for h in hashes}) == 1 and len({h & mask for h in hashes}) == 1 and len({h & 0xFFFFFFFF & ~low for h in hashes}) == len(hashes)
    h = collide_store("one_hash")[1].craft.h
    assert (h & mask) + 5 == mask + 1  # the chain of 32 wraps here as well


@pytest.mark.parametrize("name", CRAFTED)
def test_a_table_that_confirms_a_tag_hit_by_less_groups_wrongly(name):
    """tests/test_join_host.py's test of that name for the group call: the full confirmation gives the dict's partition in every
    insertion order, each weakening a different one on the fixtures CATCHES names."""
    st, _ = collide_store(name)
    want = want_group(st)
    for order in orders(st.n):
        assert model_group(st, order, "full") == want
        for weak, caught in CATCHES.items():
            assert (model_group(st, order, weak) != want) == (name in caught), (weak, name)
