"""et_join_packed_device as far as it can be checked without a GPU: declared, bound, exported, the result struct's size; et_join_hash
against the definition in csrc/et_join.h written out in Python -- for every division of a body's words into two groups and every
alignment of the buffer --; et_join_table_slots; and, in pure Python with the oracle, that on the stores and key sets of
tests/test_gpu_join.py the byte rule the kernels implement selects the rows dict membership over the texts selects, and that those
fixtures reach the cases the GPU tests name.  For the fixtures whose hash tags collide by construction (tests/hashcraft.py): that
hashcraft's hash is the library's, that every crafted pair collides as its docstring claims, and that a model of the hash table which
confirms a tag hit by less than length, byte count and ALL bytes answers wrongly on a named fixture -- so the fixtures can fail."""
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
from tests.test_gpu_join import COLLIDERS, CRAFT_KEYS, CRAFT_RECORDS, CRAFTED, FIXTURES, LANE_BYTES, LOW_BITS, NOT, TILE, WAVE_STEP, _raw, collide_fixture, collisions_fixture, \
    duplicates_fixture, handmade_fixture, hash_fixture, host_hash, table_slots, trap_fixture, want_join
from tests.test_gpu_match import _pack, judged
from tests.test_gpu_shared import _length_batch, want_decode  # noqa: F401
from tests.test_shared_host import table_2bit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("et_join_packed_device", "et_join_hash", "et_join_table_slots", "et_join_keys_max", "et_join_result_size", "et_selftest_join_hash")
OK, ARG = 0, 6  # et_status
M64 = (1 << 64) - 1
STEP = 0x9E3779B97F4A7C15  # csrc/et_join.h ET_JOIN_STEP


def test_join_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared and name in N.SIGNATURES and name in exported, name
    assert len(N.SIGNATURES["et_join_packed_device"][1]) == 19  # (the argument list of the header's declaration)
    assert N.lib().et_join_result_size() == ctypes.sizeof(N.JoinResult) == 48
    assert N.lib().et_join_keys_max() == 1 << 24
    assert [name for name, _ in N.JoinResult._fields_] == ["n_match", "n_failed", "first_failed", "n_keys_failed", "first_key_failed", "first_status", "first_key_status"]


def test_the_python_layer_exposes_the_calls():
    assert callable(E.Context.join_packed_device) and callable(E.Context.join_packed)
    assert [f.name for f in E.JoinResult.__dataclass_fields__.values()][:2] == ["status", "n_match"]


def test_a_null_context_is_an_argument_error():
    assert N.lib().et_join_packed_device(None, None, None, 0, None, None, 0, None, 0, None, None, 0, 0, None, 0, None, None, None, None) == ARG
    assert N.lib().et_selftest_join_hash(None, None, 0, None, None, 0, None) == ARG


# --- the hash ----------------------------------------------------------------------------------------------------------------------


def _mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _term(i, body):
    """Word i of the body -- 8 bytes, little-endian, the last one zero-extended -- with its position."""
    return _mix((int.from_bytes(body[8 * i : 8 * i + 8], "little") + (i + 1) * STEP) & M64)


def _finish(total, n_bytes, length):
    return _mix((total + _mix((length * STEP + n_bytes) & M64)) & M64)


def test_the_hash_is_its_definition_for_every_division_of_the_words_and_every_alignment():
    rng = np.random.default_rng(0x10A5E700)
    for n_bytes in list(range(0, 42)) + [63, 64, 65, LANE_BYTES - 1, LANE_BYTES, LANE_BYTES + 1, 1000]:
        body = rng.integers(0, 256, size=n_bytes).astype(np.uint8).tobytes()
        length = int(rng.integers(0, 1 << 18))
        words = (n_bytes + 7) // 8
        want = _finish(sum(_term(i, body) for i in range(words)) & M64, n_bytes, length)
        # the terms in two groups, summed apart and in the other order: any division of the words among lanes gives the sum
        for split in range(words + 1) if words <= 17 else (1, 64, words - 1):
            tail = sum(_term(i, body) for i in reversed(range(split, words))) & M64
            head = sum(_term(i, body) for i in range(split)) & M64
            assert _finish((tail + head) & M64, n_bytes, length) == want
        for shift in range(8):
            raw = np.full(n_bytes + 16, 0xA5, np.uint8)
            base = (-raw.ctypes.data) % 8 + shift
            raw[base : base + n_bytes] = np.frombuffer(body, np.uint8)
            assert (raw.ctypes.data + base) % 8 == shift
            assert int(N.lib().et_join_hash(raw.ctypes.data + base, n_bytes, length)) == want, (n_bytes, shift)
    assert host_hash(b"abc", 3) != host_hash(b"abc", 4) and host_hash(b"abc\0", 3) != host_hash(b"abc", 3)  # the length and the byte count count
    assert host_hash(b"A" * 8 + b"B" * 8, 2) != host_hash(b"B" * 8 + b"A" * 8, 2)  # a word's position counts


def test_the_table_is_a_power_of_two_and_at_most_half_full():
    for n_keys in [0, 1, 2, 3, 100, 127, 128, 129, 255, 256, 257, 2000, 65536, 65537, (1 << 24) - 1, 1 << 24]:
        slots = table_slots(n_keys)
        assert slots & (slots - 1) == 0 and slots >= 2 * n_keys and slots >= 2, n_keys
        assert slots == max(table_slots(0), 1 << (2 * n_keys - 1).bit_length()) if n_keys else True  # no larger than needed above the floor


# --- the fixtures of the GPU tests -------------------------------------------------------------------------------------------------


def rule_rows(st, ks, mode):
    """The rows the kernels' rule selects, and their keys: no decoding anywhere -- both valid, equal lengths, equal byte counts,
    identical bytes, a body of no bytes under a length above zero excluded."""
    blob, kblob = st.bodies.tobytes(), ks.bodies.tobytes()

    def item(s, data, i):
        b0, b1 = int(s.body_index[i]), int(s.body_index[i + 1])
        return int(s.text_index[i + 1]) - int(s.text_index[i]), data[b0:b1]

    keys = [item(ks, kblob, k) if not status else None for k, (status, _, _) in enumerate(judged(ks))]
    rows, found = [], []
    for b, (status, _, _) in enumerate(judged(st)):
        if status:
            continue
        me = item(st, blob, b)
        k = next((k for k, other in enumerate(keys) if other == me and not (me[0] > 0 and not me[1])), None)
        if (k is not None) != bool(mode & NOT):
            rows.append(b)
            found.append(k)
    return rows, found


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_byte_rule_selects_what_membership_over_the_texts_selects(name):
    st, ks = FIXTURES[name]()
    for mode in (0, NOT):
        assert rule_rows(st, ks, mode) == want_join(st, ks, mode), mode
    if not name.startswith("edges"):
        assert want_join(st, ks, 0)[0] and want_join(st, ks, NOT)[0]


def test_on_a_hand_made_body_the_two_differ_as_the_header_says():
    st, ks = handmade_fixture()
    assert rule_rows(st, ks, 0) == ([1], [0]) and want_join(st, ks, 0) == ([0, 1], [0, 0])


def test_the_fixtures_reach_the_cases_the_gpu_tests_name():
    # the hash fixture: every short size at every alignment, the threshold, several steps of a wavefront
    st, _ = hash_fixture()
    sizes = np.diff(st.body_index).astype(np.int64)
    assert {(int(s), int(a) % 8) for s, a in zip(sizes, st.body_index[:-1])} >= {(s, a) for s in range(1, 41) for a in range(8)}
    assert {0, LANE_BYTES - 1, LANE_BYTES, LANE_BYTES + 1} <= set(sizes.tolist()) and int(sizes.max()) >= 8 * WAVE_STEP
    # collisions: 32 keys with one home slot, a chain over the table's last slot, a record that is no key with its home inside the chain
    st, ks, info = collisions_fixture()
    assert info.slots == table_slots(ks.n) and ks.n * 2 <= info.slots
    kblob = ks.bodies.tobytes()
    homes = [host_hash(kblob[int(a) : int(b)], int(n)) & (info.slots - 1) for a, b, n in zip(ks.body_index[:-1], ks.body_index[1:], np.diff(ks.text_index))]
    assert homes.count(info.home) >= COLLIDERS == 32 and info.home + COLLIDERS > info.slots
    key_texts = {t for _, _, t in judged(ks)}
    texts = [t for _, _, t in judged(st)]
    assert key_texts <= set(texts) and info.inside in texts and info.inside not in key_texts
    assert 0 < (host_hash(info.inside, len(info.inside)) - info.home) % info.slots < COLLIDERS
    # the trap: two different texts with identical body bytes, on both sides
    st, ks = trap_fixture()
    tab = table_2bit()
    assert int(tab[0][ord("A")]) == 0 and int(tab[1][ord("A")]) == 2
    blob = st.bodies.tobytes()
    bodies = {}
    for b, (_, _, text) in enumerate(judged(st)):
        bodies.setdefault(blob[int(st.body_index[b]) : int(st.body_index[b + 1])], set()).add(text)
    assert {b"G", b"GA", b"GAA", b"GAAA"} in bodies.values() and {b"T", b"TA", b"TAA"} in bodies.values()
    # duplicates: 50 and 3 copies, several workgroups of 256 keys
    st, ks, info = duplicates_fixture()
    key_texts = [t for _, _, t in judged(ks)]
    assert ks.n == 2000 and key_texts.count(info.many) == 50 and key_texts.count(info.few) == 3
    assert key_texts.index(info.many) == info.first_many and key_texts.index(info.few) == info.first_few and info.first_many > 256
    # failures: a body of no bytes under a length above zero on both sides, with the same length
    st, ks = FIXTURES["failures"]()
    assert _raw(st, 5) and _raw(ks, 2) and 5 in want_join(st, ks, NOT)[0]


# --- hash tags that collide by construction (tests/hashcraft.py) --------------------------------------------------------------------


def body_of(text):
    return bytes(_pack(table_2bit(), text)) if len(text) else b""


def items_of(s):
    """Per record (length, body bytes) -- what the kernels hash and compare --, or None where the record fails or is kept raw."""
    blob = s.bodies.tobytes()
    return [None if status or _raw(s, b) else (int(s.text_index[b + 1]) - int(s.text_index[b]), blob[int(s.body_index[b]) : int(s.body_index[b + 1])])
            for b, (status, _, _) in enumerate(judged(s))]


def _sizes(a, b):
    return a[0] == b[0] and len(a[1]) == len(b[1])


# How a tag hit is confirmed: in full, as csrc/et_join.h demands, and the three weakenings a build could have.
CONFIRM = {"full": lambda a, b: a == b, "tag": lambda a, b: True, "sizes": _sizes, "first512": lambda a, b: _sizes(a, b) and a[1][:WAVE_STEP] == b[1][:WAVE_STEP]}


class TableModel:
    """The kernels' hash table, one step at a time: linear probing from hash & mask, a slot holds tag << 32 | number, an insert that
    meets a confirmed slot of its tag leaves the lower number there, a probe ends at the first empty slot."""

    def __init__(self, items, order, confirm):
        self.items, self.confirm, self.slots = items, confirm, table_slots(len(items))
        self.table = [None] * self.slots
        for k in order:
            if items[k] is not None:
                self.insert(k)

    def chain(self, item):
        h = hashcraft.hash_of(item[1], item[0])
        return h >> 32, ((h + i) & (self.slots - 1) for i in range(self.slots))

    def insert(self, k):
        tag, places = self.chain(self.items[k])
        for pos in places:
            old = self.table[pos]
            if old is None:
                self.table[pos] = tag << 32 | k
                return
            if old >> 32 == tag and self.confirm(self.items[k], self.items[old & 0xFFFFFFFF]):
                self.table[pos] = min(old, tag << 32 | k)
                return
        raise AssertionError("the table is full")

    def find(self, item, own=None):
        """The number in the first confirmed slot, or None at an empty one.  own: the group's probe, which takes a slot that holds the
        record's own number without a look at the bytes."""
        tag, places = self.chain(item)
        for pos in places:
            slot = self.table[pos]
            if slot is None:
                return None
            if slot >> 32 == tag and (slot & 0xFFFFFFFF == own or self.confirm(item, self.items[slot & 0xFFFFFFFF])):
                return slot & 0xFFFFFFFF
        raise AssertionError("no empty slot")


def orders(n):
    """Insertion orders to try: the identity, the reverse and three shuffles."""
    rng = np.random.default_rng(0x10A5ED00 + n)
    return [list(range(n)), list(reversed(range(n)))] + [[int(i) for i in rng.permutation(n)] for _ in range(3)]


def model_join(st, ks, order, confirm):
    """want_join(st, ks, 0) as the table gives it, the [min, max] filter of the keys' body sizes included."""
    table = TableModel(items_of(ks), order, CONFIRM[confirm])
    sizes = [len(item[1]) for item in table.items if item is not None]
    rows, keys = [], []
    for b, item in enumerate(items_of(st)):
        k = table.find(item) if item is not None and min(sizes) <= len(item[1]) <= max(sizes) else None
        if k is not None:
            rows.append(b)
            keys.append(k)
    return rows, keys


# Which fixture a weakened confirmation answers wrongly on, in every insertion order; on the others it answers as the dict does.
CATCHES = {"tag": {"one_tag", "one_hash", "sizes", "wave"}, "sizes": {"one_tag", "one_hash", "sizes", "wave"}, "first512": {"wave"}}


def test_hashcraft_restates_the_librarys_hash_and_inverts_it():
    rng = np.random.default_rng(0x10A5ED10)
    for x in [0, 1, hashcraft.M64, hashcraft.STEP] + [int(v) for v in rng.integers(0, 1 << 64, size=200, dtype=np.uint64)]:
        assert hashcraft.unmix(hashcraft.mix(x)) == x == hashcraft.mix(hashcraft.unmix(x)) and hashcraft.mix(x) == _mix(x)
    stores = [hash_fixture()[0]] + [s for name in CRAFTED for s in collide_fixture(name)[:2]]
    for st in stores:
        blob = st.bodies.tobytes()
        for a, b, n in zip(st.body_index[:-1], st.body_index[1:], np.diff(st.text_index)):
            assert hashcraft.hash_of(blob[int(a) : int(b)], int(n)) == host_hash(blob[int(a) : int(b)], int(n))
    for name in CRAFTED:
        for text, h in collide_fixture(name)[2].hashes.items():
            assert host_hash(body_of(text), len(text)) == h, name
    # the solved word at every place of a body, its last word partial or not
    for n_bytes in (8, 16, 21, 24, 136, 529):
        words = hashcraft.words_of(rng.integers(0, 256, size=n_bytes).astype(np.uint8).tobytes())
        for i in range(n_bytes // 8):
            h, length = int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, 1 << 18))
            w = hashcraft.solve_word(words[:i], words[i + 1 :], h, n_bytes, length)
            body = hashcraft.body_of(words[:i] + [w] + words[i + 1 :])[:n_bytes]
            assert host_hash(body, length) == h


def _differing_words(a, b):
    wa, wb = hashcraft.words_of(body_of(a)), hashcraft.words_of(body_of(b))
    assert len(wa) == len(wb)
    return {i for i, (x, y) in enumerate(zip(wa, wb)) if x != y}


def _size(text):
    return len(body_of(text)), len(text)


def test_the_crafted_fixtures_collide_as_they_claim():
    low = (1 << LOW_BITS) - 1
    for name in CRAFTED:
        st, ks, c = collide_fixture(name)
        crafted = list(c.keys) + list(c.strangers)
        texts, key_texts = [t for _, _, t in judged(st)], [t for _, _, t in judged(ks)]
        assert (st.n, ks.n, table_slots(ks.n)) == (CRAFT_RECORDS, CRAFT_KEYS, 256) and len(set(crafted)) == len(crafted) == len(c.hashes)
        assert all(texts.count(t) == 1 for t in crafted) and all(t in key_texts for t in c.keys) and not set(c.strangers) & set(key_texts)
        for part in (c.keys, c.strangers):
            assert len({texts.index(t) // TILE for t in part}) == 3 and len({texts.index(t) // 64 for t in part}) >= 3, "colliders in different tiles and wavefronts"
        assert all(host_hash(body_of(t), len(t)) == c.hashes[t] for t in crafted)
        rows, keys = want_join(st, ks, 0)
        assert {texts.index(t) for t in c.keys} <= set(rows) and not {texts.index(t) for t in c.strangers} & set(rows)
        sizes = [len(item[1]) for item in items_of(ks)]
        assert all(min(sizes) <= len(item[1]) <= max(sizes) for item in items_of(st)), "the [min, max] filter decides no record"
    # one tag, one home: equal upper halves, equal low 12 bits -- the home under the key set's 256 slots and the group's 2 048 --, and
    # a difference between the mask and bit 31; one word each
    c = collide_fixture("one_tag")[2]
    hashes = list(c.hashes.values())
    assert {h >> 32 for h in hashes} == {c.tag} and {h & low for h in hashes} == {c.low} and len({(h >> LOW_BITS) & 0xFFFFF for h in hashes}) == 16
    assert {_size(t) for t in c.hashes} == {(8, 32)} and len(c.keys) == len(c.strangers) == 8
    # one full hash: 32 texts of two words, both different in every pair; the home 5 below the table's end, 17 keys from there; one text
    # a key twice, at numbers apart
    st, ks, c = collide_fixture("one_hash")
    key_texts = [t for _, _, t in judged(ks)]
    assert set(c.hashes.values()) == {c.h} and len(c.hashes) == 32 and {_size(t) for t in c.hashes} == {(16, 64)}
    assert all(_differing_words(a, b) == {0, 1} for a in c.hashes for b in c.hashes if a != b)
    assert c.h & 255 == 256 - 5 and sum(t in c.hashes for t in key_texts) == 17 and len(c.keys) == 16
    twice = [k for k, t in enumerate(key_texts) if t == c.twice]
    assert len(twice) == 2 and twice[1] - twice[0] > 1 and c.twice in c.keys
    rows, keys = want_join(st, ks, 0)
    assert keys[rows.index([t for _, _, t in judged(st)].index(c.twice))] == twice[0]
    # one hash, other sizes
    c = collide_fixture("sizes")[2]
    a, b, c0 = c.keys
    c1, d, a2, b2 = c.strangers
    assert [_size(t) for t in (a, b, c0, c1, d, a2, b2)] == [(8, 32), (8, 31), (16, 64), (16, 64), (8, 30), (8, 32), (8, 31)]
    assert {c.hashes[t] for t in (a, b, c0, c1, d)} == {c.h} and c.hashes[a2] == c.hashes[b2] == c.h2 != c.h
    assert c.h2 >> 32 == c.h >> 32 and c.h2 & low == c.h & low
    assert len({body_of(t) for t in (a, b, d, a2, b2)}) == 5 and _differing_words(c0, c1) == {0, 1}
    # the wavefront path: one step and two; which words differ; lane-sized texts with the same hash on both sides
    c = collide_fixture("wave")[2]
    assert set(c.hashes.values()) == {c.h}
    assert [_size(t) for t in c.a + c.b + c.c + c.lanes] == [(136, 544)] * 2 + [(528, 2112)] * 5 + [(16, 64)] * 2
    assert 16 <= LANE_BYTES < 136 <= WAVE_STEP < 528 <= 2 * WAVE_STEP
    assert _differing_words(*c.a) == {0, 16} and _differing_words(*c.b) == {0, 65}
    assert all(_differing_words(x, y) == {64, 65} and body_of(x)[:WAVE_STEP] == body_of(y)[:WAVE_STEP] for x in c.c for y in c.c if x != y)
    assert c.keys == [c.a[0], c.b[0], c.c[0], c.c[2], c.lanes[0]] and c.strangers == [c.a[1], c.b[1], c.c[1], c.lanes[1]]


@pytest.mark.parametrize("name", CRAFTED)
def test_a_table_that_confirms_a_tag_hit_by_less_answers_wrongly(name):
    """The fixture can fail: the table model with the full confirmation gives the dict's answer in every insertion order; confirming by
    the tag alone, by tag and sizes, by tag, sizes and the first 512 bytes, it answers wrongly on the fixtures CATCHES names."""
    st, ks, _ = collide_fixture(name)
    want = want_join(st, ks, 0)
    for order in orders(ks.n):
        assert model_join(st, ks, order, "full") == want
        for weak, caught in CATCHES.items():
            assert (model_join(st, ks, order, weak) != want) == (name in caught), (weak, name)
    assert set().union(*CATCHES.values()) == set(CRAFTED) and all(CATCHES.values())
