"""et_join_packed_device as far as it can be checked without a GPU: declared, bound, exported, the result struct's size; et_join_hash
against the definition in csrc/et_join.h written out in Python -- for every division of a body's words into two groups and every
alignment of the buffer --; et_join_table_slots; and, in pure Python with the oracle, that on the stores and key sets of
tests/test_gpu_join.py the byte rule the kernels implement selects the rows dict membership over the texts selects, and that those
fixtures reach the cases the GPU tests name."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from tests.test_gpu_gather import make_store, upload, want_rows  # noqa: F401  (the helpers the fixtures are made with)
from tests.test_gpu_join import COLLIDERS, FIXTURES, LANE_BYTES, NOT, WAVE_STEP, _raw, collisions_fixture, duplicates_fixture, handmade_fixture, hash_fixture, host_hash, \
    table_slots, trap_fixture, want_join
from tests.test_gpu_match import judged
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
