"""The tables and texts of tests/limits.py reach the limits they are named for -- checked on the host, so that an input of
tests/test_gpu_limits.py which stops reaching its limit fails HERE: complete trees that the tree walk and the chained tables
take, chain plans as narrow (comb11: two index bits) and as wide (ladder32: eight) as the planner gets, encode rounds that fill a
ring to the last word, 32-bit codewords at every bit offset and across every kind of boundary, K4 chunks on the path they are
listed under, and histograms whose trees are 31, 32 and 33 levels deep.  No GPU."""
import ctypes

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from oracle import oracle as O
from tests import limits as L
from tests.test_host_logic import _chain_tables

TABLES = [t.name for t in L.all_tables()]


def _path(cb):
    p = ctypes.c_uint32(99)
    rc = N.lib().et_decode_path(ctypes.byref(cb.raw), ctypes.byref(p))
    return rc, p.value


def test_shapes_are_what_the_names_say():
    def lens(t):
        return sorted(t.length[t.length > 0].tolist())

    assert lens(L.ladder32()) == list(range(1, 33)) + [32]
    assert lens(L.ladder31()) == list(range(1, 32)) + [31]
    assert lens(L.broom32()) == list(range(1, 28)) + [32] * 32
    ladder = list(range(12, 33)) + [32]
    assert lens(L.comb8()) == sorted(list(range(1, 8)) + [11] * 8 + ladder * 8)
    assert lens(L.comb11()) == sorted(list(range(1, 8)) + [11] * 5 + ladder * 11) and L.comb11().coded.size == 254
    # the combs' ladders hang under the 16 nodes 1111111xxxx, their 32-bit codes end in 20 ones and one more bit
    for t, k in ((L.comb8(), 8), (L.comb11(), 11)):
        deep = t.data[t.of_len(32)].astype(np.int64)
        assert sorted(set((deep >> 21).tolist())) == [(0x7F << 4) | j for j in range(k)] and bool((((deep >> 1) & 0xFFFFF) == 0xFFFFF).all())
    for t in (L.ladder32(), L.comb11()):
        m = L.mirror(t)
        assert np.array_equal(m.length, t.length)
        assert all(int(m.data[s]) + int(t.data[s]) == (1 << int(t.length[s])) - 1 for s in t.coded)
    assert int(L.mirror(L.ladder32()).data[L.ladder32().of_len(32)].min()) == 0  # a run of 32 zeros
    t = L.long255()
    assert not t.complete and t.max_len == 255 and t.of_len(255).size == 4


@pytest.mark.parametrize("name", TABLES)
def test_tables_are_complete_trees_for_the_tree_walk(name):
    t = L.table(name)
    cb = t.codebook()
    assert cb.raw.max_length == t.max_len and cb.raw.n_coded == t.coded.size
    if not t.complete:
        assert N.lib().et_codebook_is_complete(ctypes.byref(cb.raw)) == N.ET_ERR_UNSUPPORTED
        return
    assert N.lib().et_codebook_is_complete(ctypes.byref(cb.raw)) == N.ET_OK
    assert _path(cb) == (N.ET_OK, N.ET_PATH_TREE_WALK)
    n_int = ctypes.c_uint32(0)
    table = np.zeros((256 + 7) * 256, dtype=np.uint16)
    assert N.lib().et_treewalk_table(ctypes.byref(cb.raw), table.ctypes.data, table.size, ctypes.byref(n_int)) == N.ET_OK
    assert n_int.value == t.coded.size - 1


def test_chain_plans_at_their_narrowest_and_widest():
    """Index bits of the widest sub-table (the root has 11): the planner narrows all of them together until they fit."""
    widest, count = {}, {}
    for t in L.complete_tables():
        table, first, bits = _chain_tables(t.codebook())
        assert bits[0] == 11 and table.size <= 2048 + 576
        widest[t.name], count[t.name] = int(bits[1:].max()), first.size - 1
    assert widest["comb11"] <= 2 and widest["mirror_comb11"] <= 2
    assert widest["comb8"] <= 3
    assert widest["ladder32"] >= 8 and widest["mirror_ladder32"] >= 8
    assert count["comb11"] >= 100  # (121 at the time of writing: a 32-bit codeword takes about a dozen lookups)


def test_dense_rounds_fill_the_rings():
    for name, bits_per_round in (("ladder32", 131072), ("ladder31", 126976), ("broom32", 131072), ("long255", 4096 * 255)):
        t = L.table(name)
        for text_name in ("dense", "alternating"):
            if (name, text_name) not in L.RING_PAIRS:
                continue
            text = L.text_of(name, text_name, L.RING_N)
            per_round = t.bits(text[: L.RING_N // L.ROUND * L.ROUND]).reshape(-1, L.ROUND).sum(axis=1)
            assert per_round.size == 5
            if text_name == "dense":
                assert (per_round == bits_per_round).all(), name
            else:  # full rounds and rounds of 1-bit symbols take turns
                assert per_round.tolist() == [bits_per_round, 4096, bits_per_round, 4096, bits_per_round], name
    assert L.dense(L.broom32(), L.RING_N).min() >= 127 and np.unique(L.dense(L.broom32(), L.RING_N)).size == 32
    # a step of the long kernel: 256 symbols of 255 bits
    assert int(L.long255().bits(L.text_of("long255", "dense", L.RING_N)[:256]).sum()) == 256 * 255


def test_phases_put_the_longest_codeword_everywhere():
    t = L.ladder32()
    for n in (L.DECODE_N, L.COLD_N):
        text = L.text_of("ladder32", "phases", n)
        b = t.bits(text)
        assert set(b[0::2].tolist()) == {32} and set(b[1::2].tolist()) == set(range(1, 32))
        assert {131, 132} <= set(text.tolist())
        for first_bit in (0, 8, 13):  # the body as packed; behind a pointer offset of 1 with start bits 0 and 5
            s = L.starts(t, text, first_bit)
            at = s[b == 32] % 256
            assert np.unique(at).size == 256, "32-bit codewords do not begin at every offset of a 256-bit subsequence"
            assert int(np.count_nonzero(at >= 224)) >= 1
            assert L.straddles(t, text, 2048 * 8, first_bit) >= 1, "no 32-bit codeword across a 2 KiB quarter boundary"
            assert L.straddles(t, text, 8192 * 8, first_bit) >= 1, "no 32-bit codeword across an 8 KiB block boundary"
    # every 32-bit-code table: the longest codeword begins at every offset of a 32-bit word
    for name in L.DECODE_TABLES:
        t = L.table(name)
        text = L.text_of(name, "phases", L.DECODE_N)
        b = t.bits(text)
        assert np.unique(L.starts(t, text)[b == t.max_len] % 32).size == 32, name


def test_uniform_texts_use_every_symbol():
    for name in L.DECODE_TABLES:
        t = L.table(name)
        assert np.unique(L.text_of(name, "uniform", L.DECODE_N)).size == t.coded.size, name


def test_k4_patterns_take_the_paths_they_are_listed_under():
    t = L.ladder32()
    assert len(L.K4_PATTERNS) == 16 and len({q for _, q in L.K4_PATTERNS}) == 16
    for path, quad in L.K4_PATTERNS:
        assert L.k4_path(tuple(quad) * 4) == path, quad
        for position in range(4):  # one such quad among 1-bit symbols decides the same way
            assert L.k4_path(L.k4_chunk_lengths(quad, position)) == path, (quad, position)
        bits = sum(0 if x == L.Z else x for x in quad)
        assert (bits == 32) if path == L.QUAD else (bits > 32)
        text = L.k4_whole_rounds(t, quad, L.K4_N)
        assert text.size == L.K4_N and t.bits(text[:4]).tolist() == [0 if x == L.Z else x for x in quad]
        for lane in L.K4_LANES:
            one = L.k4_one_chunk(t, quad, L.K4_N, lane, 2)
            other = np.flatnonzero(one != t.sym(1))
            assert other.size and other.min() >= lane * 16 + 8 and (other % L.ROUND).max() < lane * 16 + 12 and other.max() < 2 * L.ROUND
    assert L.k4_path((1,) * 16) == L.QUAD  # the chunks around the one: the wavefront's other lanes vote for whole quads
    assert t.length[t.sym(L.Z)] == 0


@pytest.mark.parametrize("max_len", [31, 32, 33])
def test_fibonacci_histograms_give_trees_of_31_32_and_33_levels(max_len):
    hist = L.fibonacci_histogram(max_len)
    _, length, _ = O.build_dict(hist)
    assert int(length.max()) == max_len
    cb = E.Codebook.from_histogram(hist)
    assert cb.raw.max_length == max_len and np.array_equal(cb.length, length)
    assert int(hist.sum()) <= 13_000_000


def _image(t, text, start_bit=0):
    body = O.pack_body(t.data, t.length, text, start_bit)[0]
    return t.codebook().header(text.size) + body


@pytest.mark.parametrize("name,text_name", L.DECODE_PAIRS + [p for p in L.RING_PAIRS if p[0] != "long255"] + L.COLD_PAIRS)
def test_the_oracle_round_trips_every_pair(name, text_name):
    t = L.table(name)
    n = L.DECODE_N if (name, text_name) in L.DECODE_PAIRS else L.RING_N
    sizes = {n} | ({L.COLD_N} if (name, text_name) in L.COLD_PAIRS else set()) | ({L.RING_N} if (name, text_name) in L.RING_PAIRS else set())
    for n in sorted(sizes):
        text = L.text_of(name, text_name, n)
        assert O.decode(_image(t, text)[4:]) == text.tobytes(), (name, text_name, n)


def test_the_oracle_round_trips_the_k4_patterns_without_uncoded_bytes():
    t = L.ladder32()
    for _, quad in L.K4_PATTERNS:
        if L.Z in quad:
            continue
        for text in (L.k4_whole_rounds(t, quad, L.K4_N), L.k4_one_chunk(t, quad, L.K4_N, 63, 3)):
            assert O.decode(_image(t, text)[4:]) == text.tobytes(), quad


def test_the_header_of_a_hand_made_table_is_the_oracles():
    for t in L.complete_tables():
        assert t.codebook().header(L.DECODE_N) == O.write_header(t.data, t.length, L.DECODE_N), t.name


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("name,text_name", L.COLD_PAIRS)
def test_cold_ranges_cut_through_a_longest_codeword(name, text_name, ranks):
    """The block ranges tests/test_gpu_limits.py hands to 2 and 3 ranks (the image at a 4-byte aligned address): at least four
    blocks, and a 32-bit codeword across a boundary between two ranges."""
    t = L.table(name)
    text = L.text_of(name, text_name, L.COLD_N)
    body_off = len(t.codebook().header(text.size)) - 4
    first_bit = (body_off & 3) * 8
    n_bytes = (body_off & 3) + (int(t.bits(text).sum()) + 7) // 8
    n_blocks = (n_bytes + 8191) // 8192
    assert n_blocks >= 4
    begins, bits = L.starts(t, text, first_bit), t.bits(text)
    cuts = [r * n_blocks // ranks * 8192 * 8 for r in range(1, ranks)]
    assert any(bool(((begins < at) & (begins + bits > at) & (bits == 32)).any()) for at in cuts), cuts
