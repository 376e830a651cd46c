"""GPU: the order modes of et_match_packed_device -- ET_MATCH_LESS and ET_MATCH_LESS_EQUAL, with ET_MATCH_NOT >= and > -- found on the
compressed bytes, against the oracle: a record's status is judged from its own two pairs of offsets (want_rows), its text is
want_decode's, and the expected rows are Python's `text < needle` / `text <= needle` over those texts; never the bit rule the kernel
implements.  d_rows (cap_rows + TAIL entries) and d_status are filled with sentinels first; everything behind n_match must still hold
them.

The stores and needles are made by the *_fixture functions below, without a GPU: tests/test_order_host.py states the bit rule in
Python, checks on the same fixtures that it selects what Python's comparison selects, that they reach the cases named here, and that
under no needle more than a quarter of a store's records take one branch of the rule -- which is why a needle has a store of its own,
made of the records that stand in every relation to it (relatives)."""
import bisect
import functools
import os

import numpy as np
import pytest

from tests.test_gpu_batch import SENTINEL
from tests.test_gpu_gather import _mixed_store, upload
from tests.test_gpu_match import EQUAL, NOT, PREFIX, ROW_SENTINEL, TILE, _pack, _store, judged, run_match, want_match
from tests.test_gpu_packed import TAIL, _dev_index, _index_of
from tests.test_shared_host import canonical, oracle_table, table_255, table_2bit, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
LESS, LESS_EQUAL = 4, 5  # ET_MATCH_*
ORDER_MODES = [LESS, LESS_EQUAL, LESS | NOT, LESS_EQUAL | NOT]
HEAD_BITS = 64  # what a lane compares alone (csrc/et_batch.h MATCH_HEAD_BITS)
GRID = 2048  # workgroups of the flag kernel at most (csrc/et_batch.h MATCH_GRID)
STEP_BYTES = 256  # what the wavefront compares per step behind the head: 64 lanes x 4 bytes


# --- the expected rows: the oracle's texts, Python's comparison -------------------------------------------------------------------


def select_order(wants, needle, mode):
    needle, out = bytes(needle), []
    for b, (status, _, text) in enumerate(wants):
        if status:
            continue
        hit = text < needle if mode & ~NOT == LESS else text <= needle
        if hit != bool(mode & NOT):
            out.append(b)
    return out


def want_order(st, needle, mode):
    return select_order(judged(st), needle, mode)


def codable_bits(tab, needle):
    """pattern_bits of an order call: the bits of the needle's bytes in front of its first byte without a code."""
    bits = 0
    for s in bytes(needle):
        if not int(tab[1][s]):
            break
        bits += int(tab[1][s])
    return bits


def check_order(r, wants, needle, mode, call_status=OK, pattern_bits=None):
    want = select_order(wants, needle, mode)
    statuses = [s for s, _, _ in wants]
    failed = [b for b, s in enumerate(statuses) if s]
    assert (r.res.status, r.res.n_match, r.res.n_failed) == (call_status, len(want), len(failed)), (r.res, len(want), len(failed))
    if failed:
        assert (r.res.first_failed, r.res.first_status) == (failed[0], statuses[failed[0]]), r.res
    if pattern_bits is not None:
        assert r.res.pattern_bits == pattern_bits
    assert list(r.status) == statuses, "a status byte differs"
    if r.count_only or call_status != OK:
        assert bool((r.rows == ROW_SENTINEL).all()), "an entry of d_rows was written"
        return want
    got = r.rows[: len(want)].tolist()
    assert got == want, f"the rows differ from Python's, first at {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"
    assert bool((r.rows[len(want) :] == ROW_SENTINEL).all()), "an entry at or behind d_rows + n_match was written"
    return want


def order(ctx, st, needle, mode, dev=None, **kw):
    """Run with cap_rows = the need exactly, and check."""
    need = len(want_order(st, needle, mode))
    r = run_match(ctx, st.cb, dev or upload(st), st.n, needle, mode, need)
    check_order(r, judged(st), needle, mode, pattern_bits=codable_bits(st.tab, needle), **kw)
    return r


def all_modes(ctx, st, needles, dev=None):
    dev = dev or upload(st, spare=st.bodies.size)  # (what lies behind body_bytes is mapped: a bad pair that is followed shows, or faults)
    for needle in needles:
        for mode in ORDER_MODES:
            order(ctx, st, needle, mode, dev=dev)


# --- the fixtures: (store, needles), made without a GPU -----------------------------------------------------------------------------

CUT_BEHIND = 2  # where relatives() puts the record whose body is cut exactly behind the needle


def relatives(tab, nd, diffs, more):
    """The records that stand in every relation to the needle `nd`, about as many in each: -> [(text, body or None)].  diffs: (position,
    a byte below nd[position], a byte above it), all with a code; `more` is a byte whose code has 8 bits or more (so a body cut behind
    the needle's last byte ends inside it)."""
    nd = bytes(nd)
    whole, pat_bytes = _pack(tab, nd), (codable_bits(tab, nd) + 7) // 8
    j, low, high = diffs[0]
    out = [(nd, None), (nd, whole + b"\0\0"),  # equal; with a body longer than its length needs
           (nd + bytes([more]), _pack(tab, nd + bytes([more]))[:pat_bytes]),  # cut exactly behind the needle: EQUAL here, not under ET_MATCH_EQUAL
           (nd + bytes([low]), None), (nd + bytes([high]), None), (nd + bytes([more]), None),  # the needle a proper prefix of the record
           (nd[:j] + bytes([low]), None), (nd[:j] + bytes([high]), None),  # the first difference at symbol j, and the record ends there
           (nd[:-1], None),  # a proper prefix of the needle
           (nd, whole[:-1]), (nd, b""), (b"", b""),  # a body that ends inside the needle's bits; none under a length above zero; the empty record
           (nd[:-1], whole)]  # a whole body whose length stops before the needle does
    if len(nd) > 2:
        out.append((nd[:-2], whole))
    for k, lo, hi in diffs:  # the first difference at symbol k, the rest as the needle's
        out += [(nd[:k] + bytes([lo]) + nd[k + 1 :], None), (nd[:k] + bytes([hi]) + nd[k + 1 :], None)]
    return out


def _related_store(tab, families):
    texts, bodies = [], []
    for fam in families:
        for text, body in fam:
            texts.append(text)
            bodies.append(_pack(tab, text) if body is None else body)
    return _store(tab, texts, bodies)


def with_failures(st):
    """The store with its last four records made to fail (ET_ERR_ARG): two body offsets of 2^63 spoil two pairs each."""
    st.body_index[st.n - 3] = st.body_index[st.n - 1] = np.uint64(1) << np.uint64(63)
    return st


def _midsummer_table():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "res", "a_midsummer_nights_dream.txt"), "rb") as f:
        return oracle_table(np.frombuffer(f.read(), np.uint8))


def left_aligned(tab, s):
    return int(tab[0][s]) << (32 - int(tab[1][s]))


def order_pairs(tab, symbols):
    """-> (pairs a < b whose codes order the same way, pairs a < b whose codes order the other way) among `symbols`."""
    same, other = [], []
    for a in symbols:
        for b in symbols:
            if a < b:
                (same if left_aligned(tab, a) < left_aligned(tab, b) else other).append((a, b))
    return same, other


def _around(tab, s):
    """A byte below and a byte above `s`, both with a code."""
    coded = [int(c) for c in np.flatnonzero(tab[1])]
    return max(c for c in coded if c < s), min(c for c in coded if c > s)


SYMBOL_LETTERS = b" etaoinshrdlu,.AEIOT"


@functools.lru_cache(maxsize=None)
def symbol_order_fixture(k, swapped):
    """The Midsummer table: a needle and records that differ from it first at a pair of symbols a < b whose codes order as the bytes do
    (k = 0 .. 2) or the other way (k = 3 .. 5) -- the needle with a and records with b, or swapped -- behind stems of 1, 3 and 11
    shared symbols."""
    tab = _midsummer_table()
    same, other = order_pairs(tab, [s for s in SYMBOL_LETTERS if int(tab[1][s])])
    a, b = (same[:3] + other[:3])[k][:: -1 if swapped else 1]
    stem = [b"t", b"the", b"the fair Hi"][k % 3]
    nd = stem + bytes([a]) + b"e."
    fam = relatives(tab, nd, [(len(stem), *_around(tab, a)), (len(stem) + 1, *_around(tab, ord("e")))], int(np.argmax(tab[1])))
    fam += [(stem + bytes([b]) + b"e.", None), (stem + bytes([b]), None)]
    return _related_store(tab, [fam]), [nd]


FIRST_DIFF_BITS = sorted(set(range(8)) | {8 * k for k in range(1, 21)} | {63, 64, 65} | {64 + 32 * k + e for k in (1, 2, 63, 64) for e in (-1, 0, 1)}
                         | {8 * 20 + 3, 8 * STEP_BYTES + 5, 8 * (8 + STEP_BYTES) + 2, 8 * 299 + 7})


@functools.lru_cache(maxsize=None)
def first_difference_fixture():
    """table_255: byte s >= 2 has the 8-bit code s, byte 1 the 7-bit code 0000000.  A needle of 300 bytes 0x55 / 0xAA (then one byte 1: a
    last, partial pattern byte) and records that are the needle with ONE bit flipped -- 0 -> 1 is above, 1 -> 0 below -- at every bit of
    byte 0, behind 1 .. 20 shared symbols, at the head's edge, at the wavefront path's word edges 64 + 32k +- 1 and across its first
    step boundary (byte 264); then the relations, so that the flips are no majority."""
    tab = table_255()
    assert all(int(tab[0][s]) == s and int(tab[1][s]) == 8 for s in (0x55, 0xAA, 0x15, 0xD5)) and int(tab[1][1]) == 7
    base = bytes([0x55, 0xAA] * 150)
    nd = base + b"\x01"
    texts = []
    for p in FIRST_DIFF_BITS:
        t = bytearray(nd)
        t[p // 8] ^= 0x80 >> (p % 8)
        texts.append(bytes(t))
    fam = [(t, None) for t in texts] + [(base + b"\x02", None), (base + b"\x03q", None)]  # ... and in the last, partial byte
    whole = _pack(tab, nd)
    for _ in range(3):
        fam += [(nd, None), (nd, whole + b"\0"), (nd + b"\x07", _pack(tab, nd + b"\x07")[:-1]),  # equal; cut behind the needle
                (nd + b"\x01", None), (nd + b"\x02", None), (nd + b"\xf0", None),  # the needle a proper prefix
                (base, None), (base[:264], None), (base[:8], None), (nd, whole[:270]), (nd, b""),  # the body a prefix of the pattern
                (base, whole), (base[:100], whole), (base[:9], whole)]  # the length stops inside the needle
    return _related_store(tab, [fam]), [nd]


@functools.lru_cache(maxsize=None)
def relations_fixture(k):
    """Prefix relations under table_255: the zero-codeword trap -- the needle goes on with k symbols whose code is all zero bits, so a
    shorter record's pad bits agree with it -- and (k = 1) hand-made bodies whose pad bits DIFFER from the needle."""
    tab = table_255()
    stem = bytes([65, 200, 3])
    nd = stem + b"\x01" * k
    fam = relatives(tab, nd, [(2, 2, 250), (0, 60, 70)], 77)
    if k == 1:
        pad = bytearray(_pack(tab, stem))
        fam += [(stem, bytes(pad) + b"\xff"), (stem[:2], _pack(tab, stem[:2]) + b"\x7f")]  # bytes behind the last codeword, above the needle's next symbol
    if k >= 2:  # behind the 7-bit codeword an 8-bit one straddles bytes: cut at 4 bytes it differs from the needle in its first bit and ends beyond the body
        fam.append((stem + b"\x01\xf0", _pack(tab, stem + b"\x01\xf0")[:4]))
    return _related_store(tab, [fam]), [nd]


RELATIONS_2BIT = [b"GC", b"TGA", b"CGTA", b"CGTAA", b"TCAAA"]
PAD_RECORDS = {b"GC": [(b"G", bytes([0b10110000])), (b"G", bytes([0b10100000]))], b"CGTA": [(b"CG", bytes([0b01101111])), (b"CGT", bytes([0b01101111]))]}


@functools.lru_cache(maxsize=None)
def relations_2bit_fixture(nd):
    """Four symbols of 2 bits, A = 00: needles that end in A's (the trap), and hand-made bodies whose pad bits differ from the needle and
    would decode to a symbol ABOVE needle[i] -- "G" = 10 with the pad 11: T, against GC -- still a proper prefix, still LESS."""
    tab = table_2bit()
    first = {ord("G"): [(0, ord("C"), ord("T"))], ord("C"): [(0, ord("A"), ord("G"))]}.get(nd[0], [])  # (nothing is above T)
    fam = relatives(tab, nd, [(1, ord("A"), ord("T"))] + first, ord("T")) + PAD_RECORDS.get(nd, [])
    return _related_store(tab, [fam]), [nd]


@functools.lru_cache(maxsize=None)
def empty_needle_fixture():
    """The empty needle: nothing is less; LESS_EQUAL selects the records whose stored text is empty -- by their length, or because no
    codeword ends inside their body.  A quarter each: length 0, no body or a cut one, a text, and records that fail."""
    tab = table_2bit()
    fam = [(b"", b""), (b"", b"\x1b"), (b"", b""), (b"", b"\x00")]
    fam += [(b"G", b""), (b"TA", b""), (b"ACGT", b""), (b"C", b"")]
    fam += [(b"G", None), (b"A", None), (b"TACG", None), (b"AAAAA", None)]
    fam += [(b"GC", None)] * 4
    return with_failures(_related_store(tab, [fam])), [b""]


def table_254():
    """255 byte values (0 .. 254): byte 0 has the 7-bit code, byte 255 none -- table_255 with the hole at the other end."""
    return canonical({0: 7, **{s: 8 for s in range(1, 255)}})


UNCODED_STEM = bytes([66, 201, 9, 130, 47])


@functools.lru_cache(maxsize=None)
def uncoded_fixture(which, where):
    """A needle byte without a code -- 0 under table_255, below every symbol; 255 under table_254, above every symbol -- at position 0
    ("first"), behind two bytes with a code ("middle") and last, against records that stop before, at and beyond the codable prefix."""
    tab, hole = (table_255(), 0) if which == "below" else (table_254(), 255)
    assert int(tab[1][hole]) == 0
    stem, h = UNCODED_STEM, bytes([hole])
    if where == "first":  # no codable prefix: a quarter each of empty records, raw or cut ones, texts, and records that fail
        fam = [(b"", b""), (b"", b"\x1b"), (b"", b""), (b"", b"\x99")]
        fam += [(b"\x42", b""), (b"\x42\x43", b""), (b"\x09", b""), (b"\xc9", b"")]
        fam += [(b"\x02", None), (b"\xfe", None), (stem, None), (b"\x01\x01", None)]
        fam += [(stem, None)] * 4
        return with_failures(_related_store(tab, [fam])), [h, h + stem]
    pre = stem[:2] if where == "middle" else stem
    fam = relatives(tab, pre, [(1, pre[1] - 1, pre[1] + 1), (0, pre[0] - 1, pre[0] + 1)], 0x20)
    return _related_store(tab, [fam]), [pre + h + stem[len(pre) :]] + ([pre + h + h] if where == "last" else [])


@functools.lru_cache(maxsize=None)
def ladder_fixture(which):
    """The ladder table: bytes 131 and 132 have the two 32-bit codes (all ones but the last bit), byte 107 an 8-bit one, byte 100 one
    bit.  "short": behind a 32-bit, an 8-bit and a 1-bit symbol a 32-bit codeword straddles two words.  "long": the longest needle there
    is -- 4 096 bytes of 32-bit codes, 16 KiB of pattern -- takes the boundary table up to 2^17."""
    tab = table_ladder()
    assert int(tab[1][131]) == 32 and int(tab[1][132]) == 32 and int(tab[1][107]) == 8 and int(tab[1][100]) == 1
    rng = np.random.default_rng(0x0DE40010)
    long = (131 + rng.integers(0, 2, size=4096)).astype(np.uint8).tobytes()
    if which == "short":
        short = long[:1] + bytes([107, 100, 131, 132, 131])
        return _related_store(tab, [relatives(tab, short, [(3, 130, 132), (1, 106, 108)], 131)]), [short]

    def flip(t, i, to=None):
        u = bytearray(t)
        u[i] = 263 - u[i] if to is None else to
        return bytes(u)

    if which == "cut":  # where the needle has 8 bits and a record 32, a body can end inside the deciding codeword on the wavefront path
        p = 150 + long[150:].index(131)
        nd = flip(long[:200], 100, 107)
        fam = relatives(tab, nd, [(100, 106, 108), (p, 130, 132)], 131) + [(long[:200], _pack(tab, long[:200])[:401]), (long[:101], _pack(tab, long[:200])[:402])]
        return _related_store(tab, [fam]), [nd]
    whole = _pack(tab, long)
    up, down = [i for i in range(66, 4095) if long[i] == 131], [i for i in range(66, 4095) if long[i] == 132]  # (131 -> 132 is above, 132 -> 131 below)
    fam = [(flip(long, i), None) for i in (0, 1, up[0], up[-1], down[0], down[-1], 4095)] + [(flip(long, i, 107), None) for i in (0, 1, 66)]  # (107 is below both)
    fam += [(long, None), (long, whole + b"\0"), (long, None)]
    fam += [(long[:4095], None), (long[:1000], None), (long, whole[:-1]), (long, b""), (b"", b"")]
    fam += [(long[:4095], whole), (long[:1000], whole), (long[:1], whole), (long[:3], whole)]
    return _related_store(tab, [fam]), [long]


TILE_TEXTS = [(b"G", None)] * 3 + [(b"GC", None)] * 3 + [(b"GG", None)] * 2 + [(b"GA", None)] * 2 + [(b"GT", None)] + [(b"GCA", None)] * 3 + [(b"A", None), (b"C", None), (b"T", None)] + [(b"", b"")] * 2 + [(b"GC", b"")]


@functools.lru_cache(maxsize=None)
def tiles_fixture(n):
    """n tiny records under the 2-bit table: twenty records in every relation to the needle GC in turn, from a place that depends on n."""
    return _related_store(table_2bit(), [[TILE_TEXTS[(7 * i + n) % 20] for i in range(n)]]), [b"GC"]


WRAP_N = GRID * TILE + 300
WRAP_NEEDLE = b"GC"
WRAP_TEXTS = [[b"A", b"C", b"GA"], [b"T", b"GG", b"GT"], [b"GC"] * 3, [b"G"] * 3, [b"GC"] * 3]  # below; above; equal; a proper prefix; raw: no body under a length of 2
WRAP_BELOW, WRAP_ABOVE, WRAP_EQUAL, WRAP_PREFIX, WRAP_RAW = range(5)


@functools.lru_cache(maxsize=None)
def wrap_store():
    """One store that wraps the tile grid once: GRID x TILE + 300 records of one or two symbols under the 2-bit table, made with numpy, a
    fifth each in five relations to the needle GC -> (bodies, body_index, lengths, kind, which): record b is WRAP_TEXTS[kind[b]][which[b]],
    its body one byte, or none (WRAP_RAW)."""
    rng = np.random.default_rng(0x0DE40020)
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    assert all(int(table_2bit()[0][s]) == c and int(table_2bit()[1][s]) == 2 for s, c in code.items())
    kind, which = rng.integers(0, 5, size=WRAP_N), rng.integers(0, 3, size=WRAP_N)
    byte = np.array([[code[t[0]] << 6 | (code[t[1]] << 4 if len(t) == 2 else 0) for t in row] for row in WRAP_TEXTS], np.uint8)
    length = np.array([[len(t) for t in row] for row in WRAP_TEXTS], np.uint64)
    sizes = (kind != WRAP_RAW).astype(np.uint64)
    return byte[kind, which][kind != WRAP_RAW], _index_of(sizes), length[kind, which], kind, which


@functools.lru_cache(maxsize=None)
def operators_fixture():
    """A store in every relation to its needle, with four records that fail: for the four operators, capacity and count-only calls."""
    tab = table_255()
    nd = bytes([65, 200, 3, 1, 1])
    fam = relatives(tab, nd, [(2, 2, 250), (0, 60, 70)], 77) + [(nd, None)] * 4
    return with_failures(_related_store(tab, [fam])), [nd]


@functools.lru_cache(maxsize=None)
def splitters_fixture():
    """_mixed_store's 300 records and 64 splitters from its own texts, sorted."""
    st = _mixed_store()
    texts = sorted(t for _, _, t in judged(st))
    return st, [texts[(i * len(texts)) // 64] for i in range(64)]


FIXTURES = {**{f"symbol_order_{k}{'_swapped' * s}": functools.partial(symbol_order_fixture, k, bool(s)) for k in range(6) for s in (0, 1)}, "first_difference": first_difference_fixture,
            **{f"relations_{k}": functools.partial(relations_fixture, k) for k in (0, 1, 2, 5, 8)},
            **{f"relations_2bit_{nd.decode()}": functools.partial(relations_2bit_fixture, nd) for nd in RELATIONS_2BIT}, "empty_needle": empty_needle_fixture,
            **{f"uncoded_{which}_{where}": functools.partial(uncoded_fixture, which, where) for which in ("below", "above") for where in ("first", "middle", "last")},
            "ladder_short": functools.partial(ladder_fixture, "short"), "ladder_long": functools.partial(ladder_fixture, "long"), "ladder_cut": functools.partial(ladder_fixture, "cut"),
            **{f"tiles_{n}": functools.partial(tiles_fixture, n) for n in (1, TILE - 1, TILE, TILE + 1)}, "operators": operators_fixture}


# --- 1. every fixture under the four operators: symbol order against code order, prefix relations, cut and raw records, needle bytes
#        without a code, 32-bit codewords, tile edges ----------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(set(FIXTURES) - {"first_difference", "operators"}))
def test_the_four_operators_on_every_fixture(ctx, name):
    st, needles = FIXTURES[name]()
    all_modes(ctx, st, needles)


# --- 2. where the first difference lies ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shift", range(8))
def test_first_difference_at_every_edge_and_body_alignment(ctx, shift):
    import torch

    st, needles = first_difference_fixture()
    raw = torch.full((shift + st.bodies.size + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    raw[shift : shift + st.bodies.size] = torch.from_numpy(st.bodies.copy()).cuda()
    assert raw.data_ptr() % 16 == 0
    dev = (raw[shift : shift + st.bodies.size], _dev_index(st.body_index), _dev_index(st.text_index))
    for needle in needles:
        for mode in (ORDER_MODES if shift in (0, 5) else (LESS, LESS_EQUAL | NOT)):
            order(ctx, st, needle, mode, dev=dev)


# --- 3. the documented difference ---------------------------------------------------------------------------------------------------


def test_a_body_cut_behind_the_needle_is_less_equal_and_not_equal(ctx):
    """Its stored text is the needle, so LESS_EQUAL selects it and LESS does not; ET_MATCH_EQUAL, which asks for length_b == needle_len,
    rejects it."""
    st, (nd,) = relations_fixture(2)
    status, length, text = judged(st)[CUT_BEHIND]
    assert (status, length, text) == (OK, len(nd) + 1, nd)
    dev = upload(st)
    assert CUT_BEHIND in order(ctx, st, nd, LESS_EQUAL, dev=dev).rows.tolist() and CUT_BEHIND not in order(ctx, st, nd, LESS, dev=dev).rows.tolist()
    want = want_match(st, nd, EQUAL)
    r = run_match(ctx, st.cb, dev, st.n, nd, EQUAL, len(want))
    assert want and CUT_BEHIND not in want and (r.res.status, r.res.n_match, r.rows[: len(want)].tolist()) == (OK, len(want), want)


# --- 4. needle bytes without a code: pattern_bits, and EQUAL / PREFIX keep their rule ---------------------------------------------------


@pytest.mark.parametrize("which", ["below", "above"])
def test_pattern_bits_of_a_needle_with_a_byte_without_a_code(ctx, which):
    for where, bits in (("first", [0, 0]), ("middle", [16]), ("last", [40, 40])):
        st, needles = uncoded_fixture(which, where)
        assert [codable_bits(st.tab, nd) for nd in needles] == bits
    r = run_match(ctx, st.cb, upload(st), st.n, needles[0], PREFIX, 0)  # EQUAL and PREFIX keep their rule: nothing matches, pattern_bits is 0
    assert (r.res.status, r.res.n_match, r.res.pattern_bits) == (OK, 0, 0)


# --- 5. 32-bit codewords ------------------------------------------------------------------------------------------------------------


def test_the_longest_pattern_and_a_needle_too_long(ctx):
    st, needles = ladder_fixture("long")
    assert codable_bits(st.tab, needles[0]) == 1 << 17 and len(needles[0]) == 4096
    r = run_match(ctx, st.cb, upload(st), st.n, needles[0] + b"\x83", LESS, st.n)
    assert r.res.status == ARG and bool((r.rows == ROW_SENTINEL).all()) and bool((r.status == 0xEE).all())


# --- 6. a store that wraps the tile grid --------------------------------------------------------------------------------------------


def test_a_store_that_wraps_the_tile_grid(ctx):
    import torch

    bodies, body_index, lengths, kind, _ = wrap_store()
    dev = (torch.from_numpy(bodies.copy()).cuda(), _dev_index(body_index), _dev_index(_index_of(lengths)))
    cb = _store(table_2bit(), [b"A"]).cb
    d_rows = torch.full((WRAP_N + TAIL,), -1, dtype=torch.int32, device="cuda")
    below = (kind == WRAP_BELOW) | (kind == WRAP_PREFIX) | (kind == WRAP_RAW)
    for mode, want in ((LESS, below), (LESS_EQUAL, below | (kind == WRAP_EQUAL)), (LESS_EQUAL | NOT, kind == WRAP_ABOVE)):
        want = np.flatnonzero(want)
        assert 0 < want.size < WRAP_N
        d_rows.fill_(-1)
        r = ctx.match_packed_device(cb, *dev, WRAP_NEEDLE, mode, rows=d_rows[: want.size])
        torch.cuda.synchronize()
        assert (r.status, r.n_match, r.n_failed) == (OK, want.size, 0)
        got = d_rows.cpu().numpy()
        assert np.array_equal(got[: want.size], want.astype(np.int32)) and bool((got[want.size :] == -1).all())


# --- 7. the four operators, failures ------------------------------------------------------------------------------------------------


def test_the_four_operators_partition_the_valid_records(ctx):
    st, (nd,) = operators_fixture()
    wants = judged(st)
    valid = [b for b, (s, _, _) in enumerate(wants) if not s]
    assert [b for b in range(st.n) if b not in valid] == list(range(st.n - 4, st.n))
    dev = upload(st, spare=st.bodies.size)  # (what lies behind body_bytes is mapped; 2^63 is not: a pair that is followed faults or shows)
    rows = {}
    for mode in ORDER_MODES:
        r = order(ctx, st, nd, mode, dev=dev)
        assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (4, st.n - 4, ARG)
        rows[mode] = r.rows[: r.res.n_match].tolist()
    assert sorted(rows[LESS] + rows[LESS | NOT]) == valid and sorted(rows[LESS_EQUAL] + rows[LESS_EQUAL | NOT]) == valid
    equal = {b for b in valid if wants[b][2] == nd}
    assert set(rows[LESS]) <= set(rows[LESS_EQUAL]) and set(rows[LESS_EQUAL]) - set(rows[LESS]) == equal and len(equal) >= 3
    assert rows[LESS] and rows[LESS_EQUAL | NOT]


# --- 8. capacity and count only -----------------------------------------------------------------------------------------------------


def test_capacity_and_count_only(ctx):
    st, (needle,) = operators_fixture()
    wants, mode = judged(st), LESS_EQUAL
    dev = upload(st, spare=st.bodies.size)
    need = len(select_order(wants, needle, mode))
    assert 3 < need < st.n - 4
    short = run_match(ctx, st.cb, dev, st.n, needle, mode, need - 1)
    check_order(short, wants, needle, mode, call_status=CAP)
    check_order(run_match(ctx, st.cb, dev, st.n, needle, mode, 0), wants, needle, mode, call_status=CAP)
    exact = run_match(ctx, st.cb, dev, st.n, needle, mode, need)
    check_order(exact, wants, needle, mode)
    count = run_match(ctx, st.cb, dev, st.n, needle, mode, need, count_only=True)
    check_order(count, wants, needle, mode)
    assert count.res == exact.res and np.array_equal(count.status, exact.status) and np.array_equal(short.status, exact.status)
    assert dict(vars(short.res), status=OK) == vars(exact.res)


# --- 9. order as a whole ------------------------------------------------------------------------------------------------------------


def test_counts_of_sorted_splitters_are_bisect_left(ctx):
    st, splitters = splitters_fixture()
    texts = sorted(t for _, _, t in judged(st))
    dev = upload(st)
    counts = [ctx.match_packed_device(st.cb, *dev, s, LESS).n_match for s in splitters]
    assert counts == [bisect.bisect_left(texts, s) for s in splitters]
    assert counts == sorted(counts) and counts[0] == 0 and counts[-1] > st.n // 2


# --- 10. chains on one ctx ----------------------------------------------------------------------------------------------------------


def test_between_through_take_then_gather_with_no_synchronisation(ctx):
    """match(NOT | LESS, lo) -> take -> match(LESS_EQUAL, hi) on the taken store -> gather, nothing in between: lo <= t <= hi."""
    import torch

    st, splitters = splitters_fixture()
    lo, hi = splitters[20], splitters[45]
    texts = [t for _, _, t in judged(st)]
    first = [b for b, t in enumerate(texts) if t >= lo]
    second = [k for k, b in enumerate(first) if texts[b] <= hi]
    want = [first[k] for k in second]
    assert want == [b for b, t in enumerate(texts) if lo <= t <= hi] and 20 < len(want) < len(first) < st.n
    dev = upload(st)
    i32 = dict(dtype=torch.int32, device="cuda")
    d_rows, d_rows2 = torch.full((st.n,), -1, **i32), torch.full((st.n,), -1, **i32)
    d_taken = torch.full((st.bodies.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_tb, d_tt = (torch.full((len(first) + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    total = sum(len(texts[b]) for b in want)
    d_out = torch.full((total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_index = torch.full((len(want) + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m1 = ctx.match_packed_device(st.cb, *dev, lo, LESS | NOT, rows=d_rows)
    t = ctx.take_packed_device(*dev, d_rows[: m1.n_match], d_taken[: st.bodies.size], d_tb, d_tt)
    m2 = ctx.match_packed_device(st.cb, d_taken[: t.out_bytes], d_tb, d_tt, hi, LESS_EQUAL, rows=d_rows2)
    g = ctx.decode_packed_gather_device(st.cb, d_taken[: t.out_bytes], d_tb, d_tt, d_rows2[: m2.n_match], d_out[:total], d_index)
    torch.cuda.synchronize()
    assert (m1.status, m1.n_match, t.status, t.n_failed, m2.status, m2.n_match, g.status, g.n_failed, g.n_short) == (OK, len(first), OK, 0, OK, len(second), OK, 0, 0)
    assert d_rows[: len(first)].tolist() == first and d_rows2[: len(second)].tolist() == second
    assert [first[k] for k in d_rows2[: len(second)].tolist()] == want
    host = d_out.cpu().numpy()
    assert host[:total].tobytes() == b"".join(texts[b] for b in want) and bool((host[total:] == SENTINEL).all())


def test_equal_and_prefix_calls_around_a_less_call_on_one_ctx(ctx):
    """The workspace layouts differ: EQUAL and PREFIX calls before and behind a LESS call give what they give alone."""
    import torch

    st, (long,) = ladder_fixture("long")
    other = long[:999] + b"\x64"
    dev = upload(st)
    plan = [(long[:1000], PREFIX), (long, LESS), (long[:1000], PREFIX), (long[:1000], EQUAL), (other, LESS_EQUAL | NOT), (long, EQUAL), (long[:1000], LESS), (long[:2], PREFIX)]
    wants = [want_match(st, nd, mode) if mode & ~NOT in (EQUAL, PREFIX) else want_order(st, nd, mode) for nd, mode in plan]
    rows = [torch.full((len(w) + TAIL,), -1, dtype=torch.int32, device="cuda") for w in wants]
    torch.cuda.synchronize()
    res = [ctx.match_packed_device(st.cb, *dev, nd, mode, rows=d[: len(w)]) for (nd, mode), w, d in zip(plan, wants, rows)]
    torch.cuda.synchronize()
    for r, w, d in zip(res, wants, rows):
        assert (r.status, r.n_match, r.n_failed) == (OK, len(w), 0)
        assert d[: len(w)].tolist() == w and bool((d[len(w) :] == -1).all())
    assert wants[0] == wants[2] and wants[0] and wants[3] and wants[5]


# --- 11. the list helper ------------------------------------------------------------------------------------------------------------


def test_list_helper_with_the_order_modes(ctx):
    import entreepy_amd as E

    rng = np.random.default_rng(0x0DE400E0)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "res", "a_midsummer_nights_dream.txt"), "rb") as f:
        words = f.read().split()[:400]
    strings = [b" ".join(words[i : i + int(rng.integers(0, 4))]) for i in range(0, 396, 2)]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(strings), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, strings)
    lengths = [len(s) for s in strings]
    for needle in (strings[3], sorted(strings)[100], b"", b"zzz", strings[9][:2]):
        assert ctx.match_packed(cb, blob, out_index, lengths, needle, E.MATCH_LESS) == [i for i, s in enumerate(strings) if s < needle]
        assert ctx.match_packed(cb, blob, out_index, lengths, needle, E.MATCH_LESS_EQUAL) == [i for i, s in enumerate(strings) if s <= needle]
        assert ctx.match_packed(cb, blob, out_index, lengths, needle, E.MATCH_LESS | E.MATCH_NOT) == [i for i, s in enumerate(strings) if s >= needle]
        assert ctx.match_packed(cb, blob, out_index, lengths, needle, E.MATCH_LESS_EQUAL | E.MATCH_NOT) == [i for i, s in enumerate(strings) if s > needle]
