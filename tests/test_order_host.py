"""The order modes of et_match_packed_device (ET_MATCH_LESS, ET_MATCH_LESS_EQUAL) as far as they can be checked without a GPU: the
two values declared, bound and exported to the package; the layout of the boundary table; and, in pure Python, the BIT RULE the
kernel implements -- the first differing bit, the needle's codeword boundary at or before it, one codeword decoded there, one byte
comparison -- stated below and checked against Python's `<` on the stores and needles of tests/test_gpu_order.py, with the count of
records that reach each of its branches."""
import collections
import os
import re

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from tests.test_gpu_match import judged
from tests.test_gpu_order import (FIRST_DIFF_BITS, FIXTURES, HEAD_BITS, LESS, LESS_EQUAL, NOT, ORDER_MODES, SYMBOL_LETTERS, WRAP_NEEDLE, WRAP_TEXTS, _midsummer_table, codable_bits,
                                  left_aligned, order_pairs, select_order, splitters_fixture, wrap_store)
from tests.test_shared_host import table_2bit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT, EQ, GT = -1, 0, 1


def test_the_two_modes_are_declared_bound_and_exposed():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    for name, value in (("ET_MATCH_LESS", 4), ("ET_MATCH_LESS_EQUAL", 5)):
        assert re.search(rf"\b{name} = {value}\b", header), name
    assert (N.ET_MATCH_LESS, N.ET_MATCH_LESS_EQUAL) == (4, 5) and (E.MATCH_LESS, E.MATCH_LESS_EQUAL) == (4, 5)
    assert len(N.SIGNATURES["et_match_packed_device"][1]) == 14 and N.lib().et_match_result_size() == 32  # neither changed
    with open(os.path.join(ROOT, "entreepy_amd", "csrc", "et_batch.h")) as f:
        assert "k_order_flag" in f.read()


# --- the boundary table ------------------------------------------------------------------------------------------------------------


def starts_of(tab, needle):
    """-> (starts, K): entry i = (the bit at which the needle's codeword i begins) << 8 | needle[i] for the K leading bytes with a code;
    entry K = pattern_bits << 8 | the first byte without one, or 0."""
    needle = bytes(needle)
    starts, bit, k = [], 0, 0
    while k < len(needle) and int(tab[1][needle[k]]):
        starts.append(bit << 8 | needle[k])
        bit += int(tab[1][needle[k]])
        k += 1
    starts.append(bit << 8 | (needle[k] if k < len(needle) else 0))
    return starts, k


def test_the_boundary_table_is_strictly_increasing_and_fits_32_bits():
    for name in sorted(FIXTURES):
        st, needles = FIXTURES[name]()
        for nd in needles:
            starts, k = starts_of(st.tab, nd)
            assert len(starts) == k + 1 and starts[k] >> 8 == codable_bits(st.tab, nd)
            assert all(a < b for a, b in zip(starts, starts[1:])) and starts[-1] < 1 << 32
            assert [s & 0xFF for s in starts[:k]] == list(nd[:k]) and starts[0] >> 8 == 0
    st, needles = FIXTURES["ladder_long"]()
    starts, k = starts_of(st.tab, needles[0])
    assert k == 4096 and starts[k] == (1 << 17) << 8 and starts[k - 1] >> 8 == (1 << 17) - 32  # the longest there is


# --- the bit rule ------------------------------------------------------------------------------------------------------------------


def _codeword_at(codes, body, at):
    """-> (length, symbol) of the codeword at bit `at` of the body, its bits zero beyond the body's end."""
    bits = 0
    for n in range(1, 33):
        byte = (at + n - 1) >> 3
        bits = bits << 1 | ((body[byte] >> (7 - (at + n - 1) % 8)) & 1 if byte < len(body) else 0)
        if (n, bits) in codes:
            return n, codes[(n, bits)]
    raise AssertionError("the table is not complete")


def rule(tab, codes, body, length, needle):
    """-> (LT | EQ | GT, the branch taken): the record's stored text against the needle, with no text decoded."""
    starts, K = starts_of(tab, needle)
    tail = K < len(needle)
    P, B = starts[K] >> 8, 8 * len(body)
    pattern = E.Codebook.from_tables(*tab).encode_pattern(bytes(needle[:K]))[0]
    m = min(B, P)
    d = next((8 * i + 7 - (body[i] ^ pattern[i]).bit_length() + 1 for i in range((m + 7) // 8) if body[i] != pattern[i]), None)
    if d is not None and d >= m:
        d = None
    if d is not None:
        where = "head" if d < HEAD_BITS else "wave"  # found by the lane alone, or by its wavefront
        i = max(k for k in range(K) if starts[k] >> 8 <= d)
        if i >= length:
            return LT, f"{where}: a difference behind the record's last symbol"
        n, c = _codeword_at(codes, body, starts[i] >> 8)
        if (starts[i] >> 8) + n > B:
            return LT, f"{where}: the deciding codeword is cut"
        assert c != needle[i]
        return (LT, f"{where}: symbol below") if c < needle[i] else (GT, f"{where}: symbol above")
    if B < P:
        return LT, "the body is a prefix of the pattern"
    if length < K:
        return LT, "the length stops inside the needle"
    at_k = (LT, "equal up to a byte without a code") if tail else (EQ, "equal")
    if length == K:
        return at_k
    n, c = _codeword_at(codes, body, P)
    if P + n > B:
        return at_k[0], at_k[1] + ", the next codeword is cut"
    if not tail:
        return GT, "the needle is a proper prefix"
    return (LT, "the next symbol is below the byte without a code") if c < needle[K] else (GT, "the next symbol is above the byte without a code")


def rule_rows(st, needle, mode, tally=None):
    codes = {(int(st.tab[1][s]), int(st.tab[0][s])): s for s in range(256) if int(st.tab[1][s])}
    blob = st.bodies.tobytes()
    out = []
    for b, (status, _, _) in enumerate(judged(st)):
        if status:
            continue
        b0, b1, length = int(st.body_index[b]), int(st.body_index[b + 1]), int(st.text_index[b + 1]) - int(st.text_index[b])
        cmp, branch = rule(st.tab, codes, blob[b0:b1], length, needle)
        if tally is not None:
            tally[branch] += 1
        if (cmp == LT or (mode & ~NOT == LESS_EQUAL and cmp == EQ)) != bool(mode & NOT):
            out.append(b)
    return out


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_bit_rule_selects_what_pythons_comparison_selects(name):
    st, needles = FIXTURES[name]()
    wants = judged(st)
    for needle in needles:
        for mode in ORDER_MODES:
            assert rule_rows(st, needle, mode) == select_order(wants, needle, mode), (needle[:20], mode)


def test_the_bit_rule_on_the_splitters():
    st, splitters = splitters_fixture()
    for needle in splitters[::7]:
        assert rule_rows(st, needle, LESS) == select_order(judged(st), needle, LESS)


# --- the branches the fixtures reach -----------------------------------------------------------------------------------------------
# The rule's branches are the issue's cases, the ordinary one (a symbol against the needle's) split by its outcome and by who found the
# bit, the lane or its wavefront -- nothing finer: the kernel has ONE decode-and-compare, whatever the codeword's index.


def _branches(st, needle):
    tally = collections.Counter()
    rule_rows(st, needle, LESS, tally)
    return tally


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_no_branch_takes_more_than_a_quarter_of_a_stores_records(name):
    """Per call -- one store, one needle, no pooling -- and over ALL the store's records, the failing ones included: a wrong branch
    cannot hide behind a majority.  (Three stores get there only with a quarter of failing records: under the empty needle, or a
    needle that begins with a byte without a code, the rule has three branches.)"""
    st, needles = FIXTURES[name]()
    if name == "tiles_1":  # one record is all of its store whatever branch it takes: the condition cannot be put to a store below four
        assert st.n == 1
        return
    assert st.n >= 16
    for needle in needles:
        tally = _branches(st, needle)
        for branch, count in tally.items():
            assert 4 * count <= st.n, (needle[:20], branch, count, st.n, dict(tally))


def test_the_splitter_store_cannot_meet_the_quarter():
    """The store of GPU cases 9 and 10 (order as a whole, the chain) is a plain store of texts swept by 64 of its own as needles, as the
    issue asks.  Under its lowest splitter every record is at or above the needle, and the rule has four branches for "above": no
    assignment of 300 ordinary texts keeps each under a quarter for all 64 needles.  It is under the rule-against-Python check above
    and deliberately not under the quarter; this test pins that the reason holds, so that nobody takes it for an oversight."""
    st, splitters = splitters_fixture()
    tally = _branches(st, splitters[0])
    assert sum(count for branch, count in tally.items() if "above" in branch or "proper prefix" in branch) > 3 * st.n // 4


def _reached(names):
    total = collections.Counter()
    for name in names:
        st, needles = FIXTURES[name]()
        for needle in needles:
            total += _branches(st, needle)
    return total


def test_the_fixtures_reach_the_cases_the_gpu_tests_name():
    # symbol order against code order: pairs that order both ways, and the stores decide at them in either direction
    tab = _midsummer_table()
    same, other = order_pairs(tab, [s for s in SYMBOL_LETTERS if int(tab[1][s])])
    assert len(same) >= 3 and len(other) >= 3 and all(a < b and left_aligned(tab, a) > left_aligned(tab, b) for a, b in other)
    for k, (a, b) in enumerate(same[:3] + other[:3]):
        (st_a, (nd_a,)), (st_b, (nd_b,)) = FIXTURES[f"symbol_order_{k}"](), FIXTURES[f"symbol_order_{k}_swapped"]()
        j = next(i for i in range(len(nd_a)) if nd_a[i] != nd_b[i])
        assert (nd_a[j], nd_b[j]) == (a, b)
        # against nd_a a record has b where the needle has a -- above by bytes, whatever the bits say -- against nd_b the other way round
        assert nd_b in [t for _, _, t in judged(st_a)] and nd_a in [t for _, _, t in judged(st_b)]
        assert _branches(st_a, nd_a)["head: symbol above"] >= 3 and _branches(st_b, nd_b)["head: symbol below"] >= 3
    # where the first difference lies: found by the lane and by the wavefront, at the named bits
    first = _reached(["first_difference"])
    for branch in ("head: symbol below", "head: symbol above", "wave: symbol below", "wave: symbol above"):
        assert first[branch] >= 4, (branch, dict(first))
    assert {63, 64, 65, 95, 96, 97, 2079, 2080, 2081, 2111, 2112, 2113} <= set(FIRST_DIFF_BITS) and {8 * k + e for k in range(21) for e in range(8 if k == 0 else 1)} <= set(FIRST_DIFF_BITS)
    st, (nd,) = FIXTURES["first_difference"]()
    assert codable_bits(st.tab, nd) % 8 == 7  # the pattern's last byte is partial
    # prefix relations, cut and raw records, under every table
    families = {"relations": [f"relations_{k}" for k in (0, 1, 2, 5, 8)], "relations_2bit": [n for n in FIXTURES if n.startswith("relations_2bit")],
                "symbol_order": [n for n in FIXTURES if n.startswith("symbol_order")], "ladder": ["ladder_short", "ladder_long", "ladder_cut"]}
    for family, names in families.items():
        r = _reached(names)
        for branch in ("equal", "equal, the next codeword is cut", "the needle is a proper prefix", "the body is a prefix of the pattern", "the length stops inside the needle",
                       "head: a difference behind the record's last symbol", "head: symbol below", "head: symbol above"):
            if family == "ladder" and branch.startswith("head: a difference behind"):  # (a body of 32-bit codewords has no pad bits)
                continue
            assert r[branch] > 0, (family, branch, dict(r))
    assert _reached(families["relations"])["head: the deciding codeword is cut"] or _reached(families["symbol_order"])["head: the deciding codeword is cut"]
    ladder = _reached(["ladder_long", "ladder_cut"])
    assert ladder["wave: symbol below"] and ladder["wave: symbol above"] and ladder["wave: the deciding codeword is cut"]
    empty = _reached(["empty_needle"])
    assert set(empty) == {"equal", "equal, the next codeword is cut", "the needle is a proper prefix"}
    # needle bytes without a code: below and above the record's next symbol, at the first place, in the middle and last
    for which, reaches, never in (("below", "above", "below"), ("above", "below", "above")):
        for where in ("first", "middle", "last"):
            r = _reached([f"uncoded_{which}_{where}"])
            assert r[f"the next symbol is {reaches} the byte without a code"] and not r[f"the next symbol is {never} the byte without a code"]
            assert r["equal up to a byte without a code"] and r["equal up to a byte without a code, the next codeword is cut"]
            if where != "first":
                assert r["the length stops inside the needle"] and r["the body is a prefix of the pattern"] and r["head: symbol below"] and r["head: symbol above"]


def test_the_pad_bits_decide_nothing():
    """Hand-made bodies whose pad bits differ from the needle and read as a symbol ABOVE needle[i]: still a proper prefix, LESS."""
    tab = table_2bit()
    codes = {(2, c): s for c, s in enumerate(b"ACGT")}
    for body, length, needle in ((bytes([0b10110000]), 1, b"GC"), (bytes([0b01101111]), 2, b"CGGA"), (bytes([0b10110000]), 1, b"GA")):
        cmp, branch = rule(tab, codes, body, length, needle)
        assert (cmp, branch) == (LT, "head: a difference behind the record's last symbol")
        n, c = _codeword_at(codes, body, 2 * length)
        assert c > needle[length]  # what decoding the pad would say
    st, _ = FIXTURES["relations_2bit_GC"]()
    assert bytes([0b10110000]) in [st.bodies[int(a) : int(b)].tobytes() for a, b in zip(st.body_index[:-1], st.body_index[1:])]


def test_the_wrapping_store_has_a_fifth_of_its_records_in_each_relation():
    bodies, body_index, lengths, kind, which = wrap_store()
    tab = table_2bit()
    codes = {(2, c): s for c, s in enumerate(b"ACGT")}
    want = {0: (LT, "head: symbol below"), 1: (GT, "head: symbol above"), 2: (EQ, "equal"), 3: (LT, "head: a difference behind the record's last symbol"),
            4: (LT, "the body is a prefix of the pattern")}
    for b in range(0, 4000, 13):  # the rule and Python's comparison on a sample: kind says which relation, and so which branch
        body = bodies[int(body_index[b]) : int(body_index[b + 1])].tobytes()
        text = WRAP_TEXTS[kind[b]][which[b]]
        assert int(lengths[b]) == len(text) and rule(tab, codes, body, len(text), WRAP_NEEDLE) == want[int(kind[b])]
        stored = text if body else b""
        assert ((stored > WRAP_NEEDLE) - (stored < WRAP_NEEDLE)) == want[int(kind[b])][0]
    for k in range(5):
        assert 0 < int((kind == k).sum()) <= kind.size // 4

