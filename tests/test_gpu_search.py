"""GPU: et_search_packed_device -- which records of a packed store contain a needle, or end with it, and where, found on the
compressed bytes by a walk over the codeword boundaries -- against the oracle: a record's status is judged from its own two pairs of
offsets (tests/test_gpu_gather.py's want_rows), its text is want_decode's, and the expected rows and positions are Python's `in`,
find and endswith over those texts; never the bit rule the kernels implement.  d_rows and d_pos (cap_rows + TAIL entries each) and
d_status are filled with sentinels first; everything behind n_match must still hold them.

The stores and needles are made by the *_fixture functions below, without a GPU: tests/test_search_host.py checks on the same
fixtures that the bit rule selects what the texts select, and that they reach the cases named here."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import bitwalk
from tests.test_gpu_batch import SENTINEL, _u8
from tests.test_gpu_gather import upload
from tests.test_gpu_match import (ROW_SENTINEL, TILE, _pack, _res_files, _store, alignment_fixture as match_alignment_fixture, bit_edges_fixture, failures_fixture, judged,
                                  pattern_bits, tiles_fixture, tiny_fixture)
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_gpu_shared import _cb, _family, want_decode
from tests.test_gpu_take import _guards_intact, _taken
from tests.test_shared_host import oracle_table, table_255, table_2bit, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
CONTAINS, SUFFIX, NOT = 0, 1, 0x100  # ET_SEARCH_*, ET_MATCH_NOT
MODES = [CONTAINS, SUFFIX, CONTAINS | NOT, SUFFIX | NOT]
LANE_BITS = 256  # what a lane of the workgroup path owns of a block (csrc/et_batch.hip decode_stream)
BLOCK_BITS = 65536  # the 8 KiB block the workgroup path stages


def lane_bytes():
    """Bodies up to this many bytes are walked by one lane, longer ones by a workgroup (no GPU needed to ask)."""
    from entreepy_amd import _native as N

    return int(N.lib().et_search_lane_bytes())


# --- the expected rows and positions: the oracle's texts, Python's comparison ------------------------------------------------------


def select(wants, needle, mode):
    """-> (rows, positions): positions are None under NOT."""
    needle, rows, pos = bytes(needle), [], []
    for b, (status, length, text) in enumerate(wants):
        if status:
            continue
        if mode & SUFFIX:
            hit, at = len(text) == length and text.endswith(needle), length - len(needle)
        else:
            hit, at = needle in text, text.find(needle)
        if hit != bool(mode & NOT):
            rows.append(b)
            pos.append(at if hit else None)
    return rows, pos


def want_search(st, needle, mode):
    return select(judged(st), needle, mode)


# --- one call ----------------------------------------------------------------------------------------------------------------------


def run_search(ctx, cb, dev, n, needle, mode, cap, count_only=False, with_pos=True):
    """One call through the C ABI (a capacity of zero is still a pointer), every output full of sentinels first."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    d_bodies, d_body_index, d_text_index = dev
    needle = bytes(needle)
    r = SimpleNamespace(cap=cap, count_only=count_only, with_pos=with_pos and not count_only and not mode & NOT)
    r.d_rows, r.d_pos = (torch.full((4 * (cap + TAIL),), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.int32) for _ in range(2))
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = N.MatchResult()
    rc = N.lib().et_search_packed_device(ctx._h, ctypes.byref(cb.raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), n, needle, len(needle),
                                         mode, None if count_only else r.d_rows.data_ptr(), cap, r.d_pos.data_ptr() if r.with_pos else None, r.d_status.data_ptr(), ctypes.byref(res))
    torch.cuda.synchronize()
    r.res = E.MatchResult(rc, res.n_match, res.n_failed, res.first_failed, res.first_status, res.pattern_bits)
    r.rows, r.pos, r.status = r.d_rows.cpu().numpy().view(np.uint32), r.d_pos.cpu().numpy().view(np.uint32), r.d_status.cpu().numpy()
    return r


def check_search(r, wants, needle, mode, call_status=OK, pattern_bits=None):
    want, want_pos = select(wants, needle, mode)
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
        assert bool((r.pos == ROW_SENTINEL).all()), "an entry of d_pos was written"
        return want
    got = r.rows[: len(want)].tolist()
    assert got == want, f"the rows differ from the oracle's, first at {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"
    assert bool((r.rows[len(want) :] == ROW_SENTINEL).all()), "an entry at or behind d_rows + n_match was written"
    if r.with_pos:
        got = r.pos[: len(want)].tolist()
        assert got == want_pos, f"the positions differ from Python's, first at row {next(i for i, (a, b) in enumerate(zip(got, want_pos)) if a != b)}"
        assert bool((r.pos[len(want) :] == ROW_SENTINEL).all()), "an entry at or behind d_pos + n_match was written"
    else:
        assert bool((r.pos == ROW_SENTINEL).all()), "d_pos was not handed in, and written"
    return want


def search(ctx, st, needle, mode, dev=None, **kw):
    """Run with cap_rows = the need exactly, and check."""
    need = len(want_search(st, needle, mode)[0])
    r = run_search(ctx, st.cb, dev or upload(st), st.n, needle, mode, need)
    check_search(r, judged(st), needle, mode, **kw)
    return r


def search_all_modes(ctx, st, needles, dev=None, modes=MODES):
    dev = dev or upload(st)
    for needle in needles:
        for mode in modes:
            search(ctx, st, needle, mode, dev=dev, pattern_bits=pattern_bits(st.tab, needle))


# --- the fixtures: (store, needles), made without a GPU -----------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _midsummer():
    """(the play's bytes with its rarest byte -- one 17-bit codeword -- replaced by a space, the table of the ORIGINAL bytes, that byte)."""
    text = np.frombuffer(_res_files()["a_midsummer_nights_dream.txt"], np.uint8)
    tab = oracle_table(text)
    rare = ord("_")
    assert int(tab[1][rare]) == 17 and int(np.count_nonzero(text == rare)) == 1
    return np.where(text == rare, 32, text).astype(np.uint8), tab, rare


def bit_string(body, n_bits=None):
    s = "".join(format(b, "08b") for b in bytes(body))
    return s if n_bits is None else s[:n_bits]


def bits_of(tab, text):
    return int(tab[1][_u8(text)].astype(np.int64).sum())


@functools.lru_cache(maxsize=None)
def no_boundary_fixture(which):
    """Records in whose bodies the needle's bits occur, and at no codeword boundary, on both sides of the lane-path threshold.
    "2bit": C = 01, G = 10: CCCC... holds G's bits at every odd bit.  "text": a needle found by search, here on the host."""
    if which == "2bit":
        tab = table_2bit()
        assert (int(tab[0][ord("C")]), int(tab[0][ord("G")])) == (1, 2)
        texts = [b"C" * k for k in (1, 2, 3, 4, 5, 40, 41, 600, 2000, 40_000)] + [b"CCGCC", b"C" * 700 + b"G", b"G" + b"C" * 700, b"C" * 39_000 + b"GG" + b"C" * 50]
        return _store(tab, texts), [b"G", b"GG", b"GC"]
    pool, tab, _ = _midsummer()
    coded = [int(s) for s in np.flatnonzero(tab[1]) if 3 < int(tab[1][s]) <= 9]
    texts, needles = [], []
    for size, start in ((50, 2000), (3000, 9000)):
        text = pool[start : start + size].tobytes()
        body_bits = bit_string(_pack(tab, text), bits_of(tab, text))
        found = None
        for a in coded:
            for b in coded:
                nd = bytes([a, b])
                if nd not in text and bit_string(_pack(tab, nd), bits_of(tab, nd)) in body_bits:
                    found = nd
                    break
            if found:
                break
        assert found, "no pair of symbols has its bits in this body off the boundaries alone"
        texts += [text, text + found]
        needles.append(found)
    return _store(tab, texts), needles


@functools.lru_cache(maxsize=None)
def pad_fixture(which):
    """Records followed by pad bits that read as the needle: the all-zero codeword's symbol -- table_255: byte 1, 7 zeros, behind a
    record with a whole byte of pad; the ladder: byte 100, one zero, in any pad -- so the occurrence lies behind the record's length."""
    if which == "table_255":
        tab, zero = table_255(), 1
        stems = [bytes([65, 200]), (bytes(range(2, 252)) * 4)[: lane_bytes() + 200]]  # 2 bytes of body, and 200 above the lane path's
        texts, bodies = [], []
        for stem in stems:
            texts += [stem, stem, stem + bytes([zero]), stem]
            bodies += [_pack(tab, stem) + b"\0", _pack(tab, stem) + b"\0\0\0", _pack(tab, stem + bytes([zero])), _pack(tab, stem)]
        needles = [bytes([zero]), bytes([zero]) * 2, stems[0][-1:] + bytes([zero]), stems[1][-1:] + bytes([zero])]
    else:
        tab, zero = table_ladder(), 100
        assert (int(tab[0][zero]), int(tab[1][zero])) == (0, 1)
        stems = [bytes([101, 102]), bytes([101, 102, 103, 104] * 60)]  # 5 bits -> 3 pad bits; 840 bits = 105 bytes, no pad
        stems.append(stems[1] * (lane_bytes() // 105 + 1) + bytes([101]))  # k x 840 + 2 bits: 6 pad bits, above the lane path's bodies
        texts, bodies = [], []
        for stem in stems:
            texts += [stem, stem + bytes([zero]), stem]
            bodies += [_pack(tab, stem), _pack(tab, stem + bytes([zero])), _pack(tab, stem) + b"\0"]
        needles = [bytes([zero]), bytes([zero]) * 3, bytes([102, zero]), bytes([101, zero])]
    return _store(tab, texts, bodies), needles


@functools.lru_cache(maxsize=None)
def first_fixture():
    """The first of several occurrences; a head that passes where the rest does not; needles as long as the record and one longer --
    short, and behind 1 500 bytes of filler (the workgroup path; whole_fixture has its needles as long as a record)."""
    pool, tab, _ = _midsummer()
    filler = pool[31_000:32_500].tobytes()
    assert b"aa" not in filler and b"abab" not in filler and filler[-1:] not in b"ab"
    texts = []
    for lead in (b"", filler):
        texts += [lead + b"aaaa", lead + b"abababc", lead + b"ababc", lead + b"abab", lead + b"xaay", lead + b"aa", lead + b"a"]
    needles = [b"aa", b"ababc", b"abababc", b"abababcd", b"aaaa", b"aaaaa", filler[-200:] + b"aaaa"]
    st = _store(tab, texts)
    assert want_search(st, b"aa", CONTAINS) == ([0, 4, 5, 7, 11, 12], [0, 1, 0, 1500, 1501, 1500])
    assert want_search(st, b"ababc", CONTAINS) == ([1, 2, 8, 9], [2, 0, 1502, 1500])
    assert int(np.diff(st.body_index.astype(np.int64))[7:].min()) > lane_bytes()
    return st, needles


@functools.lru_cache(maxsize=None)
def whole_fixture():
    """Needles as long as a record, and one longer, on the workgroup path: 200 symbols of the ladder's two 32-bit codewords are 800
    bytes of body and still a needle."""
    tab = table_ladder()
    assert int(tab[1][131]) == 32 and int(tab[1][132]) == 32 and 200 * 4 > lane_bytes()
    base = (131 + np.random.default_rng(0x5EA2C420).integers(0, 2, size=201)).astype(np.uint8).tobytes()
    texts = [base[:200], base[:199], base, base[1:], b"\x64" + base[:200], base[:100] + b"\x64" + base[100:200]]
    return _store(tab, texts), [base[:200], base, base[1:], base[:199]]


def _planted(base, needle, at):
    text = base.copy()
    text[at : at + len(needle)] = _u8(needle)
    return text


@functools.lru_cache(maxsize=None)
def edges_fixture():
    """One needle planted per record, in text records of 64 bytes (every position: the lane path) and of about 17 KiB of BODY (three
    blocks of the workgroup path), so that it begins in the last codeword of a lane's 256 bits, straddles bit 65 536 of the body,
    lies wholly in the last block, or is the record's last symbols; and records whose bodies are et_search_lane_bytes() - 1, exactly
    that, and + 1 bytes.  Needles of 1, 12 and 256 bytes -- and 256 bytes of 3-bit codewords, which fit a lane's body.
    -> (store, needles, where): where[record] = (needle, symbol, case)."""
    pool, tab, rare = _midsummer()
    lane = lane_bytes()
    n1, n12, n256 = bytes([rare]), pool[7000:7011].tobytes() + bytes([rare]), bytes([rare]) + pool[5000:5255].tobytes()
    n256s = bytes(np.where(np.random.default_rng(0x5EA2C401).random(256) < 0.5, ord(" "), ord("e")).astype(np.uint8))
    assert bits_of(tab, n256s) == 768 and [len(x) for x in (n1, n12, n256)] == [1, 12, 256]
    texts, where, offset = [], {}, 0

    def add(text, note=None):
        nonlocal offset
        if note:
            assert text.tobytes().find(note[0]) == note[1], note
            where[len(texts)] = note
        texts.append(text)
        offset += len(_pack(tab, text))

    # the lane path: 64 bytes of text, the needle at every position
    short = pool[12_000:12_064]
    for nd in (n1, n12):
        for at in range(0, 65 - len(nd)):
            add(_planted(short, nd, at), (nd, at, "short"))
    add(np.concatenate((_u8(b"xy "), _u8(n256s), _u8(b"z"))), (n256s, 3, "short"))
    add(np.concatenate((_u8(b"x"), _u8(n256s))), (n256s, 1, "short_suffix"))
    assert all(len(_pack(tab, t)) <= lane for t in texts)
    # the threshold: bodies of lane - 1, lane, lane + 1 bytes that end with n12
    for target in (lane - 1, lane, lane + 1):
        stem = pool[40_000:42_000]
        bits = np.cumsum(tab[1][stem].astype(np.int64)) + bits_of(tab, n12)
        k = int(np.flatnonzero((bits + 7) // 8 == target)[0]) + 1
        add(np.concatenate((stem[:k], _u8(n12))), (n12, k, f"body_{target - lane:+d}"))
        assert len(_pack(tab, texts[-1])) == target
    # the workgroup path: about 17 KiB of body, three blocks
    n_long = 30_500
    for j, nd in enumerate((n1, n12, n256)):
        for case in ("lane_edge", "block_edge", "last_block", "suffix"):
            base = pool[1000 + 977 * (4 * j + len(texts) % 4) :][:n_long]
            bounds = bitwalk.boundaries((offset % 4) * 8, tab[1], base)
            bits = bits_of(tab, nd)
            if case == "lane_edge":  # codeword `at` begins in a lane's bits and ends behind them
                at = int(next(i for i in range(200, n_long) if int(bounds[i]) % LANE_BITS + int(tab[1][nd[0]]) > LANE_BITS))
            elif case == "block_edge":
                hits = np.flatnonzero((bounds < BLOCK_BITS) & (bounds + bits > BLOCK_BITS))
                at = int(hits[hits.size // 2])
            elif case == "last_block":
                at = int(np.flatnonzero(bounds >= 2 * BLOCK_BITS + 100)[0])
                assert at + len(nd) < n_long - 100
            else:
                at = n_long - len(nd)
            add(_planted(base, nd, at), (nd, at, case))
            body = len(_pack(tab, texts[-1]))
            assert 2 * BLOCK_BITS // 8 + 4 < body < 3 * BLOCK_BITS // 8, body
    return _store(tab, texts), [n1, n12, n256, n256s], where


SLOW = {"2bit": 40_000, "uniform255": 10_000, "zeros90": 60_000, "ladder32": 40_000}  # symbols: more than 8 KiB of body each


@functools.lru_cache(maxsize=None)
def slow_fixture(name):
    """Records above 8 KiB under codes that synchronise slowly or never (the lanes' entries settle over many trips of the fixed point),
    and a small one; the needles are 12-byte slices of record 0 -- at its start, across bit 65 536, in the middle, at its end --
    and each with one byte changed."""
    tab, draw = _family(name, _res_files())
    n = SLOW[name]
    texts = [draw(n, 0x5EA2C410), draw(n + 777, 0x5EA2C411), draw(150, 0x5EA2C412)]
    st = _store(tab, texts)
    assert int(st.body_index[1]) > 8192 and int(st.body_index[2] - st.body_index[1]) > 8192
    bounds = bitwalk.boundaries(0, tab[1], texts[0])
    across = int(np.searchsorted(bounds, BLOCK_BITS)) - 4
    assert bounds[across] < BLOCK_BITS < bounds[across + 12]
    coded = np.flatnonzero(tab[1])
    needles = []
    for at in (3, across, n // 2, n - 12):
        nd = texts[0][at : at + 12].copy()
        needles.append(nd.tobytes())
        nd[6] = coded[(int(np.searchsorted(coded, nd[6])) + 1) % coded.size]
        needles.append(nd.tobytes())
    return st, needles


@functools.lru_cache(maxsize=None)
def cut_fixture():
    """Bodies cut before their length, and empty bodies under a length above zero, on both paths: CONTAINS is judged on what is
    there, a needle across the cut does not match, SUFFIX never matches."""
    pool, tab, _ = _midsummer()
    texts, bodies, needles = [], [], []
    for size, start in ((60, 50_000), (4000, 60_000)):
        text = pool[start : start + size].tobytes()
        body = _pack(tab, text)
        cut = body[: len(body) // 2]
        assert (len(cut) > lane_bytes()) == (size > 60)
        kept = len(want_decode(tab, cut, size)[1])  # symbols that end inside the cut body
        assert 4 < kept < size - 4
        texts += [text, text, text, text[:kept]]
        bodies += [body, cut, b"", cut]
        needles += [text[kept - 4 : kept], text[kept - 2 : kept + 2], text[kept : kept + 4], text[-4:], text[:3]]
    return _store(tab, texts, bodies), needles + [b""]


@functools.lru_cache(maxsize=None)
def alignment_fixture():
    """The match's alignment fixture's records (0 .. 200 bytes of text back to back: every start alignment, the lane path) and, for
    the workgroup path, 48 more made of sixteen of them each."""
    base, _ = match_alignment_fixture()
    texts = [t for _, _, t in judged(base)]
    texts += [b"".join(texts[(7 * i + k) % 256] for k in range(16)) for i in range(48)]
    st = _store(base.tab, texts)
    sizes = np.diff(st.body_index.astype(np.int64))
    assert int(np.count_nonzero(sizes > lane_bytes())) >= 40 and int(np.count_nonzero((sizes > 0) & (sizes <= lane_bytes()))) >= 200
    long = texts[300]
    return st, [texts[20][5:9], long[-12:], long[200:212], texts[25][-6:], long[100:102]]


@functools.lru_cache(maxsize=None)
def search_tiles_fixture(n):
    st, _ = tiles_fixture(n)  # tiny records over ACGT; the first and the last of every tile begin ACGT
    return st, [b"CGT", b"", b"T" * 20]


@functools.lru_cache(maxsize=None)
def search_tiny_fixture():
    st, (needle,) = tiny_fixture()  # 20 000 records of 0 .. 8 bytes, every third begins with the needle
    return st, [needle]


@functools.lru_cache(maxsize=None)
def search_failures_fixture():
    st, needles = failures_fixture()
    text6 = judged(st)[6][2]
    return st, [text6[40:52], text6[-12:], text6[40:42], b""]


FIXTURES = {"no_boundary_2bit": functools.partial(no_boundary_fixture, "2bit"), "no_boundary_text": functools.partial(no_boundary_fixture, "text"),
            "pad_table_255": functools.partial(pad_fixture, "table_255"), "pad_ladder": functools.partial(pad_fixture, "ladder"), "first": first_fixture, "whole": whole_fixture,
            "bit_edges": bit_edges_fixture, "edges": lambda: edges_fixture()[:2], "cut": cut_fixture, "alignment": alignment_fixture, "tiny": search_tiny_fixture,
            "failures": search_failures_fixture, **{f"tiles_{n}": functools.partial(search_tiles_fixture, n) for n in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)},
            **{f"slow_{name}": functools.partial(slow_fixture, name) for name in SLOW}}


# --- 1. no boundary, no match ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["2bit", "text"])
def test_bits_at_no_boundary_are_no_occurrence(ctx, which):
    st, needles = no_boundary_fixture(which)
    search_all_modes(ctx, st, needles)
    if which == "2bit":
        assert want_search(st, b"G", CONTAINS) == ([10, 11, 12, 13], [2, 700, 0, 39_000])
    else:
        assert all(2 * k not in want_search(st, nd, CONTAINS)[0] and 2 * k + 1 in want_search(st, nd, CONTAINS)[0] for k, nd in enumerate(needles))


# --- 2. pad bits -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["table_255", "ladder"])
def test_an_occurrence_in_the_pad_bits_is_rejected_by_the_length(ctx, which):
    st, needles = pad_fixture(which)
    search_all_modes(ctx, st, needles)
    rows, pos = want_search(st, needles[0], CONTAINS)
    per = 4 if which == "table_255" else 3
    assert rows == [k * per + (2 if which == "table_255" else 1) for k in range(st.n // per)]  # the records that really end with it
    assert want_search(st, needles[0], SUFFIX)[0] == rows


# --- 3. the first occurrence, every end position -----------------------------------------------------------------------------------


def test_the_first_occurrence_and_needles_as_long_as_the_record(ctx):
    st, needles = first_fixture()
    search_all_modes(ctx, st, needles)
    st, needles = whole_fixture()
    search_all_modes(ctx, st, needles)
    assert want_search(st, needles[0], CONTAINS) == ([0, 2, 4], [0, 0, 1]) and want_search(st, needles[0], SUFFIX)[0] == [0, 4]


def test_needles_that_end_at_every_bit_of_a_byte(ctx):
    st, needles = bit_edges_fixture()  # a stem plus k 7-bit symbols; records equal, one symbol longer, cut, with pad and without
    assert sorted(pattern_bits(st.tab, nd) % 8 for nd in needles) == list(range(8))
    search_all_modes(ctx, st, needles + [nd[1:] for nd in needles[:3]])


# --- 4. edges of the walk ----------------------------------------------------------------------------------------------------------


def test_edges_of_the_walk_on_both_paths(ctx):
    st, needles, where = edges_fixture()
    dev = upload(st)
    for needle in needles:
        for mode in (CONTAINS, SUFFIX):
            r = search(ctx, st, needle, mode, dev=dev, pattern_bits=pattern_bits(st.tab, needle))
        rows, pos = want_search(st, needle, CONTAINS)
        planted = {b: at for b, (nd, at, _) in where.items() if nd == needle}
        assert set(planted) <= set(rows) and all(pos[rows.index(b)] == at for b, at in planted.items())
    search(ctx, st, needles[1], CONTAINS | NOT, dev=dev)
    search(ctx, st, needles[2], SUFFIX | NOT, dev=dev)
    assert r.res.pattern_bits == 768


# --- 5. slow synchronisation -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(SLOW))
def test_codes_that_synchronise_slowly(ctx, name):
    st, needles = slow_fixture(name)
    search_all_modes(ctx, st, needles, modes=(CONTAINS, SUFFIX))
    search(ctx, st, needles[2], CONTAINS | NOT)
    assert all(0 in want_search(st, nd, CONTAINS)[0] for nd in needles[::2])
    assert want_search(st, needles[6], SUFFIX)[0] == [0]


# --- 6. short bodies ---------------------------------------------------------------------------------------------------------------


def test_bodies_cut_before_their_length_and_empty_bodies(ctx):
    st, needles = cut_fixture()
    search_all_modes(ctx, st, needles)
    for k in (0, 4):  # per size: [whole, cut, empty body, cut with the length of what is there]
        before, across, behind, end, _ = needles[5 * (k // 4) : 5 * (k // 4) + 5]
        assert {k, k + 1, k + 3} <= set(want_search(st, before, CONTAINS)[0]) and k + 2 not in want_search(st, before, CONTAINS)[0]
        assert k in want_search(st, across, CONTAINS)[0] and not {k + 1, k + 2, k + 3} & set(want_search(st, across, CONTAINS)[0])
        assert want_search(st, end, SUFFIX)[0] == [k] and want_search(st, before, SUFFIX)[0] == [k + 3]
    assert want_search(st, b"", SUFFIX)[0] == [0, 3, 4, 7] and want_search(st, b"", CONTAINS)[0] == list(range(8))


# --- 7. alignment ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_body_alignment_and_base(ctx, shift):
    import torch

    st, needles = alignment_fixture()
    assert {int(b) % 16 for b, e in zip(st.body_index[:-1], st.body_index[1:]) if e > b} == set(range(16))
    raw = torch.zeros(shift + st.bodies.size + 16, dtype=torch.uint8, device="cuda")
    raw[shift : shift + st.bodies.size] = torch.from_numpy(st.bodies.copy()).cuda()
    assert raw.data_ptr() % 16 == 0
    dev = (raw[shift : shift + st.bodies.size], _dev_index(st.body_index), _dev_index(st.text_index))
    search_all_modes(ctx, st, needles, dev=dev, modes=(CONTAINS, SUFFIX))


# --- 8. tiles and scan edges, many tiny records ------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tile_and_scan_edges(ctx, n):
    st, (needle, everything, nothing) = search_tiles_fixture(n)
    dev = upload(st)
    want = want_search(st, needle, CONTAINS)[0]
    for t0 in range(0, n, TILE):
        assert t0 in want and min(t0 + TILE, n) - 1 in want
    for mode in MODES:
        search(ctx, st, needle, mode, dev=dev)
    assert want_search(st, everything, CONTAINS) == (list(range(n)), [0] * n) and want_search(st, nothing, CONTAINS)[0] == []
    search(ctx, st, everything, CONTAINS, dev=dev)
    search(ctx, st, everything, SUFFIX, dev=dev)
    search(ctx, st, nothing, CONTAINS, dev=dev)
    search(ctx, st, nothing, SUFFIX | NOT, dev=dev)


def test_20000_tiny_records_a_third_of_them_matching(ctx):
    st, (needle,) = search_tiny_fixture()
    want = want_search(st, needle, CONTAINS)[0]
    assert 6_600 < len(want) < 6_800 and want == sorted(want)
    dev = upload(st)
    for mode in MODES:
        search(ctx, st, needle, mode, dev=dev)


# --- 9. failures stay local, capacity, count only ----------------------------------------------------------------------------------


def test_failures_stay_local(ctx):
    st, needles = search_failures_fixture()
    wants = judged(st)
    assert [s for s, _, _ in wants] == [OK, OK, OK, ARG, OK, OK, OK, OK, ARG, ARG, OK, ARG, OK, UNSUPPORTED]
    dev = upload(st, spare=st.bodies.size)  # (what lies behind body_bytes is mapped; 2^63 is not: a pair that is followed faults or shows)
    for needle in needles:
        for mode in MODES:
            r = search(ctx, st, needle, mode, dev=dev)
            assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (5, 3, ARG)
    assert want_search(st, b"", CONTAINS | NOT)[0] == [] and want_search(st, b"", CONTAINS)[0] == [0, 1, 2, 4, 5, 6, 7, 10, 12]
    assert 6 in want_search(st, needles[0], CONTAINS)[0] and want_search(st, needles[1], SUFFIX)[0] == [6]


def test_capacity_and_count_only(ctx):
    import torch

    import entreepy_amd as E

    st, needles = search_failures_fixture()
    wants, needle, mode = judged(st), needles[2], CONTAINS
    dev = upload(st, spare=st.bodies.size)
    need = len(select(wants, needle, mode)[0])
    assert need == 4
    short = run_search(ctx, st.cb, dev, st.n, needle, mode, need - 1)
    check_search(short, wants, needle, mode, call_status=CAP)
    check_search(run_search(ctx, st.cb, dev, st.n, needle, mode, 0), wants, needle, mode, call_status=CAP)
    exact = run_search(ctx, st.cb, dev, st.n, needle, mode, need)
    check_search(exact, wants, needle, mode)
    check_search(run_search(ctx, st.cb, dev, st.n, needle, mode, need, with_pos=False), wants, needle, mode)
    count = run_search(ctx, st.cb, dev, st.n, needle, mode, need, count_only=True)
    check_search(count, wants, needle, mode)
    assert count.res == exact.res and np.array_equal(count.status, exact.status) and np.array_equal(short.status, exact.status)
    assert dict(vars(short.res), status=OK) == vars(exact.res)
    check_search(run_search(ctx, st.cb, dev, st.n, needle, mode | NOT, 9 - need - 1), wants, needle, mode | NOT, call_status=CAP)
    # the Python call: rows=None counts, a tensor one entry short reports the need
    d_rows, d_pos = (torch.full((need + TAIL,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    assert ctx.search_packed_device(st.cb, *dev, needle, E.SEARCH_CONTAINS) == exact.res
    r = ctx.search_packed_device(st.cb, *dev, needle, mode, rows=d_rows[: need - 1], pos=d_pos[: need - 1])
    assert (r.status, r.n_match) == (CAP, need)
    r = ctx.search_packed_device(st.cb, *dev, needle, mode, rows=d_rows[:need], pos=d_pos[:need])
    torch.cuda.synchronize()
    rows, pos = select(wants, needle, mode)
    assert r == exact.res and d_rows[:need].tolist() == rows and d_pos[:need].tolist() == pos
    assert bool((d_rows[need:] == -1).all()) and bool((d_pos[need:] == -1).all())


# --- 10. refusals ------------------------------------------------------------------------------------------------------------------


def test_a_needle_byte_without_a_code_matches_nothing(ctx):
    st, needles = search_failures_fixture()
    assert int(st.tab[1][0xFF]) == 0
    dev = upload(st, spare=st.bodies.size)
    for needle in (b"\xff", needles[2] + b"\xff", b"\xff" + needles[2]):
        for mode in MODES:
            r = search(ctx, st, needle, mode, dev=dev, pattern_bits=0)
            assert r.res.n_match == (9 if mode & NOT else 0)


def test_an_incomplete_table_is_refused_with_nothing_enqueued(ctx):
    import torch

    import entreepy_amd as E

    data, length = table_ladder()
    data[110], length[110] = 0, 0  # a hole
    d_bodies, d_index = _dev_bytes(np.full(120, 100, np.uint8)), _dev_index(_index_of([50, 70]))
    d_rows, d_pos = (torch.full((8,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    d_status = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EntreepyError) as e:
        ctx.search_packed_device(_cb((data, length)), d_bodies, d_index, d_index, b"dd", CONTAINS, rows=d_rows, pos=d_pos, status=d_status)
    assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_rows == -1).all()) and bool((d_pos == -1).all()) and bool((d_status == 0xEE).all()), "something was enqueued"


# --- 11. offsets above 2^32 --------------------------------------------------------------------------------------------------------


def test_offsets_above_4_gib(ctx):
    import torch

    tab = table_255()
    cb = _cb(tab)
    needle = bytes([9, 1, 250, 33] * 5)  # 155 bits
    long = bytes(range(2, 252)) * 4  # 1 000 bytes of body: the workgroup path
    texts = [b"xyz" + needle + b"xyz", needle[:-1] + b"\x02", b"", b"q" + needle, long + needle, long + needle[:-1]]
    bodies = [_pack(tab, t) for t in texts]
    bodies[2] = None  # the filler: a record of length 0 whose body spans 4 GiB + 5 bytes of zeros
    gap = (1 << 32) + 5
    sizes = [gap if b is None else len(b) for b in bodies]
    body_index = _index_of(sizes)
    d_bodies = torch.zeros(int(body_index[-1]) + 1, dtype=torch.uint8, device="cuda")
    for b, at in zip(bodies, body_index[:-1]):
        if b is not None:
            d_bodies[int(at) : int(at) + len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    assert int(body_index[3]) > 1 << 32
    wants = [(OK, len(t), b"" if b is None else want_decode(tab, b, len(t))[1]) for t, b in zip(texts, bodies)]
    assert [w[2] for w in wants] == texts
    dev = (d_bodies[: int(body_index[-1])], _dev_index(body_index), _dev_index(_index_of([len(t) for t in texts])))
    for nd, mode, rows in ((needle, CONTAINS, [0, 3, 4]), (needle, SUFFIX, [3, 4]), (needle, CONTAINS | NOT, [1, 2, 5]), (b"", SUFFIX, [0, 1, 2, 3, 4, 5])):
        assert select(wants, nd, mode)[0] == rows
        check_search(run_search(ctx, cb, dev, 6, nd, mode, len(rows)), wants, nd, mode)


# --- 12. pipelines with nothing in between -----------------------------------------------------------------------------------------


def test_search_then_gather_with_no_synchronisation(ctx):
    import torch

    st, needles = alignment_fixture()
    needle = needles[4]
    want, want_pos = want_search(st, needle, CONTAINS)
    texts = [judged(st)[b][2] for b in want]
    assert len(want) > 3
    dev = upload(st)
    d_rows, d_pos = (torch.full((st.n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    d_out = torch.full((sum(len(t) for t in texts) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_index = torch.full((len(want) + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m = ctx.search_packed_device(st.cb, *dev, needle, CONTAINS, rows=d_rows, pos=d_pos)
    g = ctx.decode_packed_gather_device(st.cb, *dev, d_rows[: m.n_match], d_out[: d_out.numel() - TAIL], d_index)
    torch.cuda.synchronize()
    assert (m.status, m.n_match, m.n_failed) == (OK, len(want), 0) and (g.status, g.n_failed, g.n_short) == (OK, 0, 0)
    assert d_rows[: m.n_match].tolist() == want and bool((d_rows[m.n_match :] == -1).all())
    assert d_pos[: m.n_match].tolist() == want_pos and bool((d_pos[m.n_match :] == -1).all())
    host = d_out.cpu().numpy()
    assert host[: g.out_bytes].tobytes() == b"".join(texts) and bool((host[g.out_bytes :] == SENTINEL).all())
    assert all(t.find(needle) == p for t, p in zip(texts, want_pos))


def _search_take_join(ctx, st, dev, needle):
    """search(SUFFIX) -> take -> join with the taken store as the key set, nothing waited for -> (search, take, join results, d_rows,
    d_hits, the taken d_out)."""
    import torch

    d_rows, d_hits = (torch.full((st.n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    m = ctx.search_packed_device(st.cb, *dev, needle, SUFFIX, rows=d_rows)
    d_out, d_bi, d_ti, t = _taken(ctx, dev, m.n_match, d_rows[: m.n_match], st.bodies.size)
    j = ctx.join_packed_device(st.cb, *dev, d_out[: max(t.out_bytes, 1)], d_bi, d_ti, rows=d_hits)
    return m, t, j, d_rows, d_hits, d_out


def test_search_take_join_on_one_context_and_on_a_side_stream(ctx):
    import torch

    import entreepy_amd as E

    st, needles = alignment_fixture()
    needle = needles[3]
    want = want_search(st, needle, SUFFIX)[0]
    chosen = {judged(st)[b][2] for b in want}
    joined = [b for b, (_, _, t) in enumerate(judged(st)) if t in chosen]
    assert len(want) >= 2 and set(want) <= set(joined)
    dev = upload(st)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    other = E.Context(0)
    try:
        runs = [_search_take_join(ctx, st, dev, needle)]
        other.use_stream(side.cuda_stream)
        runs.append(_search_take_join(other, st, dev, needle))
        torch.cuda.synchronize()
    finally:
        other.close()
    for m, t, j, d_rows, d_hits, d_out in runs:
        assert (m.status, m.n_match, m.n_failed) == (OK, len(want), 0) and (t.status, t.n_failed) == (OK, 0) and (j.status, j.n_failed, j.n_keys_failed) == (OK, 0, 0)
        assert d_rows[: m.n_match].tolist() == want and bool((d_rows[m.n_match :] == -1).all())
        assert d_hits[: j.n_match].tolist() == joined and _guards_intact(d_out, t.out_bytes)


# --- 13. the list helper -----------------------------------------------------------------------------------------------------------


def test_list_helper_on_100_random_byte_strings(ctx):
    import entreepy_amd as E

    rng = np.random.default_rng(0x5EA2C4E0)
    strings = []
    for _ in range(100):
        alphabet = rng.choice(255, size=int(rng.integers(1, 255)), replace=False).astype(np.uint8)
        strings.append(alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(0, 2000)))].tobytes())
    strings[7] = b""
    strings[40], strings[41], strings[42] = strings[3], b"zz" + strings[3][10:60], strings[4][:7] + strings[3][-30:]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(strings), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, strings)
    lengths = [len(s) for s in strings]
    for needle in (strings[3][10:60], strings[3][-30:], strings[3][:1], b""):
        hits = [i for i, s in enumerate(strings) if needle in s]
        assert ctx.search_packed(cb, blob, out_index, lengths, needle, E.SEARCH_CONTAINS) == (hits, [strings[i].find(needle) for i in hits])
        ends = [i for i, s in enumerate(strings) if s.endswith(needle)]
        assert ctx.search_packed(cb, blob, out_index, lengths, needle, E.SEARCH_SUFFIX) == (ends, [len(strings[i]) - len(needle) for i in ends])
        assert ctx.search_packed(cb, blob, out_index, lengths, needle, E.SEARCH_CONTAINS | E.MATCH_NOT) == ([i for i, s in enumerate(strings) if needle not in s], [])
    assert ctx.search_packed(cb, blob, out_index, lengths, strings[3][10:60], E.SEARCH_CONTAINS)[0] == [3, 40, 41]
    assert ctx.search_packed(cb, [], np.zeros(1, np.uint64), [], b"x", E.SEARCH_CONTAINS) == ([], [])
    rows, _ = ctx.search_packed(cb, blob, out_index, lengths, strings[3][-30:], E.SEARCH_SUFFIX)
    assert rows == [3, 40, 42] and ctx.decode_packed_rows(cb, blob, out_index, lengths, rows) == [strings[i] for i in rows]
