"""GPU: et_match_packed_device -- which records of a packed store equal a needle, or begin with it, found on the compressed bytes --
against the oracle: a record's status is judged from its own two pairs of offsets (tests/test_gpu_gather.py's want_rows), its text is
want_decode's, and the expected rows are Python's startswith / == over those texts; never the bit rule the kernels implement.
d_rows (cap_rows + TAIL entries) and d_status are filled with sentinels first; everything behind n_match must still hold them.

The stores and needles are made by the *_fixture functions below, without a GPU: tests/test_match_host.py checks on the same fixtures
that the bit rule selects what decode-and-compare selects, and that they reach the cases named here."""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus
from tests.test_gpu_batch import SENTINEL, _oracle, _small_max, _u8
from tests.test_gpu_gather import _mixed_store, make_store, upload, want_rows
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_gpu_shared import _cb, _family, _length_batch, want_decode
from tests.test_shared_host import oracle_table, table_255, table_2bit, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
EQUAL, PREFIX, NOT = 0, 1, 0x100  # ET_MATCH_*
MODES = [EQUAL, PREFIX, EQUAL | NOT, PREFIX | NOT]
HEAD_BITS = 64  # what a lane compares alone (csrc/et_batch.h MATCH_HEAD_BITS)
TILE = 256  # records per tile of the flag and emit kernels (csrc/et_batch.h MATCH_TILE)
ROW_SENTINEL = int(np.array([SENTINEL] * 4, np.uint8).view(np.uint32)[0])


# --- the expected rows: the oracle's texts, Python's comparison -------------------------------------------------------------------


def judged(st):
    """Per record (status, length, text), once per store."""
    if not hasattr(st, "wants"):
        st.wants = want_rows(st, range(st.n))
    return st.wants


def select(wants, needle, mode):
    needle, out = bytes(needle), []
    for b, (status, length, text) in enumerate(wants):
        if status:
            continue
        hit = text.startswith(needle) if mode & PREFIX else (length == len(needle) and text == needle)
        if hit != bool(mode & NOT):
            out.append(b)
    return out


def want_match(st, needle, mode):
    return select(judged(st), needle, mode)


# --- one call ----------------------------------------------------------------------------------------------------------------------


def run_match(ctx, cb, dev, n, needle, mode, cap, count_only=False):
    """One call through the C ABI (a capacity of zero is still a pointer), every output full of sentinels first."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    d_bodies, d_body_index, d_text_index = dev
    needle = bytes(needle)
    r = SimpleNamespace(cap=cap, count_only=count_only)
    r.d_rows = torch.full((4 * (cap + TAIL),), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.int32)
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = N.MatchResult()
    rc = N.lib().et_match_packed_device(ctx._h, ctypes.byref(cb.raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), n, needle, len(needle),
                                        mode, None if count_only else r.d_rows.data_ptr(), cap, r.d_status.data_ptr(), ctypes.byref(res))
    torch.cuda.synchronize()
    r.res = E.MatchResult(rc, res.n_match, res.n_failed, res.first_failed, res.first_status, res.pattern_bits)
    r.rows, r.status = r.d_rows.cpu().numpy().view(np.uint32), r.d_status.cpu().numpy()
    return r


def check_match(r, wants, needle, mode, call_status=OK, pattern_bits=None):
    want = select(wants, needle, mode)
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
    assert got == want, f"the rows differ from the oracle's, first at {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"
    assert bool((r.rows[len(want) :] == ROW_SENTINEL).all()), "an entry at or behind d_rows + n_match was written"
    return want


def match(ctx, st, needle, mode, dev=None, **kw):
    """Run with cap_rows = the need exactly, and check."""
    need = len(want_match(st, needle, mode))
    r = run_match(ctx, st.cb, dev or upload(st), st.n, needle, mode, need)
    check_match(r, judged(st), needle, mode, **kw)
    return r


def pattern_bits(tab, needle):
    needle = _u8(needle)
    return int(tab[1][needle].astype(np.int64).sum()) if needle.size and bool((tab[1][needle] > 0).all()) else 0


def _pack(tab, text):
    return _oracle().pack_body(tab[0], tab[1], text, 0)[0] if len(text) else b""


def _store(tab, texts, bodies=None):
    return make_store(tab, [_u8(t) for t in texts], None if bodies is None else [_u8(b) for b in bodies])


# --- the fixtures: (store, needles), made without a GPU -----------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def lengths_fixture():
    """_length_batch()'s texts (0 .. 8193 bytes, small_max, small_max + 1) plus duplicates of four of them."""
    tab, texts = _length_batch()
    texts = list(texts) + [texts[5], texts[7], texts[13], texts[9]]
    t17, t255, t4096 = (texts[i].tobytes() for i in (5, 9, 13))
    assert (len(t17), len(t255), len(t4096)) == (17, 255, 4096)
    extra = t17[:1]
    return _store(tab, texts), [b"", extra, t17, t4096, t17[:-1], t255[:-1], t17 + extra, t255 + extra]


BIT_EDGE_STEM = bytes([65, 200, 3])


@functools.lru_cache(maxsize=None)
def bit_edges_fixture():
    """table_255: byte 1 has the 7-bit codeword 0000000, every other byte 8 bits -- a stem plus k ones ends at every bit of a byte."""
    tab = table_255()
    assert int(tab[1][1]) == 7 and int(tab[0][1]) == 0
    needles = [BIT_EDGE_STEM + b"\x01" * k for k in range(1, 9)]
    texts, bodies = [], []

    def add(text, body=None):
        texts.append(text)
        bodies.append(_pack(tab, text) if body is None else body)

    for nd in needles:
        add(nd)  # equal
        add(nd[:-1] + b"\x02")  # the last symbol alone differs: 00000010 against 0000000
        add(nd[:-1] + b"\xff")
        for s in (1, 2, 255):  # one symbol more
            add(nd + bytes([s]))
        add(nd[:-1])  # the zero-codeword trap: the pad bits read as the needle's last symbol ...
        add(nd[:-1], _pack(tab, nd[:-1]) + b"\0")  # ... also where a whole byte of pad follows
        add(nd, _pack(tab, nd)[:-1])  # the exact body cut by a byte
        add(nd + b"ABCDE", _pack(tab, nd + b"ABCDE")[:-1])  # a longer one cut: the needle is still all there
        add(nd, b"")  # no body under a length above zero
    return _store(tab, texts, bodies), needles


@functools.lru_cache(maxsize=None)
def bit_edges_2bit_fixture():
    """Four symbols of 2 bits, A = 00: a record one A short of the needle has the needle's bytes whenever the A falls into its pad."""
    tab = table_2bit()
    needles = [b"A", b"GA", b"TAA", b"CGTA", b"CGTAA", b"TTTTTTTA"]
    texts = []
    for nd in needles:
        texts += [nd, nd[:-1], nd + b"A", nd + b"T", nd[:-1] + b"C", nd[:-1] + b"AA"]
    return _store(tab, texts), needles


@functools.lru_cache(maxsize=None)
def alignment_fixture():
    st = _mixed_store(256, 0x6A7E4030)  # 0 .. 200 bytes, back to back: every start alignment mod 16
    texts = [t for _, _, t in judged(st)]
    long = max(texts, key=len)
    return st, [texts[10][:2], texts[20], texts[30][:40], long, long[:-1], b" "]


@functools.lru_cache(maxsize=None)
def survivors_fixture():
    """300 records under the ladder table, made of its two 32-bit codewords (bytes 131 and 132: 4 bytes of body per symbol, the head
    window is two symbols) around one 1 000-symbol text.  Records 0 .. 63 -- the first wavefront -- all equal it: every lane survives
    its head.  Records 64 .. 127 differ inside the head except record 81: one lane survives."""
    tab = table_ladder()
    assert int(tab[1][131]) == 32 and int(tab[1][132]) == 32 and int(tab[1][107]) == 8
    rng = np.random.default_rng(0x3A7C4040)
    long = (131 + rng.integers(0, 2, size=4200)).astype(np.uint8)
    base = long[:1000]

    def flip(t, i, to=None):
        u = t.copy()
        u[i] = 263 - int(u[i]) if to is None else to
        return u

    texts = [base] * 64
    texts += [base if i == 17 else flip(base, i % 2) for i in range(64)]
    variants = [base, flip(base, 2), flip(base, 2, to=107), flip(base, 500), flip(base, 999), base[:999], np.concatenate((base, base[:1])), flip(base, 8), flip(base, 63),
                flip(base, 64), base[:64], base[:9], base[:8], flip(base, 3)]
    longs = [long, long[:4096], flip(long, 4095), flip(long, 4096), flip(long, 2048), long[:4095]]
    texts += [variants[i % len(variants)] for i in range(300 - 128 - len(longs))] + longs
    assert len(texts) == 300
    return _store(tab, texts), [base[:9].tobytes(), base[:64].tobytes(), base.tobytes(), long[:4096].tobytes()]


@functools.lru_cache(maxsize=None)
def tiles_fixture(n):
    """n tiny records over four symbols; those at the first and the last place of every tile, and a tenth of the rest, begin ACGT."""
    tab = table_2bit()
    rng = np.random.default_rng(0x3A7C4050 + n)
    hits = set(rng.integers(0, n, size=n // 10).tolist())
    for t0 in range(0, n, TILE):
        hits |= {t0, min(t0 + TILE, n) - 1}
    letters = np.frombuffer(b"ACGT", np.uint8)
    texts = [(b"ACGT" if i in hits else b"G") + letters[rng.integers(0, 4, size=int(rng.integers(0, 13)))].tobytes() for i in range(n)]
    return _store(tab, texts), [b"ACGT", b"", b"T" * 20]


@functools.lru_cache(maxsize=None)
def tiny_fixture():
    """20 000 records of 0 .. 8 bytes, every third beginning with the needle."""
    tab = table_255()
    rng = np.random.default_rng(0x3A7C4060)
    needle = bytes([77, 1, 200])
    texts = []
    for i in range(20_000):
        tail = rng.integers(1, 256, size=int(rng.integers(0, 9))).astype(np.uint8).tobytes()
        texts.append(needle + tail[:5] if i % 3 == 0 else tail)
    return _store(tab, texts), [needle]


@functools.lru_cache(maxsize=None)
def failures_fixture():
    """14 records; 3 (a decreasing body pair), 8 and 9 (a body entry at 2^63), 11 (a decreasing text pair) and 13 (a length above the
    small-stream limit) fail.  Record 4's body begins 5 bytes early, record 12 asks for more symbols than its body holds."""
    sizes = [150, 140, 1, 130, 166, 0, 145, 155, 152, 135, 149, 144, 150, 138]
    pool = corpus.text_like(sum(sizes), 0x3A7C4070)
    cuts = _index_of(sizes)
    st = make_store(oracle_table(pool), [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(14)])
    st.body_index[4] = st.body_index[3] - np.uint64(5)
    st.body_index[9] = np.uint64(1) << np.uint64(63)
    st.text_index[12] = st.text_index[11] - np.uint64(3)
    st.text_index[14] = st.text_index[13] + np.uint64(_small_max() + 1)
    return st, [pool[:3].tobytes(), pool[int(cuts[6]) : int(cuts[7])].tobytes(), b""]


def _res_files():
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "res")
    out = {}
    for name in ("a_midsummer_nights_dream.txt",):
        with open(os.path.join(golden, name), "rb") as f:
            out[name] = f.read()
    return out


FAMILIES = ["text", "2bit", "uniform255", "zeros90", "ladder32"]


@functools.lru_cache(maxsize=None)
def family_fixture(name):
    tab, draw = _family(name, _res_files())
    rng = np.random.default_rng(0x3A7C40B0)
    texts = [draw(int(n), 0x3A7C40B1 + i) for i, n in enumerate(rng.integers(1, 201, size=60))]
    texts += [texts[5], texts[0][:3], texts[5][:-1]]
    t0, t5 = texts[0].tobytes(), texts[5].tobytes()
    return _store(tab, texts), [t0[:1], t0[:3], t5[:12], t5, t5[:-1]]


FIXTURES = {"lengths": lengths_fixture, "bit_edges": bit_edges_fixture, "bit_edges_2bit": bit_edges_2bit_fixture, "alignment": alignment_fixture, "survivors": survivors_fixture,
            "tiny": tiny_fixture, "failures": failures_fixture, **{f"tiles_{n}": functools.partial(tiles_fixture, n) for n in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)},
            **{f"family_{name}": functools.partial(family_fixture, name) for name in FAMILIES}}


# --- 1. lengths and modes ----------------------------------------------------------------------------------------------------------


def test_lengths_and_modes(ctx):
    st, needles = lengths_fixture()
    dev = upload(st)
    assert [s for s, _, _ in judged(st)].count(UNSUPPORTED) == 1  # (the text of small_max + 1 bytes)
    for needle in needles:
        for mode in MODES:
            match(ctx, st, needle, mode, dev=dev, pattern_bits=pattern_bits(st.tab, needle))
    assert len(want_match(st, needles[2], EQUAL)) == 2 and len(want_match(st, needles[3], EQUAL)) == 2  # a record and its duplicate
    assert len(want_match(st, needles[4], PREFIX)) == 2 and want_match(st, needles[4], EQUAL) == []
    assert want_match(st, needles[6], PREFIX) == [] and len(want_match(st, b"", EQUAL)) == 1


# --- 2. bit edges ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["table_255", "2bit"])
def test_bit_edges(ctx, which):
    st, needles = bit_edges_fixture() if which == "table_255" else bit_edges_2bit_fixture()
    dev = upload(st)
    if which == "table_255":
        assert sorted(pattern_bits(st.tab, nd) % 8 for nd in needles) == list(range(8))
    for needle in needles:
        for mode in MODES:
            match(ctx, st, needle, mode, dev=dev, pattern_bits=pattern_bits(st.tab, needle))


# --- 3. alignment ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_body_alignment_and_base(ctx, shift):
    import torch

    st, needles = alignment_fixture()
    assert {int(b) % 16 for b, e in zip(st.body_index[:-1], st.body_index[1:]) if e > b} == set(range(16))
    raw = torch.zeros(shift + st.bodies.size + 16, dtype=torch.uint8, device="cuda")
    raw[shift : shift + st.bodies.size] = torch.from_numpy(st.bodies.copy()).cuda()
    assert raw.data_ptr() % 16 == 0
    dev = (raw[shift : shift + st.bodies.size], _dev_index(st.body_index), _dev_index(st.text_index))
    for needle in needles:
        for mode in (EQUAL, PREFIX):
            match(ctx, st, needle, mode, dev=dev)
    assert len(want_match(st, needles[3], EQUAL)) >= 1 and len(needles[3]) * 8 > HEAD_BITS


# --- 4. survivors ------------------------------------------------------------------------------------------------------------------


def test_survivors(ctx):
    st, needles = survivors_fixture()
    dev = upload(st)
    assert [len(nd) for nd in needles] == [9, 64, 1000, 4096]
    for needle in needles:
        for mode in (EQUAL, PREFIX):
            r = match(ctx, st, needle, mode, dev=dev, pattern_bits=32 * len(needle))
    assert r.res.pattern_bits == 16384 * 8  # the whole 16 KiB pattern
    base = want_match(st, needles[2], PREFIX)
    assert set(range(64)) <= set(base) and [b for b in base if 64 <= b < 128] == [81]
    assert len(want_match(st, needles[3], PREFIX)) == 3 and len(want_match(st, needles[3], EQUAL)) == 1


# --- 5. tiles and scan edges -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tile_and_scan_edges(ctx, n):
    st, (needle, everything, nothing) = tiles_fixture(n)
    dev = upload(st)
    want = want_match(st, needle, PREFIX)
    for t0 in range(0, n, TILE):
        assert t0 in want and min(t0 + TILE, n) - 1 in want
    match(ctx, st, needle, PREFIX, dev=dev)
    match(ctx, st, needle, PREFIX | NOT, dev=dev)
    assert want_match(st, everything, PREFIX) == list(range(n)) and want_match(st, nothing, PREFIX) == []
    match(ctx, st, everything, PREFIX, dev=dev)
    match(ctx, st, nothing, PREFIX, dev=dev)
    match(ctx, st, nothing, EQUAL, dev=dev)


# --- 6. many tiny records ----------------------------------------------------------------------------------------------------------


def test_20000_tiny_records_a_third_of_them_matching(ctx):
    st, (needle,) = tiny_fixture()
    want = want_match(st, needle, PREFIX)
    assert 6_600 < len(want) < 6_800 and want == sorted(want)
    dev = upload(st)
    match(ctx, st, needle, PREFIX, dev=dev)
    match(ctx, st, needle, EQUAL | NOT, dev=dev)


# --- 7. failures stay local --------------------------------------------------------------------------------------------------------


def test_failures_stay_local(ctx):
    st, needles = failures_fixture()
    wants = judged(st)
    assert [s for s, _, _ in wants] == [OK, OK, OK, ARG, OK, OK, OK, OK, ARG, ARG, OK, ARG, OK, UNSUPPORTED]
    dev = upload(st, spare=st.bodies.size)  # (what lies behind body_bytes is mapped; 2^63 is not: a pair that is followed faults or shows)
    for needle in needles:
        for mode in MODES:
            r = match(ctx, st, needle, mode, dev=dev)
            assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (5, 3, ARG)
    assert want_match(st, b"", PREFIX | NOT) == [] and want_match(st, b"", PREFIX) == [0, 1, 2, 4, 5, 6, 7, 10, 12]
    assert want_match(st, needles[1], EQUAL) == [6] and 0 in want_match(st, needles[0], PREFIX)


# --- 8. capacity and count only ----------------------------------------------------------------------------------------------------


def test_capacity_and_count_only(ctx):
    st, needles = failures_fixture()
    wants, needle, mode = judged(st), needles[1], EQUAL | NOT
    dev = upload(st, spare=st.bodies.size)
    need = len(select(wants, needle, mode))
    assert need == 8
    short = run_match(ctx, st.cb, dev, st.n, needle, mode, need - 1)
    check_match(short, wants, needle, mode, call_status=CAP)
    check_match(run_match(ctx, st.cb, dev, st.n, needle, mode, 0), wants, needle, mode, call_status=CAP)
    exact = run_match(ctx, st.cb, dev, st.n, needle, mode, need)
    check_match(exact, wants, needle, mode)
    count = run_match(ctx, st.cb, dev, st.n, needle, mode, need, count_only=True)
    check_match(count, wants, needle, mode)
    assert count.res == exact.res and np.array_equal(count.status, exact.status) and np.array_equal(short.status, exact.status)
    assert dict(vars(short.res), status=OK) == vars(exact.res)
    # the Python call: rows=None counts, a tensor one entry short reports the need
    import torch

    import entreepy_amd as E

    d_rows = torch.full((need + TAIL,), -1, dtype=torch.int32, device="cuda")
    assert ctx.match_packed_device(st.cb, *dev, needle, E.MATCH_EQUAL | E.MATCH_NOT) == exact.res
    r = ctx.match_packed_device(st.cb, *dev, needle, mode, rows=d_rows[: need - 1])
    assert (r.status, r.n_match) == (CAP, need)
    r = ctx.match_packed_device(st.cb, *dev, needle, mode, rows=d_rows[:need])
    torch.cuda.synchronize()
    assert r == exact.res and d_rows[:need].tolist() == select(wants, needle, mode) and bool((d_rows[need:] == -1).all())


# --- 9. a needle outside the table -------------------------------------------------------------------------------------------------


def test_a_needle_byte_without_a_code_matches_nothing(ctx):
    st, needles = failures_fixture()
    assert int(st.tab[1][0xFF]) == 0
    dev = upload(st, spare=st.bodies.size)
    for needle in (b"\xff", needles[0] + b"\xff", b"\xff" + needles[0]):
        for mode in MODES:
            r = match(ctx, st, needle, mode, dev=dev, pattern_bits=0)
            assert r.res.n_match == (9 if mode & NOT else 0)


# --- 10. an incomplete table -------------------------------------------------------------------------------------------------------


def test_an_incomplete_table_is_refused_with_nothing_enqueued(ctx):
    import torch

    import entreepy_amd as E

    data, length = table_ladder()
    data[110], length[110] = 0, 0  # a hole
    d_bodies, d_index = _dev_bytes(np.full(120, 100, np.uint8)), _dev_index(_index_of([50, 70]))
    d_rows = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    d_status = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EntreepyError) as e:
        ctx.match_packed_device(_cb((data, length)), d_bodies, d_index, d_index, b"dd", PREFIX, rows=d_rows, status=d_status)
    assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_rows == -1).all()) and bool((d_status == 0xEE).all()), "something was enqueued"


# --- 11. code families -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", FAMILIES)
def test_code_families(ctx, name):
    st, needles = family_fixture(name)
    dev = upload(st)
    for needle in needles:
        for mode in (EQUAL, PREFIX):
            match(ctx, st, needle, mode, dev=dev, pattern_bits=pattern_bits(st.tab, needle))
    assert len(want_match(st, needles[3], EQUAL)) >= 2 and len(want_match(st, needles[4], PREFIX)) >= 3


# --- 12. offsets above 2^32 --------------------------------------------------------------------------------------------------------


def test_offsets_above_4_gib(ctx):
    import torch

    tab = table_255()
    cb = _cb(tab)
    needle = bytes([9, 1, 250, 33] * 5)  # 155 bits: beyond the head window
    texts = [needle + b"xyz", needle[:-1] + b"\x02", b"", needle, b"q" + needle]
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
    for nd, mode, rows in ((needle, PREFIX, [0, 3]), (needle, EQUAL, [3]), (needle, PREFIX | NOT, [1, 2, 4]), (b"", EQUAL, [2]), (b"", PREFIX, [0, 1, 2, 3, 4])):
        assert select(wants, nd, mode) == rows
        check_match(run_match(ctx, cb, dev, 5, nd, mode, len(rows)), wants, nd, mode)


# --- 13. pipeline and ordering -----------------------------------------------------------------------------------------------------


def test_match_then_gather_with_no_synchronisation(ctx):
    """filter -> rows -> gather on one ctx, nothing in between: the rows the match wrote are the gather's."""
    import torch

    st, needles = alignment_fixture()
    needle = needles[5]
    want = want_match(st, needle, PREFIX)
    texts = [judged(st)[b][2] for b in want]
    assert len(want) > 3
    dev = upload(st)
    d_rows = torch.full((st.n,), -1, dtype=torch.int32, device="cuda")
    d_out = torch.full((sum(len(t) for t in texts) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_index = torch.full((len(want) + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    m = ctx.match_packed_device(st.cb, *dev, needle, PREFIX, rows=d_rows)
    g = ctx.decode_packed_gather_device(st.cb, *dev, d_rows[: m.n_match], d_out[: d_out.numel() - TAIL], d_index)
    torch.cuda.synchronize()
    assert (m.status, m.n_match, m.n_failed) == (OK, len(want), 0) and (g.status, g.n_failed, g.n_short) == (OK, 0, 0)
    assert d_rows[: m.n_match].tolist() == want and bool((d_rows[m.n_match :] == -1).all())
    host = d_out.cpu().numpy()
    assert host[: g.out_bytes].tobytes() == b"".join(texts) and bool((host[g.out_bytes :] == SENTINEL).all())
    assert all(t.startswith(needle) for t in texts)


def test_match_between_packed_and_shared_calls_and_on_a_side_stream(ctx):
    """A packed decode, a match under another table and a shared-table encode under a third on one ctx with no synchronisation in
    between -- the packed calls' workspace, counters and report slot are rewritten in stream order -- and one more match of another
    context on a side stream."""
    import torch

    import entreepy_amd as E

    a = _mixed_store()
    b, (needle, *_) = survivors_fixture()
    c, _ = bit_edges_2bit_fixture()
    dev_a, dev_b = upload(a), upload(b)
    a_total = int(a.text_index[-1])
    d_a = torch.full((a_total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    want = want_match(b, needle, PREFIX)
    runs = [SimpleNamespace(d_rows=torch.full((len(want) + TAIL,), -1, dtype=torch.int32, device="cuda"), d_status=torch.full((b.n,), 0xEE, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    texts = [judged(c)[k][2] for k in range(c.n)]
    d_text = _dev_bytes(np.frombuffer(b"".join(texts), np.uint8))
    offs = _index_of([len(t) for t in texts])
    caps = np.array([c.cb.body_bound(len(t)) for t in texts], np.uint64)
    out_off = _index_of(caps)[:-1]
    d_shared = torch.full((int(caps.sum()) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    other = E.Context(0)
    try:
        p = ctx.decode_packed_device(a.cb, *dev_a, d_a[:a_total])
        runs[0].res = ctx.match_packed_device(b.cb, *dev_b, needle, PREFIX, rows=runs[0].d_rows[: len(want)], status=runs[0].d_status)
        out_len, status, _ = ctx.encode_shared_device(c.cb, d_text, offs[:-1], np.diff(offs), d_shared, out_off, caps)
        other.use_stream(side.cuda_stream)
        runs[1].res = other.match_packed_device(b.cb, *dev_b, needle, PREFIX, rows=runs[1].d_rows[: len(want)], status=runs[1].d_status)
        torch.cuda.synchronize()
    finally:
        other.close()
    for r in runs:
        assert (r.res.status, r.res.n_match, r.res.n_failed, r.res.pattern_bits) == (OK, len(want), 0, 32 * len(needle))
        assert r.d_rows[: len(want)].tolist() == want and bool((r.d_rows[len(want) :] == -1).all()) and not bool(r.d_status.any())
    assert (p.status, p.out_bytes, p.n_failed) == (OK, a_total, 0)
    host = d_a.cpu().numpy()
    assert host[:a_total].tobytes() == b"".join(t for _, _, t in want_rows(a, range(a.n))) and bool((host[a_total:] == SENTINEL).all())
    host = d_shared.cpu().numpy()
    assert not status.any()
    for t, o, n in zip(texts, out_off, out_len):
        assert host[int(o) : int(o) + int(n)].tobytes() == _pack(c.tab, t)


# --- 14. the list helper -----------------------------------------------------------------------------------------------------------


def test_list_helper_on_100_random_byte_strings(ctx):
    import entreepy_amd as E

    rng = np.random.default_rng(0x3A7C40E0)
    strings = []
    for _ in range(100):
        alphabet = rng.choice(255, size=int(rng.integers(1, 255)), replace=False).astype(np.uint8)
        strings.append(alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(0, 2000)))].tobytes())
    strings[7] = b""
    strings[40], strings[41], strings[42] = strings[3], strings[3][:50], strings[3] + strings[4][:1]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(strings), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, strings)
    lengths = [len(s) for s in strings]
    for needle in (strings[3], strings[3][:50], strings[3][:1], b""):
        assert ctx.match_packed(cb, blob, out_index, lengths, needle, E.MATCH_PREFIX) == [i for i, s in enumerate(strings) if s.startswith(needle)]
        assert ctx.match_packed(cb, blob, out_index, lengths, needle, E.MATCH_EQUAL) == [i for i, s in enumerate(strings) if s == needle]
        assert ctx.match_packed(cb, blob, out_index, lengths, needle, E.MATCH_EQUAL | E.MATCH_NOT) == [i for i, s in enumerate(strings) if s != needle]
    assert ctx.match_packed(cb, blob, out_index, lengths, strings[3], E.MATCH_EQUAL) == [3, 40]
    assert ctx.match_packed(cb, [], np.zeros(1, np.uint64), [], b"x", E.MATCH_PREFIX) == []
    rows = ctx.match_packed(cb, blob, out_index, lengths, strings[3][:50], E.MATCH_PREFIX)
    assert ctx.decode_packed_rows(cb, blob, out_index, lengths, rows) == [strings[i] for i in rows]
