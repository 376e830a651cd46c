"""GPU: et_concat_packed_device -- row k = text(A[rows_a[k]]) + a literal + text(B[rows_b[k]]) as a new packed store, laid out on the
compressed bytes -- against the oracle: each side's record is judged from its own two pairs of offsets, its stored text is
want_decode's, the row's text is Python's concatenation of the three, and the expected bytes are the oracle's shared-table encode of
that text (want_concat()); never the bit walk the kernels implement.  d_out lies between sentinel bytes as in tests/test_gpu_take.py,
whose check_take() compares bytes, both offset arrays, the status bytes and the report.

The stores and the rows are made by the *_fixture functions below, without a GPU: tests/test_concat_host.py checks on the same fixtures
that the bit rule gives what the oracle gives, and that they reach the cases named here."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import retained_concat  # noqa: F401  (the call's row joins the table of tests/retained.py)
from tests.test_gpu_batch import SENTINEL, _small_max
from tests.test_gpu_gather import dev_rows, make_store, upload
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_gpu_shared import _cb, want_decode, want_encode
from tests.test_gpu_slice import cut_fixture, ladder_fixture, main_fixture, set_pad_fixture, stored_text
from tests.test_gpu_take import C, LEAD, SCAN_TILE, _guards_intact, check_take, failures_store
from tests.test_shared_host import table_255, table_2bit

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
BLOCK = 8192  # the bytes of body the workgroup path stages at a time


def lane_bytes():
    """A body of either side whose reach() is up to this many bytes is walked by the row's lane; a row with a longer one on either side
    goes to a workgroup."""
    from entreepy_amd import _native as N

    return int(N.lib().et_concat_lane_bytes())


def left_reach(st, r):
    """What the walk of record r can touch of its body, as a left or as a right record: min(bytes, 4 * length + 8) (csrc/et_batch.h
    clip_body) -- what decides between the lane and the workgroup."""
    nb, length = int(st.body_index[r + 1] - st.body_index[r]), int(st.text_index[r + 1] - st.text_index[r])
    return min(nb, 4 * length + 8)


def bits_of(tab, text):
    return int(tab[1][np.frombuffer(bytes(text), np.uint8)].astype(np.int64).sum())


# --- the expected store --------------------------------------------------------------------------------------------------------------------


def judge(st, r):
    """-> the status of record r by the take's rule; an absent side (st is None) is an OK record of nothing."""
    if st is None:
        return OK
    if r >= st.n:
        return ARG
    b0, b1, t0, t1 = (int(x) for x in (st.body_index[r], st.body_index[r + 1], st.text_index[r], st.text_index[r + 1]))
    if not (b0 <= b1 <= st.bodies.size and t0 <= t1):
        return ARG
    return UNSUPPORTED if t1 - t0 > _small_max() or b1 - b0 > 4 * _small_max() else OK


def want_concat(A, B, rows_a, rows_b, sep):
    """-> what tests/test_gpu_take.py's model() returns, for the rows; .texts: the rows' texts."""
    tab = (A or B).tab
    n = len(rows_a) if rows_a is not None else len(rows_b) if rows_b is not None else (A or B).n
    rows_a = np.arange(n) if rows_a is None else np.asarray(rows_a, dtype=np.int64)
    rows_b = np.arange(n) if rows_b is None else np.asarray(rows_b, dtype=np.int64)
    memo = {}
    status, nb, ln, pieces, texts = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint64), [], []
    for k, (ra, rb) in enumerate(zip((int(r) for r in rows_a), (int(r) for r in rows_b))):
        if (ra, rb) not in memo:
            row = (judge(A, ra) or judge(B, rb), b"", b"")
            if not row[0]:
                text = (stored_text(A, ra) if A is not None else b"") + sep + (stored_text(B, rb) if B is not None else b"")
                if len(text) > _small_max():
                    row = (UNSUPPORTED, b"", b"")
                else:
                    rc, body = want_encode(tab, text)
                    assert rc == OK
                    row = (OK, body, text)
            memo[ra, rb] = row
        status[k], body, text = memo[ra, rb]
        nb[k], ln[k] = len(body), len(text)
        pieces.append(np.frombuffer(body, np.uint8))
        texts.append(text)
    data = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    return SimpleNamespace(status=status, body_index=_index_of(nb), text_index=_index_of(ln), data=data, total=int(nb.sum()), text_total=int(ln.sum()), texts=texts)


# --- the fixtures ----------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def literals():
    """Literals under the main fixture's table by the bits they take mod 8 -> {0: b"", 1 .. 7: ..., "byte": a multiple of 8, "long": the
    longest allowed}.  (Literals of 1, 2, 4, 6 and 7 bits in all: under the ladder, the 2-bit table and table_255.)"""
    st, texts = main_fixture()
    pool = [bytes([s]) for s in np.flatnonzero(st.tab[1]) if 32 <= s < 127]
    out = {0: b""}
    for a in pool:
        for b in [b""] + pool:
            n = bits_of(st.tab, a + b)
            out.setdefault(n % 8 if n % 8 else "byte", a + b)
    out["long"] = (texts[9] * 3)[:256]
    return out


@functools.lru_cache(maxsize=None)
def main_rows():
    """600 pairs over the main fixture (44 records of text, bodies of 0 bytes to 22 KiB): every left record with many right ones."""
    st, _ = main_fixture()
    rng = np.random.default_rng(0xC07CA701)
    rows_a, rows_b = np.concatenate((np.arange(st.n), rng.integers(0, st.n, size=600 - st.n))), rng.integers(0, st.n, size=600)
    rows_a[-3:], rows_b[-3:] = [0, 0, 5], [0, 5, 0]  # record 0 is empty: both sides empty, the left alone, the right alone
    return rows_a, rows_b


@functools.lru_cache(maxsize=None)
def dna_fixture():
    """Under the 2-bit table: records of 0 .. 40 symbols (left bits 0, 2, 4, 6 mod 8), and at the end 60 of 1 .. 3 symbols: a byte each."""
    rng = np.random.default_rng(0xC07CA702)
    sizes = list(range(41)) + [int(x) for x in rng.integers(1, 4, size=60)]
    texts = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).tobytes()) for n in sizes]
    return make_store(table_2bit(), texts), texts


@functools.lru_cache(maxsize=None)
def edge_fixture():
    """Under table_255 (byte 1: 7 bits, every other: 8), bodies of exactly chosen sizes -> (store, {name: record}): around the lane's
    threshold, over one 8 KiB block, over two tiles of output (the right side of the tile-crossing row), a left run that ends mid-byte."""
    rng = np.random.default_rng(0xC07CA703)
    lane = lane_bytes()
    sizes = {"lane-1": lane - 1, "lane": lane, "lane+1": lane + 1, "lane+2": lane + 2, "block+": BLOCK + 700, "tiles": 2 * C + 4000, "few": 5}
    texts = [rng.integers(2, 256, size=n, dtype=np.uint8).tobytes() for n in sizes.values()]
    names = {name: i for i, name in enumerate(sizes)}
    for name in ("lane+1m", "block+m"):  # the same with a 7-bit codeword in front: every byte behind it straddles two
        names[name] = len(texts)
        texts.append(b"\x01" + texts[names[name[:-1]]])
    names["mid"] = len(texts)
    texts.append(b"\x01" + texts[names["few"]])
    return make_store(table_255(), texts), names


@functools.lru_cache(maxsize=None)
def empties_fixture():
    """Under the main fixture's table -> store: 0 the empty record; 1, 2 two texts; 3 kept raw (no bytes, length 9); 4 one symbol."""
    st, texts = main_fixture()
    keep = [b"", texts[5], texts[6], b"nine char", texts[1]]
    bodies = [want_encode(st.tab, t)[1] for t in keep]
    bodies[3] = b""
    return make_store(st.tab, keep, bodies)


def empty_run_rows(run):
    """Full rows with a run of empty ones between them, at the start and at the end."""
    empty = np.zeros(run, dtype=np.int64)
    return np.concatenate((empty, [1], empty, [2], empty))


@functools.lru_cache(maxsize=None)
def right_pad_fixture():
    """The dna fixture's records with every pad bit of every body SET (hand-made bodies) -> store."""
    st, texts = dna_fixture()
    bodies = []
    for r, t in enumerate(texts):
        body = bytearray(st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes())
        if len(t) % 4:
            body[-1] |= (1 << (8 - 2 * (len(t) % 4))) - 1
        bodies.append(bytes(body))
    return make_store(st.tab, texts, bodies)


@functools.lru_cache(maxsize=None)
def limit_fixture():
    """Under the 2-bit table -> (store, the limit): 0 = 10 symbols; 1, 2 = texts that bring row (0, "AC", .) exactly to the limit and one
    above it; 3 = a text of the limit itself."""
    small = _small_max()
    pool = np.random.default_rng(0xC07CA704).choice(np.frombuffer(b"ACGT", np.uint8), size=small).tobytes()
    return make_store(table_2bit(), [pool[:10], pool[: small - 12], pool[: small - 11], pool]), small


def with_table(st, tab):
    st.tab, st.cb = tab, _cb(tab)
    return st


# --- one call and its check ------------------------------------------------------------------------------------------------------------------


def run_concat(ctx, A, B, rows_a, rows_b, sep, cap, dev_a=None, dev_b=None, sizes_only=False, shift=0, tile_off=None):
    """One call, every output full of sentinels first (tests/test_gpu_take.py's run_take).  rows_x=None: d_rows_x == NULL."""
    import torch

    dev_a = dev_a or (upload(A) if A is not None else None)
    dev_b = dev_b or (dev_a if B is A else upload(B) if B is not None else None)
    n = len(rows_a) if rows_a is not None else len(rows_b) if rows_b is not None else (A or B).n
    r = SimpleNamespace(cap=cap, sizes_only=sizes_only)
    r.d_raw = torch.full((3 * C + LEAD + 16 + cap + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert r.d_raw.data_ptr() % 16 == 0
    r.at = LEAD + shift if tile_off is None else (-r.d_raw.data_ptr()) % C + C + tile_off
    r.d_out = r.d_raw[r.at : r.at + max(cap, 1)]
    r.d_body_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_text_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.res = ctx.concat_packed_device((A or B).cb, dev_a, sep, dev_b, None if sizes_only else r.d_out, r.d_body_index, r.d_text_index,
                                     rows_a=None if rows_a is None or A is None else dev_rows(rows_a), rows_b=None if rows_b is None or B is None else dev_rows(rows_b),
                                     status=r.d_status)
    torch.cuda.synchronize()
    r.host = r.d_raw.cpu().numpy()
    r.body_index, r.text_index = r.d_body_index.cpu().numpy().view(np.uint64), r.d_text_index.cpu().numpy().view(np.uint64)
    r.status = r.d_status.cpu().numpy()
    return r


def concat(ctx, A, B, rows_a, rows_b, sep, **kw):
    """Run with cap = the need exactly, and check."""
    want = want_concat(A, B, rows_a, rows_b, sep)
    r = check_take(run_concat(ctx, A, B, rows_a, rows_b, sep, want.total, **kw), want)
    r.want = want
    return r


def stored_rows(r, tab):
    """The stored texts of the rows the call wrote, by the oracle's decode."""
    out = []
    for k in range(r.body_index.size - 1):
        body = r.host[r.at + int(r.body_index[k]) : r.at + int(r.body_index[k + 1])].tobytes()
        out.append(want_decode(tab, body, int(r.text_index[k + 1] - r.text_index[k]))[1])
    return out


# --- 1. bit offsets ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("literal", [0, 1, 2, 3, 4, 5, 6, 7, "byte", "long"])
def test_every_left_bit_count_with_every_literal_bit_count(ctx, literal):
    st, _ = main_fixture()
    rows_a, rows_b = main_rows()
    r = concat(ctx, st, st, rows_a, rows_b, literals()[literal])  # (A == B: one store on both sides)
    assert r.res.n_failed == 0 and r.res.text_bytes == sum(len(t) for t in r.want.texts)


@pytest.mark.parametrize("sep", [b"", b"A", b"AC", b"ACG", b"ACGT", b"ACGTACGTA"])
def test_two_bit_codes_and_rows_that_end_on_byte_boundaries(ctx, sep):
    st, _ = dna_fixture()
    rng = np.random.default_rng(0xC07CA710)
    rows_a, rows_b = np.concatenate((np.arange(41), rng.integers(0, 41, size=159))), rng.integers(0, st.n, size=200)
    concat(ctx, st, st, rows_a, rows_b, sep)


@pytest.mark.parametrize("sep", [b"", bytes([100]), bytes([107]), bytes([131, 132, 100])])
def test_codewords_of_1_to_32_bits(ctx, sep):
    st = ladder_fixture()
    rows_a, rows_b = np.array([0, 1, 2, 3, 3, 0, 1, 2, 3]), np.array([3, 3, 3, 3, 0, 1, 2, 0, 1])
    concat(ctx, st, st, rows_a, rows_b, sep)


def test_whole_bytes_and_bytes_that_straddle(ctx):
    st, at = edge_fixture()
    names = ["few", "mid", "lane", "lane+1m"]
    rows = np.array([(at[a], at[b]) for a in names for b in names])
    for sep in (b"", b"\x01", b"\x07\x08", b"\x01\x09"):
        concat(ctx, st, st, rows[:, 0], rows[:, 1], sep)


# --- 2. empty pieces, many rows in one word ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("literal", [0, 3, "byte"])
def test_empty_and_raw_records_on_either_side(ctx, literal):
    st = empties_fixture()
    rows = np.array([(a, b) for a in range(st.n) for b in range(st.n)])
    sep = literals()[literal]
    r = concat(ctx, st, st, rows[:, 0], rows[:, 1], sep)
    # a record kept raw (no bytes under a length of 9) is the empty text on either side, as in the slice
    assert r.want.texts[3 * st.n + 1] == sep + stored_text(st, 1) and r.want.texts[1 * st.n + 3] == stored_text(st, 1) + sep and r.want.texts[3 * st.n + 3] == sep
    assert stored_rows(r, st.tab) == r.want.texts
    if literal == 0:
        assert int(r.body_index[1]) == 0 and int(r.text_index[1]) == 0  # both empty, no literal: the empty record


@pytest.mark.parametrize("run", [1, 40, 3000])
def test_runs_of_empty_rows_between_full_ones(ctx, run):
    st = empties_fixture()
    rows = empty_run_rows(run)
    concat(ctx, st, st, rows, rows[::-1].copy(), b"")


def test_many_rows_of_a_few_bits_in_one_word(ctx):
    st, _ = dna_fixture()
    rng = np.random.default_rng(0xC07CA720)
    small = np.arange(41, st.n)  # records of 1 .. 3 symbols
    rows_a, rows_b = rng.choice(np.concatenate((small, [0])), size=3000), rng.choice(np.concatenate((small, [0, 0, 0])), size=3000)
    r = concat(ctx, st, st, rows_a, rows_b, b"")
    assert int(np.diff(r.body_index.astype(np.int64)).max()) <= 2 and r.res.out_bytes > 3000
    for shift in (1, 15):
        concat(ctx, st, st, rows_a[:777], rows_b[:777], b"G", shift=shift)


# --- 3. tiles, paths, the scan ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shift", [1, 7, 8, 15])
def test_one_row_across_three_tiles_with_a_left_run_that_ends_mid_byte(ctx, shift):
    st, at = edge_fixture()
    r = concat(ctx, st, st, [at["few"], at["mid"], at["few"]], [at["few"], at["tiles"], at["mid"]], b"\x01\x02", shift=shift)
    assert int(r.body_index[2] - r.body_index[1]) > 2 * C + 4000 and r.d_out.data_ptr() % 16 == shift
    concat(ctx, st, st, [at["mid"]], [at["tiles"]], b"", tile_off=C - shift)


def test_left_bodies_on_both_sides_of_the_lane_threshold_and_over_a_block(ctx):
    st, at = edge_fixture()
    left = ["lane-1", "lane", "lane+1", "lane+2", "lane+1m", "block+", "block+m", "tiles"]
    rows_a = np.array([at[name] for name in left] * 2)
    rows_b = np.array([at["few"]] * len(left) + [at["mid"]] * len(left))
    for sep in (b"", b"\x01"):
        concat(ctx, st, st, rows_a, rows_b, sep)
    st, _ = main_fixture()
    concat(ctx, st, st, [13, 12, 13, 9, 8], [12, 13, 13, 8, 9], b" ")  # text under its own table: the long walk across blocks


def test_one_row_more_than_a_scan_tile(ctx):
    st, _ = dna_fixture()
    rng = np.random.default_rng(0xC07CA730)
    r = concat(ctx, st, st, rng.integers(0, st.n, size=SCAN_TILE + 1), rng.integers(0, st.n, size=SCAN_TILE + 1), b"T")
    assert r.res.n_failed == 0


# --- 4. row selection ---------------------------------------------------------------------------------------------------------------------------


def test_rows_repeated_reversed_and_absent(ctx):
    st, _ = main_fixture()
    dev = upload(st)
    sep = literals()[5]
    back = np.arange(st.n)[::-1].copy()
    concat(ctx, st, st, None, None, sep, dev_a=dev)  # d_rows == NULL on both sides: row k = record k + sep + record k
    concat(ctx, st, st, back, None, sep, dev_a=dev)
    concat(ctx, st, st, None, np.repeat(back[: st.n // 2], 2), sep, dev_a=dev)
    concat(ctx, st, st, np.full(50, 7), np.full(50, 11), sep, dev_a=dev)


def test_two_different_stores(ctx):
    st, texts = main_fixture()
    other = make_store(st.tab, [t[::-1] for t in texts[:12]])
    rng = np.random.default_rng(0xC07CA740)
    concat(ctx, st, other, rng.integers(0, st.n, size=100), rng.integers(0, other.n, size=100), b", ")
    concat(ctx, other, st, rng.integers(0, other.n, size=100), rng.integers(0, st.n, size=100), b"")


@pytest.mark.parametrize("literal", [0, 3, "byte"])
def test_an_absent_side_prefixes_or_suffixes_every_record(ctx, literal):
    st, texts = main_fixture()
    sep, dev = literals()[literal], upload(st)
    rows = np.random.default_rng(0xC07CA750).integers(0, st.n, size=120)
    r = concat(ctx, None, st, None, rows, sep, dev_b=dev)  # the prefix
    assert r.want.texts == [sep + texts[k] for k in rows]
    r = concat(ctx, st, None, rows, None, sep, dev_a=dev)  # the suffix
    assert r.want.texts == [texts[k] + sep for k in rows]
    r = concat(ctx, None, st, None, None, sep, dev_b=dev)
    if literal == 0:  # the right side alone, no literal: the take's identity
        assert np.array_equal(r.body_index, st.body_index) and np.array_equal(r.host[r.at : r.at + st.bodies.size], st.bodies)


# --- 5. hand-made bodies --------------------------------------------------------------------------------------------------------------------------


def test_set_pad_bits_are_masked_on_both_sides(ctx):
    own, texts = dna_fixture()
    st = right_pad_fixture()
    rows_a, rows_b = np.arange(st.n), np.arange(st.n)[::-1].copy()
    for A, B in ((st, st), (st, None), (None, st)):
        r = concat(ctx, A, B, rows_a if A else None, rows_b if B else None, b"C")
        assert np.array_equal(r.want.data, want_concat(A and own, B and own, rows_a if A else None, rows_b if B else None, b"C").data)  # the encoder's bytes
    st, _ = set_pad_fixture()
    own, _ = main_fixture()
    r = concat(ctx, st, st, [3, 5, 9, 12, 13, 1], [1, 2, 3, 4, 13, 12], b"")
    assert np.array_equal(r.want.data, want_concat(own, own, [3, 5, 9, 12, 13, 1], [1, 2, 3, 4, 13, 12], b"").data)


def test_bodies_that_end_before_their_length(ctx):
    st = cut_fixture()
    own, texts = main_fixture()
    rows = np.arange(st.n)
    r = concat(ctx, own, st, rows % own.n, rows, b"; ")  # cut on the right: the row holds what the body holds, whole codewords alone
    assert stored_rows(r, st.tab) == r.want.texts == [texts[k % own.n] + b"; " + stored_text(st, int(k)) for k in rows]
    assert all(len(t) < len(texts[k % own.n]) + 2 + int(st.text_index[k + 1] - st.text_index[k]) for k, t in zip(rows, r.want.texts))
    r = concat(ctx, st, own, rows, rows % own.n, b"; ")  # cut on the left
    assert stored_rows(r, st.tab) == r.want.texts == [stored_text(st, int(k)) + b"; " + texts[k % own.n] for k in rows]


# --- 6. failures, each alone ----------------------------------------------------------------------------------------------------------------------


def test_failures_stay_local_and_the_left_status_wins(ctx):
    st, bad = failures_store()
    st = with_table(st, table_255())
    dev = upload(st, spare=4096)  # (what lies behind body_bytes is mapped: a pair that is followed shows as wrong bytes)
    pairs = [(0, 1), (3, 1), (1, 3), (3, 14), (14, 3), (16, 2), (2, 0xFFFFFFFF), (14, 15), (6, 7), (8, 9), (11, 0), (0, 11), (15, 0), (5, 5), (12, 13)]
    rows_a, rows_b = (np.array(x, dtype=np.uint32) for x in zip(*pairs))
    want = want_concat(st, st, rows_a, rows_b, b"\x05")
    first = lambda r: bad.get(r, OK) if r < 16 else ARG  # noqa: E731  (what the take's test expects of these records)
    assert [int(s) for s in want.status] == [first(a) or first(b) for a, b in pairs] and want.status[3] == ARG and want.status[4] == UNSUPPORTED
    r = check_take(run_concat(ctx, st, st, rows_a, rows_b, b"\x05", want.total, dev_a=dev), want)
    assert r.res.n_failed == int((want.status != OK).sum()) == 11 and (r.res.first_failed, r.res.first_status) == (1, ARG)


def test_a_new_length_at_the_limit_passes_and_one_above_fails(ctx):
    """Texts of the limit's size are walked by workgroups: the rows above it are failed by k_concat_long, each once."""
    st, small = limit_fixture()
    dev = upload(st)
    r = concat(ctx, st, st, [0, 0, 0, 3, 1, 2], [1, 2, 0, 3, 0, 0], b"AC", dev_a=dev)
    assert [int(s) for s in r.status] == [OK, UNSUPPORTED, OK, UNSUPPORTED, OK, UNSUPPORTED] and int(r.text_index[1]) == small
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 1, UNSUPPORTED)
    r = concat(ctx, None, st, None, [3, 0, 3], b"", dev_b=dev)
    assert r.res.n_failed == 0 and int(r.text_index[1]) == small
    r = concat(ctx, st, None, [3, 0, 3], None, b"A", dev_a=dev)
    assert [int(s) for s in r.status] == [UNSUPPORTED, OK, UNSUPPORTED] and (r.res.n_failed, r.res.first_failed) == (2, 0)


# --- 7. capacity ------------------------------------------------------------------------------------------------------------------------------------


def test_a_capacity_one_short_writes_nothing_and_sizes_only_writes_no_byte(ctx):
    st, _ = main_fixture()
    rows_a, rows_b = main_rows()
    sep = literals()[3]
    want = want_concat(st, st, rows_a[:100], rows_b[:100], sep)
    dev = upload(st)
    r = check_take(run_concat(ctx, st, st, rows_a[:100], rows_b[:100], sep, want.total - 1, dev_a=dev), want, call_status=CAP)
    assert r.res.out_bytes == want.total
    check_take(run_concat(ctx, st, st, rows_a[:100], rows_b[:100], sep, want.total, dev_a=dev, sizes_only=True), want)
    check_take(run_concat(ctx, st, st, rows_a[:100], rows_b[:100], sep, want.total + 100, dev_a=dev, shift=5), want)


# --- 8. with the neighbouring calls -------------------------------------------------------------------------------------------------------------------


def test_field_concat_join_on_one_context(ctx):
    """encode_packed of CSV lines and of a key set of user=<id> -> field 2 -> concat("user=", .) -> join against the keys: nothing is
    synchronised in between, and no text appears."""
    import torch

    import entreepy_amd as E

    rng = np.random.default_rng(0xC07CA760)
    users = [b"u%03d" % i for i in range(300)]
    lines = [b"get,%d," % i + users[int(rng.integers(0, 300))] + b",ok" if i % 4 else b"put,%d" % i for i in range(2000)]
    keys = [b"user=" + u for u in users[::3]]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(lines + keys), np.uint8), minlength=256))
    sides = []
    for column in (keys, lines):
        index = _index_of([len(w) for w in column])
        d_text, d_index = _dev_bytes(np.frombuffer(b"".join(column), np.uint8)), _dev_index(index)
        d_out = torch.empty(cb.body_bound(int(index[-1])) + len(column), dtype=torch.uint8, device="cuda")
        sides.append((d_out, torch.empty(len(column) + 1, dtype=torch.int64, device="cuda"), d_index, d_text))
    n = len(lines)
    d_hits, d_key = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    d_ids, d_new = (torch.full((LEAD + 24 * n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")[LEAD:] for _ in range(2))
    d_bi, d_ti, d_nbi, d_nti = (torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(4))
    torch.cuda.synchronize()
    enc = [ctx.encode_packed_device(cb, s[3], s[2], s[0], s[1]) for s in sides]
    key_store, line_store = ((s[0][: e.out_bytes], s[1], s[2]) for s, e in zip(sides, enc))
    f = ctx.field_packed_device(cb, *line_store, None, 2, 1, b",", d_ids[: 24 * n], d_bi, d_ti)
    c = ctx.concat_packed_device(cb, None, b"user=", (d_ids[: max(f.out_bytes, 1)], d_bi, d_ti), d_new[: 24 * n], d_nbi, d_nti)
    j = ctx.join_packed_device(cb, d_new[: max(c.out_bytes, 1)], d_nbi, d_nti, *key_store, rows=d_hits, key_of_row=d_key)
    torch.cuda.synchronize()
    made = [b"user=" + (l.split(b",")[2] if l.count(b",") >= 2 else b"") for l in lines]
    hits = [k for k, m in enumerate(made) if m in set(keys)]
    assert 0 < len(hits) < n and all(e.status == OK and e.n_failed == 0 for e in enc) and (f.status, f.n_failed) == (OK, 0)
    assert (c.status, c.n_failed, c.text_bytes) == (OK, 0, sum(len(m) for m in made)) and _guards_intact(d_new, c.out_bytes)
    tab = (np.array(cb.raw.data, dtype=np.uint32), np.array(cb.raw.length, dtype=np.uint8))
    assert d_new[: c.out_bytes].cpu().numpy().tobytes() == b"".join(want_encode(tab, m)[1] for m in made)
    assert (j.status, j.n_failed, j.n_keys_failed) == (OK, 0, 0) and d_hits[: j.n_match].tolist() == hits
    assert d_key[: j.n_match].tolist() == [keys.index(made[k]) for k in hits]


def test_list_helper_returns_the_store_of_the_concatenated_texts(ctx):
    import entreepy_amd as E

    _, texts = main_fixture()
    texts = texts[:30]
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(texts), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb, texts)
    store = (blob, out_index, [len(t) for t in texts])
    rng = np.random.default_rng(0xC07CA770)
    rows_a, rows_b = rng.integers(0, 30, size=90), rng.integers(0, 30, size=90)
    for a, b, ra, rb, want in ((store, store, rows_a, rows_b, [texts[x] + b" and " + texts[y] for x, y in zip(rows_a, rows_b)]),
                               (store, store, None, None, [t + b" and " + t for t in texts]), (None, store, None, rows_b, [b" and " + texts[y] for y in rows_b]),
                               (store, None, rows_a, None, [texts[x] + b" and " for x in rows_a])):
        new_blob, new_index, new_lengths = ctx.concat_packed(cb, a, b" and ", b, rows_a=ra, rows_b=rb)
        assert [int(x) for x in new_lengths] == [len(w) for w in want]
        assert (new_blob, new_index.tolist()) == (lambda bl, i: (bl, i.tolist()))(*ctx.encode_packed(cb, want))
        assert ctx.decode_packed(cb, new_blob, new_index, new_lengths) == want
    assert ctx.concat_packed(cb, store, b"", store, rows_a=[], rows_b=[])[0] == b""
    with pytest.raises(E.EntreepyError, match="row 1") as e:
        ctx.concat_packed(cb, store, b"-", store, rows_a=[3, 4, 0], rows_b=[0, 30, 1])
    assert e.value.status == ARG
    with pytest.raises(E.EntreepyError) as e:  # a literal byte without a code: the call's own status
        ctx.concat_packed(cb, store, b"\xff\x00", store)
    assert e.value.status == UNSUPPORTED


# --- 9. the state a context keeps between calls ---------------------------------------------------------------------------------------------------
# The cells of tests/test_gpu_retained.py for the row `concat` (tests/retained_concat.py): a concat between the call that sets a state
# and the calls that read it leaves the histogram link, the held range and the last codebook as they were.


@pytest.mark.parametrize("reader", ["body", "head", "on_host"])
def test_histogram_link_survives_a_concat(reader):
    from tests import test_gpu_retained as G

    G.test_histogram_link("concat", reader)


@pytest.mark.parametrize("how", ["sync", "maps", "between", "windows"])
def test_held_range_survives_a_concat(how):
    from tests import test_gpu_retained as G

    G.test_held_range("concat", how)


def test_last_codebook_survives_a_concat():
    from tests import test_gpu_retained as G

    G.test_last_codebook("concat")
