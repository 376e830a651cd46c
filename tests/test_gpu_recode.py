"""GPU: et_recode_packed_device -- a selection's records walked under table IN, every byte sent through a 256-entry map (or dropped) and
written under table OUT as a new packed store, no text in between -- against the oracle: a row's status is judged from its record's own
two pairs of offsets, its stored text is want_decode's under table IN, the translation is Python's bytes.translate, and the expected
bytes are the oracle's shared-table encode of that under table OUT (want_recode()); never the bit rule the kernels implement.  d_out
lies between sentinel bytes as in tests/test_gpu_take.py, whose check_take() compares bytes, both offset arrays, the status bytes and
the report.

The stores, tables and maps are made by the *_fixture functions below, without a GPU: tests/test_recode_host.py checks on the same
fixtures that the bit rule gives what the oracle gives, and that they reach the cases named here."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus, limits
from tests import retained_recode  # noqa: F401  (the call's row joins the table of tests/retained.py)
from tests.test_gpu_batch import SENTINEL, _small_max
from tests.test_gpu_concat import dna_fixture, edge_fixture, empties_fixture
from tests.test_gpu_gather import dev_rows, make_store, upload
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_gpu_shared import _cb, want_encode
from tests.test_gpu_slice import BLOCK_BITS, LANE_BITS, TO_END, bit_at, cut_fixture, ladder_fixture, main_fixture, pad_fixture, run_slice, set_pad_fixture, stored_text
from tests.test_gpu_take import C, LEAD, SCAN_TILE, SELECTIONS, _guards_intact, check_take, failures_store, selection
from tests.test_shared_host import canonical, oracle_table, table_255, table_2bit, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
DROP = -1  # ET_RECODE_DROP
ROUND_BITS = 16384 * 8  # destination bits per flush of the long write (csrc/et_batch.h RECODE_ROUND_BITS)
IDENTITY = np.arange(256, dtype=np.int16)


def lane_bytes():
    """A body whose reach() is up to this many bytes is walked by its row's lane, a longer one by a workgroup."""
    from entreepy_amd import _native as N

    return int(N.lib().et_recode_lane_bytes())


def reach(st, r):
    """What the walk of record r can touch of its body: min(bytes, 4 * length + 8) (csrc/et_batch.h clip_body)."""
    nb, length = int(st.body_index[r + 1] - st.body_index[r]), int(st.text_index[r + 1] - st.text_index[r])
    return min(nb, 4 * length + 8)


def a_map(frm=b"", to=b"", delete=b""):
    """bytes.maketrans plus deletions as 256 int16 values -- made here, not by the package's byte_map(), which is under test."""
    m = IDENTITY.copy()
    m[list(frm)] = list(to)
    m[list(delete)] = DROP
    return m


UPPER = a_map(bytes(range(97, 123)), bytes(range(65, 91)))
LOWER = a_map(bytes(range(65, 91)), bytes(range(97, 123)))


def translate(text, bmap):
    """Python's answer: text.translate(table, delete)."""
    if bmap is None:
        return text
    m = np.asarray(bmap)
    return text.translate(bytes(int(x) if x >= 0 else 0 for x in m), bytes(c for c in range(256) if m[c] < 0))


# --- the expected store: the oracle's texts under table IN, Python's translate, the oracle's encode under table OUT ---------------------


def want_recode(st, tab_out, rows, bmap=None):
    """-> what tests/test_gpu_take.py's model() returns, for the recoded rows; .texts: the rows' new texts."""
    small, body_bytes = _small_max(), st.bodies.size
    rows = np.arange(st.n) if rows is None else np.asarray(rows, dtype=np.int64)
    memo = {}
    status, nb, ln, pieces, texts = np.full(rows.size, ARG, np.uint8), np.zeros(rows.size, np.uint64), np.zeros(rows.size, np.uint64), [], []
    for k, r in enumerate(int(r) for r in rows):
        texts.append(b"")
        if r >= st.n:
            continue
        b0, b1, t0, t1 = (int(x) for x in (st.body_index[r], st.body_index[r + 1], st.text_index[r], st.text_index[r + 1]))
        if not (b0 <= b1 <= body_bytes and t0 <= t1):
            continue
        if t1 - t0 > small or b1 - b0 > 4 * small:
            status[k] = UNSUPPORTED
            continue
        if r not in memo:
            t = translate(stored_text(st, r), bmap)
            rc, body = want_encode(tab_out, t)  # (UNSUPPORTED: a kept byte without a code under table OUT)
            assert rc in (OK, UNSUPPORTED)
            memo[r] = (rc, t if rc == OK else b"", np.frombuffer(body, np.uint8))
        status[k], texts[k], body = memo[r]
        nb[k], ln[k] = body.size, len(texts[k])
        pieces.append(body)
    data = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    return SimpleNamespace(status=status, body_index=_index_of(nb), text_index=_index_of(ln), data=data, total=int(nb.sum()), text_total=int(ln.sum()), texts=texts)


# --- the fixtures ----------------------------------------------------------------------------------------------------------------------


def other_table(tab):
    """A second complete table over the same symbols, from the histogram turned upside down: what was frequent is rare."""
    from oracle import oracle as O

    length = tab[1].astype(np.int64)
    weight = np.where(length > 0, (1 << np.minimum(length, 40)), 0).astype(np.uint64)  # (a symbol of a long code is made frequent)
    data, new_length, _ = O.build_dict(weight)
    assert (new_length > 0).tolist() == (length > 0).tolist()
    return data, new_length


@functools.lru_cache(maxsize=None)
def main_tables():
    """The main fixture's table T1 (of its own bytes), T2 over the same symbols from another histogram, and TU: the table of the
    upper-cased text's own bytes -> {name: table}."""
    st, texts = main_fixture()
    pool = np.frombuffer(b"".join(texts), np.uint8)
    return {"T1": st.tab, "T2": other_table(st.tab), "TU": oracle_table(np.frombuffer(pool.tobytes().upper(), np.uint8))}


def retabled(st, tab):
    """The same texts (the stored texts of `st`) as a store under `tab`."""
    return make_store(tab, [stored_text(st, r) for r in range(st.n)])


@functools.lru_cache(maxsize=None)
def table_reddal():
    """The ladder's symbols under reversed weights: byte 132 has 1 bit, ..., bytes 101 and 100 have 32."""
    return canonical({100 + i: min(33 - i, 32) for i in range(33)})


@functools.lru_cache(maxsize=None)
def ladder_back_fixture():
    """The ladder fixture's texts under the reversed ladder."""
    return retabled(ladder_fixture(), table_reddal())


PHASE_MAP = a_map(b"\x01\x03", b"\x02\x01")  # under table_255 both ways: the 7-bit byte becomes an 8-bit one, byte 3 the 7-bit one


@functools.lru_cache(maxsize=None)
def phase_fixture():
    """Under table_255 (byte 1: 7 bits, every other: 8): 128 records -- a ones and c threes among other bytes, a, c = 0 .. 7, once in a
    body a lane walks and once in a longer one: the input has -a bits mod 8, the output through PHASE_MAP -c -> (store, {(a, c, long): record})."""
    rng = np.random.default_rng(0x4EC0DE01)
    texts, at = [], {}
    for long in (False, True):
        for a in range(8):
            for c in range(8):
                n = int(rng.integers(700, 1500)) if long else int(rng.integers(0, 60))
                t = np.concatenate((rng.integers(4, 256, size=n, dtype=np.uint8), np.full(a, 1, np.uint8), np.full(c, 3, np.uint8)))
                at[a, c, long] = len(texts)
                texts.append(rng.permutation(t).tobytes())
    return make_store(table_255(), texts), at


@functools.lru_cache(maxsize=None)
def expansion_fixture():
    """Under the ladder (byte 100: 1 bit): 0 = 65 536 + 3 symbols of one bit, one 8 KiB block and 3 bits, which the reversed ladder
    turns into 32 bits each: 256 KiB; 1 = et_batch_small_max() of them: 1 MiB, the largest body there is; 2 = a mixture with every
    length, for the bits in between -> store."""
    t = limits.ladder32()
    return make_store(table_ladder(), [bytes([100]) * (BLOCK_BITS + 3), bytes([100]) * _small_max(), limits.uniform(t, 3000).tobytes()])


@functools.lru_cache(maxsize=None)
def contraction_fixture():
    """The reverse: the first and the last record of the expansion fixture under the reversed ladder, 32 bits a symbol: 256 KiB that
    become 8 KiB -> store."""
    texts = [bytes([100]) * (BLOCK_BITS + 3), limits.uniform(limits.ladder32(), 3000).tobytes()]
    return make_store(table_reddal(), texts)


@functools.lru_cache(maxsize=None)
def length_fixture():
    """The main fixture's longest record (a body of 2.7 blocks) again and again, the body whole and the LENGTH cut: the stored text ends
    with the length -- on a lane's first codeword and on its last, around a lane's edge, in block 0, 1 and 2, around both block edges
    -> (store, {name: record})."""
    st, texts = main_fixture()
    r = 13
    text = texts[r]
    body = st.bodies[int(st.body_index[r]) : int(st.body_index[r + 1])].tobytes()
    starts = bit_at(st, r, 0) + np.concatenate(([0], np.cumsum(st.tab[1][np.frombuffer(text, np.uint8)].astype(np.int64))))
    first_of = lambda bit: int(np.searchsorted(starts, bit))  # noqa: E731  the first symbol that begins at or behind `bit`
    lane, block1, block2 = first_of(40 * LANE_BITS), first_of(BLOCK_BITS), first_of(2 * BLOCK_BITS)
    cuts = {"lane_first": lane, "lane_last": first_of(41 * LANE_BITS) - 1, "lane_first+1": lane + 1, "lane_first-1": lane - 1, "block0": block1 - 500, "block1_first": block1,
            "block1_first-1": block1 - 1, "block1_first+1": block1 + 1, "block1": block2 - 500, "block2_first": block2, "block2_first-1": block2 - 1, "block2": len(text) - 7,
            "one": 1, "whole": len(text), "beyond": len(text) + 100}
    keep = [text[:n] + b"\x00" * max(n - len(text), 0) for n in cuts.values()]  # (make_store takes the lengths from these)
    return make_store(st.tab, keep, [body] * len(keep)), {name: i for i, name in enumerate(cuts)}


TAB_NO_A, TAB_NO_T = canonical({ord("C"): 1, ord("G"): 2, ord("T"): 2}), canonical({ord("A"): 1, ord("C"): 2, ord("G"): 2})


@functools.lru_cache(maxsize=None)
def behind_fixture():
    """Under the 2-bit table -> store: texts of C, G and T whose bodies go on with codewords of A BEHIND the length -- 0 a lane's, 1 a
    workgroup's --, 2 and 3 the same with one A inside the stored text, as its last symbol."""
    rng = np.random.default_rng(0x4EC0DE02)
    texts, bodies = [], []
    for n, inside in ((41, False), (3001, False), (41, True), (3001, True)):
        t = bytes(rng.choice(np.frombuffer(b"CGT", np.uint8), size=n).tobytes()) + (b"A" if inside else b"")
        texts.append(t)
        bodies.append(want_encode(table_2bit(), t + b"AAAGAAAA" * 9)[1])
    return make_store(table_2bit(), texts, bodies)


@functools.lru_cache(maxsize=None)
def drop_fixture():
    """Under the 2-bit table -> (store, [texts]): A in front of a run of C, G and T, behind it, on both ends, alone, and runs whose
    kept symbols are a multiple of four (whole bytes once the A's are gone); short and long."""
    rng = np.random.default_rng(0x4EC0DE03)
    run = lambda n: bytes(rng.choice(np.frombuffer(b"CGT", np.uint8), size=n).tobytes())  # noqa: E731
    texts = []
    for n in (5, 8, 3000, 3001):
        texts += [b"A" + run(n), run(n) + b"A", b"A" + run(n) + b"A", run(n // 2) + b"AAA" + run(n - n // 2)]
    texts += [b"A", b"AAAAAAA", b"A" * 4000, b""]
    return make_store(table_2bit(), texts), texts


def with_table(st, tab):
    """The store's bytes read under another table."""
    return SimpleNamespace(tab=tab, cb=_cb(tab), bodies=st.bodies, body_index=st.body_index, text_index=st.text_index, n=st.n)


# --- one call and its check ------------------------------------------------------------------------------------------------------------


def run_recode(ctx, st, tab_out, dev, rows, bmap, cap, sizes_only=False, shift=0, tile_off=None):
    """One call, every output full of sentinels first (tests/test_gpu_take.py's run_take).  rows=None: d_rows == NULL."""
    import torch

    d_bodies, d_body_index, d_text_index = dev
    n = st.n if rows is None else len(rows)
    r = SimpleNamespace(cap=cap, sizes_only=sizes_only)
    r.d_raw = torch.full((3 * C + LEAD + 16 + cap + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert r.d_raw.data_ptr() % 16 == 0
    r.at = LEAD + shift if tile_off is None else (-r.d_raw.data_ptr()) % C + C + tile_off
    r.d_out = r.d_raw[r.at : r.at + max(cap, 1)]
    r.d_body_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_text_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    r.d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.res = ctx.recode_packed_device(st.cb, _cb(tab_out), d_bodies, d_body_index, d_text_index, None if rows is None else dev_rows(rows), None if sizes_only else r.d_out,
                                     r.d_body_index, r.d_text_index, byte_map=bmap, status=r.d_status)
    torch.cuda.synchronize()
    r.host = r.d_raw.cpu().numpy()
    r.body_index, r.text_index = r.d_body_index.cpu().numpy().view(np.uint64), r.d_text_index.cpu().numpy().view(np.uint64)
    r.status = r.d_status.cpu().numpy()
    return r


def recode(ctx, st, tab_out, rows=None, bmap=None, dev=None, **kw):
    """Run with cap = the need exactly, and check."""
    want = want_recode(st, tab_out, rows, bmap)
    r = check_take(run_recode(ctx, st, tab_out, dev or upload(st), rows, bmap, want.total, **kw), want)
    r.want = want
    return r


def guarded(size):
    """`size` bytes of output and TAIL more, all sentinels, LEAD sentinel bytes in front: what _guards_intact() looks at."""
    import torch

    return torch.full((LEAD + size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")[LEAD:]


def out_bytes_of(r):
    return r.host[r.at : r.at + r.want.total].tobytes()


# --- 1. bit counts and tables --------------------------------------------------------------------------------------------------------------


def test_every_output_bit_count_against_every_input_bit_count_on_both_paths(ctx):
    st, at = phase_fixture()
    r = recode(ctx, st, table_255(), None, PHASE_MAP)
    assert r.res.n_failed == 0 and r.res.text_bytes == int(st.text_index[-1])
    recode(ctx, st, table_255(), np.random.default_rng(0x4EC0DE10).permutation(st.n), PHASE_MAP)  # ... and with other neighbours in the output


@pytest.mark.parametrize("tables", ["T1>T2", "T2>T1", "T1>TU upper", "T1>T1 lower", "T2>TU upper"])
def test_a_table_change_a_map_and_both_at_once(ctx, tables):
    st, _ = main_fixture()
    T = main_tables()
    src, dst = tables.split()[0].split(">")
    bmap = {"upper": UPPER, "lower": LOWER}.get(tables.split()[-1])
    store = st if src == "T1" else retabled(st, T[src])
    r = recode(ctx, store, T[dst], None, bmap)
    assert r.res.n_failed == 0 and r.want.texts == [translate(stored_text(st, k), bmap) for k in range(st.n)]
    if bmap is None:  # re-tabling gives the store the encoder writes under the other table
        other = st if dst == "T1" else retabled(st, T[dst])
        assert np.array_equal(r.want.data, other.bodies) and np.array_equal(r.body_index, other.body_index)


def test_the_2_bit_table(ctx):
    st, texts = dna_fixture()
    complement = a_map(b"ACGT", b"TGCA")
    for bmap in (None, complement, a_map(b"A", b"C"), a_map(delete=b"G")):
        r = recode(ctx, st, table_2bit(), None, bmap)
        assert r.want.texts == [translate(t, bmap) for t in texts]
    recode(ctx, st, TAB_NO_A, None, a_map(b"A", b"T"))  # 2-bit codes become 1- and 2-bit ones


@pytest.mark.parametrize("way", ["ladder>reversed", "reversed>ladder", "ladder>ladder", "reversed>reversed rotated"])
def test_codewords_of_1_to_32_bits_become_codewords_of_32_to_1(ctx, way):
    src, dst = way.split()[0].split(">")
    stores, tabs = {"ladder": ladder_fixture(), "reversed": ladder_back_fixture()}, {"ladder": table_ladder(), "reversed": table_reddal()}
    bmap = a_map(bytes(range(100, 133)), bytes(range(101, 133)) + b"\x64") if "rotated" in way else None  # every symbol takes its neighbour's length
    r = recode(ctx, stores[src], tabs[dst], None, bmap)
    assert r.res.n_failed == 0
    if bmap is None:
        assert np.array_equal(r.want.data, stores[dst].bodies)
    recode(ctx, stores[src], tabs[dst], [0, 3, 3, 1, 0, 2, 3], bmap)


def test_table_255_to_a_text_table_and_back(ctx):
    st, at = edge_fixture()
    rows = [at[n] for n in ("few", "mid", "lane", "lane+1m", "block+m", "tiles", "few")]
    wide = oracle_table(np.concatenate([np.frombuffer(stored_text(st, r), np.uint8) for r in range(st.n)] + [np.arange(1, 256, dtype=np.uint8)]))
    r = recode(ctx, st, wide, rows)
    assert r.res.n_failed == 0
    back = recode(ctx, retabled(st, wide), table_255(), rows)
    assert np.array_equal(back.want.data, want_recode(st, table_255(), rows).data)


# --- 2. expansion and contraction ------------------------------------------------------------------------------------------------------------


def test_expansion_one_block_of_1_bit_codes_becomes_256_kib(ctx):
    st = expansion_fixture()
    r = recode(ctx, st, table_reddal(), [2, 0, 2])
    sizes = np.diff(r.body_index).astype(np.int64)
    assert sizes[1] == 4 * (BLOCK_BITS + 3) and r.res.n_failed == 0
    assert out_bytes_of(r)[int(r.body_index[1]) : int(r.body_index[2])] == (table_reddal()[0][100].item().to_bytes(4, "big")) * (BLOCK_BITS + 3)


def test_expansion_at_the_small_stream_limit(ctx):
    st = expansion_fixture()
    r = recode(ctx, st, table_reddal(), [1])
    assert r.res.out_bytes == 4 * _small_max() and r.res.text_bytes == _small_max()


def test_contraction_256_kib_become_8_kib(ctx):
    st = contraction_fixture()
    assert int(st.body_index[1]) == 4 * (BLOCK_BITS + 3)
    r = recode(ctx, st, table_ladder(), [1, 0, 1, 0])
    assert int(r.body_index[2] - r.body_index[1]) == (BLOCK_BITS + 3 + 7) // 8 and r.res.n_failed == 0
    assert np.array_equal(r.want.data[int(r.body_index[1]) : int(r.body_index[2])], expansion_fixture().bodies[: int(expansion_fixture().body_index[1])])


# --- 3. thresholds, blocks, lanes ------------------------------------------------------------------------------------------------------------


def test_bodies_around_the_lane_threshold(ctx):
    st, at = edge_fixture()
    rows = [at[n] for n in ("lane-1", "lane", "lane+1", "lane+2", "lane+1m", "lane+2", "lane+1", "lane", "lane-1")]
    shifted = a_map(bytes(range(2, 256)), bytes(range(3, 256)) + b"\x01")  # the 7-bit codeword comes from byte 255, byte 1 takes 8 bits
    for bmap in (None, shifted, a_map(delete=b"\x07")):
        recode(ctx, st, table_255(), rows, bmap)


def test_the_length_ends_the_stored_text_in_every_block_and_at_the_lanes_edges(ctx):
    st, at = length_fixture()
    T = main_tables()
    r = recode(ctx, st, T["T2"])
    lens = [int(x) for x in np.diff(r.text_index)]
    assert lens[at["lane_first"]] + 1 == lens[at["lane_first+1"]] and lens[at["beyond"]] >= lens[at["whole"]] == 40000 and lens[at["one"]] == 1
    recode(ctx, st, T["TU"], np.arange(st.n)[::-1], UPPER)


# --- 4. drops --------------------------------------------------------------------------------------------------------------------------------


def test_dropped_symbols_at_the_ends_and_whole_bytes(ctx):
    st, texts = drop_fixture()
    r = recode(ctx, st, table_2bit(), None, a_map(delete=b"A"))
    assert r.want.texts == [t.replace(b"A", b"") for t in texts] and r.res.n_failed == 0
    assert [int(x) for x in np.diff(r.text_index)[-4:]] == [0, 0, 0, 0]  # nothing but dropped symbols: the empty record, ET_OK
    r = recode(ctx, st, TAB_NO_A, None, a_map(delete=b"A"))  # the dropped byte has no code under table OUT: it is dropped
    assert r.res.n_failed == 0 and not r.status.any()
    recode(ctx, st, table_2bit(), None, a_map(b"C", b"T", delete=b"AG"))


def test_every_symbol_dropped(ctx):
    st, _ = main_fixture()
    r = recode(ctx, st, main_tables()["T2"], None, np.full(256, DROP, np.int16))
    assert (r.res.status, r.res.out_bytes, r.res.text_bytes, r.res.n_failed) == (OK, 0, 0, 0) and bool((r.host == SENTINEL).all())


# --- 5. kept and uncoded ---------------------------------------------------------------------------------------------------------------------


def test_a_kept_byte_without_a_code_fails_its_row_alone_on_both_paths(ctx):
    st, texts = pad_fixture()  # 0 .. 5: no A, the zero pad reads as A; 6 .. 11: no T, the set pad reads as T; short and long of each
    r = recode(ctx, st, TAB_NO_A)
    assert r.status.tolist() == [UNSUPPORTED if b"A" in t else OK for t in texts] and r.status[:6].tolist() == [OK] * 6 and r.status[9:].tolist() == [UNSUPPORTED] * 3
    rows = [11, 0, 6, 3, 9, 5, 7]
    r = recode(ctx, st, TAB_NO_T, rows)
    assert r.status.tolist() == [UNSUPPORTED if b"T" in texts[k] else OK for k in rows] and r.status[[0, 2, 4, 6]].tolist() == [OK] * 4 and r.status[[3, 5]].tolist() == [UNSUPPORTED] * 2
    for k in np.flatnonzero(r.status):  # a failed row is the empty record
        assert r.body_index[k] == r.body_index[k + 1] and r.text_index[k] == r.text_index[k + 1]
    r = recode(ctx, st, TAB_NO_A, None, a_map(b"A", b"C"))  # mapped to a byte with a code, nothing fails
    assert r.res.n_failed == 0


def test_the_same_codeword_behind_the_length_fails_nothing(ctx):
    st = behind_fixture()
    r = recode(ctx, st, TAB_NO_A)
    assert r.status.tolist() == [OK, OK, UNSUPPORTED, UNSUPPORTED] and [int(x) for x in np.diff(r.text_index)] == [41, 3001, 0, 0]
    r = recode(ctx, st, table_2bit())  # ... and is no symbol of the new record
    assert [int(x) for x in np.diff(r.text_index)] == [41, 3001, 42, 3002]


# --- 6. odd records --------------------------------------------------------------------------------------------------------------------------


def test_set_pad_bits_are_cleared_and_cut_bodies_give_what_they_hold(ctx):
    T = main_tables()
    st, _ = set_pad_fixture()
    own, _ = main_fixture()
    r = recode(ctx, st, T["T1"])  # the identity normalises the store
    assert np.array_equal(r.want.data, own.bodies) and not np.array_equal(st.bodies, own.bodies)
    recode(ctx, st, T["TU"], None, UPPER)
    st = cut_fixture()
    r = recode(ctx, st, T["T2"])
    stored = [len(stored_text(st, k)) for k in range(st.n)]
    assert [int(x) for x in np.diff(r.text_index)] == stored and all(s < l for s, l in zip(stored, np.diff(st.text_index).astype(np.int64)))  # lengths cut to what the bodies hold


def test_raw_and_empty_records_and_a_run_of_5000_empty_results(ctx):
    st = empties_fixture()  # 0 the empty record; 3 no bytes under a length of 9
    T = main_tables()
    r = recode(ctx, st, T["T2"], [3, 1, 0, 2, 3, 4, 0])
    assert [int(x) for x in np.diff(r.text_index)][0::2] == [0, 0, 0, 0] and r.res.n_failed == 0
    empty = np.where(np.arange(5000) % 3 == 2, 3, 0)
    for rows in (np.concatenate(([1], empty, [2])), np.concatenate((empty, [1, 2])), np.concatenate(([2, 1], empty))):
        r = recode(ctx, st, T["T2"], rows)
        assert int(np.count_nonzero(np.diff(r.body_index))) == 2
    r = recode(ctx, st, T["T2"], empty)
    assert r.res.out_bytes == 0 and bool((r.host == SENTINEL).all())


def test_3000_rows_of_a_few_bits_share_destination_words(ctx):
    st, texts = dna_fixture()
    rows = 41 + np.random.default_rng(0x4EC0DE20).integers(0, 60, size=3000)  # 1 .. 3 symbols: a byte each
    r = recode(ctx, st, TAB_NO_T, rows, a_map(b"T", b"A"))
    assert r.res.out_bytes == 3000
    lad = ladder_fixture()
    recode(ctx, lad, table_reddal(), np.full(3000, 3))  # 18 symbols of 32 bits become 18 of 1 and 2


@pytest.mark.parametrize("n_rows", [1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_scan_edges(ctx, n_rows):
    st, _ = main_fixture()
    rows = np.random.default_rng(0x4EC0DE30 + n_rows).integers(1, 9, size=n_rows)
    recode(ctx, st, main_tables()["TU"], rows, UPPER)


@pytest.mark.parametrize("name", SELECTIONS)
def test_rows_in_every_order_with_repeats_and_null(ctx, name):
    st, _ = main_fixture()
    T = main_tables()
    with_rows = recode(ctx, st, T["T2"], selection(name, st.n), LOWER)
    if name == "identity":
        without = recode(ctx, st, T["T2"], None, LOWER)
        assert without.res == with_rows.res and out_bytes_of(without) == out_bytes_of(with_rows)


# --- 7. alignment and offsets ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shift", range(16))
def test_every_output_base_and_body_alignment(ctx, shift):
    import torch

    st, _ = main_fixture()
    d = torch.full((shift + st.bodies.size + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
    d[shift : shift + st.bodies.size] = torch.from_numpy(st.bodies).cuda()
    dev = (d[shift : shift + st.bodies.size], _dev_index(st.body_index), _dev_index(st.text_index))
    assert d.data_ptr() % 16 == 0 and dev[0].data_ptr() % 16 == shift
    rows = np.random.default_rng(0x4EC0DE40 + shift).integers(0, st.n, size=120)
    r = recode(ctx, st, main_tables()["TU"], rows, UPPER, dev=dev, shift=shift)
    assert r.d_out.data_ptr() % 16 == shift
    recode(ctx, st, main_tables()["T2"], [13, 0, 2, 1, 13], None, dev=dev, shift=shift)


@pytest.mark.parametrize("shift", [1, 7, 8, 15])
def test_a_long_row_across_the_write_rounds_at_odd_addresses(ctx, shift):
    st = expansion_fixture()
    r = recode(ctx, st, table_reddal(), [2, 0], shift=shift)
    assert r.d_out.data_ptr() % 16 == shift
    assert int(r.body_index[2] - r.body_index[1]) * 8 > 15 * ROUND_BITS
    recode(ctx, contraction_fixture(), table_ladder(), [1, 0], shift=shift)


def test_offsets_above_4_gib(ctx):
    import torch

    page_len = 256 << 10
    rng = np.random.default_rng(0x4EC0DE50)
    text = rng.integers(2, 256, size=page_len, dtype=np.uint8)
    text[:5] = 1  # five 7-bit codewords: every byte behind them straddles two source bytes
    tab_in, bmap = table_255(), a_map(bytes(range(2, 256)), bytes(range(3, 256)) + b"\x02")
    tab_out = canonical({3: 7, **{s: 8 for s in range(1, 256) if s != 3}})
    body = np.frombuffer(want_encode(tab_in, text)[1], np.uint8)
    piece = np.frombuffer(want_encode(tab_out, translate(text.tobytes(), bmap))[1], np.uint8)  # what every long row becomes
    small_text = text[:9].tobytes()
    small_body = np.frombuffer(want_encode(tab_in, small_text)[1], np.uint8)
    small = np.frombuffer(want_encode(tab_out, translate(small_text, bmap))[1], np.uint8)
    L, P = body.size, piece.size
    assert page_len <= _small_max() and P != L
    d_two = torch.from_numpy(np.concatenate((small_body, body))).cuda()  # record 0: the few bytes; record 1: the page
    two_bi, two_ti = _dev_index([0, small_body.size, small_body.size + L]), _dev_index([0, 9, 9 + page_len])
    d_piece = torch.from_numpy(piece.copy()).cuda()
    cb_in, cb_out = _cb(tab_in), _cb(tab_out)
    # output: one record n_pages times behind one row of a few bytes, so that a row straddles 2^32
    n_pages = (1 << 32) // P + 3
    total = small.size + n_pages * P
    n_rows = n_pages + 1
    d_rows = torch.ones(n_rows, dtype=torch.int32, device="cuda")
    d_rows[0] = 0
    d_raw = torch.full((LEAD + total + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((n_rows + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_status = torch.full((n_rows,), 0xEE, dtype=torch.uint8, device="cuda")
    res = ctx.recode_packed_device(cb_in, cb_out, d_two, two_bi, two_ti, d_rows, d_raw[LEAD : LEAD + total], d_bi, d_ti, byte_map=bmap, status=d_status)
    torch.cuda.synchronize()
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed) == (OK, total, 9 + n_pages * page_len, 0)
    steps = torch.arange(n_rows + 1, dtype=torch.int64, device="cuda")
    want_bi, want_ti = steps * P + (small.size - P), steps * page_len + (9 - page_len)
    want_bi[0] = want_ti[0] = 0
    assert torch.equal(d_bi, want_bi) and torch.equal(d_ti, want_ti) and not bool(d_status.any())
    assert total > 1 << 32
    d_out = d_raw[LEAD : LEAD + total]
    assert d_out[: small.size].cpu().numpy().tobytes() == small.tobytes()
    assert torch.equal(d_out[small.size :].view(n_pages, P), d_piece.unsqueeze(0).expand(n_pages, P)), "a row differs from the oracle's encode of the translated text"
    assert bool((d_raw[:LEAD] == SENTINEL).all()) and bool((d_raw[LEAD + total :] == SENTINEL).all())
    del d_out, d_raw
    # input: a body behind offset 2^32 + 37 of a zero-filled buffer, another at 0, a record of length zero that spans what lies between
    far = (1 << 32) + 37
    d_bodies = torch.zeros(far + L + 1, dtype=torch.uint8, device="cuda")
    d_bodies[:L] = d_two[small_body.size :]
    d_bodies[far : far + L] = d_two[small_body.size :]
    d_raw = torch.full((LEAD + 3 * P + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_bi, d_ti = (torch.full((5,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_status = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    res = ctx.recode_packed_device(cb_in, cb_out, d_bodies[: far + L], _dev_index([0, L, far, far + L]), _dev_index([0, page_len, page_len, 2 * page_len]), dev_rows([2, 1, 0, 2]),
                                   d_raw[LEAD : LEAD + 3 * P], d_bi, d_ti, byte_map=bmap, status=d_status)
    torch.cuda.synchronize()
    # (record 1's body of 2^32 + 37 - L zeros is above 4 * small_max: that row fails alone)
    n = page_len
    assert (res.status, res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (OK, 3 * P, 3 * n, 1, 1, UNSUPPORTED)
    assert d_bi.tolist() == [0, P, P, 2 * P, 3 * P] and d_ti.tolist() == [0, n, n, 2 * n, 3 * n] and d_status.tolist() == [OK, UNSUPPORTED, OK, OK]
    assert torch.equal(d_raw[LEAD : LEAD + 3 * P].view(3, P), d_piece.unsqueeze(0).expand(3, P))
    assert bool((d_raw[:LEAD] == SENTINEL).all()) and bool((d_raw[LEAD + 3 * P :] == SENTINEL).all())


# --- 8. failures, capacity, sizes only ---------------------------------------------------------------------------------------------------------


def test_failures_stay_local(ctx):
    st, bad = failures_store()  # random bytes: under table_255 every byte string is a text
    st = with_table(st, table_255())
    dev = upload(st, spare=4096)
    rows = np.array([0, 16, 1, 3, 2, 0xFFFFFFFF, 8, 4, 15, 9, 5, 11, 6, 14, 12, 13, 7, 10, 3, 0], dtype=np.uint32)
    want = want_recode(st, table_255(), rows, PHASE_MAP)
    assert [int(s) for s in want.status] == [bad.get(int(r), OK) if r < 16 else ARG for r in rows]
    r = check_take(run_recode(ctx, st, table_255(), dev, rows, PHASE_MAP, want.total), want)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (9, 1, ARG)
    for k in np.flatnonzero(want.status):  # a failed row is an empty record
        assert r.body_index[k] == r.body_index[k + 1] and r.text_index[k] == r.text_index[k + 1]
    r = recode(ctx, st, table_255(), np.array([0, 1, 2, 15, 9, 3], dtype=np.uint32), dev=dev)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 3, UNSUPPORTED)
    r = recode(ctx, st, table_255(), np.array([13, 0, 1, 2, 4, 5, 6, 7, 10, 12, 13], dtype=np.uint32), dev=dev)  # a bad record that no row selects does not matter
    assert r.res.n_failed == 0 and not r.status.any()
    want = want_recode(st, table_255(), None)  # d_rows == NULL: every record, the bad ones among them
    r = check_take(run_recode(ctx, st, table_255(), dev, None, None, want.total), want)
    assert r.res.n_failed == len(bad)


def test_capacity_and_sizes_only(ctx):
    st, _ = main_fixture()
    T = main_tables()
    rows = np.concatenate((np.random.default_rng(0x4EC0DE60).integers(0, st.n, size=200), [st.n + 5, 0]))  # (one row fails: d_status is complete either way)
    dev = upload(st)
    want = want_recode(st, T["TU"], rows, UPPER)
    args = (ctx, st, T["TU"], dev, rows, UPPER)
    exact = check_take(run_recode(*args, want.total), want)
    assert exact.res.n_failed == 1
    check_take(run_recode(*args, want.total - 1), want, call_status=CAP)  # not a byte is written, the arrays and statuses are complete
    check_take(run_recode(*args, 1), want, call_status=CAP)
    sizes_only = check_take(run_recode(*args, want.total, sizes_only=True), want)
    assert sizes_only.res == exact.res
    check_take(run_recode(*args, want.total + 1000), want)  # the ctx is as good as before; room to spare stays untouched


def _raw_call(ctx, st, dev, n_rows, d_rows, d_out, d_a, d_b, res, cb_in=None, cb_out=None, bmap=None, **ptr):
    """One call through the C ABI; ptr: p_rows, p_out -- addresses (or None) in place of those arrays -- and cap."""
    from entreepy_amd import _native as N

    d_bodies, d_body_index, d_text_index = dev
    m = None if bmap is None else np.ascontiguousarray(bmap, dtype=np.int16)
    return N.lib().et_recode_packed_device(ctx._h, ctypes.byref((cb_in or st.cb).raw), ctypes.byref((cb_out or st.cb).raw), None if m is None else m.ctypes.data, d_bodies.data_ptr(),
                                           d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n, ptr.get("p_rows", d_rows.data_ptr()), n_rows,
                                           ptr.get("p_out", d_out.data_ptr()), ptr.get("cap", d_out.numel()), d_a.data_ptr(), d_b.data_ptr(), None, ctypes.byref(res))


def test_call_level_errors_enqueue_nothing_on_a_live_context(ctx):
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    st, _ = main_fixture()
    dev = upload(st)
    before = dev[0].clone()
    d_rows = dev_rows([1, 2])
    d_out = torch.full((4000,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_a, d_b = (torch.full((3,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    fresh = lambda: N.TakeResult(out_bytes=99, text_bytes=98, n_failed=97, first_failed=96, first_status=95)  # noqa: E731
    untouched = lambda res: (res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (99, 98, 97, 96, 95)  # noqa: E731
    res = fresh()
    assert _raw_call(ctx, st, dev, 0, d_rows, d_out, d_a, d_b, res) == OK
    assert (res.out_bytes, res.text_bytes, res.n_failed, res.first_failed, res.first_status) == (0, 0, 0, 0, 0)
    data, length = (a.copy() for a in st.tab)
    length[int(np.flatnonzero(length)[0])] = 0  # a hole in the tree
    holed = E.Codebook.from_tables(data, length)
    assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, fresh(), cb_in=holed) == UNSUPPORTED
    assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, fresh(), cb_out=holed) == UNSUPPORTED
    cases = {"misaligned d_rows": dict(p_rows=d_rows.data_ptr() + 3), "d_out inside d_bodies": dict(p_out=dev[0].data_ptr() + 8, cap=16),
             "d_out around d_bodies' end": dict(p_out=dev[0].data_ptr() + dev[0].numel() - 1, cap=64), "no d_rows, and n_rows is not n_records": dict(p_rows=None)}
    for value in (-2, 256, 32767, -32768):
        bad = IDENTITY.copy()
        bad[200] = value
        cases[f"a map entry of {value}"] = dict(bmap=bad)
    for what, kw in cases.items():
        res = fresh()
        assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, **kw) == ARG, what
        assert untouched(res), f"{what}: *res was touched"
    res = fresh()
    assert _raw_call(ctx, st, dev, 0x80000000, d_rows, d_out, d_a, d_b, res) == ARG and untouched(res)
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_a == -1).all()) and bool((d_b == -1).all()) and torch.equal(dev[0], before), "something was enqueued"
    res = fresh()
    assert _raw_call(ctx, st, dev, 2, d_rows, d_out, d_a, d_b, res, bmap=UPPER) == OK  # the ctx is as good as before
    torch.cuda.synchronize()
    want = want_recode(st, st.tab, [1, 2], UPPER)
    assert res.out_bytes == want.total and d_out[: want.total].cpu().numpy().tobytes() == want.data.tobytes() and bool((d_out[want.total :] == SENTINEL).all())


# --- 9. agreement with the existing calls ------------------------------------------------------------------------------------------------------


def test_the_identity_under_one_table_is_the_slice_to_the_end(ctx):
    for st in (main_fixture()[0], set_pad_fixture()[0], cut_fixture(), length_fixture()[0]):
        dev = upload(st)
        rows = np.random.default_rng(0x4EC0DE70).integers(0, st.n, size=60)
        want = want_recode(st, st.tab, rows)
        mine = check_take(run_recode(ctx, st, st.tab, dev, rows, None, want.total), want)
        sliced = check_take(run_slice(ctx, st, dev, rows, 0, TO_END, None, want.total), want)
        assert np.array_equal(mine.host[mine.at : mine.at + want.total], sliced.host[sliced.at : sliced.at + want.total]) and mine.res == sliced.res
        assert np.array_equal(mine.body_index, sliced.body_index) and np.array_equal(mine.text_index, sliced.text_index)


def test_there_and_back_is_the_normalised_store(ctx):
    import torch

    T = main_tables()
    st, _ = set_pad_fixture()
    n = st.n
    normal = want_recode(st, T["T1"], None)
    there = want_recode(st, T["T2"], None)
    d_mid, d_back = (guarded(size) for size in (there.total, normal.total))
    idx = [torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(4)]
    a = ctx.recode_packed_device(_cb(T["T1"]), _cb(T["T2"]), *upload(st), None, d_mid[: there.total], idx[0], idx[1])
    b = ctx.recode_packed_device(_cb(T["T2"]), _cb(T["T1"]), d_mid[: there.total], idx[0], idx[1], None, d_back[: normal.total], idx[2], idx[3])  # nothing in between
    torch.cuda.synchronize()
    assert (a.status, a.out_bytes, a.n_failed, b.status, b.out_bytes, b.n_failed) == (OK, there.total, 0, OK, normal.total, 0)
    assert d_mid[: there.total].cpu().numpy().tobytes() == there.data.tobytes() and d_back[: normal.total].cpu().numpy().tobytes() == normal.data.tobytes()
    assert np.array_equal(idx[2].cpu().numpy().view(np.uint64), normal.body_index) and np.array_equal(idx[3].cpu().numpy().view(np.uint64), normal.text_index)
    assert _guards_intact(d_mid, there.total) and _guards_intact(d_back, normal.total)
    assert np.array_equal(normal.data, main_fixture()[0].bodies)


# --- 10. pipelines with nothing in between -------------------------------------------------------------------------------------------------------


def _words(seed, n, pool):
    rng = np.random.default_rng(seed)
    return [pool[int(rng.integers(0, len(pool)))] for _ in range(n)]


def _encode_store(ctx, cb, texts):
    """encode_packed_device of a list -> (bodies, body_index, text_index) on the device; the caller synchronises."""
    import torch

    index = _index_of([len(t) for t in texts])
    d_text, d_index = _dev_bytes(np.frombuffer(b"".join(texts), np.uint8)), _dev_index(index)
    d_out = torch.empty(cb.body_bound(int(index[-1])) + len(texts), dtype=torch.uint8, device="cuda")
    d_bi = torch.empty(len(texts) + 1, dtype=torch.int64, device="cuda")
    e = ctx.encode_packed_device(cb, d_text, d_index, d_out, d_bi)
    assert e.status == OK and e.n_failed == 0
    return d_out[: max(e.out_bytes, 1)], d_bi, d_index


def test_recode_join_gather_across_two_tables(ctx):
    """A store written under T1 and a key set written under T2: recode the store to T2, join, gather -- dict membership over the texts."""
    import torch

    import entreepy_amd as E

    pool = [b"k%04d" % i + b"xyz"[: i % 4] for i in range(400)]
    records, keys = _words(0x4EC0DE80, 3000, pool), pool[::3]
    hist = np.bincount(np.frombuffer(b"".join(pool), np.uint8), minlength=256)
    cb1 = E.Codebook.from_histogram(hist)
    cb2 = _cb(other_table((np.array(cb1.raw.data, dtype=np.uint32), np.array(cb1.raw.length, dtype=np.uint8))))
    n = len(records)
    d_new = guarded(16 * n)
    d_bi, d_ti = (torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_hits, d_key = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    d_texts = torch.full((16 * n + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_texts_index = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    store, key_store = _encode_store(ctx, cb1, records), _encode_store(ctx, cb2, keys)
    rc = ctx.recode_packed_device(cb1, cb2, *store, None, d_new[: 16 * n], d_bi, d_ti)
    new = (d_new[: max(rc.out_bytes, 1)], d_bi, d_ti)
    j = ctx.join_packed_device(cb2, *new, *key_store, rows=d_hits, key_of_row=d_key)
    g = ctx.decode_packed_gather_device(cb2, *new, d_hits[: j.n_match], d_texts[: 16 * n], d_texts_index[: j.n_match + 1])
    torch.cuda.synchronize()
    hits = [k for k, t in enumerate(records) if t in set(keys)]
    assert 0 < len(hits) < n and (rc.status, rc.n_failed, rc.text_bytes) == (OK, 0, sum(len(t) for t in records)) and _guards_intact(d_new, rc.out_bytes)
    assert (j.status, j.n_failed, j.n_keys_failed) == (OK, 0, 0) and d_hits[: j.n_match].tolist() == hits
    assert d_key[: j.n_match].tolist() == [keys.index(records[k]) for k in hits]
    assert (g.status, g.n_failed, g.n_short) == (OK, 0, 0) and d_texts[: g.out_bytes].cpu().numpy().tobytes() == b"".join(records[k] for k in hits)


def test_a_case_insensitive_match_is_a_match_on_the_upper_cased_store(ctx):
    import torch

    import entreepy_amd as E

    names = [b"Ada", b"ADA", b"ada", b"aDa", b"Adam", b"Ad", b"", b"Bob", b"bOB", b"ada ", b"Ada Lovelace", b"ADA LOVELACE"]
    records = _words(0x4EC0DE90, 2000, names)
    cb = E.Codebook.from_histogram(np.bincount(np.frombuffer(b"".join(names) + b"".join(names).upper(), np.uint8), minlength=256))
    n = len(records)
    d_new = guarded(16 * n)
    d_bi, d_ti = (torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    d_hits = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    store = _encode_store(ctx, cb, records)
    rc = ctx.recode_packed_device(cb, cb, *store, None, d_new[: 16 * n], d_bi, d_ti, byte_map=E.ASCII_UPPER)
    new = (d_new[: max(rc.out_bytes, 1)], d_bi, d_ti)
    eq = ctx.match_packed_device(cb, *new, b"aDa".upper(), E.MATCH_EQUAL, rows=d_hits[0])
    pre = ctx.match_packed_device(cb, *new, b"ada l".upper(), E.MATCH_PREFIX, rows=d_hits[1])
    torch.cuda.synchronize()
    assert (rc.status, rc.n_failed) == (OK, 0) and _guards_intact(d_new, rc.out_bytes)
    assert d_hits[0][: eq.n_match].tolist() == [k for k, t in enumerate(records) if t.upper() == b"ADA"] and eq.n_match > 0
    assert d_hits[1][: pre.n_match].tolist() == [k for k, t in enumerate(records) if t.upper().startswith(b"ADA L")] and pre.n_match > 0


def test_field_recode_concat_on_one_context(ctx):
    """Column 1 of CSV lines under T1 -> recoded, upper-cased, to T2 -> concatenated with a store written under T2."""
    import torch

    import entreepy_amd as E

    rng = np.random.default_rng(0x4EC0DEA0)
    names = [bytes(rng.choice(np.frombuffer(b"abcdefgh", np.uint8), size=int(rng.integers(0, 9))).tobytes()) for _ in range(500)]
    lines = [b"%d," % i + w + b",x%d" % (i % 7) for i, w in enumerate(names)]
    ids = [b"id%d" % i for i in range(500)]
    hist = np.bincount(np.frombuffer(b"".join(lines + ids) + b"=ABCDEFGH", np.uint8), minlength=256)
    cb1 = E.Codebook.from_histogram(hist)
    cb2 = _cb(other_table((np.array(cb1.raw.data, dtype=np.uint32), np.array(cb1.raw.length, dtype=np.uint8))))
    n = len(lines)
    outs = [guarded(32 * n) for _ in range(3)]
    idx = [torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(6)]
    line_store, id_store = _encode_store(ctx, cb1, lines), _encode_store(ctx, cb2, ids)
    f = ctx.field_packed_device(cb1, *line_store, None, 1, 1, b",", outs[0][: 32 * n], idx[0], idx[1])
    col = (outs[0][: max(f.out_bytes, 1)], idx[0], idx[1])
    rc = ctx.recode_packed_device(cb1, cb2, *col, None, outs[1][: 32 * n], idx[2], idx[3], byte_map=E.ASCII_UPPER)
    up = (outs[1][: max(rc.out_bytes, 1)], idx[2], idx[3])
    c = ctx.concat_packed_device(cb2, id_store, b"=", up, outs[2][: 32 * n], idx[4], idx[5])
    torch.cuda.synchronize()
    want = [i + b"=" + w.upper() for i, w in zip(ids, names)]
    assert all((x.status, x.n_failed) == (OK, 0) for x in (f, rc, c)) and c.text_bytes == sum(len(w) for w in want)
    tab2 = (np.array(cb2.raw.data, dtype=np.uint32), np.array(cb2.raw.length, dtype=np.uint8))
    assert outs[2][: c.out_bytes].cpu().numpy().tobytes() == b"".join(want_encode(tab2, w)[1] for w in want)
    assert all(_guards_intact(o, x.out_bytes) for o, x in zip(outs, (f, rc, c)))


# --- 11. the list helper ---------------------------------------------------------------------------------------------------------------------------


def test_the_list_helper_on_100_random_records(ctx):
    import entreepy_amd as E

    rng = np.random.default_rng(0x4EC0DEB0)
    texts = [corpus.text_like(int(rng.integers(0, 3000)), 0x4EC0DEB1 + i).tobytes() for i in range(100)]
    pool = b"".join(texts)
    cb1 = E.Codebook.from_histogram(np.bincount(np.frombuffer(pool, np.uint8), minlength=256))
    cb2 = E.Codebook.from_histogram(np.bincount(np.frombuffer(pool.upper() + pool.lower(), np.uint8), minlength=256))
    blob, out_index = ctx.encode_packed(cb1, texts)
    lengths = [len(t) for t in texts]
    strip = E.byte_map(b"e", b"E", delete=b" \n")
    for rows, bmap in ((None, None), (None, E.ASCII_UPPER), (rng.integers(0, 100, size=150), E.ASCII_LOWER), ([99, 0, 0, 5], strip)):
        new_blob, new_index, new_lengths = ctx.recode_packed(cb1, cb2, blob, out_index, lengths, rows=rows, byte_map=bmap)
        want = [translate(texts[r], bmap) for r in (range(100) if rows is None else rows)]
        assert [int(x) for x in new_lengths] == [len(w) for w in want]
        assert (new_blob, new_index.tolist()) == (lambda b, i: (b, i.tolist()))(*ctx.encode_packed(cb2, want))
        assert ctx.decode_packed(cb2, new_blob, new_index, new_lengths) == want
    assert ctx.recode_packed(cb1, cb2, blob, out_index, lengths, rows=[])[0] == b""
    with pytest.raises(E.EntreepyError, match="row 1") as e:
        ctx.recode_packed(cb1, cb2, blob, out_index, lengths, rows=[3, 100, 4])
    assert e.value.status == ARG
    with pytest.raises(E.EntreepyError) as e:
        ctx.recode_packed(cb1, cb2, blob, out_index, lengths, byte_map=np.full(256, 256))
    assert e.value.status == ARG


# --- 12. the state a context keeps between calls ---------------------------------------------------------------------------------------------------
# The cells of tests/test_gpu_retained.py for the row `recode` (tests/retained_recode.py): a recode between the call that sets a state
# and the calls that read it leaves the histogram link, the held range and the last codebook as they were.


@pytest.mark.parametrize("reader", ["body", "head", "on_host"])
def test_histogram_link_survives_a_recode(reader):
    from tests import test_gpu_retained as G

    G.test_histogram_link("recode", reader)


@pytest.mark.parametrize("how", ["sync", "maps", "between", "windows"])
def test_held_range_survives_a_recode(how):
    from tests import test_gpu_retained as G

    G.test_held_range("recode", how)


def test_last_codebook_survives_a_recode():
    from tests import test_gpu_retained as G

    G.test_last_codebook("recode")
