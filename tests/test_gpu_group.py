"""GPU: et_group_packed_device -- which records of a packed store hold the same text (DISTINCT, GROUP BY, COUNT(*)), found on the
compressed bytes as a join of the store with itself -- against the oracle, as tests/test_gpu_join.py: a record's status is judged from
its own two pairs of offsets and its text is want_decode's; the expected groups are a Python dict over (length, text) of the valid
records in order of first appearance, a body of no bytes under a length above zero a group of its own; never the byte rule the kernels
implement.  The one exception is the hand-made-body fixture, where the documented byte rule IS the expectation.  Every output is filled
with sentinels first; everything at or behind n_groups must still hold them.

The stores are made by the *_fixture functions below, without a GPU: tests/test_group_host.py checks on the same fixtures that the
byte rule gives the partition that dict membership gives, and that they reach the cases named here.  The stores: edges, counting, trap,
chain (one home slot, tags that differ), near, long, failures, mixed, csv -- and collide_one_tag, collide_one_hash, collide_sizes,
collide_wave: the join's texts with hash tags, or whole hashes, equal by construction (tests/hashcraft.py), the only ones in which a tag
hit is confirmed between two DIFFERENT texts."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus
from tests import retained_group  # noqa: F401  (the call's row joins the table of tests/retained.py)
from tests.test_gpu_batch import SENTINEL, _small_max
from tests.test_gpu_gather import _mixed_store, dev_rows, make_store, upload, want_rows  # noqa: F401  (through judged)
from tests.test_gpu_join import CRAFT_RECORDS, CRAFTED, CRAFTS, LANE_BYTES, TILE, _rand_texts, _raw, acgt_texts, check_crafted_hashes, handmade_fixture, host_hash, long_fixture, \
    near_fixture, run_join, spread, table_slots, trap_fixture
from tests.test_gpu_match import EQUAL, ROW_SENTINEL, _pack, _store, judged, run_match
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_gpu_shared import _cb, want_decode  # noqa: F401
from tests.test_shared_host import oracle_table, table_2bit, table_255, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
NONE = 0xFFFFFFFF  # ET_GROUP_NONE
COLLIDERS = 32
EDGE_SIZES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


# --- the expected groups: the oracle's texts, Python's dict ---------------------------------------------------------------------------


def want_group(st):
    """-> (first rows, counts, group_of): a dict over (length, text) of the valid records in order of first appearance; a record kept
    raw is a group of its own; a failed record has NONE."""
    seen, first, counts, group_of = {}, [], [], []
    for b, (status, length, text) in enumerate(judged(st)):
        if status:
            group_of.append(NONE)
            continue
        key = ("raw", b) if _raw(st, b) else (length, text)
        if key not in seen:
            seen[key] = len(first)
            first.append(b)
            counts.append(0)
        counts[seen[key]] += 1
        group_of.append(seen[key])
    return first, counts, group_of


# --- one call ------------------------------------------------------------------------------------------------------------------------


def run_group(ctx, cb, dev, n, cap, count_only=False, counts=True, numbers=True):
    """One call through the C ABI (a capacity of zero is still a pointer), every output full of sentinels first."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    d_bodies, d_body_index, d_text_index = dev
    r = SimpleNamespace(cap=cap, count_only=count_only, counts=counts and not count_only, numbers=numbers and not count_only)
    sentinels = lambda k: torch.full((4 * k,), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.int32)  # noqa: E731
    r.d_first, r.d_count, r.d_group_of = sentinels(cap + TAIL), sentinels(cap + TAIL), sentinels(n + TAIL)
    r.d_status = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = N.GroupResult()
    rc = N.lib().et_group_packed_device(ctx._h, ctypes.byref(cb.raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), n,
                                        None if count_only else r.d_first.data_ptr(), cap, r.d_count.data_ptr() if r.counts else None,
                                        r.d_group_of.data_ptr() if r.numbers else None, r.d_status.data_ptr(), ctypes.byref(res))
    torch.cuda.synchronize()
    r.res = E.GroupResult(rc, res.n_groups, res.n_failed, res.first_failed, res.first_status)
    r.first, r.count, r.group_of = (t.cpu().numpy().view(np.uint32) for t in (r.d_first, r.d_count, r.d_group_of))
    r.status = r.d_status.cpu().numpy()[:n]
    return r


def check_group(r, st, call_status=OK, want=None):
    first, counts, group_of = want or want_group(st)
    statuses = [s for s, _, _ in judged(st)]
    failed = [b for b, s in enumerate(statuses) if s]
    assert (r.res.status, r.res.n_groups, r.res.n_failed) == (call_status, len(first), len(failed)), (r.res, len(first))
    if failed:
        assert (r.res.first_failed, r.res.first_status) == (failed[0], statuses[failed[0]]), r.res
    assert list(r.status) == statuses, "a record's status byte differs"
    assert sum(counts) == st.n - len(failed) and len(group_of) == st.n
    untouched = lambda a: bool((a == ROW_SENTINEL).all())  # noqa: E731
    if r.count_only or call_status != OK:
        assert untouched(r.first) and untouched(r.count) and untouched(r.group_of), "an entry of d_first_rows, d_count or d_group_of was written"
        return
    g = len(first)
    assert r.first[:g].tolist() == first, "the first rows differ from the oracle's"
    assert untouched(r.first[g:]), "an entry at or behind d_first_rows + n_groups was written"
    if r.counts:
        assert r.count[:g].tolist() == counts, "the counts differ from the oracle's"
        assert int(r.count[:g].sum()) == st.n - len(failed), "the counts do not sum to the valid records"
        assert untouched(r.count[g:]), "an entry at or behind d_count + n_groups was written"
    else:
        assert untouched(r.count)
    if r.numbers:
        assert r.group_of[: st.n].tolist() == group_of, "a record's group differs from the oracle's"
        assert untouched(r.group_of[st.n :]), "an entry behind d_group_of + n_records was written"
    else:
        assert untouched(r.group_of)


def group(ctx, st, dev=None, **kw):
    """Run with cap_groups = the need exactly, and check."""
    r = run_group(ctx, st.cb, dev or upload(st), st.n, len(want_group(st)[0]))
    check_group(r, st, **kw)
    return r


# --- the fixtures: stores, made without a GPU -----------------------------------------------------------------------------------------


def merged(a, b):
    """Two untampered stores under one table as one: a's records, then b's."""
    assert a.tab is b.tab or all(np.array_equal(x, y) for x, y in zip(a.tab, b.tab))
    st = SimpleNamespace(tab=a.tab, cb=a.cb, bodies=np.concatenate((a.bodies, b.bodies)), n=a.n + b.n)
    st.body_index = np.concatenate((a.body_index, b.body_index[1:] + np.uint64(a.bodies.size))).astype(np.uint64)
    st.text_index = np.concatenate((a.text_index, b.text_index[1:] + a.text_index[-1])).astype(np.uint64)
    return st


@functools.lru_cache(maxsize=None)
def edges_fixture(n):
    """n records drawn from a pool of about n / 3 texts: the members of a group lie in different wavefronts, tiles and workgroups."""
    rng = np.random.default_rng(0x6E0A9100 + n)
    pool = _rand_texts(rng, max(1, n // 3), 3, 12)
    return _store(table_255(), [pool[int(i)] for i in rng.integers(0, len(pool), size=n)])


@functools.lru_cache(maxsize=None)
def counting_fixture(kind):
    """2 * TILE + 1 records -- three tiles: of ONE text (the combining path); all different (the single adds); one text on 90 % of them."""
    n = 2 * TILE + 1
    rng = np.random.default_rng(0x6E0A9200)
    hot = bytes([9, 8, 7, 6, 5, 4, 3])
    if kind == "one":
        texts = [hot] * n
    elif kind == "distinct":
        texts = [bytes([2 + i % 250, 2 + i // 250, 77]) for i in range(n)]
    else:
        others = _rand_texts(rng, 20, 3, 6)
        texts = [hot if rng.random() < 0.9 else others[int(rng.integers(0, 20))] for _ in range(n)]
    return _store(table_255(), texts)


@functools.lru_cache(maxsize=None)
def trap_store():
    """The join's trap fixture as a single store: table_2bit, A = 00 -- texts that differ only by trailing As share their body bytes."""
    return merged(*trap_fixture())


@functools.lru_cache(maxsize=None)
def chain_fixture():
    """104 records in a table of 256 slots: 32 different texts crafted (et_join_hash, et_join_table_slots) to the home slot 251, so
    their chain runs over the table's last slot into its first, each of them twice; 20 others, twice as well; shuffled."""
    tab = table_255()
    rng = np.random.default_rng(0x6E0A9300)
    n = 2 * (COLLIDERS + 20)
    slots = table_slots(n)
    home = slots - 5
    colliders, others = [], []
    while len(colliders) < COLLIDERS or len(others) < 20:
        t = _rand_texts(rng, 1, 8, 9)[0]
        at = host_hash(t, len(t)) & (slots - 1)  # (the text is its own body)
        if at == home and len(colliders) < COLLIDERS and t not in colliders:
            colliders.append(t)
        elif at != home and len(others) < 20 and t not in others:
            others.append(t)
    texts = (colliders + others) * 2
    texts = [texts[int(i)] for i in rng.permutation(n)]
    assert all(_pack(tab, t) == t for t in colliders)
    return _store(tab, texts), SimpleNamespace(slots=slots, home=home, colliders=colliders)


@functools.lru_cache(maxsize=None)
def near_stores():
    """Records that differ in the last byte, in the last bit, in the length with one more body byte (the join's near fixture as one
    store); in the length only (the trap store); and in the byte count only: two texts of one length under a code of several lengths,
    the same stem and eight frequent bytes against eight rare ones."""
    pool = corpus.text_like(4000, 0x6E0A9400)
    tab = oracle_table(pool)
    used = [s for s in range(256) if tab[1][s]]
    short, long_ = min(used, key=lambda s: int(tab[1][s])), max(used, key=lambda s: int(tab[1][s]))
    stem = pool[:40].tobytes()
    a, b = stem + bytes([short]) * 8, stem + bytes([long_]) * 8
    return [merged(*near_fixture()), trap_store(), _store(tab, [a, b, stem, a, b, stem + bytes([short]) * 7])]


@functools.lru_cache(maxsize=None)
def long_store():
    """The join's long fixture as one store: bodies of 4 KiB among short ones in one tile, pairs that differ only in their last
    8-byte word, one that differs in length only, and one equal pair at et_batch_small_max() symbols."""
    return merged(*long_fixture())


@functools.lru_cache(maxsize=None)
def failures_fixture():
    """18 records under one table.  Records 3 (a decreasing body pair), 8 and 9 (a body entry at 2^63), 11 (a decreasing text pair) and
    17 (a length above the small-stream limit) fail; record 4's body begins 5 bytes early.  Records 0, 1 and 13 are one text, 6 and 7
    another; 2 and 14 are empty (length 0, no bytes): one group of two; 5 and 10 are one text kept raw (no body under the length):
    two groups of one."""
    sizes = [150, 150, 0, 130, 166, 120, 145, 145, 152, 135, 120, 144, 150, 150, 0, 141, 133, 139]
    pool = corpus.text_like(sum(sizes) + 400, 0x6E0A9500)
    tab = oracle_table(pool)
    cuts = _index_of(sizes)
    texts = [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(18)]
    texts[1] = texts[13] = texts[0]
    texts[7] = texts[6]
    texts[10] = texts[5]
    bodies = [_pack(tab, t) for t in texts]
    bodies[5] = bodies[10] = b""
    st = _store(tab, texts, bodies)
    st.body_index[4] = st.body_index[3] - np.uint64(5)
    st.body_index[9] = np.uint64(1) << np.uint64(63)
    st.text_index[12] = st.text_index[11] - np.uint64(3)
    st.text_index[18] = st.text_index[17] + np.uint64(_small_max() + 1)
    return st


@functools.lru_cache(maxsize=None)
def mixed_fixture():
    """_mixed_store()'s 300 records and 150 of them again, shuffled in behind: groups of one, two and more, the empty text among them."""
    st = _mixed_store()
    rng = np.random.default_rng(0x6E0A9600)
    texts = [t for _, _, t in judged(st)]
    return _store(st.tab, texts + [texts[int(i)] for i in rng.integers(0, st.n, size=150)])


@functools.lru_cache(maxsize=None)
def csv_fixture():
    """600 lines `<id>,<key>,<value>` with the keys from a pool of 40: the store the pipeline takes field 1 of."""
    rng = np.random.default_rng(0x6E0A9700)
    keys = [b"key-%d" % int(k) for k in rng.integers(0, 10**6, size=40)] + [b""]
    lines = [b"%d,%s,%d" % (i, keys[int(rng.integers(0, len(keys)))], int(rng.integers(0, 1000))) for i in range(600)]
    return _store(oracle_table(np.frombuffer(b"".join(lines), np.uint8)), lines), lines


@functools.lru_cache(maxsize=None)
def collide_store(name):
    """-> (store, info).  The join's crafted texts (tests/test_gpu_join.py's *_craft: one tag and one home slot; one whole hash; one hash
    under other sizes; one hash on the wavefront path) as ONE store of 632 records -- three tiles, a table of 2 048 slots, under whose
    mask the crafted homes are still equal --: every crafted text two or three times, its copies in different tiles, among fillers that
    are all different.  In the second tile a record fails (a decreasing body pair; the filler behind it begins 2 bytes early), in
    the third one is kept raw (no body under its length)."""
    c = CRAFTS[name]()
    tab = table_2bit()
    rng = np.random.default_rng(0x6E0A9800 + CRAFTED.index(name))
    crafted = list(c.keys) + list(c.strangers)
    placed = [((i + j) % 3, t) for i, t in enumerate(crafted) for j in range(2 + i % 2)]
    texts = spread(rng, CRAFT_RECORDS, placed, acgt_texts(rng, CRAFT_RECORDS - len(placed), avoid=c.hashes))
    filler = lambda b: texts[b] not in c.hashes  # noqa: E731
    failed = next(b for b in range(TILE + 1, 2 * TILE - 1) if filler(b - 1) and filler(b) and filler(b + 1))
    raw = next(b for b in range(2 * TILE, CRAFT_RECORDS) if filler(b))
    bodies = [_pack(tab, t) for t in texts]
    bodies[raw] = b""
    st = _store(tab, texts, bodies)
    st.body_index[failed + 1] = st.body_index[failed] - np.uint64(2)
    return st, SimpleNamespace(craft=c, crafted=crafted, copies={t: 2 + i % 2 for i, t in enumerate(crafted)}, failed=failed, raw=raw, others=CRAFT_RECORDS - len(placed) - 1)


STORES = {"trap": trap_store, "chain": lambda: chain_fixture()[0], "long": long_store, "failures": failures_fixture, "mixed": mixed_fixture,
          **{f"collide_{name}": (lambda name=name: collide_store(name)[0]) for name in CRAFTED},
          **{f"near_{i}": (lambda i=i: near_stores()[i]) for i in range(3)},
          **{f"counting_{kind}": (lambda kind=kind: counting_fixture(kind)) for kind in ("one", "distinct", "skewed")},
          **{f"edges_{n}": (lambda n=n: edges_fixture(n)) for n in EDGE_SIZES}}


# --- 1. tile and wavefront edges, the counting extremes ---------------------------------------------------------------------------------


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_tile_and_wavefront_edges(ctx, n):
    st = edges_fixture(n)
    assert st.n == n
    group(ctx, st)


@pytest.mark.parametrize("kind", ["one", "distinct", "skewed"])
def test_counting_extremes(ctx, kind):
    st = counting_fixture(kind)
    first, counts, _ = want_group(st)
    if kind == "one":
        assert (first, counts) == ([0], [2 * TILE + 1])
    elif kind == "distinct":
        assert counts == [1] * (2 * TILE + 1)
    else:
        assert max(counts) > 0.85 * st.n and len(counts) > 10
    group(ctx, st)


# --- 2. the zero-codeword trap, near-equal records, a chain that wraps --------------------------------------------------------------------


def test_texts_that_share_their_body_bytes_pair_by_length(ctx):
    st = trap_store()
    r = group(ctx, st)
    texts = [t for _, _, t in judged(st)]
    by_text = {texts[b]: c for b, c in zip(r.first[: r.res.n_groups].tolist(), r.count.tolist())}
    assert (by_text[b"G"], by_text[b"GA"], by_text[b"GAA"], by_text[b"GAAA"], by_text[b"T"], by_text[b""], by_text[b"C"]) == (1, 2, 1, 2, 2, 2, 1)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_near_equal_records(ctx, which):
    st = near_stores()[which]
    group(ctx, st)
    if which == 2:
        assert want_group(st) == ([0, 1, 2, 5], [2, 2, 1, 1], [0, 1, 2, 0, 1, 3])


def test_a_chain_of_32_records_with_one_home_slot_that_wraps(ctx):
    st, info = chain_fixture()
    r = group(ctx, st)
    assert r.res.n_groups == COLLIDERS + 20 and r.count[: r.res.n_groups].tolist() == [2] * (COLLIDERS + 20)


@pytest.mark.parametrize("name", CRAFTED)
def test_the_device_gives_every_crafted_record_the_crafted_hash(ctx, name):
    st, info = collide_store(name)
    assert check_crafted_hashes(ctx, st, info.craft.hashes) == sum(info.copies.values())


@pytest.mark.parametrize("name", CRAFTED)
def test_texts_whose_tags_collide_by_construction_are_groups_apart(ctx, name):
    """Three times with identical arrays (the order of the inserts races), and count-only: as many groups as there are different crafted
    texts and fillers, each crafted text's with its two or three members."""
    st, info = collide_store(name)
    dev = upload(st)
    runs = [group(ctx, st, dev=dev) for _ in range(3)]
    r = runs[0]
    for again in runs[1:]:
        assert np.array_equal(again.first, r.first) and np.array_equal(again.count, r.count) and np.array_equal(again.group_of, r.group_of) and again.res == r.res
    assert len(set(info.crafted)) == len(info.crafted)
    assert r.res.n_groups == len(info.crafted) + info.others, "two different texts with one tag were merged, or one text was split"
    texts = [t for _, _, t in judged(st)]
    by_text = {texts[b]: c for b, c in zip(r.first[: r.res.n_groups].tolist(), r.count.tolist()) if not _raw(st, b)}
    assert {t: by_text.get(t) for t in info.crafted} == info.copies
    check_group(run_group(ctx, st.cb, dev, st.n, r.res.n_groups, count_only=True), st)


def test_take_of_the_first_rows_of_one_hash_is_the_key_set_the_join_numbers_the_groups_by(ctx):
    """test_take_of_the_first_rows_is_the_key_set_the_join_numbers_the_groups_by on the store of 32 texts with ONE 64-bit hash: the taken
    key set holds every one of them, and the join gives each record its group although every probe passes slots of its own tag.  The
    failed record has no row; the record kept raw is taken as it is and, as a key and as a record, equals nothing."""
    import torch

    st, info = collide_store("one_hash")
    first, counts, group_of = want_group(st)
    dev = upload(st)
    r = group(ctx, st, dev=dev)
    g = r.res.n_groups
    d_keys = torch.full((st.bodies.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_key_body_index, d_key_text_index = (torch.full((g + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    t = ctx.take_packed_device(*dev, r.d_first[:g], d_keys[: st.bodies.size], d_key_body_index, d_key_text_index)
    assert (t.status, t.n_failed) == (OK, 0)
    kdev = (d_keys[: max(t.out_bytes, 1)], d_key_body_index, d_key_text_index)
    j = run_join(ctx, st.cb, dev, st.n, kdev, g, 0, st.n)
    rows = [b for b in range(st.n) if group_of[b] != NONE and not _raw(st, b)]
    assert rows == [b for b in range(st.n) if b not in (info.failed, info.raw)]
    assert (j.res.status, j.res.n_match, j.res.n_failed, j.res.first_failed, j.res.n_keys_failed) == (OK, len(rows), 1, info.failed, 0)
    assert j.rows[: len(rows)].tolist() == rows and j.keys[: len(rows)].tolist() == [group_of[b] for b in rows] == [int(r.group_of[b]) for b in rows]


# --- 3. long bodies -------------------------------------------------------------------------------------------------------------------


def test_long_bodies_on_the_wavefront_path_beside_short_ones(ctx):
    st = long_store()
    sizes = np.diff(st.body_index).astype(int)
    assert int((sizes > LANE_BYTES).sum()) >= 10 and int((sizes <= LANE_BYTES).sum()) >= 3 and int(sizes.max()) == _small_max() // 4 and st.n <= TILE
    first, counts, group_of = want_group(st)
    assert max(counts) == 2 and counts.count(2) >= 4 and group_of[6] == group_of[12 + 2]  # the pair at the small-stream limit
    group(ctx, st)


# --- 4. failures stay local -----------------------------------------------------------------------------------------------------------


def test_failures_stay_local(ctx):
    st = failures_fixture()
    assert [s for s, _, _ in judged(st)] == [OK, OK, OK, ARG, OK, OK, OK, OK, ARG, ARG, OK, ARG, OK, OK, OK, OK, OK, UNSUPPORTED]
    assert _raw(st, 5) and _raw(st, 10) and judged(st)[5][:2] == judged(st)[10][:2]
    first, counts, group_of = want_group(st)
    assert first == [0, 2, 4, 5, 6, 10, 12, 15, 16] and counts == [3, 2, 1, 1, 2, 1, 1, 1, 1]
    assert group_of == [0, 0, 1, NONE, 2, 3, 4, 4, NONE, NONE, 5, NONE, 6, 0, 1, 7, 8, NONE]
    r = group(ctx, st, dev=upload(st, spare=st.bodies.size))  # (2^63 is not mapped: a pair that is followed faults or shows)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (5, 3, ARG)


# --- 5. hand-made bodies, and the match call --------------------------------------------------------------------------------------------


def test_a_byte_behind_the_last_codeword_is_a_group_apart(ctx):
    """The documented difference to ET_MATCH_EQUAL: here the byte rule itself is the expectation."""
    st, _ = handmade_fixture()
    texts = [t for _, _, t in judged(st)]
    assert texts[0] == texts[1] != texts[2] and want_group(st)[0] == [0, 2]  # by their texts, records 0 and 1 are one group
    dev = upload(st)
    m = run_match(ctx, st.cb, dev, st.n, texts[0], EQUAL, 2)
    assert (m.res.status, m.res.n_match) == (OK, 2) and m.rows[:2].tolist() == [0, 1]
    check_group(run_group(ctx, st.cb, dev, st.n, 3), st, want=([0, 1, 2], [1, 1, 1], [0, 1, 2]))


# --- 6. the edges of the call -----------------------------------------------------------------------------------------------------------


def test_count_only_capacity_no_records_and_optional_outputs(ctx):
    import torch

    from entreepy_amd import _native as N

    st = failures_fixture()
    dev = upload(st, spare=st.bodies.size)
    need = len(want_group(st)[0])
    exact = run_group(ctx, st.cb, dev, st.n, need)
    check_group(exact, st)
    count = run_group(ctx, st.cb, dev, st.n, need, count_only=True)
    check_group(count, st)
    short = run_group(ctx, st.cb, dev, st.n, need - 1)
    check_group(short, st, call_status=CAP)
    assert count.res == exact.res and dict(vars(short.res), status=OK) == vars(exact.res)
    roomy = run_group(ctx, st.cb, dev, st.n, need + 5)
    check_group(roomy, st)
    for counts, numbers in ((False, True), (True, False), (False, False)):
        check_group(run_group(ctx, st.cb, dev, st.n, need, counts=counts, numbers=numbers), st)
    # no records: nothing enqueued, *res zeroed
    res = N.GroupResult(n_groups=77, n_failed=78, first_failed=79, first_status=80, pad=81)
    d_first = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    d_status = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = N.lib().et_group_packed_device(ctx._h, ctypes.byref(st.cb.raw), dev[0].data_ptr(), dev[0].numel(), dev[1].data_ptr(), dev[2].data_ptr(), 0, d_first.data_ptr(), 8,
                                        d_first.data_ptr(), d_first.data_ptr(), d_status.data_ptr(), ctypes.byref(res))
    torch.cuda.synchronize()
    assert rc == OK and bytes(res) == bytes(N.GroupResult()) and bool((d_first == -1).all()) and bool((d_status == 0xEE).all())


class _Args:
    """A complete, well-formed argument list in HOST memory: nothing is dereferenced before the checks pass, and every call made
    with it fails one of them."""

    def __init__(self, ctx):
        from entreepy_amd import _native as N

        self.N = N
        self.cb = N.Codebook()
        self.res = N.GroupResult(n_groups=77, n_failed=78, first_failed=79, first_status=80, pad=81)
        self.buf = (ctypes.c_uint64 * 16)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=ctx._h, cb=ctypes.addressof(self.cb), d_bodies=p, body_bytes=16, d_body_index=p, d_text_index=p + 16, n_records=1, d_first_rows=p + 32, cap_groups=4,
                      d_count=p + 48, d_group_of=p + 64, d_status=None, res=ctypes.addressof(self.res))

    def call(self, **changed):
        N, v = self.N, dict(self.v, **changed)
        rc = N.lib().et_group_packed_device(v["ctx"], ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None, v["d_bodies"], v["body_bytes"], v["d_body_index"],
                                            v["d_text_index"], v["n_records"], v["d_first_rows"], v["cap_groups"], v["d_count"], v["d_group_of"], v["d_status"],
                                            ctypes.cast(v["res"], ctypes.POINTER(N.GroupResult)) if v["res"] else None)
        r = self.res
        assert (r.n_groups, r.n_failed, r.first_failed, r.first_status, r.pad) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


def test_every_argument_error_of_the_contract_leaves_res_untouched(ctx):
    from entreepy_amd import _native as N

    a = _Args(ctx)
    for name in ("ctx", "cb", "res", "d_bodies", "d_body_index", "d_text_index"):
        assert a.call(**{name: None}) == ARG, name
    for name in ("d_body_index", "d_text_index"):
        for by in (1, 4):
            assert a.call(**{name: a.v[name] + by}) == ARG, (name, by)
    for name in ("d_first_rows", "d_count", "d_group_of"):
        for by in (1, 2, 3):
            assert a.call(**{name: a.v[name] + by}) == ARG, (name, by)
    assert a.call(n_records=(1 << 24) + 1) == ARG and a.call(n_records=1 << 40) == ARG
    assert a.call(d_first_rows=None) == ARG  # (counts and group numbers without first rows)
    assert a.call(d_first_rows=None, d_count=None) == ARG and a.call(d_first_rows=None, d_group_of=None) == ARG
    assert N.lib().et_group_records_max() == N.lib().et_join_keys_max() == 1 << 24


def test_an_incomplete_table_is_refused_with_nothing_enqueued(ctx):
    import torch

    import entreepy_amd as E

    data, length = table_ladder()
    data[110], length[110] = 0, 0  # a hole
    d_bodies, d_index = _dev_bytes(np.full(120, 100, np.uint8)), _dev_index(_index_of([50, 70]))
    d_first, d_count, d_group_of = (torch.full((8,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    d_status = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EntreepyError) as e:
        ctx.group_packed_device(_cb((data, length)), d_bodies, d_index, d_index, first_rows=d_first, count=d_count, group_of=d_group_of, status=d_status)
    assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == -1).all()) for t in (d_first, d_count, d_group_of)) and bool((d_status == 0xEE).all()), "something was enqueued"


# --- 7. determinism ---------------------------------------------------------------------------------------------------------------------


def test_the_same_call_three_times_gives_identical_arrays(ctx):
    for st in (counting_fixture("skewed"), mixed_fixture()):
        dev = upload(st)
        runs = [group(ctx, st, dev=dev) for _ in range(3)]
        for r in runs[1:]:
            assert np.array_equal(r.first, runs[0].first) and np.array_equal(r.count, runs[0].count) and np.array_equal(r.group_of, runs[0].group_of) and r.res == runs[0].res


# --- 8. against the existing calls ------------------------------------------------------------------------------------------------------


def test_take_of_the_first_rows_is_the_key_set_the_join_numbers_the_groups_by(ctx):
    """take(d_first_rows) -> the distinct texts as a store; the join of the store against it gives every record its group again."""
    import torch

    st = mixed_fixture()
    texts = [t for _, _, t in judged(st)]
    first, counts, group_of = want_group(st)
    distinct = list(dict.fromkeys(texts))
    assert [texts[b] for b in first] == distinct and len(distinct) < st.n and b"" in distinct
    dev = upload(st)
    r = group(ctx, st, dev=dev)
    g = r.res.n_groups
    d_keys = torch.full((st.bodies.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_key_body_index, d_key_text_index = (torch.full((g + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    t = ctx.take_packed_device(*dev, r.d_first[:g], d_keys[: st.bodies.size], d_key_body_index, d_key_text_index)
    assert (t.status, t.n_failed) == (OK, 0)
    kdev = (d_keys[: max(t.out_bytes, 1)], d_key_body_index, d_key_text_index)
    j = run_join(ctx, st.cb, dev, st.n, kdev, g, 0, st.n)
    assert (j.res.status, j.res.n_match, j.res.n_failed, j.res.n_keys_failed) == (OK, st.n, 0, 0)
    assert j.rows[: st.n].tolist() == list(range(st.n)) and j.keys[: st.n].tolist() == r.group_of[: st.n].tolist() == group_of
    d_text = torch.full((int(d_key_text_index[-1].item()) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d = ctx.decode_packed_device(st.cb, *kdev, d_text[: max(d_text.numel() - TAIL, 1)])
    torch.cuda.synchronize()
    assert (d.status, d.n_failed, d.n_short) == (OK, 0, 0)
    host, at = d_text.cpu().numpy(), d_key_text_index.cpu().numpy()
    assert [host[int(a) : int(b)].tobytes() for a, b in zip(at[:-1], at[1:])] == distinct


def test_field_then_group_then_take_then_decode_with_no_synchronisation(ctx):
    """SELECT key, COUNT(*) ... GROUP BY key over column 1 of a CSV store, on one ctx with nothing in between, against split and dict."""
    import torch

    st, lines = csv_fixture()
    column = [line.split(b",")[1] for line in lines]
    distinct = list(dict.fromkeys(column))
    want_counts = [column.count(k) for k in distinct]
    want_of = [distinct.index(k) for k in column]
    assert len(distinct) == 41 and b"" in distinct
    dev = upload(st)
    u8 = lambda n: torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")  # noqa: E731
    i32 = lambda n: torch.full((n,), -1, dtype=torch.int32, device="cuda")  # noqa: E731
    i64 = lambda n: torch.full((n,), -1, dtype=torch.int64, device="cuda")  # noqa: E731
    f_out, f_body_index, f_text_index = u8(st.bodies.size + TAIL), i64(st.n + 1), i64(st.n + 1)
    g_first, g_count, g_of = i32(st.n), i32(st.n), i32(st.n)
    t_out, t_body_index, t_text_index = u8(st.bodies.size + TAIL), i64(len(distinct) + 1), i64(len(distinct) + 1)
    d_text = u8(sum(len(k) for k in distinct) + TAIL)
    torch.cuda.synchronize()
    f = ctx.field_packed_device(st.cb, *dev, None, 1, 1, b",", f_out[: st.bodies.size], f_body_index, f_text_index)
    fdev = (f_out[: st.bodies.size], f_body_index, f_text_index)
    g = ctx.group_packed_device(st.cb, *fdev, first_rows=g_first, count=g_count, group_of=g_of)
    t = ctx.take_packed_device(*fdev, g_first[: g.n_groups], t_out[: st.bodies.size], t_body_index, t_text_index)
    d = ctx.decode_packed_device(st.cb, t_out[: st.bodies.size], t_body_index, t_text_index, d_text[: d_text.numel() - TAIL])
    torch.cuda.synchronize()
    assert (f.status, f.n_failed) == (OK, 0) and (g.status, g.n_groups, g.n_failed) == (OK, len(distinct), 0) and (t.status, t.n_failed) == (OK, 0)
    assert (d.status, d.n_failed, d.n_short) == (OK, 0, 0)
    k = len(distinct)
    assert g_count[:k].tolist() == want_counts and g_of.tolist() == want_of and bool((g_first[k:] == -1).all()) and bool((g_count[k:] == -1).all())
    assert [column[b] for b in g_first[:k].tolist()] == distinct
    host, at = d_text.cpu().numpy(), t_text_index.cpu().numpy()
    assert [host[int(a) : int(b)].tobytes() for a, b in zip(at[:-1], at[1:])] == distinct and bool((host[int(at[-1]) :] == SENTINEL).all())


def test_python_calls_give_the_same_arrays(ctx):
    import torch

    import entreepy_amd as E

    st = mixed_fixture()
    first, counts, group_of = want_group(st)
    dev = upload(st)
    d_first, d_count, d_of = (torch.full((st.n,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    r = ctx.group_packed_device(st.cb, *dev, first_rows=d_first, count=d_count, group_of=d_of)
    torch.cuda.synchronize()
    assert isinstance(r, E.GroupResult) and (r.status, r.n_groups, r.n_failed) == (OK, len(first), 0)
    assert d_first[: r.n_groups].tolist() == first and d_count[: r.n_groups].tolist() == counts and d_of.tolist() == group_of
    got = ctx.group_packed(st.cb, st.bodies.tobytes(), st.body_index, np.diff(st.text_index))
    assert [a.tolist() for a in got] == [first, counts, group_of] and all(a.dtype == np.uint32 for a in got)
    assert [a.size for a in ctx.group_packed(st.cb, b"", np.zeros(1, np.uint64), [])] == [0, 0, 0]
    count = ctx.group_packed_device(st.cb, *dev)
    assert (count.status, count.n_groups) == (OK, len(first))
    short = ctx.group_packed_device(st.cb, *dev, first_rows=d_first[: len(first) - 1])
    assert (short.status, short.n_groups) == (CAP, len(first)) and E.GROUP_NONE == NONE


# --- 9. the state a context keeps between calls -----------------------------------------------------------------------------------------
# The cells of tests/test_gpu_retained.py for the row `group` (tests/retained_group.py): a group call between the call that sets a state
# and the calls that read it leaves the histogram link, the held range and the last codebook as they were.


@pytest.mark.parametrize("reader", ["body", "head", "on_host"])
def test_histogram_link_survives_a_group_call(reader):
    from tests import test_gpu_retained as G

    G.test_histogram_link("group", reader)


@pytest.mark.parametrize("how", ["sync", "maps", "between", "windows"])
def test_held_range_survives_a_group_call(how):
    from tests import test_gpu_retained as G

    G.test_held_range("group", how)


def test_last_codebook_survives_a_group_call():
    from tests import test_gpu_retained as G

    G.test_last_codebook("group")
