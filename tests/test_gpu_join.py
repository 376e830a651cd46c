"""GPU: et_join_packed_device -- which records of a packed store equal SOME key of a key set, itself a packed store on the device, found
on the compressed bytes through a hash table -- against the oracle: an item's status is judged from its own two pairs of offsets and its
text is want_decode's (tests/test_gpu_gather.py's want_rows); the expected selection is Python dict membership of (length, text) over the
valid keys, and d_key_of_row is the first index of that text in the key list; never the byte rule the kernels implement.  What the
header excludes by name -- a body of no bytes under a length above zero, on either side -- is excluded here from the offsets.  The one
exception is the hand-made-body fixture, where the documented byte rule IS the expectation.  Every output is filled with sentinels
first; everything behind n_match must still hold them.

The stores and key sets are made by the *_fixture functions below, without a GPU: tests/test_join_host.py checks on the same fixtures
that the byte rule selects what membership selects, and that they reach the cases named here.  The fixtures: hash (hand-made bodies for
the device's hash), edges, trap, near, collisions (one home slot, tags that differ), duplicates, minmax, long, failures, handmade, mixed,
family -- and collide_one_tag, collide_one_hash, collide_sizes, collide_wave: texts made with tests/hashcraft.py whose hash tags, or
whole hashes, are equal by construction, the only ones in which a tag hit is confirmed between two DIFFERENT texts."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus, hashcraft
from tests.test_gpu_batch import SENTINEL, _small_max, _u8
from tests.test_gpu_gather import _mixed_store, dev_rows, make_store, upload, want_rows  # noqa: F401  (want_rows, want_decode: through judged)
from tests.test_gpu_match import EQUAL, HEAD_BITS, PREFIX, ROW_SENTINEL, _pack, _store, judged, pattern_bits, run_match, want_match
from tests.test_gpu_packed import TAIL, _dev_bytes, _dev_index, _index_of
from tests.test_gpu_take import model
from tests.test_gpu_shared import _cb, want_decode  # noqa: F401
from tests.test_shared_host import oracle_table, table_255, table_2bit, table_ladder

pytestmark = pytest.mark.gpu

OK, CAP, ARG, UNSUPPORTED = 0, 3, 6, 7  # et_status
NOT = 0x100  # ET_MATCH_NOT
TILE = 256  # records per tile of the build, flag and emit kernels (csrc/et_batch.h MATCH_TILE)
LANE_BYTES = 128  # the longest body a lane hashes and compares alone (csrc/et_batch.h JOIN_LANE_BYTES)
WAVE_STEP = 512  # bytes a wavefront takes per step above it: 64 lanes of 8
NONE = 0xFFFFFFFF


def _lib():
    from entreepy_amd import _native as N

    return N.lib()


def host_hash(body, length):
    body = np.ascontiguousarray(_u8(body))
    return int(_lib().et_join_hash(body.ctypes.data if body.size else None, body.size, length))


def table_slots(n_keys):
    return int(_lib().et_join_table_slots(n_keys))


# --- the expected rows: the oracle's texts, Python's dict ----------------------------------------------------------------------------


def _raw(st, i):
    """A body of no bytes under a length above zero: how a record looks whose encode failed; it equals nothing."""
    return int(st.body_index[i + 1]) == int(st.body_index[i]) and int(st.text_index[i + 1]) > int(st.text_index[i])


def want_join(st, ks, mode):
    """-> (rows, their keys): dict membership of (length, text) over the valid keys, the first index of each."""
    first = {}
    for k, (status, length, text) in enumerate(judged(ks)):
        if not status and not _raw(ks, k):
            first.setdefault((length, text), k)
    rows, keys = [], []
    for b, (status, length, text) in enumerate(judged(st)):
        if status:
            continue
        k = None if _raw(st, b) else first.get((length, text))
        if (k is not None) != bool(mode & NOT):
            rows.append(b)
            keys.append(k)
    return rows, keys


# --- one call ----------------------------------------------------------------------------------------------------------------------


def run_join(ctx, cb, dev, n, kdev, n_keys, mode, cap, count_only=False, key_rows=True):
    """One call through the C ABI (a capacity of zero is still a pointer), every output full of sentinels first."""
    import torch

    import entreepy_amd as E
    from entreepy_amd import _native as N

    d_bodies, d_body_index, d_text_index = dev
    k_bodies, k_body_index, k_text_index = kdev
    r = SimpleNamespace(cap=cap, count_only=count_only, key_rows=key_rows and not count_only and not mode & NOT)
    r.d_rows = torch.full((4 * (cap + TAIL),), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.int32)
    r.d_keys = torch.full((4 * (cap + TAIL),), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.int32)
    r.d_status = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    r.d_key_status = torch.full((max(n_keys, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = N.JoinResult()
    rc = N.lib().et_join_packed_device(ctx._h, ctypes.byref(cb.raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), n,
                                       k_bodies.data_ptr(), k_bodies.numel(), k_body_index.data_ptr(), k_text_index.data_ptr(), n_keys, mode,
                                       None if count_only else r.d_rows.data_ptr(), cap, r.d_keys.data_ptr() if r.key_rows else None, r.d_status.data_ptr(),
                                       r.d_key_status.data_ptr(), ctypes.byref(res))
    torch.cuda.synchronize()
    r.res = E.JoinResult(rc, res.n_match, res.n_failed, res.first_failed, res.n_keys_failed, res.first_key_failed, res.first_status, res.first_key_status)
    r.rows, r.keys = r.d_rows.cpu().numpy().view(np.uint32), r.d_keys.cpu().numpy().view(np.uint32)
    r.status, r.key_status = r.d_status.cpu().numpy()[:n], r.d_key_status.cpu().numpy()[:n_keys]
    return r


def check_join(r, st, ks, mode, call_status=OK, want=None):
    rows, keys = want or want_join(st, ks, mode)
    statuses, key_statuses = [s for s, _, _ in judged(st)], [s for s, _, _ in judged(ks)]
    failed, keys_failed = [b for b, s in enumerate(statuses) if s], [k for k, s in enumerate(key_statuses) if s]
    assert (r.res.status, r.res.n_match, r.res.n_failed, r.res.n_keys_failed) == (call_status, len(rows), len(failed), len(keys_failed)), (r.res, len(rows))
    if failed:
        assert (r.res.first_failed, r.res.first_status) == (failed[0], statuses[failed[0]]), r.res
    if keys_failed:
        assert (r.res.first_key_failed, r.res.first_key_status) == (keys_failed[0], key_statuses[keys_failed[0]]), r.res
    assert list(r.status) == statuses, "a record's status byte differs"
    assert list(r.key_status) == key_statuses, "a key's status byte differs"
    if r.count_only or call_status != OK:
        assert bool((r.rows == ROW_SENTINEL).all()) and bool((r.keys == ROW_SENTINEL).all()), "an entry of d_rows or d_key_of_row was written"
        return rows
    assert r.rows[: len(rows)].tolist() == rows, "the rows differ from the oracle's"
    assert bool((r.rows[len(rows) :] == ROW_SENTINEL).all()), "an entry at or behind d_rows + n_match was written"
    if r.key_rows:
        assert r.keys[: len(rows)].tolist() == keys, "a key number is not the first index of the record's text among the keys"
        assert bool((r.keys[len(rows) :] == ROW_SENTINEL).all()), "an entry at or behind d_key_of_row + n_match was written"
    else:
        assert bool((r.keys == ROW_SENTINEL).all())
    return rows


def join(ctx, st, ks, mode=0, dev=None, kdev=None, **kw):
    """Run with cap_rows = the need exactly, and check."""
    need = len(want_join(st, ks, mode)[0])
    r = run_join(ctx, st.cb, dev or upload(st), st.n, kdev or upload(ks), ks.n, mode, need)
    check_join(r, st, ks, mode, **kw)
    return r


def both_modes(ctx, st, ks, **kw):
    dev, kdev = kw.pop("dev", None) or upload(st), kw.pop("kdev", None) or upload(ks)
    return join(ctx, st, ks, 0, dev=dev, kdev=kdev, **kw), join(ctx, st, ks, NOT, dev=dev, kdev=kdev, **kw)


# --- the fixtures: (store, key set), made without a GPU ------------------------------------------------------------------------------


def _rand_texts(rng, n, lo, hi):
    """n random texts of lo .. hi - 1 bytes over 2 .. 255: under table_255 a text is its own body."""
    return [rng.integers(2, 256, size=int(rng.integers(lo, hi))).astype(np.uint8).tobytes() for _ in range(n)]


@functools.lru_cache(maxsize=None)
def hash_fixture():
    """Hand-made bodies for et_selftest_join_hash, packed back to back: 0 .. 40 bytes at every start alignment 0 .. 7 (a record of one
    byte behind each run moves the next run by 5 mod 8), the lane / wavefront threshold - 1, + 0, + 1, one body of several wavefront
    steps, and one under a length of et_batch_small_max() symbols.  The lengths are arbitrary: the hash takes them as numbers."""
    rng = np.random.default_rng(0x10A5E001)
    sizes = []
    for _ in range(8):
        sizes += list(range(41)) + [1]
    sizes += [LANE_BYTES - 1, LANE_BYTES, LANE_BYTES + 1, 3, 5 * WAVE_STEP + 77, 2, 8 * WAVE_STEP]
    lengths = [(7 * s + 3) % 1000 for s in sizes]
    lengths[-1] = _small_max()
    bodies = [rng.integers(0, 256, size=s).astype(np.uint8) for s in sizes]
    st = make_store(table_255(), [np.full(n, 2, np.uint8) for n in lengths], bodies)
    return st, None


@functools.lru_cache(maxsize=None)
def edges_fixture(n):
    """n records; those at the first and last lane of every wavefront-and-tile edge there is hold one hot text.  Key sets of 1, 2, 255
    and 257 keys: the hot text first, then a third of them texts of other records, the rest absent."""
    tab = table_255()
    rng = np.random.default_rng(0x10A5E100 + n)
    hot = bytes([7, 7, 200, 9, 33])
    special = sorted({0, 63, 64, 127, 128, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1} & set(range(n)))
    texts = _rand_texts(rng, n, 3, 12)
    for i in special:
        texts[i] = hot
    others = [i for i in range(n) if i not in special]
    keysets = {}
    for nk in (1, 2, 255, 257):
        present = [texts[i] for i in rng.permutation(others)[: nk // 3]]
        keys = ([hot] + present + _rand_texts(rng, nk, 12, 15))[:nk]
        keysets[nk] = _store(tab, keys)
    return _store(tab, texts), keysets, special


@functools.lru_cache(maxsize=None)
def trap_fixture():
    """table_2bit, A = 00: texts that differ only by trailing As share their body bytes; keys and records of both lengths."""
    tab = table_2bit()
    records = [b"G", b"GA", b"GAA", b"GAAA", b"GAAAA", b"T", b"TA", b"TAA", b"CGT", b"CGTA", b"CGTAA", b"A", b"AA", b"AAAA", b"AAAAA", b"", b"AAA"]
    keys = [b"GA", b"GAAA", b"T", b"CGTA", b"AA", b"AAAAA", b"", b"C", b"TAAA"]
    return _store(tab, records), _store(tab, keys)


NEAR_STEM = bytes([50, 60, 70, 80, 90, 100, 110, 120, 130])


@functools.lru_cache(maxsize=None)
def near_fixture():
    """table_255, where byte s >= 2 has the 8-bit code s.  Keys and records that differ in the last byte only, in the last bit only
    (100 and 101), in length only with one more body byte; a key that is a prefix of a record and a record that is a prefix of a key."""
    tab = table_255()
    x = NEAR_STEM
    keys = [x + b"\x64", x + b"\xfa", x, x + b"\x64\x07", x[:4], x + x + b"\x09", x + x[:7] + b"\x64"]
    records = [x + b"\x64", x + b"\x65", x + b"\xfa", x + b"\x05", x, x + b"\x64\x07", x + b"\x64\x08", x[:4], x[:5], x + x, x[:3], x[:8], x + x[:7] + b"\x64", x + x[:7] + b"\x65",
               x + x + b"\x09", x + x + b"\x09\x09"]
    return _store(tab, records), _store(tab, keys)


COLLIDERS = 32


@functools.lru_cache(maxsize=None)
def collisions_fixture():
    """72 keys in a table of 256 slots: 32 of them crafted (et_join_hash, et_join_table_slots) to the home slot 251, so their chain
    runs over the table's last slot into its first; 40 others.  The store holds every key's text, a text that is no key and whose home
    lies in the middle of that chain, and 30 absent ones."""
    tab = table_255()
    rng = np.random.default_rng(0x10A5E200)
    n_keys = COLLIDERS + 40
    slots = table_slots(n_keys)
    home = slots - 5
    colliders, inside, others = [], None, []
    while len(colliders) < COLLIDERS or inside is None or len(others) < 40:
        t = _rand_texts(rng, 1, 8, 9)[0]
        at = host_hash(t, len(t)) & (slots - 1)  # (the text is its own body)
        if at == home and len(colliders) < COLLIDERS:
            colliders.append(t)
        elif (at - home) % slots in range(8, 24) and inside is None:
            inside = t
        elif len(others) < 40:
            others.append(t)
    keys = [None] * n_keys
    spots = rng.permutation(n_keys)
    for t, k in zip(colliders + others, spots):
        keys[int(k)] = t
    records = colliders + others + [inside] + _rand_texts(rng, 30, 9, 12)
    records = [records[i] for i in rng.permutation(len(records))]
    ks = _store(tab, keys)
    assert all(_pack(tab, t) == t for t in colliders + [inside])
    return _store(tab, records), ks, SimpleNamespace(slots=slots, home=home, colliders=colliders, inside=inside)


@functools.lru_cache(maxsize=None)
def duplicates_fixture():
    """2 000 keys -- eight workgroups of the build -- 50 of them copies of one text and 3 of another at scattered places; 600 records."""
    tab = table_255()
    rng = np.random.default_rng(0x10A5E300)
    keys = _rand_texts(rng, 2000, 6, 15)
    many, few = bytes([9, 8, 7, 6, 5, 4, 3]), bytes([200, 201, 202, 203, 204, 205, 206, 207, 208, 209])
    places = sorted(int(p) for p in rng.choice(np.arange(300, 2000), size=50, replace=False))
    for p in places:
        keys[p] = many
    few_places = [p for p in (1900, 417, 1033, 1901, 418, 1034) if p not in places][:3]
    for p in few_places:
        keys[p] = few
    records = [many] * 40 + [few] * 5 + [keys[int(i)] for i in rng.integers(0, 2000, size=300)] + _rand_texts(rng, 255, 15, 18)
    records = [records[i] for i in rng.permutation(len(records))]
    return _store(tab, records), _store(tab, keys), SimpleNamespace(many=many, few=few, first_many=places[0], first_few=min(few_places))


@functools.lru_cache(maxsize=None)
def minmax_fixture():
    """Keys of 5 .. 9 body bytes; records of 4 (min - 1), 5, 9 and 10 (max + 1), equal ones and others among those of 5 and 9."""
    tab = table_255()
    rng = np.random.default_rng(0x10A5E400)
    keys = _rand_texts(rng, 5, 5, 6) + _rand_texts(rng, 5, 7, 8) + _rand_texts(rng, 5, 9, 10)
    records = [keys[0][:4], keys[0], keys[1], keys[0][:4] + b"\x99", keys[10], keys[11][:8] + b"\x99", keys[10] + b"\x02", keys[12] + b"\x63", keys[6], keys[12][:4]]
    return _store(tab, records), _store(tab, keys)


@functools.lru_cache(maxsize=None)
def long_fixture():
    """table_2bit: keys and records of 4 KiB of body, and one pair at et_batch_small_max() symbols (64 KiB): equal ones, ones that differ
    in the last byte, and one that differs in length only (its last symbol is an A that falls into the pad)."""
    tab = table_2bit()
    rng = np.random.default_rng(0x10A5E500)
    letters = np.frombuffer(b"ACGT", np.uint8)

    def draw(n):
        return letters[rng.integers(0, 4, size=n)].copy()

    def flip(t, i):
        u = t.copy()
        u[i] = ord("T") if u[i] != ord("T") else ord("C")
        return u

    base, other, big = draw(16383), draw(16400), draw(_small_max())
    base[-1] = ord("G")
    grown = np.concatenate((base, np.frombuffer(b"A", np.uint8)))  # 16 384 symbols: the same 4 096 bytes
    keys = [grown, other, big, flip(big, 70_000), flip(other, 0), draw(9)]
    records = [draw(12), grown, base, flip(grown, 16_382), other, flip(other, 16_399), big, flip(big, _small_max() - 1), flip(big, 0), draw(16384), keys[5], flip(other, 0)]
    return _store(tab, records), _store(tab, keys)


@functools.lru_cache(maxsize=None)
def failures_fixture():
    """16 records and 12 keys under one table.  Records 3 (a decreasing body pair), 8 and 9 (a body entry at 2^63), 11 (a decreasing text
    pair) and 15 (a length above the small-stream limit) fail; record 5 has no body under its length; record 4's body begins 5 bytes
    early.  Keys 4 (decreasing), 7 and 8 (2^63) and 11 (too long) fail; key 2 is record 5's text with no body; key 5 begins 2 bytes
    early.  Keys 0, 1, 3, 6 and 9 are the texts of records 0, 1, 6, 10 and 7."""
    sizes = [150, 140, 1, 130, 166, 120, 145, 155, 152, 135, 149, 144, 150, 138, 0, 141]
    pool = corpus.text_like(sum(sizes) + 400, 0x10A5E600)
    tab = oracle_table(pool)
    cuts = _index_of(sizes)
    texts = [pool[int(cuts[i]) : int(cuts[i + 1])] for i in range(16)]
    bodies = [_pack(tab, t) for t in texts]
    bodies[5] = b""
    st = _store(tab, texts, bodies)
    st.body_index[4] = st.body_index[3] - np.uint64(5)
    st.body_index[9] = np.uint64(1) << np.uint64(63)
    st.text_index[12] = st.text_index[11] - np.uint64(3)
    st.text_index[16] = st.text_index[15] + np.uint64(_small_max() + 1)
    absent = [pool[int(cuts[-1]) + 40 * i : int(cuts[-1]) + 40 * i + 37] for i in range(6)]
    ktexts = [texts[0], texts[1], texts[5], texts[6], absent[0], absent[1], texts[10], absent[2], absent[3], texts[7], texts[2], absent[4]]
    kbodies = [_pack(tab, t) for t in ktexts]
    kbodies[2] = b""
    ks = _store(tab, ktexts, kbodies)
    ks.body_index[5] = ks.body_index[4] - np.uint64(2)
    ks.body_index[8] = np.uint64(1) << np.uint64(63)
    ks.text_index[12] = ks.text_index[11] + np.uint64(_small_max() + 1)
    return st, ks


@functools.lru_cache(maxsize=None)
def handmade_fixture():
    """Record 0's body carries one byte behind its last codeword; its text is key 0's.  Record 1 is the encoder's."""
    tab = table_255()
    x = NEAR_STEM
    return _store(tab, [x, x, x[:5]], [_pack(tab, x) + b"\0", _pack(tab, x), _pack(tab, x[:5])]), _store(tab, [x])


@functools.lru_cache(maxsize=None)
def mixed_fixture():
    """_mixed_store() and, as keys, its own records 0, 5, 5 and 9 encoded again with the oracle."""
    st = _mixed_store()
    texts = [judged(st)[b][2] for b in (0, 5, 5, 9)]
    return st, _store(st.tab, texts)


# --- hash tags that collide by construction (tests/hashcraft.py): the only fixtures in which the confirmation of a tag hit says "different" ----
# All under table_2bit, where every string of 8 k bytes is the encoder's own body of 32 k symbols.  A *_craft function makes the texts --
# .keys: those the key set holds, .strangers: those the store holds beside them and that equal no key, .hashes: text -> the hash it was
# made for --, collide_fixture puts them among fillers.  The expectations stay want_join's: a dict over (length, text).

LOW_BITS = 12  # the crafted hashes agree in their low 12 bits: one home slot under every table of up to 4 096 slots
CRAFT_RECORDS = 2 * TILE + 120  # three tiles, the last one partial
CRAFT_KEYS = 56  # a table of 256 slots
CRAFTED = ("one_tag", "one_hash", "sizes", "wave")


def _word(rng):
    return int(rng.integers(0, 1 << 64, dtype=np.uint64))


def _crafted(length, words):
    """The text of `length` symbols whose body is these full words; the encoder packs it back into exactly them."""
    body = hashcraft.body_of(words)
    text = hashcraft.text_2bit(body, length)
    assert bytes(_pack(table_2bit(), text)) == body
    return text


@functools.lru_cache(maxsize=None)
def one_tag_craft():
    """16 one-word texts (8 bytes, 32 symbols) whose hashes share the upper 32 bits -- the tag -- and the low 12 bits -- the home slot --
    and differ between them: a slot that holds one of them is passed by no tag test, only by the comparison of the bytes.  8 are keys."""
    rng = np.random.default_rng(0x10A5EB00)
    tag, low = int(rng.integers(1, 1 << 32)), int(rng.integers(0, 1 << LOW_BITS))
    mids = rng.choice(1 << (32 - LOW_BITS), size=16, replace=False)
    hashes = [tag << 32 | int(m) << LOW_BITS | low for m in mids]
    texts = [_crafted(32, [hashcraft.solve_word([], [], h, 8, 32)]) for h in hashes]
    return SimpleNamespace(tag=tag, low=low, hashes=dict(zip(texts, hashes)), keys=texts[:8], strangers=texts[8:], twice=None)


@functools.lru_cache(maxsize=None)
def one_hash_craft():
    """32 different two-word texts (16 bytes, 64 symbols) with ONE 64-bit hash, whose low 12 bits are 4 096 - 5: the home slot lies 5
    below the end of every table of up to 4 096 slots, so the chain wraps.  16 are keys, and key 5's text is a key twice."""
    rng = np.random.default_rng(0x10A5EB10)
    h = (_word(rng) & ~((1 << LOW_BITS) - 1)) | ((1 << LOW_BITS) - 5)
    firsts = []
    while len(firsts) < 32:
        w = _word(rng)
        if w not in firsts:
            firsts.append(w)
    texts = [_crafted(64, [w, hashcraft.solve_word([w], [], h, 16, 64)]) for w in firsts]
    return SimpleNamespace(h=h, hashes={t: h for t in texts}, keys=texts[:16], strangers=texts[16:], twice=texts[5])


@functools.lru_cache(maxsize=None)
def sizes_craft():
    """One 64-bit hash under other sizes: 8 bytes under 32 symbols, 8 bytes under 31 (the solved word's last symbol must be an A, which
    it is for a quarter of the hashes tried) and 16 bytes under 64 -- the three keys.  The strangers: a second 16-byte text and an 8-byte
    text under 30 symbols with that same hash; and, because a one-word body is determined by its hash, length and byte count -- no second
    one exists --, for 8 bytes under 32 and under 31 symbols a text each whose hash has the keys' tag and low 12 bits."""
    rng = np.random.default_rng(0x10A5EB20)
    while True:
        h = _word(rng)
        w31, w30 = hashcraft.solve_word([], [], h, 8, 31), hashcraft.solve_word([], [], h, 8, 30)
        if (w31 >> 56) & 3 == 0 and (w30 >> 56) & 15 == 0:  # (the symbols behind the length lie in the low bits of byte 7)
            break
    a, b, d = _crafted(32, [hashcraft.solve_word([], [], h, 8, 32)]), _crafted(31, [w31]), _crafted(30, [w30])
    c = [_crafted(64, [w, hashcraft.solve_word([w], [], h, 16, 64)]) for w in (_word(rng), _word(rng))]
    mid = (1 << 32) - (1 << LOW_BITS)
    while True:
        h2 = h ^ (int(rng.integers(1, 1 << (32 - LOW_BITS))) << LOW_BITS)
        w31 = hashcraft.solve_word([], [], h2, 8, 31)
        if (w31 >> 56) & 3 == 0:
            break
    assert h2 != h and (h2 ^ h) & ~mid == 0
    a2, b2 = _crafted(32, [hashcraft.solve_word([], [], h2, 8, 32)]), _crafted(31, [w31])
    return SimpleNamespace(h=h, h2=h2, hashes={a: h, b: h, d: h, c[0]: h, c[1]: h, a2: h2, b2: h2}, keys=[a, b, c[0]], strangers=[c[1], d, a2, b2], twice=None)


@functools.lru_cache(maxsize=None)
def wave_craft():
    """Bodies above LANE_BYTES, all with ONE 64-bit hash.  17 words (136 bytes: one step of the wavefront): a pair that differs in word
    0 and the solved last word.  66 words (528 bytes: past one WAVE_STEP): such a pair, and three texts whose first 512 bytes are equal
    and that differ only in words 64 and 65, so that the second trip decides.  Of each pair one is a key and one a stranger; of the three,
    two are keys.  Two lane-sized texts (16 bytes) with that hash as well: a key beside the wave-sized strangers, a stranger beside the
    wave-sized keys."""
    rng = np.random.default_rng(0x10A5EB30)
    h = _word(rng)

    def solved(words, n):
        return _crafted(32 * n, words + [hashcraft.solve_word(words, [], h, 8 * n, 32 * n)])

    short, long_, stem = [_word(rng) for _ in range(16)], [_word(rng) for _ in range(65)], [_word(rng) for _ in range(64)]
    a = [solved(short, 17), solved([short[0] ^ 1] + short[1:], 17)]
    b = [solved(long_, 66), solved([long_[0] ^ (1 << 63)] + long_[1:], 66)]
    c = [solved(stem + [w], 66) for w in (5, 6, 1 << 40)]
    lanes = [solved([_word(rng)], 2) for _ in range(2)]
    texts = a + b + c + lanes
    return SimpleNamespace(h=h, hashes={t: h for t in texts}, keys=[a[0], b[0], c[0], c[2], lanes[0]], strangers=[a[1], b[1], c[1], lanes[1]], twice=None, a=a, b=b, c=c, lanes=lanes)


CRAFTS = {"one_tag": one_tag_craft, "one_hash": one_hash_craft, "sizes": sizes_craft, "wave": wave_craft}


def acgt_texts(rng, n, avoid=()):
    """n different random texts of 9 .. 40 symbols over ACGT, none of them in `avoid`: the fillers."""
    letters, out, seen = np.frombuffer(b"ACGT", np.uint8), [], set(avoid)
    while len(out) < n:
        t = letters[rng.integers(0, 4, size=int(rng.integers(9, 41)))].tobytes()
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def spread(rng, n, placed, fillers):
    """n texts: every (tile, text) of `placed` at a random place of that tile of 256, the fillers in order at the other places."""
    free = [[int(i) for i in rng.permutation(np.arange(t * TILE, min((t + 1) * TILE, n)))] for t in range((n + TILE - 1) // TILE)]
    texts = [None] * n
    for tile, t in placed:
        texts[free[tile].pop()] = t
    rest = iter(fillers)
    return [t if t is not None else next(rest) for t in texts]


@functools.lru_cache(maxsize=None)
def collide_fixture(name):
    """-> (store, key set, the craft).  56 keys -- a table of 256 slots --: the craft's keys (and the one that occurs twice) at scattered
    numbers among fillers.  632 records: every crafted key and stranger, dealt over the three tiles in turn so that colliders lie in
    different wavefronts and workgroups, 20 of the filler keys' texts, and fillers that are no key."""
    c = CRAFTS[name]()
    tab = table_2bit()
    rng = np.random.default_rng(0x10A5EC00 + CRAFTED.index(name))
    key_texts = list(c.keys) + ([c.twice] if c.twice else [])
    fill = acgt_texts(rng, CRAFT_KEYS - len(key_texts) + CRAFT_RECORDS, avoid=c.hashes)
    key_fill, fill = fill[: CRAFT_KEYS - len(key_texts)], fill[CRAFT_KEYS - len(key_texts) :]
    keys = [None] * CRAFT_KEYS
    for t, k in zip(key_texts + key_fill, rng.permutation(CRAFT_KEYS)):
        keys[int(k)] = t
    placed = [(i % 3, t) for i, t in enumerate(list(c.keys) + list(c.strangers))]
    records = spread(rng, CRAFT_RECORDS, placed, key_fill[:20] + fill[: CRAFT_RECORDS - len(placed) - 20])
    return _store(tab, records), _store(tab, keys), c


FIXTURES = {"trap": trap_fixture, "near": near_fixture, "collisions": lambda: collisions_fixture()[:2], "duplicates": lambda: duplicates_fixture()[:2], "minmax": minmax_fixture,
            "long": long_fixture, "failures": failures_fixture, "mixed": mixed_fixture, **{f"collide_{name}": (lambda name=name: collide_fixture(name)[:2]) for name in CRAFTED},
            **{f"edges_{n}_{nk}": (lambda n=n, nk=nk: (edges_fixture(n)[0], edges_fixture(n)[1][nk])) for n in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1) for nk in (1, 2, 255, 257)}}


# --- 1. the hash on the device ------------------------------------------------------------------------------------------------------


def test_device_hash_is_the_host_hash_on_the_lane_and_the_wavefront_path(ctx):
    import torch

    from entreepy_amd import _native as N

    st, _ = hash_fixture()
    sizes, lengths = np.diff(st.body_index).astype(np.int64), np.diff(st.text_index).astype(np.int64)
    assert {(int(s), int(a) % 8) for s, a in zip(sizes, st.body_index[:-1])} >= {(s, a) for s in range(1, 41) for a in range(8)}
    assert {LANE_BYTES - 1, LANE_BYTES, LANE_BYTES + 1} <= set(sizes.tolist()) and int(sizes.max()) >= 8 * WAVE_STEP and int(lengths.max()) == _small_max()
    d_bodies, d_body_index, d_text_index = upload(st)
    d_hash = torch.full((st.n + 8,), -1, dtype=torch.int64, device="cuda")
    assert N.lib().et_selftest_join_hash(ctx._h, d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n, d_hash.data_ptr()) == OK
    got = d_hash.cpu().numpy().view(np.uint64)
    want = [host_hash(st.bodies[int(a) : int(b)], int(n)) for a, b, n in zip(st.body_index[:-1], st.body_index[1:], lengths)]
    assert got[: st.n].tolist() == want
    assert bool((got[st.n :] == np.uint64(0xFFFFFFFFFFFFFFFF)).all())


# --- 2. tile and wavefront edges -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tile_and_wavefront_edges(ctx, n):
    st, keysets, special = edges_fixture(n)
    dev = upload(st)
    for nk, ks in keysets.items():
        assert ks.n == nk
        rows, _ = want_join(st, ks, 0)
        assert set(special) <= set(rows)
        both_modes(ctx, st, ks, dev=dev)


# --- 3. the zero-codeword trap, near-equal keys -------------------------------------------------------------------------------------


def test_texts_that_share_their_body_bytes_pair_by_length(ctx):
    st, ks = trap_fixture()
    both_modes(ctx, st, ks)
    texts = [t for _, _, t in judged(st)]
    assert [texts[b] for b in want_join(st, ks, 0)[0]] == [b"GA", b"GAAA", b"T", b"CGTA", b"AA", b"AAAAA", b""]


def test_near_equal_keys(ctx):
    st, ks = near_fixture()
    both_modes(ctx, st, ks)
    assert want_join(st, ks, 0) == ([0, 2, 4, 5, 7, 12, 14], [0, 1, 2, 3, 4, 6, 5])


# --- 4. slot collisions --------------------------------------------------------------------------------------------------------------


def test_a_chain_of_32_keys_with_one_home_slot_that_wraps(ctx):
    st, ks, info = collisions_fixture()
    r, _ = both_modes(ctx, st, ks)
    texts = [t for _, _, t in judged(st)]
    selected = {texts[b] for b in r.rows[: r.res.n_match].tolist()}
    assert set(info.colliders) <= selected and info.inside not in selected and info.inside in texts


def device_hashes(ctx, st):
    """et_selftest_join_hash over a store -> one uint64 per record; all ones where the call left the sentinel."""
    import torch

    from entreepy_amd import _native as N

    d_bodies, d_body_index, d_text_index = upload(st)
    d_hash = torch.full((st.n + 8,), -1, dtype=torch.int64, device="cuda")
    assert N.lib().et_selftest_join_hash(ctx._h, d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n, d_hash.data_ptr()) == OK
    got = d_hash.cpu().numpy().view(np.uint64)
    assert bool((got[st.n :] == np.uint64(0xFFFFFFFFFFFFFFFF)).all())
    return got[: st.n].tolist()


def check_crafted_hashes(ctx, st, hashes):
    """The device gives every valid record the hash of its definition, and every crafted text the hash it was made for -> how many
    crafted records that were.  Without this a fixture could fail to collide on the device and its tests pass for the wrong reason."""
    got, blob, crafted = device_hashes(ctx, st), st.bodies.tobytes(), 0
    for b, (status, length, text) in enumerate(judged(st)):
        if status:
            assert got[b] == 0xFFFFFFFFFFFFFFFF, b
            continue
        assert got[b] == hashcraft.hash_of(blob[int(st.body_index[b]) : int(st.body_index[b + 1])], length), b
        if text in hashes and not _raw(st, b):
            assert got[b] == hashes[text], b
            crafted += 1
    return crafted


@pytest.mark.parametrize("name", CRAFTED)
def test_the_device_gives_every_crafted_record_and_key_the_crafted_hash(ctx, name):
    st, ks, c = collide_fixture(name)
    assert check_crafted_hashes(ctx, st, c.hashes) == len(c.keys) + len(c.strangers)
    assert check_crafted_hashes(ctx, ks, c.hashes) == len(c.keys) + (c.twice is not None)


@pytest.mark.parametrize("name", CRAFTED)
def test_texts_whose_tags_collide_by_construction_are_told_apart_by_their_bytes(ctx, name):
    """Both modes, three times with identical arrays (the order of the inserts races), and count-only: every crafted key's text is found
    under the first number of that text, every stranger -- same tag, same home slot or same whole hash -- is unmatched."""
    st, ks, c = collide_fixture(name)
    dev, kdev = upload(st), upload(ks)
    texts, key_texts = [t for _, _, t in judged(st)], [t for _, _, t in judged(ks)]
    runs = [both_modes(ctx, st, ks, dev=dev, kdev=kdev) for _ in range(3)]
    (r, rn) = runs[0]
    for again, again_not in runs[1:]:
        assert np.array_equal(again.rows, r.rows) and np.array_equal(again.keys, r.keys) and again.res == r.res
        assert np.array_equal(again_not.rows, rn.rows) and again_not.res == rn.res
    got = dict(zip((texts[b] for b in r.rows[: r.res.n_match].tolist()), r.keys.tolist()))
    unmatched = {texts[b] for b in rn.rows[: rn.res.n_match].tolist()}
    assert [got.get(t) for t in c.keys] == [key_texts.index(t) for t in c.keys], "a crafted key's text is not found under its first number"
    assert all(t not in got and t in unmatched for t in c.strangers), "a text that is no key was matched by one with its tag"
    for mode in (0, NOT):
        check_join(run_join(ctx, st.cb, dev, st.n, kdev, ks.n, mode, len(want_join(st, ks, mode)[0]), count_only=True), st, ks, mode)


# --- 5. duplicates -------------------------------------------------------------------------------------------------------------------


def test_duplicate_keys_give_the_lowest_number_every_time(ctx):
    st, ks, info = duplicates_fixture()
    dev, kdev = upload(st), upload(ks)
    texts = [t for _, _, t in judged(st)]
    runs = [join(ctx, st, ks, 0, dev=dev, kdev=kdev) for _ in range(5)]
    for r in runs:
        assert np.array_equal(r.keys, runs[0].keys) and np.array_equal(r.rows, runs[0].rows)
    got = {texts[b]: k for b, k in zip(runs[0].rows[: runs[0].res.n_match].tolist(), runs[0].keys.tolist())}
    assert (got[info.many], got[info.few]) == (info.first_many, info.first_few)
    join(ctx, st, ks, NOT, dev=dev, kdev=kdev)


# --- 6. the [min, max] filter, long records -----------------------------------------------------------------------------------------


def test_records_around_the_keys_smallest_and_largest_body(ctx):
    st, ks = minmax_fixture()
    assert (int(np.diff(ks.body_index).min()), int(np.diff(ks.body_index).max())) == (5, 9)
    assert np.diff(st.body_index).astype(int).tolist() == [4, 5, 5, 5, 9, 9, 10, 10, 7, 4]
    both_modes(ctx, st, ks)
    assert want_join(st, ks, 0) == ([1, 2, 4, 8], [0, 1, 10, 6])


def test_long_records_and_one_pair_at_the_small_stream_limit(ctx):
    st, ks = long_fixture()
    sizes = np.diff(st.body_index).astype(int).tolist()
    assert sizes[1] == sizes[2] == 4096 and sizes[6] == _small_max() // 4
    both_modes(ctx, st, ks)
    assert want_join(st, ks, 0) == ([1, 4, 6, 10, 11], [0, 1, 2, 5, 4])


# --- 7. failures stay local ---------------------------------------------------------------------------------------------------------


def test_failures_stay_local_on_both_sides(ctx):
    st, ks = failures_fixture()
    assert [s for s, _, _ in judged(st)] == [OK, OK, OK, ARG, OK, OK, OK, OK, ARG, ARG, OK, ARG, OK, OK, OK, UNSUPPORTED]
    assert [s for s, _, _ in judged(ks)] == [OK, OK, OK, OK, ARG, OK, OK, ARG, ARG, OK, OK, UNSUPPORTED]
    assert _raw(st, 5) and _raw(ks, 2) and judged(st)[5][:2] == judged(ks)[2][:2]
    dev, kdev = upload(st, spare=st.bodies.size), upload(ks, spare=ks.bodies.size)  # (2^63 is not mapped: a pair that is followed faults or shows)
    r, rn = both_modes(ctx, st, ks, dev=dev, kdev=kdev)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status, r.res.n_keys_failed, r.res.first_key_failed, r.res.first_key_status) == (5, 3, ARG, 4, 4, ARG)
    assert want_join(st, ks, 0) == ([0, 1, 2, 6, 7, 10], [0, 1, 10, 3, 9, 6])
    assert want_join(st, ks, NOT)[0] == [4, 5, 12, 13, 14]  # the record without a body among them; no failed one


# --- 8. modes and outputs -----------------------------------------------------------------------------------------------------------


def test_no_keys_no_records_count_only_and_capacity(ctx):
    st, ks = failures_fixture()
    dev, kdev = upload(st, spare=st.bodies.size), upload(ks, spare=ks.bodies.size)
    none = _store(st.tab, [])
    valid = [b for b, (s, _, _) in enumerate(judged(st)) if not s]
    assert want_join(st, none, 0) == ([], []) and want_join(st, none, NOT)[0] == valid
    both_modes(ctx, st, none, dev=dev)
    # ... with null key pointers too
    import torch

    from entreepy_amd import _native as N

    res = N.JoinResult()
    d_rows = torch.full((len(valid) + TAIL,), -1, dtype=torch.int32, device="cuda")
    rc = N.lib().et_join_packed_device(ctx._h, ctypes.byref(st.cb.raw), dev[0].data_ptr(), dev[0].numel(), dev[1].data_ptr(), dev[2].data_ptr(), st.n, None, 0, None, None, 0, NOT,
                                       d_rows.data_ptr(), len(valid), None, None, None, ctypes.byref(res))
    torch.cuda.synchronize()
    assert (rc, res.n_match, res.n_failed, res.n_keys_failed) == (OK, len(valid), 5, 0) and d_rows[: len(valid)].tolist() == valid and bool((d_rows[len(valid) :] == -1).all())
    # no records: nothing enqueued, *res zeroed
    res = N.JoinResult(n_match=77, n_failed=78, first_failed=79, n_keys_failed=80, first_key_failed=81, first_status=82, first_key_status=83)
    d_key_status = torch.full((ks.n,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = N.lib().et_join_packed_device(ctx._h, ctypes.byref(st.cb.raw), dev[0].data_ptr(), dev[0].numel(), dev[1].data_ptr(), dev[2].data_ptr(), 0, kdev[0].data_ptr(),
                                       kdev[0].numel(), kdev[1].data_ptr(), kdev[2].data_ptr(), ks.n, 0, d_rows.data_ptr(), 4, None, None, d_key_status.data_ptr(), ctypes.byref(res))
    torch.cuda.synchronize()
    assert rc == OK and bytes(res) == bytes(N.JoinResult()) and bool((d_key_status == 0xEE).all()) and bool((d_rows[len(valid) :] == -1).all())
    # count only; cap_rows = the need, and one less
    for mode in (0, NOT):
        need = len(want_join(st, ks, mode)[0])
        exact = run_join(ctx, st.cb, dev, st.n, kdev, ks.n, mode, need)
        check_join(exact, st, ks, mode)
        count = run_join(ctx, st.cb, dev, st.n, kdev, ks.n, mode, need, count_only=True)
        check_join(count, st, ks, mode)
        short = run_join(ctx, st.cb, dev, st.n, kdev, ks.n, mode, need - 1)
        check_join(short, st, ks, mode, call_status=CAP)
        assert count.res == exact.res and dict(vars(short.res), status=OK) == vars(exact.res)
        without = run_join(ctx, st.cb, dev, st.n, kdev, ks.n, mode, need, key_rows=False)
        check_join(without, st, ks, mode)


class _Args:
    """A complete, well-formed argument list in HOST memory: nothing is dereferenced before the checks pass, and every call made
    with it fails one of them."""

    def __init__(self, ctx):
        from entreepy_amd import _native as N

        self.N = N
        self.cb = N.Codebook()
        self.res = N.JoinResult(n_match=77, n_failed=78, first_failed=79, n_keys_failed=80, first_key_failed=81, first_status=82, first_key_status=83)
        self.buf = (ctypes.c_uint64 * 16)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=ctx._h, cb=ctypes.addressof(self.cb), d_bodies=p, body_bytes=16, d_body_index=p, d_text_index=p + 16, n_records=1, d_key_bodies=p + 32, key_body_bytes=16,
                      d_key_body_index=p + 48, d_key_text_index=p + 64, n_keys=1, mode=0, d_rows=p + 80, cap_rows=4, d_key_of_row=p + 96, d_status=None, d_key_status=None,
                      res=ctypes.addressof(self.res))

    def call(self, **changed):
        N, v = self.N, dict(self.v, **changed)
        rc = N.lib().et_join_packed_device(v["ctx"], ctypes.cast(v["cb"], ctypes.POINTER(N.Codebook)) if v["cb"] else None, v["d_bodies"], v["body_bytes"], v["d_body_index"],
                                           v["d_text_index"], v["n_records"], v["d_key_bodies"], v["key_body_bytes"], v["d_key_body_index"], v["d_key_text_index"], v["n_keys"],
                                           v["mode"], v["d_rows"], v["cap_rows"], v["d_key_of_row"], v["d_status"], v["d_key_status"],
                                           ctypes.cast(v["res"], ctypes.POINTER(N.JoinResult)) if v["res"] else None)
        r = self.res
        assert (r.n_match, r.n_failed, r.first_failed, r.n_keys_failed, r.first_key_failed, r.first_status, r.first_key_status) == (77, 78, 79, 80, 81, 82, 83), "*res was touched"
        return rc


def test_every_argument_error_of_the_contract_leaves_res_untouched(ctx):
    a = _Args(ctx)
    for name in ("ctx", "cb", "res", "d_bodies", "d_body_index", "d_text_index", "d_key_bodies", "d_key_body_index", "d_key_text_index"):
        assert a.call(**{name: None}) == ARG, name
    for name in ("d_body_index", "d_text_index", "d_key_body_index", "d_key_text_index"):
        for by in (1, 4):
            assert a.call(**{name: a.v[name] + by}) == ARG, (name, by)
    for name in ("d_rows", "d_key_of_row"):
        for by in (1, 2, 3):
            assert a.call(**{name: a.v[name] + by}) == ARG, (name, by)
    assert a.call(n_records=0x80000000) == ARG and a.call(n_records=1 << 40) == ARG
    assert a.call(n_keys=(1 << 24) + 1) == ARG
    for mode in (1, 2, 0x101, 0x200, -1):
        assert a.call(mode=mode) == ARG, mode
    assert a.call(mode=NOT) == ARG  # (d_key_of_row is given)
    assert a.call(d_rows=None) == ARG  # (key numbers without rows)
    assert _lib().et_join_keys_max() == 1 << 24


def test_an_incomplete_table_is_refused_with_nothing_enqueued(ctx):
    import torch

    import entreepy_amd as E

    data, length = table_ladder()
    data[110], length[110] = 0, 0  # a hole
    d_bodies, d_index = _dev_bytes(np.full(120, 100, np.uint8)), _dev_index(_index_of([50, 70]))
    d_rows = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    d_status = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    d_key_status = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EntreepyError) as e:
        ctx.join_packed_device(_cb((data, length)), d_bodies, d_index, d_index, d_bodies, d_index, d_index, rows=d_rows, status=d_status, key_status=d_key_status)
    assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_rows == -1).all()) and bool((d_status == 0xEE).all()) and bool((d_key_status == 0xEE).all()), "something was enqueued"


# --- 9. hand-made bodies, and the match call ----------------------------------------------------------------------------------------


def test_a_byte_behind_the_last_codeword_equals_the_needle_but_not_the_key(ctx):
    """The documented difference to ET_MATCH_EQUAL: here the byte rule itself is the expectation."""
    st, ks = handmade_fixture()
    dev = upload(st)
    assert [t for _, _, t in judged(st)] == [NEAR_STEM, NEAR_STEM, NEAR_STEM[:5]]
    m = run_match(ctx, st.cb, dev, st.n, NEAR_STEM, EQUAL, 2)
    assert (m.res.status, m.res.n_match) == (OK, 2) and m.rows[:2].tolist() == [0, 1]
    r = run_join(ctx, st.cb, dev, st.n, upload(ks), ks.n, 0, 1)
    check_join(r, st, ks, 0, want=([1], [0]))
    check_join(run_join(ctx, st.cb, dev, st.n, upload(ks), ks.n, NOT, 2), st, ks, NOT, want=([0, 2], [None, None]))


def test_the_rows_are_the_union_of_one_match_call_per_key(ctx):
    st, ks = mixed_fixture()
    dev = upload(st)
    union = set()
    for _, _, text in judged(ks):
        m = run_match(ctx, st.cb, dev, st.n, text, EQUAL, st.n)
        assert m.res.status == OK
        union |= set(m.rows[: m.res.n_match].tolist())
    r = join(ctx, st, ks, 0, dev=dev)
    assert r.rows[: r.res.n_match].tolist() == sorted(union) and {0, 5, 9} <= union
    assert set(r.keys[: r.res.n_match].tolist()) == {0, 1, 3}  # (key 2 is key 1 again)


# --- 10. pipeline and ordering -------------------------------------------------------------------------------------------------------


def test_encode_keys_then_join_then_gather_with_no_synchronisation(ctx):
    """A key column encoded on the device -> join -> rows -> gather on one ctx, nothing in between; then a join under another table."""
    import torch

    st, _ = mixed_fixture()
    wants = judged(st)
    key_texts = [wants[b][2] for b in (17, 3, 200, 17, 0)] + [b"no such record", wants[40][2] + b"x"]
    ks = _store(st.tab, key_texts)
    rows, keys = want_join(st, ks, 0)
    texts = [wants[b][2] for b in rows]
    assert len(rows) >= 4 and all(t in key_texts for t in texts)
    other, other_keys = trap_fixture()
    other_rows, other_key_rows = want_join(other, other_keys, 0)
    dev, dev_other, kdev_other = upload(st), upload(other), upload(other_keys)
    d_key_text = _dev_bytes(np.frombuffer(b"".join(key_texts), np.uint8))
    d_key_text_index = _dev_index(ks.text_index)
    d_key_bodies = torch.full((ks.bodies.size + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_key_body_index = torch.full((ks.n + 1,), -1, dtype=torch.int64, device="cuda")
    d_rows = torch.full((st.n,), -1, dtype=torch.int32, device="cuda")
    d_keys = torch.full((st.n,), -1, dtype=torch.int32, device="cuda")
    d_out = torch.full((sum(len(t) for t in texts) + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_index = torch.full((len(rows) + 1,), -1, dtype=torch.int64, device="cuda")
    d_rows2 = torch.full((other.n,), -1, dtype=torch.int32, device="cuda")
    d_keys2 = torch.full((other.n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e = ctx.encode_packed_device(st.cb, d_key_text, d_key_text_index, d_key_bodies[: ks.bodies.size], d_key_body_index)
    j = ctx.join_packed_device(st.cb, *dev, d_key_bodies[: ks.bodies.size], d_key_body_index, d_key_text_index, rows=d_rows, key_of_row=d_keys)
    g = ctx.decode_packed_gather_device(st.cb, *dev, d_rows[: j.n_match], d_out[: d_out.numel() - TAIL], d_index)
    j2 = ctx.join_packed_device(other.cb, *dev_other, *kdev_other, rows=d_rows2, key_of_row=d_keys2)
    torch.cuda.synchronize()
    assert (e.status, e.out_bytes, e.n_failed) == (OK, ks.bodies.size, 0) and d_key_bodies.cpu().numpy()[: ks.bodies.size].tobytes() == ks.bodies.tobytes()
    assert (j.status, j.n_match, j.n_failed, j.n_keys_failed) == (OK, len(rows), 0, 0) and (g.status, g.n_failed, g.n_short) == (OK, 0, 0)
    assert d_rows[: j.n_match].tolist() == rows and d_keys[: j.n_match].tolist() == keys and bool((d_rows[j.n_match :] == -1).all()) and bool((d_keys[j.n_match :] == -1).all())
    host = d_out.cpu().numpy()
    assert host[: g.out_bytes].tobytes() == b"".join(texts) and bool((host[g.out_bytes :] == SENTINEL).all())
    assert (j2.status, j2.n_match) == (OK, len(other_rows)) and d_rows2[: j2.n_match].tolist() == other_rows and d_keys2[: j2.n_match].tolist() == other_key_rows


@functools.lru_cache(maxsize=None)
def family_fixture():
    """-> (store, 40 key texts, rows, a needle whose pattern is longer than the head).  600 records of 0 .. 40 bytes -- three tiles, the
    last one partial -- under the table of their own text; records 100, 300 and 599 are one text of 30 bytes, record 450 begins with it;
    record 3's body pair decreases (the empty record 4 begins 2 bytes early).  30 keys are records' texts, none empty, 10 are no
    record's.  The rows hold record 3, a number beyond the store, and repeats."""
    rng = np.random.default_rng(0x10A5EA00)
    sizes = rng.integers(0, 41, size=600)
    sizes[3], sizes[4] = 20, 0
    sizes[5::20] = np.maximum(sizes[5::20], 1)
    pool = corpus.text_like(int(sizes.sum()) + 400, 0x10A5EA01)
    cuts = _index_of(sizes)
    texts = [pool[int(cuts[i]) : int(cuts[i + 1])].tobytes() for i in range(600)]
    stem = pool[int(cuts[-1]) : int(cuts[-1]) + 30].tobytes()
    texts[100] = texts[300] = texts[599] = stem
    texts[450] = stem + b"tail"
    st = _store(oracle_table(pool), texts)
    st.body_index[4] = st.body_index[3] - np.uint64(2)
    key_texts = [texts[b] for b in range(5, 600, 20)] + [pool[int(cuts[-1]) + 40 + 36 * i : int(cuts[-1]) + 40 + 36 * i + 33].tobytes() for i in range(10)]
    rows = [int(r) for r in rng.integers(4, 600, size=300)] + [3, 599, st.n + 7, 0, 599]
    return st, key_texts, rows, stem[:24]


def test_every_call_of_the_family_shares_one_upload_region_with_no_synchronisation(ctx):
    """match (a pattern beyond the head) -> encode -> join -> take -> gather -> match (one byte), twice round on one ctx with nothing in
    between: each call refills the pinned region the call before it uploaded from -- table, counters, pattern -- and every result is the
    oracle's, never another run's."""
    import torch

    st, key_texts, rows, needle = family_fixture()
    ks = _store(st.tab, key_texts)
    one = key_texts[0][:1]
    assert len(key_texts) == 40 and pattern_bits(st.tab, needle) > HEAD_BITS and 0 < pattern_bits(st.tab, one) <= HEAD_BITS
    wants = judged(st)
    statuses = [s for s, _, _ in wants]
    assert [b for b, s in enumerate(statuses) if s] == [3] and statuses[3] == ARG
    want_long, want_one = want_match(st, needle, PREFIX), want_match(st, one, PREFIX)
    want_j, want_k = want_join(st, ks, 0)
    assert want_long == [100, 300, 450, 599] and len(want_one) > 4 and len(want_j) >= 30
    taken, gathered = model(st, rows), want_rows(st, rows)
    row_failed = [k for k, s in enumerate(taken.status) if s]
    assert len(row_failed) == 2 and [s for s, _, _ in gathered] == list(taken.status)
    room = sum(r for _, r, _ in gathered)
    g_index = _index_of([r for _, r, _ in gathered])

    dev, d_rows = upload(st), dev_rows(rows)
    d_key_text, d_key_text_index = _dev_bytes(np.frombuffer(b"".join(key_texts), np.uint8)), _dev_index(ks.text_index)

    def outputs():
        u8 = lambda n: torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")  # noqa: E731
        i32 = lambda n: torch.full((n,), -1, dtype=torch.int32, device="cuda")  # noqa: E731
        i64 = lambda n: torch.full((n,), -1, dtype=torch.int64, device="cuda")  # noqa: E731
        return SimpleNamespace(m_rows=i32(st.n), m_status=u8(st.n), key_bodies=u8(ks.bodies.size + TAIL), key_index=i64(ks.n + 1), j_rows=i32(st.n), j_keys=i32(st.n), j_status=u8(st.n),
                               t_out=u8(taken.total + TAIL), t_body_index=i64(len(rows) + 1), t_text_index=i64(len(rows) + 1), t_status=u8(len(rows)), g_out=u8(room + TAIL),
                               g_index=i64(len(rows) + 1), g_status=u8(len(rows)), o_rows=i32(st.n), o_status=u8(st.n))

    rounds = [outputs(), outputs()]
    torch.cuda.synchronize()
    for o in rounds:
        o.m = ctx.match_packed_device(st.cb, *dev, needle, PREFIX, rows=o.m_rows, status=o.m_status)
        o.e = ctx.encode_packed_device(st.cb, d_key_text, d_key_text_index, o.key_bodies[: ks.bodies.size], o.key_index)
        o.j = ctx.join_packed_device(st.cb, *dev, o.key_bodies[: ks.bodies.size], o.key_index, d_key_text_index, rows=o.j_rows, key_of_row=o.j_keys, status=o.j_status)
        o.t = ctx.take_packed_device(*dev, d_rows, o.t_out[: max(taken.total, 1)], o.t_body_index, o.t_text_index, status=o.t_status)
        o.g = ctx.decode_packed_gather_device(st.cb, *dev, d_rows, o.g_out[:room], o.g_index, status=o.g_status)
        o.o = ctx.match_packed_device(st.cb, *dev, one, PREFIX, rows=o.o_rows, status=o.o_status)
    torch.cuda.synchronize()

    def selected(d, want):
        return d[: len(want)].tolist() == want and bool((d[len(want) :] == -1).all())

    for o in rounds:
        for m, d, status, want, bits in ((o.m, o.m_rows, o.m_status, want_long, pattern_bits(st.tab, needle)), (o.o, o.o_rows, o.o_status, want_one, pattern_bits(st.tab, one))):
            assert (m.status, m.n_match, m.n_failed, m.first_failed, m.first_status, m.pattern_bits) == (OK, len(want), 1, 3, ARG, bits), m
            assert selected(d, want) and status.tolist() == statuses
        assert (o.e.status, o.e.out_bytes, o.e.n_failed) == (OK, ks.bodies.size, 0), o.e
        key_bodies = o.key_bodies.cpu().numpy()
        assert key_bodies[: ks.bodies.size].tobytes() == ks.bodies.tobytes() and bool((key_bodies[ks.bodies.size :] == SENTINEL).all())
        assert np.array_equal(o.key_index.cpu().numpy().view(np.uint64), ks.body_index)
        assert (o.j.status, o.j.n_match, o.j.n_failed, o.j.first_failed, o.j.first_status, o.j.n_keys_failed) == (OK, len(want_j), 1, 3, ARG, 0), o.j
        assert selected(o.j_rows, want_j) and selected(o.j_keys, want_k) and o.j_status.tolist() == statuses
        assert (o.t.status, o.t.out_bytes, o.t.text_bytes, o.t.n_failed, o.t.first_failed, o.t.first_status) == (OK, taken.total, taken.text_total, 2, row_failed[0], ARG), o.t
        t_out = o.t_out.cpu().numpy()
        assert t_out[: taken.total].tobytes() == taken.data.tobytes() and bool((t_out[taken.total :] == SENTINEL).all())
        assert np.array_equal(o.t_body_index.cpu().numpy().view(np.uint64), taken.body_index) and np.array_equal(o.t_text_index.cpu().numpy().view(np.uint64), taken.text_index)
        assert o.t_status.tolist() == list(taken.status)
        assert (o.g.status, o.g.out_bytes, o.g.n_failed, o.g.first_failed, o.g.first_status, o.g.n_short) == (OK, room, 2, row_failed[0], ARG, 0), o.g
        g_out = o.g_out.cpu().numpy()
        assert g_out[:room].tobytes() == b"".join(data for _, _, data in gathered) and bool((g_out[room:] == SENTINEL).all())
        assert np.array_equal(o.g_index.cpu().numpy().view(np.uint64), g_index) and o.g_status.tolist() == list(taken.status)



def test_python_calls_give_the_same_rows(ctx):
    import torch

    import entreepy_amd as E

    st, ks = near_fixture()
    rows, keys = want_join(st, ks, 0)
    d_rows = torch.full((st.n,), -1, dtype=torch.int32, device="cuda")
    d_keys = torch.full((st.n,), -1, dtype=torch.int32, device="cuda")
    r = ctx.join_packed_device(st.cb, *upload(st), *upload(ks), rows=d_rows, key_of_row=d_keys)
    torch.cuda.synchronize()
    assert isinstance(r, E.JoinResult) and (r.status, r.n_match, r.n_failed, r.n_keys_failed) == (OK, len(rows), 0, 0)
    assert d_rows[: r.n_match].tolist() == rows and d_keys[: r.n_match].tolist() == keys
    lengths, key_lengths = np.diff(st.text_index), np.diff(ks.text_index)
    assert ctx.join_packed(st.cb, st.bodies.tobytes(), st.body_index, lengths, ks.bodies.tobytes(), ks.body_index, key_lengths) == rows
    assert ctx.join_packed(st.cb, st.bodies.tobytes(), st.body_index, lengths, ks.bodies.tobytes(), ks.body_index, key_lengths, E.MATCH_NOT) == want_join(st, ks, NOT)[0]
    assert ctx.join_packed(st.cb, st.bodies.tobytes(), st.body_index, lengths, b"", np.zeros(1, np.uint64), []) == []
    count = ctx.join_packed_device(st.cb, *upload(st), *upload(ks))
    assert (count.status, count.n_match) == (OK, len(rows))
    short = ctx.join_packed_device(st.cb, *upload(st), *upload(ks), rows=d_rows[: len(rows) - 1])
    assert (short.status, short.n_match) == (CAP, len(rows))
