"""GPU: et_number_packed_device -- symbols [first, first + count) of a selection's records, cut in front of a stop byte, READ as
integers on the compressed bytes, and SUM / COUNT / MIN / MAX of them per group -- against ONE Python statement of the rule
(number_rule(): a regular expression, int(), the 32-symbol cap and the int64 bounds) over the oracle's texts sliced as Python slices
them (tests/test_gpu_slice.py's stored_text and py_slice); never the walk the kernels implement.  A row's status is judged from its
record's own two pairs of offsets and from its group number.  Every output array lies between sentinel entries, which stay untouched.

The stores and the rows are made by the *_fixture functions below, without a GPU: tests/test_number_host.py checks on the same
fixtures that the rule stated over tests/bitwalk.py's codeword boundaries agrees with number_rule(), and that they reach the cases
named here: which rows are long, which numbers straddle which edge, which sums wrap."""
import ctypes
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import corpus
from tests import retained_number  # noqa: F401  (the call's row joins the table of tests/retained.py)
from tests.test_gpu_batch import _small_max
from tests.test_gpu_gather import dev_rows, make_store, upload
from tests.test_gpu_packed import _dev_bytes, _dev_index, _index_of
from tests.test_gpu_shared import _cb, want_encode
from tests.test_gpu_slice import bit_at, per_row, py_slice, stored_text  # noqa: F401  (bit_at: for tests/test_number_host.py)
from tests.test_shared_host import canonical, oracle_table, table_255, table_ladder

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED = 0, 6, 7  # et_status
N_OK, N_EMPTY, N_BAD, N_RANGE = 0, 1, 2, 3  # ET_NUMBER_*
TO_END, NONE = 0xFFFFFFFF, 0xFFFFFFFF  # ET_SLICE_TO_END, ET_GROUP_NONE
SYMBOLS_MAX = 32  # et_number_symbols_max()
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LANE_BITS = 256  # what a lane of the workgroup path owns of a block (csrc/et_batch.hip settle_block)
BLOCK_BITS = 65536  # the 8 KiB block the workgroup path stages
GUARD = 4  # sentinel entries in front of and behind every output array
S64, S8 = 0x5E5E5E5E5E5E5E5E, 0xEE  # what they hold


def lane_bytes():
    """What of a body the ask's end can reach (reach()) up to this many bytes is walked by one lane, more by a workgroup."""
    from entreepy_amd import _native as N

    return int(N.lib().et_number_lane_bytes())


def reach(st, r, first, count):
    """The bytes of record r's body that the walk to the ask's end can touch: 4 bytes per symbol in front of the end, and 8
    (csrc/et_batch.h clip_body) -- what decides between the lane and the workgroup."""
    nb, length = int(st.body_index[r + 1] - st.body_index[r]), int(st.text_index[r + 1] - st.text_index[r])
    return min(nb, 4 * min(first + count, length) + 8)


# --- THE rule, and what a call should give ---------------------------------------------------------------------------------------------
GRAMMAR = re.compile(rb"[+-]?[0-9]+")


def number_rule(s):
    """-> (kind, value) of the text s: the header's four kinds; the value is 0 unless the kind is OK."""
    if not s:
        return N_EMPTY, 0
    if len(s) > SYMBOLS_MAX or not GRAMMAR.fullmatch(s):
        return N_BAD, 0
    v = int(s)
    return (N_OK, v) if I64_MIN <= v <= I64_MAX else (N_RANGE, 0)


def wrap64(v):
    """v modulo 2^64, as an int64 holds it."""
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def want_number(st, rows, first, count, stop=None, group_of=None, n_groups=None):
    """-> status, kind, values and texts per row; with n_groups the four aggregates (group_of=None: every row in group 0)."""
    small, body_bytes = _small_max(), st.bodies.size
    rows = np.arange(st.n) if rows is None else np.asarray(rows, dtype=np.int64)
    firsts, counts = per_row(first, rows.size), per_row(count, rows.size)
    if isinstance(stop, bytes):
        (stop,) = stop
    w = SimpleNamespace(status=np.full(rows.size, ARG, np.uint8), kind=np.full(rows.size, N_EMPTY, np.uint8), values=np.zeros(rows.size, np.int64), texts=[b""] * rows.size)
    for k, r in enumerate(int(r) for r in rows):
        if r >= st.n:
            continue
        b0, b1, t0, t1 = (int(x) for x in (st.body_index[r], st.body_index[r + 1], st.text_index[r], st.text_index[r + 1]))
        if not (b0 <= b1 <= body_bytes and t0 <= t1):
            continue
        if t1 - t0 > small or b1 - b0 > 4 * small:
            w.status[k] = UNSUPPORTED
            continue
        if group_of is not None and int(group_of[k]) != NONE and int(group_of[k]) >= n_groups:
            continue
        w.texts[k] = py_slice(stored_text(st, r), firsts[k], counts[k], stop)
        w.status[k] = OK
        w.kind[k], w.values[k] = number_rule(w.texts[k])
    failed = np.flatnonzero(w.status)
    w.counts = {"n_ok": int(((w.kind == N_OK) & (w.status == OK)).sum()), "n_empty": int(((w.kind == N_EMPTY) & (w.status == OK)).sum()), "n_bad": int((w.kind == N_BAD).sum()),
                "n_range": int((w.kind == N_RANGE).sum()), "n_failed": int(failed.size)}
    w.first = (int(failed[0]), int(w.status[failed[0]])) if failed.size else None
    if n_groups is not None:
        w.sum, w.n, w.min, w.max = [0] * n_groups, [0] * n_groups, [I64_MAX] * n_groups, [I64_MIN] * n_groups
        for k in np.flatnonzero((w.status == OK) & (w.kind == N_OK)):
            g = 0 if group_of is None else int(group_of[k])
            if g == NONE:
                continue
            v = int(w.values[k])
            w.sum[g], w.n[g], w.min[g], w.max[g] = wrap64(w.sum[g] + v), w.n[g] + 1, min(w.min[g], v), max(w.max[g], v)
    return w


# --- the fixtures ----------------------------------------------------------------------------------------------------------------------
GRAMMAR_OK = [b"0", b"-0", b"+7", b"007", b"%d" % I64_MAX, b"%d" % I64_MIN, b"0" * 31 + b"1"]
GRAMMAR_BAD = [b"-", b"+", b"+-1", b"1 ", b" 1", b"1a", b"a1", b"1-", b"0" * 32 + b"1"]
GRAMMAR_RANGE = [b"%d" % (I64_MAX + 1), b"%d" % (I64_MIN - 1), b"18446744073709551616", b"1" + b"0" * 31]
STRINGS = [b""] + GRAMMAR_OK + GRAMMAR_BAD + GRAMMAR_RANGE
SHORT_PAD, LONG_PAD = 3, 1500  # symbols in front of the "=" of a record of the grammar fixture
VARIANTS = ("short_open", "short_closed", "long_open", "long_closed")


@functools.lru_cache(maxsize=None)
def grammar_fixture():
    """Every string of the grammar table four times: behind 3 or 1 500 symbols of text and a "=" (the lane's record, the
    workgroup's), the record ending with the string (open) or going on with ";" and text that holds digits (closed) -> (store,
    [texts]); record 4 * i + v is STRINGS[i] in VARIANTS[v]."""
    filler = corpus.text_like(LONG_PAD + 40, 0x4E0B0001).tobytes().replace(b";", b",").replace(b"=", b"-")
    texts = []
    for s in STRINGS:
        for pad in (SHORT_PAD, LONG_PAD):
            texts += [filler[:pad] + b"=" + s, filler[:pad] + b"=" + s + b";x9" + filler[pad : pad + 37]]
    return make_store(oracle_table(np.frombuffer(b"".join(texts) + b" a+-0123456789", np.uint8)), texts), texts


def grammar_rows(variant):
    """-> (rows, first) of the grammar fixture's records of one variant: the ask begins behind the "="."""
    v = VARIANTS.index(variant)
    return np.arange(len(STRINGS)) * 4 + v, (LONG_PAD if v >= 2 else SHORT_PAD) + 1


DIGITS_255 = bytes(b for b in range(2, 256) if b not in b"0123456789+-;")


@functools.lru_cache(maxsize=None)
def edge_fixture():
    """Under table_255 (byte 1: 7 bits, every other: 8): record 0 begins with byte 1, so symbol i > 0 begins at bit 8 i - 1 -- three
    8 KiB blocks of it, with numbers planted around a lane's edge, around the block edge and at the very end of the body; records 1
    .. 4 hold no byte 1 and are et_number_lane_bytes() - 1, + 0, + 1 and + 2 bytes long, a number at their end -> (store, [texts],
    {case: (row, first, the number)})."""
    rng = np.random.default_rng(0x4E0B0002)
    fill = lambda n: bytes(rng.choice(np.frombuffer(DIGITS_255, np.uint8), size=n).tobytes())  # noqa: E731
    n0 = 3 * BLOCK_BITS // 8 - 100
    big = bytearray(b"\x01" + fill(n0 - 1))
    plant = {"lane_edge": (40 * LANE_BITS // 8 - 2, b"-12345"), "lane_edge_32": (90 * LANE_BITS // 8 - 15, b"0" * 13 + b"8999999999999999998"),
             "block_edge": (BLOCK_BITS // 8 - 3, b"+9007199254740993"), "second_block_edge": (2 * BLOCK_BITS // 8 - 18, b"-9223372036854775808")}
    for at, num in plant.values():
        big[at : at + len(num) + 1] = num + b";"
    tail = b"4611686018427387904"
    big[n0 - len(tail) :] = tail
    cases = {case: (0, at, num) for case, (at, num) in plant.items()}
    cases["body_end"] = (0, n0 - len(tail), tail)
    texts = [bytes(big)]
    for r, d in enumerate((-1, 0, 1, 2), start=1):
        num = b"%d" % (1000 + d)
        texts.append(fill(lane_bytes() + d - len(num)) + num)
        cases["threshold%+d" % d] = (r, lane_bytes() + d - len(num), num)
    return make_store(table_255(), texts), texts, cases


def table_digits_2bit():
    return canonical({s: 2 for s in b"0123"})


def table_digit_ladder():
    """The ladder's lengths (1, 2, ..., 31, 32, 32) with the sign and the digits on the longest codewords: "+" 22 bits, "-" 23, "0" 24,
    ..., "8" and "9" 32."""
    symbols = list(range(100, 121)) + list(b"+-0123456789")
    assert len(symbols) == 33
    return canonical({s: min(i + 1, 32) for i, s in enumerate(symbols)})


LADDER_32 = b"0" * 13 + b"8999999999999999998"  # 32 symbols, 13 x 24 + 32 + 18 x 32 bits: OK, and nearly 1 KiB of bits for one parse lane


@functools.lru_cache(maxsize=None)
def tables_fixture():
    """-> {name: (store, [texts], [(row, first, count)])}: the 2-bit table whose four symbols are digits; the digit ladder, numbers of
    32 symbols behind 2 and behind 400 symbols of 20-bit codewords; table_255 is the edge fixture's."""
    rng = np.random.default_rng(0x4E0B0003)
    two = [b"1230", b"0", b"3" * 19, b"3" * 33, bytes(rng.choice(np.frombuffer(b"0123", np.uint8), size=3000).tobytes()), b""]
    asks2 = [(0, 0, TO_END), (0, 1, 2), (1, 0, 1), (2, 0, TO_END), (2, 1, 18), (3, 0, TO_END), (3, 1, 32), (3, 1, 20), (4, 2990, 9), (4, 2968, 32), (4, 100, 33), (4, 2999, TO_END), (5, 0, 5)]
    pad = bytes([119])  # 20 bits
    lad = [pad * 2 + LADDER_32, pad * 400 + LADDER_32, pad * 400 + b"9" * 32, pad * 400 + b"-" + LADDER_32[1:], pad * 400 + b"9" * 33, pad * 2 + b"+8" + pad]
    asksl = [(0, 2, TO_END), (1, 400, TO_END), (2, 400, 32), (3, 400, TO_END), (4, 400, TO_END), (4, 401, TO_END), (5, 2, 2), (5, 2, 3), (1, 413, 19)]
    return {"digits_2bit": (make_store(table_digits_2bit(), two), two, asks2), "digit_ladder": (make_store(table_digit_ladder(), lad), lad, asksl)}


@functools.lru_cache(maxsize=None)
def no_symbol_fixture():
    """What is no symbol, on a lane's record (3 symbols in front) and on a workgroup's (1 500) -> (store, [(row, first)]): per path,
    in this order: a body that goes on with digits behind the record's length; a body cut inside the number (by a byte, and to the
    byte in which the number begins); a record kept raw (no bytes under a length); the empty record.  Then, under the 2-bit digit
    table, texts of 4 k + 3 symbols whose 2 pad bits are SET and read as "3", short and long."""
    st0, _ = grammar_fixture()
    filler = corpus.text_like(LONG_PAD + 40, 0x4E0B0001).tobytes().replace(b";", b",").replace(b"=", b"-")  # (the grammar fixture's: its table codes these bytes)
    texts, bodies, asks = [], [], []
    enc = lambda t: want_encode(st0.tab, t)[1]  # noqa: E731
    for pad in (SHORT_PAD, LONG_PAD):
        head = filler[:pad] + b"="
        whole = enc(head + b"1234567890123")
        at = len(enc(head))  # (the byte in which the number's first bit lies, or the one behind)
        for text, body in ((head + b"1234", whole), (head + b"1234567890123", whole[:-1]), (head + b"1234567890123", whole[: at + 1]), (head + b"77", b""), (b"", b"")):
            asks.append((len(texts), pad + 1))
            texts.append(text)
            bodies.append(body)
    return make_store(st0.tab, texts, bodies), asks


@functools.lru_cache(maxsize=None)
def set_pad_fixture():
    rng = np.random.default_rng(0x4E0B0005)
    texts = [bytes(rng.choice(np.frombuffer(b"012", np.uint8), size=n).tobytes()) for n in (3, 7, 19, 3003, 2403)]
    st = make_store(table_digits_2bit(), texts)
    for r in range(st.n):
        st.bodies[int(st.body_index[r + 1]) - 1] |= 3  # the pad: "11", which reads as "3"
    return st, texts


@functools.lru_cache(maxsize=None)
def column_fixture(n=4097, seed=0x4E0B0006):
    """n CSV lines `<id>,<key>,<amount>,<note>` under the table of their own bytes -> (store, [lines]): the amounts are mostly small
    integers of either sign; every 50th is malformed, every 70th empty, every 90th beyond int64, and some lie near the int64 bounds,
    so that their sum wraps."""
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(n):
        amount = b"%d" % int(rng.integers(-10**6, 10**6))
        if i % 50 == 7:
            amount = b"12x"
        if i % 70 == 9:
            amount = b""
        if i % 90 == 11:
            amount = b"99999999999999999999"
        if i % 40 == 13:
            amount = b"%d" % (I64_MAX - int(rng.integers(0, 1000)))
        if i % 400 == 17:
            amount = b"%d" % (I64_MIN + int(rng.integers(0, 1000)))
        lines.append(b"%d,key-%d,%s,note %d" % (i, int(rng.integers(0, 40)), amount, i % 7))
    return make_store(oracle_table(np.frombuffer(b"".join(lines), np.uint8)), lines), lines


def column_asks(lines):
    """-> the symbol at which field 2 of every line begins: what the field call's d_pos holds."""
    return np.array([len(b",".join(line.split(b",")[:2])) + 1 for line in lines])


@functools.lru_cache(maxsize=None)
def failures_fixture():
    """16 records `v=<number>;`, four of them spoilt as tests/test_gpu_take.py spoils them, one with a length above the small-stream
    limit and one with a body above four times that -- over zeros, which nothing reads -> (store, {bad record: status})."""
    small = _small_max()
    texts = [b"v=%d;" % (100 + i) for i in range(14)]
    st = make_store(oracle_table(np.frombuffer(b"".join(texts), np.uint8)), texts)
    good = int(st.bodies.size)
    st.bodies = np.concatenate((st.bodies, np.zeros(10 + 4 * small + 1, np.uint8)))
    st.body_index = np.concatenate((st.body_index, np.array([good + 10, good + 10 + 4 * small + 1], np.uint64)))
    st.text_index = np.concatenate((st.text_index, st.text_index[-1] + np.array([small + 1, small + 101], np.uint64)))
    st.n = 16
    st.body_index[4] = st.body_index[3] - np.uint64(5)  # a decreasing body pair: record 3 fails; record 4's body begins 5 bytes early
    st.body_index[9] = np.uint64(st.bodies.size + 77)  # a body pair beyond body_bytes: records 8 and 9 fail
    st.text_index[12] = st.text_index[11] - np.uint64(3)  # a decreasing text pair: record 11 fails; record 12 is 3 longer
    return st, {3: ARG, 8: ARG, 9: ARG, 11: ARG, 14: UNSUPPORTED, 15: UNSUPPORTED}


# --- one call and its check ------------------------------------------------------------------------------------------------------------
OUTPUTS = ("values", "kind", "sum", "n", "min", "max", "status")


def _guarded(n, dtype, fill):
    import torch

    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return t, t[GUARD : GUARD + n]


def _dev(v):
    """A per-row argument for the call: a scalar as it is, a device tensor (another call's output) as it is, a list on the device."""
    return v if v is None or np.isscalar(v) or hasattr(v, "data_ptr") else dev_rows(v)


def run_number(ctx, st, dev, rows, first, count, stop=None, group_of=None, n_groups=None, outputs=OUTPUTS):
    """One call, every output that is asked for full of sentinels first, sentinel entries on either side.  rows=None: d_rows == NULL;
    rows, first, count and group_of may be device tensors that another call has just written: nothing lies in between then."""
    import torch

    n = st.n if rows is None else len(rows)
    r = SimpleNamespace(raw={}, view={}, n=n, n_groups=n_groups)
    for name in outputs:
        if name in ("sum", "n", "min", "max") and n_groups is None:
            continue
        size = n if name in ("values", "kind", "status") else n_groups
        r.raw[name], r.view[name] = _guarded(size, torch.uint8 if name in ("kind", "status") else torch.int64, S8 if name in ("kind", "status") else S64)
    v = r.view
    r.res = ctx.number_packed_device(st.cb, *dev, _dev(rows), _dev(first), _dev(count), stop=stop, values=v.get("values"), kind=v.get("kind"), group_of=_dev(group_of),
                                     n_groups=n_groups, sum=v.get("sum"), n=v.get("n"), min=v.get("min"), max=v.get("max"), status=v.get("status"))
    torch.cuda.synchronize()
    r.host = {name: t.cpu().numpy() for name, t in r.raw.items()}
    return r


def check_number(r, want):
    """Every output that was asked for against the rule, the sentinels around it, and the report."""
    for name, host in r.host.items():
        fill = S8 if host.dtype == np.uint8 else S64
        assert (host[:GUARD] == fill).all() and (host[-GUARD:] == fill).all(), f"{name}: a sentinel was overwritten"
        got = host[GUARD:-GUARD]
        expect = {"values": want.values, "kind": want.kind, "status": want.status}[name] if name in ("values", "kind", "status") else np.array(getattr(want, name), dtype=np.int64)
        bad = np.flatnonzero(got != expect)
        assert bad.size == 0, f"{name}[{int(bad[0])}]: got {got[bad[0]]}, want {expect[bad[0]]}" + (f" for {want.texts[int(bad[0])]!r}" if name in ("values", "kind") else "")
    res = r.res
    assert {k: getattr(res, k) for k in want.counts} == want.counts
    assert res.n_ok + res.n_empty + res.n_bad + res.n_range + res.n_failed == r.n and res.status == OK
    if want.first:
        assert (res.first_failed, res.first_status) == want.first
    return r


def number(ctx, st, rows, first, count, stop=None, dev=None, group_of=None, n_groups=None, outputs=OUTPUTS):
    want = want_number(st, rows, first, count, stop, group_of, n_groups)
    r = check_number(run_number(ctx, st, dev or upload(st), rows, first, count, stop, group_of, n_groups, outputs), want)
    r.want = want
    return r


# --- 1. the grammar, on both paths -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_grammar_table(ctx, variant):
    st, _ = grammar_fixture()
    rows, first = grammar_rows(variant)
    r = number(ctx, st, rows, first, TO_END, stop=b";")
    assert r.want.texts == STRINGS
    kinds = dict(zip(STRINGS, r.want.kind.tolist()))
    assert kinds[b""] == N_EMPTY and all(kinds[s] == N_OK for s in GRAMMAR_OK) and all(kinds[s] == N_BAD for s in GRAMMAR_BAD) and all(kinds[s] == N_RANGE for s in GRAMMAR_RANGE)
    values = dict(zip(STRINGS, r.want.values.tolist()))
    assert values[b"-0"] == 0 and values[b"007"] == 7 and values[b"%d" % I64_MIN] == I64_MIN and values[b"0" * 31 + b"1"] == 1 and values[b"1" + b"0" * 31] == 0


# --- 2. the ask ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", ["short_closed", "long_closed"])
def test_first_and_count_as_scalars_and_as_device_arrays(ctx, variant):
    st, _ = grammar_fixture()
    dev = upload(st)
    rows, first = grammar_rows(variant)
    lens = np.array([len(s) for s in STRINGS])
    for count in (0, 1, 5, TO_END):
        a = number(ctx, st, rows, first, count, stop=b";", dev=dev)
        b = number(ctx, st, rows, np.full(rows.size, first), np.full(rows.size, count), stop=b";", dev=dev)
        assert a.res == b.res
    exact = number(ctx, st, rows, first, lens, dev=dev)  # the count ends the number: the stop lies behind it, and none is given
    assert exact.want.texts == STRINGS
    number(ctx, st, rows, first, lens, stop=b";", dev=dev)
    number(ctx, st, rows, first + lens // 2, lens, stop=b";", dev=dev)  # from the middle of the number


@pytest.mark.parametrize("variant", ["short_closed", "long_closed"])
def test_the_edges_of_the_ask(ctx, variant):
    st, texts = grammar_fixture()
    dev = upload(st)
    rows, first = grammar_rows(variant)
    lens = np.array([len(texts[r]) for r in rows])
    for f in (lens, lens + 1, 0xFFFFFFFF):  # first >= len: EMPTY
        r = number(ctx, st, rows, f, TO_END, stop=b";", dev=dev)
        assert (r.want.kind == N_EMPTY).all() and r.res.n_empty == rows.size
    for f, c in ((first, 0xFFFFFFFF), (first, 0xFFFFFFFF - first + 1), (0xFFFFFFFF, 0xFFFFFFFF)):  # first + count past 2^32
        assert f + c >= 1 << 32
        r = number(ctx, st, rows, f, c, stop=b";", dev=dev)
    assert number(ctx, st, rows, first, 0xFFFFFFFF, stop=b";", dev=dev).want.texts == STRINGS
    at_stop = number(ctx, st, rows, first + np.array([len(s) for s in STRINGS]), TO_END, stop=b";", dev=dev)  # the stop at `first` itself
    assert (at_stop.want.kind == N_EMPTY).all()
    absent = number(ctx, st, rows, first, TO_END, stop=None, dev=dev)  # nothing cuts: the rest of the record is the text
    assert all(t.endswith(texts[r][-5:]) for t, r in zip(absent.want.texts, rows)) and (absent.want.kind == N_BAD).all()
    assert int(st.tab[1][0xFF]) == 0
    uncoded = number(ctx, st, rows, first, TO_END, stop=0xFF, dev=dev)  # a stop byte without a code cuts nothing
    assert uncoded.want.texts == absent.want.texts
    digit = number(ctx, st, rows, first, TO_END, stop=b"0", dev=dev)  # a digit as the stop
    assert digit.want.texts[STRINGS.index(b"007")] == b"" and digit.want.texts[STRINGS.index(b"1" + b"0" * 31)] == b"1"


def test_first_from_the_field_calls_positions(ctx):
    import torch

    st, lines = column_fixture()
    dev = upload(st)
    d_pos = torch.full((st.n,), -1, dtype=torch.int32, device="cuda")
    d_index = [torch.empty(st.n + 1, dtype=torch.int64, device="cuda") for _ in range(2)]
    want = want_number(st, None, column_asks(lines), TO_END, b",")
    f = ctx.field_packed_device(st.cb, *dev, None, 2, 1, b",", None, *d_index, pos=d_pos)
    r = check_number(run_number(ctx, st, dev, None, d_pos, TO_END, b","), want)
    assert (f.status, f.n_failed) == (OK, 0) and d_pos.tolist() == column_asks(lines).tolist()
    assert want.texts == [line.split(b",")[2] for line in lines]
    assert r.res.n_bad >= 60 and r.res.n_empty >= 40 and r.res.n_range >= 30 and r.res.n_failed == 0


@functools.lru_cache(maxsize=None)
def pages_fixture():
    """40 pages of text, in most of them `user=<number>;` somewhere: short pages and pages of 3 000 symbols -> (store, [pages])."""
    rng = np.random.default_rng(0x4E0B0007)
    pages = []
    for i in range(40):
        n = 60 if i % 2 else 3000
        text = corpus.text_like(n, 0x4E0B0100 + i).tobytes().replace(b";", b",")
        at = int(rng.integers(0, n - 40))
        value = [b"%d" % int(rng.integers(-10**9, 10**9)), b"", b"12ab", b"%d" % (1 << 64)][i % 9 % 4 if i % 9 < 4 else 0]
        pages.append(text if i % 7 == 6 else text[:at] + b"user=" + value + b";" + text[at:])
    return make_store(oracle_table(np.frombuffer(b"".join(pages), np.uint8)), pages), pages


def test_first_from_the_search_calls_positions_plus_five(ctx):
    import torch

    st, pages = pages_fixture()
    dev = upload(st)
    hits = [k for k, p in enumerate(pages) if b"user=" in p]
    assert 0 < len(hits) < st.n
    d_rows, d_pos = (torch.full((st.n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    s = ctx.search_packed_device(st.cb, *dev, b"user=", 0, rows=d_rows, pos=d_pos)  # SEARCH_CONTAINS
    want = want_number(st, hits, [pages[k].index(b"user=") + 5 for k in hits], TO_END, b";")
    check_number(run_number(ctx, st, dev, d_rows[: len(hits)], d_pos[: len(hits)] + 5, TO_END, b";"), want)
    assert (s.status, s.n_match) == (OK, len(hits)) and d_rows[: len(hits)].tolist() == hits
    assert sorted(set(want.kind.tolist())) == [N_OK, N_EMPTY, N_BAD, N_RANGE]


# --- 3. where the number lies ------------------------------------------------------------------------------------------------------------


def test_numbers_at_the_lane_block_and_body_edges_and_at_the_lane_threshold(ctx):
    st, texts, cases = edge_fixture()
    rows, first, nums = zip(*cases.values())
    r = number(ctx, st, list(rows), list(first), TO_END, stop=b";")
    assert r.want.texts == list(nums) and (r.want.kind == N_OK).all() and r.want.values.tolist() == [int(x) for x in nums]
    exact = number(ctx, st, list(rows), list(first), [len(x) for x in nums])  # by the count, without a stop
    assert exact.want.values.tolist() == r.want.values.tolist()


# --- 4. tables ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["digits_2bit", "digit_ladder"])
def test_tables_whose_digits_are_the_shortest_and_the_longest_codewords(ctx, name):
    st, texts, asks = tables_fixture()[name]
    rows, first, count = (list(x) for x in zip(*asks))
    r = number(ctx, st, rows, first, count)
    assert sorted(set(r.want.kind.tolist())) == [N_OK, N_EMPTY, N_BAD, N_RANGE] if name == "digits_2bit" else N_OK in r.want.kind and N_RANGE in r.want.kind and N_BAD in r.want.kind
    if name == "digit_ladder":
        assert r.want.texts[1] == LADDER_32 and r.want.values[1] == 8999999999999999998 and r.want.values[3] == -8999999999999999998


# --- 5. what is no symbol ----------------------------------------------------------------------------------------------------------------


def test_codewords_behind_the_length_cut_bodies_raw_and_empty_records(ctx):
    st, asks = no_symbol_fixture()
    rows, first = (list(x) for x in zip(*asks))
    r = number(ctx, st, rows, first, TO_END)
    for half in (0, 5):
        texts = r.want.texts[half : half + 5]
        assert texts[0] == b"1234" and b"1234567890123".startswith(texts[1]) and 8 <= len(texts[1]) < 13 and len(texts[2]) <= 3 and b"1234567890123".startswith(texts[2]) and texts[3:] == [b"", b""]
    assert r.res.n_failed == 0 and r.res.n_empty >= 4
    number(ctx, st, rows, first, TO_END, stop=b"5")
    number(ctx, st, rows, 0, 2)  # (in front of the "=": text)


def test_set_pad_bits_that_read_as_a_digit(ctx):
    st, texts = set_pad_fixture()
    r = number(ctx, st, None, 0, TO_END)
    assert r.want.texts == texts
    r = number(ctx, st, None, np.array([len(t) - 3 for t in texts]), 19)
    assert r.want.texts == [t[-3:] for t in texts] and (r.want.kind == N_OK).all()
    r = number(ctx, st, None, np.array([len(t) - 1 for t in texts]), TO_END)
    assert r.want.values.tolist() == [int(t[-1:]) for t in texts]


# --- 6. rows -----------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("selection", ["null", "reversed", "repeated", "257", "4097"])
def test_rows_in_every_order_and_with_repeats(ctx, selection):
    st, lines = column_fixture()
    at = column_asks(lines)
    rng = np.random.default_rng(0x4E0B0008)
    rows = {"null": None, "reversed": np.arange(st.n)[::-1], "repeated": np.repeat(rng.permutation(st.n)[:300], 3), "257": rng.integers(0, st.n, size=257),
            "4097": rng.permutation(st.n)}[selection]
    r = number(ctx, st, rows, at if rows is None else at[rows], TO_END, stop=b",")
    assert r.n == {"null": 4097, "reversed": 4097, "repeated": 900, "257": 257, "4097": 4097}[selection] and r.res.n_failed == 0


def test_failures_stay_local(ctx):
    st, bad = failures_fixture()
    dev = upload(st, spare=4096)  # (what lies behind body_bytes is mapped: a pair that is followed shows as a wrong value)
    rows = np.array([0, 16, 1, 3, 2, 0xFFFFFFFF, 8, 4, 15, 9, 5, 11, 6, 14, 12, 13, 7, 10, 3, 0], dtype=np.uint32)
    r = number(ctx, st, rows, 2, TO_END, stop=b";", dev=dev, n_groups=1)
    assert [int(s) for s in r.want.status] == [bad.get(int(x), OK) if x < 16 else ARG for x in rows]
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (9, 1, ARG)
    failed = np.flatnonzero(r.want.status)
    assert (r.want.kind[failed] == N_EMPTY).all() and not r.want.values[failed].any()  # EMPTY, value 0 ...
    assert r.res.n_empty == r.want.counts["n_empty"] < rows.size - 9 and r.want.n[0] == r.res.n_ok  # ... and counted in n_failed only
    r = number(ctx, st, np.array([0, 1, 2, 15, 9, 3], dtype=np.uint32), 2, TO_END, stop=b";", dev=dev)  # the lowest failing row is not the first failing record
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 3, UNSUPPORTED)
    r = number(ctx, st, np.array([13, 0, 1, 2, 5, 6, 7, 10, 13], dtype=np.uint32), 2, TO_END, stop=b";", dev=dev)  # a bad record that no row selects does not matter
    assert r.res.n_failed == 0 and r.want.values.tolist() == [113, 100, 101, 102, 105, 106, 107, 110, 113]


# --- 7. aggregates -----------------------------------------------------------------------------------------------------------------------


def _column(n):
    st, lines = column_fixture()
    rows = np.arange(n)
    return st, rows, column_asks(lines)[:n]


def test_whole_column_aggregates_without_group_numbers(ctx):
    st, rows, at = _column(513)
    r = number(ctx, st, rows, at, TO_END, stop=b",", n_groups=1)
    assert r.want.n[0] == r.res.n_ok > 400 and r.want.min[0] < I64_MIN + 1000 and r.want.max[0] > I64_MAX - 1000


def test_513_groups_of_one(ctx):
    st, rows, at = _column(513)
    r = number(ctx, st, rows, at, TO_END, stop=b",", group_of=np.arange(513)[::-1], n_groups=513)
    assert sorted(set(r.want.n)) == [0, 1]
    empty = [g for g in range(513) if r.want.n[g] == 0]  # a group with no OK row keeps the first values
    assert empty and all((r.want.sum[g], r.want.min[g], r.want.max[g]) == (0, I64_MAX, I64_MIN) for g in empty)


def test_one_group_on_nine_tenths_of_4096_rows_none_rows_and_sums_that_wrap(ctx):
    st, rows, at = _column(4096)
    rng = np.random.default_rng(0x4E0B0009)
    group_of = np.where(rng.random(4096) < 0.9, 3, rng.integers(0, 8, size=4096)).astype(np.uint32)
    group_of[rng.random(4096) < 0.05] = NONE
    r = number(ctx, st, rows, at, TO_END, stop=b",", group_of=group_of, n_groups=8)
    ok = (r.want.kind == N_OK) & (group_of == 3)
    true_sum = sum(int(v) for v in r.want.values[ok])
    assert r.want.n[3] > 3000 and true_sum > I64_MAX and r.want.sum[3] == wrap64(true_sum) != true_sum  # the sum wraps modulo 2^64
    assert r.want.min[3] < 0 and sum(r.want.n) < r.res.n_ok  # negative minima; the rows of ET_GROUP_NONE are skipped


def test_a_group_number_equal_to_n_groups_fails_its_row_alone(ctx):
    st, rows, at = _column(300)
    group_of = (np.arange(300) % 5).astype(np.uint32)
    group_of[[7, 70, 299]] = [5, 0x7FFFFFFF, 0xFFFFFFFE]
    r = number(ctx, st, rows, at, TO_END, stop=b",", group_of=group_of, n_groups=5)
    assert (r.res.n_failed, r.res.first_failed, r.res.first_status) == (3, 7, ARG) and r.want.status[[7, 70, 299]].tolist() == [ARG] * 3


@pytest.mark.parametrize("which", ["sum", "n", "min", "max"])
def test_each_aggregate_alone(ctx, which):
    st, rows, at = _column(700)
    group_of = (np.arange(700) % 3).astype(np.uint32)
    number(ctx, st, rows, at, TO_END, stop=b",", group_of=group_of, n_groups=3, outputs=(which,))


def test_three_identical_runs(ctx):
    st, rows, at = _column(4096)
    dev = upload(st)
    group_of = (np.random.default_rng(0x4E0B000A).integers(0, 17, size=4096)).astype(np.uint32)
    runs = [number(ctx, st, rows, at, TO_END, stop=b",", dev=dev, group_of=group_of, n_groups=17) for _ in range(3)]
    for r in runs[1:]:
        assert r.res == runs[0].res and all(np.array_equal(r.host[k], runs[0].host[k]) for k in r.host)


# --- 8. a call that only counts, the call's own errors ------------------------------------------------------------------------------------


def test_a_count_only_call_agrees_with_the_writing_call(ctx):
    st, lines = column_fixture()
    dev, at = upload(st), column_asks(lines)
    rows = np.concatenate((np.arange(600), [st.n + 3]))
    first = np.concatenate((at[:600], [0]))
    full = number(ctx, st, rows, first, TO_END, stop=b",", dev=dev)
    count = number(ctx, st, rows, first, TO_END, stop=b",", dev=dev, outputs=("status",))
    bare = number(ctx, st, rows, first, TO_END, stop=b",", dev=dev, outputs=())
    assert full.res == count.res == bare.res and full.res.n_failed == 1 and np.array_equal(full.host["status"], count.host["status"])


def test_no_rows_is_ok_zeroes_the_result_and_leaves_the_aggregates(ctx):
    import torch

    from entreepy_amd import _native as N

    st, _ = grammar_fixture()
    d_bodies, d_body_index, d_text_index = upload(st)
    d_rows, d_sum = dev_rows([1, 2]), torch.full((4,), S64, dtype=torch.int64, device="cuda")
    res = N.NumberResult(n_ok=71, n_empty=72, n_bad=73, n_range=74, n_failed=75, first_failed=76, first_status=77)
    rc = N.lib().et_number_packed_device(ctx._h, ctypes.byref(st.cb.raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n,
                                         d_rows.data_ptr(), 0, None, 0, None, 5, -1, None, None, d_rows.data_ptr(), 4, d_sum.data_ptr(), None, None, None, None, ctypes.byref(res))
    torch.cuda.synchronize()
    assert (rc, res.n_ok, res.n_empty, res.n_bad, res.n_range, res.n_failed, res.first_failed, res.first_status) == (OK, 0, 0, 0, 0, 0, 0, 0)
    assert bool((d_sum == S64).all())  # nothing enqueued: the aggregates are not initialised either


def test_an_incomplete_table_is_refused_with_nothing_enqueued(ctx):
    import torch

    import entreepy_amd as E

    data, length = table_ladder()
    data[110], length[110] = 0, 0  # a hole
    d_bodies, d_index = _dev_bytes(np.full(120, 100, np.uint8)), _dev_index(_index_of([50, 70]))
    d_values, d_sum = (torch.full((2,), S64, dtype=torch.int64, device="cuda") for _ in range(2))
    d_status = torch.full((2,), S8, dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EntreepyError) as e:
        ctx.number_packed_device(_cb((data, length)), d_bodies, d_index, d_index, None, 0, TO_END, values=d_values, sum=d_sum, n_groups=1, status=d_status)
    assert e.value.status == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_values == S64).all()) and bool((d_sum == S64).all()) and bool((d_status == S8).all()), "something was enqueued"


def test_the_argument_errors_of_the_aggregates_leave_res_untouched(ctx):
    import torch

    from entreepy_amd import _native as N

    st, _ = grammar_fixture()
    d_bodies, d_body_index, d_text_index = upload(st)
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    res = N.NumberResult(n_ok=71, n_empty=72, n_bad=73, n_range=74, n_failed=75, first_failed=76, first_status=77)

    def call(**changed):
        v = dict(stop=-1, d_values=p, d_kind=p + 64, d_group_of=p + 128, n_groups=2, d_sum=p + 192, d_n=p + 256, d_min=p + 320, d_max=p + 384)
        v.update(changed)
        rc = N.lib().et_number_packed_device(ctx._h, ctypes.byref(st.cb.raw), d_bodies.data_ptr(), d_bodies.numel(), d_body_index.data_ptr(), d_text_index.data_ptr(), st.n, None,
                                             st.n, None, 0, None, 5, v["stop"], v["d_values"], v["d_kind"], v["d_group_of"], v["n_groups"], v["d_sum"], v["d_n"], v["d_min"], v["d_max"],
                                             None, ctypes.byref(res))
        assert (res.n_ok, res.n_empty, res.n_bad, res.n_range, res.n_failed, res.first_failed, res.first_status) == (71, 72, 73, 74, 75, 76, 77), "*res was touched"
        return rc

    for name, at in (("d_values", p), ("d_sum", p + 192), ("d_n", p + 256), ("d_min", p + 320), ("d_max", p + 384)):
        for by in (1, 4):
            assert call(**{name: at + by}) == ARG, (name, by)
    for by in (1, 2, 3):
        assert call(d_group_of=p + 128 + by) == ARG
    assert call(d_sum=None, d_n=None, d_min=None, d_max=None) == ARG  # group numbers without an aggregate output
    assert call(n_groups=0) == ARG and call(n_groups=0x80000000) == ARG and call(n_groups=1 << 40) == ARG
    assert call(d_group_of=None, n_groups=2) == ARG  # without group numbers every row is in group 0
    # the order: the slice call's errors first, then alignment, then the aggregates' own
    why = lambda **changed: (call(**changed), N.lib().et_last_error(ctx._h).decode())  # noqa: E731
    assert "stop" in why(stop=256, d_values=p + 1, n_groups=0)[1] and "8-byte" in why(d_values=p + 1, d_group_of=p + 129, n_groups=0)[1]
    assert "4-byte" in why(d_group_of=p + 129, n_groups=0)[1] and "without an aggregate" in why(d_sum=None, d_n=None, d_min=None, d_max=None, n_groups=0)[1]
    assert "without a group" in why(n_groups=0)[1] and "too many" in why(d_group_of=None, n_groups=1 << 40)[1]
    torch.cuda.synchronize()
    assert not buf.any()


# --- 9. pipelines on one ctx with nothing in between --------------------------------------------------------------------------------------


def test_field_then_group_then_number_gives_the_sums_per_key(ctx):
    """SELECT key, SUM(amount), COUNT(amount), MIN(amount), MAX(amount) ... GROUP BY key over a CSV store, against split and a dict."""
    import torch

    st, lines = column_fixture()
    dev = upload(st)
    keys = [line.split(b",")[1] for line in lines]
    distinct = list(dict.fromkeys(keys))
    want = want_number(st, None, column_asks(lines), TO_END, b",", group_of=[distinct.index(k) for k in keys], n_groups=len(distinct))
    by_key = {}
    for line in lines:
        key, amount = line.split(b",")[1:3]
        if number_rule(amount)[0] == N_OK:
            by_key.setdefault(key, []).append(int(amount))
    assert want.sum == [wrap64(sum(by_key[k])) for k in distinct] and want.n == [len(by_key[k]) for k in distinct] and want.min == [min(by_key[k]) for k in distinct]
    i64 = lambda n: torch.full((n,), -1, dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda n: torch.full((n,), -1, dtype=torch.int32, device="cuda")  # noqa: E731
    f_out, f_body_index, f_text_index = torch.empty(st.bodies.size, dtype=torch.uint8, device="cuda"), i64(st.n + 1), i64(st.n + 1)
    d_pos, p_index = i32(st.n), [i64(st.n + 1), i64(st.n + 1)]
    g_first, g_of = i32(st.n), i32(st.n)
    k = len(distinct)
    agg = {name: i64(k) for name in ("sum", "n", "min", "max")}
    d_values = i64(st.n)
    torch.cuda.synchronize()
    f = ctx.field_packed_device(st.cb, *dev, None, 1, 1, b",", f_out, f_body_index, f_text_index)
    g = ctx.group_packed_device(st.cb, f_out, f_body_index, f_text_index, first_rows=g_first, group_of=g_of)
    p = ctx.field_packed_device(st.cb, *dev, None, 2, 1, b",", None, *p_index, pos=d_pos)
    n = ctx.number_packed_device(st.cb, *dev, None, d_pos, TO_END, stop=b",", values=d_values, group_of=g_of, n_groups=k, **agg)
    torch.cuda.synchronize()
    assert (f.status, f.n_failed, g.status, g.n_groups, g.n_failed, p.status, p.n_failed) == (OK, 0, OK, k, 0, OK, 0)
    assert {name: getattr(n, name) for name in want.counts} == want.counts and d_values.tolist() == want.values.tolist()
    assert [keys[b] for b in g_first[:k].tolist()] == distinct
    assert agg["sum"].tolist() == want.sum and agg["n"].tolist() == want.n and agg["min"].tolist() == want.min and agg["max"].tolist() == want.max


def test_number_then_a_decode_of_the_same_store(ctx):
    import torch

    st, lines = column_fixture()
    dev = upload(st)
    total = int(st.text_index[-1])
    d_values, d_text = torch.empty(st.n, dtype=torch.int64, device="cuda"), torch.full((total + 64,), S8, dtype=torch.uint8, device="cuda")
    want = want_number(st, None, column_asks(lines), TO_END, b",")
    n = ctx.number_packed_device(st.cb, *dev, None, dev_rows(column_asks(lines)), TO_END, stop=b",", values=d_values)
    d = ctx.decode_packed_device(st.cb, *dev, d_text[:total])
    torch.cuda.synchronize()
    assert n.n_ok == want.counts["n_ok"] and d_values.tolist() == want.values.tolist()
    assert (d.status, d.n_failed, d.n_short) == (OK, 0, 0) and d_text[:total].cpu().numpy().tobytes() == b"".join(lines) and bool((d_text[total:] == S8).all())


def test_the_list_helper(ctx):
    import entreepy_amd as E

    st, lines = column_fixture()
    rows = list(range(0, 600, 3))
    at = column_asks(lines)[rows]
    want = want_number(st, rows, at, TO_END, b",", group_of=[r % 4 for r in rows], n_groups=4)
    store = (st.bodies.tobytes(), st.body_index, np.diff(st.text_index))
    values, kinds = ctx.number_packed(st.cb, *store, rows, at, E.SLICE_TO_END, stop=b",")
    assert values.dtype == np.int64 and kinds.dtype == np.uint8 and values.tolist() == want.values.tolist() and kinds.tolist() == want.kind.tolist()
    got = ctx.number_packed(st.cb, *store, rows, at, E.SLICE_TO_END, stop=b",", group_of=[r % 4 for r in rows], n_groups=4)
    assert [a.tolist() for a in got[2:]] == [want.sum, want.n, want.min, want.max] and got[3].dtype == np.uint64
    assert (E.NUMBER_OK, E.NUMBER_EMPTY, E.NUMBER_BAD, E.NUMBER_RANGE) == (N_OK, N_EMPTY, N_BAD, N_RANGE)
    assert [a.size for a in ctx.number_packed(st.cb, *store, [], 0, 1)] == [0, 0]
    with pytest.raises(E.EntreepyError) as e:
        ctx.number_packed(st.cb, *store, [0, st.n], 0, 1)
    assert e.value.status == ARG


# --- 10. the state a context keeps between calls -------------------------------------------------------------------------------------------
# The cells of tests/test_gpu_retained.py for the row `number` (tests/retained_number.py): a number call between the call that sets a
# state and the calls that read it leaves the histogram link, the held range and the last codebook as they were.


@pytest.mark.parametrize("reader", ["body", "head", "on_host"])
def test_histogram_link_survives_a_number_call(reader):
    from tests import test_gpu_retained as G

    G.test_histogram_link("number", reader)


@pytest.mark.parametrize("how", ["sync", "maps", "between", "windows"])
def test_held_range_survives_a_number_call(how):
    from tests import test_gpu_retained as G

    G.test_held_range("number", how)


def test_last_codebook_survives_a_number_call():
    from tests import test_gpu_retained as G

    G.test_last_codebook("number")
