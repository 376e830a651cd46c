"""The table of tests/retained.py against the header and against the oracle, without a GPU: every context call of
include/entreepy_hip.h has a place in it (a call added later without one fails here), the rows that drop a state are exactly the
named ones, and the fixtures and references of tests/test_gpu_retained.py are what that file takes them for."""
import ctypes
import os
import re

import numpy as np
import pytest

import entreepy_amd as E
from entreepy_amd import _native as N
from oracle import oracle as O
from tests import bitwalk as W
from tests import retained as R
from tests.conftest import ROOT


def _context_calls():
    """Every function of the header whose first parameter is `et_ctx *` or `const et_ctx *`."""
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return re.findall(r"\b(et_[a-z0-9_]+)\s*\(\s*(?:const\s+)?et_ctx\s*\*", header)


def test_every_context_call_has_a_place_in_the_table():
    calls = _context_calls()
    assert len(calls) == len(set(calls)) and len(calls) >= 45, calls
    placed = {c for cs in R.SETTERS.values() for c in cs} | {c for cs in R.READERS.values() for c in cs} | {c for r in R.ROWS for c in r.calls}
    assert not placed & set(R.EXCLUDED), placed & set(R.EXCLUDED)
    missing = [c for c in calls if c not in placed and c not in R.EXCLUDED]
    assert not missing, f"context calls without a row in tests/retained.py (or a reason in EXCLUDED): {missing}"
    unknown = sorted((placed | set(R.EXCLUDED)) - set(calls) - {"et_ctx_create"})  # (whose context is its second parameter, an output)
    assert not unknown, f"tests/retained.py names calls the header does not declare with a context: {unknown}"
    assert all(c in N.SIGNATURES for c in calls)
    assert all(reason for reason in R.EXCLUDED.values())
    # a reader's refusal has its message, and the messages are the library's own
    with open(os.path.join(ROOT, "entreepy_amd", "csrc", "et_api.cpp")) as a, open(os.path.join(ROOT, "entreepy_amd", "csrc", "et_decode.cpp")) as d:
        source = a.read() + d.read()
    for state in (R.HISTOGRAM, R.RANGE):
        for reader in R.READERS[state]:
            assert f'"{R.MISSING[reader]}"' in source, reader


def test_the_rows_that_drop_are_exactly_the_named_ones():
    assert len(set(R.NAMES)) == len(R.NAMES)
    assert {r.name for r in R.ROWS if r.hist == R.DROPS} == R.DROPS_HISTOGRAM and len(R.DROPS_HISTOGRAM) == 7
    assert {r.name for r in R.ROWS if r.held == R.DROPS} == R.DROPS_RANGE and len(R.DROPS_RANGE) == 8
    assert {r.name for r in R.ROWS if r.held == R.REPLACED} == {"range_sync_other", "range_maps_other"}
    for r in R.ROWS:
        assert r.hist in (R.KEEPS, R.DROPS) and r.held in (R.KEEPS, R.DROPS, R.REPLACED), r.name
        assert (r.why is not None) == (R.DROPS in (r.hist, r.held)), f"{r.name}: a row that drops says which buffer it touches, and only such a row"
        assert r.names is None or r.hist == R.DROPS, r.name
        # a whole encode leaves its table behind AND its histogram: the rows that encode are rows that name another text
        assert r.encodes is None or r.names == r.encodes, r.name
        assert (r.name == "nothing") == (not r.calls), r.name
    assert [r.name for r in R.ROWS if r.encodes] == ["encode_device_other", "encode_other", "encode_fd", "batch_encode_delegated"]


def test_the_growing_reserve_grows_what_the_states_live_in():
    """By the library's own sizes (tests/retained.py reserve_growth): the buffers after the setters on the small fixtures are smaller
    than what et_ctx_reserve(RESERVE_GROWS) asks for, and reserve(1) asks for no more than they hold."""
    for name, (held, wanted) in R.reserve_growth().items():
        assert held % 4096 == 0 and 2 * held < wanted, (name, held, wanted)
    assert R.reserve_growth()["tile_hist"][0] == 20480  # 18 tiles of 256 counters
    assert 2 * 1024 <= 20480 and ((1 + 8192) * 8 // 256 + 2) * 4 <= 4096  # reserve(1): two tiles; 258 lanes


def test_the_histogram_fixture_and_its_references():
    """70 001 bytes at byte offset 3 under tiles of one round: more than one tile, a ragged last chunk.  The body the oracle packs at
    start bit 5 and its whole image, against the oracle's own decode of them."""
    text = R.hist_text()
    counts, body, end_bit, image = R.hist_reference()
    assert text.size == R.HIST_N and (R.HIST_OFFSET + R.HIST_N) // (R.HIST_ROUNDS * 4096) >= 17 and (R.HIST_OFFSET + R.HIST_N) % 16
    assert np.array_equal(counts, O.histogram(text)) and int(counts.sum()) == R.HIST_N
    data, length = R.table_of("hist")
    cb = E.Codebook.from_histogram(counts)
    assert np.array_equal(cb.length, length) and np.array_equal(cb.data[length > 0], data[length > 0])  # et_build_codebook is build_dict
    assert end_bit == R.HIST_START_BIT + cb.bits(counts) and len(body) == (end_bit + 7) // 8
    # the packed body decodes to the text: as an image made of the library's header and the body moved to bit 0 ...
    header = cb.header(R.HIST_N)
    assert image.startswith(header) and O.decode(image[4:]) == text.tobytes()
    # ... and bit for bit: the body from bit 5 is the image's body shifted by five bits
    whole = np.unpackbits(np.frombuffer(image[len(header) :], np.uint8))
    shifted = np.unpackbits(np.frombuffer(body, np.uint8))
    n_bits = end_bit - R.HIST_START_BIT
    assert not shifted[: R.HIST_START_BIT].any() and np.array_equal(shifted[R.HIST_START_BIT : end_bit], whole[:n_bits]) and not shifted[end_bit:].any()
    # X's texts have other tables, and the delegated one is above the batch kernels' limit by one byte
    assert not np.array_equal(R.table_of("other")[1], length) and R.big_text().size == N.lib().et_batch_small_max() + 1
    for name in ("other", "big"):
        assert O.decode(R.image(name)) == R.TEXTS[name]().tobytes()


def _path(cb):
    p = ctypes.c_uint32(99)
    assert N.lib().et_decode_path(ctypes.byref(cb.raw), ctypes.byref(p)) == N.ET_OK
    return p.value


@pytest.mark.parametrize("name", ["text", "rows"])
def test_the_range_fixtures_and_their_references(name):
    """Five 8 KiB blocks and a ragged tail; the family the GPU test takes each for; the symbols of the held range and of the range
    that replaces it are the slices of the text that the serial walk says begin in them, which is the oracle's decode."""
    fx = R.range_fixture(name)
    assert fx.n_blocks == 6 and fx.n_bytes % W.BLOCK_BYTES and O.decode(fx.comp) == fx.text.tobytes()
    cb = fx.codebook()
    t = ctypes.c_uint32(999)
    rc = N.lib().et_row_code(ctypes.byref(cb.raw), ctypes.byref(t))
    if name == "text":  # et_decode_range_sync by tree walk; its blind run-in is on the true chain before the range begins
        assert _path(cb) == N.ET_PATH_TREE_WALK and rc == N.ET_ERR_UNSUPPORTED and cb.is_complete()
        assert int(W.merge_distances(fx.L, fx.on_chain)[R.HELD[0] * 8 // W.LANE_BITS]) <= W.RUN_IN_BITS
    else:  # et_decode_range_maps by rows: 255 symbols, one codeword of 7 bits, maps of 8 entries
        assert _path(cb) == N.ET_PATH_ROWS and rc == N.ET_OK and t.value == 1 and (cb.raw.min_length, cb.raw.max_length) == (7, 8)
    exit_, syms = W.walk_symbols(fx.L, fx.S, fx.first_bit, fx.n_bits)
    assert syms[: fx.text.size].tobytes() == fx.text.tobytes()
    bounds = W.boundaries(fx.first_bit, fx.length, fx.text)
    for begin, end in (R.HELD, R.other_range(name)):
        s, x, n, got = fx.truth(begin, end)
        assert s < 8 and x < 32 and (x, n) == fx.range_count(begin, end, s)
        i = int(np.searchsorted(bounds, begin * 8))
        assert bounds[i] == begin * 8 + s and np.array_equal(got[: fx.text.size - i], fx.text[i : i + n])  # (behind the text: codewords in the pad bits)
        assert n > 8000
    assert R.other_range(name)[1] == fx.n_bytes and R.HELD[1] + 16 <= fx.n_bytes
    assert not np.array_equal(fx.truth(*R.HELD)[3][:1000], fx.truth(*R.other_range(name))[3][:1000])  # a replaced range is visible


def test_the_window_family_fixture_holds_its_range_in_the_decode_tables():
    """The third held range: the sparse dictionary's stream of tests/test_syncwork_host.py (which holds its walk against the oracle),
    no tree the walk can hold, so et_decode_range_sync runs the window sweeps over the tables of ctx->lut."""
    fx = R.range_fixture("sparse")
    cb = fx.codebook()
    n_int = ctypes.c_uint32(0)
    assert _path(cb) == N.ET_PATH_WINDOWS and N.lib().et_treewalk_table(ctypes.byref(cb.raw), None, 0, ctypes.byref(n_int)) != N.ET_OK
    s, x, n, syms = fx.truth(*R.HELD)
    assert fx.n_blocks >= 6 and R.HELD[1] + 16 <= fx.n_bytes and s < 32 and x < 32 and n > 8000 and (x, n) == fx.range_count(*R.HELD, s)
    i = int(np.searchsorted(W.boundaries(fx.first_bit, fx.length, fx.text), R.HELD[0] * 8))
    assert np.array_equal(syms, fx.text[i : i + n])


def test_the_packed_store_is_the_oracles():
    data, length, blob, index, lengths = R.store()
    cb = E.Codebook.from_tables(data, length)
    assert cb.is_complete() and index.size == len(R.RECORDS) + 1 and int(index[-1]) == len(blob)
    for r, a, b in zip(R.RECORDS, index[:-1], index[1:]):
        assert cb.encode_pattern(r)[0] == blob[int(a) : int(b)]
        if r:
            assert O.decode(cb.header(len(r))[4:] + blob[int(a) : int(b)]) == r
