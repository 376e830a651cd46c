"""et_take_packed_device's C ABI as far as it can be checked without a GPU: declared, bound, exported, the argument check that comes
before anything touches a device -- every call-level ET_ERR_ARG, with a null ctx, *res untouched -- and the fixtures of
tests/test_gpu_take.py: numpy's take of them (model()) is a store the oracle decodes to exactly the selected texts."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from entreepy_amd import _native as N
from tests.test_gpu_shared import want_decode
from tests.test_gpu_take import ARG, OK, SELECTIONS, SMALL_SIZES, UNSUPPORTED, empties_store, empty_run_rows, failures_store, mixed_store, model, selection, small_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "et_take_packed_device"


def test_take_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "entreepy_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r" T (et_[a-z0-9_]+)", out))
    for name in (NAME, "et_take_result_size"):
        assert name in declared and name in N.SIGNATURES and name in exported, name
    args = re.search(r"int et_take_packed_device\(([^;]*)\);", header).group(1)
    assert len(N.SIGNATURES[NAME][1]) == len(args.split(",")) == 14 and "et_codebook" not in args
    assert N.lib().et_take_result_size() == ctypes.sizeof(N.TakeResult) == 40


def test_the_python_layer_exposes_the_call_the_list_helper_and_the_result():
    import entreepy_amd as E

    assert callable(E.Context.take_packed_device) and callable(E.Context.take_packed)
    assert [f for f in E.TakeResult.__dataclass_fields__] == ["status", "out_bytes", "text_bytes", "n_failed", "first_failed", "first_status"]


class _Args:
    """A complete, well-formed argument list in host memory (nothing is dereferenced before the checks pass)."""

    def __init__(self):
        self.res = N.TakeResult(out_bytes=77, text_bytes=78, n_failed=79, first_failed=80, first_status=81)
        self.buf = (ctypes.c_uint64 * 64)()  # 8-byte aligned
        p = ctypes.addressof(self.buf)
        self.v = dict(ctx=None, d_bodies=p, body_bytes=16, d_body_index=p + 64, d_text_index=p + 80, n_records=1, d_rows=p + 96, n_rows=1, d_out=p + 128, cap=16,
                      d_out_body_index=p + 160, d_out_text_index=p + 176, d_status=None, res=ctypes.addressof(self.res))

    def call(self, **changed):
        v = dict(self.v, **changed)
        rc = N.lib().et_take_packed_device(v["ctx"], v["d_bodies"], v["body_bytes"], v["d_body_index"], v["d_text_index"], v["n_records"], v["d_rows"], v["n_rows"], v["d_out"], v["cap"],
                                           v["d_out_body_index"], v["d_out_text_index"], v["d_status"], ctypes.cast(v["res"], ctypes.POINTER(N.TakeResult)) if v["res"] else None)
        r = self.res
        assert (r.out_bytes, r.text_bytes, r.n_failed, r.first_failed, r.first_status) == (77, 78, 79, 80, 81), "*res was touched"
        return rc


def test_null_context_is_an_argument_error():
    assert _Args().call() == ARG
    assert N.lib().et_take_packed_device(None, None, 0, None, None, 0, None, 0, None, 0, None, None, None, None) == ARG


@pytest.mark.parametrize("name", ["res", "d_bodies", "d_body_index", "d_text_index", "d_rows", "d_out_body_index", "d_out_text_index"])
def test_every_null_pointer_is_an_argument_error_before_a_device_is_touched(name):
    assert _Args().call(**{name: None}) == ARG


@pytest.mark.parametrize("name", ["d_body_index", "d_text_index", "d_out_body_index", "d_out_text_index"])
@pytest.mark.parametrize("by", [1, 4])
def test_a_misaligned_offset_array_is_an_argument_error(name, by):
    a = _Args()
    assert a.call(**{name: a.v[name] + by}) == ARG


@pytest.mark.parametrize("by", [1, 2, 3])
def test_misaligned_rows_are_an_argument_error(by):
    a = _Args()
    assert a.call(d_rows=a.v["d_rows"] + by) == ARG


@pytest.mark.parametrize("name", ["n_records", "n_rows"])
def test_more_than_2_31_records_or_rows_are_an_argument_error(name):
    assert _Args().call(**{name: 0x80000000}) == ARG
    assert _Args().call(**{name: 1 << 40}) == ARG


@pytest.mark.parametrize("where", ["same", "out_begins_inside", "out_ends_inside", "out_around", "last_byte", "first_byte"])
def test_an_output_that_overlaps_the_bodies_is_an_argument_error(where):
    a = _Args()
    b = a.v["d_bodies"]  # the bodies are [b, b + 16)
    d_out, cap = {"same": (b, 16), "out_begins_inside": (b + 8, 16), "out_ends_inside": (b - 8, 16), "out_around": (b - 8, 48), "last_byte": (b + 15, 4),
                  "first_byte": (b - 3, 4)}[where]
    assert a.call(d_out=d_out, cap=cap) == ARG


# --- the fixtures of tests/test_gpu_take.py -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", SELECTIONS)
def test_the_model_of_the_mixed_store_decodes_to_the_selected_texts(name):
    st, texts = mixed_store()
    lengths = [len(t) for t in texts]
    assert st.n == 300 and min(lengths) == 0 and max(lengths) == 5000 and 1 in lengths
    rows = selection(name, st.n)
    want = model(st, rows)
    assert not want.status.any() and want.total == int(want.body_index[-1]) == want.data.size and want.text_total == sum(lengths[int(r)] for r in rows)
    for k, r in enumerate(rows):
        b0, b1, count = int(want.body_index[k]), int(want.body_index[k + 1]), int(want.text_index[k + 1] - want.text_index[k])
        assert want_decode(st.tab, want.data[b0:b1].tobytes(), count) == (OK, texts[int(r)]), (k, int(r))


def test_the_small_and_empty_fixtures_are_what_the_gpu_tests_take_them_for():
    st = small_store()
    assert sorted(set(int(x) for x in np.diff(st.body_index))) == SMALL_SIZES and st.n == 360
    e = empties_store()
    assert [int(x) for x in np.diff(e.body_index)] == [0, 50, 70, 0] and [int(x) for x in np.diff(e.text_index)] == [0, 60, 80, 9]
    for place in ("between", "start", "end"):
        for run in (1, 63, 64, 257, 5000):
            rows = empty_run_rows(run, place)
            want = model(e, rows)
            assert rows.size == run + 2 and want.total == 120 and not want.status.any()
            firsts = {"between": (0, rows.size - 1), "start": (run, run + 1), "end": (0, 1)}[place]  # where the two bodies are
            assert [int(rows[i]) for i in firsts] == [1, 2] and int(np.count_nonzero(np.diff(want.body_index))) == 2
    want = model(e, [0, 3, 0])
    assert want.total == 0 and want.text_total == 9 and want.data.size == 0


def test_the_failures_fixture_fails_the_rows_it_is_meant_to():
    st, bad = failures_store()
    want = model(st, np.arange(18))
    assert [int(s) for s in want.status] == [bad.get(r, OK) for r in range(16)] + [ARG, ARG]
    assert set(bad.values()) == {ARG, UNSUPPORTED}
    body_sizes = np.diff(st.body_index.astype(np.int64))
    assert body_sizes[15] == 4 * N.lib().et_batch_small_max() + 1 and not st.bodies[int(st.body_index[15]) :].any()  # over zeros
    for k in np.flatnonzero(want.status):  # a failed row is an empty record
        assert want.body_index[k] == want.body_index[k + 1] and want.text_index[k] == want.text_index[k + 1]
