"""et_concat_packed_device's row of the table in tests/retained.py: what the call does to the state a context keeps between calls --
nothing: it works in ctx->packed_ws and the packed calls' pinned region, as the slice does, so both the histogram link and the held
range survive it.  The row joins the table when this module is imported, once; tests/test_gpu_concat.py imports it, and with that
tests/test_concat_host.py, and runs the table's cells for it."""
import numpy as np

from tests import retained as R


def _concat(env):
    _, _, blob, index, lengths = R.store()
    store = (blob, index, lengths)
    got, got_index, got_lengths = env.ctx.concat_packed(env.store_cb(), store, b" or ", store, rows_a=[0, 3, 1], rows_b=[1, 0, 3])
    want, want_index = env.ctx.encode_packed(env.store_cb(), [b"to be or or not", b" or to be", b"or not or "])  # RECORDS[0, 3, 1] + " or " + RECORDS[1, 0, 3]
    assert got == want and np.array_equal(got_index, want_index) and got_lengths.tolist() == [15, 9, 10]


ROW = R.Row("concat", ("et_concat_packed_device", "et_encode_packed_device"), _concat)

if ROW.name not in R.NAMES:
    R.ROWS.append(ROW)
    R.NAMES.append(ROW.name)
