"""et_field_packed_device's row of the table in tests/retained.py: what the call does to the state a context keeps between calls --
nothing: it works in ctx->packed_ws and the packed calls' pinned region, as the slice does, so both the histogram link and the held
range survive it.  The row joins the table when this module is imported, once; tests/test_gpu_field.py imports it, and with that
tests/test_field_host.py, and runs the table's cells for it."""
import numpy as np

from tests import retained as R


def _field(env):
    _, _, blob, index, lengths = R.store()
    got, got_index, got_lengths, pos = env.ctx.field_packed(env.store_cb(), blob, index, lengths, [2, 4, 3, 0], 2, 2, delim=b" ")
    want, want_index = env.ctx.encode_packed(env.store_cb(), [b"or not", b"the question", b"", b""])  # words 2 and 3 of RECORDS[2] and [4]; the empty record; no word 2
    assert got == want and np.array_equal(got_index, want_index) and got_lengths.tolist() == [6, 12, 0, 0] and pos.tolist() == [6, 8, 0xFFFFFFFF, 0xFFFFFFFF]


ROW = R.Row("field", ("et_field_packed_device", "et_encode_packed_device"), _field)

if ROW.name not in R.NAMES:
    R.ROWS.append(ROW)
    R.NAMES.append(ROW.name)
