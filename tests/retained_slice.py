"""et_slice_packed_device's row of the table in tests/retained.py: what the call does to the state a context keeps between calls --
nothing: it works in ctx->packed_ws and the packed calls' pinned region, as the take does, so both the histogram link and the held
range survive it.  The row joins the table when this module is imported, once; tests/test_gpu_slice.py imports it, and with that
tests/test_slice_host.py, and runs the table's cells for it."""
import numpy as np

from tests import retained as R


def _slice(env):
    _, _, blob, index, lengths = R.store()
    got, got_index, got_lengths = env.ctx.slice_packed(env.store_cb(), blob, index, lengths, [2, 4, 3], 3, 9, stop=b"t")
    want, want_index = env.ctx.encode_packed(env.store_cb(), [b"be or no", b"", b""])  # RECORDS[2][3:12] and RECORDS[4][3:12], cut in front of "t"; the empty record
    assert got == want and np.array_equal(got_index, want_index) and got_lengths.tolist() == [8, 0, 0]


ROW = R.Row("slice", ("et_slice_packed_device", "et_encode_packed_device"), _slice)

if ROW.name not in R.NAMES:
    R.ROWS.append(ROW)
    R.NAMES.append(ROW.name)
