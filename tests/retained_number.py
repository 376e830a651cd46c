"""et_number_packed_device's row of the table in tests/retained.py: what the call does to the state a context keeps between calls --
nothing: it works in ctx->packed_ws and the packed calls' pinned region, as the slice does, so both the histogram link and the held
range survive it.  The row joins the table when this module is imported, once; tests/test_gpu_number.py imports it, and with that
tests/test_number_host.py, and runs the table's cells for it."""
import numpy as np

from tests import retained as R


def _number(env):
    _, _, blob, index, lengths = R.store()
    # RECORDS[2][3:12] and RECORDS[4][3:12], cut in front of "t", and the empty record: the table's records hold no digit
    values, kinds, sums, counts, minima, maxima = env.ctx.number_packed(env.store_cb(), blob, index, lengths, [2, 4, 3], 3, 9, stop=b"t", n_groups=1)
    assert kinds.tolist() == [2, 1, 1] and not values.any()  # "be or no" is BAD; "" is EMPTY
    assert (sums.tolist(), counts.tolist(), minima.tolist(), maxima.tolist()) == ([0], [0], [np.iinfo(np.int64).max], [np.iinfo(np.int64).min])


ROW = R.Row("number", ("et_number_packed_device",), _number)

if ROW.name not in R.NAMES:
    R.ROWS.append(ROW)
    R.NAMES.append(ROW.name)
