"""et_group_packed_device's row of the table in tests/retained.py: what the call does to the state a context keeps between calls --
nothing: it works in ctx->packed_ws and the packed calls' pinned region, as the join does, so both the histogram link and the held
range survive it.  The row joins the table when this module is imported, once; tests/test_gpu_group.py imports it, and with that
tests/test_group_host.py, and runs the table's cells for it."""
from tests import retained as R


def _group(env):
    _, _, blob, index, lengths = R.store()
    # RECORDS twice over: every text a second time, five groups of two in the order of RECORDS
    first_rows, counts, group_of = env.ctx.group_packed(env.store_cb(), blob + blob, list(index) + [int(index[-1]) + int(i) for i in index[1:]], list(lengths) * 2)
    assert first_rows.tolist() == [0, 1, 2, 3, 4] and counts.tolist() == [2] * 5 and group_of.tolist() == [0, 1, 2, 3, 4] * 2


ROW = R.Row("group", ("et_group_packed_device",), _group)

if ROW.name not in R.NAMES:
    R.ROWS.append(ROW)
    R.NAMES.append(ROW.name)
