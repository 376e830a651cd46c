"""et_recode_packed_device's row of the table in tests/retained.py: what the call does to the state a context keeps between calls --
nothing: it works in ctx->packed_ws and the packed calls' pinned region, as the slice does, so both the histogram link and the held
range survive it.  The row joins the table when this module is imported, once; tests/test_gpu_recode.py imports it, and with that
tests/test_recode_host.py, and runs the table's cells for it."""
import numpy as np

from tests import retained as R


def _recode(env):
    import entreepy_amd as E

    _, _, blob, index, lengths = R.store()
    swap = E.byte_map(b"ot", b"to", delete=b" ")  # (bytes of the store's own table: the one table serves both ways)
    got, got_index, got_lengths = env.ctx.recode_packed(env.store_cb(), env.store_cb(), blob, index, lengths, rows=[0, 3, 1], byte_map=swap)
    want, want_index = env.ctx.encode_packed(env.store_cb(), [b"otbe", b"", b"trnto"])  # RECORDS[0, 3, 1], o and t swapped, the blanks gone
    assert got == want and np.array_equal(got_index, want_index) and got_lengths.tolist() == [4, 0, 5]


ROW = R.Row("recode", ("et_recode_packed_device", "et_encode_packed_device"), _recode)

if ROW.name not in R.NAMES:
    R.ROWS.append(ROW)
    R.NAMES.append(ROW.name)
