"""Plain numpy restatement of the FN_STAGE_ROWS_I64 field of fn_stage_padded, written from include/fragnet_hip.h and not from the
kernel, next to tests/batch_io_ref.py (whose ``stage_field`` covers the older kinds).  Test infrastructure only:
tests/test_gpu_pair_stage.py compares the kernel with it bit for bit, tests/test_pair_graphstep_host.py pins it to
``graphstep.pad_pair_batch``."""
import numpy as np

STAGE_ROWS_I64 = 8


def stage_rows_i64(src, n_real, cap, width):
    """int64 [cap, width] <- [n_real, width], zero rows behind the real ones (``src`` may be None when there are none)."""
    assert 0 <= n_real <= cap and width >= 1
    out = np.zeros((cap, width), dtype=np.int64)
    if n_real:
        out[:n_real] = np.asarray(src, dtype=np.int64).reshape(-1, width)[:n_real]
    return out
