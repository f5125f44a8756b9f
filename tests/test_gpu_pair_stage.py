"""FN_STAGE_ROWS_I64 of fn_stage_padded (csrc/batch_io.hip) against tests/batch_io_rows_i64_ref.py, bit for bit: the widths of the pair
models' second inputs (903 gene values, 1000 protein tokens) and 1; no real row, some, all; a field past the blocks-per-field cap of
k_stage_padded; the new kind beside older ones in one launch; and what the entry point refuses.  Every destination is allocated with
guard words on both sides and pre-filled, so a write outside the field, or no write inside it, shows."""
import os
import re

import numpy as np
import pytest
import torch

from tests import batch_io_ref as R
from tests import batch_io_rows_i64_ref as R64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
FILL = {torch.int64: -(1 << 40) - 3, torch.int32: -77, torch.float32: 7.0}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


class _Dst:
    def __init__(self, numel, dtype):
        self.buf = torch.full((numel + 2 * GUARD,), FILL[dtype], dtype=dtype, device=DEV)
        self.numel, self.ptr = numel, self.buf.data_ptr() + GUARD * self.buf.element_size()

    def body(self):
        return self.buf[GUARD: GUARD + self.numel].cpu().numpy()

    def guards_intact(self):
        fill = FILL[self.buf.dtype]
        return bool((self.buf[:GUARD] == fill).all()) and bool((self.buf[GUARD + self.numel:] == fill).all())

    def untouched(self):
        return bool((self.buf == FILL[self.buf.dtype]).all())


def _field(kind, src, dst, n_real, cap, width=1, hi=0, mod=1):
    from fragnet_amd import _lib
    return _lib.StageField(None if src is None else src.data_ptr(), dst.ptr, n_real, cap, width, kind, hi, mod)


def _launch(fields):
    from fragnet_amd import _lib
    table = (_lib.StageField * _lib.FN_MAX_STAGE_FIELDS)()
    for i, f in enumerate(fields):
        table[i] = f
    rc = _lib.load().fn_stage_padded(table, len(fields), _stream())
    torch.cuda.synchronize()
    return rc


def _rows(rng, n, width):
    return rng.integers(-(1 << 62), 1 << 62, (n, width), dtype=np.int64)


@pytest.mark.parametrize("width", [1, 903, 1000])
def test_rows_i64_matches_the_numpy_reference(width):
    rng = np.random.default_rng(width)
    fields, checks, keep = [], [], []
    for n_real, cap in ((0, 8), (5, 8), (8, 8)):
        src_np = _rows(rng, n_real, width)
        src = torch.from_numpy(src_np).to(DEV) if n_real else None
        dst = _Dst(cap * width, torch.int64)
        keep.append(src)
        fields.append(_field(R64.STAGE_ROWS_I64, src, dst, n_real, cap, width))
        checks.append((dst, R64.stage_rows_i64(src_np, n_real, cap, width), (n_real, cap)))
    assert _launch(fields) == 0
    for dst, want, note in checks:
        assert np.array_equal(dst.body().reshape(want.shape), want), note
        assert dst.guards_intact(), note


def _stage_launch_constants():
    """(blocks-per-field cap, work items per block) as csrc/batch_io.hip and csrc/fn_internal.h state them."""
    from fragnet_amd import _lib
    csrc = os.path.join(_lib._HERE, "csrc")
    take = re.search(r"std::max<int64_t>\(\(work \+ (\d+) \* kBlock - 1\) / \(\1 \* kBlock\), 1\), (\d+)\)", open(os.path.join(csrc, "batch_io.hip")).read())
    block = re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(csrc, "fn_internal.h")).read())
    assert take and block, "the staging launch's block arithmetic moved: update this test"
    return int(take.group(2)), int(take.group(1)) * int(block.group(1))


def test_rows_i64_field_past_the_block_cap():
    block_cap, per_block = _stage_launch_constants()
    assert (block_cap, per_block) == (R.STAGE_BLOCK_CAP, 1024)
    n_real, cap, width = 1999, 2100, 1000
    assert (cap * width + 1) // 2 > block_cap * per_block              # a work item = 16 bytes = two int64: the blocks stride more than once
    rng = np.random.default_rng(5)
    src_np = _rows(rng, n_real, width)
    src, dst = torch.from_numpy(src_np).to(DEV), _Dst(cap * width, torch.int64)
    small_np = _rows(rng, 3, 7)
    small, small_dst = torch.from_numpy(small_np).to(DEV), _Dst(5 * 7, torch.int64)
    assert _launch([_field(R64.STAGE_ROWS_I64, src, dst, n_real, cap, width), _field(R64.STAGE_ROWS_I64, small, small_dst, 3, 5, 7)]) == 0
    assert np.array_equal(dst.body().reshape(cap, width), R64.stage_rows_i64(src_np, n_real, cap, width)) and dst.guards_intact()
    assert np.array_equal(small_dst.body().reshape(5, 7), R64.stage_rows_i64(small_np, 3, 5, 7)) and small_dst.guards_intact()


def test_rows_i64_beside_rows_ids_and_a_count_in_one_launch():
    rng = np.random.default_rng(9)
    rows_np = rng.standard_normal((5, 167)).astype(np.float32)
    ids_np = rng.integers(0, 1000, 6)
    tok_np = rng.integers(0, 26, (5, 1000), dtype=np.int64)
    rows, ids, tok = (torch.from_numpy(a).to(DEV) for a in (rows_np, ids_np, tok_np))
    d_rows, d_ids, d_tok, d_cnt = _Dst(8 * 167, torch.float32), _Dst(9, torch.int64), _Dst(8 * 1000, torch.int64), _Dst(1, torch.int32)
    fields = [_field(R.STAGE_ROWS, rows, d_rows, 5, 8, 167), _field(R64.STAGE_ROWS_I64, tok, d_tok, 5, 8, 1000),
              _field(R.STAGE_IDS, ids, d_ids, 6, 9, 1, 999, 4), _field(R.STAGE_COUNT, None, d_cnt, 5, 1)]
    assert _launch(fields) == 0
    assert np.array_equal(d_rows.body().reshape(8, 167), R.stage_field(R.STAGE_ROWS, rows_np, 5, 8, 167))
    assert np.array_equal(d_tok.body().reshape(8, 1000), R64.stage_rows_i64(tok_np, 5, 8, 1000))
    assert np.array_equal(d_ids.body(), R.stage_field(R.STAGE_IDS, ids_np, 6, 9, 1, 999, 4))
    assert np.array_equal(d_cnt.body(), R.stage_field(R.STAGE_COUNT, None, 5, 1))
    assert all(d.guards_intact() for d in (d_rows, d_ids, d_tok, d_cnt))


def test_rows_i64_refusals_write_nothing():
    from fragnet_amd import _lib
    src = torch.arange(8 * 4, dtype=torch.int64, device=DEV).reshape(8, 4)
    ok_dst = _Dst(8 * 4, torch.int64)                                   # a good field in front: a refusal launches nothing at all
    good = _field(R64.STAGE_ROWS_I64, src, ok_dst, 8, 8, 4)
    for what, bad in (("n_real > cap", dict(n_real=9, cap=8, width=4)), ("width 0", dict(n_real=4, cap=8, width=0)),
                      ("null src with real rows", dict(n_real=4, cap=8, width=4, src=None))):
        dst = _Dst(8 * 4, torch.int64)
        f = _field(R64.STAGE_ROWS_I64, bad.get("src", src), dst, bad["n_real"], bad["cap"], bad["width"])
        assert _launch([good, f]) == _lib.FN_EINVAL, what
        assert b"fn_stage_padded" in _lib.load().fn_last_error()
        assert dst.untouched() and ok_dst.untouched(), what
    # 8-byte alignment of both tables
    dst = _Dst(8 * 4, torch.int64)
    f = _field(R64.STAGE_ROWS_I64, src, dst, 8, 8, 4)
    f.dst = dst.ptr + 4
    assert _launch([f]) == _lib.FN_EINVAL and dst.untouched()
    f.dst, f.src = dst.ptr, src.data_ptr() + 4
    assert _launch([f]) == _lib.FN_EINVAL and dst.untouched()
    assert _launch([good]) == 0 and np.array_equal(ok_dst.body().reshape(8, 4), src.cpu().numpy())
