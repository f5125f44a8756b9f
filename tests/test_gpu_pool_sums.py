"""The order of additions of the pooling kernels and the destination-sorted edge term, bit for bit against the numpy restatement of
tests/pool_sum_ref.py (no kernel is the yardstick of another here).  Every kernel below runs block_rows_sum or row_dots_sorted_body of
csrc/shared_bodies.inc, or reproduces the former's order with another body (the tiled coalition read-out)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import pool_sum_ref as ref
from tests.test_gpu_fragment_shapley import FORMS, KEY          # the forms of FN_TUNE_COALITION_STAGED that test sweeps, and the key's number

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FULL64 = 2 ** 64 - 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _orders(seg):
    """The rows of every segment in the plan's pooling order."""
    rowptr, perm = seg.rowptr.cpu().numpy().astype(np.int64) - seg.pos_base, seg.perm.cpu().numpy()
    return [perm[rowptr[s]:rowptr[s + 1]] for s in range(seg.n_seg)]


@pytest.fixture(scope="module")
def batch():
    from fragnet_amd.plan import GraphPlan
    b = ref.batch_inputs()
    B = len(ref.ATOMS)
    plan = GraphPlan([dict(kind="seg", name="mol_atoms", key=_dev(b["batch"]), n_seg=B),
                      dict(kind="seg", name="mol_frags", key=_dev(b["frag_batch"]), n_seg=B)], torch.device(DEV))
    oa, of = _orders(plan.segs["mol_atoms"]), _orders(plan.segs["mol_frags"])
    assert [len(o) for o in oa] == list(ref.ATOMS) and [len(o) for o in of] == list(ref.FRAGS)
    assert any(not np.array_equal(o, np.arange(o[0], o[0] + len(o))) for o in oa if len(o)), "perm is not the identity"
    frags = np.stack([ref.pooled(b["xf"], o) for o in of])
    return dict(b, plan=plan, oa=oa, of=of, frags=frags, xa_d=_dev(b["xa"]), xf_d=_dev(b["xf"]))


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    bad = np.flatnonzero((got.view(np.int32) != np.asarray(want, dtype=np.float32).view(np.int32)).any(axis=-1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ from the restatement, first {bad[0]}"


def test_pool_cat_and_the_wide_segment_sum(batch):
    from fragnet_amd import ops
    b = batch
    atoms = np.stack([ref.pooled(b["xa"], o) for o in b["oa"]])
    long_ones = [o for o in b["oa"] if len(o) >= 17]
    assert any(not np.array_equal(ref.block_rows_sum(b["xa"][o]).view(np.int32), ref.sequential_sum(b["xa"][o]).view(np.int32))
               for o in long_ones), "the plain ascending sum gives the same bits on these inputs: the test could not tell the orders apart"
    out = ops.pool_cat(b["xa_d"], b["xf_d"], b["plan"])
    _same_bits(out[:, :128], atoms, "pool_cat, atoms' half")
    _same_bits(out[:, 128:], b["frags"], "pool_cat, fragments' half")
    assert bool((out[0] == 0.0).all()), "a molecule without atoms and fragments"
    seg = b["plan"].segs["mol_atoms"]
    x = b["xa_d"]
    assert seg.n_items >= 4 * seg.n_seg and x.shape[1] == 128 and x.data_ptr() % 16 == 0, "fn_segment_sum_f32 takes the wide kernel"
    got = ops.segment_sum(x, seg)
    assert got.data_ptr() % 16 == 0
    _same_bits(got, atoms, "segment_sum, wide")


def test_pool_cat_groups(batch):
    from fragnet_amd import ops
    b = batch
    rows = []                                    # (molecule, group left out)
    for m, n in enumerate(ref.ATOMS):
        rows += [(m, -1), (m, 100 * ((m + 1) % len(ref.ATOMS)) + 1)]                       # nothing; a group of another molecule
        rows += [(m, 100 * m + g) for g in ((0, 3) if n else ())]                          # groups of its own (3: none in the 1-atom one)
    want = np.stack([np.concatenate([ref.pooled(b["xa"], b["oa"][m], None if g < 0 else b["group"] != g), b["frags"][m]]) for m, g in rows])
    out = ops.pool_cat_groups(b["xa_d"], b["xf_d"], b["plan"], _dev(b["group"]), _dev(np.array([m for m, _ in rows], dtype=np.int32)),
                              _dev(np.array([g for _, g in rows], dtype=np.int64)))
    _same_bits(out, want, "pool_cat_groups")
    plain = ops.pool_cat(b["xa_d"], b["xf_d"], b["plan"])
    assert all(torch.equal(out[r], plain[m]) for r, (m, g) in enumerate(rows) if g < 0 or g // 100 != m)


def test_pool_cat_coalitions_in_every_form(batch):
    from fragnet_amd import _lib, ops
    b = batch
    masks = (0, FULL64, 1 << 3, 1 << 63)
    rows = [(m, k) for m in range(len(ref.ATOMS)) for k in masks]          # molecule-major: row_mol is non-decreasing
    keep = {k: np.array([x < 0 or (k >> int(x)) & 1 == 1 for x in b["bit"]]) for k in masks}
    want = np.stack([np.concatenate([ref.pooled(b["xa"], b["oa"][m], keep[k]), b["frags"][m]]) for m, k in rows])
    args = (b["xa_d"], b["xf_d"], b["plan"], _dev(b["bit"]), _dev(np.array([m for m, _ in rows], dtype=np.int32)),
            _dev(np.array([k for _, k in rows], dtype=np.uint64).view(np.int64)))
    try:
        for name, form in FORMS.items():
            _lib.call("fn_set_tuning", KEY, form)
            _same_bits(ops.pool_cat_coalitions(*args), want, f"pool_cat_coalitions, {name}")
    finally:
        _lib.call("fn_set_tuning", KEY, 1)
    only63 = want[rows.index((9, 1 << 63))]
    assert not np.array_equal(only63, want[rows.index((9, 0))]) and not np.array_equal(only63, want[rows.index((9, FULL64))])


def test_the_wide_kernel_grid_strides():
    """8 * kGridCap + 1 = 16 385 segments of four rows on 16 384 blocks: the last segment is the only one of a second trip."""
    from fragnet_amd import ops
    from fragnet_amd.plan import GraphPlan
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "fragnet_amd", "csrc", "fn_internal.h")) as f:
        cap = int(re.search(r"constexpr int kGridCap = (\d+);", f.read()).group(1))
    with open(os.path.join(ROOT, "fragnet_amd", "csrc", "fragnet_hip.hip")) as f:
        assert "n_seg < 8 * kGridCap ? n_seg : 8 * kGridCap" in f.read(), "the wide kernel's grid is no longer min(n_seg, 8 * kGridCap)"
    S = 8 * cap + 1
    rng = np.random.default_rng(21)
    key = rng.permutation(np.repeat(np.arange(S), 4)).astype(np.int64)
    x = ref.values(rng, (4 * S, 128))
    plan = GraphPlan([dict(kind="seg", name="s", key=_dev(key), n_seg=S)], torch.device(DEV))
    seg = plan.segs["s"]
    order = np.stack(_orders(seg))                                # [S, 4]
    assert seg.n_items >= 4 * seg.n_seg
    x_d = _dev(x)
    assert x_d.data_ptr() % 16 == 0
    _same_bits(ops.segment_sum(x_d, seg), ref.block_rows_sum(x[order].transpose(1, 0, 2)), f"segment_sum over {S} segments")


@pytest.mark.parametrize("J", [1, 2, 3, 4, 8])
def test_the_sorted_edge_term(J):
    """k_row_dots_sorted at every number of rows of A: loop positions are exactly 0.0, the words behind [J][m] keep their NaN, every
    other entry has the restatement's bits -- the fused multiply-adds of dot4 included (pool_sum_ref.fma32), so the edge term is pinned
    bitwise too."""
    from fragnet_amd import _lib
    from fragnet_amd.plan import GraphPlan, _stream_ptr
    n, m_real, lda, off = 5, 22, 160, 32
    rng = np.random.default_rng(30 + J)
    dst, src = rng.integers(0, n, m_real), rng.integers(0, n, m_real)
    plan = GraphPlan([dict(kind="gat", name="l", dst=_dev(dst.astype(np.int64)), src=_dev(src.astype(np.int64)), n=n, n_loops=n)], DEV)
    lv = plan.levels["l"]
    m = lv.m
    assert m == m_real + n and m % 8 and lv.m_real == m_real
    base = next(t[2] for t in plan.task_meta if t[0] == "l")                      # the destination CSR's slice of the arena
    eid = plan.perm[base:base + m].cpu().numpy()                          # GatPlan.eid_d
    assert int((eid >= m_real).sum()) == n and sorted(eid[eid < m_real].tolist()) == list(range(m_real))
    feat, A = ref.values(rng, (m_real, 128)), ref.values(rng, (J, lda))
    feat_d, A_d = _dev(feat), _dev(A)
    s = torch.full((J * m + 64,), float("nan"), device=DEV)
    _lib.call("fn_row_dots_sorted_f32", feat_d.data_ptr(), A_d.data_ptr(), lda, off, J, C.byref(lv.c), s.data_ptr(), _stream_ptr(feat_d.device))
    torch.cuda.synchronize()
    assert bool(torch.isnan(s[J * m:]).all()), "words behind the result were written"
    got = s[:J * m].reshape(J, m).cpu().numpy()
    want = np.zeros((J, m), dtype=np.float32)
    for pos in np.flatnonzero(eid < m_real):
        want[:, pos] = ref.row_dots(feat[eid[pos]], A[:, off:off + 128])
    assert np.all(got[:, eid >= m_real].view(np.int32) == 0), "loop positions are +0.0"
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, f"J={J}: {len(bad)} entries differ from the restatement, first (row, position) {tuple(bad[0])}"
