"""tests/batch_io_ref.py (the numpy restatements the GPU edge tests of csrc/batch_io.hip compare with) against what the project
already trusts -- the bond-graph oracle, graphstep.pad_batch, the torch collate of a CPU FlatMolStore -- and the two argument
errors fn_plan_build / fn_bond_graph_count return before they launch anything.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import batch_io_ref as R
from tests import topologies as T


def test_csr_is_the_sequential_scatter_order():
    keys = np.asarray([3, 0, 3, 1, 0, 3, 5, 0])
    rowptr, perm = R.csr(keys, 7)
    want = [[i for i, k in enumerate(keys) if k == s] for s in range(7)]          # ascending item id inside every segment
    assert rowptr.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert perm.tolist() == [i for w in want for i in w]


def test_level_csr_positions_are_mutually_inverse():
    rng = np.random.default_rng(4)
    n, m, loops = 9, 40, 9
    dst, src = rng.integers(0, n, m), rng.integers(0, n, m)
    L = R.level_csr(dst, src, n, n_loops=loops)
    d_all, s_all = np.concatenate([dst, np.arange(loops)]), np.concatenate([src, np.arange(loops)])
    for pos in range(m + loops):
        e = L["eid_d"][pos]                                    # edge at destination-order position pos
        assert L["src_d"][pos] == s_all[e] and L["inv_d"][e] == pos
        assert L["rowptr_d"][d_all[e]] <= pos < L["rowptr_d"][d_all[e] + 1]
        q = L["spos_d"][pos]                                   # the same edge in the source order
        assert L["dpos_s"][q] == pos and L["dst_s"][q] == d_all[e]
        assert L["rowptr_s"][s_all[e]] <= q < L["rowptr_s"][s_all[e] + 1]
    assert (np.diff(L["eid_d"])[np.diff(d_all[L["eid_d"]]) == 0] > 0).all()      # ascending edge id inside a destination row


def _zoo(fragments):
    ring = lambda n: (n, [(i, (i + 1) % n) for i in range(n)])
    mols = [T.two_atoms()[:2], T.components([2, 2])[:2], T.star(5)[:2], ring(6), T.chain(12)[:2], (1, []), T.chain(3)[:2]]
    zoo = [(n, R.directed(bonds)) for n, bonds in mols]
    if fragments:
        zoo.append((3, [(0, 1), (1, 0), (1, 2)]))              # exactly three connection nodes
    return zoo


@pytest.mark.parametrize("fragments", [False, True])
def test_tile_bond_graph_equals_the_batched_oracle(fragments):
    from oracle.bond_graph_ref import bond_graph_batch
    zoo = _zoo(fragments)
    order = np.random.default_rng(2).integers(0, len(zoo), 40)
    order[0], order[17] = 5, 5                                 # a bond-less atom first and in the middle
    ei, batch, want = R.tile_bond_graph(zoo, order, fragments)
    assert batch.shape[0] == sum(zoo[k][0] for k in order) and ei.shape[1] == sum(len(zoo[k][1]) for k in order)
    assert np.array_equal(bond_graph_batch(ei, batch, 40, fragments=fragments), want)
    assert want.shape[1] > 0 and set(order.tolist()) == set(range(len(zoo)))


def test_stage_field_reproduces_pad_batch():
    from fragnet_amd import data, graphstep, synth
    from fragnet_amd.plan import SPACES
    big = data.collate_fn_pt(synth.synth_molecules(24, seed=5, profile="esol", pretrain_targets=True))
    b = data.collate_fn_pt(synth.synth_molecules(17, seed=6, profile="esol", pretrain_targets=True))
    shapes = graphstep.StaticShapes.from_batches([big, b], margin=0.1)
    ref = graphstep.pad_batch(b, shapes)
    counts = graphstep.batch_counts(b)
    kinds = {"rows": R.STAGE_ROWS, "ids": R.STAGE_IDS, "cols": R.STAGE_COLS}
    seen = set()
    for name, (space, layout, target) in graphstep.FIELDS.items():
        src, cap, n = b[name].numpy(), shapes.cap[space], counts[space]
        assert cap > n
        hi, mod = shapes.pad_rule(target) if target else (0, 1)
        width = int(np.prod(src.shape[1:])) if layout == "rows" else 1
        got = R.stage_field(kinds[layout], src, n, cap, width, hi, mod)
        assert np.array_equal(got.reshape(ref[name].shape), ref[name].numpy()), name
        seen.add(layout)
    assert seen == set(kinds)
    for space, key in graphstep.MASKS.items():
        assert np.array_equal(R.stage_field(R.STAGE_MASK, None, counts[space], shapes.cap[space]), ref[key].numpy()), key
    got = R.stage_field(R.STAGE_OFFSETS, b.offsets.numpy(), counts["mol"], shapes.cap["mol"], width=len(SPACES))
    assert got.dtype == np.int32 and np.array_equal(got, ref.offsets.numpy())
    assert R.stage_field(R.STAGE_COUNT, None, 17, 1).tolist() == [17] and not R.stage_field(R.STAGE_ZERO, None, 0, 5).any()
    assert R.stage_field(R.STAGE_BUMP, None, 3, 1, before=[40]).tolist() == [43]


@pytest.mark.parametrize("pt", [False, True])
def test_collate_field_reproduces_the_torch_collate_of_a_cpu_store(pt):
    from fragnet_amd import synth
    from fragnet_amd.dataset import FlatMolStore
    from fragnet_amd.plan import SPACES
    store = FlatMolStore.from_records(synth.synth_molecules(40, seed=12, profile="esol", pretrain_targets=pt))
    idx = np.asarray([7, 0, 33, 3, 3, 39, 11, 20, 38, 1])
    want = store.collate(torch.from_numpy(idx), pretrain=pt)
    B, S = len(idx), len(SPACES)
    starts, offsets = np.zeros((S, B), dtype=np.int64), np.zeros((S, B + 1), dtype=np.int64)
    for s, name in enumerate(SPACES):
        if name == "mol":
            starts[s], offsets[s] = idx, np.arange(B + 1)
        else:
            off = store.off[name].numpy()
            starts[s] = off[idx]
            offsets[s, 1:] = np.cumsum(off[idx + 1] - off[idx])
    assert np.array_equal(offsets, want.offsets.numpy())
    sp = SPACES.index
    rows = dict(store._FUSED_ROWS, **(store._FUSED_PT if pt else {}))
    for key, (f, space) in rows.items():
        got = R.collate_field(R.COLLATE_ROWS, store.t[f].numpy(), starts, offsets, sp(space))
        assert got.dtype == want[key].numpy().dtype and np.array_equal(got, want[key].numpy()), key
    for key, (f, space, into) in store._FUSED_IDS.items():
        src = store.t[f].numpy()
        got = R.collate_field(R.COLLATE_IDS, src, starts, offsets, sp(space), rebase_space=sp(into))
        assert np.array_equal(got, want[key].numpy()), key
        # the same index stored store-global (every value counted from the store's first row of the space it points into)
        per_mol = np.diff(store.off[space].numpy())
        glob = src + np.repeat(store.off[into].numpy()[:-1], per_mol)
        got = R.collate_field(R.COLLATE_IDS, glob, starts, offsets, sp(space), rebase_space=sp(into), src_global=1)
        assert np.array_equal(got, want[key].numpy()), key
    for key, space in (("batch", "atom"), ("frag_batch", "frag")):
        assert np.array_equal(R.collate_field(R.COLLATE_BATCH, None, starts, offsets, sp(space)), want[key].numpy()), key
    assert np.array_equal(R.collate_field(R.COLLATE_ROWS, store.y.numpy(), starts, offsets, sp("mol")), want["y"].numpy())


def test_launch_geometry_helpers():
    assert [R.scan_blocks(n) for n in (1, 2048, 2049, 131072, 131073, 133121)] == [1, 1, 2, 64, 65, 66]
    assert [R.lookback_trips(n) for n in (2048, 2049, 131072, 133120, 133121, 266245)] == [0, 1, 1, 1, 2, 3]
    assert [R.grid_trips(n) for n in (1, 524288, 524289)] == [1, 1, 2]


def test_items_without_segments_and_bonds_without_molecules_are_refused_before_any_launch():
    """fn_plan_build with items but total_segs == 0 and fn_bond_graph_count with E > 0 but B == 0 would launch the look-back scan
    with no blocks (the second also counts bonds past its one-entry molecule table): FN_EINVAL from the host checks, nothing is
    enqueued.  The buffers are host memory nobody dereferences."""
    from fragnet_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    tasks = (_lib.CsrTask * _lib.FN_MAX_TASKS)()
    tasks[0] = _lib.CsrTask(p, None, 5, 0, 0, 0, 0, _lib.ROLE_PLAIN, -1)
    ti, ts = C.c_int64(), C.c_int64()
    assert lib.fn_plan_layout(tasks, 1, C.byref(ti), C.byref(ts)) == 0 and (ti.value, ts.value) == (5, 0)
    assert lib.fn_plan_build(tasks, 1, p, p, p, p, p, p, 0, None) == _lib.FN_EINVAL
    assert b"no segments" in lib.fn_last_error()
    tasks[0].n_loops, tasks[0].n_real = 3, 0                   # loop items alone count as items too
    assert lib.fn_plan_layout(tasks, 1, C.byref(ti), C.byref(ts)) == 0 and (ti.value, ts.value) == (3, 0)
    assert lib.fn_plan_build(tasks, 1, p, p, p, p, p, p, 0, None) == _lib.FN_EINVAL
    for mode in (0, 1):
        assert lib.fn_bond_graph_count(p, p, 2, 2, 0, mode, p, p, None) == _lib.FN_EINVAL
        assert b"no molecules" in lib.fn_last_error()
