"""Plain numpy restatements of the integer / byte contracts of csrc/batch_io.hip, written from include/fragnet_hip.h (graph plan,
bond-graph topology, static-shape staging, one-launch collate) and not from the kernels.  Test infrastructure only: the GPU tests
in tests/test_gpu_batch_io_edges.py compare the kernels with these bit for bit, tests/test_batch_io_ref_host.py pins them to what
the project already trusts (oracle/bond_graph_ref.py, graphstep.pad_batch, the torch collate of a FlatMolStore).

The launch constants further down are copies of the kernels' (kScanChunk, kBlock, kGridCap, kCollChunk): the tests use them only to
SAY on which side of a boundary a case sits -- how many scan blocks, look-back windows and grid trips it has -- never to compute an
expected value.
"""
import numpy as np

from oracle import bond_graph_ref

# ---------------------------------------------------------------------------------------------- launch geometry (for the claims)
SCAN_CHUNK = 2048          # items per block of k_scan_lookback
SCAN_WINDOW = 64           # predecessors one look-back trip reads
GRID_ITEMS = 2048 * 256    # kGridCap x kBlock: items one trip of a grid-stride plan kernel covers
COLL_CHUNK = 2048          # 4-byte words per chunk of k_collate_store
STAGE_BLOCK_CAP = 1024     # blocks per field of k_stage_padded, 1024 work items each


def scan_blocks(n):
    return -(-int(n) // SCAN_CHUNK)


def lookback_trips(n):
    """Trips of the window loop the LAST block of a scan over n entries makes when no predecessor cuts it short."""
    return -(-(scan_blocks(n) - 1) // SCAN_WINDOW)


def grid_trips(n):
    return -(-int(n) // GRID_ITEMS)


# ---------------------------------------------------------------------------------------------- graph plan
def csr(keys, n_seg):
    """(rowptr [n_seg + 1], perm [items]) of a key vector: rowptr = cumulative per-segment counts, perm = stable argsort."""
    keys = np.asarray(keys, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=n_seg))]).astype(np.int64)
    return rowptr, np.argsort(keys, kind="stable")


def level_csr(dst, src, n, n_loops=0):
    """The paired DST / SRC tasks of one attention level over ``n`` nodes: ``n_loops`` identity items i -> i follow the real edges.
    Returns the arrays of fn_gat_plan, row pointers and positions task-local."""
    loops = np.arange(n_loops, dtype=np.int64)
    dst = np.concatenate([np.asarray(dst, dtype=np.int64), loops])
    src = np.concatenate([np.asarray(src, dtype=np.int64), loops])
    m = dst.shape[0]
    rowptr_d, order = csr(dst, n)
    rowptr_s, order_s = csr(src, n)
    inv = np.empty(m, dtype=np.int64)
    inv[order] = np.arange(m)
    dpos = inv[order_s]
    spos = np.empty(m, dtype=np.int64)
    spos[dpos] = np.arange(m)
    return dict(rowptr_d=rowptr_d, eid_d=order, src_d=src[order], inv_d=inv, spos_d=spos,
                rowptr_s=rowptr_s, dst_s=dst[order_s], dpos_s=dpos)


def check_level_arena(plan, lv, dst, src, n):
    """A built GraphPlan's level ``lv`` read through the raw arena against the stable argsorts of ``dst`` / ``src`` (numpy, loop
    items included): the seven per-level arrays and both row pointers.  Returns the destination order."""
    c = lv.c
    arena = plan._arena.cpu().numpy()
    base_ptr = plan._arena.data_ptr()
    off = lambda p: (p - base_ptr) // 4
    rp = arena[off(c.rowptr_d): off(c.rowptr_d) + n + 1].astype(np.int64) - c.pos_base_d
    eid = arena[off(c.eid_d): off(c.eid_d) + lv.m]
    srcd = arena[off(c.src_d): off(c.src_d) + lv.m]
    order = np.argsort(dst, kind="stable")
    assert np.array_equal(eid, order)
    assert np.array_equal(srcd, src[order])
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]))
    rps = arena[off(c.rowptr_s): off(c.rowptr_s) + n + 1].astype(np.int64) - c.pos_base_s
    dsts = arena[off(c.dst_s): off(c.dst_s) + lv.m]
    dpos = arena[off(c.dpos_s): off(c.dpos_s) + lv.m]
    order_s = np.argsort(src, kind="stable")
    assert np.array_equal(dsts, dst[order_s])
    inv = np.empty(lv.m, dtype=np.int64)
    inv[order] = np.arange(lv.m)
    assert np.array_equal(dpos, inv[order_s])
    inv_d = arena[off(c.inv_d): off(c.inv_d) + lv.m]
    assert np.array_equal(inv_d, inv)
    spos = arena[off(c.spos_d): off(c.spos_d) + lv.m]
    want_spos = np.empty(lv.m, dtype=np.int64)
    want_spos[dpos] = np.arange(lv.m)                      # inverse of dpos_s
    assert np.array_equal(spos, want_spos)
    assert np.array_equal(rps, np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]))
    return order


# ---------------------------------------------------------------------------------------------- bond-graph topology
def directed(bonds):
    """Undirected bonds [(a, b), ...] -> directed ends (a, b), (b, a), ... in the order a featuriser lists them."""
    out = []
    for a, b in bonds:
        out += [(int(a), int(b)), (int(b), int(a))]
    return out


def tile_bond_graph(zoo, order, fragments=False):
    """The batched bond graph (``fragments``: fragment-bond graph) of a batch made of copies of a few small molecules.
    ``zoo``: [(n_nodes, ends)] with ``ends`` the molecule's directed bonds (connection nodes) as local (u, v) pairs; ``order``:
    zoo index of every batch molecule.  The oracle runs once per distinct molecule; copies are shifted by the running bond count.
    Returns (edge_index [2, E], batch [N], edge_index_bonds_graph [2, Eb]), int64."""
    order = np.asarray(order, dtype=np.int64)
    pairs, ends_of = [], []
    for n_nodes, ends in zoo:
        ends = [(int(u), int(v)) for u, v in ends]
        assert all(0 <= u < n_nodes and 0 <= v < n_nodes for u, v in ends)
        pairs.append(bond_graph_ref.fbond_graph_one_molecule(ends) if fragments else bond_graph_ref.bond_graph_one_molecule(n_nodes, ends))
        ends_of.append(np.asarray(ends, dtype=np.int64).reshape(-1, 2).T)
    n_nodes = np.asarray([z[0] for z in zoo], dtype=np.int64)[order]
    n_ends = np.asarray([e.shape[1] for e in ends_of], dtype=np.int64)[order]
    a0 = np.cumsum(n_nodes) - n_nodes
    e0 = np.cumsum(n_ends) - n_ends
    ei = [ends_of[k] + a0[m] for m, k in enumerate(order)]
    want = [pairs[k] + e0[m] for m, k in enumerate(order)]
    cat = lambda parts: np.concatenate(parts, axis=1) if parts else np.zeros((2, 0), dtype=np.int64)
    return cat(ei), np.repeat(np.arange(order.shape[0], dtype=np.int64), n_nodes), cat(want)


# ---------------------------------------------------------------------------------------------- static-shape staging
STAGE_ROWS, STAGE_IDS, STAGE_COLS, STAGE_MASK, STAGE_COUNT, STAGE_BUMP, STAGE_ZERO, STAGE_OFFSETS = 0, 1, 2, 3, 4, 5, 6, 7


def stage_field(kind, src, n_real, cap, width=1, pad_hi=0, pad_mod=1, before=None):
    """What one FN_STAGE_* field leaves in its destination (``before``: the destination's previous content, read by BUMP only)."""
    if kind == STAGE_ROWS:
        out = np.zeros((cap, width), dtype=np.float32)
        if n_real:
            out[:n_real] = np.asarray(src, dtype=np.float32).reshape(-1, width)[:n_real]
        return out
    if kind in (STAGE_IDS, STAGE_COLS):
        i = np.arange(cap, dtype=np.int64)
        row = pad_hi - (i - n_real) % pad_mod              # padding position i points at slot pad_hi - (i - n_real) % pad_mod
        out = row if kind == STAGE_IDS else np.stack([row, row.copy()])
        if n_real:                                             # an empty field has no source
            out[..., :n_real] = np.asarray(src, dtype=np.int64).reshape(out.shape[:-1] + (-1,))[..., :n_real]
        return out
    if kind == STAGE_MASK:
        return (np.arange(cap) < n_real).astype(np.float32)
    if kind == STAGE_COUNT:
        return np.asarray([n_real], dtype=np.int32)
    if kind == STAGE_BUMP:
        return np.asarray(before, dtype=np.int64).reshape(1) + n_real
    if kind == STAGE_ZERO:
        return np.zeros(cap, dtype=np.int32)
    if kind == STAGE_OFFSETS:
        src = np.asarray(src, dtype=np.int32).reshape(width, n_real + 1)
        out = np.empty((width, cap + 1), dtype=np.int32)
        out[:, : n_real + 1] = src
        out[:, n_real + 1:] = src[:, n_real:]              # entries behind molecule n_real repeat the space's total
        return out
    raise ValueError(f"unknown staging kind {kind}")


# ---------------------------------------------------------------------------------------------- one-launch collate
COLLATE_ROWS, COLLATE_BATCH, COLLATE_IDS = 0, 1, 2


def collate_field(kind, src, starts, offsets, space, rebase_space=0, src_global=0):
    """One FN_COLLATE_* output tensor.  ``starts`` [n_spaces, B]: first STORE row of batch molecule b in every index space;
    ``offsets`` [n_spaces, B + 1]: its first BATCH row.  ROWS: src [store rows, ...] -> [rows, ...]; BATCH: int64 [rows]; IDS: src
    [width, store rows] -> [width, rows], values rebased into ``rebase_space``."""
    starts, offsets = np.asarray(starts, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    B = starts.shape[1]
    n = offsets[space, 1:] - offsets[space, :-1]
    assert offsets[space, 0] == 0 and (n >= 0).all()
    mol = np.repeat(np.arange(B, dtype=np.int64), n)                       # batch molecule of every batch row
    if kind == COLLATE_BATCH:
        return mol
    rows = starts[space][mol] + (np.arange(mol.shape[0], dtype=np.int64) - offsets[space][mol])      # store row of every batch row
    if kind == COLLATE_ROWS:
        return np.asarray(src)[rows]
    if kind == COLLATE_IDS:
        shift = offsets[rebase_space][:B] - (starts[rebase_space] if src_global else 0)
        return np.asarray(src, dtype=np.int64)[..., rows] + shift[mol]
    raise ValueError(f"unknown collate kind {kind}")
