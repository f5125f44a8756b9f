"""csrc/batch_io.hip at the sizes where its kernels change regime, bit for bit against tests/batch_io_ref.py (numpy, written from
include/fragnet_hip.h): the look-back scan past one chunk and past one window of 64 predecessors, the plan kernels past one grid
of 2048 x 256 items, the bond-graph builder's three scans with more than one block, the staging launch on unaligned pointers,
straddling groups and capped block ranges, and the one-launch collate on molecules of several chunks.

Every case builds its expected value on the CPU and asserts the boundary it claims to sit on BEFORE anything is launched; ids are
always inside their tables (the kernels do not guard them)."""
import numpy as np
import pytest
import torch

from tests import batch_io_ref as R
from tests import topologies as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ===================================================================================================== a. scan and plan
# n_seg -> (blocks of the scan over the segment counts, look-back trips of its last block)
SCAN_CASES = {2047: (1, 0), 2048: (1, 0), 2049: (2, 1), 4097: (3, 1),           # chunk edges
              131071: (64, 1), 131072: (64, 1), 131073: (65, 1),                # 65 blocks: the window is full, block 0 its last lane
              133121: (66, 2),                                                  # block 65 starts a second window
              266245: (131, 3)}
MAX_SEG_LEN = 64                                                                # the rank sort costs sum(len^2)


def _keys(pattern, n_seg, rng):
    if pattern == "uniform":
        return rng.integers(0, n_seg, 2 * n_seg)
    if pattern == "carry":                 # one item in segment 0, forty in the last: the prefix 1 travels over every block between
        return np.concatenate([np.full(20, n_seg - 1), [0], np.full(20, n_seg - 1)]).astype(np.int64)
    if pattern == "front":                 # everything in the first chunk: every later block adds nothing to the same prefix
        return rng.integers(0, min(n_seg, R.SCAN_CHUNK), 6000)
    raise ValueError(pattern)


def _check_segments_only(keys, n_seg):
    from fragnet_amd.plan import GraphPlan
    counts = np.bincount(keys, minlength=n_seg)
    assert keys.min() >= 0 and keys.max() < n_seg and counts.max() <= MAX_SEG_LEN
    want_ptr, want_perm = R.csr(keys, n_seg)
    plan = GraphPlan.segments_only(torch.from_numpy(keys).to(DEV), n_seg)
    torch.cuda.synchronize()
    plan.check()
    assert not plan.mol_built
    seg = plan.segs["s"]
    assert np.array_equal(seg.rowptr.cpu().numpy().astype(np.int64) - seg.pos_base, want_ptr)
    assert np.array_equal(seg.perm.cpu().numpy(), want_perm)


@pytest.mark.parametrize("pattern", ["uniform", "carry", "front"])
@pytest.mark.parametrize("n_seg", sorted(SCAN_CASES))
def test_segment_plan_across_scan_chunks_and_lookback_windows(n_seg, pattern):
    keys = _keys(pattern, n_seg, np.random.default_rng(n_seg))
    blocks, trips = SCAN_CASES[n_seg]
    assert (R.scan_blocks(n_seg), R.lookback_trips(n_seg)) == (blocks, trips)
    counts = np.bincount(keys, minlength=n_seg)
    if pattern == "carry" and blocks >= 3:                     # every block between the first and the last has total 0
        assert not counts[R.SCAN_CHUNK: (blocks - 1) * R.SCAN_CHUNK].any() and counts[0] == 1 and counts[-1] == 40
    if pattern == "front":
        assert not counts[R.SCAN_CHUNK:].any()
    _check_segments_only(keys, n_seg)


# ===================================================================================================== b. grid stride
def test_segment_plan_past_one_grid_of_items():
    """524288 + 257 items: the plan kernels make a second trip, whose last wave holds one item."""
    n_seg, items = 200000, R.GRID_ITEMS + 257
    assert R.grid_trips(items) == 2 and (items - R.GRID_ITEMS) % 64 == 1 and R.scan_blocks(n_seg) == 98
    _check_segments_only(np.random.default_rng(7).integers(0, n_seg, items), n_seg)


def test_multi_task_plan_past_the_window_and_the_grid():
    """The general builder on a paired level with self loops plus a plain CSR: the scan runs across three tasks' segments (103
    blocks), the item kernels make two trips, and the second trip lies in the SRC task and the plain one."""
    from fragnet_amd.plan import GraphPlan
    rng = np.random.default_rng(11)
    n, m, k = 70000, 300000, 100001
    dst, src, key = rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(0, n, k)
    loops = np.arange(n)
    dst_all, src_all = np.concatenate([dst, loops]), np.concatenate([src, loops])
    for v in (dst_all, src_all, key):
        assert np.bincount(v, minlength=n).max() <= MAX_SEG_LEN
    total_items, total_segs = 2 * (m + n) + k, 3 * n
    assert R.grid_trips(total_items) == 2 and total_items % 64 != 0
    assert (R.scan_blocks(total_segs), R.lookback_trips(total_segs)) == (103, 2)
    want_ptr, want_perm = R.csr(key, n)
    t = lambda a: torch.from_numpy(a).to(DEV)
    plan = GraphPlan([dict(kind="gat", name="g", dst=t(dst), src=t(src), n=n, n_loops=n),
                      dict(kind="seg", name="s", key=t(key), n_seg=n)], DEV)
    torch.cuda.synchronize()
    plan.check()
    assert not plan.mol_built and [x[2:] for x in plan.task_meta] == [(0, 0, m + n, n), (m + n, n, m + n, n), (2 * (m + n), 2 * n, k, n)]
    R.check_level_arena(plan, plan.levels["g"], dst_all, src_all, n)
    seg = plan.segs["s"]
    assert np.array_equal(seg.rowptr.cpu().numpy().astype(np.int64) - seg.pos_base, want_ptr)
    assert np.array_equal(seg.perm.cpu().numpy(), want_perm)


# ===================================================================================================== c. bond graph
def _ring(n):
    return n, [(i, (i + 1) % n) for i in range(n)]


TWO, LONE, COMP22, CHAIN3, RING3 = 0, 1, 2, 3, 4          # positions in the zoo


def _zoo(fragments):
    """(n_nodes, directed ends) of hand-made molecules.  Bond mode: atoms and directed bonds; fragment mode: the same lists read
    as fragments and connection nodes (two_atoms: exactly two connection nodes -- the special rule) plus one with exactly three."""
    mols = [T.two_atoms()[:2], (1, []), T.components([2, 2])[:2], T.chain(3)[:2], _ring(3), T.star(5)[:2], _ring(6), T.chain(12)[:2],
            T.star(12)[:2], T.star(16)[:2], T.chain(40)[:2]]
    zoo = [(n, R.directed(bonds)) for n, bonds in mols]
    if fragments:
        zoo.append((3, [(0, 1), (1, 0), (1, 2)]))
    assert [len(z[1]) for z in zoo[:5]] == [2, 0, 4, 4, 6]
    return zoo


def _one_bond_frags(zoo):
    from oracle.bond_graph_ref import one_bond_fragments
    return np.asarray([len(one_bond_fragments(n, ends)) for n, ends in zoo])


def _bond_graph_case(zoo, order, fragments):
    """(edge_index, batch, expected pairs) of a tiling, with the input contract asserted: molecule-contiguous, ids in their tables."""
    ei, batch, want = R.tile_bond_graph(zoo, order, fragments)
    B = len(order)
    assert ei.shape[1] > 0 and (ei >= 0).all() and (ei < batch.shape[0]).all() and (np.diff(batch) >= 0).all() and batch[-1] == B - 1
    assert (batch[ei[0]] == batch[ei[1]]).all() and (np.diff(batch[ei[0]]) >= 0).all()
    return ei, batch, want


def _check_bond_graph(zoo, order, fragments, e_want=None):
    from fragnet_amd import ops
    ei, batch, want = _bond_graph_case(zoo, order, fragments)
    if e_want is not None:
        assert ei.shape[1] == e_want
    got = ops.bond_graph(torch.from_numpy(ei).to(DEV), torch.from_numpy(batch).to(DEV), len(order), fragments=fragments)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("fragments", [False, True])
@pytest.mark.parametrize("B", [2047, 2048, 2049, 4100])
def test_bond_graph_across_the_molecule_scans(B, fragments):
    """two_atoms and bond-less atoms only (about B directed bonds): the two per-molecule scans get a second and a third block."""
    zoo = _zoo(fragments)
    order = np.where(np.random.default_rng(B).random(B) < 0.5, TWO, LONE)
    order[0], order[B // 2], order[-1] = LONE, LONE, TWO           # a bond-less atom first and in the middle
    assert R.scan_blocks(B) == {2047: 1, 2048: 1, 2049: 2, 4100: 3}[B]
    _check_bond_graph(zoo, order, fragments)


@pytest.mark.parametrize("fragments", [False, True])
@pytest.mark.parametrize("B", [2047, 2048, 2049, 4100, 6244])
def test_bond_graph_one_bond_fragments_at_both_ends_only(B, fragments):
    """One-bond fragments only among the first 100 and the last 100 molecules: the prefix of the flagged-bond scan (mol_ob) is
    the same for every molecule in between.  B = 6244 puts the last 100 into a block of their own, with two blocks of total 0
    before it."""
    zoo = _zoo(fragments)
    rng = np.random.default_rng(B + 1)
    order = rng.choice([LONE, CHAIN3, RING3], B)
    ends = np.r_[0:100, B - 100:B]
    order[ends] = rng.choice([TWO, COMP22, CHAIN3], 200)
    order[[0, 99, B - 100, B - 1]] = [LONE, COMP22, TWO, COMP22]
    ob = _one_bond_frags(zoo)[order]
    assert ob[:100].sum() > 0 and ob[-100:].sum() > 0 and not ob[100:B - 100].any()
    if B == 6244:
        assert R.scan_blocks(B) == 4 and not ob[R.SCAN_CHUNK: 3 * R.SCAN_CHUNK].any() and ob[3 * R.SCAN_CHUNK:].sum() > 0
    _check_bond_graph(zoo, order, fragments)


def _mixed_order(zoo, target, rng):
    """A random tiling of the whole zoo with exactly ``target`` directed bonds (the last molecules are two_atoms, and in fragment
    mode one three-connection molecule where the parity needs it)."""
    nb = np.asarray([len(z[1]) for z in zoo])
    draw = rng.integers(0, len(zoo), target)                   # more than enough: every draw has >= 0 bonds, the mean is > 1
    order = list(draw[: int(np.searchsorted(np.cumsum(nb[draw]), target, side="right"))])
    while True:
        d = target - int(nb[order].sum())
        if d % 2 == 0:
            return np.asarray(order + [TWO] * (d // 2))
        if d >= 3 and nb[-1] == 3:
            return np.asarray(order + [len(zoo) - 1] + [TWO] * ((d - 3) // 2))
        order.pop()


@pytest.mark.parametrize("fragments", [False, True])
@pytest.mark.parametrize("case", ["second_window", "window_minus_one_molecule", "window_exact", "window_plus_one_molecule"])
def test_bond_graph_across_the_bond_scan_window(case, fragments):
    """The mixed zoo, about 7500 molecules.  The scan over the per-bond pair counts has E entries: 131072 = 64 blocks exactly,
    one molecule more makes block 64 look back over a full window, E >= 133121 starts a second window."""
    zoo = _zoo(fragments)
    target = 133122 if case == "second_window" else 131072
    order = _mixed_order(zoo, target, np.random.default_rng(17 + fragments))
    if case == "window_minus_one_molecule":
        order = order[:-1]
    elif case == "window_plus_one_molecule":
        order = np.concatenate([order, [TWO]])
    E = int(sum(len(zoo[k][1]) for k in order))
    assert set(order.tolist()) == set(range(len(zoo))) and 6000 <= len(order) <= 9000 and R.scan_blocks(len(order)) >= 3
    assert {"second_window": E == 133122, "window_minus_one_molecule": 131072 - 78 <= E < 131072, "window_exact": E == 131072,
            "window_plus_one_molecule": E == 131074}[case]
    want = {"second_window": (66, 2), "window_minus_one_molecule": (64, 1), "window_exact": (64, 1), "window_plus_one_molecule": (65, 1)}[case]
    assert (R.scan_blocks(E), R.lookback_trips(E)) == want
    _check_bond_graph(zoo, order, fragments, e_want=E)


# ===================================================================================================== d. staging
GUARD = 8                                                      # elements in front of and behind every destination


class _Dst:
    """A destination of ``n`` elements inside a buffer of guard words (``mis`` elements off the buffer's 32-byte-aligned start)."""

    def __init__(self, n, dtype, mis=0, before=None):
        self.fill = -7.5 if dtype == torch.float32 else -99
        self.buf = torch.full((GUARD + mis + n + GUARD,), self.fill, dtype=dtype, device=DEV)
        self.lo, self.n = GUARD + mis, n
        if before is not None:
            self.buf[self.lo: self.lo + n] = torch.as_tensor(before, dtype=dtype)
        self.ptr = self.buf.data_ptr() + self.lo * self.buf.element_size()

    def check(self, want, note):
        got = self.buf.cpu().numpy()
        want = np.asarray(want).reshape(-1)
        assert want.shape[0] == self.n and want.dtype == got.dtype, note
        assert (got[: self.lo] == self.fill).all() and (got[self.lo + self.n:] == self.fill).all(), f"{note}: guard words overwritten"
        assert np.array_equal(got[self.lo: self.lo + self.n], want), note


def _dev(a, mis=0):
    """``a`` on the device, ``mis`` elements off an aligned allocation: (tensor to keep alive, pointer)."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + mis + 4, dtype=torch.from_numpy(a).dtype, device=DEV)
    buf[mis: mis + a.size] = torch.from_numpy(a.reshape(-1))
    return buf, buf.data_ptr() + mis * buf.element_size()


def _run_stage(specs, repeat=1):
    """specs: [(kind, src array or None, n_real, cap, width, pad_hi, pad_mod, src_mis, dst_mis, before)]; one launch for all of them."""
    from fragnet_amd import _lib
    assert 1 <= len(specs) <= _lib.FN_MAX_STAGE_FIELDS
    sizes = {R.STAGE_ROWS: lambda c, w: c * w, R.STAGE_COLS: lambda c, w: 2 * c, R.STAGE_COUNT: lambda c, w: 1, R.STAGE_BUMP: lambda c, w: 1,
             R.STAGE_OFFSETS: lambda c, w: w * (c + 1)}
    types = {R.STAGE_ROWS: torch.float32, R.STAGE_MASK: torch.float32, R.STAGE_COUNT: torch.int32, R.STAGE_ZERO: torch.int32,
             R.STAGE_OFFSETS: torch.int32}
    fields = (_lib.StageField * _lib.FN_MAX_STAGE_FIELDS)()
    keep, checks = [], []
    for i, (kind, src, n_real, cap, width, hi, mod, src_mis, dst_mis, before) in enumerate(specs):
        want = R.stage_field(kind, src, n_real, cap, width, hi, mod, before=before)
        for _ in range(repeat - 1):
            want = R.stage_field(kind, src, n_real, cap, width, hi, mod, before=want)
        dst = _Dst(sizes.get(kind, lambda c, w: c)(cap, width), types.get(kind, torch.int64), dst_mis, before)
        sp = None
        if src is not None:
            sbuf, sp = _dev(src, src_mis)
            keep.append(sbuf)
        fields[i] = _lib.StageField(sp, dst.ptr, n_real, cap, width, kind, hi, mod)
        checks.append((dst, want, f"field {i}: kind {kind}, n_real {n_real}, cap {cap}, width {width}, src+{src_mis}, dst+{dst_mis}"))
    for _ in range(repeat):
        _lib.call("fn_stage_padded", fields, len(specs), _stream())
    torch.cuda.synchronize()
    for dst, want, note in checks:
        dst.check(want, note)


ROW_WIDTHS = (1, 3, 4, 5, 128, 167)


@pytest.mark.parametrize("align", ["aligned", "src_off_one_float", "dst_off_one_float"])
def test_stage_rows_straddle_tail_and_unaligned_pointers(align):
    """Row tables of every width x n_real in {0, 1, cap - 1, cap} at cap = 7 in ONE launch (25 block ranges), plus one of 124
    blocks; the empty ones have no source (NULL: nothing may read it).  Aligned: the 16-byte path with its straddling group (n_real * width % 4 = 1, 2, 3) and its tail (cap * width % 4
    != 0); one pointer a float off a 16-byte boundary: the element-wise branch."""
    rng = np.random.default_rng(3)
    cap = 7
    src_mis, dst_mis = int(align == "src_off_one_float"), int(align == "dst_off_one_float")
    specs, rem_real, rem_all = [], set(), set()
    for width in ROW_WIDTHS:
        for n_real in (0, 1, cap - 1, cap):
            rem_real.add(n_real * width % 4)
            rem_all.add(cap * width % 4)
            src = rng.standard_normal((n_real, width)).astype(np.float32) if n_real else None      # an empty field may come without a source
            specs.append((R.STAGE_ROWS, src, n_real, cap, width, 0, 1, src_mis, dst_mis, None))
    assert rem_real == {0, 1, 2, 3} and {0, 3} <= rem_all
    cap, width, n_real = 3000, 167, 2999
    assert (cap * ((width + 3) // 4) + 1023) // 1024 == 124 and n_real * width % 4 == 1
    specs.append((R.STAGE_ROWS, rng.standard_normal((n_real, width)).astype(np.float32), n_real, cap, width, 0, 1, src_mis, dst_mis, None))
    _run_stage(specs)


def test_stage_rows_field_past_the_block_cap():
    """cap x ceil(width / 4) > 1024 x 1024 work items: the field's 1024 blocks stride; aligned and unaligned, a small field behind
    each so that the block ranges after a capped one are exercised."""
    rng = np.random.default_rng(4)
    cap, width, n_real = 25001, 167, 24999
    assert cap * ((width + 3) // 4) > R.STAGE_BLOCK_CAP * 1024 and n_real * width % 4 == 1 and cap * width % 4 != 0
    src = rng.standard_normal((n_real, width)).astype(np.float32)
    small = rng.standard_normal((5, 3)).astype(np.float32)
    _run_stage([(R.STAGE_ROWS, src, n_real, cap, width, 0, 1, 0, 0, None), (R.STAGE_ROWS, small, 5, 6, 3, 0, 1, 0, 0, None),
                (R.STAGE_ROWS, src, n_real, cap, width, 0, 1, 0, 1, None), (R.STAGE_ROWS, small, 4, 6, 3, 0, 1, 1, 0, None)])


def test_stage_ids_cols_masks_counters_and_offsets():
    rng = np.random.default_rng(5)
    specs = []
    for mod in (1, 7):
        for n_real, cap in ((13, 50), (0, 50), (50, 50), (1, 2)):
            specs.append((R.STAGE_IDS, rng.integers(0, 1000, n_real) if n_real else None, n_real, cap, 1, 999, mod, 0, 0, None))
            specs.append((R.STAGE_COLS, rng.integers(0, 1000, (2, n_real)) if n_real else None, n_real, cap, 1, 999, mod, 0, 0, None))
    big_n, big_cap = 1_000_003, 1_100_000                      # more than 1024 x 1024 ids: the field strides
    assert big_cap > R.STAGE_BLOCK_CAP * 1024
    specs.append((R.STAGE_IDS, rng.integers(0, 1 << 40, big_n), big_n, big_cap, 1, (1 << 40) + 6, 7, 0, 0, None))
    specs.append((R.STAGE_MASK, None, 77, 300, 1, 0, 1, 0, 0, None))
    specs.append((R.STAGE_MASK, None, 0, 2500, 1, 0, 1, 0, 1, None))
    specs.append((R.STAGE_COUNT, None, 12345, 1, 1, 0, 1, 0, 0, None))
    specs.append((R.STAGE_ZERO, None, 0, 5000, 1, 0, 1, 0, 0, None))
    offs = np.cumsum(rng.integers(0, 40, (7, 24)), axis=1).astype(np.int32)
    offs[:, 0] = 0
    specs.append((R.STAGE_OFFSETS, offs, 23, 40, 7, 0, 1, 0, 0, None))
    specs.append((R.STAGE_OFFSETS, offs[:, :1], 0, 3, 7, 0, 1, 0, 0, None))
    _run_stage(specs)


def test_stage_bump_applied_twice_adds_twice():
    specs = [(R.STAGE_BUMP, None, 5, 1, 1, 0, 1, 0, 0, [1 << 40]), (R.STAGE_COUNT, None, 9, 1, 1, 0, 1, 0, 0, None),
             (R.STAGE_BUMP, None, 1 << 33, 1, 1, 0, 1, 0, 0, [-3])]
    assert R.stage_field(R.STAGE_BUMP, None, 5, 1, before=R.stage_field(R.STAGE_BUMP, None, 5, 1, before=[1 << 40])).tolist() == [(1 << 40) + 10]
    _run_stage(specs, repeat=2)


# ===================================================================================================== e. collate
# a hand-made store of nine molecules in three index spaces: rows (0), index items pointing into the rows (1), molecules (2)
STORE_LENS = np.asarray([[5, 0, 2500, 13, 1, 40, 12, 7, 2], [9, 0, 2500, 30, 2, 0, 25, 3, 1], [1] * 9])
COLLATE_IDX = np.asarray([1, 3, 2, 0, 6, 3, 7, 1, 5, 4, 8, 1])          # a repeat, the 0-row molecule first, in the middle and last


@pytest.fixture(scope="module")
def hand_store():
    rng = np.random.default_rng(6)
    off = np.concatenate([np.zeros((3, 1), dtype=np.int64), np.cumsum(STORE_LENS, axis=1)], axis=1)
    na, nb = int(off[0, -1]), int(off[1, -1])
    local = rng.integers(0, 1000, (2, nb))
    return dict(off=off, rows1=rng.standard_normal(na).astype(np.float32), rows167=rng.standard_normal((na, 167)).astype(np.float32),
                ids_local=local, ids_global=local + np.repeat(off[0, :-1], STORE_LENS[1]))


@pytest.mark.parametrize("tables_host", [False, True])
@pytest.mark.parametrize("bound", ["exact", "unknown", "half"])
def test_collate_store_chunked_molecules(hand_store, bound, tables_host):
    """One molecule of 2500 rows among small ones and molecules of 0 rows: ROWS (1 and 167 words), IDS (width 2, stored local and
    store-global, rebased into another space) and BATCH fields, with max_seg_rows exact (several chunks per molecule), 0 (one chunk
    walks everything) and half the truth (the last chunk takes the rest)."""
    from fragnet_amd import _lib
    st, idx = hand_store, COLLATE_IDX
    S, B = 3, len(idx)
    starts = st["off"][:, :-1][:, idx]
    offsets = np.concatenate([np.zeros((S, 1), dtype=np.int64), np.cumsum(STORE_LENS[:, idx], axis=1)], axis=1)
    biggest = int(STORE_LENS[:2].max())
    msr = {"exact": biggest, "unknown": 0, "half": biggest // 2}[bound]
    chunks = lambda unit: max(1, -(-unit // R.COLL_CHUNK))
    n_chunks = (chunks(msr * 167), chunks(2 * msr), chunks(msr))          # ROWS x 167, IDS, BATCH
    assert n_chunks == {"exact": (204, 3, 2), "unknown": (1, 1, 1), "half": (102, 2, 1)}[bound]
    assert biggest > 2048 and 0 in STORE_LENS[0, idx] and offsets[0, -1] == STORE_LENS[0, idx].sum()

    plan = [("rows1", R.COLLATE_ROWS, st["rows1"], 0, 1, 0, 0), ("rows167", R.COLLATE_ROWS, st["rows167"], 0, 167, 0, 0),
            ("ids_local", R.COLLATE_IDS, st["ids_local"], 1, 2, 0, 0), ("ids_global", R.COLLATE_IDS, st["ids_global"], 1, 2, 0, 1),
            ("batch", R.COLLATE_BATCH, None, 0, 1, 0, 0), ("batch_items", R.COLLATE_BATCH, None, 1, 1, 0, 0)]
    want = {name: R.collate_field(kind, src, starts, offsets, space, rebase, glob) for name, kind, src, space, _, rebase, glob in plan}
    assert np.array_equal(want["ids_local"], want["ids_global"]) and want["rows167"].shape == (offsets[0, -1], 167)

    # [starts int64 [S, B] | offsets int32 [S, B + 1]] in one allocation, as fn_collate_store wants it with tables_host
    n_st, n_off = S * B, S * (B + 1)
    tab_h = torch.empty(2 * n_st + n_off, dtype=torch.int32, pin_memory=tables_host)
    tab_h[: 2 * n_st].view(torch.long).view(S, B).copy_(torch.from_numpy(starts))
    tab_h[2 * n_st:].view(S, B + 1).copy_(torch.from_numpy(offsets.astype(np.int32)))
    tab_d = torch.zeros(2 * n_st + n_off, dtype=torch.int32, device=DEV)           # zero tables copy nothing if the upload were lost
    if not tables_host:
        tab_d.copy_(tab_h)
    fields = (_lib.CollateField * _lib.FN_MAX_COLLATE_FIELDS)()
    keep, dsts = [], {}
    for i, (name, kind, src, space, width, rebase, glob) in enumerate(plan):
        rows = int(offsets[space, -1])
        sp = None
        if src is not None:
            sbuf, sp = _dev(src)
            keep.append(sbuf)
        dsts[name] = _Dst(want[name].size, torch.from_numpy(want[name]).dtype)
        fields[i] = _lib.CollateField(sp, dsts[name].ptr, rows, src.shape[-1] if kind == R.COLLATE_IDS else 0, width, space, kind, rebase, glob, msr)
    _lib.call("fn_collate_store", fields, len(plan), tab_d.data_ptr(), tab_d.data_ptr() + 8 * n_st, S, B,
              tab_h.data_ptr() if tables_host else None, _stream())
    torch.cuda.synchronize()
    assert torch.equal(tab_d.cpu(), tab_h)
    for name in want:
        dsts[name].check(want[name], name)


def test_fused_collate_of_a_store_with_a_300_atom_chain():
    """A resident store holding chain(300) among ordinary molecules: its bond-graph index has more than 1024 rows, so the IDS
    fields are cut into chunks (and every row table into many).  Fused against the torch collate, every tensor and the offsets."""
    from fragnet_amd import dataset, synth
    from fragnet_amd.dataset import FlatMolStore
    recs = synth.synth_molecules(14, seed=21, profile="esol")
    recs.insert(5, synth.make_molecule(np.random.default_rng(22), topology=T.chain(300)))
    store = FlatMolStore.from_records(recs).to(DEV)
    bound = store.max_per_mol()
    assert bound["bedge"] > R.COLL_CHUNK // 2 and bound["atom"] == 300 and 2 * bound["bedge"] > 2 * R.COLL_CHUNK
    idx = torch.tensor([7, 5, 0, 14, 5, 3, 3, 11])
    got = store.collate(idx)
    assert getattr(got, "_keep", None) is not None                  # the fused path ran
    dataset.FUSED_COLLATE = False
    try:
        want = store.collate(idx)
    finally:
        dataset.FUSED_COLLATE = True
    assert getattr(want, "_keep", None) is None and set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert torch.equal(got.offsets, want.offsets) and got.max_per_mol == want.max_per_mol
