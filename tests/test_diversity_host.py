"""Host side of the diverse-subset path (tests/kcenter_ref.py, fragnet_amd/diversity.py, ops.KCenter, csrc/kcenter.hip's argument
checks): the float64 reference against a brute-force restatement, ``check_selection`` on the reference's own output and on a spoiled
one, ``Diverse`` and its cluster split on hand-made labels, the binding, and every refusal.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from fragnet_amd import diversity as dv
from tests import kcenter_ref as R


def brute_force(x, k, metric, first):
    """Greedy k-centre restated without running state: at every step the full [centres, n] distance table is rebuilt and reduced."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    picked, radius = [], []
    for t in range(k + 1):
        table = np.stack([R.distances(x, x[c], metric) for c in picked]) if picked else np.full((1, n), np.inf)
        mind = table.min(0)
        left = [i for i in range(n) if i not in picked]
        if not left:
            radius.append(0.0)
            break
        far = max(mind[i] for i in left)
        row = first if t == 0 and first is not None else min(i for i in left if mind[i] == far)
        radius.append(mind[row] if t < k else far)
        if t < k:
            picked.append(row)
    table = np.stack([R.distances(x, x[c], metric) for c in picked])
    return np.array(picked), np.array(radius), table.min(0), table.argmin(0)          # argmin: the FIRST (earliest) centre on a tie


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n,d,k,first", [(1, 4, 1, 0), (2, 4, 2, 1), (9, 3, 9, None), (17, 2, 6, 16), (17, 2, 17, 0), (40, 5, 12, None)])
def test_reference_equals_a_brute_force_restatement(n, d, k, first, metric):
    x = np.random.default_rng(n + d).integers(-2, 3, (n, d)).astype(np.float64)       # a coarse grid: many exact ties
    if n >= 9:
        x[5] = x[7] = x[1]
    picked, radius, mind, label = R.kcenter(x, k, metric, first)
    b_picked, b_radius, b_mind, b_label = brute_force(x, k, metric, first)
    assert np.array_equal(picked, b_picked) and len(set(picked.tolist())) == k
    assert np.array_equal(radius, b_radius) and np.isposinf(radius[0]) and (np.diff(radius[1:]) <= 0).all()
    assert np.array_equal(mind, b_mind) and np.array_equal(label, b_label)


def test_ties_go_to_the_smaller_row_and_the_earlier_centre():
    x = np.array([[0.0], [1.0], [-1.0], [1.0], [0.5]])
    picked, radius, mind, label = R.kcenter(x, 4, 0, 0)
    assert picked.tolist() == [0, 1, 2, 4]               # rows 1, 2, 3 all at 1 of row 0: row 1; then row 2 (row 3 is at 0 of row 1)
    assert radius.tolist() == [np.inf, 1.0, 1.0, 0.25, 0.0] and mind.tolist() == [0, 0, 0, 0, 0]
    assert label.tolist() == [0, 1, 2, 1, 3]
    x = np.array([[0.0], [2.0], [1.0]])                  # row 2 is at 1 of both centres: the earlier one keeps it
    assert R.kcenter(x, 2, 0, 0)[3].tolist() == [0, 1, 0]
    assert R.kcenter(x, 2, 0, None)[0].tolist() == [0, 1]
    seeded = R.kcenter(x, 1, 0, None, seeds=np.array([[2.0]]))
    assert seeded[0].tolist() == [-1, 0] and np.isnan(seeded[1][0]) and seeded[1][1:].tolist() == [4.0, 1.0] and seeded[3].tolist() == [1, 0, 0]


@pytest.mark.parametrize("metric", [0, 1])
def test_check_selection_accepts_the_reference_and_rejects_a_swap(metric):
    rng = np.random.default_rng(3)
    x, seeds = rng.standard_normal((60, 8)), rng.standard_normal((3, 8))
    for kw in (dict(), dict(seeds=seeds), dict(init=rng.random(60) * 4)):
        first = 0 if not kw else None
        picked, radius, mind, label = R.kcenter(x, 10, metric, first, **kw)
        R.check_selection(x, picked, radius, label, 0.0, metric, **kw)
        swapped = picked.copy()
        swapped[[-2, -5]] = swapped[[-5, -2]]
        with pytest.raises(AssertionError):
            R.check_selection(x, swapped, radius, label, 0.0, metric, **kw)
        with pytest.raises(AssertionError, match="radius"):
            R.check_selection(x, picked, np.where(np.isfinite(radius), radius * 1.01, radius), label, 1e-4, metric, **kw)
        wrong = label.copy()
        wrong[np.flatnonzero(label != label[30])[0]] = label[30]
        with pytest.raises(AssertionError, match="labelled centre"):
            R.check_selection(x, picked, radius, wrong, 1e-4, metric, **kw)
        twice = picked.copy()
        twice[-1] = twice[-2]
        with pytest.raises(AssertionError, match="distinct"):
            R.check_selection(x, twice, radius, label, 1e-4, metric, **kw)


def _diverse(label, picks=None, level="mol"):
    label = np.asarray(label)
    k = int(label.max()) + 1 if picks is None else picks
    return dv.Diverse(level, "l2", np.arange(k), np.zeros(k + 1), np.zeros(label.shape[0]), label, np.arange(label.shape[0] + 1))


def test_split_deals_whole_clusters_by_the_filling_rule():
    # clusters: 0 -> {0, 3, 4, 9} (4), 1 -> {1, 2, 8} (3), 2 -> {5, 6} (2), 3 -> {7} (1); N = 10, cutoffs 6 and 8
    res = _diverse([0, 1, 1, 0, 0, 2, 2, 3, 1, 0])
    train, valid, test = res.split((0.6, 0.2, 0.2))
    assert train.tolist() == [0, 3, 4, 5, 6, 9]          # 4; the 3-cluster would pass 6 and goes on; the 2-cluster after it still fits: 6 <= 6
    assert valid.tolist() == [1, 2, 8]                   # dealt second: 4 + 0 + 3 = 7 <= 8
    assert test.tolist() == [7]                          # 6 + 1 > 6 and 6 + 3 + 1 > 8
    # cutoffs that are exact in binary: a cluster that lands exactly ON a cutoff still fits (the rule moves on only when it would PASS it)
    res = _diverse([0, 0, 1, 2, 0, 1, 0, 3])             # sizes 4, 2, 1, 1; N = 8, cutoffs 4.0 and 6.0
    train, valid, test = res.split((0.5, 0.25, 0.25))
    assert (train.tolist(), valid.tolist(), test.tolist()) == ([0, 1, 4, 6], [2, 5], [3, 7])
    # largest first, not label order: the big cluster has the largest label
    res = _diverse([0, 1, 2, 2, 2, 2])
    assert [p.tolist() for p in res.split((0.7, 0.15, 0.15))] == [[2, 3, 4, 5], [0], [1]]      # 4 <= 4.2; 4 + 0 + 1 <= 5.1; 4 + 1 + 1 > 5.1


def test_split_edge_cases_and_refusals():
    res = _diverse([0, 1, 1, 0, 0, 2, 2, 3, 1, 0])
    parts = res.split()
    assert sorted(np.concatenate(parts).tolist()) == list(range(10)) and all((np.diff(p) > 0).all() for p in parts)
    for p in parts:                                       # whole clusters only
        for c in range(4):
            members = np.flatnonzero(res.label == c)
            assert np.isin(members, p).all() or not np.isin(members, p).any()
    assert [p.tolist() for p in res.split((1.0, 0.0, 0.0))] == [list(range(10)), [], []]
    assert [p.tolist() for p in res.split((0.0, 0.0, 1.0))] == [[], [], list(range(10))]
    assert [p.tolist() for p in res.split((0.0, 1.0, 0.0))] == [[], list(range(10)), []]
    # equal sizes: the cluster with the smallest member first; seed clusters (-1 - s) and rows without a centre (-1) are groups too
    res = _diverse([-1, 0, -2, 0, -1, -2], picks=1)
    assert [p.tolist() for p in res.split((0.34, 0.33, 0.33))] == [[0, 4], [1, 3], [2, 5]]
    with pytest.raises(ValueError, match="add up to 1"):
        res.split((0.5, 0.1, 0.1))
    with pytest.raises(ValueError, match="add up to 1"):
        res.split((1.2, -0.2, 0.0))
    with pytest.raises(ValueError, match='level="mol"'):
        _diverse([0, 0, 1], level="frag").split()


def test_diverse_shapes_and_items():
    offsets = np.array([0, 2, 2, 5])                      # three molecules: 2, 0 and 3 fragment rows
    res = dv.Diverse("frag", "cosine", [4, 0], [np.inf, 0.5, 0.25], [0, 0.1, 0.25, 0.2, 0], [1, 1, 0, 0, 0], offsets)
    assert len(res) == 2 and res.mol.tolist() == [2, 0] and res.frag.tolist() == [2, 0]
    item = res[-1]
    assert (item["row"], item["mol"], item["frag"], item["radius"]) == (0, 0, 0, 0.5) and item["members"].tolist() == [0, 1]
    with pytest.raises(IndexError):
        res[2]
    arrays = res.arrays()
    assert set(arrays) == {"picked", "mol", "frag", "radius", "distance", "label", "offsets", "level", "metric"}
    assert arrays["radius"].dtype == np.float32 and arrays["label"].dtype == np.int64 and str(arrays["level"]) == "frag"
    with pytest.raises(ValueError, match="radius"):
        dv.Diverse("frag", "l2", [4, 0], [1.0, 0.5], np.zeros(5), np.zeros(5, dtype=int), offsets)
    with pytest.raises(ValueError, match="distance / label"):
        dv.Diverse("frag", "l2", [4, 0], [1.0, 0.5, 0.1], np.zeros(4), np.zeros(5, dtype=int), offsets)
    with pytest.raises(ValueError, match="beyond the picks"):
        dv.Diverse("frag", "l2", [4, 0], [1.0, 0.5, 0.1], np.zeros(5), [0, 1, 2, 0, 0], offsets)
    with pytest.raises(ValueError, match="a row outside"):
        dv.Diverse("frag", "l2", [5, 0], [1.0, 0.5, 0.1], np.zeros(5), np.zeros(5, dtype=int), offsets)
    with pytest.raises(ValueError, match="unknown level"):
        dv.Diverse("atom", "l2", [], [0.0], [], [], [0])


def test_header_binding():
    from fragnet_amd import _lib, ops
    assert _lib.ABI_VERSION == 12 and _lib.load().fn_abi_version() == 12
    for name in ("fn_kcenter_scratch_bytes", "fn_kcenter_seed_f32", "fn_kcenter_pick_f32"):
        assert name in _lib.SIGNATURES and name in _lib.HEADER.functions
    assert [name for name, _ in _lib.Kcenter._fields_] == ["x", "aux", "mind", "label", "picked", "radius", "count", "scratch", "scratch_bytes",
                                                           "n", "cap", "host_count", "host_picks", "d", "metric", "splits"]
    assert _lib.HEADER.functions["fn_kcenter_scratch_bytes"][0] is C.c_int64
    assert ops.KCENTER_METRICS == {"l2": 0, "cosine": 1} == R.METRICS


def _descriptor(_lib, **kw):
    fields = dict(x=None, aux=None, mind=None, label=None, picked=None, radius=None, count=None, scratch=None, scratch_bytes=0, n=1000,
                  cap=64, host_count=0, host_picks=0, d=256, metric=0, splits=0)
    fields.update(kw)
    k = _lib.Kcenter()
    for name, v in fields.items():
        setattr(k, name, v)
    return k


FAKE = dict(x=1 << 20, aux=1 << 21, mind=1 << 22, label=1 << 23, picked=1 << 24, radius=1 << 25, count=1 << 26, scratch=1 << 27)     # never dereferenced


def test_library_refuses_bad_descriptors_before_any_launch():
    from fragnet_amd import _lib
    lib = _lib.load()
    need = lib.fn_kcenter_scratch_bytes(C.byref(_descriptor(_lib)))
    assert need == 2 * (16 + 12 * 512) == lib.fn_kcenter_scratch_bytes(C.byref(_descriptor(_lib, splits=7, n=0, d=128)))      # two tables, whatever the shape
    ok = dict(FAKE, scratch_bytes=need)
    pick = lambda first=0, k=8, **kw: lib.fn_kcenter_pick_f32(C.byref(_descriptor(_lib, **dict(ok, **kw))), first, k, None)       # noqa: E731
    seed = lambda s=4, centres=1 << 28, c_aux=1 << 29, **kw: lib.fn_kcenter_seed_f32(C.byref(_descriptor(_lib, **dict(ok, **kw))), centres, c_aux, s, None)     # noqa: E731
    assert lib.fn_kcenter_pick_f32(None, 0, 1, None) == _lib.FN_EINVAL and lib.fn_kcenter_seed_f32(None, None, None, 1, None) == _lib.FN_EINVAL
    assert lib.fn_kcenter_scratch_bytes(None) == _lib.FN_EINVAL
    for bad in (dict(n=-1), dict(cap=-1), dict(splits=-1), dict(host_count=-1), dict(host_picks=-1), dict(metric=2), dict(metric=-1)):
        assert lib.fn_kcenter_scratch_bytes(C.byref(_descriptor(_lib, **bad))) == _lib.FN_EINVAL, bad
        assert pick(**bad) == _lib.FN_EINVAL and seed(**bad) == _lib.FN_EINVAL, bad
    for d in (0, 64, 127, 192, 512):
        assert pick(d=d) == _lib.FN_EUNSUPPORTED and seed(d=d) == _lib.FN_EUNSUPPORTED and b"128 or 256" in lib.fn_last_error()
        assert lib.fn_kcenter_scratch_bytes(C.byref(_descriptor(_lib, d=d))) == _lib.FN_EUNSUPPORTED
    # the picks: more than the rows left, more than cap holds, a first row that is none or comes too late
    assert pick(k=-1) == _lib.FN_EINVAL
    assert pick(k=11, n=10) == _lib.FN_EINVAL and b"not yet picked" in lib.fn_last_error()
    assert pick(k=8, n=10, host_count=3, host_picks=3) == _lib.FN_EINVAL
    assert pick(k=8, cap=7) == _lib.FN_EINVAL and b"cap" in lib.fn_last_error()
    assert pick(k=8, cap=12, host_count=5, host_picks=0) == _lib.FN_EINVAL
    assert pick(first=-2) == _lib.FN_EINVAL and pick(first=1000) == _lib.FN_EINVAL and b"first" in lib.fn_last_error()
    assert pick(first=0, host_count=1, host_picks=1) == _lib.FN_EINVAL and pick(first=0, host_count=1) == _lib.FN_EINVAL
    assert pick(first=0, n=0, k=0) == _lib.FN_EINVAL
    # buffers: null, misaligned, aux for the cosine metric, the scratch
    for name in ("x", "mind", "label", "picked", "radius", "count", "scratch"):
        assert pick(**{name: None}) == _lib.FN_EINVAL and b"null" in lib.fn_last_error(), name
    assert pick(metric=1, aux=None) == _lib.FN_EINVAL and b"null" in lib.fn_last_error()
    for name, off in (("x", 8), ("scratch", 8), ("picked", 4), ("count", 4), ("mind", 2), ("label", 2), ("radius", 2)):
        assert pick(**{name: FAKE[name] + off}) == _lib.FN_EINVAL and b"misaligned" in lib.fn_last_error(), name
    assert pick(metric=1, aux=FAKE["aux"] + 2) == _lib.FN_EINVAL
    assert pick(scratch_bytes=need - 1) == _lib.FN_EINVAL and b"scratch" in lib.fn_last_error()
    # the seeds
    assert seed(s=-1) == _lib.FN_EINVAL
    assert seed(s=65) == _lib.FN_EINVAL and seed(s=4, host_count=61) == _lib.FN_EINVAL and b"cap" in lib.fn_last_error()
    assert seed(centres=None) == _lib.FN_EINVAL and seed(centres=(1 << 28) + 4) == _lib.FN_EINVAL
    assert seed(metric=1, c_aux=None) == _lib.FN_EINVAL and seed(metric=1, aux=None) == _lib.FN_EINVAL
    for name in ("x", "mind", "label", "picked", "radius", "count", "scratch"):
        assert seed(**{name: None}) == _lib.FN_EINVAL, name
    # nothing to do: nothing is launched, nothing is looked at
    nothing = dict.fromkeys(FAKE)
    assert pick(first=-1, k=0, n=0, **nothing) == 0 and pick(first=3, k=0, **nothing) == 0 and seed(s=0, centres=None, c_aux=None, **nothing) == 0


def test_python_side_refusals():
    from fragnet_amd import _lib, ops, synth
    from fragnet_amd.dataset import FlatMolStore
    from fragnet_amd.model import FragNetFineTune
    with pytest.raises(ValueError, match="not a distance"):
        ops.KCenter(10, 256, "dot", "cuda:0", cap=4)
    with pytest.raises(ValueError, match="unknown metric"):
        ops.KCenter(10, 256, 2, "cuda:0", cap=4)
    with pytest.raises(_lib.FragnetHipError, match="built for"):
        ops.KCenter(10, 64, "l2", "cuda:0", cap=4)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        ops.KCenter(10, 256, "l2", "cpu", cap=4)
    with pytest.raises(ValueError, match="splits"):
        ops.KCenter(10, 256, "l2", "cuda:0", cap=4, splits=513)
    with pytest.raises(ValueError, match="non-negative"):
        ops.KCenter(-1, 256, "l2", "cuda:0", cap=4)
    torch.manual_seed(0)
    model = FragNetFineTune(num_layer=2, h1=8, h2=8, h3=8, h4=8, edge_features=17)
    mols = synth.synth_molecules(6, seed=2, profile="esol")
    store = FlatMolStore.from_records(mols)
    with pytest.raises(ValueError, match="not a distance"):
        dv.select(model, store, 2, metric="dot")
    with pytest.raises(ValueError, match="k = 7 exceeds the 6 molecules"):
        dv.select(model, store, 7)
    with pytest.raises(ValueError, match="k = 7 exceeds the 6 molecules"):
        dv.select(model, mols, 7)
    with pytest.raises(ValueError, match="exceeds the .* fragment rows"):
        dv.select(model, store, 10 ** 6, level="frag")
    with pytest.raises(ValueError, match="non-negative integer"):
        dv.select(model, store, -1)
    with pytest.raises(ValueError, match="leave `first` at its default"):
        dv.select(model, store, 2, first=3, seeds=mols[:2])
    with pytest.raises(ValueError, match="leave `first` at its default"):
        dv.select(model, store, 2, first=3, init_distance=np.zeros(6, dtype=np.float32))
    with pytest.raises(ValueError, match="not both"):
        dv.select(model, store, 2, seeds=mols[:2], init_distance=np.zeros(6, dtype=np.float32))
    with pytest.raises(ValueError, match="no row of the source"):
        dv.select(model, store, 2, first=6)
    with pytest.raises(ValueError, match="unknown level"):
        dv.select(model, store, 2, level="atom")
    with pytest.raises(ValueError, match="no molecules"):
        dv.select(model, [], 0)

    class Pair(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.drug_model = model

    with pytest.raises(ValueError, match="pair model"):
        dv.select(Pair(), store, 2)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):           # everything above was refused before the device was asked for
        dv.select(model, store, 2)
