"""Greedy k-centre on the GPU (ops.KCenter, csrc/kcenter.hip) against tests/kcenter_ref.py.

Exact cases: rows are integers in [-4, 4], so every difference (<= 8), square (<= 64) and partial sum (<= 64 * 256 < 2^24) is an
integer fp32 holds exactly, whatever the order of addition: ``picked``, ``radius``, ``mind`` and ``label`` must EQUAL the float64
reference, ties (frequent among small integers) included.  Gaussian rows: near-ties make the pick SEQUENCE a test of rounding, so
those are held to ``check_selection`` at the project's parity bar 1e-4 + 1e-4 |ref| -- and to bit equality across launch shapes."""
import numpy as np
import pytest
import torch

from fragnet_amd import ops
from tests import kcenter_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 2, 63, 64, 65, 257, 1003)          # wave / half-wave steps (8, 16 rows), tiles (32, 64 rows), several workgroups, grid stride


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def integer_rows(n, d, seed):
    x = np.random.default_rng(seed).integers(-4, 5, (n, d)).astype(np.float32)
    if n >= 3:
        x[n // 2] = x[n - 1] = x[0]             # two rows duplicating a third: mind 0 once one of them is a centre, still pickable
    return x


def gaussian_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    x[n // 3] = 0                               # an all-zero row: cosine distance 1 of everything
    return x


def run(x, k, metric="l2", first=None, splits=0, seeds=None, init=None, cuts=None):
    """(picked, radius, mind, label) as numpy, by ordinal; ``cuts``: the picks made in several calls of these sizes."""
    n, d = x.shape
    xd = torch.from_numpy(x).to(DEV)
    aux = ops.rows_rnorm(xd) if metric == "cosine" else None
    s = 0 if seeds is None else seeds.shape[0]
    kc = ops.KCenter(n, d, metric, DEV, cap=s + k, splits=splits, init_distance=None if init is None else torch.from_numpy(init).to(DEV))
    if s:
        sd = torch.from_numpy(seeds).to(DEV)
        kc.seed(xd, sd, ops.rows_rnorm(sd) if metric == "cosine" else None, aux)
    for i, part in enumerate(cuts or [k]):
        kc.pick(xd, part, first if i == 0 else None, aux)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in kc.result())


def assert_equal_to_reference(got, ref):
    for name, g, r in zip(("picked", "radius", "mind", "label"), got, ref):
        np.testing.assert_array_equal(g, r.astype(g.dtype), err_msg=name)          # (-0.0, a picked row's mind, equals 0.0)


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("n", NS)
def test_integer_rows_equal_the_float64_reference(n, d):
    x = integer_rows(n, d, 100 * n + d)
    for k in sorted({k for k in (1, 2, 33) if k <= n} | ({n} if n <= 65 else set())):
        for first in sorted({0, n - 1}) + [None]:
            assert_equal_to_reference(run(x, k, first=first), R.kcenter(x, k, 0, first))


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("d", [128, 256])
def test_results_are_bit_identical_for_every_launch_shape(d, metric):
    x = gaussian_rows(1003, d, 5 + d)
    base = run(x, 33, metric, first=7)
    for splits in (1, 3, ops.KCENTER_MAX_SPLITS):
        for b, g in zip(base, run(x, 33, metric, first=7, splits=splits)):
            assert np.array_equal(b.view(np.uint8), g.view(np.uint8)), splits
    for cuts in ([12, 21], [1, 31, 1]):
        for b, g in zip(base, run(x, 33, metric, first=7, cuts=cuts, splits=3)):
            assert np.array_equal(b.view(np.uint8), g.view(np.uint8)), cuts


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("d", [128, 256])
def test_gaussian_rows_are_a_valid_greedy_selection(d, metric):
    x = gaussian_rows(1003, d, 11 + d)
    picked, radius, mind, label = run(x, 33, metric, first=0)
    worst = R.check_selection(x.astype(np.float64), picked, radius, label, 1e-4, R.METRICS[metric])
    print(f"d {d} {metric}: max |radius - float64| = {worst:.3e}")
    assert np.isposinf(radius[0]) and (np.diff(radius[1:]) <= 0).all()
    ref = R.kcenter(x, 33, R.METRICS[metric], 0)
    assert (mind[picked] == 0).all() and np.signbit(mind[picked]).all()              # a picked row: distance zero, marked by the sign
    if np.array_equal(picked, ref[0]):                                               # the same sequence: then the same distances too
        rest = np.setdiff1d(np.arange(1003), picked)                                 # (the formula puts a picked all-zero row at 1 of itself)
        np.testing.assert_allclose(mind[rest], ref[2][rest], rtol=1e-4, atol=1e-4)
    if metric == "cosine":
        zero = 1003 // 3
        assert mind[zero] == 1.0 or zero in picked                                  # an all-zero row is at distance 1 of every centre


@pytest.mark.parametrize("d", [128, 256])
def test_seeds_and_initial_distances(d):
    n = 257
    x = integer_rows(n, d, 31 + d)
    seeds = np.random.default_rng(9).integers(-4, 5, (5, d)).astype(np.float32)
    seeds[3] = x[17]                                                                 # a seed that is a row: the row stays pickable, at mind 0
    assert_equal_to_reference(run(x, 20, seeds=seeds), R.kcenter(x, 20, 0, None, seeds=seeds))
    got = run(gaussian_rows(n, d, 2), 20, "cosine", seeds=seeds)
    R.check_selection(gaussian_rows(n, d, 2).astype(np.float64), got[0], got[1], got[3], 1e-4, 1, seeds=seeds)
    # initial distances: rows that start at or below every distance they will meet are never lowered and keep label -1
    init = np.full(n, 5000.0, dtype=np.float32)
    init[::3] = 0.0
    init[1] = -0.0                                                                   # (not the mark of a picked row: the binding adds +0)
    init[5], init[6] = np.nan, np.nan                                                # never lowered, never picked while a number is left
    got = run(x, 20, init=init)
    ref = R.kcenter(x, 20, 0, None, init=init)
    assert_equal_to_reference(got, ref)
    assert (got[3][::3] == -1).all() and got[3][1] == -1 and (got[3][[5, 6]] == -1).all() and not np.isin([5, 6], got[0]).any()
    assert (got[3] >= 0).sum() > 100
    all_nan = np.full(8, np.nan, dtype=np.float32)
    got = run(x[:8].copy(), 3, init=all_nan)
    assert got[0].tolist() == [0, 1, 2] and np.isnan(got[1]).all() and (got[3] == -1).all()


def test_nothing_to_do_launches_nothing():
    x = torch.from_numpy(integer_rows(65, 128, 1)).to(DEV)
    kc = ops.KCenter(65, 128, "l2", DEV, cap=4).pick(x, 2, first=3)
    torch.cuda.synchronize()
    before = [t.clone() for t in (kc.picked, kc.radius, kc.mind, kc.label, kc.count)]
    kc.pick(x, 0)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, (kc.picked, kc.radius, kc.mind, kc.label, kc.count)))
    assert kc.count.item() == kc.centres == 2 and kc.result()[0].tolist()[0] == 3
    empty = ops.KCenter(0, 256, "cosine", DEV, cap=0)
    empty.pick(torch.empty(0, 256, device=DEV), 0, aux=torch.empty(0, device=DEV))
    assert empty.count.item() == 0 and [t.numel() for t in empty.result()] == [0, 1, 0, 0]
