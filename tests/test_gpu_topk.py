"""The fused similarity + top-k kernel on the GPU (csrc/topk.hip through ops.TopK / ops.rows_rnorm) against tests/topk_ref.py.

a. Integer-valued inputs in [-4, 4]: every product and sum is exact in fp32 (|dot| <= 16 d, L2 <= 64 d), so an fp32 chain equals the
   float64 reference bit for bit and scores AND indices must be equal -- ties (frequent among small integers) and duplicates included.
b. Chunk invariance on Gaussian rows: lists bit-identical for one chunk, chunks of 1 / 7 / 64 / 500 rows, a call after a partial state,
   forced slice counts, and a base of 2^33.
c. Cosine on Gaussian rows: near-ties (gaps down to 1e-5) make index equality a test of rounding, so every query must meet the four
   conditions of topk_ref.check_lists at the project's parity tolerance 1e-4 + 1e-4 |ref|; fp32 against float64 differs by ~2e-7 here.
d. Exclusion, an all-zero row under cosine, no-op calls.
e. rows_rnorm against float64 within 1e-6 relative: at most 4 sequential + 6 butterfly additions per lane at d = 256, each within 2^-24
   relative, halved by the square root, plus the root's and the division's own rounding -- under 6e-7 in the worst case."""
import numpy as np
import pytest
import torch

from fragnet_amd import ops
from tests import topk_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def aux_of(x, metric):
    """What the kernel is handed: nothing for dot, ops.rows_rnorm for cosine, the fp32 squared norms for l2."""
    if metric == 0:
        return None
    return ops.rows_rnorm(x) if metric == 1 else (x * x).sum(1)


def run(q, lib, k, metric, chunks=None, index_base=0, exclude=None, splits=0, q_aux=None, lib_aux=None):
    """Feeds lib [n, d] (a device tensor) in the row ranges `chunks` (default: one) and returns the lists as numpy."""
    tk = ops.TopK(q.shape[0], k, metric, DEV, splits=splits)
    q_aux = aux_of(q, metric) if q_aux is None else q_aux
    lib_aux = aux_of(lib, metric) if lib_aux is None else lib_aux
    for lo, hi in chunks or [(0, lib.shape[0])]:
        tk.update(q, lib[lo:hi], index_base + lo, q_aux, None if lib_aux is None else lib_aux[lo:hi], exclude)
    score, index = tk.result()
    torch.cuda.synchronize()
    return score.cpu().numpy(), index.cpu().numpy()


def cuts(n, step):
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def integer_rows(rng, n, d):
    return rng.integers(-4, 5, size=(n, d)).astype(np.float32)


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("n_q", [1, 16, 17, 37])
def test_exact_lists_on_integer_rows(d, n_q):
    rng = np.random.default_rng(1000 * d + n_q)
    q_all, lib_all = integer_rows(rng, n_q, d), integer_rows(rng, 1003, d)
    lib_all[3] = lib_all[11]
    lib_all[7] = lib_all[11]                    # two rows that duplicate a third: equal scores for every query
    q_all[0] = lib_all[11]
    qd = dev(q_all)
    tied = 0
    for n_lib in (1, 5, 16, 1000, 1003):
        lib = lib_all[:n_lib]
        libd = dev(lib)
        for metric in (0, 2):
            sc = R.scores(q_all, lib, metric)
            assert np.abs(sc).max() <= (16 * d if metric == 0 else 64 * d) < 2 ** 24        # exact in fp32
            for k in (1, 9, 32):
                want_s, want_i = R.topk(q_all, lib, k, metric)
                got_s, got_i = run(qd, libd, k, metric)
                assert np.array_equal(got_i, want_i), (n_lib, metric, k, np.argwhere(got_i != want_i)[:4])
                assert np.array_equal(got_s.astype(np.float64), want_s), (n_lib, metric, k)
                if k == 9 and n_lib == 1000:
                    tied += int((np.diff(want_s, axis=1) == 0).any(axis=1).sum())
    assert tied > 0, "no equal scores among the 9 best: the tie rule was not exercised"


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("d", [128, 256])
def test_lists_do_not_depend_on_chunks_or_launch_shape(metric, d):
    rng = np.random.default_rng(7 + d + metric)
    n, k = 1003, 9
    q, lib = dev(rng.standard_normal((37, d))), dev(rng.standard_normal((n, d)))
    lib[40] = lib[900]                          # equal scores across chunk boundaries
    lib[901] = lib[900]
    q_aux, lib_aux = aux_of(q, metric), aux_of(lib, metric)
    kw = dict(q_aux=q_aux, lib_aux=lib_aux)
    want_s, want_i = run(q, lib, k, metric, **kw)
    assert (want_i >= 0).all() and (want_i < n).all()
    for step in (1, 7, 64, 500):
        got_s, got_i = run(q, lib, k, metric, chunks=cuts(n, step), **kw)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.view(np.int32), want_s.view(np.int32)), step
    got_s, got_i = run(q, lib, k, metric, chunks=[(0, 300), (300, n)], **kw)           # one call after a partial state
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.view(np.int32), want_s.view(np.int32))
    for splits in (1, 3, 63):
        got_s, got_i = run(q, lib, k, metric, splits=splits, **kw)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.view(np.int32), want_s.view(np.int32)), splits
    base = 2 ** 33
    got_s, got_i = run(q, lib, k, metric, chunks=cuts(n, 500), index_base=base, **kw)
    assert np.array_equal(got_i - base, want_i) and np.array_equal(got_s.view(np.int32), want_s.view(np.int32))
    # and the lists are the right ones: the float64 reference's conditions (ties between duplicates are exact, so indices are checked too)
    R.check_lists(want_s, want_i, R.scores(q.cpu().numpy(), lib.cpu().numpy(), metric), metric)


@pytest.mark.parametrize("d", [128, 256])
def test_cosine_on_gaussian_rows(d):
    rng = np.random.default_rng(31 + d)
    qn, libn = rng.standard_normal((37, d)).astype(np.float32), rng.standard_normal((1003, d)).astype(np.float32)
    ref = R.scores(qn, libn, 1)
    got_s, got_i = run(dev(qn), dev(libn), 9, 1)
    worst = R.check_lists(got_s, got_i, ref, 1)
    print(f"cosine d={d}: max |fp32 - float64| over the lists = {worst:.3e}")
    assert worst < 1e-5
    exact_s, exact_i = R.topk(qn, libn, 9, 1)
    print(f"cosine d={d}: {int((got_i != exact_i).sum())} of {got_i.size} indices differ from the float64 order (near-ties)")


def test_exclusion_skips_the_own_row_and_keeps_a_duplicate():
    rng = np.random.default_rng(5)
    lib = integer_rows(rng, 200, 128)
    lib[50] = lib[2]                            # a twin of query 2
    q = lib[:17].copy()
    exclude = np.arange(17, dtype=np.int64)
    exclude[5] = -1                             # query 5 keeps its own row
    for metric in (0, 2):
        want_s, want_i = R.topk(q, lib, 9, metric, exclude=exclude)
        got_s, got_i = run(dev(q), dev(lib), 9, metric, exclude=dev(exclude, torch.int64), chunks=cuts(200, 64))
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)
    assert got_i[2, 0] == 50 and got_s[2, 0] == 0 and got_i[5, 0] == 5
    for i in range(17):
        assert (i in got_i[i].tolist()) == (i == 5)
    # the same with a base: exclusion compares GLOBAL ids
    base = 2 ** 33
    got_s, got_b = run(dev(q), dev(lib), 9, 2, exclude=dev(np.where(exclude < 0, -1, exclude + base), torch.int64), index_base=base)
    assert np.array_equal(got_b - base, want_i)


def test_zero_row_under_cosine_scores_zero():
    rng = np.random.default_rng(6)
    qn, libn = rng.standard_normal((5, 128)).astype(np.float32), rng.standard_normal((20, 128)).astype(np.float32)
    libn[7] = 0
    got_s, got_i = run(dev(qn), dev(libn), 20, 1)
    assert not np.isnan(got_s).any() and (np.sort(got_i, axis=1) == np.arange(20)).all()
    assert (got_s[got_i == 7] == 0).all()
    R.check_lists(got_s, got_i, R.scores(qn, libn, 1), 1)


def test_empty_calls_change_nothing():
    rng = np.random.default_rng(8)
    q, lib = dev(rng.standard_normal((3, 128))), dev(rng.standard_normal((10, 128)))
    tk = ops.TopK(3, 4, "dot", DEV)
    tk.update(q, lib[:0], 0)
    assert (tk.result()[1] == -1).all() and torch.isinf(tk.result()[0]).all()
    tk.update(q, lib, 0)
    before = [t.clone() for t in tk.result()]
    tk.update(q, lib[:0], 10)
    assert all(torch.equal(a, b) for a, b in zip(before, tk.result()))
    none = ops.TopK(0, 4, "l2", DEV)
    none.update(q[:0], lib, 0, q_aux=q[:0, 0], lib_aux=(lib * lib).sum(1))
    assert none.result()[0].shape == (0, 4) and none.result()[1].shape == (0, 4)
    fresh = ops.TopK(2, 3, "l2", DEV).result()
    assert (fresh[0] == float("inf")).all() and (fresh[1] == -1).all()


def test_refusals_on_the_device():
    q = torch.zeros(3, 64, device=DEV)
    with pytest.raises(ops._lib.FragnetHipError, match="64"):
        ops.TopK(3, 4, "dot", DEV).update(q, q, 0)
    q = torch.zeros(3, 128, device=DEV)
    with pytest.raises(ValueError, match="q_aux"):
        ops.TopK(3, 4, "cosine", DEV).update(q, q, 0)
    with pytest.raises(ops._lib.FragnetHipError):
        ops.TopK(3, 4, "dot", DEV).update(q.cpu(), q, 0)


@pytest.mark.parametrize("n", [1, 63, 1000])
@pytest.mark.parametrize("d", [128, 256, 77])
def test_rows_rnorm_against_float64(n, d):
    rng = np.random.default_rng(n + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.01, 100.0, size=(n, 1))).astype(np.float32)
    if n > 2:
        x[2] = 0
    got = ops.rows_rnorm(dev(x)).cpu().numpy().astype(np.float64)
    want = R.rnorm(x)
    rel = np.abs(got - want) / want
    print(f"rows_rnorm n={n} d={d}: max relative error {rel.max():.3e}")
    assert rel.max() <= 1e-6
    # the same row gives the same bits wherever it sits and however many rows there are
    again = ops.rows_rnorm(dev(x[::-1].copy())).cpu().numpy()[::-1]
    assert np.array_equal(again.astype(np.float64), got)
