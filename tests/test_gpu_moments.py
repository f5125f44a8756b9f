"""The moments and projection kernels on the GPU (csrc/moments.hip through ops.Moments / ops.rows_project) against the float64
references of tests/moments_ref.py: exact on integer rows at every size where the code takes another path (MFMA k-step, staging step,
chunk, super-chunk), bit-identical for every launch shape, and inside Higham's bound on Gaussian rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from fragnet_amd import _lib, ops
from fragnet_amd.plan import _stream_ptr
from tests import moments_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK, GROUP = _lib.MOMENTS_CHUNK, _lib.MOMENTS_GROUP
SIZES = (1, 2, 15, 16, 17, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, CHUNK * GROUP + 1)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def raw_moments(x, shift, accumulate, splits, total, gram):
    """One fn_rows_moments_f32 call into the caller's float64 buffers."""
    m = _lib.Moments(x.data_ptr(), None if shift is None else shift.data_ptr(), total.data_ptr(), gram.data_ptr(), None, 0, x.shape[0], x.shape[1],
                     int(accumulate), splits)
    need = _lib.load().fn_moments_scratch_bytes(C.byref(m))
    assert need >= 0
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    m.scratch, m.scratch_bytes = scratch.data_ptr(), scratch.numel()
    _lib.call("fn_rows_moments_f32", C.byref(m), _stream_ptr(x.device))
    torch.cuda.synchronize()
    return total, gram


def fresh(d, fill=float("nan")):
    return (torch.full((d,), fill, dtype=torch.float64, device=DEV), torch.full((d, d), fill, dtype=torch.float64, device=DEV))


@pytest.fixture(scope="module")
def integer_rows():
    rng = np.random.default_rng(7)
    x = rng.integers(-4, 5, (SIZES[-1], 256)).astype(np.float32)
    shift = rng.integers(-4, 5, 256).astype(np.float32)
    return x, shift


@pytest.fixture(scope="module")
def gaussian_rows():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((CHUNK * GROUP + 1003, 256)) * 1.5 + 0.75).astype(np.float32)
    shift = x[:200].mean(0).astype(np.float32)
    return x, shift


@pytest.mark.parametrize("with_shift", [False, True])
@pytest.mark.parametrize("d", [128, 256])
def test_integer_rows_are_exact(d, with_shift, integer_rows):
    x_all, shift_all = integer_rows
    x_all = np.ascontiguousarray(x_all[:, :d])
    shift = shift_all[:d] if with_shift else None
    xd = torch.from_numpy(x_all).to(DEV)
    sd = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift)).to(DEV)
    z = R.z_of(x_all, shift)
    assert np.abs(z).max() <= 8
    for n in SIZES:
        ref_sum, ref_gram = z[:n].sum(0), z[:n].T @ z[:n]
        total, gram = raw_moments(xd[:n], sd, False, 0, *fresh(d))         # overwrites: the NaN fill must be gone
        total, gram = total.cpu().numpy(), gram.cpu().numpy()
        assert np.array_equal(total, ref_sum), n
        assert np.array_equal(gram, ref_gram), n
        assert np.array_equal(gram, gram.T), n
    # a store that arrives in two and in three unequal cuts: exact for integers, whatever the cut
    n = 2 * CHUNK + 3
    ref_sum, ref_gram = z[:n].sum(0), z[:n].T @ z[:n]
    for cuts in ((0, 700, n), (0, 1, CHUNK + 65, n)):
        mom = ops.Moments(d, DEV)
        for a, b in zip(cuts[:-1], cuts[1:]):
            mom.update(xd[a:b], sd)
        count, total, gram = mom.result()
        assert count == n and np.array_equal(total.cpu().numpy(), ref_sum) and np.array_equal(gram.cpu().numpy(), ref_gram), cuts
        assert torch.equal(gram, gram.T)
    # accumulate adds onto what is there; n = 0 leaves it alone, or zeroes it when not accumulating
    total, gram = raw_moments(xd[:17], sd, True, 0, torch.full((d,), 3.0, dtype=torch.float64, device=DEV),
                              torch.full((d, d), -2.0, dtype=torch.float64, device=DEV))
    assert np.array_equal(total.cpu().numpy(), 3.0 + z[:17].sum(0)) and np.array_equal(gram.cpu().numpy(), -2.0 + z[:17].T @ z[:17])
    total, gram = raw_moments(xd[:0], sd, True, 0, *fresh(d, 5.0))
    assert (total == 5.0).all() and (gram == 5.0).all()
    total, gram = raw_moments(xd[:0], sd, False, 0, *fresh(d, 5.0))
    assert (total == 0.0).all() and (gram == 0.0).all()
    with pytest.raises(ValueError, match="fixed by the first update"):
        ops.Moments(d, DEV).update(xd[:5], sd).update(xd[5:9], torch.ones(d, device=DEV))


@pytest.mark.parametrize("d", [128, 256])
def test_result_is_bit_identical_for_every_launch_shape(d, gaussian_rows):
    x, shift = gaussian_rows
    xd, sd = torch.from_numpy(np.ascontiguousarray(x[:, :d])).to(DEV), torch.from_numpy(np.ascontiguousarray(shift[:d])).to(DEV)
    for n in (1003, xd.shape[0]):                                          # one super-chunk, and two
        base = [t.clone() for t in raw_moments(xd[:n], sd, False, 0, *fresh(d))]
        assert torch.isfinite(base[1]).all() and torch.equal(base[1], base[1].T)
        for splits in (1, 2, 7, 63):
            total, gram = raw_moments(xd[:n], sd, False, splits, *fresh(d))
            assert torch.equal(total, base[0]) and torch.equal(gram, base[1]), (n, splits)


@pytest.mark.parametrize("n", [1003, 2 * CHUNK + 3])
@pytest.mark.parametrize("d", [128, 256])
def test_gaussian_rows_stay_inside_the_chain_bound(d, n, gaussian_rows):
    x, shift = gaussian_rows
    x, shift = np.ascontiguousarray(x[:n, :d]), np.ascontiguousarray(shift[:d])
    total, gram = raw_moments(torch.from_numpy(x).to(DEV), torch.from_numpy(shift).to(DEV), False, 0, *fresh(d))
    total, gram = total.cpu().numpy(), gram.cpu().numpy()
    ref_sum, ref_gram = R.moments(x, shift)
    b_sum, b_gram = R.moments_bound(x, shift, CHUNK)
    print(f"d {d} n {n}: max |gram - ref| / bound = {(np.abs(gram - ref_gram) / b_gram).max():.3f}, sum {(np.abs(total - ref_sum) / b_sum).max():.3f}")
    assert (np.abs(gram - ref_gram) <= b_gram).all() and (np.abs(total - ref_sum) <= b_sum).all()
    assert np.array_equal(gram, gram.T)
    # the bound has teeth: a reference that lacks one row is outside it on the diagonal
    z = R.z_of(x, shift)
    lacking = ref_gram - np.outer(z[n // 2], z[n // 2])
    assert (np.abs(np.diag(gram) - np.diag(lacking)) > np.diag(b_gram)).any()


# ---------------------------------------------------------------------------------------- projection
KS = lambda d: (1, 2, 15, 16, 17, 128, d)          # noqa: E731
NS = (1, 63, 64, 65, 257, 1003)


@pytest.mark.parametrize("with_shift", [False, True])
@pytest.mark.parametrize("d", [128, 256])
def test_integer_projections_are_exact(d, with_shift):
    rng = np.random.default_rng(d + with_shift)
    x = rng.integers(-2, 3, (NS[-1], d)).astype(np.float32)
    shift = rng.integers(-2, 3, d).astype(np.float32) if with_shift else None
    W_all = rng.integers(-2, 3, (d, d)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    sd = None if shift is None else torch.from_numpy(shift).to(DEV)
    for k in KS(d):
        W = np.ascontiguousarray(W_all[:, :k])
        ref, _ = R.project(x, W, shift)
        ref_sq = (ref * ref).sum(1)
        assert np.abs(ref).max() < 2 ** 24 and ref_sq.max() < 2 ** 24          # every partial sum is an integer fp32 holds
        Wd = torch.from_numpy(W).to(DEV)
        for n in NS:
            out, sq = ops.rows_project(xd[:n], Wd, sd, want_rows=True, want_sq=True)
            assert out.shape == (n, k) and sq.shape == (n,)
            assert np.array_equal(out.cpu().numpy(), ref[:n]), (k, n)
            assert np.array_equal(sq.cpu().numpy(), ref_sq[:n]), (k, n)
            none, only = ops.rows_project(xd[:n], Wd, sd, want_rows=False, want_sq=True)
            assert none is None and torch.equal(only, sq)
            rows, none = ops.rows_project(xd[:n], Wd, sd)
            assert none is None and torch.equal(rows, out)


@pytest.mark.parametrize("d", [128, 256])
def test_gaussian_projections_bound_and_slice_invariance(d, gaussian_rows):
    x, shift = gaussian_rows
    x, shift = np.ascontiguousarray(x[:1003, :d]), np.ascontiguousarray(shift[:d])
    rng = np.random.default_rng(d)
    W_all = rng.standard_normal((d, d)).astype(np.float32)
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(shift).to(DEV)
    for k in KS(d):
        W = np.ascontiguousarray(W_all[:, :k])
        Wd = torch.from_numpy(W).to(DEV)
        out, sq = ops.rows_project(xd, Wd, sd, want_rows=True, want_sq=True)
        ref, bound = R.project(x, W, shift)
        o = out.cpu().numpy()
        assert (np.abs(o - ref) <= bound).all(), k
        ref_sq, b_sq = R.sq_of(o)
        assert (np.abs(sq.cpu().numpy() - ref_sq) <= b_sq).all(), k
        assert torch.equal(ops.rows_project(xd, Wd, sd, want_rows=False, want_sq=True)[1], sq)
        for a, b in ((0, 1), (1, 64), (5, 70), (130, 387), (997, 1003)):
            part, part_sq = ops.rows_project(xd[a:b], Wd, sd, want_rows=True, want_sq=True)
            assert torch.equal(part, out[a:b]) and torch.equal(part_sq, sq[a:b]), (k, a, b)
    assert (np.abs(o - (ref - np.outer(R.z_of(x, shift)[:, 3], W_all[3]))) > bound).any()      # teeth: a reference that lacks one column of the chain
