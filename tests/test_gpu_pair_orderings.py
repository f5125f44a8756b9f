"""The pair orderings of a factored batch built on the GPU in one launch (csrc/pair_factored.hip, fn_pair_orderings_i32;
ops.pair_orderings_both), against ``ops.pair_orderings`` -- the torch implementation (stable sort, bincount, cumsum) -- on the first
``n`` entries of each list.

Everything is an integer, so every comparison is for EQUALITY: the row pointers, ``perm[: rowptr[N]]`` (``pair_orderings`` lists the
out-of-range pairs behind the in-range ones; the kernel writes -1 there, which is asserted), and two runs of the kernel against each
other.  The lists hold, among in-range values, -1, ``N`` and ``2^32 + k`` with ``k`` in range (in range only after a narrowing to 32
bits, which the kernel must not do before it compares), and behind ``n`` garbage of both kinds.  The two sides of one call have
different N.  The output buffers start as 77 everywhere, so an entry the kernel left alone shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS = (0, 1, 255, 256, 257, 4096)
NS = (1, 17, 4096)
LISTS = ("one", "distinct", "random")
OTHER = {1: 17, 17: 4096, 4096: 1}        # the second side's N for a drug side of N: never the same


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _list(kind, M, N, n, gen):
    """int64 [M] on the host: the first n entries by ``kind`` with out-of-range values sprinkled in, garbage behind n."""
    if kind == "one":
        pl = torch.full((M,), N - 1, dtype=torch.int64)             # one long segment: its order is the test of stability
    elif kind == "distinct":
        pl = torch.randperm(M, generator=gen) % N if M > N else torch.randperm(N, generator=gen)[:M].clone()
    else:
        pl = torch.randint(0, max(1, min(N, 40)), (M,), generator=gen) * max(1, N // 40) % N
    pl = pl.to(torch.int64)
    if kind != "one" and M >= 8:                                    # out of range, in three ways
        where = torch.randperm(M, generator=gen)[: max(3, M // 16)]
        pl[where[0::3]] = -1
        pl[where[1::3]] = N
        pl[where[2::3]] = (1 << 32) + torch.randint(0, N, (len(where[2::3]),), generator=gen)
    if n < M:                                                       # behind n: garbage, in range and out of it
        tail = torch.randint(0, N, (M - n,), generator=gen)
        tail[0::3] = -(1 << 40)
        tail[1::3] = (1 << 32) + (N - 1)
        pl[n:] = tail
    return pl


def _run(pd, ps, U, C, count):
    from fragnet_amd import ops
    out = (torch.full((U + 1,), 77, dtype=torch.int32, device=DEV), torch.full((pd.numel(),), 77, dtype=torch.int32, device=DEV),
           torch.full((C + 1,), 77, dtype=torch.int32, device=DEV), torch.full((pd.numel(),), 77, dtype=torch.int32, device=DEV))
    got = ops.pair_orderings_both(pd, ps, U, C, real_pairs=count, out=out)
    torch.cuda.synchronize()
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    return [t.cpu() for t in got]


def _counts(M):
    return sorted({c for c in (0, 1, M - 1, M) if 0 <= c <= M}) + [None]


@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_orderings_equal_the_torch_reference_on_the_first_n(M, N, kind):
    from fragnet_amd import ops
    U, C = N, OTHER[N]
    gen = torch.Generator().manual_seed(1000 * M + 10 * N + LISTS.index(kind))
    for n in _counts(M):
        nn = M if n is None else n
        pd, ps = _list(kind, M, U, nn, gen), _list("random" if kind == "one" else kind, M, C, nn, gen)
        count = None if n is None else torch.tensor([n], dtype=torch.int32, device=DEV)
        got = _run(pd.to(DEV), ps.to(DEV), U, C, count)
        again = _run(pd.to(DEV), ps.to(DEV), U, C, count)
        for a, b in zip(got, again):
            assert torch.equal(a, b), "two runs must give identical bits"
        for (rowptr, perm), pl, rows in ((got[:2], pd, U), (got[2:], ps, C)):
            want_rp, want_pm = (t.cpu() for t in ops.pair_orderings(pl[:nn].to(DEV), rows))
            inside = int(((pl[:nn] >= 0) & (pl[:nn] < rows)).sum())
            assert int(want_rp[-1]) == inside
            assert rowptr.shape == (rows + 1,) and perm.shape == (M,)
            assert torch.equal(rowptr, want_rp), f"rowptr, M={M} N={rows} n={n} {kind}"
            assert torch.equal(perm[:inside], want_pm[:inside]), f"perm, M={M} N={rows} n={n} {kind}"
            assert bool((perm[inside:] == -1).all()), "behind rowptr[N] perm holds -1"
            if nn == 0:
                assert bool((rowptr == 0).all())


def test_a_count_beyond_the_list_is_clamped():
    gen = torch.Generator().manual_seed(3)
    pd, ps = _list("random", 257, 17, 257, gen).to(DEV), _list("random", 257, 4096, 257, gen).to(DEV)
    plain = _run(pd, ps, 17, 4096, None)
    for c in (258, 2 ** 31 - 1):
        for a, b in zip(plain, _run(pd, ps, 17, 4096, torch.tensor([c], dtype=torch.int32, device=DEV))):
            assert torch.equal(a, b)
    for a in _run(pd, ps, 17, 4096, torch.tensor([-5], dtype=torch.int32, device=DEV))[0::2]:
        assert bool((a == 0).all())


def test_sizes_above_the_limit_and_bad_arguments_are_refused():
    from fragnet_amd import _lib, ops
    big = ops.DENSE_MAX_ROWS + 1
    pl = torch.zeros(big, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.FragnetHipError, match="FN_DENSE_MAX_ROWS"):
        ops.pair_orderings_both(pl, pl, 4, 4)
    with pytest.raises(_lib.FragnetHipError, match="FN_DENSE_MAX_ROWS"):
        ops.pair_orderings_both(pl[:8], pl[:8], big, 4)
    with pytest.raises(_lib.FragnetHipError, match="FN_DENSE_MAX_ROWS"):
        ops.pair_orderings_both(pl[:8], pl[:8], 4, big)
    with pytest.raises(TypeError, match="int64"):
        ops.pair_orderings_both(pl[:8].int(), pl[:8], 4, 4)
    with pytest.raises(TypeError, match="int32"):
        ops.pair_orderings_both(pl[:8], pl[:8], 4, 4, real_pairs=torch.tensor([8], device=DEV))
    with pytest.raises(_lib.FragnetHipError, match="GPU"):
        ops.pair_orderings_both(pl[:8].cpu(), pl[:8].cpu(), 4, 4)
    torch.cuda.synchronize()
