"""Property test of one attention level: ``ops.gat_level`` (HIP, through the C-ABI) against the oracle's materialised-message
restatement of gat2.py:146-169 over RANDOM graphs -- next to the hand-picked cases of test_gpu_parity.py.

hypothesis draws the head count (1, 2, 4, 8), the edge-term form (a stored per-edge row, gat2.py:196-219, or the folded
``Linear(K -> d)`` of a raw attribute, gat2.py:146-164), ``add_self_loops`` (gat2.py:190-194), and the graph: isolated nodes,
duplicate edges, explicit self loops, hubs whose in-degree exceeds the 2 * (32 / heads) edges a half-wave takes in its fast path
(serial three-pass walk), and levels without any edge.  Forward rows, probabilities, the by-source attention read-out and the
gradient of every input are compared; tolerances as in test_gpu_parity.py (2e-5 absolute on O(1) rows, gradients 5e-5 x scale).
"""
import pytest
import torch

hypothesis = pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, given, settings  # noqa: E402
from hypothesis import strategies as st  # noqa: E402

pytestmark = pytest.mark.gpu

from tests.gat_level_common import DEV, _run  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    _lib.load()


@st.composite
def level_cases(draw):
    heads = draw(st.sampled_from([1, 2, 4, 8]))
    mode = draw(st.sampled_from([0, 2]))
    loops = draw(st.booleans())
    n = draw(st.integers(min_value=1, max_value=70))
    shape = draw(st.sampled_from(["empty", "sparse", "dense", "hub", "two_hubs", "self_loops", "chain"]))
    seed = draw(st.integers(min_value=0, max_value=2 ** 31 - 1))
    g = torch.Generator().manual_seed(seed)
    lph2 = 2 * (32 // heads)                         # edges of a row the half-wave's fast path takes
    if shape == "empty":
        m = 0
    elif shape == "sparse":
        m = draw(st.integers(min_value=1, max_value=max(1, n // 2)))          # most nodes isolated
    elif shape == "chain":
        m = max(1, n - 1)
    else:
        m = draw(st.integers(min_value=1, max_value=260))
    dst = torch.randint(0, n, (m,), generator=g)
    src = torch.randint(0, n, (m,), generator=g)
    if shape == "chain" and n > 1:
        dst, src = torch.arange(1, n), torch.arange(0, n - 1)
    if shape in ("hub", "two_hubs") and m > 0:
        k = min(m, lph2 + draw(st.integers(min_value=1, max_value=40)))       # in-degree beyond the fast path
        dst[:k] = draw(st.integers(min_value=0, max_value=n - 1))
        if shape == "two_hubs" and m > k:
            dst[k:k + min(m - k, lph2 + 3)] = draw(st.integers(min_value=0, max_value=n - 1))
    if shape == "self_loops" and m > 0:
        src[: (m + 1) // 2] = dst[: (m + 1) // 2]                             # explicit loops among the real edges
    K = draw(st.integers(min_value=1, max_value=8)) if mode == 2 else 0
    return dict(heads=heads, mode=mode, loops=loops, n=n, m=int(dst.numel()), dst=dst, src=src, K=K, seed=seed, shape=shape)


@settings(max_examples=240, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(level_cases())
def test_gat_level_equals_the_materialised_oracle_on_random_graphs(case):
    _run(case)


@pytest.mark.parametrize("heads", [1, 2, 4, 8])
def test_gat_level_hub_just_beyond_the_fast_path(heads):
    """in-degree 2 * (32 / heads) is the last row the half-wave takes in its fast path, + 1 the first it walks serially."""
    for extra in (0, 1):
        k = 2 * (32 // heads) + extra
        n = 9
        dst = torch.cat([torch.full((k,), 3), torch.tensor([0, 8])])
        src = torch.cat([torch.arange(k) % n, torch.tensor([5, 8])])
        _run(dict(heads=heads, mode=0, loops=False, n=n, m=int(dst.numel()), dst=dst, src=src, K=0, seed=heads + extra, shape=f"hub{k}"))
