"""Every launch geometry that ``bench.py --tune KEY=VALUE`` can select, forced into play on small inputs.

The attention, row-dots, weight-gradient and projection kernels have two regimes: a half-wave or block handles one row or tile, or it
loops over several.  Which one runs is host arithmetic over the tuning table (tests/launch_geometry_common.py has the formula); at the
defaults, sized for 512 molecules, the 4 - 96 molecules of the parity tests never leave the first regime.  Here the keys are set so that
the 51-molecule "edges" batch of tests/topologies.py (bond level: 1330 rows = 167 row groups) and a 70-row level walk several rows per
half-wave, end in a short last block whose trailing half-waves have no row, run as a single block, and write 1 .. 4096 partial rows.

  a. backward geometry (keys 23, 25, 12, 11, 13, 3, 21, 1): logits bit-identical to the default geometry, every parameter gradient within
     the suite's 1e-4 + 1e-4 |ref| of the float32 oracle (tests/test_topologies_host.py: itself 100 x closer to float64 on this batch)
  b. training-forward geometry (key 0) under dropout: outputs and gradients bit-identical to the default geometry -- mask bits belong to
     element positions, not to half-waves; tests/test_gpu_dropout_parity.py pins the default run to the oracle under the same masks
  c. operators: ops.linear128 under key 1 against float64 (tolerances of test_linear128_matches_torch), ops.gat_level under the
     forward / one-pass / two-pass keys against the materialised oracle (tests/gat_level_common.py, its tolerances)
  d. key 24 = 0 on a padded static batch: tests/test_gpu_engine_topologies.py, the captured step

Every key is set through tests/helpers.py::tuning, which puts back what it found."""
import ctypes as C

import pytest
import torch

from tests import launch_geometry_common as G
from tests.helpers import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    _lib.load()


def _check_rows(plan):
    """The geometry claims below are about THESE row counts."""
    assert plan.mol_built
    assert {lv: plan.levels[lv].n for lv in G.EDGES_ROWS} == G.EDGES_ROWS


# ----------------------------------------------------------------------------------------------- a. backward geometry against the oracle
def _step(heads, setting):
    """One training step (no dropout, the oracle's weights) on the "edges" batch under ``setting``: logits and the model with its gradients."""
    from tests import test_gpu_engine_topologies as ET
    gold, _, _ = ET._oracle("edges", heads)
    model = ET._model(heads, state=gold.state_dict())
    b = ET._dev_batch("edges")
    with tuning(setting):
        got = model(b)
        torch.nn.functional.mse_loss(got.view(-1), b["y"]).backward()
        torch.cuda.synchronize()
    b["_fragnet_plan"].check()
    _check_rows(b["_fragnet_plan"])
    return got.detach().cpu(), model


def _default_logits(heads):
    if ("logits", heads) not in _CACHE:
        _CACHE["logits", heads] = _step(heads, {})[0]
    return _CACHE["logits", heads]


def test_the_sweep_reaches_both_regimes_and_their_edges():
    """Of the bond level under the one-pass key: 1, 2, 3 and >= 8 rows per half-wave, the single-block launch, and a row count that is
    no multiple of a block's rows (the last block has idle half-waves).  The other keys take the same formula at their levels."""
    n = G.EDGES_ROWS["bond"]
    geo = {v: G.geometry(n, v) for v in G.ONE_BLOCKS_VALUES}
    print(geo)
    assert {1, 2, 3} <= {r for r, _ in geo.values()}
    assert any(r >= 8 for r, _ in geo.values())
    assert any(nblk == 1 for _, nblk in geo.values())
    assert any(n % (G.ROWS * r) != 0 for r, _ in geo.values())
    assert G.geometry(n, 768) == (1, -(-n // G.ROWS))                     # the default: the regime every other test runs
    for setting in G.BACKWARD_SETTINGS:
        if G.SRC_BLOCKS in setting:
            assert setting[G.BWD_ONE] == 0
    assert {G.geometry(n, s[G.SRC_BLOCKS])[0] for s in G.BACKWARD_SETTINGS if G.SRC_BLOCKS in s} == {167, 56, 5, 1}


def test_one_pass_launch_geometry_is_the_formula():
    """fn_gat_bwd_one_f32 on a level of the bond level's row count: the partial rows it reports (= its blocks) are the formula's nblk
    under every swept value of key 23 and at the default, and its outputs do not depend on the geometry beyond summation order."""
    from fragnet_amd import _lib
    from fragnet_amd.plan import GraphPlan, _stream_ptr
    from tests.test_gpu_bwd_one import _graph
    H, d, n, m = 4, 32, G.EDGES_ROWS["bond"], 3001
    dst, src, g = _graph(n, m, seed=23, hub="both")
    plan = GraphPlan([dict(kind="gat", name="l", dst=dst.to(DEV), src=src.to(DEV), n=n, n_loops=n)], DEV)
    lv = plan.levels["l"]
    M = lv.m
    assert lv.n == n
    st = _stream_ptr(torch.device(DEV))
    f32 = dict(dtype=torch.float32, device=DEV)
    h, gout = torch.randn(n, 128, generator=g).to(DEV), torch.randn(n, 128, generator=g).to(DEV)
    att_w = 2 * d + 128
    att = (torch.randn(H, att_w, generator=g) * 0.3).to(DEV)
    s_edge = (torch.randn(H, M, generator=g) * 0.5).to(DEV)
    et = _lib.EdgeTerm(0, 0, 0, 0, s_edge.data_ptr(), None, None, None)
    s_dst, s_src = torch.empty(n, H, **f32), torch.empty(n, H, **f32)
    out, out2, sigma, p_em = torch.empty(n, 128, **f32), torch.empty(n, 128, **f32), torch.empty(n, H, **f32), torch.empty(M, H, **f32)
    _lib.call("fn_node_scalars_f32", h.data_ptr(), att.data_ptr(), att_w, 0, att_w - d, s_dst.data_ptr(), s_src.data_ptr(), n, H, st)
    _lib.call("fn_gat_fwd_f32", h.data_ptr(), s_dst.data_ptr(), s_src.data_ptr(), att.data_ptr(), att_w, C.byref(et), C.byref(lv.c),
              0.2, out.data_ptr(), p_em.data_ptr(), None, out2.data_ptr(), sigma.data_ptr(), 1, None, H, st)
    cdot, gsd = torch.empty(n, H, **f32), torch.empty(n, H, **f32)
    _lib.call("fn_gat_cu_f32", gout.data_ptr(), out.data_ptr(), out2.data_ptr(), sigma.data_ptr(), 1.0, cdot.data_ptr(), gsd.data_ptr(), n, H, st)

    def run():
        g_h, dz_s = torch.empty(n, 128, **f32), torch.zeros(H, M, **f32)
        part_a = torch.zeros(256, _lib.FN_MAX_PART, **f32)                      # column-major [256][FN_MAX_PART]
        n_a, n_e = C.c_int(-1), C.c_int(-1)
        _lib.call("fn_gat_bwd_one_f32", gout.data_ptr(), h.data_ptr(), p_em.data_ptr(), cdot.data_ptr(), gsd.data_ptr(), C.byref(et),
                  att.data_ptr(), att_w, 0, att_w - d, C.byref(lv.c), 0.2, g_h.data_ptr(), dz_s.data_ptr(), None, part_a.data_ptr(),
                  C.byref(n_a), None, C.byref(n_e), 1, None, H, st)
        torch.cuda.synchronize()
        plan.check()
        assert not bool(part_a[:, n_a.value:].any())                            # no partial row behind the reported ones
        return n_a.value, n_e.value, g_h, dz_s, part_a[:, : n_a.value].sum(1)

    base = run()
    assert base[:2] == (G.geometry(n, _lib.load().fn_get_tuning(G.ONE_BLOCKS))[1], 0)
    for v in G.ONE_BLOCKS_VALUES:
        with tuning({G.ONE_BLOCKS: v}):
            got = run()
        assert got[:2] == (G.geometry(n, v)[1], 0), v
        for a, b, nm in zip(got[2:], base[2:], ("g_h", "dz", "column sums of part_a")):
            torch.testing.assert_close(a, b, atol=2e-5 * max(1.0, float(b.abs().max())), rtol=1e-4, msg=lambda s, nm=nm, v=v: f"{nm}, key 23 = {v}: {s}")


@pytest.mark.parametrize("setting", G.BACKWARD_SETTINGS, ids=G.sid)
@pytest.mark.parametrize("heads", [4, 2], ids=["engine_const_h4", "general_h2"])
def test_backward_geometry_matches_the_oracle(heads, setting):
    from tests import test_gpu_engine_topologies as ET
    _, want, want_g = ET._oracle("edges", heads)
    base = _default_logits(heads)
    got, model = _step(heads, setting)
    print(f"logits: max|diff| to the oracle = {float((got - want).abs().max()):.3e}, to the default geometry = {float((got - base).abs().max()):.3e}")
    torch.testing.assert_close(base, want, atol=ET.ATOL, rtol=1e-4)
    assert torch.equal(got, base), "a row's forward arithmetic does not depend on who walks it"
    ET._compare_grads(model, want_g)


# ----------------------------------------------------------------------------------------------- b. training-forward geometry
def _dropout_run(heads, setting):
    from tests import test_gpu_engine_topologies as ET
    from tests.test_gpu_tuning_keys import _encoder_run
    net = ET._model(heads, drop=0.1)
    b = ET._dev_batch("edges")
    with tuning(setting):
        res = _encoder_run(net, b, 999)
    _check_rows(b["_fragnet_plan"])
    return res


@pytest.mark.parametrize("blocks", G.FWD_BLOCKS_VALUES)
@pytest.mark.parametrize("heads", [4, 2], ids=["engine_const_h4", "general_h2"])
def test_training_forward_geometry_does_not_change_a_bit(heads, blocks):
    """drop_ratio 0.1, the same Philox offset: 167 / 84 / 34 / 8 rows per half-wave at the bond level against one."""
    if ("drop", heads) not in _CACHE:
        _CACHE["drop", heads] = _dropout_run(heads, {})
    o0, g0 = _CACHE["drop", heads]
    o1, g1 = _dropout_run(heads, {G.FWD_BLOCKS: blocks})
    assert G.geometry(G.EDGES_ROWS["bond"], blocks)[0] > 1
    assert len(o0) == len(o1) and len(o0) >= 2
    for a, c in zip(o0, o1):
        assert bool((a == 0).any()) and bool((a != 0).any())                   # the dropout epilogue ran
        assert torch.equal(a, c)
    assert set(g0) == set(g1) and len(g0) >= 20              # the encoder's parameters (the head is not run)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ----------------------------------------------------------------------------------------------- c. the operators
@pytest.mark.parametrize("slots", G.LINEAR_SLOTS)
@pytest.mark.parametrize("K", [6, 17, 128, 167])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 200, 1000])
def test_linear128_under_a_workgroup_cap_matches_float64(M, K, slots):
    """Key 1 > 0: a launch with more 64-row tiles (x two column halves) than slots walks several tiles per workgroup -- 200 rows are four
    tiles, the last one ragged; at 1, 2 and 3 slots one workgroup walks all of a column half's tiles, two walk them, three share them
    unevenly.  1024 slots: the cap set, one tile each.  The input gradient is asked for at K = 128, where it is this kernel too (every
    other K takes csrc/input_grad.hip, which the key does not reach), as in test_linear128_matches_torch."""
    from fragnet_amd import ops
    g = torch.Generator().manual_seed(M + K)
    xgrad = K == 128
    x = torch.randn(M, K, generator=g).to(DEV).requires_grad_(xgrad)
    w = (torch.randn(128, K, generator=g) * 0.2).to(DEV).requires_grad_(True)
    b = torch.randn(128, generator=g).to(DEV).requires_grad_(True)
    gy = torch.randn(M, 128, generator=g).to(DEV)
    with tuning({G.GEMM_SLOTS: slots}):
        y = ops.linear128(x, w, b)
        y.backward(gy)
        torch.cuda.synchronize()
    x2, w2, b2 = x.detach().double().requires_grad_(xgrad), w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    y2 = torch.nn.functional.linear(x2, w2, b2)
    y2.backward(gy.double())
    torch.testing.assert_close(y.detach(), y2.detach().float(), atol=2e-5, rtol=1e-5)
    torch.testing.assert_close(w.grad, w2.grad.float(), atol=2e-5 * max(1.0, float(w2.grad.abs().max())), rtol=1e-5)
    torch.testing.assert_close(b.grad, b2.grad.float(), atol=2e-5 * max(1.0, float(b2.grad.abs().max())), rtol=1e-5)
    if xgrad:
        torch.testing.assert_close(x.grad, x2.grad.float(), atol=2e-5, rtol=1e-5)


def _level_case(heads, mode, loops):
    """70 rows (9 row groups: 9 / 5 / 3 / 1 rows per half-wave at 1 / 2 / 4 / 9 blocks, the last block short at 2 and 4), 260 edges, a
    hub five edges beyond the half-wave's fast path in the middle of a block and a shorter one in the last row."""
    n, m = 70, 260
    g = torch.Generator().manual_seed(1000 * heads + 10 * mode + int(loops))
    dst = torch.randint(0, n, (m,), generator=g)
    src = torch.randint(0, n, (m,), generator=g)
    k = 2 * (32 // heads) + 5
    dst[:k] = 37
    dst[k: k + 7] = n - 1
    return dict(heads=heads, mode=mode, loops=loops, n=n, m=m, dst=dst, src=src, K=6 if mode == 2 else 0, seed=heads + mode, shape=f"hub{k}")


@pytest.mark.parametrize("one_pass", [True, False], ids=["fwd_and_one_pass", "dst_and_src_pass"])
@pytest.mark.parametrize("loops", [False, True], ids=["no_loops", "self_loops"])
@pytest.mark.parametrize("mode", [0, 2], ids=["stored_edge_term", "folded_linear"])
@pytest.mark.parametrize("heads", [1, 2, 4, 8])
def test_gat_level_geometry_matches_the_materialised_oracle(heads, mode, loops, one_pass):
    """BWD_ONE_PASS on: keys 10 (the forward) and 23 (the one-pass backward) at 1, 2, 4, 9 blocks; off: keys 11 and 12 (destination and
    source pass)."""
    from fragnet_amd import ops
    from tests.gat_level_common import _run
    case = _level_case(heads, mode, loops)
    assert [G.geometry(case["n"], v) for v in G.LEVEL_BLOCKS] == [(9, 1), (5, 2), (3, 3), (1, 9)]
    old = ops.BWD_ONE_PASS
    ops.BWD_ONE_PASS = one_pass
    try:
        for setting in G.LEVEL_SETTINGS[one_pass]:
            with tuning(setting):
                _run(case)
    finally:
        ops.BWD_ONE_PASS = old
