"""Store policy of the row tables (csrc/fn_internal.h: st4_next / st4_late and their 4-byte twins).

A store flavour changes no value: its hazard is visibility and ordering.  So every test here runs a producer and its consumer back to back
on one stream, with no synchronisation in between, on the smallest shapes that reach every store site, and asks for the values the plain
stores gave: the oracle at the suite's tolerances, and the same bits from run to run, from the eager launches to a replayed hipGraph and
from replay to replay.

  a. one attention level, forward then backward, through ops.gat_level: 1 row (one half-wave), 2, 33 (crosses a wave), 65 (eight full
     blocks of 8 rows and a block of one); no edge at all, an odd number of edges (the last probability store of a lane pair is partial),
     a hub row beyond the fast path's 2 (32 / H) in-edges (the serial walk); one head and four
  b. projection -> attention level -> input-gradient product: ops.linear128 with K = 6, 17, 128, 167 and M = 1, 63, 65 rows feeding a level
  c. the engine's chain (projections, attention launches, the input-gradient products with the row-dots epilogue) on the 6-molecule golden
     batch and the 51-molecule "edges" batch of tests/topologies.py: eager launches against a captured step replayed three times
  d. an evaluation pass behind a training step on the same workspace against the evaluation pass alone

Every case first asserts, from the built plan's row pointers, that the rows and edges it relies on are there."""
import numpy as np
import pytest
import torch

from tests import topologies as T
from tests.gat_level_common import _run as run_level_against_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# ----------------------------------------------------------------------------------------------- a. one attention level
def _level_case(n, heads, shape, mode):
    g = torch.Generator().manual_seed(1000 * n + 10 * heads + mode + {"none": 0, "odd": 1, "hub": 2}[shape] * 100)
    fast = T.fast_rows(heads)                         # 2 (32 / heads): the longest row of the fast path
    if shape == "none":
        dst = src = torch.zeros(0, dtype=torch.int64)
    else:
        m = 2 * n + 1                                 # odd
        dst = torch.randint(0, n, (m,), generator=g)
        src = torch.randint(0, n, (m,), generator=g)
        if shape == "hub":                            # row 0 takes fast + 1 edges more: beyond the fast path whatever the draw gave it
            dst = torch.cat([dst, torch.zeros(fast + 1, dtype=torch.int64)])
            src = torch.cat([src, torch.randint(0, n, (fast + 1,), generator=g)])
            if dst.numel() % 2 == 0:
                dst, src = torch.cat([dst, dst[:1]]), torch.cat([src, src[:1]])
    return dict(heads=heads, mode=mode, loops=False, n=n, m=int(dst.numel()), dst=dst, src=src, K=6, seed=int(g.initial_seed()),
                shape=f"store-policy {shape}")


def _row_lengths(dst, src, n):
    """Destination-row lengths of the level, read from the row pointers of the plan the kernels walk."""
    from fragnet_amd.plan import GraphPlan
    plan = GraphPlan([dict(kind="gat", name="l", dst=dst.to(DEV), src=src.to(DEV), n=n, n_loops=0)], DEV)
    for name, role, ib, sb, items, segs in plan.task_meta:
        if name == "l" and role == 1:
            assert segs == n
            return np.diff(plan.rowptr[sb: sb + segs + 1].cpu().numpy().astype(np.int64))
    raise AssertionError("the plan has no by-destination task for the level")


def _hip_level(case):
    """ops.gat_level forward + backward on the device, nothing between the launches; (out, p_sorted, gradients)."""
    from fragnet_amd import ops
    from fragnet_amd.plan import GraphPlan
    heads, mode, n, m, K = case["heads"], case["mode"], case["n"], case["m"], case["K"]
    d = 128 // heads
    g = torch.Generator().manual_seed(case["seed"] + 7)
    h = torch.randn(n, 128, generator=g)
    w_out = torch.randn(n, 128, generator=g).to(DEV)
    plan = GraphPlan([dict(kind="gat", name="l", dst=case["dst"].to(DEV), src=case["src"].to(DEV), n=n, n_loops=0)], DEV)
    lv = plan.levels["l"]
    if mode == 2:
        ins = (h, torch.randn(heads, 3 * d, generator=g) * 0.3, torch.randn(d, K, generator=g) * 0.5, torch.randn(d, generator=g) * 0.5)
        x = torch.randn(m, K, generator=g)
    else:
        ins = (h, torch.randn(heads, 2 * d + 128, generator=g) * 0.3, torch.randn(m, 128, generator=g))
    dl = [t.to(DEV).requires_grad_(True) for t in ins]
    if mode == 2:
        out, _, p_sorted = ops.gat_level(dl[0], dl[1], lv, heads, x_sorted=plan.sorted_attr("l", x.to(DEV)), embW=dl[2], embb=dl[3], want_probs=True)
    else:
        out, _, p_sorted = ops.gat_level(dl[0], dl[1], lv, heads, s_sorted=ops.row_dots_sorted(dl[2], dl[1], d, lv), want_probs=True)
    (out * w_out).sum().backward()
    torch.cuda.synchronize()
    plan.check()
    return [out.detach(), p_sorted.detach()] + [t.grad for t in dl if t.grad is not None]


@pytest.mark.parametrize("mode", [0, 2], ids=["stored_term", "folded_term"])
@pytest.mark.parametrize("shape", ["none", "odd", "hub"])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 33, 65])
def test_attention_level_forward_then_backward(n, heads, shape, mode):
    case = _level_case(n, heads, shape, mode)
    rows = _row_lengths(case["dst"], case["src"], n)
    assert rows.sum() == case["m"] and len(rows) == n
    if shape == "none":
        assert case["m"] == 0 and n > 0                                   # nodes without a single edge
    else:
        assert case["m"] % 2 == 1                                         # an odd edge count
    if shape == "hub":
        assert rows[0] > T.fast_rows(heads), (rows[0], T.fast_rows(heads))         # the serial walk
    run_level_against_oracle(case)                                        # rows, probabilities, read-out, every input's gradient
    a, b = _hip_level(case), _hip_level(case)
    assert len(a) == len(b) >= 3
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"tensor {i} differs between two runs"


# ----------------------------------------------------------------------------------------------- b. projection -> level -> input gradient
def _projection_chain(K, M, dev):
    """x [M, K] -> Linear(K, 128) -> one attention level over M nodes (four heads, folded edge term) -> weighted sum; backward.  On the
    device the operators are ops.linear128 / ops.gat_level, on the CPU torch and the oracle's materialised level."""
    heads, d, Ke = 4, 32, 6
    g = torch.Generator().manual_seed(31 * K + M)
    m = 2 * M + 1
    dst, src = torch.randint(0, M, (m,), generator=g), torch.randint(0, M, (m,), generator=g)
    ins = (torch.randn(M, K, generator=g), torch.randn(128, K, generator=g) / K ** 0.5, torch.randn(128, generator=g) * 0.1,
           torch.randn(heads, 3 * d, generator=g) * 0.3, torch.randn(d, Ke, generator=g) * 0.5, torch.randn(d, generator=g) * 0.5)
    xe, w_out = torch.randn(m, Ke, generator=g), torch.randn(M, 128, generator=g)
    leaves = [t.to(dev).requires_grad_(True) for t in ins]
    x, W, b, att, eW, eb = leaves
    if dev == "cpu":
        from oracle.fragnet_ref import gat_level_materialised
        h = torch.nn.functional.linear(x, W, b)
        out, _, _ = gat_level_materialised(h.view(M, heads, d), torch.nn.functional.linear(xe, eW, eb), att, dst, src, heads)
        if out.shape[0] < M:
            out = torch.cat([out, torch.zeros(M - out.shape[0], heads, d)])
        out = out.reshape(M, 128)
        rows = None
    else:
        from fragnet_amd import ops
        from fragnet_amd.plan import GraphPlan
        plan = GraphPlan([dict(kind="gat", name="l", dst=dst.to(dev), src=src.to(dev), n=M, n_loops=0)], dev)
        h = ops.linear128(x, W, b)                                        # producer ...
        out, _, _ = ops.gat_level(h, att, plan.levels["l"], heads, x_sorted=plan.sorted_attr("l", xe.to(dev)), embW=eW, embb=eb,
                                  want_probs=True)                        # ... and consumer, nothing in between
        rows = _row_lengths(dst, src, M)
    (out * w_out.to(dev)).sum().backward()
    if dev != "cpu":
        torch.cuda.synchronize()
    return out.detach(), [t.grad for t in leaves], rows, m


@pytest.mark.parametrize("M", [1, 63, 65])
@pytest.mark.parametrize("K", [6, 17, 128, 167])
def test_projection_feeds_attention_level(K, M):
    want, want_g, _, _ = _projection_chain(K, M, "cpu")
    got, got_g, rows, m = _projection_chain(K, M, DEV)
    assert len(rows) == M and rows.sum() == m and m % 2 == 1             # M rows (a 64-row tile: 1 = one row, 63 = short, 65 = two tiles)
    torch.testing.assert_close(got.cpu(), want, atol=1e-4, rtol=1e-4)
    for a, r, nm in zip(got_g, want_g, ("x", "W", "b", "att", "embW", "embb")):
        scale = max(1.0, float(r.abs().max()))
        torch.testing.assert_close(a.cpu(), r, atol=1e-4 * scale, rtol=1e-4, msg=lambda s, nm=nm: f"grad {nm}: {s}")
    again, again_g, _, _ = _projection_chain(K, M, DEV)
    assert torch.equal(got, again)
    for a, r in zip(got_g, again_g):
        assert torch.equal(a, r)


# ----------------------------------------------------------------------------------------------- c. the engine's chain, eager and replayed
def _golden6():
    from fragnet_amd import data
    from fragnet_amd.model import FragNetFineTune
    from tests.helpers import load_case
    cfg, batch, *_ = load_case("ft_edge_b6")
    torch.manual_seed(cfg["seed"])
    model = FragNetFineTune(**dict(cfg["ctor"], drop_ratio=0.0)).to(DEV).train()
    return model, data.batch_to(batch, DEV), 6


def _edges51():
    from fragnet_amd import data
    from fragnet_amd.model import FragNetFineTune
    torch.manual_seed(3)
    model = FragNetFineTune(**dict(T.CFG, drop_ratio=0.0), num_heads=4, fthead="FTHead3").to(DEV).train()
    recs = T.BATCHES["edges"]()
    T.assert_batch_claims("edges", recs, 4)
    return model, data.batch_to(T.collate(recs), DEV), 51


@pytest.mark.parametrize("make", [_golden6, _edges51], ids=["golden_6_molecules", "edges_51_molecules"])
def test_engine_chain_eager_and_replayed_give_the_same_bits(make):
    from fragnet_amd import graphstep, parallel
    model, b, n_mols = make()
    assert int(b["y"].shape[0]) == n_mols
    opt = parallel.FlatAdam.for_live_parameters(model, lambda: torch.nn.functional.mse_loss(model(b).view(-1), b["y"]).backward(), lr=0.0)
    b.pop("_fragnet_plan", None)
    shapes = graphstep.StaticShapes.from_batches([b], margin=0.02)
    if hasattr(b, "max_per_mol"):                     # a collated batch: its own maxima keep the one-launch plan builder (as test_gpu_engine_topologies.py does)
        shapes.max_per_mol = dict(b.max_per_mol)
    step = graphstep.GraphedTrainStep(model, opt, shapes, b, loss="regr")
    # eager: the launches of the captured step, one by one, on the staged batch
    assert step.static.load(b)
    opt.zero_grad()
    loss, _ = step._fwd_bwd_static()
    torch.cuda.synchronize()
    plan = step.static.t["_fragnet_plan"]
    plan.check()
    lengths = T.plan_row_lengths(plan)
    assert all(lv in lengths and max(lengths[lv]) >= 1 for lv in T.LEVELS), lengths          # every level has rows with edges
    if n_mols == 51:
        for lv, want in T.required_rows("edges", 4).items():
            assert want <= lengths[lv], (lv, sorted(want - lengths[lv]))
    want_loss, want_grad = loss.detach().clone(), opt.grad.detach().clone()
    assert torch.isfinite(want_grad).all() and float(want_grad.abs().max()) > 0
    for i in range(3):
        assert step.replay(b)
        torch.cuda.synchronize()
        assert torch.equal(step.loss.detach().view(-1), want_loss.view(-1)), f"loss of replay {i}"
        assert torch.equal(opt.grad, want_grad), f"flat gradient buffer of replay {i}"
    assert step.replays == 3 and step.fallbacks == 0


# ----------------------------------------------------------------------------------------------- d. evaluation behind a training step
def test_evaluation_pass_behind_a_training_step_reads_no_stale_line():
    """The evaluation launches reuse the workspace the training step's "late" tables live in: their outputs behind a training step are
    the bits of the evaluation pass alone."""
    model, b, _ = _edges51()
    model.eval()
    with torch.no_grad():
        alone = model(b).clone()
    torch.cuda.synchronize()
    plan = b["_fragnet_plan"]
    lengths = T.plan_row_lengths(plan)
    for lv, want in T.required_rows("edges", 4).items():
        assert want <= lengths[lv], (lv, sorted(want - lengths[lv]))
    model.train()
    b.pop("_fragnet_plan", None)
    torch.nn.functional.mse_loss(model(b).view(-1), b["y"]).backward()            # training step ...
    model.eval()
    b.pop("_fragnet_plan", None)
    with torch.no_grad():
        behind = model(b).clone()                                                 # ... and the evaluation pass right behind it
    torch.cuda.synchronize()
    assert torch.isfinite(alone).all()
    assert torch.equal(alone, behind)
