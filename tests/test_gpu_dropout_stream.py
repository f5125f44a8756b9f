"""The kernels' dropout stream against an independent reference (tests/philox_ref.py: Random123's Philox-4x32, seven rounds, keyed by
(seed, offset + element / 4), keep iff (bits >> 8) / 2^24 >= p): the standalone kernel and its backward, the fused epilogues that draw
masks of their own, and the block accounting -- no two draws of a step, and no two steps of a captured training loop, share a Philox
block.  Which elements are kept is compared exactly; a kept one carries float32(1) / (float32(1) - float32(p)) to 1 ulp (one fp32
division); nothing else has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import philox_ref
from tests.test_gpu_dropout_parity import TakeLog

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U64 = 0xFFFFFFFFFFFFFFFF

_RNG = np.random.default_rng(20240229)
P_LIST = [2.0 ** -k for k in range(1, 25)] + [float(np.float32(v)) for v in _RNG.uniform(0.0, 1.0, 16)] \
    + [2.0 ** -25, float(np.nextafter(np.float32(1), np.float32(0))), 0.0, 1.0]
SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1]
NUMELS = [1, 3, 4, 5, 1001, 4098]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    _lib.load()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _dropout(x, p, seed, offset, relu=0, offset_dev=None):
    from fragnet_amd import _lib
    y = torch.full_like(x, 7.0)
    _lib.call("fn_dropout_act_f32", x.data_ptr(), y.data_ptr(), x.numel(), float(p), seed, offset,
              None if offset_dev is None else offset_dev.data_ptr(), relu, _stream())
    return y


def _want(numel, p, seed, offset):
    return torch.from_numpy(philox_ref.mask(numel, p, seed, offset))


def _check_ones(y, p, seed, offset, note):
    """``y`` = dropout of ones: the kept elements are the reference's, and every kept one is 1 / (1 - p) to 1 ulp"""
    y = y.detach().cpu().reshape(-1)
    if p == 0.0:
        assert torch.equal(y, torch.ones_like(y)), note
        return
    want = _want(y.numel(), p, seed, offset)
    assert torch.equal(y != 0, want), f"{note}: kept elements differ from the reference at {torch.nonzero((y != 0) != want).reshape(-1)[:8].tolist()}"
    s = philox_ref.scale(p)
    kept = y[want].numpy()
    assert (np.abs(kept.astype(np.float64) - float(s)) <= float(np.spacing(s))).all(), (note, kept[:4], s)


# ------------------------------------------------------------------------------------------------ a. the standalone kernel
@pytest.mark.parametrize("numel", NUMELS)
def test_dropout_on_ones_keeps_the_references_elements_for_every_p(numel):
    """numel % 4 != 0 ends in the tail path; p = 2^-k puts the threshold on a power of two, 2^-25 makes it 1, nextafter(1, 0) leaves
    the top value only, p = 0 keeps all, p = 1 none (scale 0)."""
    ones = torch.ones(numel, device=DEV)
    seed, offset = 0x1234567, 5
    for p in P_LIST:
        _check_ones(_dropout(ones, p, seed, offset), p, seed, offset, f"numel={numel} p={p!r}")
    assert not _dropout(ones, 1.0, seed, offset).any()
    if numel >= 1001:          # nextafter(1, 0) really is "hardly any", 2^-25 "hardly none": the edge cases are not vacuous on both sides
        assert int((_dropout(ones, P_LIST[-3], seed, offset) != 0).sum()) <= 1
        assert int((_dropout(ones, 2.0 ** -25, seed, offset) == 0).sum()) <= 1


@pytest.mark.parametrize("numel,at", [(4098, 0), (4098, 2049), (1001, 1000), (3, 1)])
def test_an_element_with_u_equal_to_p_is_kept(numel, at):
    """keep iff u >= p: with p set to the u of one element of the reference stream (k / 2^24 is exact in float32) that element sits ON
    the threshold and stays -- a random p meets this case with probability 2^-24 per element.  (1001, 1000) and (3, 1) are elements of
    the tail path."""
    seed, offset = 0xABCDEF, 17
    words = philox_ref.philox4x32(np.arange(offset, offset + (numel + 3) // 4, dtype=np.uint64), seed, philox_ref.ROUNDS).reshape(-1)
    k = int(words[at] >> 8)
    assert 0 < k < 1 << 24
    p = k / 2.0 ** 24
    assert philox_ref.threshold(p) == k and bool(philox_ref.mask(numel, p, seed, offset)[at])
    y = _dropout(torch.ones(numel, device=DEV), p, seed, offset)
    assert float(y[at]) != 0.0
    _check_ones(y, p, seed, offset, f"p = u of element {at}")


@pytest.mark.parametrize("seed", SEEDS)
def test_dropout_on_ones_uses_both_words_of_the_seed(seed):
    for numel in (5, 4098):
        _check_ones(_dropout(torch.ones(numel, device=DEV), 0.25, seed, 3), 0.25, seed, 3, f"seed={seed:#x} numel={numel}")


@pytest.mark.parametrize("offset,numel", [(0, 4098), (1, 4098), (2 ** 32 - 3, 32), (2 ** 40, 4098), (2 ** 40, 5)])
def test_dropout_on_ones_uses_both_words_of_the_block_index(offset, numel):
    """offset 2^32 - 3 with 32 elements: blocks 2^32 - 3 .. 2^32 + 4, across the carry into the high word"""
    seed = 2 ** 63 + 5
    _check_ones(_dropout(torch.ones(numel, device=DEV), 0.25, seed, offset), 0.25, seed, offset, f"offset={offset:#x} numel={numel}")


def test_masks_of_neighbouring_offsets_are_the_same_stream_shifted():
    """element e at offset o + 1 is element e + 4 at offset o: the block index is offset + element / 4 and nothing else"""
    ones = torch.ones(4098, device=DEV)
    a, b = _dropout(ones, 0.25, 9, 100), _dropout(ones, 0.25, 9, 101)
    assert torch.equal(a[4:], b[:-4])


# ------------------------------------------------------------------------------------------------ b. the device counter
@pytest.mark.parametrize("offset,d", [(7, 0), (7, 5), (2 ** 32 - 2, 3), (3, 2 ** 32 - 1), (2 ** 40, 2 ** 33 + 1)])
def test_device_counter_is_added_to_the_offset(offset, d):
    dev = torch.tensor([d], dtype=torch.int64, device=DEV)
    seed, numel, p = 2 ** 32 + 77, 1001, 0.25
    _check_ones(_dropout(torch.ones(numel, device=DEV), p, seed, offset, offset_dev=dev), p, seed, offset + d, f"offset={offset:#x} + device {d:#x}")


# ------------------------------------------------------------------------------------------------ c. the backward
@pytest.mark.parametrize("numel", [5, 1001, 4098])
def test_dropout_backward_replays_the_mask(numel):
    from fragnet_amd import _lib
    seed, offset, p = 2 ** 63 + 5, 2 ** 32 - 1, 0.25
    dev = torch.tensor([2], dtype=torch.int64, device=DEV)
    ones = torch.ones(numel, device=DEV)
    g_x = torch.full_like(ones, 7.0)
    _lib.call("fn_dropout_act_bwd_f32", ones.data_ptr(), None, g_x.data_ptr(), numel, p, seed, offset, dev.data_ptr(), 0, _stream())
    _check_ones(g_x, p, seed, offset + 2, f"backward, relu = 0, numel={numel}")
    # relu = 1: the saved output gates it further -- zero, negative and NaN rows of y pass nothing
    g = torch.Generator().manual_seed(numel)
    y = torch.randn(numel, generator=g)
    y[::7] = 0.0
    y[3::11] = float("nan")
    g_x = torch.full_like(ones, 7.0)
    _lib.call("fn_dropout_act_bwd_f32", ones.data_ptr(), y.to(DEV).data_ptr(), g_x.data_ptr(), numel, p, seed, offset, dev.data_ptr(), 1, _stream())
    want = _want(numel, p, seed, offset + 2) & (y > 0)
    if numel >= 1001:
        assert 0 < int(want.sum()) < int(_want(numel, p, seed, offset + 2).sum())
    assert torch.equal(g_x.cpu() != 0, want)
    kept = g_x.cpu()[want].numpy()
    s = philox_ref.scale(p)
    assert (np.abs(kept.astype(np.float64) - float(s)) <= float(np.spacing(s))).all()


def test_dropout_forward_with_relu_gates_by_sign_and_mask():
    numel, p, seed, offset = 4098, 0.25, 2 ** 64 - 1, 2 ** 40
    x = torch.randn(numel, generator=torch.Generator().manual_seed(1))
    y = _dropout(x.to(DEV), p, seed, offset, relu=1).cpu()
    assert torch.equal(y != 0, _want(numel, p, seed, offset) & (x > 0))


# ------------------------------------------------------------------------------------------------ d. the fused consumers
# Inputs that make every pre-activation strictly positive: y > 0 <=> the element was kept.
def _positive(shape, seed, lo=0.25):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) + lo).to(DEV)


@pytest.mark.parametrize("M,K,N", [(37, 8, 68), (1536, 32, 1024)], ids=["per_wave", "shared_tiles"])
def test_dense_forward_epilogue_draws_the_references_mask(M, K, N):
    """fn_dense_fwd_f32 with an fn_act_epilogue: the per-wave kernel, and the workgroup-shared-tile kernel at the smallest shape that
    selects it (192 tiles of 64 x 128, K a multiple of 32)."""
    from fragnet_amd import _lib
    x, w, b = _positive((M, K), 1), _positive((N, K), 2), _positive((N,), 3)
    y = torch.full((M, N), -7.0, device=DEV)
    seed, offset, p = 2 ** 63 + 5, 2 ** 32 - 11, 0.25
    dev = torch.tensor([6], dtype=torch.int64, device=DEV)
    act = _lib.ActEpilogue(y.data_ptr(), p, 1, seed, offset, dev.data_ptr())
    _lib.call("fn_dense_fwd_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, C.byref(act), _stream())
    y = y.cpu()
    assert (y >= 0).all()
    assert torch.equal(y != 0, _want(M * N, p, seed, offset + 6).view(M, N))


def test_dense_forward_dropout_of_act_draws_the_references_mask():
    """fn_dense_fwd_act_f32 in FTHead1/4's order, y = dropout(silu(z)), z > 0"""
    from fragnet_amd import _lib
    M, K, N, p = 37, 256, 128, 0.25
    x, w, b = _positive((M, K), 4), _positive((N, K), 5) / K, _positive((N,), 6)
    slope = torch.tensor([0.23], device=DEV)
    seed, off = 2 ** 33 + 1234 + M, 2 ** 32 - 4
    off_dev = torch.tensor([5], dtype=torch.int64, device=DEV)
    y, pre = torch.full((M, N), 7.0, device=DEV), torch.full((M, N), 7.0, device=DEV)
    spec = _lib.HeadAct(_lib.ACT_SILU, _lib.ACT_ACT_THEN_DROP, p, 0, seed, off, off_dev.data_ptr(), slope.data_ptr(), pre.data_ptr(), None)
    _lib.call("fn_dense_fwd_act_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, C.byref(spec), _stream())
    assert (pre > 0).all()                                    # the saved argument is z itself in this order
    y = y.cpu()
    assert (y >= 0).all()
    assert torch.equal(y != 0, _want(M * N, p, seed, off + 5).view(M, N))


@pytest.mark.parametrize("heads", [4, 8])
def test_attention_forward_epilogue_draws_the_references_mask(heads):
    """fn_gat_fwd_f32 with an fn_act_epilogue on a plan built as test_gpu_gat_level_property.py builds it (70 nodes, self loops, about
    200 random edges): every output row is a convex combination of positive rows of h, so y > 0 <=> kept."""
    from fragnet_amd import _lib, ops
    from fragnet_amd.plan import GraphPlan
    n, m, p = 70, 200, 0.25
    d = 128 // heads
    g = torch.Generator().manual_seed(heads)
    dst, src = torch.randint(0, n, (m,), generator=g), torch.randint(0, n, (m,), generator=g)
    h = _positive((n, 128), 7)
    att = (torch.randn(heads, 2 * d + 128, generator=g) * 0.3).to(DEV)
    feat = torch.randn(m, 128, generator=g).to(DEV)
    plan = GraphPlan([dict(kind="gat", name="l", dst=dst.to(DEV), src=src.to(DEV), n=n, n_loops=n)], DEV)
    lv = plan.levels["l"]
    s_sorted = ops.row_dots_sorted(feat, att, d, lv)
    att_w = att.shape[1]
    s_dst, s_src = torch.empty(n, heads, device=DEV), torch.empty(n, heads, device=DEV)
    _lib.call("fn_node_scalars_f32", h.data_ptr(), att.data_ptr(), att_w, 0, att_w - d, s_dst.data_ptr(), s_src.data_ptr(), n, heads, _stream())
    out, y = torch.full((n, 128), -7.0, device=DEV), torch.full((n, 128), -7.0, device=DEV)
    p_sorted = torch.empty(heads, lv.m, device=DEV)
    seed, offset = 2 ** 64 - 3, 2 ** 32 - 100
    dev = torch.tensor([9], dtype=torch.int64, device=DEV)
    et = _lib.EdgeTerm(0, 0, 0, 0, s_sorted.data_ptr(), None, None, None)
    act = _lib.ActEpilogue(y.data_ptr(), p, 1, seed, offset, dev.data_ptr())
    _lib.call("fn_gat_fwd_f32", h.data_ptr(), s_dst.data_ptr(), s_src.data_ptr(), att.data_ptr(), att_w, C.byref(et), C.byref(lv.c), 0.2,
              out.data_ptr(), p_sorted.data_ptr(), None, None, None, 0, C.byref(act), heads, _stream())
    torch.cuda.synchronize()
    plan.check()
    assert (out > 0).all()
    y = y.cpu()
    want = _want(n * 128, p, seed, offset + 9).view(n, 128)
    assert torch.equal(y != 0, want)
    s = float(philox_ref.scale(p))
    torch.testing.assert_close(y[want].double(), out.cpu()[want].double() * s, atol=0, rtol=2.0 ** -22)     # one product, one division


# ------------------------------------------------------------------------------------------------ e. block accounting
def _intervals(calls):
    return sorted((off, off + (numel + 3) // 4) for _, off, numel in calls)


def _assert_back_to_back(ivals, start):
    """sorted [lo, hi) intervals: pairwise disjoint, no gap, the first one at ``start``.  Returns where the last one ends."""
    for lo, hi in ivals:
        assert lo == start and hi > lo, (ivals, start)
        start = hi
    return start


def _eager_models():
    from fragnet_amd.model import FragNetFineTune, FragNetPreTrain
    from oracle import fragnet_ref as ref
    from tests.helpers import load_case
    c, batch, *_ = load_case("ft_esol_b8")
    for fthead, n_draws in (("FTHead3", 1 + 4), ("FTHead4", 1 + 2)):        # the encoder's one draw + the head's
        cfg = dict(c["ctor"], drop_ratio=0.1, fthead=fthead, act="relu")
        yield fthead, FragNetFineTune(**cfg), batch, (lambda out, b: torch.nn.functional.mse_loss(out.view(-1), b["y"])), n_draws
    c, batch, *_ = load_case("pt_esol_b4")
    yield "pretrain", FragNetPreTrain(**dict(c["ctor"], drop_ratio=0.1)), batch, ref.pretrain_loss, 1


def test_eager_steps_draw_back_to_back_block_ranges():
    """Every draw of a training step -- the encoder's range, then the head's layers -- takes the blocks right behind the draw before
    it, and the next step goes on where this one ended: no block is used twice, none is left out."""
    from fragnet_amd import data
    for name, model, batch, loss_fn, n_draws in _eager_models():
        torch.manual_seed(3)
        model = model.to(DEV).train()
        b = data.batch_to(batch, DEV)
        end = 0
        for step in range(2):
            with TakeLog(model.pretrain.rng) as log:
                loss_fn(model(dict(b)), b).backward()
            torch.cuda.synchronize()
            assert len(log.calls) == n_draws, (name, log.calls)
            assert len({seed for seed, _, _ in log.calls}) == 1
            end = _assert_back_to_back(_intervals(log.calls), end)
        assert end == model.pretrain.rng.offset and end > 0, name


def _oracle_loss_and_grads(gold, cpu_batch, masks):
    from oracle import fragnet_ref as ref
    inj = ref.inject_dropout(gold, masks)
    want = gold(cpu_batch)
    loss = torch.nn.functional.mse_loss(want.view(-1), cpu_batch["y"])
    loss.backward()
    assert inj.cursor == len(masks)
    return float(loss), {n: q.grad for n, q in gold.named_parameters() if q.grad is not None}


def test_captured_steps_and_the_eager_fallback_never_share_a_block(monkeypatch):
    """replay, replay, one batch beyond the capacities (eager fallback), replay, replay: the five steps' block ranges
    [rng_base + c, rng_base + c + drawn) -- c what the device counter held when the step's kernels ran -- are pairwise disjoint and
    lie behind everything the warm-up steps drew from the host-side offset.  The first replay after the fallback then has to agree
    with the oracle under the REFERENCE's masks at its range: the accounting is what the kernels drew."""
    from fragnet_amd import data, graphstep, parallel, synth
    from fragnet_amd.model import FragNetFineTune
    from oracle import fragnet_ref as ref
    from tests import test_gpu_dropout_parity as parity
    p = 0.1
    cfg = dict(n_classes=1, num_layer=3, num_heads=4, drop_ratio=p, h1=128, h2=256, h3=128, h4=64, act="relu", fthead="FTHead3")
    cpu_batches = [data.collate_fn(synth.synth_molecules(64, seed=700 + i, profile="esol")) for i in range(2)]
    bs = [data.batch_to(cb, DEV) for cb in cpu_batches]
    big = data.batch_to(data.collate_fn(synth.synth_molecules(96, seed=702, profile="esol")), DEV)
    torch.manual_seed(0)
    gold = ref.FragNetFineTune(**cfg).train()
    model = FragNetFineTune(**cfg)
    model.load_state_dict(gold.state_dict())
    model = model.to(DEV).train()
    model.pretrain.rng.seed = 2 ** 63 + 0x7654321
    with TakeLog(model.pretrain.rng) as log:
        opt = parallel.FlatAdam.for_live_parameters(
            model, lambda: torch.nn.functional.mse_loss(model(dict(bs[0])).view(-1), bs[0]["y"]).backward(), lr=0.0)
        shapes = graphstep.StaticShapes.from_batches(bs, margin=0.05)
        step = graphstep.GraphedTrainStep(model, opt, shapes, dict(bs[0]), loss="regr")
    drop = step.rng_counter
    base, per_step, behind = drop.base, drop.per_step, (drop.per_step if drop.staged else 0)
    captured = log.calls[-5:]                                 # the draws made inside the capture: the offsets baked into the graph
    assert per_step > 0 and _intervals(captured)[0][0] == base
    assert _assert_back_to_back(_intervals(captured), base) == base + per_step
    warm = _intervals(log.calls[:-5])
    assert warm and _assert_back_to_back(warm, 0) == base     # probe + warm-up steps: host-side offsets, device counter 0

    def counter():
        return int(step._counters[0].item())

    # c of a replay: the counter after the step when the staging launch in front of the replay moved it (single graph), the counter
    # before the graph's own advance otherwise
    ranges, seen = [], None
    for i, b in enumerate([bs[1], bs[0], big, bs[0], bs[1]]):
        before = counter()
        if b is big:
            with TakeLog(model.pretrain.rng) as flog:
                step(dict(b))
            assert step.fallbacks == 1
            c = before + behind
            lo = min(off for _, off, _ in flog.calls)
            assert lo == base                                 # the fallback draws from the captured step's base offsets
            drawn = _assert_back_to_back(_intervals(flog.calls), base) - base
            assert drawn > per_step                           # it is a larger batch
        else:
            loss = float(step(dict(b)))
            c = counter() if drop.staged else before
            drawn = per_step
        torch.cuda.synchronize()
        ranges.append((base + c, base + c + drawn))
        if i == 3:                                            # the first replay after the fallback: keep what the oracle is compared with
            grads = {}
            for name, q in model.named_parameters():
                slot = getattr(q, "_fn_grad_slot", None)
                if slot is not None:
                    grads[name] = slot[0][slot[1]: slot[1] + q.numel()].view(q.shape).cpu().clone()
            seen = (c, loss, grads)
    assert step.replays == 4 and step.fallbacks == 1
    print("block ranges:", ranges, "per step", per_step, "warm-up ends at", base)
    for i, (lo, hi) in enumerate(ranges):
        assert lo >= base, (i, ranges)                        # behind every warm-up draw
        for lo2, hi2 in ranges[i + 1:]:
            assert hi <= lo2 or hi2 <= lo, (i, ranges)
    assert ranges == sorted(ranges) and ranges[0][0] == base

    # the masks of step 4 from the reference, through the existing test's helpers
    def ref_mask(numel, p_, seed, offset):
        return torch.from_numpy(philox_ref.mask(numel, p_, seed, offset)).float() * float(philox_ref.scale(p_))
    monkeypatch.setattr(parity, "philox_mask", ref_mask)
    c, loss, grads = seen
    cap = shapes.cap
    real = tuple(int(bs[0][k].shape[0]) for k in ("x_atoms", "x_frags", "node_features_bonds", "node_features_fbonds"))
    masks = parity.encoder_masks(captured[0], p, (cap["atom"], cap["frag"], cap["edge"], cap["fedge"]), cfg["num_layer"],
                                 bs[0]["x_atoms"].shape[1], real, extra_offset=c)
    B, rows = int(bs[0]["y"].shape[0]), captured[1][2] // cfg["h1"]
    masks += parity.head3_masks(captured[1:], p, [cfg["h1"], cfg["h2"], cfg["h3"], cfg["h4"]], rows, B, extra_offset=c)
    want_loss, want_grads = _oracle_loss_and_grads(gold, cpu_batches[0], masks)
    assert abs(loss - want_loss) < parity.ATOL, (loss, want_loss)
    checked = 0
    for name, want in want_grads.items():
        if name in grads:
            torch.testing.assert_close(grads[name], want, atol=parity.ATOL, rtol=1e-4, msg=lambda s, name=name: f"{name}: {s}")
            checked += 1
    assert checked >= 40
