"""The loss kernels (k_masked_mse, k_masked_bce, k_mse_multi_partial / k_mse_multi_finish in csrc/fragnet_hip.hip) against float64
torch formulas of the same losses, loss value and gradient with respect to ``out``, at the shapes, weight patterns and logits where
such kernels go wrong: one element, more rows than threads, padded tails, fractional row weights, logits where
``log1pf(expf(-|x|))`` and ``1 / (1 + expf(-x))`` saturate, columns without a label, a single valid entry.

Bounds, from the summation shape each kernel's comment describes, with u = 2^-24 (the unit round-off of float32); none of them
comes from an observed error:

  loss       (ceil(n / threads) + log2(threads) + 8) * u * sum|term| / denom -- every thread adds ceil(n / threads) terms serially,
             a tree over the threads combines them, 8 covers the roundings inside one term and the final division.  threads = 1024
             for the one-block kernels; 64 * 256 for the multi-task kernel (64 blocks of 256 threads per task; block b takes the
             elements b * 256 + t + k * 16384), whose total is sum_k coef_k * loss_k, so the bounds of the tasks add up with |coef_k|.
             MSE terms w * d^2 are non-negative, so sum|term| / denom is the loss itself; BCE terms are the float64 stable form
             max(x, 0) - x * t + log1p(exp(-|x|)) of each valid entry.
  gradient   4 * u * |g| per element: the reciprocal of the denominator, the difference out - y, and two products (the row
             weights used here, 0, 0.25 and 1, multiply exactly); for BCE an absolute 4 * u / N more for the cancellation in
             sigmoid(x) - t, whose terms are at most 1.

Out of scope: a batch with no valid entry at all (all row weights 0, or every label missing) is 0 / 0 in the reference formulas
too; the trainers never build one (a batch has at least one real molecule), and nothing here tests it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _dev():
    return torch.device("cuda:0")


def loss_bound(n, threads, sum_abs_terms_over_denom):
    return (math.ceil(n / threads) + math.log2(threads) + 8) * U * sum_abs_terms_over_denom


def assert_grad(got, want, extra_abs, what):
    """|got - want| <= 4 u |want| + extra_abs, element-wise; ``want`` float64"""
    err = (got.detach().double().cpu() - want).abs()
    bound = 4 * U * want.abs() + extra_abs
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} gradient elements outside 4u|g| + {extra_abs:.1e}; worst {float((err / bound.clamp_min(1e-300)).max()):.2f} x the bound"
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------- masked_mse
def mse_ref(out, y, w):
    """float64: sum_i w_i sum_t (out - y)^2 / (sum_i w_i * T) and its gradient"""
    o = out.detach().double().cpu().requires_grad_(True)
    B = w.shape[0]
    d = o.reshape(B, -1) - y.double().cpu().reshape(B, -1)
    loss = (w.double().cpu()[:, None] * d * d).sum() / (w.double().cpu().sum() * d.shape[1])
    loss.backward()
    return float(loss.detach()), o.grad


def weights(pattern, B, gen):
    w = torch.ones(B)
    if pattern == "padded_tail":                       # the static-shape batch: real rows first, padding behind
        w[B - max(1, B // 8):] = 0.0
    elif pattern == "single_row":
        w.zero_()
        w[B // 2] = 1.0
    elif pattern == "fractional":                      # the kernel multiplies by w (it does not test w > 0): pin that
        w = torch.where(torch.rand(B, generator=gen) < 0.5, 0.25, 1.0)
        w[0] = 0.25
    else:
        assert pattern == "ones"
    return w


MSE_SHAPES = [(1, 1), (3, 1), (1023, 1), (1025, 3), (5000, 12)]
MSE_CASES = [(B, T, pat) for B, T in MSE_SHAPES for pat in ("ones", "padded_tail", "single_row", "fractional")
             if not (B == 1 and pat in ("padded_tail", "single_row"))]          # one row: nothing to pad, "single row" is "ones"


@pytest.mark.parametrize("B,T,pattern", MSE_CASES)
def test_masked_mse_matches_float64(B, T, pattern):
    from fragnet_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(B * 31 + T)
    out = (torch.randn(B, T, generator=gen) * 2).to(dev).requires_grad_(True)
    y = torch.randn(B, T, generator=gen).to(dev)
    w = weights(pattern, B, gen).to(dev)
    loss = ops.masked_mse(out, y, w)
    loss.backward()
    want, g_want = mse_ref(out, y, w)
    bound = loss_bound(B * T, 1024, abs(want))
    err = abs(float(loss.detach()) - want)
    print(f"masked_mse ({B},{T}) {pattern}: loss error {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    worst = assert_grad(out.grad, g_want, 0.0, f"masked_mse ({B},{T}) {pattern}")
    rows_off = (w == 0).cpu()
    assert not out.grad.cpu()[rows_off].any(), "a row of weight 0 got a gradient"
    print(f"    gradient: worst {worst:.2f} x (4 u |g|)")


# ---------------------------------------------------------------------------------------------------------- masked_bce
LOGITS = [0.0, 1e-6, -1e-6, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4]
LABELS = [0.0, 1.0, -1.0]


def bce_ref(out, y, w):
    """float64: train.compute_bce_loss with the padded rows masked out as well (the formula of test_head_ops), its gradient by
    autograd, and sum|term| / N with the terms in the stable form written out"""
    x = out.detach().double().cpu().requires_grad_(True)
    t = y.double().cpu().reshape(x.shape)
    valid = (t > -0.5) & (w.cpu()[:, None] > 0)
    n_valid = int(valid.sum())
    mat = torch.nn.functional.binary_cross_entropy_with_logits(x, t.clamp(min=0.0), reduction="none")
    loss = torch.where(valid, mat, torch.zeros_like(mat)).sum() / n_valid
    loss.backward()
    xd = x.detach()
    stable = xd.clamp(min=0.0) - xd * t.clamp(min=0.0) + torch.log1p(torch.exp(-xd.abs()))
    terms = float(torch.where(valid, stable, torch.zeros_like(stable)).abs().sum()) / n_valid
    assert abs(float(torch.where(valid, stable, torch.zeros_like(stable)).sum()) / n_valid - float(loss.detach())) <= 1e-12 * max(1.0, terms)
    return float(loss.detach()), terms, x.grad, valid, n_valid


def bce_inputs(B, T, case, gen):
    combos = [(x, t) for x in LOGITS for t in LABELS]                 # 39: every logit with every label
    if case == "moderate":                                            # the same without |x| > 20: sum|term| stays small, so the
        combos = [(x, t) for x, t in combos if abs(x) <= 20.0]        # loss bound is tight enough to see one wrong small term
    idx = torch.arange(B * T) % len(combos)
    out = torch.tensor([c[0] for c in combos])[idx].reshape(B, T).clone()
    y = torch.tensor([c[1] for c in combos])[idx].reshape(B, T).clone()
    w = torch.ones(B)
    if B > 4:
        w[B - max(1, B // 8):] = 0.0                                  # padded rows
    if case == "missing_column":
        y[:, T // 2] = -1.0
    elif case == "one_valid":
        y.fill_(-1.0)
        y[B // 3, T - 1] = 1.0
        out[B // 3, T - 1] = -1.0
        assert w[B // 3] > 0
    return out, y, w


BCE_SHAPES = [(1, 1), (5, 12), (1024, 12), (1030, 13)]
BCE_CASES = [(B, T, case) for B, T in BCE_SHAPES for case in ("grid", "moderate", "missing_column", "one_valid")
             if not (T == 1 and case == "missing_column")]            # the only column without labels: no valid entry (docstring)


@pytest.mark.parametrize("B,T,case", BCE_CASES)
def test_masked_bce_matches_float64(B, T, case):
    from fragnet_amd import ops, train
    dev = _dev()
    gen = torch.Generator().manual_seed(B + T)
    out_c, y_c, w_c = bce_inputs(B, T, case, gen)
    out = out_c.to(dev).requires_grad_(True)
    y, w = y_c.to(dev), w_c.to(dev)
    loss = ops.masked_bce(out, y, w)
    loss.backward()
    want, terms, g_want, valid, N = bce_ref(out, y, w)
    # the written-out stable form is train.compute_bce_loss on the real rows
    real = w_c > 0
    assert abs(want - float(train.compute_bce_loss(out_c[real].double(), y_c[real].double()))) <= 1e-12 * max(1.0, abs(want))
    assert math.isfinite(float(loss.detach()))
    bound = loss_bound(B * T, 1024, terms)
    err = abs(float(loss.detach()) - want)
    print(f"masked_bce ({B},{T}) {case}: N = {N}, loss {want:.6g}, error {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    g = out.grad.cpu()
    assert bool(torch.isfinite(g).all())
    worst = assert_grad(g, g_want, 4 * U / N, f"masked_bce ({B},{T}) {case}")
    print(f"    gradient: worst {worst:.2f} x (4 u |g| + 4 u / N)")
    assert not g[~valid].any(), "a missing label or a padded row got a gradient"
    # saturated logits: sigmoid is exactly 0 or 1 in float32, the gradient exactly (0 - t) / N or (1 - t) / N
    inv = torch.tensor(1.0) / torch.tensor(float(N))
    sat = valid & (out_c.abs() >= 1e4)
    if sat.any():
        expect = ((out_c > 0).float() - y_c.clamp(min=0.0)) * inv
        assert torch.equal(g[sat], expect[sat])
    if case == "missing_column":
        assert not g[:, T // 2].any()
    if case == "one_valid":
        assert N == 1 and int((g != 0).sum()) == 1


# ------------------------------------------------------------------------------------------------------ masked_mse_multi
MULTI_CASES = {
    "one_task": ([(1.0, -1)], [(5, 1)]),
    "two_tasks": ([(2.0, 0), (1.0, -1)], [(20000, 3), (5, 1)]),
    "three_tasks": ([(2.0, 0), (1.0, 1), (1.0, -1)], [(1000, 1), (20000, 3), (7, 2)]),
    "four_tasks": ([(0.5, 1), (2.0, 0), (1.0, -1), (3.0, 0)], [(5, 1), (300, 4), (20000, 3), (16385, 1)]),
}


@pytest.mark.parametrize("case", list(MULTI_CASES))
def test_masked_mse_multi_matches_float64_and_the_single_losses(case):
    """1 - 4 tasks, scale indices -1, 0, 1, from 5 rows (63 of a task's 64 blocks idle) to (20000, 3) (every thread loops)"""
    from fragnet_amd import ops
    dev = _dev()
    spec, sizes = MULTI_CASES[case]
    gen = torch.Generator().manual_seed(len(spec))
    scale = torch.tensor([0.9, 1.3], dtype=torch.float32)
    outs, ys, ws = [], [], []
    for k, (b, t) in enumerate(sizes):
        outs.append((torch.randn(b, t, generator=gen) * 2).to(dev).requires_grad_(True))
        ys.append(torch.randn(b, t, generator=gen).to(dev))
        ws.append(weights(("padded_tail", "fractional", "ones", "padded_tail")[k], b, gen).to(dev))
    triples = [x for k in range(len(spec)) for x in (outs[k], ys[k], ws[k])]
    loss = ops.masked_mse_multi(spec, scale.to(dev), *triples)
    loss.backward()
    want, bound, single_sum, single_bound = 0.0, 0.0, 0.0, 0.0
    for k, (c, idx) in enumerate(spec):
        coef = c * (float(scale[idx]) if idx >= 0 else 1.0)
        lk, gk = mse_ref(outs[k], ys[k], ws[k])
        n = sizes[k][0] * sizes[k][1]
        want += coef * lk
        bound += abs(coef) * loss_bound(n, 64 * 256, abs(lk))
        worst = assert_grad(outs[k].grad, coef * gk, 0.0, f"{case} task {k}")
        assert not outs[k].grad.cpu()[(ws[k] == 0).cpu()].any()
        with torch.no_grad():
            single_sum += coef * float(ops.masked_mse(outs[k].detach(), ys[k], ws[k]))
        single_bound += abs(coef) * loss_bound(n, 1024, abs(lk))
        print(f"{case} task {k} {sizes[k]}: gradient worst {worst:.2f} x (4 u |g|)")
    err = abs(float(loss.detach()) - want)
    print(f"{case}: loss {want:.6g}, error {err:.2e} (bound {bound:.2e}); against the single launches {abs(float(loss.detach()) - single_sum):.2e}")
    assert err <= bound
    assert abs(float(loss.detach()) - single_sum) <= bound + single_bound + 4 * U * abs(want)      # both sit within their bounds of the float64 sum
