"""tests/adam_ref.py pinned on the CPU: the float64 restatement equals torch.optim.Adam run in float64 to float64 round-off, and
torch's own float32 Adam stays within the unit counts adam_ref.TORCH_F32_UNITS records -- the yardstick (times adam_ref.GPU_FACTOR)
that tests/test_gpu_adam.py holds the fused HIP kernels to.  Also: FlatAdam.gather_grads on CPU tensors."""
import itertools

import pytest
import torch

from tests import adam_ref

BETAS = [(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)]


def wide_state(n, seed, dtype=torch.float32):
    """p in 1e-4 .. 1e2, g in 1e-8 .. 1e3 (log-uniform, random signs), m of the size of some earlier g, v >= 0 likewise"""
    gen = torch.Generator().manual_seed(seed)

    def logu(lo, hi):
        e = torch.rand(n, generator=gen, dtype=torch.float64) * (hi - lo) + lo
        return 10.0 ** e

    def sign():
        return (torch.rand(n, generator=gen) < 0.5).double() * 2 - 1
    p = logu(-4, 2) * sign()
    g = logu(-8, 3) * sign()
    m = logu(-8, 3) * sign()
    v = logu(-8, 3) ** 2
    return tuple(t.to(dtype) for t in (p, g, m, v))


def torch_adam_one_step(p, g, m, v, step, lr, betas, eps, wd):
    """torch.optim.Adam, one step (number ``step``) from the given state, in the dtype of ``p``"""
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    q.grad = g.clone()
    opt.step()
    st = opt.state[q]
    assert int(st["step"]) == step
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("betas", BETAS)
def test_restatement_equals_torch_adam_in_float64_over_20_steps(wd, betas):
    """20 steps, both sides float64, the restatement taking every step from torch's own previous state AND free-running.  Seen:
    at most 4.1e-16 of the operand scale one step at a time, 2.5e-14 * max(|p|, 1e-3) free-running over 20 steps; asserted: 1e-14
    and 1e-13 (float64 round-off is 1.1e-16; the two formulas differ by a handful of roundings per step)."""
    gen = torch.Generator().manual_seed(5)
    n, lr, eps = 4096, 1e-2, 1e-8
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p_free, m_free, v_free = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    worst_step = worst_free = 0.0
    for k in range(1, 21):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** float(torch.randint(-4, 3, (1,), generator=gen))
        if k == 1:
            prev = (q.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
        else:
            st = opt.state[q]
            prev = (q.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
        q.grad = g.clone()
        opt.step()
        st = opt.state[q]
        want = adam_ref.adam_step64(prev[0], g, prev[1], prev[2], k, lr, betas, eps, wd)
        sc = adam_ref.scales(prev[0], g, prev[1], prev[2], k, lr, betas, eps, wd)
        for name, got, ref in (("p", q.detach(), want[0]), ("m", st["exp_avg"], want[1]), ("v", st["exp_avg_sq"], want[2])):
            worst_step = max(worst_step, float(((got - ref).abs() / sc[name]).max()))
        p_free, m_free, v_free = adam_ref.adam_step64(p_free, g, m_free, v_free, k, lr, betas, eps, wd)
        worst_free = max(worst_free, float(((q.detach() - p_free).abs() / p_free.abs().clamp_min(1e-3)).max()))
    print(f"float64: one step {worst_step:.2e} of the operand scale, free-running {worst_free:.2e} relative")
    assert worst_step <= 1e-14
    assert worst_free <= 1e-13


YARDSTICK_CASES = [(wd, eps, betas, step)
                   for (wd, eps, betas), step in zip(itertools.product([0.0, 1e-2], [1e-8, 1e-4], BETAS),
                                                     itertools.cycle([1, 2, 10, 1000, 10 ** 6]))] + \
                  [(0.0, 1e-8, (0.9, 0.999), s) for s in (1, 2, 10, 1000, 10 ** 6)] + \
                  [(1e-2, 1e-8, (0.9, 0.999), s) for s in (1, 10 ** 6)]


def measure_torch_f32_units(n=1 << 16):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, (wd, eps, betas, step) in enumerate(YARDSTICK_CASES):
        for lr in (1e-3, 1e-1):
            state = wide_state(n, seed=100 + i)
            got = torch_adam_one_step(*state, step, lr, betas, eps, wd)
            un = adam_ref.worst_units(got, state, step, lr, betas, eps, wd)
            for k in worst:
                worst[k] = max(worst[k], un[k])
    return worst


def test_float32_torch_adam_stays_within_the_recorded_units():
    """The yardstick of tests/test_gpu_adam.py: torch's float32 CPU Adam against the float64 restatement, one step from the same
    float32 state, in units of 2^-24 * operand magnitude (adam_ref's docstring holds the figures seen)."""
    worst = measure_torch_f32_units()
    print("torch float32 Adam, worst units:", {k: round(x, 2) for k, x in worst.items()})
    for k, x in worst.items():
        assert x <= adam_ref.TORCH_F32_UNITS[k], (k, x)
        assert x >= 0.25, (k, x)                 # a yardstick that reads 0 measures nothing (e.g. a float64 run by mistake)


def test_units_see_a_wrong_formula_from_far_away():
    """What 4 x the yardstick still catches: each classic Adam mistake, applied in float64 (so without any rounding of its own), is
    orders of magnitude outside adam_ref.gpu_bound."""
    state = wide_state(1 << 12, seed=3)
    step, lr, betas, eps, wd = 10, 1e-3, (0.9, 0.999), 1e-8, 1e-2
    p, g, m, v = (t.double() for t in state)
    gp = g + wd * p
    m1, v1 = 0.9 * m + 0.1 * gp, 0.999 * v + 0.001 * gp * gp
    bc1, bc2 = 1 - 0.9 ** step, 1 - 0.999 ** step
    wrong = {
        "no bias correction": p - lr * m1 / (v1.sqrt() + eps),
        "step off by one": p - lr / (1 - 0.9 ** (step - 1)) * m1 / (v1.sqrt() / (1 - 0.999 ** (step - 1)) ** 0.5 + eps),
        "decoupled weight decay": p * (1 - lr * wd) - lr / bc1 * (0.9 * m + 0.1 * g) / ((0.999 * v + 0.001 * g * g).sqrt() / bc2 ** 0.5 + eps),
    }
    for what, p_wrong in wrong.items():
        un = adam_ref.worst_units((p_wrong, m1, v1), state, step, lr, betas, eps, wd)
        assert un["p"] > 100 * adam_ref.gpu_bound("p"), (what, un)
    right = adam_ref.worst_units((p - lr / bc1 * m1 / (v1.sqrt() / bc2 ** 0.5 + eps), m1, v1), state, step, lr, betas, eps, wd)
    assert max(right.values()) < 1e-6


# ------------------------------------------------------------------------------------ FlatAdam.gather_grads on CPU tensors
SIZES = (1, 3, 4, 5, 8)


def _expected_runs(sizes, offsets, in_place):
    """maximal runs of consecutive parameters that are NOT in place and have no alignment padding between them: [(first, last)]"""
    runs, cur = [], None
    for i, (n, off) in enumerate(zip(sizes, offsets)):
        if i in in_place:
            cur = None
            continue
        if cur is not None and offsets[i - 1] + sizes[i - 1] == off:
            cur[1] = i
        else:
            cur = [i, i]
            runs.append(cur)
    return [tuple(r) for r in runs]


@pytest.mark.parametrize("in_place", [(), (1, 3), (4,), (0, 2), (0, 1, 2, 3, 4), (2, 3)], ids=lambda s: "inplace_" + "".join(map(str, s)))
def test_gather_grads_copies_maximal_runs_and_keeps_the_padding_zero(in_place, monkeypatch):
    from fragnet_amd import parallel
    gen = torch.Generator().manual_seed(17)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen)) for n in SIZES]
    opt = parallel.FlatAdam(params, lr=1e-3)
    assert opt.offsets == [0, 4, 8, 12, 20] and opt.grad.numel() == 28
    grads = [torch.randn(n, generator=gen) for n in SIZES]
    for i, (p, off) in enumerate(zip(params, opt.offsets)):
        if i in in_place:                                   # a producer wrote it into its slot: p.grad aliases opt.grad
            opt.grad[off: off + SIZES[i]] = grads[i]
            p.grad = opt.grad[off: off + SIZES[i]].view_as(p)
        else:
            p.grad = grads[i].clone()
    want = torch.zeros(28)
    for gr, off in zip(grads, opt.offsets):
        want[off: off + gr.numel()] = gr
    calls = []
    real_cat = torch.cat

    def spy(tensors, *a, out=None, **kw):
        calls.append((tuple(int(t.numel()) for t in tensors),
                      None if out is None else ((out.data_ptr() - opt.grad.data_ptr()) // 4, int(out.numel()))))
        return real_cat(tensors, *a, **kw) if out is None else real_cat(tensors, *a, out=out, **kw)
    monkeypatch.setattr(torch, "cat", spy)
    opt.gather_grads()
    monkeypatch.undo()
    assert torch.equal(opt.grad, want)
    pad = torch.ones(28, dtype=torch.bool)
    for n, off in zip(SIZES, opt.offsets):
        pad[off: off + n] = False
    assert int(pad.sum()) == 28 - sum(SIZES) and not opt.grad[pad].any()
    runs = _expected_runs(SIZES, opt.offsets, set(in_place))
    assert calls == [(tuple(SIZES[a: b + 1]), (opt.offsets[a], sum(SIZES[a: b + 1]))) for a, b in runs]
    # a second gather of the same gradients changes nothing; a parameter without gradient is an error
    opt.gather_grads()
    assert torch.equal(opt.grad, want)
    params[2].grad = None
    with pytest.raises(RuntimeError):
        opt.gather_grads()
