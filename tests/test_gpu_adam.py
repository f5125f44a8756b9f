"""The fused Adam update (adam_body in csrc/shared_bodies.inc) against the float64 restatement of torch.optim.Adam in
tests/adam_ref.py -- through all four places it runs: k_adam under fn_adam_f32 (bias corrections on the host), k_adam under
fn_adam_dev_f32 (step count and learning rate in device memory, bias corrections on the device), and the riders in the encoder
backward's last and first launch (k_reduce_tasks, k_tail_bwd) of a captured training step.

Every comparison is ONE step from the kernel's own previous float32 state, so nothing drifts, and the bound is the one measured on
the CPU: adam_ref.TORCH_F32_UNITS (what torch's float32 Adam shows against the same restatement, in units of 2^-24 times the operand
magnitudes) times adam_ref.GPU_FACTOR = 4.  adam_ref's docstring has the figures and the reasoning.

The restatement is given the hyper-parameters THE KERNEL is given.  fn_adam_f32, fn_adam_dev_f32 and fn_adam_slice take beta1,
beta2, eps and weight_decay as C floats (and the device form a float32 learning rate), and adam_body derives everything from those:
``1.f - beta`` for the weights of the new gradient, ``1 - pow((double)beta, step)`` for the bias corrections.  It is therefore Adam
at the float32-rounded betas, exactly and self-consistently (the weights of m and v sum to 1, v / bc2 of a constant gradient is its
square at every step).  Against Adam at the DOUBLE betas the same update differs by more than rounding: 1 - float32(0.999) is
0.0010000467, 4.7e-5 above 0.001, so a step whose v is dominated by the new g^2 comes out 2.3e-5 (390 units) smaller.  That is the
price of a float in the ABI, not an error of the update rule, and tests/test_gpu_trajectory.py bounds what it amounts to over a
trajectory against torch's float64 Adam at the double betas; here ``kernel_hypers`` rounds them the way the call does.

Found by these tests and fixed with them: adam_body used to update m as ``m + (g - m) * (1 - beta1)`` for every beta1.  The
difference g - m rounds to -m where |g| < 2^-24 |m|, so at beta1 = 0 (where m' is simply g) a small gradient after a large one was
lost altogether and the parameter stood still -- millions of units on p in the beta1 = 0 cases below.  It now takes the lerp from
the end with the larger weight, as torch's does (``g - (g - m) * beta1`` once 1 - beta1 >= 0.5); beta1 > 0.5, the default included,
keeps the form and the bits it had."""
import pytest
import torch

from tests import adam_ref
from tests.helpers import tuning
from tests.test_adam_ref_host import YARDSTICK_CASES, wide_state

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.25
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 2048 + 5]      # the last: k_adam's grid-stride loop twice, and the n & 3 tail


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _dev():
    return torch.device("cuda:0")


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def kernel_hypers(betas, eps, wd):
    """the values the C floats of the call hold (module docstring)"""
    return (_f32(betas[0]), _f32(betas[1])), _f32(eps), _f32(wd)


def make_state(n, seed):
    """float32 CPU (p, g, m, v) over wide magnitudes, with the gradient classes of one tensor (by element index mod 8):
    1: exact zero with m = v = 0; 2: 1e-20; 3: +-1e15; the rest p in 1e-4 .. 1e2, g in 1e-8 .. 1e3 with mixed signs."""
    p, g, m, v = wide_state(n, seed)
    i = torch.arange(n)
    zero, tiny, huge = i % 8 == 1, i % 8 == 2, i % 8 == 3
    g[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
    g[tiny] = 1e-20
    g[huge] = torch.where(i[huge] % 16 == 3, 1e15, -1e15).float()
    return p, g, m, v, zero


class Guarded:
    """four buffers of ``total`` elements, each between GUARD sentinel elements; ``lo:hi`` is the range a call works on"""

    def __init__(self, state, dev):
        self.n = state[0].numel()
        self.raw = []
        for t in state:
            buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
            buf[GUARD: GUARD + self.n] = t.to(dev)
            self.raw.append(buf)
        self.p, self.g, self.m, self.v = (b[GUARD: GUARD + self.n] for b in self.raw)
        self.g0 = self.g.clone()

    def ptrs(self, lo=0):
        return [t.data_ptr() + 4 * lo for t in (self.p, self.g, self.m, self.v)]

    def state(self):
        return tuple(t.detach().cpu().clone() for t in (self.p, self.g, self.m, self.v))

    def assert_guards_and_gradient_untouched(self):
        for name, buf in zip("pgmv", self.raw):
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + self.n:] == SENTINEL).all()), f"{name}: guard elements written"
        assert torch.equal(self.g, self.g0), "the gradient was written"


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def adam_host(G, n, step, lr, betas, eps, wd, lo=0):
    from fragnet_amd import _lib
    _lib.call("fn_adam_f32", *G.ptrs(lo), n, float(lr), float(betas[0]), float(betas[1]), float(eps), float(wd), int(step), _stream(G.p.device))
    return float(lr)


def adam_dev(G, n, step, lr, betas, eps, wd, lo=0):
    """the device form: int64 step count and float32 learning rate in device memory.  Returns the learning rate the kernel read."""
    from fragnet_amd import _lib
    step_dev = torch.tensor([int(step)], dtype=torch.int64, device=G.p.device)
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=G.p.device)
    _lib.call("fn_adam_dev_f32", *G.ptrs(lo), n, lr_dev.data_ptr(), float(betas[0]), float(betas[1]), float(eps), float(wd),
              step_dev.data_ptr(), _stream(G.p.device))
    torch.cuda.synchronize()
    return _f32(lr)


FORMS = {"host": adam_host, "dev": adam_dev}


def check_step(before, after, step, lr, betas, eps, wd, what):
    """``after`` = (p, g, m, v) one step from ``before``: within adam_ref.gpu_bound of the float64 restatement"""
    betas, eps, wd = kernel_hypers(betas, eps, wd)
    un = adam_ref.worst_units((after[0], after[2], after[3]), before, step, lr, betas, eps, wd)
    for k, x in un.items():
        assert x <= adam_ref.gpu_bound(k), f"{what}: {k} off by {x:.1f} units (bound {adam_ref.gpu_bound(k)})"
    return un


def check_zero_class(before, after, zero, wd):
    """g = m = v = 0 without weight decay: p must not move, m and v stay 0 (eps > 0 keeps 0 / (0 + eps) finite).  With weight decay
    g' = wd * p is not zero and the element decays like any other: the bound against the restatement covers it."""
    if wd == 0 and zero.any():
        assert torch.equal(after[0][zero], before[0][zero]), "a parameter with g = m = v = 0 moved"
        assert not after[2][zero].any() and not after[3][zero].any()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", SIZES)
def test_one_step_at_every_size_between_guards(n, form):
    dev = _dev()
    step, lr, betas, eps = 10, 1e-3, (0.9, 0.999), 1e-8
    wd = (0.0, 1e-2)[SIZES.index(n) % 2]                 # sizes 1, 3, 5, 1023, 1025 without weight decay, the others with
    *state, zero = make_state(n, seed=n % 1000)
    G = Guarded(state, dev)
    before = G.state()
    lr_read = FORMS[form](G, n, step, lr, betas, eps, wd)
    after = G.state()
    G.assert_guards_and_gradient_untouched()
    assert all(bool(torch.isfinite(t).all()) for t in after)
    un = check_step(before, after, step, lr_read, betas, eps, wd, f"n={n} {form}")
    check_zero_class(before, after, zero, wd)
    assert not torch.equal(after[0], before[0])
    print(f"n={n} {form}: units", {k: round(x, 2) for k, x in un.items()})


@pytest.mark.parametrize("wd,eps,betas,step", YARDSTICK_CASES,
                         ids=[f"wd{wd:g}-eps{eps:g}-b{b[0]:g}_{b[1]:g}-step{s}" for wd, eps, b, s in YARDSTICK_CASES])
def test_hyper_parameters_in_both_forms(wd, eps, betas, step):
    """wd x eps x betas with the step counts 1, 2, 10, 1000, 10^6 cycled over them, and all five at the defaults, with and without
    weight decay at the ends: the host form and the device form from the same state, both within the bound of the restatement.
    Whether they agree bit for bit is printed, not asserted: pow() in double on the host and on the device may differ in the last
    bit, which can move the rounded float32 factors lr / bc1 and 1 / sqrt(bc2)."""
    dev = _dev()
    n, lr = 1027, 1e-3
    *state, zero = make_state(n, seed=step % 997 + int(eps * 1e8))
    results = {}
    for form, run in FORMS.items():
        G = Guarded(state, dev)
        before = G.state()
        lr_read = run(G, n, step, lr, betas, eps, wd)
        after = G.state()
        G.assert_guards_and_gradient_untouched()
        assert all(bool(torch.isfinite(t).all()) for t in after)
        un = check_step(before, after, step, lr_read, betas, eps, wd, form)
        check_zero_class(before, after, zero, wd)
        results[form] = (after, un)
    same = all(torch.equal(a, b) for a, b in zip(results["host"][0], results["dev"][0]))
    print(f"host form vs device form bit-identical: {same}; units host", {k: round(x, 2) for k, x in results["host"][1].items()},
          "dev", {k: round(x, 2) for k, x in results["dev"][1].items()})


@pytest.mark.parametrize("form", list(FORMS))
def test_slice_of_a_larger_buffer_leaves_its_neighbours_alone(form):
    """[lo, hi) 16-byte aligned with (hi - lo) % 4 == 3 -- what FlatAdam.adam_in_graph(lo, hi) and the rider's slice pass"""
    dev = _dev()
    total, lo, hi = 4096, 1024, 1024 + 515
    assert lo % 4 == 0 and (hi - lo) % 4 == 3
    step, lr, betas, eps, wd = 2, 1e-3, (0.9, 0.999), 1e-8, (0.0 if form == "host" else 1e-2)
    *state, zero = make_state(total, seed=9)
    G = Guarded(state, dev)
    before = G.state()
    lr_read = FORMS[form](G, hi - lo, step, lr, betas, eps, wd, lo=lo)
    after = G.state()
    G.assert_guards_and_gradient_untouched()
    for b, a, name in zip(before, after, "pgmv"):
        assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[hi:], b[hi:]), f"{name}: elements outside [lo, hi) written"
    check_step(tuple(t[lo:hi] for t in before), tuple(t[lo:hi] for t in after), step, lr_read, betas, eps, wd, f"slice {form}")
    check_zero_class(tuple(t[lo:hi] for t in before), tuple(t[lo:hi] for t in after), zero[lo:hi], wd)
    assert not torch.equal(after[0][lo:hi], before[0][lo:hi])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("where", [517, 1028], ids=["vector_part", "tail"])
def test_one_nan_gradient_poisons_one_element(where, form):
    dev = _dev()
    n, step, lr, betas, eps, wd = 1029, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2
    *state, _ = make_state(n, seed=4)
    clean = Guarded(state, dev)
    FORMS[form](clean, n, step, lr, betas, eps, wd)
    state[1][where] = float("nan")
    bad = Guarded(state, dev)
    FORMS[form](bad, n, step, lr, betas, eps, wd)
    for name, buf in zip("pgmv", bad.raw):          # (its gradient holds a NaN, NaN != NaN: the guards only)
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), name
    keep = torch.ones(n, dtype=torch.bool)
    keep[where] = False
    for a, b, name in ((bad.p, clean.p, "p"), (bad.m, clean.m, "m"), (bad.v, clean.v, "v")):
        a, b = a.cpu(), b.cpu()
        assert not bool(torch.isfinite(a[where])), f"{name}[{where}] stayed finite under a NaN gradient"
        assert torch.equal(a[keep], b[keep]), f"{name}: a NaN gradient leaked into other elements"
        assert bool(torch.isfinite(a[keep]).all())


def test_refusals_return_einval_and_change_nothing():
    """step < 1, a pointer off 16-byte alignment, a null lr_dev / step_dev: FN_EINVAL, nothing written"""
    from fragnet_amd import _lib
    dev = _dev()
    lib = _lib.load()
    n = 64
    *state, _ = make_state(n, seed=2)
    G = Guarded(state, dev)
    before = G.state()
    st = _stream(dev)
    hyper = (0.9, 0.999, 1e-8, 0.0)
    step_dev = torch.tensor([1], dtype=torch.int64, device=dev)
    lr_dev = torch.tensor([1e-3], dtype=torch.float32, device=dev)
    for step in (0, -1):
        assert lib.fn_adam_f32(*G.ptrs(), n, 1e-3, *hyper, step, st) == _lib.FN_EINVAL
    for k in range(4):                                   # each of p, g, m, v one float off a 16-byte boundary
        ptrs = G.ptrs()
        ptrs[k] += 4
        assert lib.fn_adam_f32(*ptrs, n - 1, 1e-3, *hyper, 1, st) == _lib.FN_EINVAL
        assert lib.fn_adam_dev_f32(*ptrs, n - 1, lr_dev.data_ptr(), *hyper, step_dev.data_ptr(), st) == _lib.FN_EINVAL
    assert lib.fn_adam_dev_f32(*G.ptrs(), n, None, *hyper, step_dev.data_ptr(), st) == _lib.FN_EINVAL
    assert lib.fn_adam_dev_f32(*G.ptrs(), n, lr_dev.data_ptr(), *hyper, None, st) == _lib.FN_EINVAL
    torch.cuda.synchronize()
    for b, a in zip(before, G.state()):
        assert torch.equal(a, b)
    G.assert_guards_and_gradient_untouched()
    # and the valid call right after them goes through
    adam_host(G, n, 1, 1e-3, (0.9, 0.999), 1e-8, 0.0)
    assert not torch.equal(G.state()[0], before[0])


def test_adam_slice_wants_a_16_byte_aligned_start():
    from fragnet_amd import parallel
    dev = _dev()
    opt = parallel.FlatAdam([torch.nn.Parameter(torch.randn(n, device=dev)) for n in (5, 8, 3)], lr=1e-3)
    step_dev = torch.tensor([1], dtype=torch.int64, device=dev)
    lr_dev = torch.tensor([1e-3], dtype=torch.float32, device=dev)
    for lo in (1, 2, 3, 5, 9):
        with pytest.raises(ValueError):
            opt.adam_slice(step_dev, lr_dev, lo)
    with pytest.raises(ValueError):
        opt.adam_slice(step_dev, lr_dev, 8, 4)
    assert opt.adam_slice(step_dev, lr_dev, 8).n == opt.flat.numel() - 8


# -------------------------------------------------- the captured step: Adam node, riders, device step counter, lr_dev plumbing
CONFIGS = {"adam_node_only": dict(rider=False, at=0, wd=0.0),
           "rider_in_last_launch": dict(rider=True, at=0, wd=0.0),
           "rider_in_first_launch": dict(rider=True, at=1, wd=0.0),
           "rider_with_weight_decay": dict(rider=True, at=0, wd=1e-2)}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_captured_step_updates_like_the_restatement(config, monkeypatch):
    """Five replays of GraphedTrainStep with Adam inside the graph, the learning rate halved after the third.  Each replay's update
    of the WHOLE flat buffer and both moment buffers is compared with the restatement, one step from the buffers as they were
    before the replay, with step number k and the learning rate in force -- which pins the device step counter, the lr_dev
    plumbing and the rider's block range to an independent reference instead of to each other.

    The gradient is read from ``opt.grad`` after the replay.  That is what the update consumed: the graph overwrites the gradients
    at the start of a replay (FlatAdam.zero_grad only drops the views; the producers rewrite every slot and gather_grads copies the
    rest), the head's slots are final once the head's backward has run -- the condition under which the rider may consume them --
    and nothing writes ``opt.grad`` behind the Adam node, the last one of the graph.  Default eps = 1e-8: one step at a time does
    not drift."""
    from fragnet_amd import data, graphstep, parallel
    from tests.test_graphstep import _batches, _make
    cfg = CONFIGS[config]
    dev = _dev()
    batches = [data.batch_to(b, dev) for b in _batches(3, 40)]
    shapes = graphstep.StaticShapes.from_batches(batches, margin=0.05)
    model, _, lr = _make(dev, drop=0.1)
    betas, eps, wd = (0.9, 0.999), 1e-8, cfg["wd"]
    opt = parallel.FlatAdam.for_live_parameters(
        model, lambda: torch.nn.functional.mse_loss(model(dict(batches[0])).view(-1), batches[0]["y"]).backward(), lr=lr, weight_decay=wd)
    assert opt.hyper["eps"] == eps and opt.hyper["betas"] == betas
    monkeypatch.setattr(graphstep, "ADAM_RIDER", cfg["rider"])
    with tuning({28: cfg["at"]}):
        step = graphstep.GraphedTrainStep(model, opt, shapes, dict(batches[0]), loss="regr")
    assert step.adam_in_graph
    numel = opt.flat.numel()
    lo = step._rider_lo
    assert lo is not None and 0 < lo < numel
    pad = torch.ones(numel, dtype=torch.bool, device=dev)
    for p, off in zip(opt.params, opt.offsets):
        pad[off: off + p.numel()] = False
    assert int(pad.sum()) > 0, "this model has no alignment padding: nothing to pin"
    for k in range(1, 6):
        if k == 4:
            opt.hyper["lr"] = lr = lr * 0.5
        before = tuple(t.detach().clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq))
        step(dict(batches[(k - 1) % 3]))
        torch.cuda.synchronize()
        g = opt.grad.detach().clone()
        after = tuple(t.detach().clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq))
        assert opt.steps == k and int(step._counters[1]) == k
        state = tuple(t.cpu() for t in (before[0], g, before[1], before[2]))
        un = adam_ref.worst_units(tuple(t.cpu() for t in after), state, k, _f32(lr), *kernel_hypers(betas, eps, wd))
        print(f"{config} replay {k}: units", {name: round(x, 2) for name, x in un.items()})
        for name, x in un.items():
            assert x <= adam_ref.gpu_bound(name), f"replay {k}: {name} off by {x:.1f} units (bound {adam_ref.gpu_bound(name)})"
        for t, name in zip(after, ("flat", "exp_avg", "exp_avg_sq")):
            assert not t[pad].any(), f"replay {k}: alignment padding of {name} is not zero"
            assert bool(torch.isfinite(t).all())
        assert not torch.equal(after[0][:lo], before[0][:lo]) and not torch.equal(after[0][lo:], before[0][lo:]), \
            f"replay {k}: one side of the rider's start did not move"
    assert step.replays == 5 and step.fallbacks == 0
