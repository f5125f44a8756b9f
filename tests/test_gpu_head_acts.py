"""The prediction heads' activation kinds on the hand-written kernels (include/fragnet_hip.h fn_head_act, csrc/head_act.inc):
the kernels against float64 torch under the masks of fn_dropout_act_f32, FTHead1/3/4 against the oracle and the reference's
golden vectors, the path the heads take, and the captured training step."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import check_grads

gpu = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 1e-4
KINDS = ["relu", "silu", "gelu", "celu", "selu", "relu6", "leakyrelu", "prelu"]
ACTS = ["silu", "gelu", "celu", "selu", "relu6", "leakyrelu", "prelu"]
SLOPE = 0.23
_KEEP_CHECKED = []


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from fragnet_amd.build import build_lib
    build_lib()
    return torch.device(DEV)


def _f(kind):
    fn = {"relu": F.relu, "silu": F.silu, "gelu": F.gelu, "celu": F.celu, "selu": F.selu, "relu6": F.relu6,
          "leakyrelu": F.leaky_relu}
    return fn.get(kind, lambda u: F.prelu(u, torch.tensor([SLOPE], dtype=u.dtype, device=u.device)))


def _df(kind, u):
    """torch's own f'(u) (its convention at the kinks), in float64"""
    u = u.detach().double().requires_grad_(True)
    _f(kind)(u).sum().backward()
    return u.grad


def _keep(shape, p, seed, offset, dev):
    """mask / (1 - p) of the Philox stream, through the standalone kernel"""
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    ones, k = torch.ones(shape, device=dev), torch.empty(shape, device=dev)
    if ones.numel():
        _lib.call("fn_dropout_act_f32", ones.data_ptr(), k.data_ptr(), ones.numel(), float(p), seed, offset, None, 0, _stream_ptr(dev))
        if p > 0.0 and not _KEEP_CHECKED:
            # once per session: the kernel's mask IS the documented stream (tests/philox_ref.py), not just what every kernel agrees on
            from tests import philox_ref
            want = torch.from_numpy(philox_ref.mask(ones.numel(), p, seed, offset)).view(k.shape)
            assert torch.equal(k.cpu() != 0, want)
            _KEEP_CHECKED.append(True)
    return k.double()


@gpu
@pytest.mark.parametrize("M", [1, 37, 512, 2048])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("order", [0, 1], ids=["act_of_dropout", "dropout_of_act"])
@pytest.mark.parametrize("kind", KINDS)
def test_head_act_kernels_match_float64(kind, order, p, M):
    """One hidden layer through fn_dense_fwd_act_f32 (M = 2048 runs the workgroup-shared-tile forward), then the layer above's
    backward through fn_dense_bwd_act_f32 / fn_small_linear_bwd_act_f32 / fn_small_linear_loss_act_f32 with it as `below`:
    outputs, the saved argument, g_x through the activation, dW, db, zero padding rows, and the PReLU slope's gradient."""
    _check_head_act_kernels(kind, order, p, M, 3)


@gpu
@pytest.mark.parametrize("Cc", [1, 3, 5])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("order", [0, 1], ids=["act_of_dropout", "dropout_of_act"])
@pytest.mark.parametrize("kind", ["silu", "prelu"])
def test_head_act_last_linear_class_widths(kind, order, p, Cc):
    """The same checks with 1, 3 and 5 outputs of the last Linear: the three class widths (1, 4, FN_SMALL_LINEAR_MAX) of
    k_small_linear_bwd / k_small_linear_loss with an activation below (the test above runs three outputs, the middle width, only)."""
    _check_head_act_kernels(kind, order, p, 37, Cc)


def _check_head_act_kernels(kind, order, p, M, Cc):
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    dev = _dev()
    st = _stream_ptr(dev)
    lib = _lib.load()
    K, N, N2 = 256, (1024 if M == 2048 else 128), 64
    torch.manual_seed(M * 31 + KINDS.index(kind) * 7 + order + int(p * 4))
    x, w, b = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5, torch.randn(N, device=dev) * 0.5
    slope = torch.tensor([SLOPE], device=dev)
    seed, off = 1234 + M, 77
    off_dev = torch.tensor([5], dtype=torch.int64, device=dev)
    y, pre = torch.full((M, N), 7.0, device=dev), torch.full((M, N), 7.0, device=dev)
    kid = KINDS.index(kind)
    spec = _lib.HeadAct(kid, order, p, 0, seed, off, off_dev.data_ptr(), slope.data_ptr(), pre.data_ptr(), None)
    _lib.call("fn_dense_fwd_act_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, C.byref(spec), st)
    z = x.double() @ w.double().t() + b.double()
    keep = _keep((M, N), p, seed, off + 5, dev)
    u = z * keep if order == 0 else z
    want = _f(kind)(u) if order == 0 else _f(kind)(u) * keep
    torch.testing.assert_close(pre.double(), u, atol=3e-5, rtol=1e-5)
    torch.testing.assert_close(y.double(), want, atol=5e-5, rtol=1e-4)

    # the layer above: g_x through this layer's activation, with padding rows behind M
    uk = pre.double()
    dfk = _df(kind, uk)

    def through(v):                                   # d loss / d z for d loss / d y = v, and the slope's gradient
        gf = v * keep if order == 1 else v
        dslope = torch.where(uk > 0, torch.zeros_like(uk), uk * gf).sum()
        return keep * dfk * v, dslope

    def check_slope(parts, want_slope, terms):
        if kind != "prelu":
            return
        n = parts.numel()
        g = torch.full((1,), 7.0, device=dev)
        _lib.call("fn_head_act_param_grad_f32", parts.data_ptr(), n, g.data_ptr(), st)
        torch.testing.assert_close(g.double()[0], want_slope, atol=1e-4 + 1e-5 * float(terms), rtol=1e-5)

    g_y, w2, b2 = torch.randn(M, N2, device=dev), torch.randn(N2, N, device=dev) / N ** 0.5, torch.randn(N2, device=dev)
    parts = torch.full((lib.fn_head_act_parts(_lib.ACT_AT_DENSE_BWD, M + 8, N),), 7.0, device=dev)
    spec.part = parts.data_ptr()
    gx, dW, db = torch.full((M + 8, N), 7.0, device=dev), torch.full_like(w2, 7.0), torch.full_like(b2, 7.0)
    _lib.call("fn_dense_bwd_act_f32", g_y.data_ptr(), y.data_ptr(), w2.data_ptr(), gx.data_ptr(), C.byref(spec), dW.data_ptr(),
                     db.data_ptr(), M, N, N2, M + 8, None, st)
    v = g_y.double() @ w2.double()
    want_gx, want_slope = through(v)
    torch.testing.assert_close(gx[:M].double(), want_gx, atol=5e-5, rtol=1e-4)
    assert not gx[M:].any()
    tol = 2e-4 * max(1.0, M / 500) ** 0.5
    torch.testing.assert_close(dW.double(), g_y.double().t() @ y.double(), atol=tol, rtol=1e-4)
    torch.testing.assert_close(db.double(), g_y.double().sum(0), atol=tol, rtol=1e-5)
    check_slope(parts, want_slope, (uk.abs() * v.abs()).sum())

    # the last Linear's backward (C <= 16 outputs) with the same activation below
    g3, w3 = torch.randn(M, Cc, device=dev), torch.randn(Cc, N, device=dev) / N ** 0.5
    parts = torch.full((lib.fn_head_act_parts(_lib.ACT_AT_SMALL_BWD, M, N),), 7.0, device=dev)
    spec.part = parts.data_ptr()
    gx3, dW3, db3 = torch.full((M, N), 7.0, device=dev), torch.empty_like(w3), torch.empty(Cc, device=dev)
    n_ws = lib.fn_small_linear_bwd_ws(M, N, Cc)
    ws = torch.empty(max(n_ws, 1), device=dev)
    _lib.call("fn_small_linear_bwd_act_f32", g3.data_ptr(), y.data_ptr(), w3.data_ptr(), gx3.data_ptr(), dW3.data_ptr(), db3.data_ptr(),
                     M, N, Cc, C.byref(spec), ws.data_ptr(), st)
    v3 = g3.double() @ w3.double()
    want_gx3, want_slope3 = through(v3)
    torch.testing.assert_close(gx3.double(), want_gx3, atol=5e-5, rtol=1e-4)
    torch.testing.assert_close(dW3.double(), g3.double().t() @ y.double(), atol=tol, rtol=1e-4)
    check_slope(parts, want_slope3, (uk.abs() * v3.abs()).sum())

    # the fused last Linear + loss: its g_x through the activation equals the ungated launch's g_x through it
    tgt, row_w = torch.randn(M, Cc, device=dev), torch.ones(M, device=dev)
    outs = []
    for act in (None, spec):
        yo, go, gxo = torch.empty(M, Cc, device=dev), torch.empty(M, Cc, device=dev), torch.full((M, N), 7.0, device=dev)
        lp = torch.empty(lib.fn_small_linear_loss_ws(M), device=dev)
        if act is None:
            _lib.call("fn_small_linear_loss_f32", y.data_ptr(), w3.data_ptr(), None, tgt.data_ptr(), row_w.data_ptr(), _lib.LOSS_MSE,
                           yo.data_ptr(), go.data_ptr(), gxo.data_ptr(), 0.0, lp.data_ptr(), M, N, Cc, M, st)
        else:
            parts = torch.full((lib.fn_head_act_parts(_lib.ACT_AT_SMALL_LOSS, M, N),), 7.0, device=dev)
            spec.part = parts.data_ptr()
            _lib.call("fn_small_linear_loss_act_f32", y.data_ptr(), w3.data_ptr(), None, tgt.data_ptr(), row_w.data_ptr(), _lib.LOSS_MSE,
                           yo.data_ptr(), go.data_ptr(), gxo.data_ptr(), C.byref(act), lp.data_ptr(), M, N, Cc, M, st)
        outs.append((yo, go, gxo))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want_gx4, want_slope4 = through(outs[0][2].double())
    torch.testing.assert_close(outs[1][2].double(), want_gx4, atol=2e-6, rtol=1e-5)
    check_slope(parts, want_slope4, (uk.abs() * outs[0][2].double().abs()).sum())


# ------------------------------------------------------------------------------------------------ modules vs the oracle
MODULE_CASES = [("FTHead3", a) for a in ACTS] + [("FTHead4", a) for a in ACTS] + [("FTHead1", "relu"), ("FTHead4", "relu")]
CFG = dict(n_classes=1, num_layer=2, drop_ratio=0.0, h1=64, h2=128, h3=128, h4=64, num_heads=4)


def _pair(fthead, act, n_classes=1, seed=3):
    from fragnet_amd.model import FragNetFineTune
    from oracle import fragnet_ref as ref
    cfg = dict(CFG, fthead=fthead, act=act, n_classes=n_classes)
    torch.manual_seed(seed)
    gold = ref.FragNetFineTune(**cfg)
    torch.manual_seed(seed)
    model = FragNetFineTune(**cfg).to(DEV)
    return gold, model


@gpu
@pytest.mark.parametrize("fthead,act", MODULE_CASES)
def test_head_matches_oracle(fthead, act):
    from fragnet_amd import data, synth
    _dev()
    gold, model = _pair(fthead, act)
    gold.fthead.dropout.p = model.fthead.dropout.p = 0.0      # FTHead1 keeps its own p = 0.2 whatever drop_ratio says
    batch = data.collate_fn(synth.synth_molecules(24, seed=808, profile="esol"))
    gold.train()
    model.train()
    want = gold(batch)
    torch.nn.functional.mse_loss(want.view(-1), batch["y"]).backward()
    b = data.batch_to(batch, DEV)
    got = model(b)
    torch.nn.functional.mse_loss(got.view(-1), b["y"]).backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(got.detach().cpu(), want.detach(), atol=ATOL, rtol=1e-4)
    full = {n: p.grad.numpy() for n, p in gold.named_parameters() if p.grad is not None}
    if act == "prelu":
        assert "fthead.activation.weight" in full
    check_grads(model, {"full": full, "samp": {}, "sum": dict.fromkeys(full)}, atol=ATOL, rtol=1e-4)


@gpu
@pytest.mark.parametrize("fthead,act", MODULE_CASES + [("FTHead3", "rrelu")])
def test_head_runs_without_torch_linear_or_dropout(fthead, act, monkeypatch):
    """Called directly on a pooled encoding, in training mode with dropout: no torch Linear and no torch dropout -- except rrelu,
    which keeps torch's path (its training slopes come from torch's generator)."""
    from fragnet_amd.model import FragNetFineTune
    _dev()
    torch.manual_seed(0)
    model = FragNetFineTune(**dict(CFG, fthead=fthead, act=act, drop_ratio=0.2)).to(DEV).train()
    head = model.fthead
    enc = torch.randn(40, 256, device=DEV, requires_grad=True)

    def refuse(*a, **k):
        raise AssertionError("torch op on the head's path")
    monkeypatch.setattr(torch.nn.functional, "linear", refuse)
    monkeypatch.setattr(torch.nn.functional, "dropout", refuse)
    if act == "rrelu":
        with pytest.raises(AssertionError, match="torch op"):
            head(enc)
        return
    out = head(enc)
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert enc.grad is not None and torch.isfinite(enc.grad).all()
    for n, p in head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    out2 = head(enc)
    assert not torch.equal(out, out2)                     # the masks come from the moving Philox stream


# ------------------------------------------------------------------------------------------------ reference goldens
@gpu
@pytest.mark.parametrize("use_engine", [True, False], ids=["engine", "per_level_ops"])
@pytest.mark.parametrize("case", ["ft_head3_celu_b4", "ft_head3_selu_b4", "ft_head4_prelu_b4", "ft_head4_gelu_b4"])
def test_head_activation_matches_reference_golden(case, use_engine):
    from tests.helpers import load_case
    from fragnet_amd.model import FragNetFineTune
    from fragnet_amd.data import batch_to
    _dev()
    cfg, batch, out, grads, _, _ = load_case(case)
    torch.manual_seed(cfg["seed"])
    model = FragNetFineTune(**cfg["ctor"]).to(DEV)
    model.pretrain.use_engine = use_engine
    model.train()
    b = batch_to(batch, DEV)
    logits = model(b)
    torch.testing.assert_close(logits.detach().cpu(), torch.from_numpy(out["logits"]), atol=ATOL, rtol=1e-4)
    loss = torch.nn.functional.mse_loss(logits.view(-1), b["y"])
    assert abs(loss.item() - float(out["loss"])) < ATOL
    loss.backward()
    torch.cuda.synchronize()
    if cfg["ctor"]["act"] == "prelu":
        assert "fthead.activation.weight" in grads["sum"]
    check_grads(model, grads, atol=ATOL, rtol=1e-4)


@gpu
def test_tox21_b1024_fthead4_gelu_matches_oracle_on_a_slice():
    """BASELINE config 2's shape (Tox21, 12 tasks, FTHead4, B = 1024) with a non-ReLU activation: the first 32 molecules' logits
    equal the oracle's on those molecules alone, and the training step is bitwise reproducible."""
    from fragnet_amd import data, synth, train
    from fragnet_amd.model import FragNetFineTune
    from oracle import fragnet_ref as ref
    _dev()
    cfg = dict(n_classes=12, num_layer=4, drop_ratio=0.0, h1=128, act="gelu", fthead="FTHead4")
    mols = synth.synth_molecules(1024, seed=2000, profile="tox21")
    batch = data.collate_fn(mols)
    torch.manual_seed(0)
    model = FragNetFineTune(**cfg).to(DEV)
    b = data.batch_to(batch, DEV)
    with torch.no_grad():
        full = model.eval()(b).cpu()
    torch.manual_seed(0)
    gold = ref.FragNetFineTune(**cfg).eval()
    with torch.no_grad():
        want = gold(data.collate_fn(mols[:32]))
    torch.testing.assert_close(full[:32], want, atol=ATOL, rtol=1e-4)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        m = FragNetFineTune(**dict(cfg, drop_ratio=0.1)).to(DEV).train()
        bb = data.batch_to(batch, DEV)
        loss = train.compute_bce_loss(m(bb), bb["y"])
        loss.backward()
        runs.append((loss.item(), m.fthead.dense.weight.grad.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------ the captured training step
GRAPH_CFG = dict(n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=2, num_heads=4,
                 h1=64, h2=64, h3=64, h4=64, emb_dim=128)
GRAPH_CASES = [("FTHead3", "selu"), ("FTHead4", "prelu")]


def _graph_setup(fthead, act, drop, lr, seed=21, n=4):
    from fragnet_amd import data, graphstep, parallel, synth
    from fragnet_amd.model import FragNetFineTune
    batches = [data.batch_to(data.collate_fn(synth.synth_molecules(48, seed=seed + i, profile="esol")), DEV) for i in range(n)]
    shapes = graphstep.StaticShapes.from_batches(batches, margin=0.05)
    torch.manual_seed(11)
    model = FragNetFineTune(**dict(GRAPH_CFG, fthead=fthead, act=act, drop_ratio=drop)).to(DEV).train()

    def optim(m):
        probe = lambda: torch.nn.functional.mse_loss(m(dict(batches[0])).view(-1), batches[0]["y"]).backward()   # noqa: E731
        return parallel.FlatAdam.for_live_parameters(m, probe, lr=lr, eps=1e-4)
    return batches, shapes, model, optim, graphstep


@gpu
@pytest.mark.parametrize("fthead,act", GRAPH_CASES)
def test_graph_step_matches_eager_steps(fthead, act):
    _dev()
    batches, shapes, model_a, optim, graphstep = _graph_setup(fthead, act, 0.0, 1e-3)
    model_b = copy.deepcopy(model_a)
    opt_a, opt_b = optim(model_a), optim(model_b)
    step_b = graphstep.GraphedTrainStep(model_b, opt_b, shapes, dict(batches[0]), loss="regr")
    torch.testing.assert_close(opt_b.flat, opt_a.flat, atol=0, rtol=0)
    w0 = model_b.fthead.activation.weight.detach().clone() if act == "prelu" else None
    for i in range(6):
        b = batches[i % 4]
        opt_a.zero_grad()
        loss_a = torch.nn.functional.mse_loss(model_a(dict(b)).view(-1), b["y"])
        loss_a.backward()
        opt_a.step()
        loss_b = step_b(dict(b)).clone()
        torch.testing.assert_close(loss_b, loss_a.detach(), atol=1e-5, rtol=1e-4)
    assert step_b.replays == 6 and step_b.fallbacks == 0
    torch.testing.assert_close(opt_b.flat, opt_a.flat, atol=2e-5, rtol=1e-3)
    if w0 is not None:                                     # the slope moved, and the replays above read the moved value
        assert not torch.equal(model_b.fthead.activation.weight.detach(), w0)
        torch.testing.assert_close(model_b.fthead.activation.weight, model_a.fthead.activation.weight, atol=2e-5, rtol=1e-3)


@gpu
@pytest.mark.parametrize("fthead,act", GRAPH_CASES)
def test_graph_step_with_dropout_is_reproducible_and_draws_fresh_masks(fthead, act):
    _dev()
    batches, shapes, model_a, optim, graphstep = _graph_setup(fthead, act, 0.1, 1e-3)
    model_b = copy.deepcopy(model_a)
    runs = []
    for m in (model_a, model_b):
        opt = optim(m)
        step = graphstep.GraphedTrainStep(m, opt, shapes, dict(batches[0]), loss="regr")
        w0 = m.fthead.activation.weight.detach().clone() if act == "prelu" else None
        losses = [step(dict(batches[i % 4])).clone() for i in range(6)]
        assert step.replays == 6 and step.fallbacks == 0
        if w0 is not None:
            assert not torch.equal(m.fthead.activation.weight.detach(), w0)
        runs.append((torch.stack(losses), opt.flat.detach().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # lr = 0: the same batch replayed gives other numbers only through fresh masks
    _, _, model_c, optim_c, _ = _graph_setup(fthead, act, 0.1, 0.0)
    opt_c = optim_c(model_c)
    step = graphstep.GraphedTrainStep(model_c, opt_c, shapes, dict(batches[0]), loss="regr")
    losses = [float(step(dict(batches[0]))) for _ in range(4)]
    assert len(set(losses)) == 4, losses
    assert step.fallbacks == 0
