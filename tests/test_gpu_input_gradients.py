"""Input-feature gradients on the engine: the ragged-width product kernel (csrc/input_grad.hip, fn_linear_dx_f32), the second C call of
a backward pass (fn_encoder_backward_inputs), ops.linear128's input gradient at K != 128, and the attributions built on them
(fragnet_amd/gradient_attribution.py).

Expected values: float64 torch for the product; for the engine the reference's own gat2.py / gat2_lite.py run on the CPU
(tests/golden/input_grad_b6.npz, input_grad_lite_b6.npz, ig_b6.npz, written by tests/golden/make_golden_inputgrad.py).

Tolerance.  An untrained model's input gradients are small (max 1.3e-3 on x_atoms, 4e-5 on the two bond tables in the fixtures): the
project's 1e-4 + 1e-4 |ref| would accept a table of zeros.  Every gradient or attribution table is therefore held to
    |got - ref| <= 1e-4 max|ref| + 1e-4 |ref|
(tests/inputgrad_common.py; the reference's own fp32-vs-float64 deviation is 3e-7 .. 8e-7 of the maximum, and an all-zero table fails --
both asserted in tests/test_input_gradients_host.py).  Logits and predictions keep the plain 1e-4 + 1e-4 |ref|.
Two per-molecule scalars of integrated gradients are remainders, not tables of their own scale, and are held to the scale of what
they are remainders OF: ``gap`` = pred - pred_baseline - sum(attr) - attr_other to 1e-4 max|pred - pred_baseline| + 1e-4 |ref| (the
attributions sum to pred - pred_baseline: that difference is their scale; the fixture's gaps are 40 x that bound, so zeros fail);
``attr_other`` is a row of the fragment-bond table and is held to that table's bound."""
import os

import numpy as np
import pytest
import torch

from tests import inputgrad_common as ic
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _z(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _plain(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    print(f"{what}: max|diff| = {err.max():.3e}")
    assert got.shape == ref.shape and (err <= ic.ATOL + ic.ATOL * np.abs(ref)).all(), f"{what}: max|diff| {err.max():.3e}"


# =============================================================================== 1. the product against float64 torch
SENTINEL = 12345.0
PAD = 96


def _case(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, 128, generator=g), torch.randn(128, K, generator=g) * 0.2, torch.randn(M, K, generator=g))


def _expect(g, W, delta):
    dx = g.double() @ W.double()
    return dx.numpy(), (dx * delta.double()).sum(1).numpy()


def _run(cases, modes):
    """One launch of the tasks ``cases`` [(g, W, delta)], task i writing ``modes[i]`` in {"dx", "dots", "both"}; the outputs are
    over-allocated and checked behind their ends.  Returns [(dx or None, dots or None)] on the host."""
    from fragnet_amd import ops
    tasks, outs = [], []
    for (g, W, delta), mode in zip(cases, modes):
        M, K = g.shape[0], W.shape[1]
        dx = torch.full((M * K + PAD,), SENTINEL, device=DEV) if mode in ("dx", "both") else None
        dots = torch.full((M + PAD,), SENTINEL, device=DEV) if mode in ("dots", "both") else None
        tasks.append((g.to(DEV), W.to(DEV), dx, delta.to(DEV) if dots is not None else None, dots))
        outs.append((dx, dots, M, K))
    ops.linear_dx(tasks)
    torch.cuda.synchronize()
    res = []
    for dx, dots, M, K in outs:
        if dx is not None:
            assert bool((dx[M * K:] == SENTINEL).all()), "dx: written past M * K elements"
        if dots is not None:
            assert bool((dots[M:] == SENTINEL).all()), "dots: written past M elements"
        res.append((None if dx is None else dx[:M * K].reshape(M, K).cpu().numpy(), None if dots is None else dots[:M].cpu().numpy()))
    return res


MS = (0, 1, 15, 16, 17, 65, 257)
KS = (1, 3, 4, 6, 17, 127, 128, 167, 168)


@pytest.mark.parametrize("K", KS)
def test_product_one_task_matches_float64(K):
    for M in MS:
        case = _case(M, K, 1000 * K + M)
        ref_dx, ref_dots = _expect(*case)
        for mode in ("dx", "dots", "both"):
            (dx, dots), = _run([case], [mode])
            if dx is not None:
                ic.assert_within(dx, ref_dx, f"dx M={M} K={K} ({mode})")
            if dots is not None:
                ic.assert_within(dots, ref_dots, f"dots M={M} K={K} ({mode})")


@pytest.mark.parametrize("shapes,modes", [(((257, 167), (65, 17), (17, 6)), ("both", "dots", "dx")),
                                          (((16, 168), (0, 17), (1, 1)), ("dx", "both", "both")),
                                          (((15, 3), (257, 128), (65, 127)), ("dots", "dx", "both")),
                                          (((17, 4), (1, 167), (15, 168)), ("both", "both", "both"))])
def test_product_three_tasks_in_one_launch(shapes, modes):
    cases = [_case(M, K, 7 * M + K) for M, K in shapes]
    res = _run(cases, modes)
    for (M, K), case, (dx, dots), mode in zip(shapes, cases, res, modes):
        ref_dx, ref_dots = _expect(*case)
        if dx is not None:
            ic.assert_within(dx, ref_dx, f"dx M={M} K={K} (three tasks, {mode})")
        if dots is not None:
            ic.assert_within(dots, ref_dots, f"dots M={M} K={K} (three tasks, {mode})")
    # a task of a three-task launch computes what it computes alone, bit for bit (nothing depends on the grid)
    for case, (dx, dots), mode in zip(cases, res, modes):
        (dx1, dots1), = _run([case], [mode])
        assert (dx is None or np.array_equal(dx, dx1)) and (dots is None or np.array_equal(dots, dots1))


def test_product_refuses_k_169_and_bad_arguments():
    from fragnet_amd import _lib, ops
    g, W, delta = (t.to(DEV) for t in _case(5, 169, 1))
    dx = torch.full((5 * 169,), SENTINEL, device=DEV)
    with pytest.raises(_lib.FragnetHipError, match=r"\[1, 168\]"):
        ops.linear_dx([(g, W, dx, None, None)])
    torch.cuda.synchronize()
    assert bool((dx == SENTINEL).all())
    g, W, delta = (t.to(DEV) for t in _case(5, 17, 2))
    with pytest.raises(ValueError):
        ops.linear_dx([(g, W, None, None, torch.empty(5, device=DEV))])                 # dots without delta
    with pytest.raises(ValueError):
        ops.linear_dx([(g, W, torch.empty(5 * 17 - 1, device=DEV), None, None)])        # dx too small
    with pytest.raises(ValueError):
        ops.linear_dx([(g, W, None, None, None)] * 4)                                   # four tasks
    with pytest.raises(_lib.FragnetHipError):
        ops.linear_dx([(g.cpu(), W, None, None, None)])                                 # no CPU fallback


# =============================================================================== 2. reproducibility
def test_product_is_bit_reproducible():
    cases = [_case(257, 167, 11), _case(65, 17, 12), _case(17, 6, 13)]
    a = _run(cases, ("both",) * 3)
    b = _run(cases, ("both",) * 3)
    for (dx_a, dots_a), (dx_b, dots_b) in zip(a, b):
        assert np.array_equal(dx_a, dx_b) and np.array_equal(dots_a, dots_b)


# =============================================================================== 3. the engine against the goldens
def _model(lite=False, train=False, drop=0.0):
    from fragnet_amd import model as M
    torch.manual_seed(ic.SEED)
    net = (M.FragNetFineTuneLite if lite else M.FragNetFineTune)(**dict(ic.CTOR, drop_ratio=drop))
    return net.to(DEV).train(train)


def _batch(need=(True, True, True)):
    from fragnet_amd import data
    batch = data.batch_to(data.collate_fn(ic.molecules()), DEV)
    for key, n in zip(ic.TABLE_KEYS, need):
        batch[key] = batch[key].detach().clone().requires_grad_(n)
    return batch


def _grads(net, batch):
    """(logits, the three input gradients, the parameter gradients) of out[:, 0].sum()."""
    net.zero_grad(set_to_none=True)
    out = net(batch)
    out[:, 0].sum().backward()
    torch.cuda.synchronize()
    return (out.detach().cpu().numpy(), [batch[k].grad for k in ic.TABLE_KEYS],
            {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})


@pytest.fixture(scope="module")
def engine_run():
    """One evaluation forward + backward of the gat2 model on the fixture batch, shared by the tests that only read it."""
    net = _model()
    logits, grads, pgrads = _grads(net, _batch())
    return logits, [None if g is None else g.cpu().numpy() for g in grads], pgrads


def test_engine_gradients_match_the_reference(engine_run):
    z = _z("input_grad_b6")
    logits, grads, _ = engine_run
    assert grads[0] is not None, "x_atoms.grad is None: the engine returned no input gradient"
    _plain(logits, z["logits"], "logits")
    for key, g in zip(ic.TABLE_KEYS, grads):
        assert g is not None, f"{key}: no gradient"
        ic.assert_within(g, z[f"grad/{key}"], f"d out / d {key} (gat2)")


def test_engine_gradients_match_the_reference_lite():
    z = _z("input_grad_lite_b6")
    logits, grads, _ = _grads(_model(lite=True), _batch())
    _plain(logits, z["logits"], "logits (gat2_lite)")
    assert grads[2] is None                                   # gat2_lite never reads the fragment-bond nodes
    for key, g in zip(ic.TABLE_KEYS[:2], grads[:2]):
        assert g is not None, f"{key}: no gradient"
        ic.assert_within(g.cpu().numpy(), z[f"grad/{key}"], f"d out / d {key} (gat2_lite)")


# =============================================================================== 4. nothing else moves
def test_parameter_gradients_and_logits_do_not_move(engine_run):
    logits, _, pgrads = engine_run
    net = _model()
    logits0, grads0, pgrads0 = _grads(net, _batch(need=(False, False, False)))
    assert all(g is None for g in grads0)
    assert np.array_equal(logits, logits0)
    assert set(pgrads) == set(pgrads0) and len(pgrads) > 10
    for name in pgrads:
        assert torch.equal(pgrads[name], pgrads0[name]), name
    # one input alone: the same gradient, bit for bit, and None for the others
    _, only_bonds, _ = _grads(net, _batch(need=(False, True, False)))
    assert only_bonds[0] is None and only_bonds[2] is None
    assert np.array_equal(only_bonds[1].cpu().numpy(), engine_run[1][1])


# =============================================================================== 5. second witness: the per-level path
def test_engine_matches_the_per_level_path(engine_run):
    net = _model()
    net.pretrain.use_engine = False
    logits, grads, _ = _grads(net, _batch())
    _plain(engine_run[0], logits, "logits, engine vs per-level path")
    for key, got, ref in zip(ic.TABLE_KEYS, engine_run[1], grads):
        assert ref is not None, f"{key}: the per-level path returned no gradient"
        ic.assert_within(got, ref.cpu().numpy(), f"d out / d {key}, engine vs per-level path")


# =============================================================================== 6. ops.linear128 at K = 167
@pytest.mark.parametrize("M,K", [(513, 167), (65, 17), (17, 6)])
def test_linear128_input_gradient_ragged_k(M, K):
    from fragnet_amd import ops
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(128, K, generator=g) * 0.2).to(DEV).requires_grad_(True)
    b = torch.randn(128, generator=g).to(DEV).requires_grad_(True)
    gy = torch.randn(M, 128, generator=g).to(DEV)
    ops.linear128(x, w, b).backward(gy)
    x2, w2, b2 = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
    torch.nn.functional.linear(x2, w2, b2).backward(gy.double().cpu())
    ic.assert_within(x.grad.cpu().numpy(), x2.grad.numpy(), f"linear128 input gradient K={K}")
    ic.assert_within(w.grad.cpu().numpy(), w2.grad.numpy(), f"linear128 weight gradient K={K}")


# =============================================================================== 7. the attributions against ig_b6.npz
def _flat(z, kind):
    return np.concatenate([z[f"m{i}/{kind}"] for i in range(6)])


def _check_tables(res, ref_tables, what):
    for kind in ("atom", "bond", "fbond"):
        ic.assert_within(res.tables[kind]["attr"], ref_tables[kind], f"{what}: {kind} attributions")


def test_input_gradients_attribution(engine_run):
    from fragnet_amd import gradient_attribution as ga
    z = _z("input_grad_b6")
    mols = ic.molecules()
    res = ga.input_gradients(_model(), mols, return_gradients=True)
    _plain(res.pred, z["logits"][:, 0], "input_gradients: pred")
    from fragnet_amd import data
    batch = data.collate_fn(mols)
    rows = [(z[f"grad64/{k}"] * batch[k].double().numpy()).sum(1) for k in ic.TABLE_KEYS]            # gradient x input per row, float64
    per_mol = ic.entry_sums(*[r.astype(np.float32) for r in rows], z["n_atoms"], z["n_bonds"], z["n_fbonds"])
    ref = {kind: np.concatenate([m[j] for m in per_mol]) for j, kind in enumerate(("atom", "bond", "fbond"))}
    _check_tables(res, ref, "gradient x input")
    scale_fb = np.concatenate([ref["fbond"], [m[3] for m in per_mol]])
    other = np.asarray([m[3] for m in per_mol])
    assert (np.abs(res.attr_other - other) <= 1e-4 * np.abs(scale_fb).max() + 1e-4 * np.abs(other)).all()
    for key, g in zip(ic.TABLE_KEYS, res.gradients):
        ic.assert_within(g, z[f"grad/{key}"], f"input_gradients: raw gradient of {key}")
    # the index columns are leave-one-out's
    from fragnet_amd import attribution as attr
    table = attr.replica_table(z["n_atoms"], z["n_bonds"], z["n_fbonds"])
    for kind, code in (("atom", attr.KIND_ATOM), ("bond", attr.KIND_BOND), ("fbond", attr.KIND_FBOND)):
        np.testing.assert_array_equal(res.tables[kind]["index"], np.concatenate([t[t[:, 0] == code, 1] for t in table]))
    # without the tables in memory: the same scores, bit for bit
    res2 = ga.input_gradients(_model(), mols)
    assert res2.gradients is None
    for kind in ("atom", "bond", "fbond"):
        assert np.array_equal(res2.tables[kind]["attr"], res.tables[kind]["attr"])


@pytest.fixture(scope="module")
def ig_run():
    from fragnet_amd import gradient_attribution as ga
    return ga.integrated_gradients(_model(), ic.molecules(), steps=int(_z("ig_b6")["steps"]))


def _check_ig(res, z, what):
    _plain(res.pred, z["pred"], f"{what}: pred")
    _plain(res.pred_baseline, z["pred_baseline"], f"{what}: pred_baseline")
    _check_tables(res, {k: _flat(z, k) for k in ("atom", "bond", "fbond")}, what)
    scale_fb = np.abs(np.concatenate([_flat(z, "fbond"), z["attr_other"]])).max()
    err = np.abs(res.attr_other.astype(np.float64) - z["attr_other"])
    print(f"{what}: attr_other max|diff| = {err.max():.3e}, bound scale {scale_fb:.3e}")
    assert (err <= 1e-4 * scale_fb + 1e-4 * np.abs(z["attr_other"])).all()
    scale = np.abs(z["pred"].astype(np.float64) - z["pred_baseline"]).max()
    err = np.abs(res.gap.astype(np.float64) - z["gap"])
    print(f"{what}: gap max|diff| = {err.max():.3e}, max|gap| = {np.abs(z['gap']).max():.3e}, bound scale max|pred - pred_baseline| = {scale:.3e}")
    assert (np.abs(z["gap"]) > 1e-4 * scale + 1e-4 * np.abs(z["gap"])).any()               # zeros would fail
    assert (err <= 1e-4 * scale + 1e-4 * np.abs(z["gap"])).all(), f"{what}: gap off by {err.max():.3e}"
    assert res.steps == int(z["steps"]) and res.method == "ig"


def test_integrated_gradients(ig_run):
    _check_ig(ig_run, _z("ig_b6"), "integrated gradients")
    # completeness as the result reports it: gap is the identity's remainder of the returned numbers
    from fragnet_amd import gradient_attribution as ga
    np.testing.assert_array_equal(ig_run.gap, ga.completeness_gap(ig_run.pred, ig_run.pred_baseline, ig_run.tables, ig_run.attr_other))


def test_integrated_gradients_chunked(ig_run):
    """max_rows = 1000: the 41-atom molecule (123 rows a replica) takes 8 of its 32 steps per chunk."""
    from fragnet_amd import gradient_attribution as ga
    z = _z("ig_b6")
    lens = {"atom": z["n_atoms"], "edge": z["n_bonds"]}
    chunks = ga.ig_plan(lens, int(z["steps"]), 1000)
    assert any(sum(1 for c in chunks if any(i == m for i, _, _ in c)) >= 2 for m in range(6))          # a molecule's steps span chunks
    res = ga.integrated_gradients(_model(), ic.molecules(), steps=int(z["steps"]), max_rows=1000)
    _check_ig(res, z, "integrated gradients, chunked")
    same = all(np.array_equal(res.tables[k]["attr"], ig_run.tables[k]["attr"]) for k in ("atom", "bond", "fbond"))
    print(f"chunked and unchunked attributions bit-identical: {same}")


def test_integrated_gradients_baseline_vectors(ig_run):
    """Three zero row vectors (an array, a tensor, a list) are the default baseline, bit for bit; a wrong width and a target column the
    model does not have are refused."""
    from fragnet_amd import gradient_attribution as ga
    steps = int(_z("ig_b6")["steps"])
    res = ga.integrated_gradients(_model(), ic.molecules(), steps=steps, baseline=(np.zeros(167), torch.zeros(17), [0.0] * 6))
    for k in ("atom", "bond", "fbond"):
        assert np.array_equal(res.tables[k]["attr"], ig_run.tables[k]["attr"])
    with pytest.raises(ValueError):
        ga.integrated_gradients(_model(), ic.molecules(), steps=steps, baseline=(np.zeros(166), np.zeros(17), np.zeros(6)))
    with pytest.raises(IndexError):
        ga.integrated_gradients(_model(), ic.molecules(), steps=2, target=1)


# =============================================================================== 8. refusals
def test_training_pass_with_dropout_is_refused_and_without_it_works():
    z = _z("input_grad_b6")
    net = _model(train=True, drop=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        net(_batch(need=(True, False, False)))
    net(_batch(need=(False, False, False)))                   # the same pass without an input that requires a gradient runs
    # a training pass at drop_ratio = 0 (the one-pass backward): the golden's gradients
    logits, grads, _ = _grads(_model(train=True), _batch())
    _plain(logits, z["logits"], "logits (training pass, p = 0)")
    for key, g in zip(ic.TABLE_KEYS, grads):
        assert g is not None
        ic.assert_within(g.cpu().numpy(), z[f"grad/{key}"], f"d out / d {key} (training pass, p = 0)")


def test_gat2_edge_is_refused():
    from fragnet_amd import model as M
    torch.manual_seed(0)
    net = M.FragNetFineTuneEdge(**ic.CTOR).to(DEV).eval()
    from fragnet_amd import data, synth
    mols = synth.synth_molecules(2, seed=3, profile="esol")
    batch = data.batch_to(data.collate_fn(mols), DEV)
    batch["x_atoms"] = batch["x_atoms"].detach().clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="gat2_edge"):
        net(batch)
