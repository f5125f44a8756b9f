"""GPU checks of the factored pair path (csrc/pair_factored.hip, ops.pair_head_factored, the two pair models on factored batches).

The kernels are compared at the C ABI with float64 CPU torch of the DUPLICATED form, fc2(fc1(cat(D[pd], S[ps]))) and its autograd, at
tests/test_gpu_cdrp.py's ``_close`` (atol 2e-5 * max(1, max|want|), rtol 1e-5: the fp32 round-off of a differently ordered sum).  The
models are compared with the reference (tests/golden/*_pairs_u3c3.npz, written from a batch that repeats 3 drugs x 3 second inputs over 7
pairs, and the existing *_b5 fixtures through ``as_factored``) and with this repository's duplicated path, at the golden tests'
ATOL = 1e-4 / rtol 1e-4."""
import copy
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import GOLDEN, check_grads, check_params_match, load_case
from tests.test_gpu_cdrp import _close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
GENE_DIM = 903
SMALL = dict(n_classes=1, num_layer=2, num_heads=4, drop_ratio=0.0, h1=32, h2=64, h3=64, h4=32, act="relu", fthead="FTHead3")
INSTANCES = {"cdrp": ("fn_cdrp_pair_factored", 256, True), "dta": ("fn_dta_pair_factored", 300, False)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    _lib.load()


def _st():
    from fragnet_amd.plan import _stream_ptr
    return _stream_ptr(torch.device(DEV))


# ------------------------------------------------------------------------------- the kernels at the C ABI
# (M, U, C, referenced drugs, referenced second rows, identity lists)
CASES = [(1, 1, 1, 1, 1, False), (5, 5, 5, 5, 5, True), (17, 3, 2, 3, 2, False), (33, 1, 7, 1, 7, False), (300, 1, 1, 1, 1, False),
         (257, 33, 5, 33, 5, False), (64, 40, 64, 20, 30, False),
         (2048, 600, 900, 600, 900, False)]          # 38 + 57 forward workgroups: they run on every XCD, so the last one reads rows published across XCDs


def _lists(M, n_ref, identity, g):
    """a pair list over the rows [0, n_ref) in which every one of them occurs (M >= n_ref)"""
    if identity:
        return torch.arange(M)
    pl = torch.cat((torch.arange(n_ref), torch.randint(0, n_ref, (M - n_ref,), generator=g)))
    return pl[torch.randperm(M, generator=g)]


def _case(kind, M, U, C_, Uref, Cref, identity, seed):
    K1 = INSTANCES[kind][1]
    g = torch.Generator().manual_seed(seed)
    D = torch.randn(U, 256, generator=g)
    S = torch.randn(C_, K1, generator=g)
    if kind == "cdrp":
        S = torch.relu(S)                      # a ReLU output: exact zeros where the draw was negative
    S[:, 3] = 0.0                              # exact zeros and negatives in known places: gated to 0 for cdrp, plain gradients for dta
    S[:, 5] = -1.0
    S[0, 8:12] = 0.0
    fc1, fc2 = torch.nn.Linear(256 + K1, 128), torch.nn.Linear(128, 1)
    y = torch.randn(M, generator=g)
    return D, S, _lists(M, Uref, identity, g), _lists(M, Cref, identity, g), fc1, fc2, y


def _reference(kind, D, S, pd, ps, fc1, fc2, y):
    """float64, the duplicated form and its autograd; the gate of the cdrp instance applied to the second gradient"""
    r1, r2 = copy.deepcopy(fc1).double(), copy.deepcopy(fc2).double()
    d2, s2 = D.double().requires_grad_(True), S.double().requires_grad_(True)
    out = r2(r1(torch.cat((d2[pd], s2[ps]), 1)))
    loss = F.mse_loss(out.view(-1), y.double())
    loss.backward()
    g_S = s2.grad * (S > 0) if INSTANCES[kind][2] else s2.grad
    return dict(out=out.detach().view(-1), loss=loss.detach(), g_D=d2.grad, g_S=g_S, dW1=r1.weight.grad, db1=r1.bias.grad,
                dW2=r2.weight.grad, db2=r2.bias.grad, A=(D.double() @ r1.weight[:, :256].T).detach(),
                B=(S.double() @ r1.weight[:, 256:].T).detach())


PAD = 2          # rows allocated behind M, U and C: they must stay as they were


def _run_abi(kind, D, S, pd, ps, fc1, fc2, y):
    """forward (with the target) and backward (with the loss) at the C ABI; every output over-allocated by PAD rows filled with 7.0"""
    from fragnet_amd import _lib, ops
    prefix, K1, _ = INSTANCES[kind]
    (U, _), (C_, _), M = D.shape, S.shape, pd.numel()
    lib = _lib.load()
    t = [q.to(DEV).contiguous() for q in (D, S, pd, ps, fc1.weight.detach(), fc1.bias.detach(), fc2.weight.detach(), fc2.bias.detach(), y)]
    full = lambda *shape: torch.full(shape, 7.0, device=DEV)
    A, B, out, g = full(U + PAD, 128), full(C_ + PAD, 128), full(M + PAD), full(M + PAD)
    ws = torch.empty(getattr(lib, prefix + "_ws")(U, C_), device=DEV)
    part, loss = full(1), full(1)
    st = _st()
    _lib.call(prefix + "_fwd_f32", *[q.data_ptr() for q in t[:8]], t[8].data_ptr(), A.data_ptr(), B.data_ptr(), ws.data_ptr(), out.data_ptr(),
              g.data_ptr(), part.data_ptr(), M, U, C_, 256, K1, 128, 1, st)
    ords = ops.pair_orderings(t[2], U) + ops.pair_orderings(t[3], C_)
    grads = dict(g_D=full(U + PAD, 256), g_S=full(C_ + PAD, K1), dW1=full(128, 256 + K1), db1=full(128), dW2=full(1, 128), db2=full(1))
    _lib.call(prefix + "_bwd_f32", g.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), A.data_ptr(), B.data_ptr(), t[4].data_ptr(), t[5].data_ptr(),
              t[6].data_ptr(), *[o.data_ptr() for o in ords], *[q.data_ptr() for q in grads.values()], part.data_ptr(), 1, loss.data_ptr(),
              M, U, C_, 256, K1, 128, 1, st)
    torch.cuda.synchronize()
    return dict(out=out, g=g, A=A, B=B, loss=loss, **grads)


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("M,U,C_,Uref,Cref,identity", CASES)
def test_factored_kernels_match_float64_duplicated_form(kind, M, U, C_, Uref, Cref, identity):
    D, S, pd, ps, fc1, fc2, y = _case(kind, M, U, C_, Uref, Cref, identity, 1000 + M + 7 * U + 13 * C_)
    want = _reference(kind, D, S, pd, ps, fc1, fc2, y)
    got = _run_abi(kind, D, S, pd, ps, fc1, fc2, y)
    rows = dict(out=M, g=M, A=U, B=C_, g_D=U, g_S=C_)
    for name, n in rows.items():
        assert bool((got[name][n:] == 7.0).all()), f"{name}: rows behind the last one were written"
    _close(got["out"][:M], want["out"], "out")
    _close(got["g"][:M], 2.0 * (want["out"] - y.double()) / M, "g")
    _close(got["loss"][0], want["loss"], "loss")
    _close(got["A"][:U], want["A"], "A")
    _close(got["B"][:C_], want["B"], "B")
    _close(got["g_D"][:U], want["g_D"], "g_D")
    _close(got["g_S"][:C_], want["g_S"], "g_S")
    for name in ("dW1", "db1", "dW2", "db2"):
        _close(got[name], want[name], name)
    # rows no pair refers to: exactly zero
    g_D, g_S = got["g_D"][:U].cpu(), got["g_S"][:C_].cpu()
    assert bool((g_D[Uref:] == 0).all()) and bool((g_S[Cref:] == 0).all())
    assert Uref == U or bool((want["g_D"][Uref:] == 0).all())
    # the gate: the known zeros and negatives of S
    known = torch.zeros_like(S, dtype=torch.bool)
    known[:, 3] = known[:, 5] = True
    known[0, 8:12] = True
    assert bool((S[known] <= 0).all())
    if kind == "cdrp":
        assert bool((g_S[S <= 0] == 0).all()), "g_cell must come back through the ReLU gate"
    else:
        assert bool((g_S[:Cref][known[:Cref]] != 0).all()), "g_xt is not gated"


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("U,C_", [(1, 1), (3, 17), (33, 65)])
def test_factored_grid_equals_the_per_pair_output(kind, U, C_):
    from fragnet_amd import _lib
    prefix, K1, _ = INSTANCES[kind]
    D, S, _, _, fc1, fc2, _ = _case(kind, 1, U, C_, 1, 1, False, 2000 + U + C_)
    pd, ps = torch.arange(U).repeat_interleave(C_), torch.arange(C_).repeat(U)
    with torch.no_grad():
        want = copy.deepcopy(fc2).double()(copy.deepcopy(fc1).double()(torch.cat((D.double()[pd], S.double()[ps]), 1))).view(U, C_)
    t = [q.to(DEV).contiguous() for q in (D, S, fc1.weight.detach(), fc1.bias.detach(), fc2.weight.detach(), fc2.bias.detach())]
    out = torch.full((U + PAD, C_), 7.0, device=DEV)
    _lib.call(prefix + "_grid_f32", *[q.data_ptr() for q in t], out.data_ptr(), U, C_, 256, K1, 128, 1, _st())
    torch.cuda.synchronize()
    _close(out[:U], want, "grid")
    assert bool((out[U:] == 7.0).all())
    lib = _lib.load()
    assert getattr(lib, prefix + "_grid_f32")(*[q.data_ptr() for q in t], out.data_ptr(), U, 4097, 256, K1, 128, 1, _st()) == _lib.FN_EINVAL
    assert getattr(lib, prefix + "_grid_f32")(*[q.data_ptr() for q in t], out.data_ptr(), U, C_, 256, K1, 64, 1, _st()) == _lib.FN_EUNSUPPORTED


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_factored_refusals_come_before_any_write_and_no_pairs_write_zeros(kind):
    from fragnet_amd import _lib, ops
    prefix, K1, _ = INSTANCES[kind]
    M, U, C_ = 5, 3, 2
    D, S, pd, ps, fc1, fc2, y = _case(kind, M, U, C_, U, C_, False, 31)
    lib, st = _lib.load(), _st()
    t = [q.to(DEV).contiguous() for q in (D, S, pd, ps, fc1.weight.detach(), fc1.bias.detach(), fc2.weight.detach(), fc2.bias.detach(), y)]
    full = lambda *shape: torch.full(shape, 7.0, device=DEV)
    A, B, out, g, part, loss = full(U, 128), full(C_, 128), full(M), full(M), full(1), full(1)
    ws = full(getattr(lib, prefix + "_ws")(U, C_))
    fwd = lambda M_, U_, C__, *w: getattr(lib, prefix + "_fwd_f32")(*[q.data_ptr() for q in t], A.data_ptr(), B.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                                         g.data_ptr(), part.data_ptr(), M_, U_, C__, *w, st)
    grads = [full(U, 256), full(C_, K1), full(128, 256 + K1), full(128), full(1, 128), full(1)]
    ords = ops.pair_orderings(t[2], U) + ops.pair_orderings(t[3], C_)
    bwd = lambda M_, U_, C__, *w: getattr(lib, prefix + "_bwd_f32")(g.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), A.data_ptr(), B.data_ptr(), t[4].data_ptr(),
                                                         t[5].data_ptr(), t[6].data_ptr(), *[o.data_ptr() for o in ords],
                                                         *[q.data_ptr() for q in grads], part.data_ptr(), 1, loss.data_ptr(), M_, U_, C__, *w, st)
    for widths in ((256, K1, 64, 1), (128, K1, 128, 1), (256, K1 - 4, 128, 1), (256, K1, 128, 2), (256, 556 - K1, 128, 1)):
        assert fwd(M, U, C_, *widths) == _lib.FN_EUNSUPPORTED and bwd(M, U, C_, *widths) == _lib.FN_EUNSUPPORTED
        assert (b"256 + %d -> 128 -> 1" % K1) in lib.fn_last_error()
    ok = (256, K1, 128, 1)
    for counts in ((M, 4097, C_), (M, U, 4097), (4097, U, C_), (M, -1, C_), (M, U, -1), (-1, U, C_)):
        assert fwd(*counts, *ok) == _lib.FN_EINVAL and bwd(*counts, *ok) == _lib.FN_EINVAL
    assert b"FN_DENSE_MAX_ROWS" in lib.fn_last_error()
    assert fwd(0, U, C_, *ok) == 0                                   # no pairs: the forward has nothing to write
    torch.cuda.synchronize()
    for q in (A, B, out, g, part, loss, ws, *grads):
        assert bool((q == 7.0).all())
    assert bwd(0, U, C_, *ok) == 0                                   # ... and every gradient is an empty sum
    torch.cuda.synchronize()
    assert all(float(q.abs().sum()) == 0.0 for q in grads) and float(loss) == 0.0


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_factored_kernels_skip_pair_indices_outside_the_rows(kind):
    """Pairs 1 and 4 point outside [0, U) / [0, C): out = 0 and g = 0 there, and everything else is what the remaining pairs alone give
    (with the mean still over all M pairs)."""
    M, U, C_ = 6, 3, 2
    D, S, pd, ps, fc1, fc2, y = _case(kind, M, U, C_, U, C_, False, 47)
    bad_d, bad_s = pd.clone(), ps.clone()
    bad_d[1], bad_s[4] = U, -1
    got = _run_abi(kind, D, S, bad_d, bad_s, fc1, fc2, y)
    keep = torch.tensor([0, 2, 3, 5])
    r1, r2 = copy.deepcopy(fc1).double(), copy.deepcopy(fc2).double()
    d2, s2 = D.double().requires_grad_(True), S.double().requires_grad_(True)
    out = r2(r1(torch.cat((d2[pd[keep]], s2[ps[keep]]), 1))).view(-1)
    loss = ((out - y.double()[keep]) ** 2).sum() / M
    loss.backward()
    assert got["out"][:M].cpu()[[1, 4]].tolist() == [0.0, 0.0] and got["g"][:M].cpu()[[1, 4]].tolist() == [0.0, 0.0]
    _close(got["out"][:M][keep.to(DEV)], out.detach(), "out")
    _close(got["loss"][0], loss.detach(), "loss")
    _close(got["g_D"][:U], d2.grad, "g_D")
    _close(got["g_S"][:C_], s2.grad * (S > 0) if kind == "cdrp" else s2.grad, "g_S")
    _close(got["dW1"], r1.weight.grad, "dW1")
    _close(got["dW2"], r2.weight.grad, "dW2")
    _close(got["db2"], r2.bias.grad, "db2")


# ------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("fused", [True, False])
def test_pair_head_factored_op_matches_float64_torch(kind, fused):
    from fragnet_amd import _lib, ops
    op = ops.pair_head_factored if kind == "cdrp" else ops.pair_head_dta_factored
    M, U, C_ = 33, 6, 4
    D, S, pd, ps, fc1, fc2, y = _case(kind, M, U, C_, U, C_, False, 77)
    want = _reference(kind, D, S, pd, ps, fc1, fc2, y)
    fc1, fc2 = fc1.to(DEV), fc2.to(DEV)
    dd, sd, yd = D.to(DEV).requires_grad_(True), S.to(DEV).requires_grad_(True), y.to(DEV)
    if fused:
        out, loss = op(dd, sd, pd.to(DEV), ps.to(DEV), fc1, fc2, loss=(_lib.LOSS_MSE, yd, None))
        assert loss is not None
    else:
        out = op(dd, sd, pd.to(DEV), ps.to(DEV), fc1, fc2)
        loss = F.mse_loss(out.view(-1), yd)
    loss.backward()
    assert out.shape == (M, 1)
    _close(out.detach().view(-1), want["out"], "out")
    _close(loss.detach(), want["loss"], "loss")
    _close(dd.grad, want["g_D"], "g_D")
    _close(sd.grad, want["g_S"], "g_S")
    for p, name in ((fc1.weight, "dW1"), (fc1.bias, "db1"), (fc2.weight, "dW2"), (fc2.bias, "db2")):
        _close(p.grad, want[name], name)
    _close((ops.pair_head_grid if kind == "cdrp" else ops.pair_head_dta_grid)(dd, sd, fc1, fc2)[pd.to(DEV), ps.to(DEV)], want["out"], "grid")
    bad = pd.clone()
    bad[3] = U
    with pytest.raises(IndexError):
        op(dd, sd, bad.to(DEV), ps.to(DEV), fc1, fc2)


def test_pair_head_factored_falls_back_outside_its_widths():
    from fragnet_amd import ops
    fc1, fc2 = torch.nn.Linear(96, 32).to(DEV), torch.nn.Linear(32, 1).to(DEV)
    a, b = torch.randn(4, 48, device=DEV), torch.randn(3, 48, device=DEV)
    pd, ps = torch.tensor([0, 3, 3, 1, 2], device=DEV), torch.tensor([2, 0, 2, 1, 1], device=DEV)
    want = fc2(fc1(torch.cat((a[pd], b[ps]), 1)))
    torch.testing.assert_close(ops.pair_head_factored(a, b, pd, ps, fc1, fc2), want)
    torch.testing.assert_close(ops.pair_head_grid(a, b, fc1, fc2)[pd, ps].view(-1, 1), want)


# ------------------------------------------------------------------------------- the models
def _model(kind, cfg, seed):
    from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
    from fragnet_amd.dta import DTAModel2
    torch.manual_seed(seed)
    return (CDRPModel(FragNetFineTuneBase(**cfg), GENE_DIM, DEV) if kind == "cdrp" else DTAModel2(FragNetFineTuneBase(**cfg))).to(DEV)


def _collates(kind):
    from fragnet_amd import data
    return (data.collate_fn_cdrp, data.collate_fn_cdrp_factored) if kind == "cdrp" else (data.collate_fn_dta, data.collate_fn_dta_factored)


def _golden_records(cfg):
    spec = importlib.util.spec_from_file_location("make_golden_pair_factored", os.path.join(GOLDEN, "make_golden_pair_factored.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.records(cfg["kind"], cfg["mol_seed"], cfg["second_seed"], cfg["pair_drug"], cfg["pair_second"], cfg["y"])


def _step_against_golden(kind, model, b, out, grads, fused):
    from fragnet_amd import _lib, ops
    second = "cell_enc" if kind == "cdrp" else "prot_enc"
    kept = {}
    hooks = [model.drug_model.register_forward_hook(lambda m, i, o: kept.__setitem__("drug_enc", o.detach().clone()))]
    tower = ops.protein_tower
    if kind == "cdrp":
        hooks.append(model.cell_model.register_forward_hook(lambda m, i, o: kept.__setitem__(second, o.detach().clone())))
    else:
        def spy(*a, **k):
            kept[second] = tower(*a, **k)
            return kept[second]
        ops.protein_tower = spy
    try:
        if fused:
            logits, loss = model(b, loss=(_lib.LOSS_MSE, b["y"], None))
            assert loss is not None, "the fused-loss launch must apply to a training step"
        else:
            logits = model(b)
            loss = F.mse_loss(logits.view(-1), b["y"])
    finally:
        ops.protein_tower = tower
        for h in hooks:
            h.remove()
    loss.backward()
    torch.cuda.synchronize()
    pd, ps = b["pair_drug"].cpu(), b["pair_second"].cpu()
    # the fixture's encodings are per PAIR (the reference duplicated the inputs): row m is the distinct row its pair names
    torch.testing.assert_close(kept["drug_enc"].detach().cpu()[pd], torch.from_numpy(out["drug_enc"]), atol=ATOL, rtol=1e-4)
    torch.testing.assert_close(kept[second].detach().cpu()[ps], torch.from_numpy(out[second]), atol=ATOL, rtol=1e-4)
    torch.testing.assert_close(logits.detach().cpu(), torch.from_numpy(out["logits"]), atol=ATOL, rtol=1e-4)
    assert abs(loss.item() - float(out["loss"])) < ATOL
    check_grads(model, grads, atol=ATOL, rtol=1e-4)


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("fused", [True, False])
def test_factored_models_match_the_reference_on_repeating_pairs(kind, fused):
    from fragnet_amd import data
    cfg, batch, out, grads, pkeys, psums = load_case(f"{kind}_pairs_u3c3")
    recs = _golden_records(cfg)
    fb = _collates(kind)[1](recs)
    assert fb[data.N_MOLS_KEY] == 3 and fb["gene_expr" if kind == "cdrp" else "protein"].shape[0] == 3 and fb["y"].shape[0] == 7
    assert fb["pair_drug"].tolist() == cfg["pair_drug"] and fb["pair_second"].tolist() == cfg["pair_second"]
    assert torch.equal(_collates(kind)[0](recs)["x_atoms"], batch["x_atoms"]), "the records are not the fixture's"
    model = _model(kind, cfg["ctor"], cfg["seed"])
    check_params_match(model, pkeys, psums)
    model.train()
    _step_against_golden(kind, model, data.batch_to(fb, DEV), out, grads, fused)


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("fused", [True, False])
def test_factored_models_match_the_reference_through_identity_lists(kind, fused):
    from fragnet_amd import data
    cfg, batch, out, grads, pkeys, psums = load_case(f"{kind}_b5")
    model = _model(kind, cfg["ctor"], cfg["seed"])
    check_params_match(model, pkeys, psums)
    model.train()
    _step_against_golden(kind, model, data.as_factored(data.batch_to(batch, DEV)), out, grads, fused)


def _pairs(kind, n_pairs=33, n_drugs=6, n_seconds=4, seed=6100):
    from fragnet_amd import synth
    return synth.pair_records(n_pairs, n_drugs, n_seconds, kind, seed)


def _grads_of(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_factored_step_matches_the_duplicated_step(kind):
    from fragnet_amd import _lib, data
    from fragnet_amd.plan import plan_for
    recs = _pairs(kind)
    dup, fac = (data.batch_to(c(recs), DEV) for c in _collates(kind))
    res = []
    for b in (dup, fac):
        model = _model(kind, SMALL, 3)
        model.train()
        out, loss = model(b, loss=(_lib.LOSS_MSE, b["y"], None))
        loss.backward()
        res.append((out.detach(), loss.detach(), _grads_of(model)))
    assert plan_for(fac).n_mols == 6 and plan_for(dup).n_mols == 33
    assert res[1][0].shape == (33, 1)
    torch.testing.assert_close(res[1][0], res[0][0], atol=ATOL, rtol=1e-4)
    torch.testing.assert_close(res[1][1], res[0][1], atol=ATOL, rtol=1e-4)
    assert res[0][2].keys() == res[1][2].keys()
    for n, g in res[0][2].items():
        torch.testing.assert_close(res[1][2][n], g, atol=ATOL, rtol=1e-4, msg=lambda m, n=n: f"{n}: {m}")


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_grid_batch_gives_every_drug_against_every_second_input(kind):
    from fragnet_amd import data
    recs = _pairs(kind)
    fb = _collates(kind)[1](recs)
    key = "gene_expr" if kind == "cdrp" else "protein"
    first = [fb["pair_drug"].tolist().index(u) for u in range(6)]
    grid = data.batch_to(data.pair_grid_batch([recs[i] for i in first], fb[key], kind), DEV)
    model = _model(kind, SMALL, 3)
    model.eval()
    with torch.no_grad():
        full = model(grid)
        out = model(data.batch_to(fb, DEV))
    assert full.shape == (6, 4)
    torch.testing.assert_close(full[fb["pair_drug"].to(DEV), fb["pair_second"].to(DEV)], out.view(-1), atol=ATOL, rtol=1e-4)


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_factored_step_is_bitwise_reproducible(kind, drop):
    """No float atomics and one arrival order-independent forward: two runs give identical bits, also with dropout on a fixed stream."""
    from fragnet_amd import _lib, data
    b = data.batch_to(_collates(kind)[1](_pairs(kind)), DEV)
    outs = []
    for _ in range(2):
        model = _model(kind, dict(SMALL, drop_ratio=drop), 0)
        model.drug_model.pretrain.rng.seed, model.drug_model.pretrain.rng.offset = 1234, 0
        model.train()
        out, loss = model(b, loss=(_lib.LOSS_MSE, b["y"], None))
        loss.backward()
        outs.append((loss.item(), out.detach().clone(), _grads_of(model)))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2].keys() == outs[1][2].keys() and "fc1.weight" in outs[0][2]
    for n, g in outs[0][2].items():
        assert torch.equal(g, outs[1][2][n]), n


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_factored_step_runs_no_library_math(kind, monkeypatch):
    from fragnet_amd import _lib, data
    b = data.batch_to(_collates(kind)[1](_pairs(kind)), DEV)
    model = _model(kind, SMALL, 1)
    model.train()

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called on the factored step")
        return f
    for name in ("linear", "conv1d", "embedding"):
        monkeypatch.setattr(F, name, refuse("F." + name))
    for name in ("addmm", "mm", "matmul", "bmm", "cat"):
        monkeypatch.setattr(torch, name, refuse("torch." + name))
    _, loss = model(b, loss=(_lib.LOSS_MSE, b["y"], None))
    loss.backward()
    out = model(b)                                                # and the plain call
    ((out.view(-1) - b["y"]) ** 2).mean().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert torch.isfinite(loss).item() and model.fc1.weight.grad is not None


class _Loader(list):
    """pre-collated batches with the ``dataset`` attribute the trainers normalise by"""
    dataset = ()


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_training_run_on_a_factored_loader_lowers_the_loss(kind):
    """Learning rates of the two existing training-run tests: 1e-3 (CDRP), 1e-4 (DTA)."""
    import numpy as np
    from fragnet_amd import data, train
    recs = _pairs(kind, n_pairs=64, n_drugs=8, n_seconds=6, seed=6300)
    ys = np.array([float(r.y) for r in recs])
    loader = _Loader([data.batch_to(_collates(kind)[1](recs), DEV)])
    loader.dataset = recs
    model = _model(kind, SMALL, 2)
    if kind == "cdrp":
        trainer, lr, kw = train.TrainerFineTuneCDRP(target_type="regr"), 1e-3, dict(label_mean=0.0, label_sdev=1.0)
    else:
        trainer, lr, kw = train.TrainerFineTuneDTA(target_type="regr"), 1e-4, dict(label_mean=float(ys.mean()), label_sdev=float(ys.std()))
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    before = trainer.validate(model, loader, device=DEV, **kw)
    for _ in range(30):
        trainer.train(model=model, loader=loader, optimizer=opt, scheduler=None, device=DEV, val_loader=None, **kw)
    after = trainer.validate(model, loader, device=DEV, **kw)
    mse, true, pred = trainer.test(model, loader, device=DEV, **kw)
    assert after < before, (before, after)
    assert true.shape == pred.shape == (64,) and np.allclose(true, ys.astype(np.float32))      # M predictions, in pair order
    assert abs(mse / 64 - after) <= 1e-4 * max(1.0, after)


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_screen_in_chunks_equals_the_whole_grid(kind):
    """scripts/screen_pairs.py: chunks that do not divide U and C give the matrix of one grid batch"""
    from fragnet_amd import data
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("screen_pairs", os.path.join(root, "scripts", "screen_pairs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    recs = _pairs(kind, n_pairs=7, n_drugs=5, n_seconds=7, seed=6400)
    fb = _collates(kind)[1](recs)
    drugs = [recs[fb["pair_drug"].tolist().index(u)] for u in range(5)]
    second = mod.second_rows(recs, "gene_expr" if kind == "cdrp" else "protein")
    model = _model(kind, SMALL, 4)
    whole = mod.screen(model, kind, drugs, second, DEV, 5, 7)
    parts = mod.screen(model, kind, drugs, second, DEV, 2, 3)
    assert whole.shape == (5, 7)
    torch.testing.assert_close(parts, whole, atol=ATOL, rtol=1e-4)
    with torch.no_grad():
        pairs = model(data.batch_to(fb, DEV)).view(-1).cpu()
    # column m is record m's second input (7 records over 7 distinct second inputs): entry (pair_drug[m], m) is pair m's prediction
    torch.testing.assert_close(whole[fb["pair_drug"], torch.arange(7)], pairs, atol=ATOL, rtol=1e-4)
