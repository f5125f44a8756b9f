"""model_version gcn2 on the GPU (fragnet_amd/gcn.py, csrc/gcn.hip).

* the aggregate kernel (forward on the by-destination CSR, backward = the same kernel on the by-source CSR, fn_gcn_coef_f32) against a
  dense float64 ``A_hat`` built here from the raw index lists, on seeded random DIRECTED graphs whose in-degrees differ from their
  out-degrees -- a kernel that normalised by the wrong endpoint's degree would fail; the reference counts ``source`` (gcn2.py:51).
  Tolerances are test_gpu_gat_level_property.py's for an attention level: rows 2e-5 absolute / 1e-4 relative, gradients 5e-5 x scale;
* parity with the reference's own numbers (tests/golden/ft_gcn2_*.npz): logits, loss, per-layer traces, gradients, 1e-4;
* dropout on, against a float64 restatement of the model with the masks of the recorded Philox draws injected;
* bit-for-bit reproducibility of a training step; the fine-tune driver.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4          # the project's standing tolerance against golden vectors
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    _lib.load()


# ----------------------------------------------------------------------------------------------- the kernel against a dense float64 A_hat
EXTENTS = (0, 1, 2, 7, 8, 9, 16, 17, 39, 40)      # real in-/out-degrees of the designated rows: the plain mode sees them as they are, the
                                                  # normalised mode one more (the loop): 0 / 1 (loop only) / 2 / 8 / 9 / 17 / a hub of 40 in both


def _graph(n, seed):
    """(dst, src) of a directed multigraph on n nodes.  n >= 33: rows 0..9 have exactly EXTENTS in-edges, rows 10..19 exactly EXTENTS
    out-edges (the backward's rows), the other endpoints and all further edges are drawn among the remaining nodes -- so in-degree and
    out-degree differ almost everywhere.  Smaller n: a few random edges, duplicates and explicit loops allowed."""
    g = torch.Generator().manual_seed(seed)
    if n < 33:
        m = 2 * n + 1
        return torch.randint(0, n, (m,), generator=g), torch.randint(0, n, (m,), generator=g)
    free = torch.cat([torch.arange(0, 10), torch.arange(20, n)])
    dst, src = [], []
    for row, k in enumerate(EXTENTS):
        dst.append(torch.full((k,), row))
        src.append(free[torch.randint(0, free.numel(), (k,), generator=g)])
    for row, k in enumerate(EXTENTS):
        src.append(torch.full((k,), 10 + row))
        dst.append(torch.randint(20, n, (k,), generator=g))
    extra = 2 * n
    dst.append(torch.randint(20, n, (extra,), generator=g))
    src.append(torch.randint(20, n, (extra,), generator=g))
    dst, src = torch.cat(dst), torch.cat(src)
    perm = torch.randperm(dst.numel(), generator=g)
    return dst[perm], src[perm]


def _a_hat(n, dst, src, normalised):
    """dense float64 [n, n]: row t, column s = sum over the edges s -> t of c[s] c[t]; normalised: with one loop per node and
    c = (out-degree incl. the loop)^-1/2 -- the reference's degree(source) --, else c = 1 and no loops"""
    if normalised:
        dst, src = torch.cat([dst, torch.arange(n)]), torch.cat([src, torch.arange(n)])
        deg = torch.zeros(n, dtype=torch.float64).scatter_add_(0, src, torch.ones(src.numel(), dtype=torch.float64))
        c = deg.pow(-0.5)
        c[deg == 0] = 0
    else:
        c = torch.ones(n, dtype=torch.float64)
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((dst, src), c[src] * c[dst], accumulate=True)
    return A, c


def _philox_mask(numel, p, seed, offset):
    from tests.test_gpu_dropout_parity import philox_mask
    return philox_mask(numel, p, seed, offset)


def _run_kernel(n, dst, src, normalised, epilogue, seed):
    from fragnet_amd import _lib, ops
    from fragnet_amd.plan import GraphPlan, _stream_ptr
    import ctypes as C
    g = torch.Generator().manual_seed(seed ^ 0x5bd1e995)
    x = torch.randn(n, 128, generator=g)
    w_raw, w_act = torch.randn(n, 128, generator=g), torch.randn(n, 128, generator=g)
    A, c = _a_hat(n, dst, src, normalised)
    plan = GraphPlan([dict(kind="gat", name="l", dst=dst.to(DEV), src=src.to(DEV), n=n, n_loops=n if normalised else 0)], DEV)
    lv = plan.levels["l"]
    coef = ops.gcn_coef(lv) if normalised else None
    note = f"n={n} m={dst.numel()} normalised={normalised} epilogue={epilogue}"
    if normalised:
        torch.testing.assert_close(coef.cpu().double(), c, atol=0, rtol=5e-7, msg=lambda s: f"coef [{note}]: {s}")

    # ---- oracle
    want_raw = A @ x.double()
    p = 0.5 if epilogue == "drop" else 0.0
    rng = ops.PhiloxStream(seed=0xABCDEF12345)
    rng.offset = 77
    mask = torch.ones(n, 128, dtype=torch.float64)
    if epilogue == "drop" and n:
        mask = _philox_mask(n * 128, p, rng.seed, rng.offset).view(n, 128).cpu().double()
        assert set(mask.unique().tolist()) <= {0.0, 2.0}
    want_act = torch.relu(want_raw * mask)
    want_gx = A.t() @ (w_raw.double() if epilogue == "off" else w_raw.double() + w_act.double() * mask * (want_raw * mask > 0))

    # ---- the C entry point on buffers of this test: over-allocated by sentinel rows, pre-filled with the sentinel
    xd = x.to(DEV)
    pad = 3
    out = torch.full((n + pad, 128), SENTINEL, device=DEV)
    y = torch.full((n + pad, 128), SENTINEL, device=DEV)
    act = None
    if epilogue != "off":
        act = _lib.ActEpilogue(y.data_ptr(), p, 1, rng.seed if p else 0, rng.offset if p else 0, None)
    _lib.call("fn_gcn_aggregate_f32", xd.data_ptr(), C.byref(lv.c), 0, None if coef is None else coef.data_ptr(), out.data_ptr(),
              None if act is None else C.byref(act), _stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    plan.check()
    assert torch.isfinite(out).all(), note
    assert bool((out[n:] == SENTINEL).all()) and bool((y[n:] == SENTINEL).all()), f"rows behind the level were written [{note}]"
    torch.testing.assert_close(out[:n].cpu().double(), want_raw, atol=2e-5, rtol=1e-4, msg=lambda s: f"raw rows [{note}]: {s}")
    if epilogue != "off":
        torch.testing.assert_close(y[:n].cpu().double(), want_act, atol=2e-5, rtol=1e-4, msg=lambda s: f"activated rows [{note}]: {s}")
    else:
        assert bool((y == SENTINEL).all()), f"an output that was not asked for was written [{note}]"
    if not normalised:
        indeg = torch.bincount(dst, minlength=n) if n else torch.zeros(0, dtype=torch.long)
        empty = (indeg == 0).nonzero().flatten()
        assert bool((out[:n].cpu()[empty] == 0).all()), f"a row without items must come back as zeros, not be skipped [{note}]"
        if epilogue != "off":
            assert bool((y[:n].cpu()[empty] == 0).all()), note
    if normalised and dst.numel() == 0:
        assert torch.equal(out[:n].cpu(), x), f"loops only: every degree is 1, y == x bit for bit [{note}]"

    # ---- the autograd operator: the same forward, bit for bit, and the input gradient (the kernel on the by-source CSR)
    leaf = xd.clone().requires_grad_(True)
    if epilogue == "off":
        raw = ops.gcn_aggregate(leaf, lv, coef)
        loss = (raw * w_raw.to(DEV)).sum()
    else:
        raw, act_rows = ops.gcn_aggregate(leaf, lv, coef, act=(p, True, True, rng), raw=True)
        assert torch.equal(act_rows, y[:n]), note
        loss = (raw * w_raw.to(DEV)).sum() + (act_rows * w_act.to(DEV)).sum()
        only = ops.gcn_aggregate(xd, lv, coef, act=(0.0, True, True, rng))          # the activated rows alone (layers 0..L-2)
        torch.testing.assert_close(only.cpu().double(), torch.relu(want_raw), atol=2e-5, rtol=1e-4)
    assert torch.equal(raw, out[:n]), note
    loss.backward()
    torch.cuda.synchronize()
    got = leaf.grad.cpu().double() if leaf.grad is not None else torch.zeros(n, 128, dtype=torch.float64)
    scale = max(1.0, float(want_gx.abs().max())) if n else 1.0
    torch.testing.assert_close(got, want_gx, atol=5e-5 * scale, rtol=1e-4, msg=lambda s: f"grad x [{note}]: {s}")


@pytest.mark.parametrize("normalised", [True, False], ids=["normalised", "plain"])
@pytest.mark.parametrize("n", [1, 2, 3, 33, 257])
def test_aggregate_equals_dense_float64_on_directed_graphs(n, normalised):
    dst, src = _graph(n, seed=1000 + n)
    if n >= 33:
        indeg, outdeg = torch.bincount(dst, minlength=n), torch.bincount(src, minlength=n)
        assert indeg[:10].tolist() == list(EXTENTS) and outdeg[10:20].tolist() == list(EXTENTS)
        assert int((indeg != outdeg).sum()) > n // 2          # a directed graph: the two degrees differ
    for epilogue in ("off", "relu", "drop"):
        _run_kernel(n, dst, src, normalised, epilogue, seed=n)


@pytest.mark.parametrize("normalised", [True, False], ids=["normalised", "plain"])
def test_aggregate_without_real_edges_and_without_rows(normalised):
    none = torch.zeros(0, dtype=torch.long)
    for n in (0, 5, 33):                    # n = 0: nothing is launched; m_real = 0: loops only (y == x bit for bit) or all rows zero
        for epilogue in ("off", "relu", "drop"):
            _run_kernel(n, none, none, normalised, epilogue, seed=50 + n)


def test_aggregate_checks_its_arguments():
    from fragnet_amd import _lib, ops
    from fragnet_amd.plan import GraphPlan
    dst, src = _graph(3, seed=5)
    lv = GraphPlan([dict(kind="gat", name="l", dst=dst.to(DEV), src=src.to(DEV), n=3, n_loops=3)], DEV).levels["l"]
    x = torch.randn(3, 128, device=DEV)
    with pytest.raises(_lib.FragnetHipError):
        ops.gcn_aggregate(x.cpu(), lv)
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x[:2], lv)
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, lv, torch.ones(4, device=DEV))
    with pytest.raises(TypeError):
        ops.gcn_aggregate(x.double(), lv)
    assert _lib.load().fn_gcn_aggregate_f32(x.data_ptr(), None, 0, None, None, None, None) == _lib.FN_EINVAL


# ----------------------------------------------------------------------------------------------- parity with the reference's numbers
def _model_and_batch(case, drop=None):
    from fragnet_amd import data
    from fragnet_amd.gcn import FragNetFineTune
    from tests.helpers import check_params_match, load_case
    cfg, batch, out, grads, pkeys, psums = load_case(case)
    ctor = dict(cfg["ctor"]) if drop is None else dict(cfg["ctor"], drop_ratio=drop)
    torch.manual_seed(cfg["seed"])
    model = FragNetFineTune(**ctor)
    check_params_match(model, pkeys, psums)
    return model.to(DEV).train(), data.batch_to(batch, DEV), batch, out, grads, ctor


@pytest.mark.parametrize("case", ["ft_gcn2_b6", "ft_gcn2_edge_b6"])
def test_golden_parity(case):
    from tests.helpers import check_grads
    model, b, _, out, grads, ctor = _model_and_batch(case)
    logits = model(b)
    loss = torch.nn.functional.mse_loss(logits.view(-1), b["y"])
    loss.backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(logits.detach().cpu(), torch.from_numpy(out["logits"]), atol=ATOL, rtol=1e-4)
    assert abs(float(loss) - float(out["loss"])) < ATOL, (float(loss), float(out["loss"]))
    check_grads(model, grads, atol=ATOL, rtol=1e-4)
    dead = [n for n, q in model.named_parameters() if n not in grads["sum"]]
    assert len(dead) == 46 if case == "ft_gcn2_b6" else dead
    assert all(dict(model.named_parameters())[n].grad is None for n in dead)
    # per-layer traces: the layers called with the reference's own 6-argument signature hand back the raw rows of both halves
    x = b["x_atoms"]
    with torch.no_grad():
        for i, layer in enumerate(model.pretrain.layers):
            raw_a, raw_f = layer(x, b["edge_index"], b["edge_attr"], b["frag_index"], b["x_frags"], b["atom_to_frag_ids"])
            for got, nm in ((raw_a, "x_atoms"), (raw_f, "x_frags")):
                torch.testing.assert_close(got.cpu(), torch.from_numpy(out[f"layer{i}/{nm}"]), atol=ATOL, rtol=1e-4,
                                           msg=lambda s, i=i, nm=nm: f"layer {i} {nm}: {s}")
            x = torch.relu(raw_a)


# ----------------------------------------------------------------------------------------------- dropout on
def _restated(sd, batch, masks, L, n_hidden):
    """the model in plain float64 torch: dense operators from the raw index lists, the given masks (already scaled by 1 / (1 - p))
    multiplied in where the model draws: input atoms, every layer's atoms, the last layer's fragments, every hidden layer of FTHead3"""
    P = {k: v.detach().cpu().double().requires_grad_(v.dtype.is_floating_point) for k, v in sd.items()}
    N, F, B = batch["x_atoms"].shape[0], batch["x_frags"].shape[0], batch["y"].shape[0]
    ei, fi = batch["edge_index"], batch["frag_index"]
    A, _ = _a_hat(N, ei[1], ei[0], True)
    Af, _ = _a_hat(F, fi[1], fi[0], False)
    onehot = lambda idx, rows: torch.zeros(rows, idx.numel(), dtype=torch.float64).index_put_((idx, torch.arange(idx.numel())), torch.ones((), dtype=torch.float64))
    S, Ma, Mf = onehot(batch["atom_to_frag_ids"], F), onehot(batch["batch"], B), onehot(batch["frag_batch"], B)
    lin = lambda x, pre: x @ P[pre + ".weight"].t() + P[pre + ".bias"]
    it = iter(masks)
    x = batch["x_atoms"].double() * next(it)
    for l in range(L):
        raw = A @ lin(x, f"pretrain.layers.{l}.atom_embed")
        x = torch.relu(raw * next(it))
    z = lin(torch.relu(lin(Af @ (S @ raw), f"pretrain.layers.{L - 1}.frag_mlp.0")), f"pretrain.layers.{L - 1}.frag_mlp.2")
    xf = torch.relu(z * next(it))
    h = torch.cat((Ma @ x, Mf @ xf), 1)
    for i in range(n_hidden):
        h = torch.relu(lin(h, f"fthead.predictor.{i}") * next(it))
    out = lin(h, f"fthead.predictor.{n_hidden}")
    assert next(it, None) is None
    return out, P


def test_dropout_on_matches_float64_restatement_under_the_same_masks():
    from tests.test_gpu_dropout_parity import TakeLog
    p = 0.1
    model, b, batch, _, grads, ctor = _model_and_batch("ft_gcn2_b6", drop=p)
    model.pretrain.rng.seed = 0x1234567
    with TakeLog(model.pretrain.rng) as log:
        logits = model(b)
        loss = torch.nn.functional.mse_loss(logits.view(-1), b["y"])
        loss.backward()
    torch.cuda.synchronize()
    L = ctor["num_layer"]
    N, F, B = b["x_atoms"].shape[0], b["x_frags"].shape[0], b["y"].shape[0]
    dims = [ctor["h1"], ctor["h2"], ctor["h3"], ctor["h4"]]
    shapes = [(N, b["x_atoms"].shape[1])] + [(N, 128)] * L + [(F, 128)] + [(B, d) for d in dims]
    assert [c[2] for c in log.calls] == [r * w for r, w in shapes]           # the draws, in the model's order
    masks = [_philox_mask(r * w, p, seed, off).view(r, w).cpu().double() for (seed, off, _), (r, w) in zip(log.calls, shapes)]
    kept = torch.cat([m.reshape(-1) for m in masks])
    assert 0.85 < float((kept > 0).double().mean()) < 0.95                     # these really are p = 0.1 masks
    want, P = _restated(model.state_dict(), batch, masks, L, len(dims))
    want_loss = torch.nn.functional.mse_loss(want.view(-1), batch["y"].double())
    want_loss.backward()
    torch.testing.assert_close(logits.detach().cpu().double(), want.detach(), atol=ATOL, rtol=1e-4)
    assert abs(float(loss) - float(want_loss)) < ATOL, (float(loss), float(want_loss))
    checked = 0
    for name, q in model.named_parameters():
        if name not in grads["sum"]:
            assert q.grad is None, name
            assert P[name].grad is None or float(P[name].grad.abs().sum()) == 0.0, name
            continue
        torch.testing.assert_close(q.grad.cpu().double(), P[name].grad, atol=ATOL, rtol=1e-4, msg=lambda s, name=name: f"{name}: {s}")
        checked += 1
    assert checked == 2 * L + 4 + 2 * (len(dims) + 1)


# ----------------------------------------------------------------------------------------------- reproducibility
def test_training_step_is_reproducible_bit_for_bit():
    model, b, _, _, grads, _ = _model_and_batch("ft_gcn2_edge_b6", drop=0.1)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(0)
        model.pretrain.rng.seed, model.pretrain.rng.offset = 99, 0
        b.pop("_fragnet_gcn_plan", None)
        loss = torch.nn.functional.mse_loss(model(b).view(-1), b["y"])
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert set(runs[0][1]) == set(runs[1][1]) == set(grads["sum"])
    for name in runs[0][1]:
        assert torch.equal(runs[0][1][name], runs[1][1][name]), name


# ----------------------------------------------------------------------------------------------- the driver
def test_finetune_driver_runs_gcn2(tmp_path):
    from fragnet_amd import synth
    from fragnet_amd.dataset import FlatMolStore
    data_dir = tmp_path / "finetune_data" / "esol_synth"
    os.makedirs(data_dir)
    for split, n, s in (("train", 64, 0), ("val", 16, 1), ("test", 16, 2)):
        FlatMolStore.from_records(synth.synth_molecules(n, seed=s, profile="esol")).save(str(data_dir / f"{split}.pt"))
    cfg = open(os.path.join(ROOT, "exps/ft/esol_synth_gcn2/config.yaml")).read()
    assert "model_version: gcn2" in cfg
    cfg = cfg.replace("batch_size: 512", "batch_size: 32").replace("n_epochs: 20\n", "n_epochs: 1\n")
    (tmp_path / "config.yaml").write_text(cfg)
    # a fresh child process under its own time limit
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "scripts", "finetune_gat2.py"), "--config", "config.yaml"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    log = [json.loads(l) for l in open(tmp_path / "exps/ft/esol_synth_gcn2/log.jsonl")]
    assert len(log) == 1 and log[0]["Loss/train"] > 0 and log[0]["Loss/train"] == log[0]["Loss/train"]
    sd = torch.load(tmp_path / "exps/ft/esol_synth_gcn2/ft.pt", map_location="cpu")
    from fragnet_amd.gcn import FragNetFineTune
    keys = list(FragNetFineTune(num_layer=4, h1=128, h2=1024, h3=1024, h4=512, act="relu", edge_features=17, drop_ratio=0.1).state_dict())
    assert list(sd) == keys and "test_res rmse" in r.stdout
