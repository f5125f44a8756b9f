"""Prediction-head small ops (include/fragnet_hip.h: fn_gate_colsum_f32, fn_small_linear(_bwd)_f32) and the fused
``ops.mlp_head`` autograd node against plain torch and against the unfused layer-by-layer path."""
import copy

import pytest
import torch

from tests.helpers import tuning

gpu = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@gpu
@pytest.mark.parametrize("rows,cols", [(528, 1024), (37, 128), (0, 64), (1, 4), (300, 36), (28104, 64), (2049, 32)])
def test_gate_colsum_matches_torch(rows, cols):
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    dev = _dev()
    torch.manual_seed(rows + cols)
    g = torch.randn(rows, cols, device=dev)
    y = torch.relu(torch.randn(rows, cols, device=dev))            # about half zeros, like relu(dropout(.))
    gx, cs = torch.full_like(g, 7.0), torch.full((cols,), 7.0, device=dev)
    n_ws = _lib.load().fn_gate_colsum_ws(rows, cols)
    ws = torch.empty(n_ws, device=dev) if n_ws else None
    assert (n_ws > 0) == (rows > 2048)
    _lib.call("fn_gate_colsum_f32", g.data_ptr(), y.data_ptr(), gx.data_ptr(), cs.data_ptr(), rows, cols, 1.25,
              None if ws is None else ws.data_ptr(), _stream_ptr(dev))
    ref = torch.where(y > 0, g * 1.25, torch.zeros_like(g))
    assert torch.equal(gx, ref)
    torch.testing.assert_close(cs, ref.double().sum(0).float(), atol=2e-4 * max(1.0, rows / 500) ** 0.5, rtol=1e-5)


@gpu
@pytest.mark.parametrize("M,K,C", [(528, 512, 1), (528, 512, 12), (5, 128, 3), (0, 64, 2), (100, 36, 16), (28104, 32, 1), (13872, 32, 3)])
def test_small_linear_matches_torch(M, K, C):
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    dev = _dev()
    torch.manual_seed(M + K + C)
    x, w, b = torch.randn(M, K, device=dev), torch.randn(C, K, device=dev) * 0.1, torch.randn(C, device=dev)
    g = torch.randn(M, C, device=dev)
    y = torch.empty(M, C, device=dev)
    st = _stream_ptr(dev)
    _lib.call("fn_small_linear_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, C, M, st)
    torch.testing.assert_close(y, (x.double() @ w.double().t() + b.double()).float(), atol=2e-5, rtol=1e-5)
    gx, dW, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    n_ws = _lib.load().fn_small_linear_bwd_ws(M, K, C)
    ws = torch.empty(n_ws, device=dev) if n_ws else None
    _lib.call("fn_small_linear_bwd_f32", g.data_ptr(), x.data_ptr(), w.data_ptr(), gx.data_ptr(), dW.data_ptr(), db.data_ptr(), M, K, C,
              0.0, None if ws is None else ws.data_ptr(), st)
    torch.testing.assert_close(gx, (g.double() @ w.double()).float(), atol=2e-5, rtol=1e-5)
    tol = 2e-4 * max(1.0, M / 500) ** 0.5
    torch.testing.assert_close(dW, (g.double().t() @ x.double()).float(), atol=tol, rtol=1e-5)
    torch.testing.assert_close(db, g.double().sum(0).float(), atol=tol, rtol=1e-5)
    gx2 = torch.empty_like(x)                                        # gated: the backward of the relu(dropout(.)) that produced x
    _lib.call("fn_small_linear_bwd_f32", g.data_ptr(), x.data_ptr(), w.data_ptr(), gx2.data_ptr(), dW.data_ptr(), db.data_ptr(), M, K, C,
              1.25, None if ws is None else ws.data_ptr(), st)
    assert torch.equal(gx2, torch.where(x > 0, gx * 1.25, torch.zeros_like(gx)))


@gpu
@pytest.mark.parametrize("M,K,N", [(528, 256, 1024), (528, 1024, 1024), (33, 128, 512), (1, 4, 4), (200, 20, 36), (0, 64, 32), (4096, 132, 68)])
def test_dense_layer_kernels_match_torch(M, K, N):
    """fn_dense_fwd_f32 / fn_dense_bwd_f32 (fp32 matrix cores, fused bias + dropout + ReLU / gate + bias gradient) against
    float64 products and the standalone fn_dropout_act_f32 Philox stream."""
    import ctypes as C
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    dev = _dev()
    st = _stream_ptr(dev)
    torch.manual_seed(M + K + N)
    x, w, b = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5, torch.randn(N, device=dev)
    lin = (x.double() @ w.double().t() + b.double()).float()
    y = torch.full((M, N), 7.0, device=dev)
    _lib.call("fn_dense_fwd_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, None, st)
    torch.testing.assert_close(y, lin, atol=2e-5, rtol=1e-5)
    off_dev = torch.tensor([40], dtype=torch.int64, device=dev)
    act = _lib.ActEpilogue(None, 0.25, 1, 99, 1000, off_dev.data_ptr())
    z = torch.full((M, N), 7.0, device=dev)
    _lib.call("fn_dense_fwd_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), M, K, N, C.byref(act), st)
    want = torch.empty_like(y)
    if M:
        _lib.call("fn_dropout_act_f32", y.data_ptr(), want.data_ptr(), y.numel(), 0.25, 99, 1040, None, 1, st)
        assert torch.equal(z > 0, want > 0) or ((z > 0) != (want > 0)).sum() <= 2          # pre-activations within rounding of 0
        torch.testing.assert_close(z, want, atol=3e-5, rtol=1e-5)
    g = torch.randn(M, N, device=dev)
    xr = torch.relu(x)                                               # a layer input that is itself relu(dropout(.)): about half zeros
    for gate in (4.0 / 3.0, 0.0):
        gx, dW, db = torch.full_like(x, 7.0), torch.full_like(w, 7.0), torch.full_like(b, 7.0)
        _lib.call("fn_dense_bwd_f32", g.data_ptr(), xr.data_ptr(), w.data_ptr(), gx.data_ptr(), gate, dW.data_ptr(), db.data_ptr(),
                  M, K, N, M, st)
        tol = 2e-4 * max(1.0, M / 500) ** 0.5
        want = g.double() @ w.double()
        if gate:
            want = torch.where(xr > 0, want * gate, torch.zeros_like(want))
        torch.testing.assert_close(gx, want.float(), atol=3e-5, rtol=1e-5)
        torch.testing.assert_close(dW, (g.double().t() @ xr.double()).float(), atol=tol, rtol=1e-5)
        torch.testing.assert_close(db, g.double().sum(0).float(), atol=tol, rtol=1e-5)
    dW2 = torch.full_like(w, 7.0)                                    # first layer: no input gradient, no bias gradient
    _lib.call("fn_dense_bwd_f32", g.data_ptr(), x.data_ptr(), w.data_ptr(), None, 0.0, dW2.data_ptr(), None, M, K, N, M, st)
    torch.testing.assert_close(dW2, (g.double().t() @ x.double()).float(), atol=2e-4 * max(1.0, M / 500) ** 0.5, rtol=1e-5)
    if 0 < M <= 4000:                                                # padding rows behind M: written as 0 by the same launch
        gx3 = torch.full((M + 40, K), 7.0, device=dev)
        _lib.call("fn_dense_bwd_f32", g.data_ptr(), xr.data_ptr(), w.data_ptr(), gx3.data_ptr(), 0.0, dW2.data_ptr(), None, M, K, N, M + 40, st)
        assert torch.equal(gx3[:M], gx) and not gx3[M:].any()
        y3 = torch.full((M + 5, N if N <= 16 else 1), 7.0, device=dev)
        Cs = y3.shape[1]
        _lib.call("fn_small_linear_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), y3.data_ptr(), M, K, Cs, M + 5, st)
        torch.testing.assert_close(y3[:M], lin[:, :Cs], atol=2e-5, rtol=1e-5)
        assert not y3[M:].any()


@gpu
@pytest.mark.parametrize("M,K,N", [(2048, 1024, 1024), (2100, 128, 1024), (1600, 64, 1000), (4096, 32, 512), (1537, 96, 1024)])
def test_dense_forward_on_workgroup_shared_tiles_matches_float64_and_the_per_wave_kernel(M, K, N):
    """fn_dense_fwd_f32 on tall inputs (>= 192 tiles of 64 x 128, K a multiple of 32: k_dense_fwd_tiles, FN_TUNE_DENSE_TILES): ragged row
    and column edges, reductions shorter than the ring (K = 32, 64), against float64 products, against the standalone Philox stream
    (bias + dropout + ReLU epilogue) and against the per-wave-operand kernel the same call runs with the key off."""
    import ctypes as C
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    dev = _dev()
    st = _stream_ptr(dev)
    assert -(-M // 64) * -(-N // 128) >= 192 and K % 32 == 0
    torch.manual_seed(M + K + N)
    x, w, b = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5, torch.randn(N, device=dev)
    lin = (x.double() @ w.double().t() + b.double()).float()
    y = torch.full((M + 3, N), 7.0, device=dev)                      # three guard rows behind the output
    _lib.call("fn_dense_fwd_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, None, st)
    torch.testing.assert_close(y[:M], lin, atol=2e-5, rtol=1e-5)
    assert bool((y[M:] == 7.0).all())
    off_dev = torch.tensor([40], dtype=torch.int64, device=dev)
    act = _lib.ActEpilogue(None, 0.25, 1, 99, 1000, off_dev.data_ptr())
    z = torch.full((M, N), 7.0, device=dev)
    _lib.call("fn_dense_fwd_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), M, K, N, C.byref(act), st)
    want = torch.empty((M, N), device=dev)
    plain = y[:M].contiguous()
    _lib.call("fn_dropout_act_f32", plain.data_ptr(), want.data_ptr(), plain.numel(), 0.25, 99, 1040, None, 1, st)
    torch.testing.assert_close(z, want, atol=3e-5, rtol=1e-5)
    with tuning({32: 0}):
        z0 = torch.full((M, N), 7.0, device=dev)
        _lib.call("fn_dense_fwd_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), z0.data_ptr(), M, K, N, C.byref(act), st)
    assert ((z > 0) != (z0 > 0)).sum() <= 2                          # the same masks; pre-activations within rounding of 0 may flip
    torch.testing.assert_close(z, z0, atol=3e-5, rtol=1e-5)


@gpu
def test_dense_layer_kernels_reject_bad_shapes():
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    dev = _dev()
    t = torch.zeros(64, 64, device=dev)
    for M, K, N in [(8, 6, 8), (8, 8, 6), (4097, 8, 8)]:
        with pytest.raises(Exception, match="fn_dense_fwd_f32"):
            _lib.call("fn_dense_fwd_f32", t.data_ptr(), t.data_ptr(), None, t.data_ptr(), M, K, N, None, _stream_ptr(dev))


@gpu
@pytest.mark.parametrize("p,n_classes", [(0.0, 1), (0.1, 1), (0.2, 12)])
def test_fused_head_equals_layer_by_layer_path(p, n_classes):
    """Same Philox draws in the same order: the fused node must reproduce the unfused path (outputs and all grads)."""
    from fragnet_amd import ops
    from fragnet_amd.model import FTHead3
    dev = _dev()
    torch.manual_seed(3)
    head_a = FTHead3(input_dim=128, drop_ratio=p, n_classes=n_classes).to(dev).train()
    head_b = copy.deepcopy(head_a)
    x_a = torch.randn(64, 256, device=dev, requires_grad=True)
    x_b = x_a.detach().clone().requires_grad_(True)
    head_a.rng, head_b.rng = ops.PhiloxStream(seed=11), ops.PhiloxStream(seed=11)
    out_a = head_a(x_a)                                            # fused (ops.mlp_head)

    h = x_b                                                        # the loop _PredictorStack._run falls back to
    for lin in head_b.predictor[:-1]:
        h = ops.dropout_act(lin(h), p, True, True, head_b.rng)
    out_b = head_b.predictor[-1](h)
    torch.testing.assert_close(out_a, out_b, atol=1e-5, rtol=1e-5)
    t = torch.randn_like(out_a)
    (out_a * t).sum().backward()
    (out_b * t).sum().backward()
    torch.testing.assert_close(x_a.grad, x_b.grad, atol=1e-5, rtol=1e-4)
    for (n, pa), (_, pb) in zip(head_a.named_parameters(), head_b.named_parameters()):
        torch.testing.assert_close(pa.grad, pb.grad, atol=2e-5, rtol=1e-4, msg=lambda m, n=n: f"{n}: {m}")
    assert head_a.rng.offset == head_b.rng.offset


@gpu
def test_fused_head_skips_padding_rows():
    """live_rows (static-shape batches): rows behind it are not computed -- outputs and input gradients 0 there, everything
    else as if the input ended at live_rows."""
    from fragnet_amd import ops
    from fragnet_amd.model import FTHead3
    dev = _dev()
    torch.manual_seed(5)
    head_a = FTHead3(input_dim=128, drop_ratio=0.0, n_classes=1).to(dev).train()
    head_b = copy.deepcopy(head_a)
    x_a = torch.randn(80, 256, device=dev, requires_grad=True)
    x_b = x_a.detach()[:64].clone().requires_grad_(True)
    head_a.rng, head_b.rng = ops.PhiloxStream(seed=11), ops.PhiloxStream(seed=11)
    head_a.live_rows = 64
    out_a, out_b = head_a(x_a), head_b(x_b)
    assert out_a.shape == (80, 1) and torch.equal(out_a[:64], out_b) and not out_a[64:].any()
    t = torch.randn_like(out_a)
    (out_a * t).sum().backward()
    (out_b * t[:64]).sum().backward()
    assert torch.equal(x_a.grad[:64], x_b.grad) and not x_a.grad[64:].any()
    for (n, pa), (_, pb) in zip(head_a.named_parameters(), head_b.named_parameters()):
        assert torch.equal(pa.grad, pb.grad), n


@gpu
def test_fused_head_matches_plain_torch_without_dropout():
    from fragnet_amd import ops
    from fragnet_amd.model import FTHead3
    dev = _dev()
    torch.manual_seed(4)
    head = FTHead3(input_dim=128, drop_ratio=0.0, n_classes=1).to(dev).train()
    head.rng = ops.PhiloxStream(seed=1)
    x = torch.randn(33, 256, device=dev, requires_grad=True)
    out = head(x)
    h = x.detach().double()
    for lin in head.predictor[:-1]:
        h = torch.relu(h @ lin.weight.double().t() + lin.bias.double())
    ref = h @ head.predictor[-1].weight.double().t() + head.predictor[-1].bias.double()
    torch.testing.assert_close(out, ref.float(), atol=1e-5, rtol=1e-5)


@gpu
def test_parameter_gradients_are_written_into_the_flat_buffer():
    """Encoder and fused head write d loss / d param straight into FlatAdam's flat gradient buffer: after backward
    every live parameter's .grad is its slot (gather_grads has nothing to copy) and holds the same numbers as a
    run without slots."""
    from fragnet_amd import data, parallel, synth, train
    from fragnet_amd.model import FragNetFineTune
    dev = _dev()
    batch = data.batch_to(data.collate_fn(synth.synth_molecules(24, seed=5)), dev)
    torch.manual_seed(2)
    model = FragNetFineTune(n_classes=1, num_layer=2, drop_ratio=0.0, act="relu").to(dev).train()     # ReLU head: fused node
    ref = copy.deepcopy(model)

    def run(m):
        loss = train.compute_mse_loss(m(dict(batch)), batch["y"]) if hasattr(train, "compute_mse_loss") else \
            torch.nn.functional.mse_loss(m(dict(batch)).reshape(-1), batch["y"].reshape(-1).float())
        loss.backward()

    opt = parallel.FlatAdam.for_live_parameters(model, lambda: run(model), lr=1e-3)
    opt.zero_grad()
    run(model)
    names = {id(q): n for n, q in model.named_parameters()}
    base, elsewhere = opt.grad.data_ptr(), []
    for p, off in zip(opt.params, opt.offsets):
        assert off % 4 == 0                                        # every slot starts on a 16-byte boundary
        if p.grad.data_ptr() != base + 4 * off:
            elsewhere.append(names[id(p)])
    assert not elsewhere, f"gradients not in place: {elsewhere}"
    opt.gather_grads()
    run(ref)                                                       # no optimiser attached: ordinary .grad tensors
    live = [q for q in ref.parameters() if q.grad is not None]
    assert len(live) == len(opt.params)
    for q, p, off in zip(live, opt.params, opt.offsets):
        torch.testing.assert_close(opt.grad[off: off + p.numel()].view_as(q), q.grad, atol=1e-6, rtol=1e-5)


@gpu
def test_masked_mse_multi_matches_the_sum_of_single_losses():
    from fragnet_amd import ops
    dev = _dev()
    torch.manual_seed(6)
    sizes = [(28104, 1), (13872, 1), (528, 3)]
    outs = [torch.randn(b, t, device=dev, requires_grad=True) for b, t in sizes]
    ys = [torch.randn(b, t, device=dev) for b, t in sizes]
    ws = [(torch.rand(b, device=dev) > 0.1).float() for b, _ in sizes]
    scale = torch.tensor([0.9, 1.3], device=dev)
    loss = ops.masked_mse_multi([(2.0, 0), (1.0, 1), (1.0, -1)], scale, outs[0], ys[0], ws[0], outs[1], ys[1], ws[1], outs[2], ys[2], ws[2])
    loss.backward()
    refs = [o.detach().double().requires_grad_(True) for o in outs]

    def mse(o, y, w):
        return (w.double()[:, None] * (o - y.double()) ** 2).sum() / (w.double().sum() * o.shape[1])
    want = 2 * 0.9 * mse(refs[0], ys[0], ws[0]) + 1.3 * mse(refs[1], ys[1], ws[1]) + mse(refs[2], ys[2], ws[2])
    want.backward()
    assert abs(float(loss) - float(want)) < 1e-5 * max(1.0, abs(float(want)))
    for o, r in zip(outs, refs):
        torch.testing.assert_close(o.grad, r.grad.float(), atol=1e-7, rtol=1e-4)


@gpu
def test_masked_bce_matches_the_torch_formula():
    from fragnet_amd import ops
    dev = _dev()
    torch.manual_seed(8)
    B, T = 1040, 12
    out = torch.randn(B, T, device=dev) * 3
    out.requires_grad_(True)
    y = torch.randint(-1, 2, (B, T), device=dev).float()             # -1 = missing label
    w = (torch.arange(B, device=dev) < 1024).float()                  # padded molecules at the end
    loss = ops.masked_bce(out, y, w)
    loss.backward()
    ref = out.detach().double().requires_grad_(True)
    valid = (y > -0.5) & (w[:, None] > 0)
    mat = torch.nn.functional.binary_cross_entropy_with_logits(ref, y.clamp(min=0).double(), reduction="none")
    want = torch.where(valid, mat, torch.zeros_like(mat)).sum() / valid.sum()
    want.backward()
    assert abs(float(loss) - float(want)) < 2e-6
    torch.testing.assert_close(out.grad, ref.grad.float(), atol=1e-8, rtol=1e-4)


@gpu
def test_dense_bwd_with_no_input_rows_zeroes_the_padding_rows_without_reading_null():
    """M = 0 with g_x and M_out > 0: g_y / X may be NULL then; the input gradient's rows are all padding = 0,
    dW and db are 0."""
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    dev = _dev()
    K, N, M_out = 64, 32, 24
    w = torch.randn(N, K, device=dev)
    gx = torch.full((M_out, K), 7.0, device=dev)
    dW, db = torch.full((N, K), 7.0, device=dev), torch.full((N,), 7.0, device=dev)
    _lib.call("fn_dense_bwd_f32", None, None, w.data_ptr(), gx.data_ptr(), 1.25, dW.data_ptr(), db.data_ptr(), 0, K, N, M_out, _stream_ptr(dev))
    torch.cuda.synchronize()
    assert float(gx.abs().max()) == 0.0 and float(dW.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


@gpu
def test_fused_head_with_drop_probability_one_passes_no_gradient():
    """p = 1 drops everything: outputs are the last bias, every gradient below the last layer is exactly 0 (the gate scale
    must not be read as "no gate")."""
    from fragnet_amd import ops
    dev = _dev()
    torch.manual_seed(0)
    lins = [torch.nn.Linear(64, 32).to(dev), torch.nn.Linear(32, 32).to(dev), torch.nn.Linear(32, 2).to(dev)]
    x = torch.randn(20, 64, device=dev, requires_grad=True)
    out = ops.mlp_head(x, lins, 1.0, True, ops.PhiloxStream(seed=3))
    torch.testing.assert_close(out, lins[-1].bias.detach().expand(20, 2))
    out.sum().backward()
    assert float(x.grad.abs().max()) == 0.0
    for lin in lins[:-1]:
        assert float(lin.weight.grad.abs().max()) == 0.0 and float(lin.bias.grad.abs().max()) == 0.0
    torch.testing.assert_close(lins[-1].bias.grad, torch.full((2,), 20.0, device=dev))


@gpu
@pytest.mark.parametrize("rows", [(0, 5), (1, 31), (33, 64), (1000, 13337), (27001, 13872)])
def test_fused_towers_match_torch(rows):
    """ops.towers (csrc/tower.hip: PretrainTask's Linear(128->64)->ReLU->Linear(64->32)->ReLU->Linear(32->1) towers, two towers in
    one launch each way) against plain torch: outputs, input gradients, all six parameter gradients per tower; ragged tile
    tails, an empty tower, tall inputs (several tiles per workgroup in the backward)."""
    from fragnet_amd import ops
    dev = _dev()
    torch.manual_seed(sum(rows))
    mk = lambda: [torch.nn.Linear(128, 64).to(dev), torch.nn.Linear(64, 32).to(dev), torch.nn.Linear(32, 1).to(dev)]
    ta, tb = mk(), mk()
    xa = torch.randn(rows[0], 128, device=dev, requires_grad=True)
    xb = torch.randn(rows[1], 128, device=dev, requires_grad=True)
    assert ops.tower_ok(xa, ta) and ops.tower_ok(xb, tb)
    oa, ob = ops.towers([(xa, ta), (xb, tb)])
    ga, gb = torch.randn_like(oa), torch.randn_like(ob)
    torch.autograd.backward([oa, ob], [ga, gb])
    got = [xa.grad.clone(), xb.grad.clone()] + [q.grad.clone() for lin in ta + tb for q in (lin.weight, lin.bias)]
    for q in [xa, xb] + [q for lin in ta + tb for q in (lin.weight, lin.bias)]:
        q.grad = None
    ref = lambda x, lins: lins[2](torch.relu(lins[1](torch.relu(lins[0](x)))))
    ra, rb = ref(xa, ta), ref(xb, tb)
    torch.testing.assert_close(oa, ra.detach(), atol=2e-5, rtol=1e-5)
    torch.testing.assert_close(ob, rb.detach(), atol=2e-5, rtol=1e-5)
    torch.autograd.backward([ra, rb], [ga, gb])
    want = [xa.grad, xb.grad] + [q.grad for lin in ta + tb for q in (lin.weight, lin.bias)]
    for i, (g, w) in enumerate(zip(got, want)):
        scale = max(1.0, float(w.abs().max())) if w.numel() else 1.0
        torch.testing.assert_close(g, w, atol=3e-5 * scale, rtol=1e-4, msg=lambda m, i=i: f"tensor {i}: {m}")


@gpu
def test_pretrain_task_fused_towers_equal_the_generic_path():
    """FragNetPreTrain with the fused towers against the same model with `fused_towers = False` (ops.mlp_head on the tall inputs):
    the four outputs and every gradient."""
    from fragnet_amd import data, synth
    from fragnet_amd.model import FragNetPreTrain
    from fragnet_amd.train import pretrain_loss
    dev = _dev()
    b = data.batch_to(data.collate_fn_pt(synth.synth_molecules(24, seed=8, profile="esol", pretrain_targets=True)), dev)
    torch.manual_seed(2)
    model = FragNetPreTrain(num_layer=2, drop_ratio=0.0, edge_features=17).to(dev).train()
    res = []
    for fused in (True, False):
        model.head.fused_towers = fused
        for q in model.parameters():
            q.grad = None
        outs = model(dict(b))
        pretrain_loss(outs, b).backward()
        res.append(([o.detach().clone() for o in outs if o is not None], {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}))
    for a, c in zip(*[r[0] for r in res]):
        torch.testing.assert_close(a, c, atol=2e-5, rtol=1e-5)
    assert res[0][1].keys() == res[1][1].keys()
    for n in res[0][1]:
        torch.testing.assert_close(res[0][1][n], res[1][1][n], atol=2e-5, rtol=1e-3, msg=lambda m, n=n: f"{n}: {m}")


@gpu
@pytest.mark.parametrize("kind", ["mse", "bce"])
@pytest.mark.parametrize("M,M_out,K,C", [(512, 552, 512, 1), (1000, 1024, 512, 12), (5, 8, 128, 3), (64, 64, 1024, 4), (3, 3, 36, 16), (0, 4, 64, 2)])
def test_last_linear_with_loss_in_one_launch_equals_the_three_launches(kind, M, M_out, K, C):
    """fn_small_linear_loss_f32 + the riders of fn_dense_bwd_tail_f32 against fn_small_linear_f32 -> fn_masked_mse/bce_f32 ->
    fn_small_linear_bwd_f32: predictions, d loss / d out and the input gradient bit for bit (same operation order), the sums over
    rows (dW, db, the loss value) to rounding; padding rows (M .. M_out) have weight 0 and prediction 0."""
    from fragnet_amd import _lib
    from fragnet_amd.plan import _stream_ptr
    import ctypes as C_
    dev = _dev()
    torch.manual_seed(M + K + C)
    st = _stream_ptr(dev)
    x = torch.relu(torch.randn(M, K, device=dev))
    w, b = torch.randn(C, K, device=dev) * 0.1, torch.randn(C, device=dev)
    tgt = torch.randn(M_out, C, device=dev)
    if kind == "bce":
        tgt = (tgt > 0).float()
        tgt[torch.rand(M_out, C, device=dev) < 0.2] = -1.0                  # missing labels
    row_w = torch.zeros(M_out, device=dev)
    row_w[:M] = 1.0
    if M > 4:
        row_w[3] = 0.0                                                      # a real row the caller masks out
    if M == 0:                                                              # padding rows only: predictions 0, nothing to reduce
        y1, parts = torch.full((M_out, C), 7.0, device=dev), torch.empty(_lib.load().fn_small_linear_loss_ws(M_out), device=dev)
        _lib.call("fn_small_linear_loss_f32", None, w.data_ptr(), b.data_ptr(), tgt.data_ptr(), row_w.data_ptr(),
                  _lib.LOSS_MSE if kind == "mse" else _lib.LOSS_BCE, y1.data_ptr(), None, None, 1.25, parts.data_ptr(), 0, K, C, M_out, st)
        assert not y1.any()
        return
    # the three launches
    y0 = torch.empty(M_out, C, device=dev)
    _lib.call("fn_small_linear_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), y0.data_ptr(), M, K, C, M_out, st)
    loss0, g0 = torch.empty((), device=dev), torch.empty(M_out, C, device=dev)
    _lib.call("fn_masked_mse_f32" if kind == "mse" else "fn_masked_bce_f32", y0.data_ptr(), tgt.data_ptr(), row_w.data_ptr(), M_out, C,
              loss0.data_ptr(), g0.data_ptr(), st)
    gx0, dW0, db0 = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    _lib.call("fn_small_linear_bwd_f32", g0.data_ptr(), x.data_ptr(), w.data_ptr(), gx0.data_ptr(), dW0.data_ptr(), db0.data_ptr(), M, K, C,
              1.25, None, st)
    # one launch + riders in a dense backward launch (a 64 -> 32 layer whose own results must not change)
    y1, g1, gx1 = torch.full((M_out, C), 7.0, device=dev), torch.full((M, C), 7.0, device=dev), torch.full_like(x, 7.0)
    n_part = _lib.load().fn_small_linear_loss_ws(M_out)
    assert n_part == (M_out + 3) // 4
    parts = torch.full((n_part,), 7.0, device=dev)
    _lib.call("fn_small_linear_loss_f32", x.data_ptr(), w.data_ptr(), b.data_ptr(), tgt.data_ptr(), row_w.data_ptr(),
              _lib.LOSS_MSE if kind == "mse" else _lib.LOSS_BCE, y1.data_ptr(), g1.data_ptr(), gx1.data_ptr(), 1.25, parts.data_ptr(), M, K, C,
              M_out, st)
    assert torch.equal(y1, y0) and torch.equal(g1, g0[:M]) and torch.equal(gx1, gx0)
    gy, X, W2 = torch.randn(40, 32, device=dev), torch.relu(torch.randn(40, 64, device=dev)), torch.randn(32, 64, device=dev)
    ref = [torch.empty(40, 64, device=dev), torch.empty(32, 64, device=dev), torch.empty(32, device=dev)]
    _lib.call("fn_dense_bwd_f32", gy.data_ptr(), X.data_ptr(), W2.data_ptr(), ref[0].data_ptr(), 1.25, ref[1].data_ptr(), ref[2].data_ptr(),
              40, 64, 32, 40, st)
    got = [torch.empty_like(t) for t in ref]
    dW1, db1, loss1 = torch.full_like(w, 7.0), torch.full_like(b, 7.0), torch.full((), 7.0, device=dev)
    tail = _lib.SmallDw(g1.data_ptr(), x.data_ptr(), dW1.data_ptr(), db1.data_ptr(), parts.data_ptr(), loss1.data_ptr(), n_part, M, K, C)
    _lib.call("fn_dense_bwd_tail_f32", gy.data_ptr(), X.data_ptr(), W2.data_ptr(), got[0].data_ptr(), 1.25, got[1].data_ptr(), got[2].data_ptr(),
              40, 64, 32, 40, C_.byref(tail), st)
    for a, r in zip(got, ref):
        assert torch.equal(a, r)
    tol = 2e-4 * max(1.0, M / 500) ** 0.5 * float(g0.abs().max().clamp_min(1e-3))
    torch.testing.assert_close(dW1, dW0, atol=tol, rtol=1e-5)
    torch.testing.assert_close(db1, db0, atol=tol, rtol=1e-5)
    torch.testing.assert_close(loss1, loss0, atol=1e-6, rtol=1e-5)
    torch.testing.assert_close(dW1, (g0[:M].double().t() @ x.double()).float(), atol=tol, rtol=1e-5)
    # ... and against a float64 Linear + loss, which shares nothing with the kernels above.  Bounds to first order in u = 2^-24 (plus
    # the second-order term of the loss), worst case over any summation order:
    #   prediction   e_y = (4 ceil(K / 256) + 8) u (|x| |w|^T + |b|)               one wave per row: a lane chains 4 ceil(K / 256) products,
    #                                                                              six butterfly levels, the bias
    #   g_out        |dg/dy| e_y + 4 u |g| (+ 4 u / N for BCE)                     dg/dy = 2 w_row / (W C) for MSE, <= 1 / (4 N) for BCE
    #   loss         sum |g| e_y + sum |dg/dy| e_y^2 / 2 + (C + 2 + n_part + 8) u sum|term| / denom
    #                                                                              C terms per row, a 4-row tree, n_part partials
    #   dW           (error bound of g_out)^T |x| + (M + 2) u |g|^T |x|            an M-term sum per element
    u = 2.0 ** -24
    xd, wd, bd, td, rw = (t.double().cpu() for t in (x, w, b, tgt[:M], row_w[:M]))
    yl = (xd @ wd.t() + bd).requires_grad_(True)
    e_y = (4 * ((K + 255) // 256) + 8) * u * (xd.abs() @ wd.abs().t() + bd.abs())
    if kind == "mse":
        d = yl - td
        terms = rw[:, None] * d * d
        den = rw.sum() * C
        slope = (2.0 * rw / den)[:, None].expand(M, C)
        extra = 0.0
    else:
        valid = (td > -0.5) & (rw[:, None] > 0)
        mat = torch.nn.functional.binary_cross_entropy_with_logits(yl, td.clamp(min=0.0), reduction="none")
        terms = torch.where(valid, mat, torch.zeros_like(mat))
        den = valid.sum().double()
        slope = valid.double() / (4.0 * den)
        extra = 4 * u / float(den)
    loss64 = terms.sum() / den
    loss64.backward()
    g64 = yl.grad
    g_bound = slope * e_y + 4 * u * g64.abs() + extra
    loss_bound = float((g64.abs() * e_y).sum() + (slope * e_y * e_y).sum() / 2
                       + (C + 2 + n_part + 8) * u * terms.detach().abs().sum() / den)
    dW_bound = g_bound.t() @ xd.abs() + (M + 2) * u * (g64.abs().t() @ xd.abs())
    g_err, dW_err = (g1.double().cpu() - g64).abs(), (dW1.double().cpu() - g64.t() @ xd).abs()
    loss_err = abs(float(loss1) - float(loss64.detach()))
    print(f"float64 Linear + {kind}: loss error {loss_err:.2e} (bound {loss_bound:.2e}), g_out worst {float((g_err / g_bound.clamp_min(1e-300)).max()):.3f} x bound, "
          f"dW worst {float((dW_err / dW_bound.clamp_min(1e-300)).max()):.3f} x bound")
    assert loss_err <= loss_bound
    assert bool((g_err <= g_bound).all()) and bool((dW_err <= dW_bound).all())
    assert bool((db1.double().cpu() - g64.sum(0)).abs().le(g_bound.sum(0) + (M + 2) * u * g64.abs().sum(0)).all())


@gpu
@pytest.mark.parametrize("loss_kind,n_classes,p", [("regr", 1, 0.1), ("clsf", 12, 0.2), ("regr", 3, 0.0)])
def test_head_with_fused_loss_equals_head_then_loss(loss_kind, n_classes, p):
    """ops.mlp_head(loss=...) -- what GraphedTrainStep arms the head with -- against the head followed by the loss kernel: predictions
    and the input gradient bit for bit, loss and parameter gradients to rounding; padding rows behind live_rows."""
    from fragnet_amd import _lib, ops
    from fragnet_amd.graphstep import masked_bce_loss, masked_regr_loss
    from fragnet_amd.model import FTHead3
    dev = _dev()
    torch.manual_seed(9)
    head_a = FTHead3(input_dim=128, drop_ratio=p, n_classes=n_classes).to(dev).train()
    head_b = copy.deepcopy(head_a)
    x_a = torch.randn(80, 256, device=dev, requires_grad=True)
    x_b = x_a.detach().clone().requires_grad_(True)
    y = torch.randn(80, n_classes, device=dev)
    if loss_kind == "clsf":
        y = (y > 0).float()
        y[torch.rand_like(y) < 0.2] = -1.0
    w = torch.zeros(80, device=dev)
    w[:70] = 1.0
    head_a.rng, head_b.rng = ops.PhiloxStream(seed=11), ops.PhiloxStream(seed=11)
    head_a.live_rows = head_b.live_rows = 70
    unit = ops.unit_grad(dev)
    head_a.loss_spec = (_lib.LOSS_MSE if loss_kind == "regr" else _lib.LOSS_BCE, y, w)
    out_a = head_a(x_a)
    head_a.loss_spec = None
    loss_a, y_seen, w_seen = out_a._fragnet_loss
    assert y_seen is y and w_seen is w and not out_a.requires_grad
    loss_a.backward(gradient=unit)
    out_b = head_b(x_b)
    loss_b = (masked_regr_loss if loss_kind == "regr" else masked_bce_loss)(out_b, y, w)
    loss_b.backward(gradient=unit)
    assert torch.equal(out_a, out_b) and torch.equal(x_a.grad, x_b.grad)
    torch.testing.assert_close(loss_a, loss_b, atol=1e-6, rtol=1e-5)
    for (n, pa), (_, pb) in zip(head_a.named_parameters(), head_b.named_parameters()):
        torch.testing.assert_close(pa.grad, pb.grad, atol=1e-6, rtol=1e-5, msg=lambda m, n=n: f"{n}: {m}")
    # a gradient other than the persistent 1 scales everything but the loss value
    head_c = copy.deepcopy(head_b)
    head_c.zero_grad()
    head_c.rng = ops.PhiloxStream(seed=11)
    x_c = x_a.detach().clone().requires_grad_(True)
    head_c.loss_spec = (_lib.LOSS_MSE if loss_kind == "regr" else _lib.LOSS_BCE, y, w)
    loss_c = head_c(x_c)._fragnet_loss[0]
    head_c.loss_spec = None
    (loss_c * 3.0).backward()
    torch.testing.assert_close(x_c.grad, 3.0 * x_b.grad, atol=1e-7, rtol=1e-5)
    torch.testing.assert_close(loss_c, loss_b, atol=1e-6, rtol=1e-5)
    torch.testing.assert_close(head_c.predictor[-1].weight.grad, 3.0 * head_b.predictor[-1].weight.grad, atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ the tall route of ops.mlp_head
# (library GEMMs around fn_dropout_act_f32 / fn_gate_colsum_f32: an input width that is no multiple of 4, more than DENSE_MAX_ROWS
# rows, or ops.DENSE_HEAD off), on the smallest shapes that reach each of its branches
TALL_CASES = {
    "odd_input_small_last": ((5, 6), (6, 8, 4, 3), 0.25),      # hidden layers tall, last Linear on the small kernel without a gate
    "wide_last": ((5, 6), (6, 8, 20), 0.25),                   # last Linear wider than SMALL_LINEAR_MAX: addmm / mm / sum
    "many_rows": ((4100, 8), (8, 8, 1), 0.1),                  # > DENSE_MAX_ROWS rows; > 2048: the chunked workspaces of both kernels
}


class _PaddedDraws:
    """A PhiloxStream whose draws are sized as if the input had ``padded`` rows instead of ``rows`` (mlp_head draws per padded row)."""

    def __init__(self, stream, rows, padded):
        self.stream, self.rows, self.padded = stream, rows, padded

    dev = None

    def take(self, numel):
        assert numel % self.rows == 0
        return self.stream.take(numel // self.rows * self.padded)


def _linears(dims, dev, seed=3):
    torch.manual_seed(seed)
    return [torch.nn.Linear(dims[i], dims[i + 1]).to(dev) for i in range(len(dims) - 1)]


def _loop_head(x, lins, p, rng):
    """the layer-by-layer loop of test_fused_head_equals_layer_by_layer_path"""
    from fragnet_amd import ops
    h = x
    for lin in lins[:-1]:
        h = ops.dropout_act(lin(h), p, True, True, rng)
    return lins[-1](h)


def _float64_head(x, lins, live=None):
    """relu between the Linears in float64 on the CPU (p = 0); rows behind ``live`` are padding: output 0, no gradient"""
    xd = x.detach().cpu().double().requires_grad_(True)
    ps = [(lin.weight.detach().cpu().double().requires_grad_(True), lin.bias.detach().cpu().double().requires_grad_(True)) for lin in lins]
    h = xd if live is None else xd[:live]
    for i, (w, b) in enumerate(ps):
        h = h @ w.t() + b
        if i < len(ps) - 1:
            h = torch.relu(h)
    if live is not None:
        h = torch.cat([h, h.new_zeros((x.shape[0] - live, h.shape[1]))])
    return h, xd, [q for wb in ps for q in wb]


def _backward(out, t, x, lins):
    """(input gradient, parameter gradients) of sum(out * t), the parameters' .grad cleared afterwards"""
    (out * t.to(out.device, out.dtype)).sum().backward()
    got = x.grad, [q.grad for lin in lins for q in (lin.weight, lin.bias)]
    for lin in lins:
        lin.weight.grad = lin.bias.grad = None
    return got


def _assert_head_close(got, want):
    """(out, input gradient, parameter gradients) at the tolerances of test_fused_head_equals_layer_by_layer_path"""
    torch.testing.assert_close(got[0], want[0].to(got[0].device, torch.float32), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(got[1], want[1].to(got[1].device, torch.float32), atol=1e-5, rtol=1e-4)
    assert len(got[2]) == len(want[2])
    for i, (a, b) in enumerate(zip(got[2], want[2])):
        torch.testing.assert_close(a, b.to(a.device, torch.float32), atol=2e-5, rtol=1e-4, msg=lambda m, i=i: f"parameter {i}: {m}")


def _mlp_head_run(x0, lins, p, t, rng, live=None):
    from fragnet_amd import ops
    x = x0.detach().clone().requires_grad_(True)
    out = ops.mlp_head(x, lins, p, True, rng, live)
    return (out.detach(), *_backward(out, t, x, lins))


def _check_against_float64(x0, lins, t, live=None):
    from fragnet_amd import ops
    rng = ops.PhiloxStream(seed=11)
    got = _mlp_head_run(x0, lins, 0.0, t, rng, live)
    assert rng.offset == 0
    ref, xd, ps = _float64_head(x0, lins, live)
    (ref * t.cpu().double()).sum().backward()
    _assert_head_close(got, (ref.detach(), xd.grad, [q.grad for q in ps]))


@gpu
@pytest.mark.parametrize("case", list(TALL_CASES))
def test_tall_head_equals_layer_by_layer_path_and_float64(case):
    """ops.mlp_head where the hidden layers take library GEMMs: outputs, input gradient, every parameter gradient and the stream's
    final offset against the layer-by-layer loop under the same Philox draws, and against float64 torch without dropout."""
    from fragnet_amd import ops
    dev = _dev()
    shape, dims, p = TALL_CASES[case]
    lins = _linears(dims, dev)
    assert ops.head_route(shape[0], lins, ops._lib.ACT_RELU) == "tall"
    x0 = torch.randn(shape, device=dev)
    t = torch.randn(shape[0], dims[-1], device=dev)
    rng_a, rng_b = ops.PhiloxStream(seed=11), ops.PhiloxStream(seed=11)
    got = _mlp_head_run(x0, lins, p, t, rng_a)
    x_b = x0.detach().clone().requires_grad_(True)
    out_b = _loop_head(x_b, lins, p, rng_b)
    _assert_head_close(got, (out_b.detach(), *_backward(out_b, t, x_b, lins)))
    assert rng_a.offset == rng_b.offset == sum((shape[0] * w + 3) // 4 for w in dims[1:-1])
    _check_against_float64(x0, lins, t)


@gpu
@pytest.mark.parametrize("p", [0.25, 0.0])
def test_tall_head_skips_padding_rows(p):
    """live rows on the tall route, bit for bit as test_fused_head_skips_padding_rows: nine rows of which five are live against the
    five alone (whose stream draws per padded row, as the head's does)."""
    from fragnet_amd import ops
    dev = _dev()
    dims = (6, 8, 4, 3)
    lins = _linears(dims, dev)
    x0 = torch.randn(9, 6, device=dev)
    t = torch.randn(9, 3, device=dev)
    rng_a, rng_b = ops.PhiloxStream(seed=11), ops.PhiloxStream(seed=11)
    out_a, gx_a, gp_a = _mlp_head_run(x0, lins, p, t, rng_a, live=5)
    out_b, gx_b, gp_b = _mlp_head_run(x0[:5], lins, p, t[:5], _PaddedDraws(rng_b, 5, 9))
    assert out_a.shape == (9, 3) and torch.equal(out_a[:5], out_b) and not out_a[5:].any()
    assert gx_a.shape == (9, 6) and torch.equal(gx_a[:5], gx_b) and not gx_a[5:].any()
    for i, (a, b) in enumerate(zip(gp_a, gp_b)):
        assert torch.equal(a, b), i
    assert rng_a.offset == rng_b.offset == (sum((9 * w + 3) // 4 for w in dims[1:-1]) if p else 0)
    if not p:
        _check_against_float64(x0, lins, t, live=5)


@gpu
@pytest.mark.parametrize("dense_head,K", [(True, 8), (False, 8), (False, 6)], ids=["dense_head_on", "dense_head_off", "library_last_linear"])
def test_single_linear_head_with_padding_rows(dense_head, K):
    """One Linear (no hidden layer) with live rows: its input gradient is the head's own, all rows of it, padding rows 0.  K = 8 runs
    the small kernel each way whatever ops.DENSE_HEAD says (with no hidden layer there is nothing for the flag to decide); K = 6
    is the library GEMM with the padding rows concatenated."""
    from fragnet_amd import ops
    dev = _dev()
    lins = _linears((K, 3), dev)
    x0 = torch.randn(5, K, device=dev)
    t = torch.randn(5, 3, device=dev)
    before = ops.DENSE_HEAD
    try:
        ops.DENSE_HEAD = dense_head
        assert ops.head_route(3, lins, ops._lib.ACT_RELU) == ("dense" if K == 8 else "tall")
        rng = ops.PhiloxStream(seed=11)
        out_a, gx_a, gp_a = _mlp_head_run(x0, lins, 0.25, t, rng, live=3)
        out_b, gx_b, gp_b = _mlp_head_run(x0[:3], lins, 0.25, t[:3], ops.PhiloxStream(seed=11))
        assert rng.offset == 0
        assert out_a.shape == (5, 3) and torch.equal(out_a[:3], out_b) and not out_a[3:].any()
        assert gx_a.shape == (5, K) and torch.equal(gx_a[:3], gx_b) and not gx_a[3:].any()
        for i, (a, b) in enumerate(zip(gp_a, gp_b)):
            assert torch.equal(a, b), i
        _check_against_float64(x0, lins, t, live=3)
    finally:
        ops.DENSE_HEAD = before


@gpu
def test_fthead3_on_the_tall_route_equals_the_dense_route():
    """FTHead3 with ops.DENSE_HEAD off (what bench.py --library-head measures) against the same head on the dense kernels."""
    from fragnet_amd import ops
    from fragnet_amd.model import FTHead3
    dev = _dev()
    torch.manual_seed(3)
    head_a = FTHead3(input_dim=128, drop_ratio=0.1, n_classes=1).to(dev).train()
    head_b = copy.deepcopy(head_a)
    x0 = torch.randn(64, 256, device=dev)
    t = torch.randn(64, 1, device=dev)
    res = []
    before = ops.DENSE_HEAD
    try:
        for head, flag in ((head_a, False), (head_b, True)):
            ops.DENSE_HEAD = flag
            assert ops.head_route(64, list(head.predictor), ops._lib.ACT_RELU) == ("dense" if flag else "tall")
            head.rng = ops.PhiloxStream(seed=11)
            x = x0.detach().clone().requires_grad_(True)
            out = head(x)
            res.append((out.detach(), *_backward(out, t, x, list(head.predictor))))
    finally:
        ops.DENSE_HEAD = before
    _assert_head_close(res[0], res[1])
    assert head_a.rng.offset == head_b.rng.offset > 0


# ------------------------------------------------------------------------------------------------ the route decision (host only)
def _stack(*dims, bias=True):
    return [torch.nn.Linear(dims[i], dims[i + 1], bias=bias) for i in range(len(dims) - 1)]


def _strided(lin):
    lin.weight = torch.nn.Parameter(torch.zeros(lin.in_features, lin.out_features).t())
    assert not lin.weight.is_contiguous()
    return lin


def test_head_route_table():
    """ops.head_route: which node a head runs on -- rows, widths, strides, biases, the activation kind and ops.DENSE_HEAD."""
    from fragnet_amd import _lib, ops
    relu, others = _lib.ACT_RELU, [_lib.ACT_SILU, _lib.ACT_GELU, _lib.ACT_CELU, _lib.ACT_SELU, _lib.ACT_RELU6, _lib.ACT_LEAKYRELU, _lib.ACT_PRELU]
    assert ops.DENSE_HEAD and ops.DENSE_MAX_ROWS == 4096 and ops.SMALL_LINEAR_MAX == 16

    def both(rows, lins, want_relu, want_others):
        assert ops.head_route(rows, lins) == ops.head_route(rows, lins, relu) == want_relu
        for kind in others:
            assert ops.head_route(rows, lins, kind) == want_others, kind

    for rows in (0, 1, 4096):
        both(rows, _stack(8, 8, 4, 3), "dense", "dense")
    both(4097, _stack(8, 8, 4, 3), "tall", None)
    both(4097, _stack(8, 3), "dense", "dense")                      # a single Linear: no hidden layer for the row bound to hold for
    both(5, _stack(6, 8, 4, 3), "tall", None)                       # first layer: input width
    both(5, _stack(8, 6, 4, 3), None, None)                         # first layer: output width
    both(5, _stack(8, 8, 6, 3), None, None)                         # a hidden layer's output width (= the last layer's input width)
    both(5, _stack(8, 8, 4, 16), "dense", "dense")                  # last layer: 16 / 17 outputs
    both(5, _stack(8, 8, 4, 17), "tall", None)
    both(5, _stack(8, 3), "dense", "dense")                         # last layer alone: input width
    both(5, _stack(6, 3), "tall", None)
    both(5, _stack(6, 17), "tall", None)
    lins = _stack(8, 8, 4, 3)
    _strided(lins[1])
    both(5, lins, "tall", None)                                     # a hidden weight that is not contiguous
    lins = _stack(8, 8, 4, 3)
    _strided(lins[-1])
    both(5, lins, "dense", "dense")                                 # (the last Linear's is made contiguous for its launch)
    for i in range(3):
        lins = _stack(8, 8, 4, 3)
        lins[i] = torch.nn.Linear(lins[i].in_features, lins[i].out_features, bias=False)
        both(5, lins, None, None)
    before = ops.DENSE_HEAD
    try:
        ops.DENSE_HEAD = False
        both(5, _stack(8, 8, 4, 3), "tall", None)
        both(5, _stack(8, 8, 6, 3), None, None)
        both(5, _stack(8, 3), "dense", "dense")                     # no hidden layer: nothing for the flag to decide
    finally:
        ops.DENSE_HEAD = before


def test_head_fuses_loss_table():
    """ops.head_fuses_loss: when mlp_head(loss=...) folds the loss into the last Linear's launch."""
    from fragnet_amd import _lib, ops
    lins = _stack(8, 8, 4, 3)

    def fuses(M=6, rows=5, lins=lins, route=None, grad=True, training=True, n_w=None, n_t=None):
        x = torch.zeros(M, lins[0].in_features, requires_grad=grad)
        loss = (_lib.LOSS_MSE, torch.zeros(M * lins[-1].out_features if n_t is None else n_t), torch.zeros(M if n_w is None else n_w))
        got = ops.head_fuses_loss(ops.head_route(rows, lins) if route is None else route, rows, x, lins, loss, training)
        assert isinstance(got, bool)
        return got

    before = ops.FUSED_HEAD_LOSS
    try:
        ops.FUSED_HEAD_LOSS = True
        _fuses_loss_rows(fuses)
        ops.FUSED_HEAD_LOSS = False
        assert not fuses()
    finally:
        ops.FUSED_HEAD_LOSS = before


def test_pair_fuses_loss_table():
    """ops.pair_fuses_loss: when a pair head (plain or factored) folds the MSE loss into its two launches."""
    from fragnet_amd import _lib, ops

    def fuses(rows=5, who=0, kind=_lib.LOSS_MSE, row_w=None, grad=True):
        # drug, second input, fc1.weight, fc1.bias, fc2.weight, fc2.bias; ``who``: the one that takes a gradient (None: none)
        tensors = [torch.zeros(3, requires_grad=(i == who)) for i in range(6)]
        with torch.set_grad_enabled(grad):
            got = ops.pair_fuses_loss((kind, torch.zeros(max(rows, 1)), row_w), rows, tensors)
        assert isinstance(got, bool)
        return got

    before = ops.FUSED_HEAD_LOSS
    try:
        ops.FUSED_HEAD_LOSS = True
        for rows in (1, 4096):
            assert fuses(rows, who=0) and fuses(rows, who=1) and all(fuses(rows, who=i) for i in (2, 3, 4, 5))
        assert not fuses(rows=0)                                    # nothing live
        assert not fuses(kind=_lib.LOSS_BCE)
        assert not fuses(row_w=torch.ones(5))
        assert not fuses(grad=False)                                # under torch.no_grad()
        assert not fuses(who=None)                                  # nothing takes a gradient
        ops.FUSED_HEAD_LOSS = False
        for rows in (1, 4096):
            assert not any(fuses(rows, who=i) for i in range(6))
        assert not fuses(rows=0) and not fuses(kind=_lib.LOSS_BCE) and not fuses(row_w=torch.ones(5)) and not fuses(grad=False) and not fuses(who=None)
    finally:
        ops.FUSED_HEAD_LOSS = before


def _fuses_loss_rows(fuses):
    assert fuses() and fuses(rows=6) and fuses(rows=1) and fuses(M=4096, rows=4096)
    assert not fuses(rows=0)                                        # nothing live
    assert not fuses(grad=False) and not fuses(training=False)
    assert not fuses(M=4100, rows=4097)                             # tall
    assert not fuses(lins=_stack(6, 8, 4, 3)) and not fuses(lins=_stack(8, 8, 4, 17)) and not fuses(route="tall")
    assert not fuses(lins=_stack(8, 3))                             # no hidden layer to carry the riders
    assert fuses(lins=_stack(8, 1024, 3)) and not fuses(lins=_stack(8, 1028, 3))        # SMALL_LINEAR_LOSS_MAX_K
    assert not fuses(n_w=5) and not fuses(n_t=6 * 3 - 1)            # one weight per padded row, one target per prediction
