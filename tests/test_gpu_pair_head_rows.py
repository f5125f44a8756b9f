"""The pair head with a device-side real-row count (csrc/pair_head.hip, fn_*_pair_fwd_rows_f32; ops.pair_head / ops.pair_head_dta with
``loss = (LOSS_MSE, y, None, real_rows)``), both instances of the one kernel template.

A call on ``cap`` rows of which the first ``n`` are real is compared with the existing head called on those ``n`` rows alone.  The rows
behind ``n`` hold large finite values in both inputs and in ``y``, so a leak shows.  ``out[:n]``, the saved ``g[:n]`` and the loss must
be EQUAL: a real row keeps its tile, its statements and its divisor, and a padding row's loss partial is +0.  The parameter gradients
and the real rows of both input gradients must be equal too, because the order of additions over rows does not depend on the row
count: every sum over rows in k_pair_bwd and pair_last_tail walks ``m = lane, lane + stride, ..`` and then adds the lanes in a fixed
order, so row m sits in the same lane at the same place whatever M is, and a padding row adds g * x = (+-)0 there, which changes no
partial sum (the accumulators start at +0).  They are also held to a float64 torch reference at the kernel tolerance of
tests/test_gpu_cdrp.py: atol 2e-5 * max(1, max|want|), rtol 1e-5."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 3.0e3          # padding values: finite through fc1 / fc2 (|h| stays far below the fp32 range), large enough to wreck any sum they leak into

CASES = [(48, n) for n in (1, 15, 16, 17, 32, 33, 47, 48)] + [(16, n) for n in (0, 1, 16)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _close(got, want64, what):
    want = want64.float()
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    torch.testing.assert_close(got.cpu(), want, atol=2e-5 * scale, rtol=1e-5, msg=lambda m: f"{what}: {m}")


def _case(kind, M, seed):
    """tests/test_gpu_cdrp.py::_pair_case / tests/test_gpu_dta.py::_pair_case"""
    g = torch.Generator().manual_seed(seed)
    drug = torch.randn(M, 256, generator=g)
    if kind == "cdrp":
        second = torch.relu(torch.randn(M, 256, generator=g))
        second[:, 3] = 0.0
        second[0, :] = 0.0
        fc1 = torch.nn.Linear(512, 128)
    else:
        second = torch.randn(M, 300, generator=g)
        second[:, 3] = 0.0
        second[0, :] = 0.0
        second[:, 299] = -second[:, 299].abs() - 0.1
        fc1 = torch.nn.Linear(556, 128)
    fc2 = torch.nn.Linear(128, 1)
    y = torch.randn(M, generator=g)
    return drug, second, fc1, fc2, y


def _head(kind):
    from fragnet_amd import ops
    return ops.pair_head if kind == "cdrp" else ops.pair_head_dta


def _run(kind, drug, second, fc1, fc2, y, count=None):
    """One fused training call on the GPU: (out, loss, g_drug, g_second, [dW1, db1, dW2, db2], saved g)."""
    from fragnet_amd import _lib
    fc1, fc2 = copy.deepcopy(fc1).to(DEV), copy.deepcopy(fc2).to(DEV)
    d, s = drug.to(DEV).requires_grad_(True), second.to(DEV).requires_grad_(True)
    loss_spec = (_lib.LOSS_MSE, y.to(DEV), None) if count is None else (_lib.LOSS_MSE, y.to(DEV), None, count)
    out, loss = _head(kind)(d, s, fc1, fc2, loss=loss_spec)
    assert loss is not None
    saved_g = loss.grad_fn.saved_tensors[3].clone()            # _PairHead saves (drug, second, h, g, parts, loss)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), loss.detach(), d.grad, s.grad, [q.grad for q in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)], saved_g


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("cap,n", CASES)
def test_counted_head_equals_the_head_on_the_real_rows_alone(kind, cap, n):
    drug, second, fc1, fc2, y = _case(kind, cap, 1000 + 50 * cap + n)
    drug[n:], y[n:] = BIG, -BIG
    second[n:] = BIG if kind == "cdrp" else -BIG               # CDRP's second input is a ReLU output: positive, so the gate lets a leak through
    count = torch.tensor([n], dtype=torch.int32, device=DEV)
    out, loss, g_drug, g_sec, grads, g = _run(kind, drug, second, fc1, fc2, y, count)
    assert out.shape == (cap, 1) and bool(torch.isfinite(out).all())
    assert g.shape == (cap,) and bool((g[n:] == 0).all()), "g behind the count must be exactly 0"
    assert bool((g_drug[n:] == 0).all()) and bool((g_sec[n:] == 0).all()), "padding rows must hand back exact zeros"
    if n == 0:
        assert float(loss) == 0.0 and all(bool((q == 0).all()) for q in grads + [g_drug, g_sec, g])
        return
    out_n, loss_n, g_drug_n, g_sec_n, grads_n, g_n = _run(kind, drug[:n], second[:n], fc1, fc2, y[:n])
    assert torch.equal(out[:n], out_n) and torch.equal(g[:n], g_n) and torch.equal(loss, loss_n)
    # float64 reference of the n real rows
    r1, r2 = copy.deepcopy(fc1).double(), copy.deepcopy(fc2).double()
    d2, s2 = drug[:n].double().requires_grad_(True), second[:n].double().requires_grad_(True)
    torch.nn.functional.mse_loss(r2(r1(torch.cat((d2, s2), 1))).view(-1), y[:n].double()).backward()
    gate = (second[:n] != 0) if kind == "cdrp" else torch.ones_like(second[:n], dtype=torch.bool)
    _close(g_drug[:n], d2.grad, "g_drug")
    _close(g_sec[:n], s2.grad * gate, "g_second")
    for got, want, name in zip(grads, (r1.weight, r1.bias, r2.weight, r2.bias), ("dW1", "db1", "dW2", "db2")):
        _close(got, want.grad, name)
    # and bit for bit: the order of additions over rows does not depend on the row count (module docstring)
    assert torch.equal(g_drug[:n], g_drug_n) and torch.equal(g_sec[:n], g_sec_n)
    for got, want, name in zip(grads, grads_n, ("dW1", "db1", "dW2", "db2")):
        assert torch.equal(got, want), name


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_without_a_count_two_calls_agree_bit_for_bit(kind):
    drug, second, fc1, fc2, y = _case(kind, 48, 77)
    a, b = _run(kind, drug, second, fc1, fc2, y), _run(kind, drug, second, fc1, fc2, y)
    for x, z in zip(a[:4] + tuple(a[4]) + (a[5],), b[:4] + tuple(b[4]) + (b[5],)):
        assert torch.equal(x, z)
    # a count equal to the row count is the plain head
    c = _run(kind, drug, second, fc1, fc2, y, torch.tensor([48], dtype=torch.int32, device=DEV))
    for x, z in zip(a[:4] + tuple(a[4]) + (a[5],), c[:4] + tuple(c[4]) + (c[5],)):
        assert torch.equal(x, z)


def test_count_is_no_row_weight_and_needs_the_fused_launch():
    from fragnet_amd import _lib, ops
    drug, second, fc1, fc2, y = _case("cdrp", 16, 5)
    fc1, fc2, d, s, yd = fc1.to(DEV), fc2.to(DEV), drug.to(DEV).requires_grad_(True), second.to(DEV), y.to(DEV)
    count = torch.tensor([5], dtype=torch.int32, device=DEV)
    params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    assert ops.pair_fuses_loss((_lib.LOSS_MSE, yd, None), 16, (d, s, *params))
    assert ops.pair_fuses_loss((_lib.LOSS_MSE, yd, None, count), 16, (d, s, *params))
    w = torch.ones(16, device=DEV)
    assert not ops.pair_fuses_loss((_lib.LOSS_MSE, yd, w), 16, (d, s, *params))           # a row-WEIGHT tensor is still refused
    assert not ops.pair_fuses_loss((_lib.LOSS_MSE, yd, w, count), 16, (d, s, *params))
    with pytest.raises(_lib.FragnetHipError, match="real-row count"):
        ops.pair_head(d, s, fc1, fc2, loss=(_lib.LOSS_MSE, yd, w, count))
    with torch.no_grad(), pytest.raises(_lib.FragnetHipError, match="real-row count"):      # no training step: no fused launch
        ops.pair_head(d, s, fc1, fc2, loss=(_lib.LOSS_MSE, yd, None, count))
    with pytest.raises(TypeError, match="int32"):
        ops.pair_head(d, s, fc1, fc2, loss=(_lib.LOSS_MSE, yd, None, count.long()))
    # the entry point itself: a count without a target is refused before anything is launched
    h, out = torch.full((16, 128), 7.0, device=DEV), torch.full((16,), 7.0, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    t = [q.detach().contiguous() for q in (d, s, *params)]
    rc = _lib.load().fn_cdrp_pair_fwd_rows_f32(*[q.data_ptr() for q in t], None, h.data_ptr(), out.data_ptr(), None, None, 16, 256, 256, 128, 1,
                                               count.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == _lib.FN_EINVAL and bool((h == 7.0).all()) and bool((out == 7.0).all())
