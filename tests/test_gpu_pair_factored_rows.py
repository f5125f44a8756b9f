"""The factored pair head with a device-side real-pair count (csrc/pair_factored.hip, fn_*_pair_factored_fwd_rows_f32), both instances,
with the pair orderings of fn_pair_orderings_i32 under the same count and the existing, count-less backward.

A counted call on padded capacities -- 320 pairs of which the first ``n`` are real, ``U_cap`` drug rows of which ``U_real`` are real,
the same for the second side -- is compared with the PLAIN entry points on the real rows alone (``M = n``, ``U = U_real``,
``C = C_real``, orderings of ``ops.pair_orderings``).  ``out[:n]``, ``g[:n]``, the loss, the four parameter gradients and the real rows
of ``g_D`` / ``g_S`` must be EQUAL bit for bit: a real row keeps its tile and its statements, the divisor is ``n`` in both, every sum
over pairs walks a row's segment (the same segment) and every sum over rows puts row r in lane ``r mod L`` at the same place whatever
the row count is, where a padding row adds ``0 * x`` to an accumulator that started at +0.  Behind the real ones ``out``, ``g`` and the
rows of ``g_D`` / ``g_S`` must be exact zeros.  The padding rows of D and S hold finite random values a hundred times the real ones',
``y`` behind ``n`` is huge and the pair lists behind ``n`` hold garbage, in range and out of it, so a leak shows.  The last real drug
(where there are two or more) is referred to by no pair.  The capacities sit at the edges of the forward's 16-row tiles and the
backward's 64-row blocks.  The plain path is held once per instance to float64 torch on the gathered rows at the project's gradient
tolerance, |got - ref| <= 1e-4 + 1e-4 |ref|."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INSTANCES = {"cdrp": ("fn_cdrp_pair_factored", 256, True), "dta": ("fn_dta_pair_factored", 300, False)}
M_CAP = 320
COUNTS = (0, 1, 255, 256, 257, M_CAP)
ROWS = ((1, 16), (15, 16), (16, 32), (17, 80))          # (real, capacity)
SIDES = [(u, c) for u in ROWS for c in ROWS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _case(kind, n, U, C, seed):
    """the padded problem on the host: D [U_cap, 256], S [C_cap, K1], pair lists and y [M_CAP], the two Linears"""
    (U_real, U_cap), (C_real, C_cap), K1 = U, C, INSTANCES[kind][1]
    g = torch.Generator().manual_seed(seed)
    D, S = torch.randn(U_cap, 256, generator=g), torch.randn(C_cap, K1, generator=g)
    D[U_real:] *= 100.0
    S[C_real:] = S[C_real:].abs() * 100.0 + 1.0            # positive: CDRP's gate lets a leak through
    if kind == "cdrp":
        S = torch.relu(S)
    S[:, 3] = 0.0
    U_ref = max(1, U_real - 1)                             # the last real drug: no pair
    pd, ps = torch.randint(0, U_ref, (M_CAP,), generator=g), torch.randint(0, C_real, (M_CAP,), generator=g)
    y = torch.randn(M_CAP, generator=g)
    y[n:] = -3.0e6
    for pl, cap in ((pd, U_cap), (ps, C_cap)):             # behind n: garbage
        tail = torch.randint(0, cap, (M_CAP - n,), generator=g)
        tail[1::3] = -7
        tail[2::3] = (1 << 32) + 1
        pl[n:] = tail
    fc1, fc2 = torch.nn.Linear(256 + K1, 128), torch.nn.Linear(128, 1)
    return D, S, pd, ps, y, fc1, fc2


def _run(kind, D, S, pd, ps, y, fc1, fc2, count=None):
    """forward with the target, orderings, backward with the loss, at the C ABI.  ``count``: the counted forward and the orderings kernel
    under it; None: the plain forward and ops.pair_orderings."""
    from fragnet_amd import _lib, ops
    from fragnet_amd.plan import _stream_ptr
    prefix, K1, _ = INSTANCES[kind]
    (U, _), (C_, _), M = D.shape, S.shape, pd.numel()
    lib, st = _lib.load(), _stream_ptr(torch.device(DEV))
    t = [q.to(DEV).contiguous() for q in (D, S, pd, ps, fc1.weight.detach(), fc1.bias.detach(), fc2.weight.detach(), fc2.bias.detach(), y)]
    full = lambda *shape: torch.full(shape, 7.0, device=DEV)
    A, B, out, g, part, loss = full(U, 128), full(C_, 128), full(M), full(M), full(1), full(1)
    ws = torch.empty(getattr(lib, prefix + "_ws")(U, C_), device=DEV)
    args = [q.data_ptr() for q in t[:9]] + [A.data_ptr(), B.data_ptr(), ws.data_ptr(), out.data_ptr(), g.data_ptr(), part.data_ptr(),
                                            M, U, C_, 256, K1, 128, 1]
    if count is None:
        _lib.call(prefix + "_fwd_f32", *args, st)
        ords = ops.pair_orderings(t[2], U) + ops.pair_orderings(t[3], C_)
    else:
        _lib.call(prefix + "_fwd_rows_f32", *args, count.data_ptr(), st)
        ords = ops.pair_orderings_both(t[2], t[3], U, C_, real_pairs=count)
    grads = dict(g_D=full(U, 256), g_S=full(C_, K1), dW1=full(128, 256 + K1), db1=full(128), dW2=full(1, 128), db2=full(1))
    _lib.call(prefix + "_bwd_f32", g.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), A.data_ptr(), B.data_ptr(), t[4].data_ptr(), t[5].data_ptr(),
              t[6].data_ptr(), *[o.data_ptr() for o in ords], *[q.data_ptr() for q in grads.values()], part.data_ptr(), 1, loss.data_ptr(),
              M, U, C_, 256, K1, 128, 1, st)
    torch.cuda.synchronize()
    return dict(out=out, g=g, loss=loss, **grads)


PARAMS = ("dW1", "db1", "dW2", "db2")


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("U,C", SIDES)
@pytest.mark.parametrize("n", COUNTS)
def test_counted_factored_head_equals_the_plain_head_on_the_real_rows(kind, n, U, C):
    D, S, pd, ps, y, fc1, fc2 = _case(kind, n, U, C, 7000 + 97 * n + 11 * U[1] + C[1] + U[0])
    count = torch.tensor([n], dtype=torch.int32, device=DEV)
    got = _run(kind, D, S, pd, ps, y, fc1, fc2, count)
    assert bool((got["out"][n:] == 0).all()) and bool((got["g"][n:] == 0).all()), "out and g behind the count must be exactly 0"
    assert bool((got["g_D"][U[0]:] == 0).all()) and bool((got["g_S"][C[0]:] == 0).all()), "padding rows must hand back exact zeros"
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    if n == 0:
        assert float(got["loss"]) == 0.0
        assert all(bool((got[k] == 0).all()) for k in PARAMS + ("g_D", "g_S", "g", "out"))
        return
    want = _run(kind, D[:U[0]], S[:C[0]], pd[:n], ps[:n], y[:n], fc1, fc2)
    assert torch.equal(got["out"][:n], want["out"]), "out"
    assert torch.equal(got["g"][:n], want["g"]), "g"
    assert torch.equal(got["loss"], want["loss"]), "loss"
    for k in PARAMS:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["g_D"][:U[0]], want["g_D"]), "g_D"
    assert torch.equal(got["g_S"][:C[0]], want["g_S"]), "g_S"
    if U[0] > 1 and n > 0:
        assert bool((got["g_D"][U[0] - 1] == 0).all()), "a drug no pair refers to gets a zero gradient"


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_a_count_equal_to_the_capacity_is_the_plain_call(kind):
    D, S, pd, ps, y, fc1, fc2 = _case(kind, M_CAP, (17, 17), (16, 16), 5)
    a = _run(kind, D, S, pd, ps, y, fc1, fc2)
    b = _run(kind, D, S, pd, ps, y, fc1, fc2, torch.tensor([M_CAP], dtype=torch.int32, device=DEV))
    c = _run(kind, D, S, pd, ps, y, fc1, fc2, torch.tensor([M_CAP + 9], dtype=torch.int32, device=DEV))       # clamped
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_plain_factored_path_matches_float64_torch_on_the_gathered_rows(kind):
    n, U, C = 257, (17, 17), (16, 16)
    D, S, pd, ps, y, fc1, fc2 = _case(kind, n, U, C, 11)
    pd, ps, y = pd[:n], ps[:n], y[:n]
    got = _run(kind, D, S, pd, ps, y, fc1, fc2)
    r1, r2 = copy.deepcopy(fc1).double(), copy.deepcopy(fc2).double()
    d2, s2 = D.double().requires_grad_(True), S.double().requires_grad_(True)
    out = r2(r1(torch.cat((d2[pd], s2[ps]), 1))).view(-1)
    loss = torch.nn.functional.mse_loss(out, y.double())
    loss.backward()
    g_S = s2.grad * (S > 0) if INSTANCES[kind][2] else s2.grad
    want = dict(out=out.detach(), g=2.0 * (out.detach() - y.double()) / n, loss=loss.detach().view(1), g_D=d2.grad, g_S=g_S,
                dW1=r1.weight.grad, db1=r1.bias.grad, dW2=r2.weight.grad, db2=r2.bias.grad)
    for k, w in want.items():
        diff = (got[k].cpu().double() - w).abs()
        assert bool((diff <= 1e-4 + 1e-4 * w.abs()).all()), f"{k}: max |got - ref| = {float(diff.max()):.3e}"


def test_the_count_through_ops_and_its_refusals():
    """ops.pair_head_factored with (LOSS_MSE, y, None, count): the counted launch; a count where the fused launch does not apply raises."""
    from fragnet_amd import _lib, ops
    n, U, C = 40, (15, 16), (17, 80)
    D, S, pd, ps, y, fc1, fc2 = _case("cdrp", n, U, C, 23)
    fc1, fc2 = fc1.to(DEV), fc2.to(DEV)
    count = torch.tensor([n], dtype=torch.int32, device=DEV)

    def step(d, s, p_d, p_s, yy, cnt):
        f1, f2 = copy.deepcopy(fc1), copy.deepcopy(fc2)
        d, s = d.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(True)
        p_d, p_s = p_d.to(DEV), p_s.to(DEV)
        if cnt is None:
            out, loss = ops.pair_head_factored(d, s, p_d, p_s, f1, f2, loss=(_lib.LOSS_MSE, yy.to(DEV), None))
        else:
            ords = ops.pair_orderings_both(p_d, p_s, d.shape[0], s.shape[0], real_pairs=cnt)
            out, loss = ops.pair_head_factored(d, s, p_d, p_s, f1, f2, loss=(_lib.LOSS_MSE, yy.to(DEV), None, cnt), orderings=ords, check=False)
        assert loss is not None
        loss.backward()
        torch.cuda.synchronize()
        return out.detach(), loss.detach(), d.grad, s.grad, [q.grad for q in (f1.weight, f1.bias, f2.weight, f2.bias)]

    out, loss, g_d, g_s, grads = step(D, S, pd, ps, y, count)
    out_n, loss_n, g_d_n, g_s_n, grads_n = step(D[:U[0]], S[:C[0]], pd[:n], ps[:n], y[:n], None)
    assert torch.equal(out[:n], out_n) and torch.equal(loss, loss_n) and bool((out[n:] == 0).all())
    assert torch.equal(g_d[:U[0]], g_d_n) and torch.equal(g_s[:C[0]], g_s_n)
    assert bool((g_d[U[0]:] == 0).all()) and bool((g_s[C[0]:] == 0).all())
    for a, b in zip(grads, grads_n):
        assert torch.equal(a, b)
    d, s, yd = D.to(DEV).requires_grad_(True), S.to(DEV), y.to(DEV)
    ok_pd, ok_ps = pd.clamp(0, U[1] - 1).to(DEV), ps.clamp(0, C[1] - 1).to(DEV)
    with pytest.raises(_lib.FragnetHipError, match="real-row count"):      # a row weight: no fused launch
        ops.pair_head_factored(d, s, ok_pd, ok_ps, fc1, fc2, loss=(_lib.LOSS_MSE, yd, torch.ones(M_CAP, device=DEV), count))
    with torch.no_grad(), pytest.raises(_lib.FragnetHipError, match="real-row count"):      # no training step
        ops.pair_head_factored(d, s, ok_pd, ok_ps, fc1, fc2, loss=(_lib.LOSS_MSE, yd, None, count))
    with pytest.raises(TypeError, match="int32"):
        ops.pair_head_factored(d, s, ok_pd, ok_ps, fc1, fc2, loss=(_lib.LOSS_MSE, yd, None, count.long()))
    # the entry point itself: a count without a target is refused before anything is launched
    t = [q.detach().contiguous() for q in (d, s, ok_pd, ok_ps, fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
    A, B, out = torch.full((U[1], 128), 7.0, device=DEV), torch.full((C[1], 128), 7.0, device=DEV), torch.full((M_CAP,), 7.0, device=DEV)
    ws = torch.empty(_lib.load().fn_cdrp_pair_factored_ws(U[1], C[1]), device=DEV)
    rc = _lib.load().fn_cdrp_pair_factored_fwd_rows_f32(*[q.data_ptr() for q in t], None, A.data_ptr(), B.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                                        None, None, M_CAP, U[1], C[1], 256, 256, 128, 1, count.data_ptr(),
                                                        torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.FN_EINVAL and bool((A == 7.0).all()) and bool((out == 7.0).all())
