"""One attention level, ``ops.gat_level`` (HIP, through the C-ABI), against the oracle's materialised-message restatement of
gat2.py:146-169: the comparison that tests/test_gpu_gat_level_property.py runs over random graphs and
tests/test_gpu_launch_geometry.py over launch geometries.  Forward rows, probabilities, the by-source attention read-out and the gradient
of every input; tolerances as in test_gpu_parity.py (2e-5 absolute on O(1) rows, gradients 5e-5 x scale)."""
import torch

DEV = "cuda:0"


def _run(case):
    from fragnet_amd import ops
    from fragnet_amd.plan import GraphPlan
    from oracle.fragnet_ref import gat_level_materialised
    heads, mode, loops, n, m, dst, src, K = (case[k] for k in ("heads", "mode", "loops", "n", "m", "dst", "src", "K"))
    d = 128 // heads
    g = torch.Generator().manual_seed(case["seed"] ^ 0x5bd1e995)
    h = torch.randn(n, 128, generator=g)
    w_out = torch.randn(n, 128, generator=g)
    if mode == 2:
        att = torch.randn(heads, 3 * d, generator=g) * 0.3
        x = torch.randn(m, K, generator=g)
        embW = torch.randn(d, K, generator=g) * 0.5
        embb = torch.randn(d, generator=g) * 0.5
        inputs = (h, att, embW, embb)
    else:
        att = torch.randn(heads, 2 * d + 128, generator=g) * 0.3
        feat = torch.randn(m, 128, generator=g)
        inputs = (h, att, feat)

    # ---- oracle: the messages materialised, torch autograd
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    edge_vec = torch.nn.functional.linear(x, leaves[2], leaves[3]) if mode == 2 else leaves[2]
    rdst, rsrc = dst, src
    if loops:
        # add_self_loops: one loop per node behind the real edges.  Stored-row form (the atom graph, the only level the reference adds
        # loops to): the loop's row is zero.  Folded-Linear form: the loop's raw ATTRIBUTE is zero (x_sorted is 0 at loop positions,
        # include/fragnet_hip.h), so its edge vector is the Linear of zero = the bias.
        rdst = torch.cat([dst, torch.arange(n)])
        rsrc = torch.cat([src, torch.arange(n)])
        loop_vec = torch.nn.functional.linear(torch.zeros(n, K), leaves[2], leaves[3]) if mode == 2 else torch.zeros(n, edge_vec.shape[1])
        edge_vec = torch.cat([edge_vec, loop_vec])
    if rdst.numel():
        want, want_p, want_attn = gat_level_materialised(leaves[0].view(n, heads, d), edge_vec, leaves[1], rdst, rsrc, heads)
        if want.shape[0] < n:                        # scatter_add sizes its result by the largest destination id
            want = torch.cat([want, torch.zeros(n - want.shape[0], heads, d)])
        if want_attn.shape[0] < n:
            want_attn = torch.cat([want_attn, torch.zeros(n - want_attn.shape[0], heads)])
        want = want.reshape(n, 128)
        (want * w_out).sum().backward()
    else:                                            # no edge at all: zero rows, no gradient
        want, want_p, want_attn = torch.zeros(n, 128), torch.zeros(0, heads), torch.zeros(n, heads)

    # ---- HIP
    plan = GraphPlan([dict(kind="gat", name="l", dst=dst.to(DEV), src=src.to(DEV), n=n, n_loops=n if loops else 0)], DEV)
    lv = plan.levels["l"]
    dl = [t.detach().clone().to(DEV).requires_grad_(True) for t in inputs]
    if mode == 2:
        out, probs, p_sorted = ops.gat_level(dl[0], dl[1], lv, heads, x_sorted=plan.sorted_attr("l", x.to(DEV)), embW=dl[2], embb=dl[3],
                                             want_probs=True)
    else:
        out, probs, p_sorted = ops.gat_level(dl[0], dl[1], lv, heads, s_sorted=ops.row_dots_sorted(dl[2], dl[1], d, lv), want_probs=True)
    (out * w_out.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    plan.check()
    note = f"{case['shape']} H={heads} mode={mode} loops={loops} n={n} m={m} K={K}"
    assert torch.isfinite(out).all(), note
    torch.testing.assert_close(out.detach().cpu(), want.detach(), atol=2e-5, rtol=1e-4, msg=lambda s: f"out [{note}]: {s}")
    torch.testing.assert_close(probs.cpu().reshape(want_p.shape), want_p.detach(), atol=2e-6, rtol=1e-4, msg=lambda s: f"probs [{note}]: {s}")
    torch.testing.assert_close(ops.attn_by_src(p_sorted, lv, heads).cpu(), want_attn.detach(), atol=2e-5, rtol=1e-4,
                               msg=lambda s: f"attention by source [{note}]: {s}")
    for got, ref, nm in zip(dl, leaves, ("h", "att", "embW / feat", "embb")):
        rg = ref.grad if ref.grad is not None else torch.zeros_like(ref)
        gg = got.grad.cpu() if got.grad is not None else torch.zeros_like(ref)
        scale = max(1.0, float(rg.abs().max())) if rg.numel() else 1.0
        torch.testing.assert_close(gg, rg, atol=5e-5 * scale, rtol=1e-4, msg=lambda s: f"grad {nm} [{note}]: {s}")
