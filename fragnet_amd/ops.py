"""torch.autograd wrappers around the C-ABI kernels (include/fragnet_hip.h).

PyTorch is plumbing here: it owns the device memory, the current HIP stream and the autograd tape.
Every numeric step of the message-passing path runs in libfragnet_hip.so; CPU tensors are rejected.

Operator surface mirrored from torch-scatter (the reference's fragnet/model/gat/gat2.py:5):
    scatter_add(src, index, dim=0, out=None, dim_size=None)
    scatter_softmax(src, index, dim=0, dim_size=None)
plus the fused per-level op the model uses (gat_level) and the small epilogues around it.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import os

import torch

from . import _lib
from ._lib import EdgeTerm, FN_D, FN_MAX_PART
from .plan import GraphPlan, Level, Segments, _stream_ptr

NEG_SLOPE = 0.2   # nn.LeakyReLU(0.2), reference gat2.py:83
BWD_ONE_PASS = True   # per-level operator path: the attention backward as one source-owner pass (False: destination + source pass)


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.FragnetHipError(f"{name}: fragnet_amd kernels need GPU tensors (got {t.device}); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def grad_slot(param):
    """The (flat gradient buffer, offset) parallel.FlatAdam assigned to ``param``, or None."""
    return getattr(param, "_fn_grad_slot", None)


def grad_buffer(param, slot):
    """Where a hand-written backward writes d loss / d param: the parameter's slot of the optimiser's flat gradient
    buffer when there is one, nothing has been accumulated yet and no other node of this backward pass has taken it
    (autograd then adopts the returned view as ``param.grad`` and FlatAdam.gather_grads finds it in place), else a
    fresh tensor.  The slot is handed out once per pass: a parameter that feeds two custom nodes (the model called on two
    batches before one ``backward()``) would otherwise have both kernels write the same memory and autograd add the
    tensor to its own alias (2 x the second gradient).  FlatAdam.zero_grad / gather_grads release the claims."""
    if slot is not None and param.grad is None and not getattr(param, "_fn_slot_claimed", False):
        flat, off = slot
        param._fn_slot_claimed = True
        return flat[off: off + param.numel()].view(param.shape)
    return torch.empty_like(param)


def _part_rows(n: int) -> int:
    return max(1, min((n + 7) // 8, FN_MAX_PART))


# ======================================================================================
# one attention level
# ======================================================================================
class _GatLevel(torch.autograd.Function):
    """out[n,128] = sum_e softmax_dst(LeakyReLU(s_dst + s_src + s_edge))_e * h[src_e].

    Inputs (differentiable): h [n,128]; att [H, att_w]; then either s_sorted [H,m] (mode 0: the edge term in
    destination-sorted order, head-major, from row_dots_sorted) or x_sorted [K,m] (mode 2: the raw edge attribute
    in destination-sorted order, not differentiated) with embW [d,K], embb [d]."""

    @staticmethod
    def forward(ctx, h, att, s_sorted, x_sorted, embW, embb, level: Level, heads: int, dst_off: int, mid_off: int,
                src_off: int, want_probs: bool):
        h = _f32c(h, "h")
        att = _f32c(att, "att")
        dev = h.device
        n, m = level.n, level.m
        if h.shape != (n, FN_D):
            raise ValueError(f"h must be [{n}, {FN_D}], got {tuple(h.shape)}")
        att_w = att.shape[1]
        mode = 0 if x_sorted is None else 2
        if mode == 0:
            s_sorted = _f32c(s_sorted, "s_sorted")
            if s_sorted.shape != (heads, m):
                raise ValueError(f"s_sorted must be head-major [{heads}, {m}], got {tuple(s_sorted.shape)}")
            et = EdgeTerm(0, 0, 0, 0, s_sorted.data_ptr(), None, None, None)
        else:
            x_sorted, embW, embb = _f32c(x_sorted, "x_sorted"), _f32c(embW, "embW"), _f32c(embb, "embb")
            K, d_e = x_sorted.shape[0], embW.shape[0]     # d_e = head_dim (gat2's a_b / f_a_b) or 128 (gat2_edge's f)
            if x_sorted.shape[1] != m or embW.shape[1] != K or embb.shape[0] != d_e or mid_off + d_e > src_off:
                raise ValueError("edge attribute / embedding shapes do not match the plan and the attention vector")
            et = EdgeTerm(2, K, d_e, mid_off, None, x_sorted.data_ptr(), embW.data_ptr(), embb.data_ptr())
        st = _stream_ptr(dev)
        s_dst = torch.empty((n, heads), dtype=torch.float32, device=dev)
        s_src = torch.empty((n, heads), dtype=torch.float32, device=dev)
        _lib.call("fn_node_scalars_f32", h.data_ptr(), att.data_ptr(), att_w, dst_off, src_off, s_dst.data_ptr(),
                  s_src.data_ptr(), n, heads, st)
        out = torch.empty((n, FN_D), dtype=torch.float32, device=dev)
        p_sorted = torch.empty((heads, m), dtype=torch.float32, device=dev)      # head-major
        probs = torch.empty((m, heads), dtype=torch.float32, device=dev) if want_probs else None
        # the one-pass backward (fn_gat_bwd_one_f32) needs the forward's second output row and its per-head weight sum
        # (levels beyond the one-pass kernel's 32-bit byte offsets keep the destination + source passes)
        one = BWD_ONE_PASS and any(ctx.needs_input_grad) and n <= (1 << 23) and m * heads <= (1 << 28)
        out2 = torch.empty((n, FN_D), dtype=torch.float32, device=dev) if one else None
        sigma = torch.empty((n, heads), dtype=torch.float32, device=dev) if one else None
        _lib.call("fn_gat_fwd_f32", h.data_ptr(), s_dst.data_ptr(), s_src.data_ptr(), att.data_ptr(), att_w,
                  C.byref(et), C.byref(level.c), NEG_SLOPE, out.data_ptr(), p_sorted.data_ptr(), _ptr(probs), _ptr(out2), _ptr(sigma),
                  0, None, heads, st)
        ctx.level, ctx.heads, ctx.mode = level, heads, mode
        ctx.offs = (dst_off, mid_off, src_off)
        ctx.one = one
        if one:
            ctx.save_for_backward(h, att, p_sorted, x_sorted, embW, embb, out, out2, sigma)
        else:
            ctx.save_for_backward(h, att, p_sorted, x_sorted, embW, embb)
        ctx.set_materialize_grads(False)
        if want_probs:
            ctx.mark_non_differentiable(probs, p_sorted)
            return out, probs, p_sorted
        return out

    @staticmethod
    def backward(ctx, g_out, *unused):
        h, att, p_sorted, x_sorted, embW, embb = ctx.saved_tensors[:6]
        level, heads, mode = ctx.level, ctx.heads, ctx.mode
        dst_off, mid_off, src_off = ctx.offs
        if g_out is None:
            return (None,) * 12
        g_out = _f32c(g_out, "g_out")
        dev = h.device
        n, m = level.n, level.m
        att_w = att.shape[1]
        st = _stream_ptr(dev)
        if mode == 0:
            et = EdgeTerm(0, 0, 0, 0, None, None, None, None)
            part_e = None
        else:
            K = x_sorted.shape[0]
            et = EdgeTerm(2, K, embW.shape[0], mid_off, None, x_sorted.data_ptr(), embW.data_ptr(), embb.data_ptr())
            part_e = torch.empty((FN_MAX_PART, heads * (K + 1)), dtype=torch.float32, device=dev)
        dz = torch.empty((heads, m), dtype=torch.float32, device=dev) if mode == 0 else None
        g_s_dst = torch.empty((n, heads), dtype=torch.float32, device=dev)
        n_e, n_a = C.c_int(0), C.c_int(0)
        g_h = torch.empty((n, FN_D), dtype=torch.float32, device=dev)
        part_a = torch.empty((FN_MAX_PART, 2 * FN_D), dtype=torch.float32, device=dev)
        if ctx.one:
            # one source-owner pass: c = <g, out> and g_s_dst = <g, out2> - c sigma are node-local (csrc/gat_bwd_one.inc)
            out, out2, sigma = ctx.saved_tensors[6:]
            cdot = torch.empty((n, heads), dtype=torch.float32, device=dev)
            _lib.call("fn_gat_cu_f32", g_out.data_ptr(), out.data_ptr(), out2.data_ptr(), sigma.data_ptr(), 1.0, cdot.data_ptr(),
                      g_s_dst.data_ptr(), n, heads, st)
            _lib.call("fn_gat_bwd_one_f32", g_out.data_ptr(), h.data_ptr(), p_sorted.data_ptr(), cdot.data_ptr(), g_s_dst.data_ptr(),
                      C.byref(et), att.data_ptr(), att_w, dst_off, src_off, C.byref(level.c), NEG_SLOPE, g_h.data_ptr(), _ptr(dz), None,
                      part_a.data_ptr(), C.byref(n_a), _ptr(part_e), C.byref(n_e), 0, None, heads, st)
        else:
            pz = torch.empty((heads, m, 2), dtype=torch.float32, device=dev)
            _lib.call("fn_gat_bwd_dst_f32", g_out.data_ptr(), h.data_ptr(), p_sorted.data_ptr(), C.byref(et),
                      C.byref(level.c), NEG_SLOPE, _ptr(dz), None, pz.data_ptr(), g_s_dst.data_ptr(), _ptr(part_e), C.byref(n_e), heads, st)
            _lib.call("fn_gat_bwd_src_f32", g_out.data_ptr(), h.data_ptr(), pz.data_ptr(), g_s_dst.data_ptr(), att.data_ptr(), att_w, dst_off, src_off, C.byref(level.c), g_h.data_ptr(),
                      part_a.data_ptr(), C.byref(n_a), heads, st)
        g_att = torch.zeros_like(att)
        g_embW = torch.empty_like(embW) if mode == 2 else None
        g_embb = torch.empty_like(embb) if mode == 2 else None
        _lib.call("fn_gat_bwd_finalize_f32", part_a.data_ptr(), n_a.value, _ptr(part_e), n_e.value, C.byref(et),
                  att.data_ptr(), att_w, dst_off, src_off, g_att.data_ptr(), _ptr(g_embW), _ptr(g_embb), heads, st)
        # dL/ds_sorted is dz itself (mode 0)
        return g_h, g_att, (dz if mode == 0 else None), None, g_embW, g_embb, None, None, None, None, None, None


def gat_level(h, att, level: Level, heads: int, *, s_sorted=None, x_sorted=None, embW=None, embb=None, want_probs=False):
    """``att`` = [dst(d) | edge | src(d)] per head, the reference's a_b / a / f / f_a_b layout."""
    d = FN_D // heads
    att_w = att.shape[1]
    return _GatLevel.apply(h, att, s_sorted, x_sorted, embW, embb, level, heads, 0, d, att_w - d, want_probs)


def attn_by_src(p_sorted: torch.Tensor, level: Level, heads: int) -> torch.Tensor:
    """scatter_add(attn_probs, source): attention mass per source node (gat2.py:165,219,268,312)."""
    out = torch.empty((level.n, heads), dtype=torch.float32, device=p_sorted.device)
    _lib.call("fn_attn_by_src_f32", p_sorted.data_ptr(), C.byref(level.c), out.data_ptr(), heads, _stream_ptr(out.device))
    return out


# ======================================================================================
# full-width edge term, destination-sorted: s_sorted[pos, j] = <feat[eid(pos), :], A[j, off:off+128]>
# ======================================================================================
class _RowDotsSorted(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, A, off: int, level: Level):
        feat, A = _f32c(feat, "feat"), _f32c(A, "A")
        J = A.shape[0]
        if feat.shape != (level.m_real, FN_D):
            raise ValueError(f"feat must be [{level.m_real}, {FN_D}], got {tuple(feat.shape)}")
        s = torch.empty((J, level.m), dtype=torch.float32, device=feat.device)      # head-major
        _lib.call("fn_row_dots_sorted_f32", feat.data_ptr(), A.data_ptr(), A.shape[1], off, J, C.byref(level.c), s.data_ptr(),
                  _stream_ptr(feat.device))
        ctx.off, ctx.level = off, level
        ctx.save_for_backward(feat, A)
        return s

    @staticmethod
    def backward(ctx, g_s):
        feat, A = ctx.saved_tensors
        level = ctx.level
        g_s = _f32c(g_s, "g_s")
        J = A.shape[0]
        st = _stream_ptr(feat.device)
        g_feat = torch.empty_like(feat)
        g_A = torch.zeros_like(A)
        if level.m_real:
            part = torch.empty((FN_MAX_PART, J * FN_D), dtype=torch.float32, device=feat.device)
            n_part = C.c_int(0)
            _lib.call("fn_row_dots_sorted_bwd_f32", g_s.data_ptr(), feat.data_ptr(), A.data_ptr(), A.shape[1], ctx.off, J,
                      C.byref(level.c), g_feat.data_ptr(), part.data_ptr(), C.byref(n_part), st)
            _lib.call("fn_colsum_f32", part.data_ptr(), n_part.value, J * FN_D, g_A.data_ptr(), A.shape[1], ctx.off, st)
        return g_feat, g_A, None, None


def row_dots_sorted(feat, A, off: int, level: Level):
    return _RowDotsSorted.apply(feat, A, off, level)


# ======================================================================================
# node projections on the fp32 matrix cores
# ======================================================================================
class _Linear128(torch.autograd.Function):
    """y = x @ W.T + b with W [128, K] (nn.Linear(K, 128)); K <= 168.  The input gradient is the K = 128 product kernel at K == 128
    (layers >= 1) and the ragged-width product of csrc/input_grad.hip (linear_dx) at every other K (layer 0)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x, weight, bias = _f32c(x, "x"), _f32c(weight, "weight"), _f32c(bias, "bias")
        M, K = x.shape
        if weight.shape != (FN_D, K) or bias.shape != (FN_D,):
            raise ValueError("linear128: weight must be [128, K], bias [128]")
        st = _stream_ptr(x.device)
        bt = torch.empty((K, FN_D), dtype=torch.float32, device=x.device)
        _lib.call("fn_transpose_w_f32", weight.data_ptr(), K, bt.data_ptr(), st)
        y = torch.empty((M, FN_D), dtype=torch.float32, device=x.device)
        _lib.call("fn_linear128_f32", x.data_ptr(), K, bt.data_ptr(), bias.data_ptr(), y.data_ptr(), M, None, st)
        ctx.save_for_backward(x, weight)
        ctx.x_needs_grad = x.requires_grad
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = _f32c(g, "g")
        M, K = x.shape
        st = _stream_ptr(x.device)
        gx = None
        if ctx.x_needs_grad:
            gx = torch.empty_like(x)
            if K != FN_D:
                linear_dx([(g, weight, gx, None, None)])
            else:
                _lib.call("fn_linear128_f32", g.data_ptr(), FN_D, weight.data_ptr(), None, gx.data_ptr(), M, None, st)
        ws = torch.empty(_lib.load().fn_linear128_wgrad_ws(M, K), dtype=torch.float32, device=x.device)
        gw = torch.empty_like(weight)
        gb = torch.empty(FN_D, dtype=torch.float32, device=x.device)
        _lib.call("fn_linear128_wgrad_f32", g.data_ptr(), x.data_ptr(), K, M, ws.data_ptr(), gw.data_ptr(), gb.data_ptr(), st)
        return gx, gw, gb


def linear128(x, weight, bias):
    return _Linear128.apply(x, weight, bias)


def linear_dx(tasks) -> None:
    """Up to three products ``dx = g @ W`` in one launch (fn_linear_dx_f32): the input gradient of ``nn.Linear(K, 128)`` for any
    1 <= K <= 168.  A task is ``(g [M, 128], W [128, K], dx_out, delta, dots_out)``: ``dx_out`` (None, or a contiguous float32 tensor
    of at least M * K elements) receives the rows unpadded, ``dots_out`` (None, or at least M elements) receives
    ``sum_k dx[m, k] * delta[m, k]`` in ascending k for the caller's ``delta [M, K]``.  Nothing past M * K / M elements is written."""
    if not 1 <= len(tasks) <= _lib.FN_MAX_DX_TASKS:
        raise ValueError(f"linear_dx: 1 to {_lib.FN_MAX_DX_TASKS} tasks")
    arr = (_lib.LinearDxTask * len(tasks))()
    keep = []
    dev = None
    for i, (g, W, dx, delta, dots) in enumerate(tasks):
        g, W = _f32c(g, "g"), _f32c(W, "weight")
        if g.dim() != 2 or g.shape[1] != FN_D or W.dim() != 2 or W.shape[0] != FN_D:
            raise ValueError("linear_dx: g must be [M, 128] and weight [128, K]")
        M, K = g.shape[0], W.shape[1]
        if delta is not None:
            delta = _f32c(delta, "delta")
            if tuple(delta.shape) != (M, K):
                raise ValueError(f"linear_dx: delta must be [{M}, {K}]")
        if dots is not None and delta is None:
            raise ValueError("linear_dx: dots needs a delta table")
        for out, need, name in ((dx, M * K, "dx_out"), (dots, M, "dots_out")):
            if out is not None and (not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < need):
                raise ValueError(f"linear_dx: {name} must be a contiguous float32 GPU tensor of at least {need} elements")
        dev = g.device
        keep.append((g, W, delta))
        arr[i] = _lib.LinearDxTask(_ptr(g) if M else None, _ptr(W), _ptr(dx) if M else None, _ptr(delta) if M else None,
                                   _ptr(dots) if M else None, M, K, 0)
    _lib.call("fn_linear_dx_f32", arr, len(tasks), _stream_ptr(dev))


# ======================================================================================
# segment sum (scatter_add along dim 0) and its gather backward
# ======================================================================================
class _SegmentSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, seg: Segments, keep_plan):
        src = _f32c(src, "src")
        if src.shape[0] != seg.n_items:
            raise ValueError(f"src has {src.shape[0]} rows, index has {seg.n_items}")
        width = 1
        for extent in src.shape[1:]:
            width *= int(extent)
        alloc = torch.zeros if seg.n_items == 0 else torch.empty
        out = alloc((seg.n_seg,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
        if seg.n_seg and width and seg.n_items:
            _lib.call("fn_segment_sum_f32", src.data_ptr(), width, seg.rowptr.data_ptr(), seg.perm.data_ptr(),
                      seg.pos_base, out.data_ptr(), seg.n_seg, width, seg.n_items, _stream_ptr(src.device))
        ctx.seg, ctx.width, ctx.keep = seg, width, keep_plan
        return out

    @staticmethod
    def backward(ctx, g_out):
        seg, width = ctx.seg, ctx.width
        g_out = _f32c(g_out, "g_out")
        g_src = torch.empty((seg.n_items,) + tuple(g_out.shape[1:]), dtype=torch.float32, device=g_out.device)
        if seg.n_items and width:
            _lib.call("fn_gather_rows_f32", g_out.data_ptr(), seg.index.data_ptr(), g_src.data_ptr(), seg.n_items, width,
                      _stream_ptr(g_out.device))
        return g_src, None, None


def segment_sum(src, seg: Segments, plan=None):
    return _SegmentSum.apply(src, seg, plan)


def _seg_struct(seg: Segments):
    return _lib.SegPlan(seg.rowptr.data_ptr(), seg.perm.data_ptr(), seg.index.data_ptr(), seg.n_seg, seg.n_items, seg.pos_base, 0)


class _PoolCat(torch.autograd.Function):
    """cat(scatter_add(x_atoms, batch), scatter_add(x_frags, frag_batch), dim=1) -> [B, 256] (gat2.py:820-823): one
    launch forward, one launch backward (two segment sums + cat, and two strided copies + two gathers, otherwise)."""

    @staticmethod
    def forward(ctx, x_atoms, x_frags, plan):
        x_atoms, x_frags = _f32c(x_atoms, "x_atoms"), _f32c(x_frags, "x_frags")
        sa, sf = plan.segs["mol_atoms"], plan.segs["mol_frags"]
        if x_atoms.shape[0] != sa.n_items or x_frags.shape[0] != sf.n_items or x_atoms.shape[1] != FN_D or x_frags.shape[1] != FN_D:
            raise ValueError("pool_cat: feature tables do not match the batch / frag_batch index")
        out = torch.empty((sa.n_seg, 2 * FN_D), dtype=torch.float32, device=x_atoms.device)
        a, f = _seg_struct(sa), _seg_struct(sf)
        _lib.call("fn_pool_cat_f32", x_atoms.data_ptr(), x_frags.data_ptr(), C.byref(a), C.byref(f), out.data_ptr(),
                  _stream_ptr(x_atoms.device))
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        sa, sf = plan.segs["mol_atoms"], plan.segs["mol_frags"]
        g = _f32c(g, "g")
        g_atoms = torch.empty((sa.n_items, FN_D), dtype=torch.float32, device=g.device)
        g_frags = torch.empty((sf.n_items, FN_D), dtype=torch.float32, device=g.device)
        _lib.call("fn_pool_cat_bwd_f32", g.data_ptr(), sa.index.data_ptr(), sf.index.data_ptr(), g_atoms.data_ptr(),
                  g_frags.data_ptr(), sa.n_items, sf.n_items, _stream_ptr(g.device))
        return g_atoms, g_frags, None


def pool_cat(x_atoms, x_frags, plan):
    return _PoolCat.apply(x_atoms, x_frags, plan)


def _readout_args(fn, x_atoms, x_frags, plan, vectors, check):
    """What ``pool_cat_groups`` and ``pool_cat_coalitions`` check alike.  ``vectors``: (tensor, name, dtype) of the per-atom vector
    (one entry per atom), of ``row_mol`` (its length is R) and of the per-row vector (R entries), in that order.
    Returns the feature tables, the two segment plans and the empty result [R, 256]."""
    x_atoms, x_frags = _f32c(x_atoms, "x_atoms"), _f32c(x_frags, "x_frags")
    dev = x_atoms.device
    for t, name, _ in vectors:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.FragnetHipError(f"{fn}: {name} must be a GPU tensor; there is no CPU fallback")
    sa, sf = plan.segs["mol_atoms"], plan.segs["mol_frags"]
    if x_atoms.shape != (sa.n_items, FN_D) or x_frags.shape != (sf.n_items, FN_D):
        raise ValueError(f"{fn}: feature tables do not match the batch / frag_batch index")
    row_mol = vectors[1][0]
    R = int(row_mol.shape[0])
    for (t, name, dtype), rows in zip(vectors, (sa.n_items, None, R)):
        if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.device != dev or (rows is not None and t.shape[0] != rows):
            raise ValueError(f"{fn}: {name} must be a contiguous {dtype} vector" + (f" of {rows} entries" if rows is not None else "")
                             + f" on {dev}")
    if check and R and bool(((row_mol < 0) | (row_mol >= sa.n_seg)).any()):
        raise IndexError(f"{fn}: row_mol must lie in [0, {sa.n_seg}) (got {int(row_mol.min())} .. {int(row_mol.max())})")
    return x_atoms, x_frags, sa, sf, torch.empty((R, 2 * FN_D), dtype=torch.float32, device=dev)


def pool_cat_groups(x_atoms, x_frags, plan, atom_group, row_mol, row_group, check: bool = True):
    """The leave-group-out read-out (fn_pool_cat_groups_f32): row r of the result [R, 256] is ``pool_cat``'s row of molecule
    ``row_mol[r]`` without the atoms i with ``atom_group[i] == row_group[r]`` (``row_group[r] < 0``: the unmasked row; an atom with
    ``atom_group < 0`` is in no group).  ``atom_group`` int64 [N], ``row_mol`` int32 [R], ``row_group`` int64 [R], on the batch's
    device.  An evaluation read-out: no autograd node.  ``row_mol`` is checked here, on the host (one synchronisation: the kernel has
    no status word); ``check=False``: the caller built ``row_mol`` on the host and has checked it there."""
    vectors = ((atom_group, "atom_group", torch.int64), (row_mol, "row_mol", torch.int32), (row_group, "row_group", torch.int64))
    x_atoms, x_frags, sa, sf, out = _readout_args("pool_cat_groups", x_atoms, x_frags, plan, vectors, check)
    if out.shape[0] == 0:
        return out
    a, f = _seg_struct(sa), _seg_struct(sf)
    _lib.call("fn_pool_cat_groups_f32", x_atoms.data_ptr(), x_frags.data_ptr(), C.byref(a), C.byref(f), atom_group.data_ptr(),
              row_mol.data_ptr(), row_group.data_ptr(), out.shape[0], out.data_ptr(), _stream_ptr(out.device))
    return out


def pool_cat_coalitions(x_atoms, x_frags, plan, atom_bit, row_mol, row_mask, check: bool = True):
    """The coalition read-out (fn_pool_cat_coalitions_f32): row r of the result [R, 256] is ``pool_cat``'s row of molecule
    ``row_mol[r]`` over the atoms i with ``atom_bit[i] < 0`` (in no group: always present) or bit ``atom_bit[i]`` of ``row_mask[r]``
    set; the fragments' half is never masked.  ``atom_bit`` int8 [N] (the position 0..63 of the atom's group among its molecule's
    groups), ``row_mol`` int32 [R], non-decreasing, ``row_mask`` int64 [R] (the 64 bits of the mask; bit 63 is the sign bit), on
    the batch's device.  An evaluation read-out: no autograd node.  ``check=True`` validates ``row_mol`` (range, order) and
    ``atom_bit`` (< 64) here, on the host (one synchronisation: the kernel has no status word); ``check=False``: the caller built
    them on the host and has checked them there."""
    vectors = ((atom_bit, "atom_bit", torch.int8), (row_mol, "row_mol", torch.int32), (row_mask, "row_mask", torch.int64))
    x_atoms, x_frags, sa, sf, out = _readout_args("pool_cat_coalitions", x_atoms, x_frags, plan, vectors, check)
    R = out.shape[0]
    if R == 0:
        return out
    if check:
        if R > 1 and bool((row_mol[1:] < row_mol[:-1]).any()):
            raise ValueError("pool_cat_coalitions: row_mol must be non-decreasing (a molecule's rows are one run)")
        if sa.n_items and int(atom_bit.max()) >= 64:
            raise IndexError(f"pool_cat_coalitions: atom_bit must be < 64 (got {int(atom_bit.max())})")
    a, f = _seg_struct(sa), _seg_struct(sf)
    _lib.call("fn_pool_cat_coalitions_f32", x_atoms.data_ptr(), x_frags.data_ptr(), C.byref(a), C.byref(f), atom_bit.data_ptr(),
              row_mol.data_ptr(), row_mask.data_ptr(), R, out.data_ptr(), _stream_ptr(out.device))
    return out


class _MaskedLoss(torch.autograd.Function):
    """A loss over a padded batch, loss and d loss / d out from one single-block kernel ``fn_<name>_f32``:
    ``masked_mse``: sum_i w_i |out_i - y_i|^2 / (sum_i w_i * T); ``masked_bce``: compute_bce_loss (train/utils.py:297-304)."""

    @staticmethod
    def forward(ctx, name, out, y, w):
        B = w.shape[0]
        out2, y2 = _f32c(out, "out").reshape(B, -1), _f32c(y, "y").reshape(B, -1)
        if out2.shape != y2.shape:
            raise ValueError(f"{name}: prediction {tuple(out.shape)} vs target {tuple(y.shape)}")
        w = _f32c(w, "w")
        loss = torch.empty((), dtype=torch.float32, device=out.device)
        g = torch.empty_like(out2)
        _lib.call(f"fn_{name}_f32", out2.data_ptr(), y2.data_ptr(), w.data_ptr(), B, out2.shape[1], loss.data_ptr(),
                  g.data_ptr(), _stream_ptr(out.device))
        ctx.save_for_backward(g)
        ctx.shape = out.shape
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (g,) = ctx.saved_tensors
        if _is_unit_grad(g_loss):      # d loss / d loss = 1: nothing to multiply
            return None, g.reshape(ctx.shape), None, None
        return None, (g * g_loss).reshape(ctx.shape), None, None


def masked_mse(out, y, w):
    return _MaskedLoss.apply("masked_mse", out, y, w)


def masked_bce(out, y, w):
    return _MaskedLoss.apply("masked_bce", out, y, w)


class _MaskedMSEMulti(torch.autograd.Function):
    """sum_k coef_k * masked_mse(out_k, y_k, w_k), coef_k = c_k * (scale[idx_k] if idx_k >= 0 else 1): loss and all
    gradients in two launches (fn_masked_mse_multi_f32)."""

    @staticmethod
    def forward(ctx, spec, scale, *tensors):
        n = len(spec)
        dev = tensors[0].device
        tasks = (_lib.MseTask * n)()
        keep, grads, shapes = [], [], []
        for k, (c, idx) in enumerate(spec):
            out, y, w = tensors[3 * k: 3 * k + 3]
            B = w.shape[0]
            out2, y2, w = _f32c(out, "out").reshape(B, -1), _f32c(y, "y").reshape(B, -1), _f32c(w, "w")
            if out2.shape != y2.shape:
                raise ValueError(f"masked_mse_multi: prediction {tuple(out.shape)} vs target {tuple(y.shape)}")
            g = torch.empty_like(out2)
            tasks[k] = _lib.MseTask(out2.data_ptr(), y2.data_ptr(), w.data_ptr(), g.data_ptr(), B, out2.shape[1], int(idx), float(c), 0.0)
            keep += [out2, y2, w]
            grads.append(g)
            shapes.append(out.shape)
        scale = None if scale is None else _f32c(scale, "scale")
        ws = torch.empty(_lib.load().fn_masked_mse_multi_ws(n), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.call("fn_masked_mse_multi_f32", tasks, n, _ptr(scale), ws.data_ptr(), loss.data_ptr(), _stream_ptr(dev))
        ctx.save_for_backward(*grads)
        ctx.shapes = shapes
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        one = _is_unit_grad(g_loss)
        out = [None, None]
        for g, shape in zip(ctx.saved_tensors, ctx.shapes):
            out += [(g if one else g * g_loss).reshape(shape), None, None]
        return tuple(out)


def masked_mse_multi(spec, scale, *triples):
    """``spec`` = [(c_k, scale_index_k or -1), ...]; ``triples`` = out_1, y_1, w_1, out_2, ...; ``scale`` a device vector."""
    return _MaskedMSEMulti.apply(tuple(spec), scale, *triples)


_UNIT_GRAD = {}


def unit_grad(device):
    """A persistent scalar 1.0 to seed ``loss.backward(gradient=...)`` with: autograd then launches no fill kernel, and
    ``masked_mse`` recognises it and skips the multiply (two launches of a captured step)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _UNIT_GRAD:
        _UNIT_GRAD[device] = torch.ones((), dtype=torch.float32, device=device)
    return _UNIT_GRAD[device]


def _is_unit_grad(t) -> bool:
    """``t`` is the persistent scalar of ``unit_grad``: the gradient is 1, a backward has nothing to multiply"""
    unit = _UNIT_GRAD.get(t.device)
    return unit is not None and t.data_ptr() == unit.data_ptr()


class _GatherRows(torch.autograd.Function):
    """index_select(table, 0, index) with a segment-sum backward (needs the CSR of ``index``)."""

    @staticmethod
    def forward(ctx, table, seg: Segments, keep_plan):
        table = _f32c(table, "table")
        width = table.shape[1]
        out = torch.empty((seg.n_items, width), dtype=torch.float32, device=table.device)
        if seg.n_items:
            _lib.call("fn_gather_rows_f32", table.data_ptr(), seg.index.data_ptr(), out.data_ptr(), seg.n_items, width,
                      _stream_ptr(table.device))
        ctx.seg, ctx.keep, ctx.rows = seg, keep_plan, table.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        seg = ctx.seg
        g = _f32c(g, "g")
        width = g.shape[1]
        out = torch.empty((ctx.rows, width), dtype=torch.float32, device=g.device)
        _lib.call("fn_segment_sum_f32", g.data_ptr(), width, seg.rowptr.data_ptr(), seg.perm.data_ptr(), seg.pos_base,
                  out.data_ptr(), seg.n_seg, width, seg.n_items, _stream_ptr(g.device))
        return out, None, None


# ======================================================================================
# torch-scatter operator surface
# ======================================================================================
def _dim0_only(dim, src):
    if dim not in (0, -src.dim()):
        raise NotImplementedError("fragnet_amd implements scatter along dim 0 (all the reference's call sites)")


def _n_seg(index: torch.Tensor, dim_size) -> int:
    if dim_size is not None:
        return int(dim_size)
    if index.numel() == 0:
        return 0
    return int(index.max()) + 1      # synchronises, exactly like torch-scatter does


def scatter_add(src, index, dim: int = 0, out=None, dim_size=None):
    """Drop-in for torch_scatter.scatter_add(src, index, dim=0): 1-D int64 ``index`` over the rows of ``src``."""
    _dim0_only(dim, src)
    if out is not None:
        raise NotImplementedError("out= is not used on the reference path")
    if index.dim() != 1 or index.numel() != src.shape[0]:
        raise RuntimeError("index must be 1-D with one entry per row of src")
    plan = GraphPlan.segments_only(index, _n_seg(index, dim_size))
    return segment_sum(src, plan.segs["s"], plan)


class _SegmentSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, seg: Segments, keep_plan):
        src = _f32c(src, "src")
        width = 1
        for extent in src.shape[1:]:
            width *= int(extent)
        probs = torch.empty_like(src)
        if src.numel():
            _lib.call("fn_segment_softmax_f32", src.data_ptr(), seg.rowptr.data_ptr(), seg.perm.data_ptr(), seg.pos_base,
                      probs.data_ptr(), seg.n_seg, width, _stream_ptr(src.device))
        ctx.seg, ctx.width, ctx.keep = seg, width, keep_plan
        ctx.save_for_backward(probs)
        return probs

    @staticmethod
    def backward(ctx, g):
        (probs,) = ctx.saved_tensors
        seg = ctx.seg
        g = _f32c(g, "g")
        out = torch.empty_like(probs)
        if probs.numel():
            _lib.call("fn_segment_softmax_bwd_f32", probs.data_ptr(), g.data_ptr(), seg.rowptr.data_ptr(),
                      seg.perm.data_ptr(), seg.pos_base, out.data_ptr(), seg.n_seg, ctx.width, _stream_ptr(g.device))
        return out, None, None


def scatter_softmax(src, index, dim: int = 0, dim_size=None):
    """Drop-in for torch_scatter.scatter_softmax(src, index, dim=0)."""
    _dim0_only(dim, src)
    if index.dim() != 1 or index.numel() != src.shape[0]:
        raise RuntimeError("index must be 1-D with one entry per row of src")
    plan = GraphPlan.segments_only(index, _n_seg(index, dim_size))
    return _SegmentSoftmax.apply(src, plan.segs["s"], plan)


# ======================================================================================
# act(dropout(x)) epilogue
# ======================================================================================
class PhiloxStream:
    """Counter-based dropout stream: (seed, running offset). One Philox block = 4 floats."""

    def __init__(self, seed: Optional[int] = None, rank: int = 0, salt: int = 0):
        self.seed = None if seed is None else (int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.rank = rank
        self.salt = int(salt)    # xor-ed into a DERIVED seed: a second stream of the same process (mask_stream) gets a key of its own
        self.offset = 0
        self.dev = None          # optional device-resident counter added to every offset when the kernels run

    def use_device_counter(self, device):
        """hipGraph mode: offsets handed out while a step is captured are baked into the graph, so the per-replay
        part of the counter lives in device memory and ``advance_device`` (captured too) moves it on."""
        if self.dev is None or self.dev.device != torch.device(device):
            self.dev = torch.zeros(1, dtype=torch.int64, device=device)
        return self.dev

    def advance_device(self, blocks: int):
        self.dev += int(blocks)

    def dev_ptr(self):
        return None if self.dev is None else self.dev.data_ptr()

    def take(self, numel: int):
        if self.seed is None:
            self.seed = ((torch.initial_seed() * 0x9E3779B97F4A7C15 + self.rank * 0xD1B54A32D192ED03) ^ self.salt) & 0xFFFFFFFFFFFFFFFF
        off = self.offset
        self.offset += (numel + 3) // 4
        return self.seed, off


class _DropoutAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p: float, relu: bool, seed: int, offset: int, dev):
        x = _f32c(x, "x")
        y = torch.empty_like(x)
        _lib.call("fn_dropout_act_f32", x.data_ptr(), y.data_ptr(), x.numel(), float(p), seed, offset, _ptr(dev), int(relu),
                  _stream_ptr(x.device))
        ctx.args = (float(p), bool(relu), seed, offset, dev)
        if relu:
            ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        p, relu, seed, offset, dev = ctx.args
        y = ctx.saved_tensors[0] if relu else None
        g = _f32c(g, "g")
        gx = torch.empty_like(g)
        _lib.call("fn_dropout_act_bwd_f32", g.data_ptr(), _ptr(y), gx.data_ptr(), g.numel(), p, seed, offset, _ptr(dev),
                  int(relu), _stream_ptr(g.device))
        return gx, None, None, None, None, None


def dropout_act(x, p: float, training: bool, relu: bool, rng: PhiloxStream):
    """relu(dropout(x)) (gat2.py:414-418) or plain dropout (gat2.py:396-397) as one elementwise kernel."""
    p_eff = float(p) if training else 0.0
    if p_eff == 0.0 and not relu:
        return x
    seed, off = rng.take(x.numel()) if p_eff > 0.0 else (0, 0)
    return _DropoutAct.apply(x, p_eff, relu, seed, off, rng.dev if p_eff > 0.0 else None)


MASK_STREAM_SALT = 0xA0761D6478BD642F      # the mask stream's seed derivation: never the dropout stream's (seed, counter) pair


def mask_stream(rank: int = 0) -> "PhiloxStream":
    """A PhiloxStream for row masks (sample_rows): seeded like the dropout stream from torch.initial_seed() and the rank, under a salt
    of its own, with its own host offset and device counter -- drawing a mask never moves the dropout stream."""
    return PhiloxStream(rank=rank, salt=MASK_STREAM_SALT)


def _row_count(n, n_dev, cap: int, dev):
    if n_dev is not None:
        if not torch.is_tensor(n_dev) or n_dev.dtype != torch.int32 or n_dev.numel() != 1 or n_dev.device != dev:
            raise ValueError("n_dev: a one-element int32 tensor on the output's device (the real row count of a padded batch)")
        return 0
    n = cap if n is None else int(n)
    if not 0 <= n <= cap:
        raise ValueError(f"n = {n}: the real row count must lie in [0, cap = {cap}]")
    return n


def select_rows(keys: torch.Tensor, keep_frac: float, n: Optional[int] = None, n_dev: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [cap]: 1 on the k = int(n * keep_frac) rows i < n with the smallest (key, index) pairs and on the padding rows n <= i < cap,
    0 elsewhere (fn_select_rows_u8).  ``keys``: contiguous uint32-valued int32 / uint32 CUDA tensor [cap]; ``n`` defaults to cap;
    ``n_dev`` (int32 [1] on the device) replaces it and is clamped to [0, cap] by the kernel."""
    if not keys.is_cuda:
        raise _lib.FragnetHipError(f"select_rows: the keys must live on the GPU (got {keys.device}); there is no CPU fallback")
    if keys.dtype not in (torch.int32, torch.uint32) or keys.dim() != 1 or not keys.is_contiguous():
        raise TypeError("select_rows: keys must be a contiguous one-dimensional int32 / uint32 tensor (the 32 key bits)")
    cap = keys.numel()
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=keys.device)
    elif out.dtype != torch.uint8 or out.numel() != cap or not out.is_contiguous() or out.device != keys.device:
        raise ValueError("select_rows: out must be a contiguous uint8 tensor of cap rows on the keys' device")
    _lib.call("fn_select_rows_u8", keys.data_ptr(), cap, _row_count(n, n_dev, cap, keys.device), _ptr(n_dev), float(keep_frac),
              out.data_ptr(), _stream_ptr(keys.device))
    return out


def sample_rows(cap: int, keep_frac: float, rng: "PhiloxStream", device, n: Optional[int] = None, n_dev: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same selection on keys the kernel draws itself (fn_sample_rows_u8): row i's key is word i % 4 of Philox block
    offset + i // 4 of ``rng`` (plus its device counter), which moves on by (cap + 3) // 4 blocks -- a function of cap alone, so a
    captured step and its eager fallback consume the stream alike."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.FragnetHipError(f"sample_rows: masks are drawn on the GPU (got {device}); there is no CPU fallback")
    cap = int(cap)
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or out.numel() != cap or not out.is_contiguous() or out.device != device:
        raise ValueError("sample_rows: out must be a contiguous uint8 tensor of cap rows on the device")
    nn_ = _row_count(n, n_dev, cap, device)
    seed, off = rng.take(cap)
    _lib.call("fn_sample_rows_u8", seed, off, _ptr(rng.dev), cap, nn_, _ptr(n_dev), float(keep_frac), out.data_ptr(), _stream_ptr(device))
    return out


# ======================================================================================
# prediction head: Linear -> act(dropout(.)) stack with a hand-written backward
# ======================================================================================
SMALL_LINEAR_MAX = _lib.FN_SMALL_LINEAR_MAX
DENSE_MAX_ROWS = _lib.FN_DENSE_MAX_ROWS
DENSE_HEAD = True            # hidden layers through fn_dense_fwd/bwd_f32 (False: library GEMMs + the element-wise kernels)
FUSED_HEAD_LOSS = os.environ.get("FRAGNET_FUSED_HEAD_LOSS", "1") != "0"       # False: last Linear, loss and the Linear's backward as three launches (A/B and tests)


def _dense_ok(rows: int, W) -> bool:
    return DENSE_HEAD and rows <= DENSE_MAX_ROWS and W.shape[0] % 4 == 0 and W.shape[1] % 4 == 0 and W.is_contiguous()


def _small_ok(W) -> bool:        # the last Linear's shapes fn_small_linear(_bwd)_f32 take
    return W.shape[0] <= SMALL_LINEAR_MAX and W.shape[1] % 4 == 0


def _scratch(n_floats: int, device):
    return torch.empty(n_floats, dtype=torch.float32, device=device) if n_floats else None


def head_route(rows: int, linears, kind: int = _lib.ACT_RELU, params=None) -> Optional[str]:
    """Which node ``mlp_head`` runs ``linears`` on for ``rows`` live rows and the activation ``kind``.  "dense": the hidden Linears on
    fn_dense_*_f32, the last one on fn_small_linear_*_f32 (``_DenseHead``); "tall": library GEMMs (``_TallHead``), ReLU only; None: no
    kernel path -- a Linear without bias, a hidden output width that is no multiple of 4, another kind than ReLU off the dense route
    (``params``: the Linears' weight, bias, weight, ... where the caller has collected them already)."""
    params = [q for lin in linears for q in (lin.weight, lin.bias)] if params is None else params
    dense = True
    for i in range(0, len(params) - 2, 2):
        if params[i + 1] is None or params[i].shape[0] % 4 != 0:
            return None
        dense = dense and _dense_ok(rows, params[i])
    if params[-1] is None:
        return None
    return "dense" if dense and _small_ok(params[-2]) else "tall" if kind == _lib.ACT_RELU else None


def head_fuses_loss(route, rows: int, x, linears, loss, training: bool) -> bool:
    """Whether ``mlp_head(loss=...)`` runs the last Linear, the loss and that Linear's backward in one launch: the dense route behind
    at least one hidden layer, a training step whose input takes a gradient, live rows, one target and one weight per padded row."""
    (_, tgt, row_w), last, M = loss, linears[-1], x.shape[0]
    return bool(FUSED_HEAD_LOSS and training and x.requires_grad and route == "dense" and len(linears) > 1 and rows > 0
                and last.in_features <= _lib.SMALL_LINEAR_LOSS_MAX_K and row_w.shape[0] == M and tgt.numel() == M * last.out_features)


def head_act_kind(act) -> Optional[int]:
    """The kernels' activation kind (``_lib.ACT_*``) of a head's activation module as ``_ACTS`` builds it (model.py), or None where
    torch keeps it: RReLU (its training slopes come from torch's generator) and non-default settings of the others."""
    nn, t = torch.nn, type(act)
    if isinstance(act, nn.ReLU):
        return _lib.ACT_RELU
    if (t is nn.GELU and act.approximate != "none") or (t is nn.CELU and act.alpha != 1.0) or (t is nn.LeakyReLU and act.negative_slope != 0.01) \
            or (t is nn.PReLU and not (act.weight.numel() == 1 and act.weight.dtype == torch.float32)):
        return None
    return {nn.SiLU: _lib.ACT_SILU, nn.GELU: _lib.ACT_GELU, nn.CELU: _lib.ACT_CELU, nn.SELU: _lib.ACT_SELU, nn.ReLU6: _lib.ACT_RELU6,
            nn.LeakyReLU: _lib.ACT_LEAKYRELU, nn.PReLU: _lib.ACT_PRELU}.get(t)


class _Relu(NamedTuple):
    """The activation behind one hidden layer, as the launches take it (the twin exports of csrc/head.hip differ in that one slot), is
    a ``_lib.HeadAct`` or, for relu(dropout(.)), this: the forward's epilogue and the gate scale of its backward (the saved output encodes
    the mask).  The kernels read a scale of 0 as "no gate", so p >= 1 (all dropped) gets a positive value, not 1 / (1 - p) = inf or 0."""
    epilogue: Optional[_lib.ActEpilogue]
    gate: float


_NO_GATE = _Relu(None, 0.0)        # what a gradient leaves through where no activation sits below: the head's input, a tall layer


def _gate_scale(p: float) -> float:
    return 1.0 / (1.0 - p) if 0.0 < p < 1.0 else 1.0


def _dense_fwd(act, h, W, b, y, st):
    """one hidden layer: y = act(h W^T + b), one launch"""
    entry, spec = ("fn_dense_fwd_act_f32", act) if isinstance(act, _lib.HeadAct) else ("fn_dense_fwd_f32", act.epilogue)
    _lib.call(entry, h.data_ptr(), W.data_ptr(), b.data_ptr(), y.data_ptr(), h.shape[0], W.shape[1], W.shape[0], C.byref(spec), st)


def _dense_bwd(below, gz, h_in, W, gx, dW, db, M_out, tail, st):
    """one hidden layer's backward: dW, db, the input gradient ``gx`` (``M_out`` rows) through the backward of ``below``; ``tail`` rides"""
    entry, spec = ("fn_dense_bwd_act_f32", C.byref(below)) if isinstance(below, _lib.HeadAct) else ("fn_dense_bwd_tail_f32", below.gate)
    _lib.call(entry, gz.data_ptr(), h_in.data_ptr(), W.data_ptr(), _ptr(gx), spec, dW.data_ptr(), db.data_ptr(), h_in.shape[0],
              W.shape[1], W.shape[0], M_out, None if tail is None else C.byref(tail), st)


def _plain_fwd(x, W, b, relu: bool, st):
    """a plain dense layer on fn_dense_fwd_f32 (the towers, ``frag_mlp``): relu?(x W^T + b) in new rows, the ReLU as the epilogue at p = 0"""
    y = torch.empty((x.shape[0], W.shape[0]), dtype=torch.float32, device=x.device)
    act = _lib.ActEpilogue(y.data_ptr(), 0.0, 1, 0, 0, None) if relu else None
    _lib.call("fn_dense_fwd_f32", x.data_ptr(), W.data_ptr(), b.data_ptr(), y.data_ptr(), x.shape[0], W.shape[1], W.shape[0],
              None if act is None else C.byref(act), st)
    return y


def _plain_bwd(g, x, W, gx, relu_below: bool, dW, db, st):
    """its backward on fn_dense_bwd_f32: dW, db (None: not kept) and the input gradient ``gx`` (None: not wanted), handed down through
    the ReLU that produced ``x`` (``relu_below``: the gate scale of p = 0) or as it is"""
    gate = _gate_scale(0.0) if relu_below else _NO_GATE.gate
    _lib.call("fn_dense_bwd_f32", g.data_ptr(), x.data_ptr(), W.data_ptr(), _ptr(gx), gate, dW.data_ptr(), _ptr(db), x.shape[0], W.shape[1],
              W.shape[0], x.shape[0], st)


def _relu_chain(h, P, st):
    """relu(Linear(.)) for the Linears P[2:] = weight, bias, .. on top of the first layer's output ``h``: every layer's output, ``h`` first"""
    acts = [h]
    for i in range(1, len(P) // 2):
        acts.append(_plain_fwd(acts[-1], P[2 * i], P[2 * i + 1], True, st))
    return acts


def _small_fwd(h, W, b, out, st):
    """the last Linear (``_small_ok``); ``out`` may have more rows than ``h``: the kernel zeroes them"""
    _lib.call("fn_small_linear_f32", h.data_ptr(), _f32c(W, "W").data_ptr(), b.data_ptr(), out.data_ptr(), h.shape[0], W.shape[1], W.shape[0],
              out.shape[0], st)


def _small_bwd(below, g, h, W, gz, dW, db, st):
    """the last Linear's backward: dW, db and its input gradient ``gz`` through the backward of the activation ``below``"""
    C_out, K = W.shape
    ws = _scratch(_lib.load().fn_small_linear_bwd_ws(h.shape[0], K, C_out), g.device)
    entry, spec = ("fn_small_linear_bwd_act_f32", C.byref(below)) if isinstance(below, _lib.HeadAct) else ("fn_small_linear_bwd_f32", below.gate)
    _lib.call(entry, g.data_ptr(), h.data_ptr(), W.data_ptr(), gz.data_ptr(), dW.data_ptr(), db.data_ptr(), h.shape[0], K, C_out, spec, _ptr(ws), st)


def _small_loss(below, h, W, b, loss, out, g, gz, parts, st):
    """last Linear + loss + d loss / d out (``g``) + the Linear's input gradient through ``below`` (``gz``); dW / db ride in a ``SmallDw``"""
    kind, tgt, row_w = loss
    entry, spec = ("fn_small_linear_loss_act_f32", C.byref(below)) if isinstance(below, _lib.HeadAct) else ("fn_small_linear_loss_f32", below.gate)
    _lib.call(entry, h.data_ptr(), _f32c(W, "W").data_ptr(), b.data_ptr(), tgt.data_ptr(), row_w.data_ptr(), int(kind), out.data_ptr(),
              g.data_ptr(), gz.data_ptr(), spec, parts.data_ptr(), h.shape[0], W.shape[1], W.shape[0], out.shape[0], st)


def _input_grad(like, M: int, last: bool, zeroed_by_kernel: bool = False):
    """buffer of d loss / d (input of a layer); the head's own input gradient (``last``) has all M rows, the padding rows 0"""
    full = torch.empty((M if last else like.shape[0], like.shape[1]), dtype=torch.float32, device=like.device)
    if not zeroed_by_kernel and full.shape[0] > like.shape[0]:
        full[like.shape[0]:].zero_()
    return full


def _head_saved(ctx):
    """a head node's saved tensors by name -- (slope partials, the fused loss's g, gz, loss partials, loss value; None where there are
    none), the layers' inputs (live rows), the weights -- and the parameters' gradient buffers, each claimed once per pass"""
    part, g, gz, parts, loss_t, *rest = ctx.saved_tensors
    n = len(ctx.params) // 2
    return (part, g, gz, parts, loss_t), rest[:n], rest[n:2 * n], [grad_buffer(q, slot) for q, slot in zip(ctx.params, ctx.slots)]


class _DenseHead(torch.autograd.Function):
    """FTHead1-5's predictor stack (gat2.py:631-637, 745-751) on route "dense": every Linear is ONE launch each way (csrc/head.hip),
    padding rows written as 0 by the kernels.  ``hact = (kind, order)``: another kind than ReLU (csrc/head_act.inc), with ``prelu`` the
    slope the layers share.  ``loss`` (``head_fuses_loss``): returns (out, loss), ``out`` without gradient.  DESIGN.md section 1.
    Precondition (``mlp_head`` sees to it): ``head_route`` says "dense" for these rows, parameters and kind."""

    @staticmethod
    def forward(ctx, x, live, p: float, draws, dev, hact, prelu, loss, *params):
        n, st, x = len(params) // 2, _stream_ptr(x.device), _f32c(x, "x")
        M, h = x.shape[0], x[:live]
        xs, pres, acts = [h], [], []
        for i in range(n - 1):
            W, b = params[2 * i], params[2 * i + 1]
            y = torch.empty((live, W.shape[0]), dtype=torch.float32, device=h.device)
            if hact is None:
                acts.append(_Relu(_lib.ActEpilogue(y.data_ptr(), p, 1, *draws[i], _ptr(dev)), _gate_scale(p)))
            else:
                pres.append(torch.empty_like(y))
                acts.append(_lib.HeadAct(*hact, p, 0, *draws[i], _ptr(dev), _ptr(prelu), pres[-1].data_ptr(), None))
            _dense_fwd(acts[-1], h, W, b, y, st)
            h = y
            xs.append(h)
        (W, b), (C_out, K), part, part_at = params[-2:], params[-2].shape, None, ()
        if prelu is not None and n > 1 and live > 0:
            # one slice of partials per hidden layer: layer i < n - 2 in the input-gradient launch of layer i + 1, the top one in
            # the last Linear's launch (its fused-loss forward, or its backward)
            lib = _lib.load()
            counts = [lib.fn_head_act_parts(_lib.ACT_AT_DENSE_BWD, live, params[2 * i].shape[0]) for i in range(n - 2)]
            counts.append(lib.fn_head_act_parts(_lib.ACT_AT_SMALL_LOSS, M, K) if loss is not None else lib.fn_head_act_parts(_lib.ACT_AT_SMALL_BWD, live, K))
            part = torch.empty(sum(counts), dtype=torch.float32, device=h.device)
            part_at = tuple(sum(counts[:i]) for i in range(n - 1))
            for act, at in zip(acts, part_at):
                act.part = part.data_ptr() + 4 * at
        ctx.params, ctx.slots = params, [grad_slot(q) for q in params]
        # the rest of what backward needs: ``dev`` is what ``acts`` point to, kept alive but not saved (the stream moves it in place)
        ctx.state = (M, acts, dev, prelu, None if prelu is None else grad_slot(prelu), part_at, loss is not None)
        out = torch.empty((M, C_out), dtype=torch.float32, device=h.device)        # the kernels zero the padding rows
        if loss is None:
            _small_fwd(h, W, b, out, st)
            ctx.save_for_backward(part, None, None, None, None, *xs, *params[0::2], *pres)
            return out
        loss = (loss[0], _f32c(loss[1], "y"), _f32c(loss[2], "w"))
        g = torch.empty((live, C_out), dtype=torch.float32, device=h.device)
        gz = torch.empty_like(h)
        parts = torch.empty(_lib.load().fn_small_linear_loss_ws(M), dtype=torch.float32, device=h.device)
        loss_t = torch.empty((), dtype=torch.float32, device=h.device)
        _small_loss(acts[-1], h, W, b, loss, out, g, gz, parts, st)
        ctx.save_for_backward(part, g, gz, parts, loss_t, *xs, *params[0::2], *pres)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)            # no zero-filled gradient for the predictions (a fill launch per step)
        return out, loss_t

    @staticmethod
    def backward(ctx, g_out, g_loss=None):
        (part, g, gz, parts, loss_t), xs, Ws, grads = _head_saved(ctx)
        M, acts, _, prelu, prelu_slot, part_at, fused_loss = ctx.state
        n, live, st, need_x = len(Ws), xs[0].shape[0], _stream_ptr(xs[0].device), ctx.needs_input_grad[0]
        W, h, dW, db, tail = Ws[-1], xs[-1], grads[-2], grads[-1], None
        if fused_loss:
            # the forward's launch left g = d loss / d out and gz for d loss / d loss = 1; dW / db / the loss value ride below
            if g_loss is not None and not _is_unit_grad(g_loss):
                g, gz = g * g_loss, gz * g_loss
                if part is not None:            # the top layer's slope partials, taken in the forward for d loss / d loss = 1
                    part[part_at[n - 2]:].mul_(g_loss)
            tail = _lib.SmallDw(g.data_ptr(), h.data_ptr(), dW.data_ptr(), db.data_ptr(), parts.data_ptr(), loss_t.data_ptr(),
                                parts.numel(), live, W.shape[1], W.shape[0])
        else:
            g = _f32c(g_out, "g")[:live]
            gz = _input_grad(h, M, n == 1) if (n > 1 or need_x) else torch.empty_like(h)
            _small_bwd(acts[-1] if n > 1 else _NO_GATE, g, h, W, gz, dW, db, st)
        for i in range(n - 2, -1, -1):          # gz is d loss / d (pre-activation) already: one launch for the layer
            gx = _input_grad(xs[i], M, i == 0, zeroed_by_kernel=True) if (i > 0 or need_x) else None
            _dense_bwd(acts[i - 1] if i > 0 else _NO_GATE, gz, xs[i], Ws[i], gx, grads[2 * i], grads[2 * i + 1], M if i == 0 else live, tail, st)
            tail, gz = None, gx
        g_prelu = None if prelu is None else grad_buffer(prelu, prelu_slot)
        if part is not None and part.numel():       # (there are partials only where there is a slope)
            _lib.call("fn_head_act_param_grad_f32", part.data_ptr(), part.numel(), g_prelu.data_ptr(), st)
        elif prelu is not None:
            g_prelu.zero_()
        return (gz if need_x else None, None, None, None, None, None, g_prelu, None, *grads)


class _TallHead(torch.autograd.Function):
    """The same stack on route "tall" (the pretrain towers run on every atom / bond), ReLU only: library GEMMs (addmm / mm) with the
    element-wise work fused around them (``fn_dropout_act_f32`` in place, ``fn_gate_colsum_f32``); padding rows written here.
    Precondition: ``head_route`` says "tall"."""

    @staticmethod
    def forward(ctx, x, live, p: float, draws, dev, *params):
        n, st, x = len(params) // 2, _stream_ptr(x.device), _f32c(x, "x")
        M, h = x.shape[0], x[:live]
        xs = [h]
        for i in range(n - 1):
            h = torch.addmm(params[2 * i + 1], h, params[2 * i].t())
            _lib.call("fn_dropout_act_f32", h.data_ptr(), h.data_ptr(), h.numel(), p, *draws[i], _ptr(dev), 1, st)
            xs.append(h)
        W, b = params[-2], params[-1]
        if _small_ok(W):
            out = torch.empty((M, W.shape[0]), dtype=torch.float32, device=h.device)
            _small_fwd(h, W, b, out, st)
        else:
            out = torch.addmm(b, h, W.t())
            if live < M:
                out = torch.cat([out, out.new_zeros((M - live, W.shape[0]))])
        ctx.params, ctx.slots, ctx.state = params, [grad_slot(q) for q in params], (M, _gate_scale(p))
        ctx.save_for_backward(None, None, None, None, None, *xs, *params[0::2])
        return out

    @staticmethod
    def backward(ctx, g):
        _, xs, Ws, grads = _head_saved(ctx)
        M, gate = ctx.state
        n, live, st, need_x = len(Ws), xs[0].shape[0], _stream_ptr(xs[0].device), ctx.needs_input_grad[0]
        g = _f32c(g, "g")[:live]
        W, h, dW, db = Ws[-1], xs[-1], grads[-2], grads[-1]

        def padded(gx):         # the head's own input gradient: all M rows
            return torch.cat([gx, gx.new_zeros((M - live, gx.shape[1]))]) if live < M else gx
        if _small_ok(W):        # (behind a hidden layer: a single small Linear is route "dense")
            gz = torch.empty_like(h)
            _small_bwd(_NO_GATE, g, h, W, gz, dW, db, st)
        else:
            gz = g @ W
            torch.mm(g.t(), h, out=dW)
            torch.sum(g, 0, out=db)
            if n == 1:
                gz = padded(gz)
        for i in range(n - 2, -1, -1):
            z = xs[i + 1]
            gy = torch.empty_like(z)
            ws = _scratch(_lib.load().fn_gate_colsum_ws(z.shape[0], z.shape[1]), z.device)
            _lib.call("fn_gate_colsum_f32", gz.data_ptr(), z.data_ptr(), gy.data_ptr(), grads[2 * i + 1].data_ptr(), z.shape[0], z.shape[1],
                      gate, _ptr(ws), st)
            torch.mm(gy.t(), xs[i], out=grads[2 * i])
            if i > 0 or need_x:
                gz = padded(gy @ Ws[i]) if i == 0 else gy @ Ws[i]
        return (gz if need_x else None, None, None, None, None, *grads)


def mlp_head(x, linears, p: float, training: bool, rng: "PhiloxStream", live=None, loss=None, act=None,
             order: int = _lib.ACT_DROP_THEN_ACT, in_drop: bool = False):
    """Runs ``linears`` (nn.Linear modules; relu(dropout(.)) after all but the last) as one autograd node, ``_DenseHead`` or
    ``_TallHead`` as ``head_route`` says.  ``live``: input rows >= live are padding (static-shape batches).

    ``act``: the hidden layers' activation module when it is not ReLU (``head_act_kind``), applied as act(dropout(.)) or, with
    ``order = _lib.ACT_ACT_THEN_DROP``, dropout(act(.)) (FTHead1/4; for ReLU both orders are the same numbers); ``in_drop``: the input
    is dropped first (FTHead1/4, one more Philox draw ahead of the layers').

    ``loss = (kind, target, row_weights)`` (kind: ``_lib.LOSS_MSE`` / ``_lib.LOSS_BCE``): the caller is a training step that will call
    ``backward`` on the loss with gradient 1 right away.  Returns ``(out, loss)``; ``loss`` is None when the fused launch does not
    apply (the caller then computes it from ``out``), else a scalar whose VALUE is complete once backward has run (the sum of the
    partials rides in the backward's first launch) and ``out`` carries no gradient."""
    p_eff = float(p) if training else 0.0
    kind = _lib.ACT_RELU if act is None else head_act_kind(act)
    if kind is None:
        raise ValueError(f"mlp_head: no kernel for the activation {act!r}")
    rows = x.shape[0] if live is None else max(0, min(int(live), x.shape[0]))
    params = [q for lin in linears for q in (lin.weight, lin.bias)]
    route = head_route(rows, linears, kind, params)
    if route is None and head_route(rows, linears, params=params) is None:
        raise ValueError("mlp_head: Linear layers need a bias, hidden ones an output width that is a multiple of 4")
    if route is None:
        raise _lib.FragnetHipError("mlp_head: activation kinds other than ReLU run on the dense-head kernels only (rows <= "
                                   f"{DENSE_MAX_ROWS}, widths multiples of 4, <= {SMALL_LINEAR_MAX} outputs)")
    if in_drop:
        x = dropout_act(x, p, training, False, rng)
    draws = tuple(rng.take(x.shape[0] * lin.out_features) if p_eff > 0.0 else (0, 0) for lin in linears[:-1])
    args = (x, rows, p_eff, draws, rng.dev if p_eff > 0.0 else None)
    hact = None if kind == _lib.ACT_RELU else (kind, int(order))
    prelu = act.weight if kind == _lib.ACT_PRELU else None
    if route == "tall":
        out = _TallHead.apply(*args, *params)
    elif loss is not None and head_fuses_loss(route, rows, x, linears, loss, training):
        return _DenseHead.apply(*args, hact, prelu, loss, *params)
    else:
        out = _DenseHead.apply(*args, hact, prelu, None, *params)
    return (out, None) if loss is not None else out


# ======================================================================================
# PretrainTask's tall towers: Linear(128 -> 64) -> ReLU -> Linear(64 -> 32) -> ReLU -> Linear(32 -> 1) on every atom / bond
# ======================================================================================
TOWER_SHAPES = ((64, 128), (32, 64), (1, 32))


def tower_ok(x, linears) -> bool:
    """The fused tower kernels take exactly the reference's `PretrainTask(128, 1)` shape (pretrain_heads.py:33-58) on GPU rows."""
    return x.is_cuda and x.dim() == 2 and x.shape[1] == FN_D and len(linears) == 3 and \
        all(tuple(lin.weight.shape) == shp and lin.bias is not None for lin, shp in zip(linears, TOWER_SHAPES))


class _Towers(torch.autograd.Function):
    """Up to FN_MAX_TOWERS towers as ONE launch each way (csrc/tower.hip): forward keeps h1 / h2, backward writes the input
    gradients and reduces the weight-gradient partials straight into the parameters' gradient buffers (FlatAdam slots)."""

    @staticmethod
    def forward(ctx, n, *args):
        xs, params = [_f32c(x, "x") for x in args[:n]], args[n:]
        dev = xs[0].device
        tw = (_lib.Tower * n)()
        keep, outs = [], []
        for i, x in enumerate(xs):
            M = x.shape[0]
            w1, b1, w2, b2, w3, b3 = (_f32c(q, "tower parameter") for q in params[6 * i: 6 * i + 6])
            h1 = torch.empty((M, 64), dtype=torch.float32, device=dev)
            h2 = torch.empty((M, 32), dtype=torch.float32, device=dev)
            out = torch.empty((M, 1), dtype=torch.float32, device=dev)
            t = tw[i]
            t.x, t.w1, t.b1, t.w2, t.b2, t.w3, t.b3 = (q.data_ptr() for q in (x, w1, b1, w2, b2, w3, b3))
            t.h1, t.h2, t.out, t.M = h1.data_ptr(), h2.data_ptr(), out.data_ptr(), M
            keep += [x, h1, h2, w1, b1, w2, b2, w3, b3]
            outs.append(out)
        _lib.call("fn_tower_fwd_f32", tw, n, _stream_ptr(dev))
        ctx.n = n
        ctx.params, ctx.slots = params, [grad_slot(q) for q in params]
        ctx.save_for_backward(*keep)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        n, saved = ctx.n, ctx.saved_tensors
        dev = saved[0].device
        tw = (_lib.Tower * n)()
        gxs, grads, keep = [], [], []
        for i in range(n):
            x, h1, h2, w1, b1, w2, b2, w3, b3 = saved[9 * i: 9 * i + 9]
            M = x.shape[0]
            g = gs[i]
            g = torch.zeros((M, 1), dtype=torch.float32, device=dev) if g is None else _f32c(g, "g")
            gx = torch.empty_like(x) if ctx.needs_input_grad[1 + i] else None
            pg = [grad_buffer(ctx.params[6 * i + k], ctx.slots[6 * i + k]) for k in range(6)]
            t = tw[i]
            t.x, t.w1, t.b1, t.w2, t.b2, t.w3, t.b3 = (q.data_ptr() for q in (x, w1, b1, w2, b2, w3, b3))
            t.h1, t.h2, t.M, t.g_out, t.g_x = h1.data_ptr(), h2.data_ptr(), M, g.data_ptr(), _ptr(gx)
            t.g_w1, t.g_b1, t.g_w2, t.g_b2, t.g_w3, t.g_b3 = (q.data_ptr() for q in pg)
            gxs.append(gx)
            grads += pg
            keep.append(g)
        ws = torch.empty(_lib.load().fn_tower_bwd_ws(tw, n), dtype=torch.float32, device=dev)
        _lib.call("fn_tower_bwd_f32", tw, n, ws.data_ptr(), _stream_ptr(dev))
        return (None, *gxs, *grads)


def towers(pairs):
    """``pairs`` = [(x [M,128], [Linear(128,64), Linear(64,32), Linear(32,1)]), ...] -> list of [M,1] outputs; every pair must pass
    ``tower_ok``."""
    if not 1 <= len(pairs) <= _lib.FN_MAX_TOWERS:
        raise ValueError("towers: 1..FN_MAX_TOWERS towers per call")
    params = [q for _, lins in pairs for lin in lins for q in (lin.weight, lin.bias)]
    return list(_Towers.apply(len(pairs), *[x for x, _ in pairs], *params))


# ======================================================================================
# pretrain bond-length head input: cat(x[src], x[dst], e_attr)
# ======================================================================================
class _EdgeConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, e_attr, edge_index, plan: GraphPlan):
        x, e_attr = _f32c(x, "x"), _f32c(e_attr, "e_attr")
        E = edge_index.shape[1]
        edge_index = edge_index.contiguous()
        out = torch.empty((E, 3 * FN_D), dtype=torch.float32, device=x.device)
        _lib.call("fn_edge_concat_f32", x.data_ptr(), e_attr.data_ptr(), edge_index.data_ptr(), out.data_ptr(), E,
                  _stream_ptr(x.device))
        ctx.plan, ctx.n = plan, x.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        plan, n = ctx.plan, ctx.n
        g = _f32c(g, "g")
        st = _stream_ptr(g.device)
        gx = torch.empty((n, FN_D), dtype=torch.float32, device=g.device)
        tmp = torch.empty_like(gx)
        s, d = plan.segs["edge_src"], plan.segs["edge_dst"]
        ld = 3 * FN_D
        _lib.call("fn_segment_sum_f32", g.data_ptr(), ld, s.rowptr.data_ptr(), s.perm.data_ptr(), s.pos_base,
                  gx.data_ptr(), n, FN_D, s.n_items, st)
        _lib.call("fn_segment_sum_f32", g.data_ptr() + 4 * FN_D, ld, d.rowptr.data_ptr(), d.perm.data_ptr(), d.pos_base,
                  tmp.data_ptr(), n, FN_D, d.n_items, st)
        gx += tmp
        return gx, g[:, 2 * FN_D:].contiguous(), None, None


def edge_concat(x, e_attr, edge_index, plan: GraphPlan):
    return _EdgeConcat.apply(x, e_attr, edge_index, plan)


# ======================================================================================
# bond-graph topology from edge_index (dataset side)
# ======================================================================================
def bond_graph(edge_index: torch.Tensor, atom_batch: torch.Tensor, n_mols: int, fragments: bool = False) -> torch.Tensor:
    """``edge_index_bonds_graph`` [2, Eb] (int64, global bond ids) of a collated batch from its ``edge_index`` [2, E] and
    ``batch`` vector -- the reference's get_bond_pair_bond_graph + one-bond-fragment rule (dataset/data.py:116-127,
    157-182) on the GPU, in the reference's order, so a dataset can ship without its largest tensor (the per-pair
    cos(theta) attribute is stored, or computed from atom coordinates in the same rows: ``bond_cos``).  ``fragments=True``: ``edge_index_fbonds`` from
    ``frag_index`` and ``frag_batch`` (get_bond_pair_fbond_graph, data.py:131-154).  One host sync to learn Eb."""
    if not edge_index.is_cuda or edge_index.dtype != torch.int64 or atom_batch.dtype != torch.int64:
        raise _lib.FragnetHipError("bond_graph: int64 GPU tensors expected (there is no CPU fallback)")
    edge_index, atom_batch = edge_index.contiguous(), atom_batch.contiguous()
    E, N, dev = edge_index.shape[1], atom_batch.shape[0], edge_index.device
    st, mode = _stream_ptr(dev), int(bool(fragments))
    ws = torch.empty(_lib.load().fn_bond_graph_ws(E, n_mols), dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.call("fn_bond_graph_count", edge_index.data_ptr(), atom_batch.data_ptr(), E, N, n_mols, mode, ws.data_ptr(), total.data_ptr(), st)
    n = int(total.item())
    out = torch.empty((2, n), dtype=torch.int64, device=dev)
    _lib.call("fn_bond_graph_fill", edge_index.data_ptr(), atom_batch.data_ptr(), E, N, n_mols, mode, ws.data_ptr(), out.data_ptr(), n, st)
    return out


# ======================================================================================
# geometry of a collated batch from atom coordinates (dataset side; csrc/geometry.hip)
# ======================================================================================
def _geom_inputs(positions, edge_index, what):
    if not (positions.is_cuda and edge_index.is_cuda):
        raise _lib.FragnetHipError(f"{what}: fragnet_amd kernels need GPU tensors; there is no CPU fallback (synth.geometry_from_positions "
                                   "is the host evaluation)")
    if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] != 3:
        raise TypeError(f"{what}: positions must be float32 [N, 3], got {positions.dtype} {tuple(positions.shape)}")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise TypeError(f"{what}: edge_index must be int64 [2, E], got {edge_index.dtype} {tuple(edge_index.shape)}")
    return positions.contiguous(), edge_index.contiguous()


def bond_cos(positions: torch.Tensor, edge_index: torch.Tensor, edge_index_bonds_graph: torch.Tensor) -> torch.Tensor:
    """``edge_attr_bonds`` [Eb, 1] of a collated batch from its atom coordinates [N, 3]: for the bond-graph edge (bond i, bond j) the
    cosine of the angle at the atom the two bonds share -- the clamped dot product of the two unit vectors, what the reference gets from
    RDKit's GetAngleRad and np.cos (dataset/data.py:185-211) -- and exactly 1 for the two directions of one bond (one-bond fragments).
    Rows follow ``edge_index_bonds_graph``, stored or rebuilt by ``bond_graph``.  One launch, no synchronisation."""
    positions, edge_index = _geom_inputs(positions, edge_index, "bond_cos")
    if not edge_index_bonds_graph.is_cuda:
        raise _lib.FragnetHipError("bond_cos: fragnet_amd kernels need GPU tensors; there is no CPU fallback")
    if edge_index_bonds_graph.dtype != torch.int64 or edge_index_bonds_graph.dim() != 2 or edge_index_bonds_graph.shape[0] != 2:
        raise TypeError("bond_cos: edge_index_bonds_graph must be int64 [2, Eb]")
    eib = edge_index_bonds_graph.contiguous()
    out = torch.empty((eib.shape[1], 1), dtype=torch.float32, device=positions.device)
    _lib.call("fn_bond_cos_f32", positions.data_ptr(), edge_index.data_ptr(), eib.data_ptr(), positions.shape[0], edge_index.shape[1],
              eib.shape[1], out.data_ptr(), _stream_ptr(positions.device))
    return out


def pretrain_geometry(positions: torch.Tensor, edge_index: torch.Tensor, batch: torch.Tensor, n_mols: int, max_per_mol=None):
    """The three pretraining targets of a collated batch from its atom coordinates (reference get_bond_angle_dhangle, dataset/data.py:
    224-260, quirks included -- DESIGN.md "Geometry from coordinates"): ``(bnd_lngth [E, 1], bnd_angl [N, 1], dh_angl [E, 1])`` = the
    SQUARED bond length, 3 S_a^2 and S_src S_dst (3 - sigma_e^2).  ``batch`` [N] is the collated atom -> molecule vector (non-decreasing,
    bonds grouped by molecule).  ``max_per_mol``: (atoms, directed bonds) of the largest molecule when the caller knows them on the host
    (a store does); None reads them back from the device, one synchronisation.  Molecules beyond 1024 atoms / 4096 directed bonds are
    refused.  Sums run in edge order without atomics: bit-identical from run to run."""
    positions, edge_index = _geom_inputs(positions, edge_index, "pretrain_geometry")
    if not batch.is_cuda:
        raise _lib.FragnetHipError("pretrain_geometry: fragnet_amd kernels need GPU tensors; there is no CPU fallback")
    if batch.dtype != torch.int64 or batch.dim() != 1 or batch.shape[0] != positions.shape[0]:
        raise TypeError("pretrain_geometry: batch must be int64 [N]")
    batch = batch.contiguous()
    N, E, dev = positions.shape[0], edge_index.shape[1], positions.device
    if max_per_mol is None:
        max_atoms = int(torch.bincount(batch, minlength=1).max()) if N else 0
        max_bonds = int(torch.bincount(batch[edge_index[0]], minlength=1).max()) if E else 0
    else:
        max_atoms, max_bonds = (int(v) for v in max_per_mol)
    bl = torch.empty((E, 1), dtype=torch.float32, device=dev)
    ba = torch.empty((N, 1), dtype=torch.float32, device=dev)
    dh = torch.empty((E, 1), dtype=torch.float32, device=dev)
    _lib.call("fn_pretrain_geometry_f32", positions.data_ptr(), edge_index.data_ptr(), batch.data_ptr(), N, E, int(n_mols), max_atoms,
              max_bonds, bl.data_ptr(), ba.data_ptr(), dh.data_ptr(), _stream_ptr(dev))
    return bl, ba, dh


# ======================================================================================
# cancer drug response model (reference model/cdrp/model.py): the cell-line tower MLP(gene_dim), csrc/cdrp.hip, and the pair head, csrc/pair_head.hip
# ======================================================================================
def _i64c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.FragnetHipError(f"{name}: fragnet_amd kernels need GPU tensors (got {t.device}); there is no CPU fallback")
    if t.dtype != torch.int64:
        raise TypeError(f"{name}: expected int64 (collate_fn_cdrp's gene_expr), got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _gene_shapes(gene, W, b):
    if gene.dim() != 2 or W.dim() != 2 or W.shape[1] != gene.shape[1] or b.shape != (W.shape[0],):
        raise ValueError(f"gene_linear: gene_expr {tuple(gene.shape)} does not match weight {tuple(W.shape)} / bias {tuple(b.shape)}")


class _GeneLinear(torch.autograd.Function):
    """relu(gene_expr.float() @ W.T + b) on the int64 rows of ``collate_fn_cdrp`` (MLP.forward's first layer): one launch each way, any
    ``gene_dim`` (no multiple-of-4 rule: fn_cdrp_gene_fwd_f32 / fn_cdrp_gene_bwd_f32).  No gradient for ``gene_expr``: it is data."""

    @staticmethod
    def forward(ctx, gene, W, b):
        gene, W, b = _i64c(gene, "gene_expr"), _f32c(W, "weight"), _f32c(b, "bias")
        _gene_shapes(gene, W, b)
        M, K = gene.shape
        y = torch.empty((M, W.shape[0]), dtype=torch.float32, device=gene.device)
        _lib.call("fn_cdrp_gene_fwd_f32", gene.data_ptr(), W.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, W.shape[0], _stream_ptr(gene.device))
        ctx.params, ctx.slots = (W, b), (grad_slot(W), grad_slot(b))
        ctx.save_for_backward(gene, y)
        return y

    @staticmethod
    def backward(ctx, g):
        gene, y = ctx.saved_tensors
        g = _f32c(g, "g")
        (W, b), slots = ctx.params, ctx.slots
        dW, db = grad_buffer(W, slots[0]), grad_buffer(b, slots[1])
        _lib.call("fn_cdrp_gene_bwd_f32", g.data_ptr(), y.data_ptr(), gene.data_ptr(), dW.data_ptr(), db.data_ptr(), gene.shape[0], gene.shape[1],
                  W.shape[0], _stream_ptr(g.device))
        return None, dW, db


def gene_linear(gene_expr, weight, bias):
    return _GeneLinear.apply(gene_expr, weight, bias)


class _CellTower(torch.autograd.Function):
    """MLP(gene_dim) (model/cdrp/model.py:7-22: Linear gene_dim -> 1024 -> 256 -> 64 -> 256, a ReLU after EVERY Linear, no dropout) as one
    autograd node: the first layer on the int64 rows (fn_cdrp_gene_fwd_f32), the others fn_dense_fwd_f32 with the ReLU epilogue (p = 0);
    backward top-down with fn_dense_bwd_f32 (gate_scale = 1: each launch hands the layer below its gradient already through that
    layer's ReLU) and fn_cdrp_gene_bwd_f32.  The incoming gradient goes through the last ReLU first -- unless the pair head's backward
    produced it, which has done that already (``_fn_relu_gated``)."""

    @staticmethod
    def forward(ctx, gene, *params):
        gene = _i64c(gene, "gene_expr")
        params = tuple(_f32c(q, "tower parameter") for q in params)
        _gene_shapes(gene, params[0], params[1])
        M, K = gene.shape
        st = _stream_ptr(gene.device)
        h = torch.empty((M, params[0].shape[0]), dtype=torch.float32, device=gene.device)
        _lib.call("fn_cdrp_gene_fwd_f32", gene.data_ptr(), params[0].data_ptr(), params[1].data_ptr(), h.data_ptr(), M, K, h.shape[1], st)
        acts = _relu_chain(h, params, st)
        ctx.params, ctx.slots = params, [grad_slot(q) for q in params]
        ctx.save_for_backward(gene, *acts)
        return acts[-1]

    @staticmethod
    def backward(ctx, g):
        gene, *acts = ctx.saved_tensors
        P, slots = ctx.params, ctx.slots
        n = len(P) // 2
        M = gene.shape[0]
        st = _stream_ptr(gene.device)
        tag = getattr(g, "_fn_relu_gated", None)
        gated = tag is not None and tag.data_ptr() == acts[-1].data_ptr() and tag.shape == acts[-1].shape
        g = _f32c(g, "g")
        if not gated:
            gy, top = torch.empty_like(g), acts[-1]
            colsum = torch.empty(top.shape[1], dtype=torch.float32, device=g.device)
            ws = _scratch(_lib.load().fn_gate_colsum_ws(M, top.shape[1]), g.device)
            _lib.call("fn_gate_colsum_f32", g.data_ptr(), top.data_ptr(), gy.data_ptr(), colsum.data_ptr(), M, top.shape[1], 1.0, _ptr(ws), st)
            g = gy
        grads = [None] * (2 * n)
        for i in range(n - 1, 0, -1):
            W, x = P[2 * i], acts[i - 1]
            dW, db = grad_buffer(P[2 * i], slots[2 * i]), grad_buffer(P[2 * i + 1], slots[2 * i + 1])
            gx = torch.empty_like(x)
            _plain_bwd(g, x, W, gx, True, dW, db, st)
            grads[2 * i], grads[2 * i + 1] = dW, db
            g = gx
        dW, db = grad_buffer(P[0], slots[0]), grad_buffer(P[1], slots[1])
        _lib.call("fn_cdrp_gene_bwd_f32", g.data_ptr(), None, gene.data_ptr(), dW.data_ptr(), db.data_ptr(), M, gene.shape[1], P[0].shape[0], st)
        grads[0], grads[1] = dW, db
        return (None, *grads)


def cell_tower(gene_expr, linears):
    """The cell-line tower on ``gene_expr`` [B, gene_dim] int64: relu(Linear(.)) for every Linear of ``linears`` (MLP.predictor), as
    ``_CellTower``.  More than ``DENSE_MAX_ROWS`` rows, or a Linear behind the first whose widths are not multiples of 4 (or a first one
    whose output width is not), fall back to plain torch ops on ``gene_expr.float()`` -- library GEMMs, the way ``mlp_head`` treats tall inputs."""
    if not gene_expr.is_cuda:
        raise _lib.FragnetHipError(f"cell_tower: fragnet_amd kernels need GPU tensors (got {gene_expr.device}); there is no CPU fallback")
    linears = list(linears)
    if not cell_tower_ok(gene_expr, gene_expr.shape[0], linears):
        v = gene_expr.float()
        for lin in linears:
            v = torch.relu(torch.nn.functional.linear(v, lin.weight, lin.bias))
        return v
    return _CellTower.apply(gene_expr, *[q for lin in linears for q in (lin.weight, lin.bias)])


def cell_tower_ok(gene_expr, rows: int, linears) -> bool:
    """Whether ``rows`` rows of ``gene_expr`` run ``linears`` on the tower's kernels (``cell_tower``'s fast path)."""
    return gene_expr.dtype == torch.int64 and gene_expr.dim() == 2 and rows <= DENSE_MAX_ROWS and linears[0].out_features % 4 == 0 \
        and all(lin.bias is not None for lin in linears) and all(_dense_ok(rows, lin.weight) for lin in linears[1:])


def _cell_path_forward(gene, P, alpha, base, st):
    """The tower on the path rows ``x0 + alpha[j] (gene[c] - x0)`` (row c S + j): every layer's output, as ``_CellTower.forward`` saves
    them, the first from fn_cdrp_gene_fwd_path_f32 -- the path rows themselves are never in memory."""
    (C_, K), S = gene.shape, alpha.shape[0]
    M = C_ * S
    h = torch.empty((M, P[0].shape[0]), dtype=torch.float32, device=gene.device)
    _lib.call("fn_cdrp_gene_fwd_path_f32", gene.data_ptr(), _ptr(base), alpha.data_ptr(), P[0].data_ptr(), P[1].data_ptr(), h.data_ptr(), C_, S, K,
              h.shape[1], st)
    return _relu_chain(h, P, st)


def _cell_path_args(gene_expr, linears, v, alpha, base, what):
    gene = _i64c(gene_expr, "gene_expr")
    linears = list(linears)
    alpha = _f32c(alpha, "alpha").reshape(-1)
    rows = gene.shape[0] * alpha.shape[0] if gene.dim() == 2 else 0
    if alpha.shape[0] < 1 or not cell_tower_ok(gene, rows, linears):
        raise ValueError(f"{what}: the cell-line tower's kernels take int64 [C, gene_dim] rows, C * steps <= {DENSE_MAX_ROWS}, Linears with a "
                         "bias and output widths that are multiples of 4; there is no other path")
    P = tuple(_f32c(q.detach(), "tower parameter") for lin in linears for q in (lin.weight, lin.bias))
    _gene_shapes(gene, P[0], P[1])
    v = _f32c(v, "v").reshape(1, -1)
    if v.shape[1] != P[-2].shape[0]:
        raise ValueError(f"{what}: v has {v.shape[1]} entries, the tower's output {P[-2].shape[0]}")
    if base is not None:
        base = _f32c(base, "baseline").reshape(-1)
        if base.shape[0] != gene.shape[1]:
            raise ValueError(f"{what}: the baseline has {base.shape[0]} entries, gene_expr {gene.shape[1]} columns")
    return gene, P, v, alpha, base


def cell_path_scores(gene_expr, linears, v, alpha, base=None):
    """``<cell_enc, v>`` on the path rows ``x0 + alpha[j] (gene_expr[c] - x0)``, [C, S] (``base`` None: x0 = 0): the tower's kernels and
    fn_small_linear_f32 for the dot, no autograd.  ``alpha = [1]`` scores the cell lines themselves, with the model's own bits."""
    gene, P, v, alpha, base = _cell_path_args(gene_expr, linears, v, alpha, base, "cell_path_scores")
    st = _stream_ptr(gene.device)
    top = _cell_path_forward(gene, P, alpha, base, st)[-1]
    out = torch.empty((top.shape[0], 1), dtype=torch.float32, device=gene.device)
    if top.shape[0]:
        _lib.call("fn_small_linear_f32", top.data_ptr(), v.data_ptr(), None, out.data_ptr(), top.shape[0], v.shape[1], 1, top.shape[0], st)
    return out.view(gene.shape[0], alpha.shape[0])


def cell_path_attributions(gene_expr, linears, v, alpha, base=None, want_gradient: bool = False):
    """Attributions of ``s = <cell_enc, v>`` to the genes over the path nodes ``alpha`` [S] (row c S + j is node j of cell line c):
    ``attr[c, k] = (gene_expr[c, k] - x0[k]) * mean_j d s / d x[c S + j, k]`` as float32 [C, gene_dim] -- gradient x input for ``alpha =
    [1]``, integrated gradients for a quadrature's nodes.  The call sequence of ``_CellTower`` without autograd: the path forward
    (fn_cdrp_gene_fwd_path_f32, then fn_dense_fwd_f32), the seed ``v`` through the last ReLU (fn_small_linear_bwd_f32 with ones for the
    upstream gradient), fn_dense_bwd_f32 top-down for the input gradients (gate_scale = 1; the weight gradients it also writes go to
    scratch) and fn_cdrp_gene_dx_f32, which multiplies by the first weight and folds the S nodes.  Returns ``(attr, gradient)``,
    ``gradient`` [C, gene_dim] the path-averaged input gradient with ``want_gradient``, else None."""
    gene, P, v, alpha, base = _cell_path_args(gene_expr, linears, v, alpha, base, "cell_path_attributions")
    dev, st = gene.device, _stream_ptr(gene.device)
    (C_, K), S = gene.shape, alpha.shape[0]
    M = C_ * S
    attr = torch.empty((C_, K), dtype=torch.float32, device=dev)
    grad = torch.empty_like(attr) if want_gradient else None
    if M == 0:
        return attr, grad
    acts = _cell_path_forward(gene, P, alpha, base, st)
    top = acts[-1]
    ones = torch.ones((M, 1), dtype=torch.float32, device=dev)
    g, dv, dvb = torch.empty_like(top), torch.empty_like(v), torch.empty(1, dtype=torch.float32, device=dev)
    ws = _scratch(_lib.load().fn_small_linear_bwd_ws(M, v.shape[1], 1), dev)
    _lib.call("fn_small_linear_bwd_f32", ones.data_ptr(), top.data_ptr(), v.data_ptr(), g.data_ptr(), dv.data_ptr(), dvb.data_ptr(), M, v.shape[1], 1,
              1.0, _ptr(ws), st)
    for i in range(len(P) // 2 - 1, 0, -1):
        W, x = P[2 * i], acts[i - 1]
        gx = torch.empty_like(x)
        _plain_bwd(g, x, W, gx, True, torch.empty_like(W), None, st)
        g = gx
    _lib.call("fn_cdrp_gene_dx_f32", g.data_ptr(), None, P[0].data_ptr(), gene.data_ptr(), _ptr(base), attr.data_ptr(), _ptr(grad), C_, S, K,
              P[0].shape[0], st)
    return attr, grad


class _PairInstance(NamedTuple):
    """One built instance of the pair-head kernels (csrc/pair_head.hip): 256 + ``width`` -> 128 -> 1."""
    prefix: str          # entry points <prefix>_loss_ws, <prefix>_fwd_f32 (<prefix>_fwd_rows_f32 with a real-row count), <prefix>_bwd_f32
    width: int           # of the second input
    gated: bool          # the second input is the output of a ReLU: its gradient comes back zero where it is <= 0
    name: str            # the public function, in error messages
    second: str          # the second input, in error messages

    @property
    def shapes(self):    # fc1, fc2: the widths the entry points are built for
        return (FN_D, 2 * FN_D + self.width), (1, FN_D)


_PAIR_CDRP = _PairInstance("fn_cdrp_pair", 256, True, "pair_head", "cell_enc")
_PAIR_DTA = _PairInstance("fn_dta_pair", 300, False, "pair_head_dta", "xt")


# What ``_PairHead`` and ``_PairHeadFactored`` share, the fused-loss contract among it.  With a target the forward's launch also leaves
# g = d MSE / d out and the loss partials, and the node returns (out, loss): ``out`` then carries no gradient and the VALUE of ``loss`` is
# complete once backward has run (its sum rides in the backward launch), as with ``_DenseHead``'s fused loss.  A node's own part is the
# buffers its launches fill and read (``keep``: drug, second input, then what its forward saved) and their argument lists.
def _pair_loss_buffers(target, rows: int, C_out: int, n_parts, dev, name: str, unit: str):
    """forward: ``(target, g, parts, loss_t)`` of the fused loss over ``rows`` outputs (``n_parts``: how many partials, called with a
    target only); four None without a target"""
    if target is None:
        return None, None, None, None
    target = _f32c(target, "y").reshape(-1)
    if target.numel() != rows * C_out:
        raise ValueError(f"{name}: {target.numel()} targets for {rows} {unit}")
    return (target, torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(n_parts(), dtype=torch.float32, device=dev),
            torch.empty((), dtype=torch.float32, device=dev))


def _pair_forward_end(ctx, inst, params, keep, out, g, parts, loss_t):
    """forward, behind the launch: what backward needs, and the node's result"""
    ctx.inst, ctx.params, ctx.slots = inst, params, [grad_slot(q) for q in params]
    ctx.n_keep, ctx.fused = len(keep), g is not None
    if not ctx.fused:
        ctx.save_for_backward(*keep)
        return out
    ctx.save_for_backward(*keep, g, parts, loss_t)
    ctx.mark_non_differentiable(out)
    ctx.set_materialize_grads(False)
    return out, loss_t


def _pair_backward_begin(ctx, g_out, g_loss):
    """backward, in front of the launch: ``(keep, g, parts, loss_t, (dW1, db1, dW2, db2), g_drug, g_second)`` -- g is the forward's
    (times a non-unit d / d loss) where the loss was fused, else the incoming gradient; the parameters' buffers are claimed here"""
    keep, parts, loss_t = ctx.saved_tensors[:ctx.n_keep], None, None
    if ctx.fused:
        g, parts, loss_t = ctx.saved_tensors[ctx.n_keep:]
        if g_loss is not None and not _is_unit_grad(g_loss):
            g = g * g_loss
    else:
        g = _f32c(g_out, "g").reshape(-1)
    grads = tuple(grad_buffer(q, s) for q, s in zip(ctx.params, ctx.slots))
    return keep, g, parts, loss_t, grads, torch.empty_like(keep[0]), torch.empty_like(keep[1])


def _pair_backward_end(ctx, x1, g_drug, g_x1, grads, n_between: int):
    """backward, behind the launch: the gate tag and the gradients in the order of forward's arguments (instance, drug, second input,
    ``n_between`` without gradient, target, parameters)"""
    if ctx.inst.gated:
        g_x1._fn_relu_gated = x1
    return (None, g_drug if ctx.needs_input_grad[1] else None, g_x1 if ctx.needs_input_grad[2] else None, *(None,) * (n_between + 1), *grads)


class _PairHead(torch.autograd.Function):
    """fc2(fc1(cat(drug_enc, second))) (model/cdrp/model.py:35-42, model/dta/model.py:141-144; nothing between the two Linears) for
    256 + ``inst.width`` -> 128 -> 1: one launch each way (<prefix>_fwd_f32 / <prefix>_bwd_f32), the two inputs read where they are.
    With ``target`` the loss is fused (above); ``target = (y, real_rows)`` hands the forward the device-side count of the real rows of a
    static-shape step (``_pair_apply``: the mean is over them, the rows behind them get g = 0).  Where ``inst.gated`` (CDRP's ``cell_enc``) the gradient handed to the second input is already through the
    backward of the ReLU that produced it (tagged ``_fn_relu_gated`` for ``_CellTower``; applying that gate again, as a plain autograd
    ReLU would, changes nothing); otherwise (DTA's ``xt``, a Linear's output) it is NOT gated."""

    @staticmethod
    def forward(ctx, inst, drug, x1, target, W1, b1, w2, b2):
        drug, x1 = _f32c(drug, "drug_enc"), _f32c(x1, inst.second)
        W1, b1, w2, b2 = (_f32c(q, "pair-head parameter") for q in (W1, b1, w2, b2))
        M, dev = drug.shape[0], drug.device
        Kd, K1, H, C_out = drug.shape[1], x1.shape[1], W1.shape[0], w2.shape[0]
        if x1.shape[0] != M or W1.shape[1] != Kd + K1 or w2.shape[1] != H or b1.shape != (H,) or b2.shape != (C_out,):
            raise ValueError(f"{inst.name}: drug_enc / {inst.second} / fc1 / fc2 shapes do not fit together")
        h = torch.empty((M, H), dtype=torch.float32, device=dev)
        out = torch.empty((M, C_out), dtype=torch.float32, device=dev)
        target, real_rows = target if isinstance(target, tuple) else (target, None)
        target, g, parts, loss_t = _pair_loss_buffers(target, M, C_out, lambda: getattr(_lib.load(), inst.prefix + "_loss_ws")(M), dev,
                                                      inst.name, "rows")
        args = (drug.data_ptr(), x1.data_ptr(), W1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), _ptr(target), h.data_ptr(),
                out.data_ptr(), _ptr(g), _ptr(parts), M, Kd, K1, H, C_out)
        if real_rows is None:
            _lib.call(inst.prefix + "_fwd_f32", *args, _stream_ptr(dev))
        else:
            _lib.call(inst.prefix + "_fwd_rows_f32", *args, real_rows.data_ptr(), _stream_ptr(dev))
        return _pair_forward_end(ctx, inst, (W1, b1, w2, b2), (drug, x1, h), out, g, parts, loss_t)

    @staticmethod
    def backward(ctx, g_out, g_loss=None):
        (drug, x1, h), g, parts, loss_t, grads, g_drug, g_x1 = _pair_backward_begin(ctx, g_out, g_loss)
        P = ctx.params
        _lib.call(ctx.inst.prefix + "_bwd_f32", g.data_ptr(), drug.data_ptr(), x1.data_ptr(), h.data_ptr(), P[0].data_ptr(), P[2].data_ptr(),
                  g_drug.data_ptr(), g_x1.data_ptr(), *(q.data_ptr() for q in grads), _ptr(parts), 0 if parts is None else parts.numel(),
                  _ptr(loss_t), drug.shape[0], drug.shape[1], x1.shape[1], P[0].shape[0], P[2].shape[0], _stream_ptr(drug.device))
        return _pair_backward_end(ctx, x1, g_drug, g_x1, grads, 0)


def pair_fuses_loss(loss, rows: int, tensors) -> bool:
    """Whether a pair head with ``loss = (kind, y, row_w)`` or ``(kind, y, row_w, real_rows)`` runs the loss in its forward launch and the
    loss's sum in its backward launch: MSE without row weights, live rows, and a training step -- gradients enabled and one of ``tensors``
    (the two inputs and the four parameters) taking one.  A real-row COUNT (``_pair_apply``) is no row weight and does not stand in the way."""
    kind, _, row_w = loss[:3]
    return bool(FUSED_HEAD_LOSS and kind == _lib.LOSS_MSE and row_w is None and torch.is_grad_enabled() and rows > 0
                and any(t.requires_grad for t in tensors))


def _pair_apply(node, args, rows: int, fc1, fc2, loss):
    """``node`` on ``args`` = (instance, drug, second input, ..), the target and the parameters: the result in ``pair_head``'s three shapes.
    A fourth element of ``loss`` is the device-side count of the REAL rows (int32 [1], ``plan.REAL_MOLS_KEY`` of a batch staged to static
    shapes; for ``_PairHeadFactored`` the count of its real PAIRS): the loss is the mean over the first ``n`` rows and the rows behind them
    receive no gradient.  It exists in the fused launches only -- a caller that computes the loss from ``out`` itself would take the
    padding rows for real ones -- so where the fused launch does not apply the count is an error."""
    params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    if loss is None:
        return node.apply(*args, None, *params)
    real_rows = loss[3] if len(loss) > 3 else None
    fused = pair_fuses_loss(loss, rows, (args[1], args[2], *params))
    if real_rows is not None:
        if not fused:
            raise _lib.FragnetHipError(f"{args[0].name}: a real-row count needs the fused MSE launch of the pair head (a training step, no "
                                       "row weights)")
        if not (real_rows.is_cuda and real_rows.dtype == torch.int32 and real_rows.numel() == 1):
            raise TypeError(f"{args[0].name}: the real-row count is one int32 word on the GPU, got {tuple(real_rows.shape)} {real_rows.dtype} on {real_rows.device}")
        return node.apply(*args, (loss[1], real_rows), *params)
    if not fused:
        return node.apply(*args, None, *params), None
    return node.apply(*args, loss[1], *params)


def _pair_widths_ok(inst, drug_enc, x1, fc1, fc2) -> bool:
    return (tuple(fc1.weight.shape), tuple(fc2.weight.shape)) == inst.shapes and fc1.bias is not None and fc2.bias is not None \
        and drug_enc.dim() == 2 and x1.dim() == 2 and drug_enc.shape[1] == FN_D * 2 and x1.shape[1] == inst.width


def _pair_head(inst, drug_enc, x1, fc1, fc2, loss):
    """``pair_head`` / ``pair_head_dta``: the instance is the caller's choice, never guessed from ``fc1``'s width -- whether the second
    gradient is gated says where the second input came from."""
    if not (drug_enc.is_cuda and x1.is_cuda):
        raise _lib.FragnetHipError(f"{inst.name}: fragnet_amd kernels need GPU tensors; there is no CPU fallback")
    if not (_pair_widths_ok(inst, drug_enc, x1, fc1, fc2) and drug_enc.shape[0] <= DENSE_MAX_ROWS):
        if loss is not None and len(loss) > 3 and loss[3] is not None:
            raise _lib.FragnetHipError(f"{inst.name}: a real-row count needs the built widths (256 + {inst.width} -> 128 -> 1)")
        out = fc2(fc1(torch.cat((drug_enc, x1), 1)))
        return (out, None) if loss is not None else out
    return _pair_apply(_PairHead, (inst, drug_enc, x1), drug_enc.shape[0], fc1, fc2, loss)


def pair_head(drug_enc, cell_enc, fc1, fc2, loss=None):
    """``fc2(fc1(cat(drug_enc, cell_enc)))`` as ``_PairHead``; ``cell_enc`` must be the output of a ReLU (the tower's: its gradient comes
    back gated by ``cell_enc > 0``).  ``loss = (_lib.LOSS_MSE, y, None)``, in the style of ``mlp_head``: the caller is a training step that
    calls ``backward`` on the loss right away (``(_lib.LOSS_MSE, y, None, real_rows)``: the mean over the first ``*real_rows`` rows, see
    ``_pair_apply``); returns ``(out, loss)`` with ``loss`` None where the fused launch does not apply (the caller
    then computes it from ``out``).  Other widths than 256 + 256 -> 128 -> 1, Linears without bias or more than ``DENSE_MAX_ROWS`` rows
    fall back to plain torch ops (``torch.cat`` + two library GEMMs)."""
    return _pair_head(_PAIR_CDRP, drug_enc, cell_enc, fc1, fc2, loss)


# ======================================================================================
# drug-target affinity model (reference model/dta/model.py, DTAModel2): the protein tower, csrc/dta.hip, and the pair head 256 + 300, csrc/pair_head.hip
# ======================================================================================
DTA_CONV_FILTERS, DTA_CONV_KS, DTA_CONV_MAX_V, DTA_CONV_MAX_L, DTA_CONV_MAX_D = 32, 8, 32, 4096, 512      # fn_dta_conv_*_f32's instance / limits


class _ProteinTower(torch.autograd.Function):
    """fc1_xt(conv_xt_1(embedding_xt(tokens)).view(B, -1)) (model/dta/model.py:134-138; no activation anywhere) as one autograd node.
    The convolution runs in its histogram form (fn_dta_conv_fwd_f32: the [B, L, D] embedded tensor is never built, the per-sample
    histogram A is saved for the backward), Linear(F J, 300) on fn_dense_fwd_f32 reading the convolution's output in place; backward:
    fn_dense_bwd_f32 (no gate: nothing sits between the two layers), then fn_dta_conv_bwd_f32 for the convolution's weight and bias
    and the embedding table.  No gradient for ``tokens``: they are data."""

    @staticmethod
    def forward(ctx, tokens, E, Wc, bc, Wf, bf):
        tokens = _i64c(tokens, "protein tokens")
        E, Wc, bc, Wf, bf = (_f32c(q, "protein-tower parameter") for q in (E, Wc, bc, Wf, bf))
        M, L = tokens.shape
        V, D = E.shape
        F_, KS = Wc.shape[0], Wc.shape[2]
        K = F_ * (D - KS + 1)
        dev, st = tokens.device, _stream_ptr(tokens.device)
        A = torch.empty((M, V, F_ * KS), dtype=torch.float32, device=dev)
        conv = torch.empty((M, K), dtype=torch.float32, device=dev)
        _lib.call("fn_dta_conv_fwd_f32", tokens.data_ptr(), E.data_ptr(), Wc.data_ptr(), bc.data_ptr(), A.data_ptr(), conv.data_ptr(), M, L, D, V,
                  F_, KS, st)
        ctx.params, ctx.slots = (E, Wc, bc, Wf, bf), [grad_slot(q) for q in (E, Wc, bc, Wf, bf)]
        ctx.save_for_backward(tokens, A, conv)
        return _plain_fwd(conv, Wf, bf, False, st)

    @staticmethod
    def backward(ctx, g):
        tokens, A, conv = ctx.saved_tensors
        g = _f32c(g, "g")
        (E, Wc, bc, Wf, bf), slots = ctx.params, ctx.slots
        dE, dWc, dbc, dWf, dbf = (grad_buffer(q, s) for q, s in zip(ctx.params, slots))
        M, L = tokens.shape
        V, D = E.shape
        st = _stream_ptr(g.device)
        g_conv = torch.empty_like(conv)
        _plain_bwd(g, conv, Wf, g_conv, False, dWf, dbf, st)
        ws = _scratch(_lib.load().fn_dta_conv_bwd_ws(M, L, D, V), g.device)
        _lib.call("fn_dta_conv_bwd_f32", g_conv.data_ptr(), tokens.data_ptr(), E.data_ptr(), A.data_ptr(), dWc.data_ptr(), dbc.data_ptr(),
                  dE.data_ptr(), _ptr(ws), M, L, D, V, Wc.shape[0], Wc.shape[2], st)
        return None, dE, dWc, dbc, dWf, dbf


def _protein_tower_ok(tokens, embedding, conv, fc) -> bool:
    W = conv.weight
    if tokens.dim() != 2 or W.dim() != 3 or conv.bias is None or fc.bias is None:
        return False
    plain_conv = tuple(conv.stride) == (1,) and tuple(conv.dilation) == (1,) and conv.groups == 1 and conv.padding in ((0,), "valid") \
        and conv.padding_mode == "zeros"
    plain_emb = embedding.padding_idx is None and embedding.max_norm is None and not embedding.scale_grad_by_freq and not embedding.sparse
    V, D = embedding.weight.shape
    return plain_conv and plain_emb and tuple(W.shape) == (DTA_CONV_FILTERS, tokens.shape[1], DTA_CONV_KS) and V <= DTA_CONV_MAX_V \
        and DTA_CONV_KS <= D <= DTA_CONV_MAX_D and 1 <= tokens.shape[1] <= DTA_CONV_MAX_L \
        and fc.in_features == DTA_CONV_FILTERS * (D - DTA_CONV_KS + 1) and _dense_ok(tokens.shape[0], fc.weight)


def protein_tower(tokens, embedding, conv, fc):
    """The protein tower of ``DTAModel2`` on ``tokens`` [B, L] int64: ``fc(conv(embedding(tokens)).view(B, -1))`` with ``embedding`` an
    nn.Embedding(V, D), ``conv`` an nn.Conv1d(L, 32, 8) (it only holds the parameters) and ``fc`` an nn.Linear(32 (D - 7), .), as
    ``_ProteinTower``.  More than ``DENSE_MAX_ROWS`` rows or other shapes than fn_dta_conv_*_f32 is built for (32 filters of 8, V <= 32,
    8 <= D <= 512, L <= 4096, plain stride / padding / dilation) fall back to plain torch ops (embedding, library convolution and GEMM)."""
    if not tokens.is_cuda:
        raise _lib.FragnetHipError(f"protein_tower: fragnet_amd kernels need GPU tensors (got {tokens.device}); there is no CPU fallback")
    if tokens.dtype != torch.int64:
        raise TypeError(f"protein_tower: expected int64 tokens (collate_fn_dta's protein), got {tokens.dtype}")
    if not _protein_tower_ok(tokens, embedding, conv, fc):
        return fc(conv(embedding(tokens)).flatten(1))
    return _ProteinTower.apply(tokens, embedding.weight, conv.weight, conv.bias, fc.weight, fc.bias)


def pair_head_dta(drug_enc, xt, fc1, fc2, loss=None):
    """``fc2(fc1(cat(drug_enc, xt)))`` as ``_PairHead``, not gated (``xt`` is a Linear's output); ``loss = (_lib.LOSS_MSE, y, None)`` as for ``pair_head``: returns
    ``(out, loss)`` with ``loss`` None where the fused launch does not apply.  Other widths than 256 + 300 -> 128 -> 1, Linears without
    bias or more than ``DENSE_MAX_ROWS`` rows fall back to plain torch ops (``torch.cat`` + two library GEMMs)."""
    return _pair_head(_PAIR_DTA, drug_enc, xt, fc1, fc2, loss)


# ======================================================================================
# the two pair heads on a factored batch: U distinct drugs, C distinct second inputs, pair lists; csrc/pair_factored.hip
# ======================================================================================
def pair_orderings(pair_list: torch.Tensor, n_rows: int):
    """``(rowptr int32 [n_rows + 1], perm int32 [M])`` of ``pair_list`` [M]: ``perm[rowptr[r] : rowptr[r + 1]]`` are the pairs of row r
    in ascending order (a stable sort of the list).  Values outside ``[0, n_rows)`` belong to no row.  Plain torch ops on the list's
    device, no synchronisation; ``data.collate_fn_*_factored`` builds the same on the host and carries them in the batch."""
    pl = pair_list.reshape(-1).to(torch.int64)
    inside = (pl >= 0) & (pl < n_rows)
    key = torch.where(inside, pl, torch.full_like(pl, n_rows))
    perm = torch.sort(key, stable=True)[1].to(torch.int32)
    counts = torch.bincount(key, minlength=n_rows + 1)[:n_rows]
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int32, device=pl.device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr, perm


def pair_orderings_both(pair_drug: torch.Tensor, pair_second: torch.Tensor, n_drug: int, n_second: int, real_pairs=None, out=None):
    """``pair_orderings`` of both pair lists as ONE launch of fn_pair_orderings_i32 (csrc/pair_factored.hip): ``(rowptr_drug [n_drug + 1],
    perm_drug [M], rowptr_second [n_second + 1], perm_second [M])``, int32, the ``orderings`` of ``pair_head_factored``.  No host read, no
    sort or scan of the library: it can sit inside a captured step.  ``real_pairs`` (int32 [1] on the GPU, or None): only the first
    ``n = clamp(*real_pairs, 0, M)`` pairs exist -- what lies behind them is not read, is in no row, and ``perm`` holds -1 from
    ``rowptr[-1]`` on (``pair_orderings`` has no -1: there every pair is listed, the out-of-range ones last).  ``out``: four int32 tensors
    to write into.  More than ``DENSE_MAX_ROWS`` pairs or rows on a side is an error."""
    if not (pair_drug.is_cuda and pair_second.is_cuda):
        raise _lib.FragnetHipError("pair_orderings_both: fragnet_amd kernels need GPU tensors; there is no CPU fallback")
    if pair_drug.dtype != torch.int64 or pair_second.dtype != torch.int64 or pair_drug.dim() != 1 or pair_drug.shape != pair_second.shape:
        raise TypeError("pair_orderings_both: the pair lists are two int64 vectors of one length")
    if real_pairs is not None and not (real_pairs.is_cuda and real_pairs.dtype == torch.int32 and real_pairs.numel() == 1):
        raise TypeError(f"pair_orderings_both: the real-pair count is one int32 word on the GPU, got {tuple(real_pairs.shape)} {real_pairs.dtype} on {real_pairs.device}")
    pd, ps, M, dev = pair_drug.contiguous(), pair_second.contiguous(), pair_drug.numel(), pair_drug.device
    sizes = (n_drug + 1, M, n_second + 1, M)
    if out is None:
        out = tuple(torch.empty(n, dtype=torch.int32, device=dev) for n in sizes)
    elif any(not t.is_contiguous() for t in out):
        raise ValueError("pair_orderings_both: the output tensors must be contiguous")
    out = tuple(_i32c(t, "pair_orderings_both: output", n) for t, n in zip(out, sizes))
    _lib.call("fn_pair_orderings_i32", pd.data_ptr(), ps.data_ptr(), _ptr(real_pairs), *(t.data_ptr() for t in out), M, n_drug, n_second,
              _stream_ptr(dev))
    return out


def _i32c(t: torch.Tensor, name: str, numel: int) -> torch.Tensor:
    if not t.is_cuda or t.dtype != torch.int32 or t.numel() != numel:
        raise ValueError(f"{name}: expected {numel} int32 entries on the GPU (ops.pair_orderings), got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t if t.is_contiguous() else t.contiguous()


class _PairHeadFactored(torch.autograd.Function):
    """``_PairHead`` on U distinct drug rows, C distinct second rows and the pair lists: <prefix>_factored_fwd_f32 saves A = D W1d^T
    [U,128] and B = S W1s^T [C,128] in place of ``h`` [M,128] and writes out [M,1]; <prefix>_factored_bwd_f32 folds the per-pair gradient
    over the pair orderings, so both input gradients come back per DISTINCT row.  The fused-loss contract, the ``_fn_relu_gated`` tag and
    the gate are ``_PairHead``'s; ``target = (y, real_pairs)`` takes <prefix>_factored_fwd_rows_f32 (a static-shape step: the mean over the
    first ``*real_pairs`` pairs; the orderings must then be those of the same count, ``pair_orderings_both``)."""

    @staticmethod
    def forward(ctx, inst, drug, x1, pd, ps, orderings, target, W1, b1, w2, b2):
        drug, x1 = _f32c(drug, "drug_enc"), _f32c(x1, inst.second)
        W1, b1, w2, b2 = (_f32c(q, "pair-head parameter") for q in (W1, b1, w2, b2))
        (U, Kd), (C_, K1), M, dev = drug.shape, x1.shape, pd.numel(), drug.device
        H, C_out = W1.shape[0], w2.shape[0]
        A = torch.empty((U, H), dtype=torch.float32, device=dev)
        B = torch.empty((C_, H), dtype=torch.float32, device=dev)
        ws = torch.empty(getattr(_lib.load(), inst.prefix + "_factored_ws")(U, C_), dtype=torch.float32, device=dev)
        out = torch.empty((M, C_out), dtype=torch.float32, device=dev)
        target, real_pairs = target if isinstance(target, tuple) else (target, None)
        target, g, parts, loss_t = _pair_loss_buffers(target, M, C_out, lambda: 1, dev, inst.name + "_factored", "pairs")
        args = (drug.data_ptr(), x1.data_ptr(), pd.data_ptr(), ps.data_ptr(), W1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                _ptr(target), A.data_ptr(), B.data_ptr(), ws.data_ptr(), out.data_ptr(), _ptr(g), _ptr(parts), M, U, C_, Kd, K1, H, C_out)
        if real_pairs is None:
            _lib.call(inst.prefix + "_factored_fwd_f32", *args, _stream_ptr(dev))
        else:
            _lib.call(inst.prefix + "_factored_fwd_rows_f32", *args, real_pairs.data_ptr(), _stream_ptr(dev))
        ctx.M = M
        return _pair_forward_end(ctx, inst, (W1, b1, w2, b2), (drug, x1, A, B, *orderings), out, g, parts, loss_t)

    @staticmethod
    def backward(ctx, g_out, g_loss=None):
        (drug, x1, *saved), g, parts, loss_t, grads, g_drug, g_x1 = _pair_backward_begin(ctx, g_out, g_loss)      # saved: A, B, the orderings
        P, (A, B) = ctx.params, saved[:2]
        _lib.call(ctx.inst.prefix + "_factored_bwd_f32", g.data_ptr(), drug.data_ptr(), x1.data_ptr(), A.data_ptr(), B.data_ptr(), P[0].data_ptr(),
                  P[1].data_ptr(), P[2].data_ptr(), *(q.data_ptr() for q in saved[2:]), g_drug.data_ptr(), g_x1.data_ptr(),
                  *(q.data_ptr() for q in grads), _ptr(parts), 0 if parts is None else parts.numel(), _ptr(loss_t), ctx.M, drug.shape[0],
                  x1.shape[0], drug.shape[1], x1.shape[1], P[0].shape[0], P[2].shape[0], _stream_ptr(drug.device))
        return _pair_backward_end(ctx, x1, g_drug, g_x1, grads, 3)


def _pair_head_factored(inst, drug_enc, x1, pair_drug, pair_second, fc1, fc2, loss, orderings, check):
    name = inst.name + "_factored"
    if not (drug_enc.is_cuda and x1.is_cuda and pair_drug.is_cuda and pair_second.is_cuda):
        raise _lib.FragnetHipError(f"{name}: fragnet_amd kernels need GPU tensors; there is no CPU fallback")
    if pair_drug.dtype != torch.int64 or pair_second.dtype != torch.int64 or pair_drug.dim() != 1 or pair_drug.shape != pair_second.shape:
        raise TypeError(f"{name}: the pair lists are two int64 vectors of one length")
    pd, ps = pair_drug.contiguous(), pair_second.contiguous()
    U, C_, M = drug_enc.shape[0], x1.shape[0], pd.numel()
    if check and M:          # one synchronisation; check=False: the caller built the lists on the host and has checked them there
        lo_hi = torch.stack((pd.min(), pd.max(), ps.min(), ps.max())).tolist()
        if lo_hi[0] < 0 or lo_hi[1] >= U or lo_hi[2] < 0 or lo_hi[3] >= C_:
            raise IndexError(f"{name}: pair lists reach outside the {U} drug rows / {C_} {inst.second} rows")
    ok = _pair_widths_ok(inst, drug_enc, x1, fc1, fc2) and max(U, C_, M) <= DENSE_MAX_ROWS and (M == 0 or (U > 0 and C_ > 0))
    if not ok:
        if loss is not None and len(loss) > 3 and loss[3] is not None:
            raise _lib.FragnetHipError(f"{name}: a real-row count needs the built widths (256 + {inst.width} -> 128 -> 1) and at most "
                                       f"{DENSE_MAX_ROWS} rows and pairs")
        out = fc2(fc1(torch.cat((drug_enc[pd], x1[ps]), 1)))
        return (out, None) if loss is not None else out
    if orderings is None:
        orderings = pair_orderings(pd, U) + pair_orderings(ps, C_)
    orderings = tuple(_i32c(t, f"{name}: pair ordering", n) for t, n in zip(orderings, (U + 1, M, C_ + 1, M)))
    return _pair_apply(_PairHeadFactored, (inst, drug_enc, x1, pd, ps, orderings), M, fc1, fc2, loss)


def pair_head_factored(drug_enc, cell_enc, pair_drug, pair_second, fc1, fc2, loss=None, orderings=None, check: bool = True):
    """``pair_head`` on a factored batch: ``out[m] = fc2(fc1(cat(drug_enc[pair_drug[m]], cell_enc[pair_second[m]])))`` [M, 1] from the U
    distinct rows of ``drug_enc``, the C distinct rows of ``cell_enc`` (the output of a ReLU: its gradient comes back gated) and the two
    int64 pair lists -- no duplicated row is ever built.  ``loss`` as for ``pair_head`` (the mean is over the M pairs).  ``orderings``:
    ``pair_orderings`` of both lists (drug's, then the second's), built here when None.  ``check=True`` validates the pair lists' range
    on the host (one synchronisation; the kernels skip an outside pair instead of indexing with it); ``check=False``: the caller built
    them on the host and has checked them there.  Other widths, or more than ``DENSE_MAX_ROWS`` rows or pairs, fall back to plain torch
    ops on the gathered rows."""
    return _pair_head_factored(_PAIR_CDRP, drug_enc, cell_enc, pair_drug, pair_second, fc1, fc2, loss, orderings, check)


def pair_head_dta_factored(drug_enc, xt, pair_drug, pair_second, fc1, fc2, loss=None, orderings=None, check: bool = True):
    """``pair_head_dta`` on a factored batch (``pair_head_factored``; ``xt``'s gradient is not gated)."""
    return _pair_head_factored(_PAIR_DTA, drug_enc, xt, pair_drug, pair_second, fc1, fc2, loss, orderings, check)


def _pair_head_grid(inst, drug_enc, x1, fc1, fc2):
    name = inst.name + "_grid"
    if not (drug_enc.is_cuda and x1.is_cuda):
        raise _lib.FragnetHipError(f"{name}: fragnet_amd kernels need GPU tensors; there is no CPU fallback")
    U, C_ = drug_enc.shape[0], x1.shape[0]
    if not (_pair_widths_ok(inst, drug_enc, x1, fc1, fc2) and max(U, C_) <= DENSE_MAX_ROWS):
        pd = torch.arange(U, device=drug_enc.device).repeat_interleave(C_)
        ps = torch.arange(C_, device=drug_enc.device).repeat(U)
        return fc2(fc1(torch.cat((drug_enc[pd], x1[ps]), 1))).view(U, C_)
    drug, x = _f32c(drug_enc.detach(), "drug_enc"), _f32c(x1.detach(), inst.second)
    W1, b1, w2, b2 = (_f32c(q.detach(), "pair-head parameter") for q in (fc1.weight, fc1.bias, fc2.weight, fc2.bias))
    out = torch.empty((U, C_), dtype=torch.float32, device=drug.device)
    _lib.call(inst.prefix + "_factored_grid_f32", drug.data_ptr(), x.data_ptr(), W1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
              out.data_ptr(), U, C_, drug.shape[1], x.shape[1], W1.shape[0], w2.shape[0], _stream_ptr(drug.device))
    return out


def pair_head_grid(drug_enc, cell_enc, fc1, fc2):
    """Every drug against every cell line: ``out[u, c] = fc2(fc1(cat(drug_enc[u], cell_enc[c])))`` [U, C] in one launch
    (fn_cdrp_pair_factored_grid_f32).  An evaluation read-out: no autograd node.  Other widths or more than ``DENSE_MAX_ROWS`` rows on
    a side: plain torch ops."""
    return _pair_head_grid(_PAIR_CDRP, drug_enc, cell_enc, fc1, fc2)


def pair_head_dta_grid(drug_enc, xt, fc1, fc2):
    """``pair_head_grid`` for the drug-target-affinity head (fn_dta_pair_factored_grid_f32)."""
    return _pair_head_grid(_PAIR_DTA, drug_enc, xt, fc1, fc2)


# ======================================================================================
# graph-convolution baseline (reference model/gcn/gcn2.py, model_version gcn2): the degree-normalised neighbour sum, csrc/gcn.hip, and the
# fragment MLP on the dense kernels
# ======================================================================================
def gcn_coef(level: Level) -> torch.Tensor:
    """deg^-1/2 per node of ``level`` (gcn2.py:51-53: out-degree of the graph with self loops, 0 where it is 0), from the row extents of
    the level's by-source CSR.  The same table for every layer and both directions: callers compute it once per batch."""
    dev = level.keep[0].device
    coef = torch.empty(level.n, dtype=torch.float32, device=dev)
    _lib.call("fn_gcn_coef_f32", C.byref(level.c), coef.data_ptr(), _stream_ptr(dev))
    return coef


class _GcnAggregate(torch.autograd.Function):
    """y[i] = c[i] sum_{k in seg(i)} c[nbr(k)] x[nbr(k)] over ``level``'s by-destination CSR (fn_gcn_aggregate_f32), optionally with
    relu?(dropout(.)) as the launch's epilogue.  Returns the raw rows, the activated rows, or both (raw, activated).  Backward: the
    gradient of the activated rows goes through fn_dropout_act_bwd_f32 first (the saved output gates the ReLU), the raw rows' gradient is
    added to it, and ONE launch of the same kernel on the by-source CSR gathers the sum (the weight c[s] c[t] is symmetric)."""

    @staticmethod
    def forward(ctx, x, coef, level: Level, want_raw: bool, epi):
        x = _f32c(x, "x")
        n = level.n
        if x.shape != (n, FN_D):
            raise ValueError(f"gcn_aggregate: x must be [{n}, {FN_D}], got {tuple(x.shape)}")
        if coef is not None:
            coef = _f32c(coef, "coef")
            if coef.shape != (n,) or coef.device != x.device:
                raise ValueError(f"gcn_aggregate: coef must be [{n}] on {x.device}, got {tuple(coef.shape)} on {coef.device}")
        if not want_raw and epi is None:
            raise ValueError("gcn_aggregate: neither the raw nor the activated rows were asked for")
        dev = x.device
        out = torch.empty((n, FN_D), dtype=torch.float32, device=dev) if want_raw else None
        y = act = None
        if epi is not None:
            p, relu, seed, offset, rdev = epi
            y = torch.empty((n, FN_D), dtype=torch.float32, device=dev)
            act = _lib.ActEpilogue(y.data_ptr(), float(p), int(relu), seed, offset, _ptr(rdev) if p > 0.0 else None)
        _lib.call("fn_gcn_aggregate_f32", x.data_ptr(), C.byref(level.c), 0, _ptr(coef), _ptr(out), None if act is None else C.byref(act),
                  _stream_ptr(dev))
        ctx.level, ctx.epi, ctx.coef, ctx.want_raw = level, epi, coef, want_raw
        if epi is not None and epi[1]:
            ctx.save_for_backward(y)
        ctx.set_materialize_grads(False)
        if want_raw and epi is not None:
            return out, y
        return out if want_raw else y

    @staticmethod
    def backward(ctx, *gs):
        level, epi, coef = ctx.level, ctx.epi, ctx.coef
        g_raw = gs[0] if ctx.want_raw else None
        g_act = gs[-1] if epi is not None else None
        if g_raw is None and g_act is None:
            return None, None, None, None, None
        g = None if g_raw is None else _f32c(g_raw, "g_out")
        dev = (g if g is not None else g_act).device
        st = _stream_ptr(dev)
        if g_act is not None:
            p, relu, seed, offset, rdev = epi
            g_act = _f32c(g_act, "g_y")
            y = ctx.saved_tensors[0] if relu else None
            gated = torch.empty_like(g_act)
            _lib.call("fn_dropout_act_bwd_f32", g_act.data_ptr(), _ptr(y), gated.data_ptr(), g_act.numel(), float(p), seed, offset,
                      _ptr(rdev) if p > 0.0 else None, int(relu), st)
            g = gated if g is None else gated.add_(g)      # both outputs were read (the last layer): autograd's own accumulation, done here
        g_x = torch.empty((level.n, FN_D), dtype=torch.float32, device=dev)
        _lib.call("fn_gcn_aggregate_f32", g.data_ptr(), C.byref(level.c), 1, _ptr(coef), g_x.data_ptr(), None, st)
        return g_x, None, None, None, None


def gcn_aggregate(x, level: Level, coef=None, act=None, raw=None):
    """The graph convolution's neighbour sum on ``level`` (a plan level: the atom graph with its loop items, or the fragment graph).
    ``coef``: ``gcn_coef(level)`` for the normalised form, None for the plain sum.  ``act = (p, training, relu, rng)``: also apply
    relu?(dropout(.)) in the same launch, drawing from the Philox stream ``rng`` like ``dropout_act``.  ``raw`` (default: True without
    ``act``, False with it): return the rows before the activation; with both, the result is (raw, activated)."""
    if not x.is_cuda:
        raise _lib.FragnetHipError(f"gcn_aggregate: fragnet_amd kernels need GPU tensors (got {x.device}); there is no CPU fallback")
    epi = None
    if act is not None:
        p, training, relu, rng = act
        p_eff = float(p) if training else 0.0
        if not 0.0 <= p_eff <= 1.0:
            raise ValueError(f"gcn_aggregate: dropout probability {p_eff} outside [0, 1]")
        if p_eff > 0.0 or relu:
            seed, off = rng.take(level.n * FN_D) if p_eff > 0.0 else (0, 0)
            epi = (p_eff, bool(relu), seed, off, rng.dev if p_eff > 0.0 else None)
    want_raw = bool(raw) if raw is not None else epi is None
    if epi is None:
        want_raw = True
    return _GcnAggregate.apply(x, coef, level, want_raw, epi)


class _FragMLP(torch.autograd.Function):
    """Linear(K -> H) -> ReLU -> Linear(H -> N) (gcn2.py:26-28, ``frag_mlp``) on the dense kernels: fn_dense_fwd_f32 with the ReLU epilogue
    at p = 0, then without one; backward top-down with fn_dense_bwd_f32 (gate_scale = 1 hands the hidden layer its gradient through its
    ReLU), as ``_CellTower``."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2):
        x = _f32c(x, "x")
        W1, b1, W2, b2 = (_f32c(q, "frag_mlp parameter") for q in (W1, b1, W2, b2))
        if x.shape[0]:
            st = _stream_ptr(x.device)
            h = _plain_fwd(x, W1, b1, True, st)
            y = _plain_fwd(h, W2, b2, False, st)
        else:
            h, y = x.new_empty((0, W1.shape[0])), x.new_empty((0, W2.shape[0]))
        ctx.params, ctx.slots = (W1, b1, W2, b2), [grad_slot(q) for q in (W1, b1, W2, b2)]
        ctx.save_for_backward(x, h)
        return y

    @staticmethod
    def backward(ctx, g):
        x, h = ctx.saved_tensors
        g = _f32c(g, "g")
        (W1, b1, W2, b2), slots = ctx.params, ctx.slots
        dW1, db1, dW2, db2 = (grad_buffer(q, s) for q, s in zip(ctx.params, slots))
        st = _stream_ptr(x.device)
        g_h = torch.empty_like(h)
        _plain_bwd(g, h, W2, g_h, True, dW2, db2, st)
        g_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _plain_bwd(g_h, x, W1, g_x, False, dW1, db1, st)
        return g_x, dW1, db1, dW2, db2


def frag_mlp(x, lin1, lin2):
    """``lin2(relu(lin1(x)))`` as ``_FragMLP``.  More than ``DENSE_MAX_ROWS`` rows, a Linear without bias or widths that are not multiples
    of 4 fall back to plain torch ops (library GEMMs), the way ``mlp_head`` and ``cell_tower`` treat tall inputs."""
    if not x.is_cuda:
        raise _lib.FragnetHipError(f"frag_mlp: fragnet_amd kernels need GPU tensors (got {x.device}); there is no CPU fallback")
    rows = x.shape[0]
    if lin1.bias is None or lin2.bias is None or not (_dense_ok(rows, lin1.weight) and _dense_ok(rows, lin2.weight)):
        return torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, lin1.weight, lin1.bias)), lin2.weight, lin2.bias)
    return _FragMLP.apply(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias)


# ======================================================================================
# nearest neighbours in embedding space: reciprocal row norms and the fused similarity + top-k update (csrc/topk.hip)
# ======================================================================================
TOPK_METRICS = {"dot": 0, "cosine": 1, "l2": 2}
TOPK_MAX_K = 32
TOPK_WIDTHS = (128, 256)


def rows_rnorm(x: torch.Tensor) -> torch.Tensor:
    """``1 / max(|x_i|_2, 1e-12)`` of the rows of ``x`` [n, d]: one summation order per row, whatever n."""
    x = _f32c(x, "rows_rnorm: x")
    if x.dim() != 2:
        raise ValueError(f"rows_rnorm: x must be [n, d], got {tuple(x.shape)}")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.call("fn_rows_rnorm_f32", x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), _stream_ptr(x.device))
    return out


def topk_metric(metric) -> int:
    """0 / 1 / 2 of ``"dot"`` / ``"cosine"`` / ``"l2"`` (squared L2: smaller is better); anything else is refused."""
    if isinstance(metric, str) and metric in TOPK_METRICS:
        return TOPK_METRICS[metric]
    if isinstance(metric, int) and not isinstance(metric, bool) and metric in TOPK_METRICS.values():
        return metric
    raise ValueError(f"unknown metric {metric!r}: one of {', '.join(TOPK_METRICS)} (or 0, 1, 2)")


def topk_k(k) -> int:
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k must be an integer in [1, {TOPK_MAX_K}], got {k!r}")
    return k


class TopK:
    """Running best-``k`` lists of ``n_q`` queries over a library that arrives chunk by chunk (fn_topk_update_f32): the [n_q, n_lib]
    scores never exist.  Lists are sorted best first under a total order (better score, then smaller global row id), empty slots are
    index -1 with score -inf (+inf for ``"l2"``), and the lists are bit-identical however the library is cut into chunks.
    ``splits``: 0 leaves the launch shape to the library; 1..63 forces that many slices per chunk (the result does not depend on it)."""

    def __init__(self, n_q: int, k: int, metric, device, splits: int = 0):
        self.k, self.metric = topk_k(k), topk_metric(metric)
        if not isinstance(n_q, int) or n_q < 0:
            raise ValueError(f"n_q must be a non-negative integer, got {n_q!r}")
        if not isinstance(splits, int) or not 0 <= splits <= 63:
            raise ValueError(f"splits must be in [0, 63], got {splits!r}")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.FragnetHipError(f"TopK: fragnet_amd kernels need a GPU device (got {device}); there is no CPU fallback")
        self.n_q, self.device, self.splits = n_q, device, splits
        self.score = torch.full((n_q, self.k), float("inf") if self.metric == 2 else float("-inf"), dtype=torch.float32, device=device)
        self.index = torch.full((n_q, self.k), -1, dtype=torch.int64, device=device)
        self._scratch = None

    def _aux(self, t, rows: int, name: str):
        if self.metric == 0:
            return None
        if t is None:
            raise ValueError(f"TopK.update: {name} is required for the cosine (reciprocal norms) and l2 (squared norms) metrics")
        t = _f32c(t, f"TopK.update: {name}")
        if t.shape != (rows,):
            raise ValueError(f"TopK.update: {name} must be [{rows}], got {tuple(t.shape)}")
        return t

    def update(self, q, lib, index_base: int, q_aux=None, lib_aux=None, exclude=None) -> "TopK":
        """Folds ``lib`` [n_lib, d], whose row 0 is global row ``index_base``, into the lists of ``q`` [n_q, d]; d is 128 or 256.
        ``q_aux`` / ``lib_aux``: ``rows_rnorm`` of the two for ``"cosine"``, the squared norms for ``"l2"``.  ``exclude`` (int64 [n_q]):
        the global row a query skips, -1 for none."""
        q, lib = _f32c(q, "TopK.update: q"), _f32c(lib, "TopK.update: lib")
        if q.dim() != 2 or lib.dim() != 2 or q.shape[0] != self.n_q or q.shape[1] != lib.shape[1]:
            raise ValueError(f"TopK.update: q must be [{self.n_q}, d] and lib [n_lib, d], got {tuple(q.shape)} and {tuple(lib.shape)}")
        if q.shape[1] not in TOPK_WIDTHS:
            raise _lib.FragnetHipError(f"TopK.update: rows of {q.shape[1]} floats; the kernel is built for {TOPK_WIDTHS}")
        q_aux, lib_aux = self._aux(q_aux, self.n_q, "q_aux"), self._aux(lib_aux, lib.shape[0], "lib_aux")
        if exclude is not None:
            if not exclude.is_cuda:
                raise _lib.FragnetHipError(f"TopK.update: exclude: fragnet_amd kernels need GPU tensors (got {exclude.device})")
            if exclude.dtype != torch.int64:
                raise TypeError(f"TopK.update: exclude: expected int64 row ids, got {exclude.dtype}")
            exclude = exclude.contiguous()
            if exclude.shape != (self.n_q,):
                raise ValueError(f"TopK.update: exclude must be [{self.n_q}], got {tuple(exclude.shape)}")
        t = _lib.Topk(q.data_ptr(), lib.data_ptr(), _ptr(q_aux), _ptr(lib_aux), _ptr(exclude), self.score.data_ptr(), self.index.data_ptr(),
                      None, 0, self.n_q, lib.shape[0], int(index_base), q.shape[1], self.k, self.metric, self.splits)
        need = _lib.load().fn_topk_scratch_bytes(C.byref(t))
        _lib.check(0 if need >= 0 else need, "fn_topk_scratch_bytes")
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        t.scratch, t.scratch_bytes = self._scratch.data_ptr(), self._scratch.numel()
        _lib.call("fn_topk_update_f32", C.byref(t), _stream_ptr(self.device))
        return self

    def result(self):
        """``(score [n_q, k], index [n_q, k])``: the lists as they stand."""
        return self.score, self.index


# ======================================================================================
# evaluation metrics on the device: exact pair-concordance counts and fp64 regression sums (csrc/metrics.hip)
# ======================================================================================
from .metrics import CONC_FIELDS, SUMS_FIELDS          # noqa: E402  (the columns of the two tables, named where they are read)

CONC_TILE = _lib.CONC_TILE          # rows of the count kernel's i- and j-tiles
SUMS_CHUNK = _lib.SUMS_CHUNK        # rows of one partial row of the sums


def _metrics_launch(name: str, sums: bool, pred, label, label_floor, scale, shift, splits, out_dtype, fields):
    pred, label = _f32c(pred, f"{name}: pred"), _f32c(label, f"{name}: label")
    if pred.dim() != 2 or pred.shape != label.shape or pred.device != label.device:
        raise ValueError(f"{name}: pred and label must be [n, c] on one device, got {tuple(pred.shape)} and {tuple(label.shape)}")
    n, c = pred.shape
    if not 1 <= c <= _lib.METRICS_MAX_COLS or n > 1 << 24:
        raise ValueError(f"{name}: c must be in [1, {_lib.METRICS_MAX_COLS}] and n <= 2^24, got n = {n}, c = {c}")
    if not isinstance(splits, int) or isinstance(splits, bool) or splits < 0:
        raise ValueError(f"{name}: splits must be a non-negative integer, got {splits!r}")
    out = torch.empty((c, fields), dtype=out_dtype, device=pred.device)
    m = _lib.Metrics(pred.data_ptr(), label.data_ptr(), out.data_ptr(), None, 0, n, float(label_floor), float(scale), float(shift), c, splits)
    need = _lib.load().fn_metrics_scratch_bytes(C.byref(m), int(sums))
    _lib.check(0 if need >= 0 else need, "fn_metrics_scratch_bytes")
    scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=pred.device)
    m.scratch, m.scratch_bytes = scratch.data_ptr(), scratch.numel()
    _lib.call(name, C.byref(m), _stream_ptr(pred.device))
    return out


def pair_concordance(pred: torch.Tensor, label: torch.Tensor, label_floor: float = float("-inf"), splits: int = 0) -> torch.Tensor:
    """Exact ordered-pair counts per column of ``pred`` / ``label`` [n, c] (fn_pair_concordance_f32): int64 [c, 5] on the device, the
    fields in ``CONC_FIELDS`` order.  Row i is valid in column k iff ``label[i, k] >= label_floor`` (never for a NaN label); -0.5 drops
    the classification targets' missing labels.  ``splits``: 0 leaves the launch shape to the library, else that many j-slices -- the
    counts do not depend on it.  No host read: ``metrics.roc_auc`` / ``metrics.concordance_index`` turn the copied table into numbers."""
    return _metrics_launch("fn_pair_concordance_f32", False, pred, label, label_floor, 1.0, 0.0, splits, torch.int64, len(CONC_FIELDS))


def regression_sums(pred: torch.Tensor, label: torch.Tensor, label_floor: float = float("-inf"), scale: float = 1.0, shift: float = 0.0,
                    splits: int = 0) -> torch.Tensor:
    """fp64 sums per column over the valid rows (fn_regression_sums_f32): float64 [c, 8] on the device, the fields in ``SUMS_FIELDS``
    order, with ``p = pred * float32(scale) + float32(shift)`` rounded twice in fp32 as numpy does.  One fixed order of addition: the
    bits are the same for every run and every ``splits``."""
    return _metrics_launch("fn_regression_sums_f32", True, pred, label, label_floor, scale, shift, splits, torch.float64, len(SUMS_FIELDS))


# ======================================================================================
# diverse subsets of embedding rows: greedy k-centre, one launch per pick (csrc/kcenter.hip)
# ======================================================================================
KCENTER_METRICS = {"l2": 0, "cosine": 1}
KCENTER_WIDTHS = (128, 256)
KCENTER_MAX_SPLITS = 512


def kcenter_metric(metric) -> int:
    """0 / 1 of ``"l2"`` (squared L2, direct form) / ``"cosine"`` (cosine distance); ``"dot"`` is no distance and is refused."""
    if isinstance(metric, str) and metric in KCENTER_METRICS:
        return KCENTER_METRICS[metric]
    if isinstance(metric, int) and not isinstance(metric, bool) and metric in KCENTER_METRICS.values():
        return metric
    hint = " (a dot product is not a distance: nothing is farthest under it)" if metric == "dot" else ""
    raise ValueError(f"unknown metric {metric!r}: one of {', '.join(KCENTER_METRICS)} (or 0, 1){hint}")


def _count(v, name: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or v < 0:
        raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
    return v


class KCenter:
    """Greedy k-centre over ``n`` rows of width ``d`` (fn_kcenter_pick_f32 / fn_kcenter_seed_f32): ``mind`` [n] the distance of every row
    to its nearest centre so far, ``label`` [n] that centre's ordinal (-1: none), ``picked`` [cap] the rows in pick order (by ordinal; a
    seed's slot holds -1), ``radius`` [cap + 1].  A pick is the unpicked row with the largest ``mind``, ties to the smaller row; an update
    is strict, so the earlier centre keeps a tie.  Every result is bit-identical for every ``splits`` (0 leaves the launch shape to the
    library; 1..512 allows at most that many workgroups) and for ``pick(a)`` then ``pick(b)`` against ``pick(a + b)``.  Nothing reads
    device memory on the host.  ``init_distance`` [n] starts ``mind`` there instead of at +inf (negative values count as 0; a NaN row is
    never lowered and never picked while a number is left)."""

    def __init__(self, n: int, d: int, metric, device, cap: int, splits: int = 0, init_distance=None):
        self.n, self.cap, self.metric = _count(n, "n"), _count(cap, "cap"), kcenter_metric(metric)
        if _count(splits, "splits") > KCENTER_MAX_SPLITS:
            raise ValueError(f"splits must be in [0, {KCENTER_MAX_SPLITS}], got {splits!r}")
        if d not in KCENTER_WIDTHS:
            raise _lib.FragnetHipError(f"KCenter: rows of {d!r} floats; the kernel is built for {KCENTER_WIDTHS}")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.FragnetHipError(f"KCenter: fragnet_amd kernels need a GPU device (got {device}); there is no CPU fallback")
        self.d, self.device, self.splits = d, device, splits
        if init_distance is None:
            self.mind = torch.full((n,), float("inf"), dtype=torch.float32, device=device)
        else:
            init_distance = _f32c(init_distance, "KCenter: init_distance")
            if init_distance.shape != (n,):
                raise ValueError(f"KCenter: init_distance must be [{n}], got {tuple(init_distance.shape)}")
            # a copy; a negative value (the rounding of an expanded-form distance) counts as 0, and -0.0, the kernel's mark of a picked
            # row, becomes +0.0; a NaN stays
            self.mind = init_distance.to(device).clamp_min(0.0) + 0.0
        self.label = torch.full((n,), -1, dtype=torch.int32, device=device)
        self.picked = torch.full((cap,), -1, dtype=torch.int64, device=device)
        self.radius = torch.full((cap + 1,), float("nan"), dtype=torch.float32, device=device)
        self.count = torch.zeros(1, dtype=torch.int64, device=device)
        self.centres, self.picks = 0, 0                         # the host's mirror of count, and how many of them are rows
        k = self._descriptor(None, None)
        need = _lib.load().fn_kcenter_scratch_bytes(C.byref(k))
        _lib.check(0 if need >= 0 else need, "fn_kcenter_scratch_bytes")
        self._scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=device)

    def _descriptor(self, x, aux):
        scratch = getattr(self, "_scratch", None)
        return _lib.Kcenter(_ptr(x), _ptr(aux), self.mind.data_ptr(), self.label.data_ptr(), self.picked.data_ptr(), self.radius.data_ptr(),
                            self.count.data_ptr(), _ptr(scratch), 0 if scratch is None else scratch.numel(), self.n, self.cap, self.centres,
                            self.picks, self.d, self.metric, self.splits)

    def _rows(self, t, rows, name: str):
        t = _f32c(t, name)
        if t.dim() != 2 or t.shape[1] != self.d or (rows is not None and t.shape[0] != rows):
            raise ValueError(f"{name} must be [{'s' if rows is None else rows}, {self.d}], got {tuple(t.shape)}")
        return t

    def _aux(self, t, rows: int, name: str):
        if self.metric == 0:
            return None
        if t is None:
            raise ValueError(f"{name} is required for the cosine metric (ops.rows_rnorm of the rows)")
        t = _f32c(t, name)
        if t.shape != (rows,):
            raise ValueError(f"{name} must be [{rows}], got {tuple(t.shape)}")
        return t

    def seed(self, x, centres, centres_aux=None, aux=None) -> "KCenter":
        """Folds the rows of ``centres`` [s, d] in as centres ``count .. count + s - 1`` of the rows ``x`` [n, d]: an update launch each,
        no pick.  ``aux`` / ``centres_aux``: ``rows_rnorm`` of the two for ``"cosine"``."""
        x, centres = self._rows(x, self.n, "KCenter.seed: x"), self._rows(centres, None, "KCenter.seed: centres")
        s = centres.shape[0]
        aux, centres_aux = self._aux(aux, self.n, "KCenter.seed: aux"), self._aux(centres_aux, s, "KCenter.seed: centres_aux")
        if self.centres + s > self.cap:
            raise ValueError(f"KCenter.seed: {self.centres} centres + {s} seeds exceed cap = {self.cap}")
        _lib.call("fn_kcenter_seed_f32", C.byref(self._descriptor(x, aux)), centres.data_ptr(), _ptr(centres_aux), s, _stream_ptr(self.device))
        self.centres += s
        return self

    def pick(self, x, k: int, first=None, aux=None) -> "KCenter":
        """``k`` more picks among the rows ``x`` [n, d] (the same rows in every call of a run).  ``first``: the row of the very first
        centre -- only before any seed or pick; ``None``: the arg-max, as for every later pick."""
        x, k = self._rows(x, self.n, "KCenter.pick: x"), _count(k, "k")
        aux = self._aux(aux, self.n, "KCenter.pick: aux")
        if k > self.n - self.picks:
            raise ValueError(f"KCenter.pick: k = {k} exceeds the {self.n - self.picks} rows not yet picked (n = {self.n})")
        if self.centres + k > self.cap:
            raise ValueError(f"KCenter.pick: {self.centres} centres + {k} picks exceed cap = {self.cap}")
        if first is not None:
            if self.centres > 0:
                raise ValueError("KCenter.pick: a first row can only be named before any centre; after seeds or picks the arg-max decides")
            if not isinstance(first, int) or isinstance(first, bool) or not (0 <= first < self.n or (self.n == 0 and k == 0)):
                raise ValueError(f"KCenter.pick: first must be a row in [0, {self.n}), got {first!r}")
        _lib.call("fn_kcenter_pick_f32", C.byref(self._descriptor(x, aux)), -1 if first is None or self.n == 0 else first, k,
                  _stream_ptr(self.device))
        if self.n > 0:
            self.centres, self.picks = self.centres + k, self.picks + k
        return self

    def result(self):
        """``(picked[:count], radius[:count + 1], mind, label)`` as device tensors; ``count`` is the host's own tally, nothing is read."""
        return self.picked[:self.centres], self.radius[:self.centres + 1], self.mind, self.label


# ======================================================================================
# moments and projections of a row table: fp64 count / column sums / Gram matrix, and rows onto a few directions (csrc/moments.hip)
# ======================================================================================
MOMENTS_WIDTHS = (128, 256)
MOMENTS_CHUNK = _lib.MOMENTS_CHUNK      # rows of one fp32 fma chain
MOMENTS_GROUP = _lib.MOMENTS_GROUP      # chunks of one super-chunk = one scratch slot


def _moment_rows(x, d, name: str):
    x = _f32c(x, name)
    if x.dim() != 2 or (d is not None and x.shape[1] != d):
        raise ValueError(f"{name} must be [n, {'d' if d is None else d}], got {tuple(x.shape)}")
    if x.shape[1] not in MOMENTS_WIDTHS:
        raise _lib.FragnetHipError(f"{name}: rows of {x.shape[1]} floats; the kernel is built for {MOMENTS_WIDTHS}")
    return x


def _moment_shift(shift, x, name: str):
    if shift is None:
        return None
    shift = _f32c(shift, name)
    if shift.shape != (x.shape[1],) or shift.device != x.device:
        raise ValueError(f"{name} must be [{x.shape[1]}] on {x.device}, got {tuple(shift.shape)} on {shift.device}")
    return shift


class Moments:
    """Running count, column sums and Gram matrix of rows of width ``d`` that arrive batch by batch (fn_rows_moments_f32), in fp64 on the
    device: with ``z = x - shift`` (one fp32 subtraction), ``sum[j] = sum_i z_ij`` and ``gram[j][l] = sum_i z_ij z_il``.  No [n, d]
    temporary exists.  Inside chunks of ``MOMENTS_CHUNK`` rows an entry is one fp32 fma chain; everything above that is added in fp64 in an
    order that depends on the batch's row count alone, so a batch's contribution is bit-identical for every ``splits`` (0 leaves the
    launch shape to the library; 1..63 allows at most that many workgroups).  Chunks are counted per ``update``: the same rows cut into
    different batches may differ in the last bits.  The shift is fixed by the first ``update``."""

    def __init__(self, d: int, device, splits: int = 0):
        if d not in MOMENTS_WIDTHS:
            raise _lib.FragnetHipError(f"Moments: rows of {d!r} floats; the kernel is built for {MOMENTS_WIDTHS}")
        if not isinstance(splits, int) or isinstance(splits, bool) or not 0 <= splits <= 63:
            raise ValueError(f"splits must be in [0, 63], got {splits!r}")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.FragnetHipError(f"Moments: fragnet_amd kernels need a GPU device (got {device}); there is no CPU fallback")
        self.d, self.device, self.splits = d, device, splits
        self.n, self.shift, self._given, self._updates = 0, None, None, 0
        self.sum = torch.zeros(d, dtype=torch.float64, device=device)
        self.gram = torch.zeros((d, d), dtype=torch.float64, device=device)
        self._scratch = None

    def update(self, x, shift=None) -> "Moments":
        """Adds the rows ``x`` [n, d] in.  ``shift`` [d] (``None``: zeros) is kept by the first call; a later call hands in the same
        tensor, an equal one, or ``None`` for "the one in use"."""
        x = _moment_rows(x, self.d, "Moments.update: x")
        if x.device != self.device:
            raise ValueError(f"Moments.update: x is on {x.device}, the moments on {self.device}")
        shift = _moment_shift(shift, x, "Moments.update: shift")
        if self._updates == 0:
            self.shift, self._given = (None if shift is None else shift.clone()), shift
        elif shift is not None and shift is not self._given and (self.shift is None or not torch.equal(shift, self.shift)):
            raise ValueError("Moments.update: the shift is fixed by the first update; this one differs")      # (the same tensor object again: no comparison, which would wait for the device)
        m = _lib.Moments(x.data_ptr(), _ptr(self.shift), self.sum.data_ptr(), self.gram.data_ptr(), None, 0, x.shape[0], self.d, 1, self.splits)
        need = _lib.load().fn_moments_scratch_bytes(C.byref(m))
        _lib.check(0 if need >= 0 else need, "fn_moments_scratch_bytes")
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        m.scratch, m.scratch_bytes = self._scratch.data_ptr(), self._scratch.numel()
        _lib.call("fn_rows_moments_f32", C.byref(m), _stream_ptr(self.device))
        self.n += int(x.shape[0])
        self._updates += 1
        return self

    def result(self):
        """``(n, sum [d], gram [d, d])``: the host's row count and the two float64 device tensors as they stand."""
        return self.n, self.sum, self.gram


def rows_project(x, W, shift=None, want_rows: bool = True, want_sq: bool = False):
    """``(out | None, sq | None)`` of the rows ``x`` [n, d] (d 128 or 256) and the directions ``W`` [d, k], 1 <= k <= d
    (fn_rows_project_f32): ``out[i][c]`` is one fp32 fma chain of ``(x_ip - shift_p) W_pc`` over a fixed order of p, ``sq[i]`` one fp32
    fma chain of ``out[i][c]^2`` over c ascending.  A row's results depend on that row, ``shift`` and ``W`` alone, so a slice of the rows
    gives the same bits as the whole table.  ``want_rows=False``: no [n, k] table is written anywhere."""
    x = _moment_rows(x, None, "rows_project: x")
    W = _f32c(W, "rows_project: W")
    d = x.shape[1]
    if W.dim() != 2 or W.shape[0] != d or W.device != x.device:
        raise ValueError(f"rows_project: W must be [{d}, k] on {x.device}, got {tuple(W.shape)} on {W.device}")
    k = int(W.shape[1])
    if not 1 <= k <= d:
        raise ValueError(f"rows_project: k must be in [1, {d}], got {k}")
    shift = _moment_shift(shift, x, "rows_project: shift")
    if not want_rows and not want_sq:
        raise ValueError("rows_project: nothing is wanted (want_rows and want_sq are both off)")
    n = int(x.shape[0])
    out = torch.empty((n, k), dtype=torch.float32, device=x.device) if want_rows else None
    sq = torch.empty(n, dtype=torch.float32, device=x.device) if want_sq else None
    p = _lib.Project(x.data_ptr(), _ptr(shift), W.data_ptr(), _ptr(out), _ptr(sq), n, d, k)
    _lib.call("fn_rows_project_f32", C.byref(p), _stream_ptr(x.device))
    return out, sq
