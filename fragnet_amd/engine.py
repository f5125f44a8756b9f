"""The whole encoder (reference FragNet.forward, gat2.py:381-442) as one autograd node backed by two C calls:
fn_encoder_forward / fn_encoder_backward walk the layers inside libfragnet_hip.so and enqueue every kernel
(MFMA projections, node scalars, segmented softmax-aggregate, segment sum, dropout+ReLU) on the current
stream.  Python does not see the per-level ops, so a training step costs two ctypes calls for the encoder
instead of ~250 autograd nodes.

``encoder_forward`` is the one way in.  It refuses what no pass serves, then runs one of three passes on the shared body
``_begin_pass`` / ``_end_pass``: the autograd node ``_EncoderFn`` (fn_encoder_forward, or fn_encoder_forward_keep behind the input
gate), ``_masked_forward`` (fn_encoder_forward_masked) or ``_attn_forward`` (fn_encoder_forward_attn).  What a pass is, beside its
three input tables and the parameters, is one ``_Spec``.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _lib, ops
from ._lib import Encoder, FN_D, LAYER_FIELDS, LayerWeights, SegPlan
from .plan import GraphPlan, _stream_ptr

# dev switch for A/B measurements: evaluation passes save everything a backward pass would read even when none can follow
_EVAL_SAVES = os.environ.get("FRAGNET_EVAL_SAVES", "0") == "1"


def layer_param_list(layer) -> List[torch.nn.Parameter]:
    """Parameters of one FragNetLayerA in the order of fn_layer_weights."""
    if hasattr(layer, "cnx_attr_transform"):        # gat2_edge layer: no fragment-bond parameters, the cnx_attr Linear sits in emb_fb_*
        ph = layer.engine_placeholders()
        return [layer.projection_b.weight, layer.projection_b.bias, layer.projection_a.weight, layer.projection_a.bias,
                ph["proj_fb_w"], ph["proj_fb_b"], layer.edge_attr_bond_embed.weight, layer.edge_attr_bond_embed.bias,
                layer.cnx_attr_transform.weight, layer.cnx_attr_transform.bias, layer.a_b, layer.a, layer.f, ph["f_a_b"]]
    return [layer.projection_b.weight, layer.projection_b.bias, layer.projection_a.weight, layer.projection_a.bias,
            layer.projection_fb.weight, layer.projection_fb.bias, layer.edge_attr_bond_embed.weight,
            layer.edge_attr_bond_embed.bias, layer.edge_attr_fbond_embed.weight, layer.edge_attr_fbond_embed.bias,
            layer.a_b, layer.a, layer.f, layer.f_a_b]


NP = len(LAYER_FIELDS)
F_IDX = LAYER_FIELDS.index("f")
LITE_DEAD = {LAYER_FIELDS.index(n) for n in ("proj_fb_w", "proj_fb_b", "emb_fb_w", "emb_fb_b", "f", "f_a_b")}
EDGE_DEAD = {LAYER_FIELDS.index(n) for n in ("proj_fb_w", "proj_fb_b", "f_a_b")}          # placeholders of a gat2_edge layer
EDGE_LAST_ONLY = {LAYER_FIELDS.index(n) for n in ("emb_fb_w", "emb_fb_b", "f")}             # read by the last layer's fragment graph only


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.FragnetHipError(f"{name}: the encoder engine needs GPU tensors (got {t.device}); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


class _Spec(NamedTuple):
    """Everything of one encoder pass that is no input table and no parameter: _EncoderFn.apply's one non-tensor argument.  None of
    its tensors is differentiable."""
    plan: GraphPlan
    cos_sorted: torch.Tensor
    fattr_sorted: torch.Tensor
    n_layers: int
    heads: int
    drop_p: float = 0.0
    training: bool = False
    seed: int = 0
    offset: int = 0
    offset_dev: Optional[torch.Tensor] = None
    variant: int = 0
    no_backward: bool = False
    edge_outputs: bool = True
    keep_atoms: Optional[torch.Tensor] = None


def _describe(tables, params: Sequence[torch.Tensor], spec: _Spec) -> Encoder:
    plan, variant, fattr_sorted = spec.plan, spec.variant, spec.fattr_sorted
    x_atoms, bond_nodes, fbond_nodes = tables
    e = Encoder()
    e.n_layers, e.heads = spec.n_layers, spec.heads
    e.k_atom0, e.k_bond0, e.k_fbond0 = x_atoms.shape[1], bond_nodes.shape[1], fbond_nodes.shape[1]
    e.k_fattr = fattr_sorted.shape[0]
    e.training, e.drop_p = int(spec.training), float(spec.drop_p)
    e.no_backward = int(bool(spec.no_backward) and not spec.training)       # an evaluation pass nobody differentiates saves nothing for a backward pass
    e.variant = int(variant)
    e.seed, e.offset = spec.seed, spec.offset
    e.offset_dev = None if spec.offset_dev is None else spec.offset_dev.data_ptr()
    L = plan.levels
    e.N, e.E, e.F, e.EF = L["atom"].n, L["bond"].n, L["frag"].n, L["fbond"].n
    e.bond, e.atom, e.fbond, e.frag = L["bond"].c, L["atom"].c, L["fbond"].c, L["frag"].c
    s = plan.segs["a2f"]
    e.a2f = SegPlan(s.rowptr.data_ptr(), s.perm.data_ptr(), s.index.data_ptr(), s.n_seg, s.n_items, s.pos_base, 0)
    e.x_atoms, e.bond_nodes, e.fbond_nodes = x_atoms.data_ptr(), bond_nodes.data_ptr(), fbond_nodes.data_ptr()
    e.cos_sorted, e.fattr_sorted = spec.cos_sorted.data_ptr(), fattr_sorted.data_ptr()
    raw_b, raw_f = plan.pending.get("bond"), plan.pending.get("frag" if variant == 2 else "fbond")      # sorted copies not filled yet: the forward does it
    e.cos_raw = None if raw_b is None else raw_b.data_ptr()
    e.fattr_raw = None if raw_f is None else raw_f.data_ptr()
    for l in range(spec.n_layers):
        for k, name in enumerate(LAYER_FIELDS):
            setattr(e.w[l], name, params[l * NP + k].data_ptr())
    # molecule CSRs: with them fn_encoder_* runs the molecule-resident fused kernels (include/fragnet_hip.h, fn_encoder.n_mols)
    ma, mf = plan.segs.get("mol_atoms"), plan.segs.get("mol_frags")
    if ma is not None and mf is not None and ma.n_seg == mf.n_seg:
        e.mol_atoms = SegPlan(ma.rowptr.data_ptr(), ma.perm.data_ptr(), ma.index.data_ptr(), ma.n_seg, ma.n_items, ma.pos_base, 0)
        e.mol_frags = SegPlan(mf.rowptr.data_ptr(), mf.perm.data_ptr(), mf.index.data_ptr(), mf.n_seg, mf.n_items, mf.pos_base, 0)
        e.n_mols = ma.n_seg
        counts = getattr(plan, "real_mols", None)
        e.counts_dev = None if counts is None else counts.data_ptr()
        e.status = plan._status.data_ptr()
        e.mol_contiguous = int(bool(getattr(plan, "mol_contiguous", False)))       # CollatedBatch: collate_fn's layout
    return e


def _out_ptrs(outs, edge_outputs: bool, spare=None):
    """The four output pointers of a pass.  edge_outputs = False: the caller reads neither the bond nor the fragment-bond output (a
    finetune head): the library gets NULL for them and does not store the last layer's activated rows; two empty tensors stand in.
    ``spare``: what an output of no rows points at instead of NULL (the read-out pass)."""
    return [(o.data_ptr() or spare) if (edge_outputs or k < 2) else None for k, o in enumerate(outs)]


_Pass = namedtuple("_Pass", "e ws outs out_ptrs pooled fused tables params spare dev lib")


def _begin_pass(tables, params, spec: _Spec, stand_in: bool = False) -> _Pass:
    """What the four forward entry points share: float32 tables and parameters, the descriptor, its workspace, the four outputs, the
    readout where the fused tail writes one (``fused``; an empty placeholder otherwise) and the output pointers.  ``stand_in`` (the
    read-out pass only; enc_check refuses a null input on the others): see below."""
    tables = tuple(_f32(t, name) for t, name in zip(tables, ("x_atoms", "node_features_bonds", "node_features_fbonds")))
    params = tuple(_f32(p, "parameter") for p in params)
    dev, lib = tables[0].device, _lib.load()
    e = _describe(tables, params, spec)
    # a batch without fragment connections (EF == 0: one-fragment molecules stripped of their placeholder row) has empty fragment-bond
    # tensors, whose data_ptr() is null; the descriptor wants a pointer for every input, read or not: a stand-in that no launch reads
    # (a level of no rows launches nothing).  out_bond and out_fbond are wanted together: an output of no rows gets its pointer too
    spare = None
    if stand_in and (e.EF == 0 or spec.plan.levels["fbond"].m == 0):
        spare = torch.zeros(max(e.k_fbond0, e.k_fattr, FN_D), dtype=torch.float32, device=dev)
        e.fbond_nodes = e.fbond_nodes or spare.data_ptr()
        e.fattr_sorted = e.fattr_sorted or spare.data_ptr()
    # keep_atoms: the input gate of x_atoms (fn_encoder_forward_keep); its gated copy may live behind the plain workspace
    ws_floats = lib.fn_encoder_ws_floats if spec.keep_atoms is None else lib.fn_encoder_keep_ws_floats
    ws = torch.empty(ws_floats(C.byref(e)), dtype=torch.float32, device=dev)
    e.ws, e.ws_floats = ws.data_ptr(), ws.numel()
    outs = [torch.empty((n if (spec.edge_outputs or k < 2) else 0, FN_D), dtype=torch.float32, device=dev) for k, n in enumerate((e.N, e.F, e.E, e.EF))]
    # molecule-contiguous batches: the last layer's fragment tail is one molecule-resident launch that also writes the
    # readout cat(scatter_add(x_atoms, batch), scatter_add(x_frags, frag_batch)) (gat2.py:820-823) -- a fifth output
    fused = bool(lib.fn_encoder_fused_tail(C.byref(e)))
    pooled = torch.empty((e.n_mols, 2 * FN_D) if fused else 0, dtype=torch.float32, device=dev)      # not fused: the caller pools with ops.pool_cat
    e.pooled = pooled.data_ptr() if fused else None
    return _Pass(e, ws, outs, _out_ptrs(outs, spec.edge_outputs, None if spare is None else spare.data_ptr()), pooled, fused, tables, params,
                 spare, dev, lib)


def _end_pass(plan: GraphPlan, variant: int) -> None:
    """The forward filled the plan's sorted attribute copies: they are pending no more."""
    plan.pending.pop("bond", None)
    plan.pending.pop("frag" if variant == 2 else "fbond", None)


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_atoms, bond_nodes, fbond_nodes, spec: _Spec, *params):
        ctx.param_objs, ctx.slots = params, [ops.grad_slot(p) for p in params]
        ps = _begin_pass((x_atoms, bond_nodes, fbond_nodes), params, spec)
        e, outs, keep_atoms = ps.e, ps.outs, spec.keep_atoms
        if keep_atoms is None:
            _lib.check(ps.lib.fn_encoder_forward(C.byref(e), *ps.out_ptrs, _stream_ptr(ps.dev)), "fn_encoder_forward")
        else:
            _lib.check(ps.lib.fn_encoder_forward_keep(C.byref(e), keep_atoms.data_ptr(), *ps.out_ptrs, _stream_ptr(ps.dev)), "fn_encoder_forward_keep")
        _end_pass(spec.plan, spec.variant)
        e.pooled = None
        e.cos_raw = e.fattr_raw = None           # the backward pass reads the sorted copies only
        ctx.desc = e
        ctx.keep = (spec.plan, *ps.tables, spec.cos_sorted, spec.fattr_sorted, ps.ws, spec.offset_dev, keep_atoms)
        ctx.n_layers, ctx.variant, ctx.edge_outputs = spec.n_layers, spec.variant, spec.edge_outputs
        ctx.save_for_backward(*ps.params, *outs)
        ctx.set_materialize_grads(False)
        dead = ([] if spec.edge_outputs else [outs[2], outs[3]]) + ([] if ps.fused else [ps.pooled])
        if dead:
            ctx.mark_non_differentiable(*dead)           # (at most one call per forward)
        return tuple(outs) + (ps.pooled,)

    @staticmethod
    def backward(ctx, g_atoms, g_frags, g_bond, g_fbond, g_pooled):
        n_layers = ctx.n_layers
        saved = ctx.saved_tensors
        params, outs = saved[: n_layers * NP], saved[n_layers * NP:]
        e = ctx.desc
        dev = outs[0].device
        lib = _lib.load()
        gs = [None if g is None else _f32(g, "grad") for g in (g_atoms, g_frags, g_bond, g_fbond)]
        g_pooled = None if g_pooled is None else _f32(g_pooled, "grad")
        e.g_pooled = None if g_pooled is None else g_pooled.data_ptr()       # only a fused-tail forward has a differentiable readout
        grads = [ops.grad_buffer(p, slot) for p, slot in zip(ctx.param_objs, ctx.slots)]      # FlatAdam slots where they exist
        gw = (LayerWeights * n_layers)()
        for l in range(n_layers):
            for k, name in enumerate(LAYER_FIELDS):
                setattr(gw[l], name, grads[l * NP + k].data_ptr())
        # gradients of the three input tables (layer 0's projections, fn_encoder_backward_inputs): only where one is asked for.  The
        # scratch is then zero-filled: a level no gradient reaches is not written by the pass, and its input gradient is zero
        need_in = tuple(ctx.needs_input_grad[:3])
        scratch = (torch.zeros if any(need_in) else torch.empty)(lib.fn_encoder_bwd_ws_floats(C.byref(e)), dtype=torch.float32, device=dev)
        rider = take_adam_rider()                # an optimiser slice that rides in this pass's last launch (arm_adam_rider)
        e.adam_rider = None if rider is None else C.addressof(rider)
        if rider is not None:
            rider.launched = 0
        try:
            _lib.check(lib.fn_encoder_backward(C.byref(e), *_out_ptrs(outs, ctx.edge_outputs), *(None if g is None else g.data_ptr() for g in gs), gw, scratch.data_ptr(),
                                               scratch.numel(), _stream_ptr(dev)), "fn_encoder_backward")
        finally:
            e.adam_rider = None
            if rider is not None:
                _ADAM_RIDER[1] = bool(rider.launched)        # the library's word that a launch carried the slice, not ours that we offered it
        e.g_pooled = None
        g_in = _input_grads(ctx, e, scratch, need_in, dev) if any(need_in) else (None, None, None)
        out = []
        have_frags = gs[1] is not None or g_pooled is not None
        any_grad = have_frags or any(g is not None for g in gs)
        for l in range(n_layers):
            for k in range(NP):
                live = any_grad and not (k == F_IDX and not (l == n_layers - 1 and have_frags))
                if ctx.variant == 1 and k in LITE_DEAD:          # gat2_lite never reads the fragment(-bond) parameters
                    live = False
                if ctx.variant == 2 and (k in EDGE_DEAD or (k in EDGE_LAST_ONLY and not (l == n_layers - 1 and have_frags))):
                    live = False
                out.append(grads[l * NP + k] if live else None)
        return tuple(g_in) + (None,) + tuple(out)


def _input_grads(ctx, e, scratch, need, dev):
    """The second C call of a backward pass whose inputs require a gradient: dL/d(x_atoms), dL/d(bond nodes), dL/d(fragment-bond
    nodes) in one launch.  With deltas armed (arm_input_dots) the launch writes the row dots <gradient, delta> instead, and the
    tables themselves only when the armer asked to keep them."""
    lite = ctx.variant == 1
    xs = ctx.keep[1:4]
    armed = take_input_dots_request()
    deltas, keep = (armed if armed is not None else ((None, None, None), True))
    live = [bool(n) and not (k == 2 and lite) for k, n in enumerate(need)]        # gat2_lite never reads the fragment-bond nodes
    dx = [torch.empty_like(x) if (lv and keep) else None for x, lv in zip(xs, live)]
    dots = [torch.empty(x.shape[0], dtype=torch.float32, device=dev) if (lv and d is not None) else None for x, lv, d in zip(xs, live, deltas)]
    for x, d, name in zip(xs, deltas, ("x_atoms", "node_features_bonds", "node_features_fbonds")):
        if d is not None and (d.shape != x.shape or d.device != x.device or d.dtype != torch.float32 or not d.is_contiguous()):
            raise ValueError(f"arm_input_dots: the delta of {name} must be a contiguous float32 tensor of shape {tuple(x.shape)} on {x.device}")
    ptr = lambda ts: [None if t is None or t.numel() == 0 else t.data_ptr() for t in ts]
    ig = _lib.InputGrads(*ptr(dx), *ptr([d if o is not None else None for d, o in zip(deltas, dots)]), *ptr(dots))
    _lib.check(_lib.load().fn_encoder_backward_inputs(C.byref(e), scratch.data_ptr(), scratch.numel(), C.byref(ig), _stream_ptr(dev)),
               "fn_encoder_backward_inputs")
    if armed is not None:
        _INPUT_DOTS[1] = tuple(dots)
    return tuple(dx)


_INPUT_DOTS = [None, None]        # [armed (deltas, keep_dx), the dots of the backward pass that took them]


def arm_input_dots(deltas, keep_dx: bool = False) -> None:
    """The next encoder backward pass of this process whose inputs require a gradient also writes, per row of each input table with a
    delta, ``dots[m] = sum_k grad[m, k] * delta[m, k]`` (ascending k, in the launch that forms the gradient: fn_linear_dx_task.dots).
    ``deltas``: (atoms [N, Ka], bond nodes [E, Kb], fragment-bond nodes [EF, Kf]), each a contiguous float32 tensor or None.
    ``keep_dx=False``: the gradient tables themselves are not written, and the inputs' ``.grad`` stays None.  ``take_input_dots()``
    hands the result out.  Per process, like arm_adam_rider."""
    if len(deltas) != 3:
        raise ValueError("arm_input_dots: a triple (atoms, bond nodes, fragment-bond nodes)")
    _INPUT_DOTS[0], _INPUT_DOTS[1] = (tuple(deltas), bool(keep_dx)), None


def take_input_dots_request():
    r = _INPUT_DOTS[0]
    _INPUT_DOTS[0] = None
    return r


def take_input_dots():
    """The (atoms, bond nodes, fragment-bond nodes) row dots of the backward pass that followed arm_input_dots -- None where there was
    no delta or no gradient -- or None if no such pass ran; disarms either way."""
    d = _INPUT_DOTS[1]
    _INPUT_DOTS[0], _INPUT_DOTS[1] = None, None
    return d


_ADAM_RIDER = [None, False]       # [armed fn_adam_slice, was it handed to a backward pass]


def arm_adam_rider(slice_struct) -> None:
    """The next encoder backward pass of this process carries ``slice_struct`` (``_lib.AdamSlice``: parameters whose gradients are
    complete before that pass starts) in its last launch.  The caller checks ``adam_rider_taken()`` afterwards and updates
    whatever did not ride itself (graphstep.GraphedTrainStep)."""
    _ADAM_RIDER[0], _ADAM_RIDER[1] = slice_struct, False


def take_adam_rider():
    r = _ADAM_RIDER[0]
    if r is not None:
        _ADAM_RIDER[0], _ADAM_RIDER[1] = None, False
    return r


def adam_rider_taken() -> bool:
    """True if a launch of a backward pass carried the armed slice (fn_adam_slice.launched, set by fn_encoder_backward); disarms
    either way.  The state is per process (one training step at a time), not per thread."""
    taken = _ADAM_RIDER[1]
    _ADAM_RIDER[0], _ADAM_RIDER[1] = None, False
    return taken


def _is_row_bytes(t, rows: int) -> bool:
    return torch.is_tensor(t) and t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.numel() == rows and t.is_contiguous()


def _row_mask(t, rows: int, name: str):
    if t is not None and not _is_row_bytes(t, rows):
        raise ValueError(f"row_masks: {name} must be a contiguous uint8 CUDA tensor of {rows} rows (1 = zero this row)")
    return t


def _masked_forward(tables, params, spec: _Spec, row_masks):
    """fn_encoder_forward_masked: an evaluation pass nobody differentiates, so no autograd node -- the outputs are plain tensors.
    no_backward is set unconditionally: the entry point refuses 0."""
    ps = _begin_pass(tables, params, spec._replace(no_backward=True))
    e = ps.e
    masks = [_row_mask(t, n, name) for t, n, name in zip(row_masks, (e.N, e.E, e.EF), ("mask_atoms", "mask_bonds", "mask_fbonds"))]
    m = _lib.RowMasks(*(None if t is None else t.data_ptr() for t in masks))
    _lib.check(ps.lib.fn_encoder_forward_masked(C.byref(e), C.byref(m), *ps.out_ptrs, _stream_ptr(ps.dev)), "fn_encoder_forward_masked")
    _end_pass(spec.plan, spec.variant)
    return tuple(ps.outs) + (ps.pooled,)


_KEEP_ATTN_WS = None      # tests: a list that collects (descriptor, workspace) of every read-out pass (the stored probabilities live there)


def _attn_forward(tables, params, spec: _Spec):
    """fn_encoder_forward_attn: an evaluation pass nobody differentiates (no autograd node) that also returns the last layer's four
    by-source attention sums, each [n, heads] for every node of its level."""
    ps = _begin_pass(tables, params, spec._replace(no_backward=not _EVAL_SAVES), stand_in=True)
    e = ps.e
    attn = [torch.empty((n, spec.heads), dtype=torch.float32, device=ps.dev) for n in (e.N, e.F, e.E, e.EF)]      # atoms, frags, bonds, fbonds
    r = _lib.AttnReadout(*(t.data_ptr() for t in attn))
    _lib.check(ps.lib.fn_encoder_forward_attn(C.byref(e), C.byref(r), *ps.out_ptrs, _stream_ptr(ps.dev)), "fn_encoder_forward_attn")
    _end_pass(spec.plan, spec.variant)
    if _KEEP_ATTN_WS is not None:
        _KEEP_ATTN_WS.append((e, ps.ws))
    return tuple(ps.outs) + (ps.pooled,) + tuple(attn)


def _evaluation_only(prefix: str, noun: str, training: bool, any_grad: bool) -> None:
    """The masked and the read-out pass are evaluation passes without a backward."""
    if training:
        raise RuntimeError(f"{prefix}: a {noun} pass is an evaluation pass (the model is in training mode)")
    if any_grad:
        raise RuntimeError(f"{prefix}: the {noun} pass has no backward; run it under torch.no_grad()")


def encoder_forward(layers, plan: GraphPlan, x_atoms, bond_nodes, fbond_nodes, cos_sorted, fattr_sorted, heads: int,
                    drop_p: float, training: bool, rng, variant: int = 0, edge_outputs: bool = True, row_masks=None,
                    attn_readout: bool = False, keep_atoms=None) -> tuple:
    """Runs all ``layers`` (FragNetLayerA modules) + the inter-layer act(dropout(.)); returns the four outputs and, fifth,
    the readout [n_mols, 256] when the fused fragment tail produced it (an empty tensor otherwise).

    ``attn_readout=True``: four more tensors follow -- the last layer's by-source attention sums of the atom, fragment, bond and
    fragment-bond levels (the reference's ``summed_attn_weights_*``), each [n, heads] with a row for EVERY node of its level
    (fn_encoder_forward_attn).  Like a masked pass it is an evaluation pass without a backward: in training mode, or with a gradient
    required anywhere, it raises; it exists for model_version gat2 and not together with row masks.

    ``row_masks``: None, or a triple (atoms [N], bonds [E], fragment bonds [EF]) of uint8 CUDA tensors or None -- 1 = that row of
    the level's output is zero for every reader, in every layer (fn_encoder_forward_masked).  A masked pass is an evaluation pass
    without a backward: in training mode, or with a gradient required anywhere, it raises.

    ``keep_atoms``: None, or a uint8 CUDA tensor [N], 1 = keep -- the input gate of masked-atom pretraining (fn_encoder_forward_keep):
    a row of ``x_atoms`` with 0 reads as zero for every consumer, gated before the input dropout, in the prologue's own pass over
    ``x_atoms``.  Training passes (with a backward) and evaluation passes alike; model_version gat2 only; not together with row
    masks or the attention read-out, and not with a gradient required on the three input tables."""
    params = [p for layer in layers for p in layer_param_list(layer)]
    n_layers = len(layers)
    # the C side takes widths from the batch and pointers from the parameters: a model built for other feature widths would
    # read and write past its layer-0 weights.  Fail the way the reference's nn.Linear does.
    for name, x, k in (("projection_b", bond_nodes, 0), ("projection_a", x_atoms, 2)) + \
            ((("projection_fb", fbond_nodes, 4),) if variant == 0 else ()):
        w = params[k]
        if w.dim() != 2 or x.dim() != 2 or w.shape[1] != x.shape[1] or w.shape[0] != FN_D:
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({x.shape[0]}x{x.shape[-1]} and {w.shape[-1]}x{w.shape[0]}): "
                               f"layer 0 {name} expects {w.shape[-1]} input features, the batch has {x.shape[-1]}")
    if row_masks is not None and len(row_masks) != 3:
        raise ValueError("row_masks: a triple (atoms, bonds, fragment bonds)")
    masked = row_masks is not None and any(t is not None for t in row_masks)
    tables = (x_atoms, bond_nodes, fbond_nodes)
    # (inside Function.forward grad mode is always off: it is read here)
    in_grad = torch.is_grad_enabled() and any(t.requires_grad for t in tables)
    any_grad = in_grad or (torch.is_grad_enabled() and any(p.requires_grad for p in params))
    if keep_atoms is not None:
        if attn_readout or masked:
            raise ValueError("keep_atoms: the input gate does not combine with row masks or the attention read-out")
        if int(variant) != 0:
            raise ValueError("keep_atoms: the input gate exists for model_version gat2 (the reference masks atoms in FragNetPreTrainMasked2 only)")
        if not _is_row_bytes(keep_atoms, x_atoms.shape[0]):
            raise ValueError(f"keep_atoms must be a contiguous uint8 CUDA tensor of {x_atoms.shape[0]} rows (1 = keep, 0 = the row reads as zero)")
        if in_grad:
            raise NotImplementedError("keep_atoms: there are no input gradients of a masked pass (fn_encoder_backward_inputs refuses it)")
    spec = _Spec(plan, cos_sorted, fattr_sorted, n_layers, heads, variant=int(variant), edge_outputs=bool(edge_outputs), keep_atoms=keep_atoms)
    if attn_readout:
        if masked:
            raise ValueError("attn_readout: there is no attention read-out of a masked pass (row_masks)")
        if int(variant) != 0:
            raise ValueError("attn_readout: the attention read-out exists for model_version gat2 (the reference's lite / edge Viz classes cannot run)")
        _evaluation_only("attn_readout", "read-out", training, any_grad)
        return _attn_forward(tables, params, spec)
    if masked:
        _evaluation_only("row_masks", "masked", training, any_grad)
        return _masked_forward(tables, params, spec, row_masks)
    p_eff = float(drop_p) if training else 0.0
    if in_grad:
        # input gradients (fn_encoder_backward_inputs): refused here, before the forward, where the backward could not serve them
        if int(variant) == 2:
            raise NotImplementedError("input gradients: the engine differentiates its inputs for gat2 and gat2_lite, not for gat2_edge")
        if p_eff > 0.0:
            raise NotImplementedError("input gradients: a training pass with dropout (drop_ratio > 0) gates x_atoms with a mask the backward "
                                      "would have to replay from the Philox stream; use eval() or drop_ratio = 0")
    if p_eff > 0.0:
        # reserve the Philox offsets the engine will consume (fn_encoder_rng_blocks): x_atoms + 4 tensors per layer
        N, E = x_atoms.shape[0], bond_nodes.shape[0]
        F, EF = plan.levels["frag"].n, fbond_nodes.shape[0]
        blocks = (N * x_atoms.shape[1] + 3) // 4 + n_layers * sum((n * FN_D + 3) // 4 for n in (N, F, E, EF))
        seed, offset = rng.take(4 * blocks)
        spec = spec._replace(drop_p=p_eff, seed=seed, offset=offset, offset_dev=rng.dev)
    # under torch.no_grad(), or when nothing it reads requires a gradient, no backward pass can follow: an evaluation pass then
    # stores nothing for one (fn_encoder.no_backward)
    return _EncoderFn.apply(*tables, spec._replace(training=bool(training), no_backward=not _EVAL_SAVES and not any_grad), *params)
