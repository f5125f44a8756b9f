"""Gradient attributions on the engine: gradient x input and integrated gradients (Sundararajan et al., ICML 2017) with respect to the
three node-feature tables of a batch -- ``x_atoms``, ``node_features_bonds``, ``node_features_fbonds`` -- the companions of the
leave-one-out masking attributions of ``fragnet_amd.attribution``.

One backward pass scores every atom, bond and fragment connection of a batch: the engine's backward leaves dL/d(layer 0's projection
outputs) behind, and one more launch (fn_encoder_backward_inputs) multiplies them by the three layer-0 weights and, in the same
launch, by the caller's ``delta`` rows -- the per-row score ``<gradient, delta>`` without the gradient tables in memory.

Entries line up with leave-one-out's (``attribution.replica_table``): atoms ``0 .. n-1``; bonds by their first directed row ``0, 2,
...`` -- a bond's score is the sum of its directed rows 2k and 2k + 1; fragment connections ``k = 0 .. EF/2 - 1`` over rows 2k and
2k + 1.  Rows that belong to no entry -- the single placeholder fragment-bond row of a one-fragment molecule -- are reported per molecule
as ``attr_other``, so that integrated gradients' completeness identity can be checked: ``pred - pred_baseline = sum(attr) + attr_other
+ gap``.

In scope: ``FragNetFineTune`` with model_version gat2 and gat2_lite, one ``target`` column per call.  The two edge-attribute tables
(``edge_attr_bonds``, ``edge_attr_fbonds``) are inputs of the path too, but are not differentiated: integrated gradients holds them at
their values on both ends of the path.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .attribution import (DEFAULT_MAX_ROWS, KIND_ORDER, _as_store, _KindTables, chunk_replicas, engine_device, evaluation, offsets_of,
                          plan_chunks, row_vector, store_batches)

TABLE_KEYS = ("x_atoms", "node_features_bonds", "node_features_fbonds")      # the differentiated inputs, in KIND_ORDER
TABLE_SPACES = ("atom", "edge", "fedge")
STORE_KEYS = ("x_atoms", "node_features_bonds", "node_feautures_fbondg")      # the same tables under a FlatMolStore's (the reference Data item's) names


def midpoint_alphas(steps: int) -> np.ndarray:
    """The midpoint rule's nodes ``(j + 1/2) / steps``, j = 0 .. steps - 1, as float32."""
    if int(steps) != steps or steps < 1:
        raise ValueError("steps must be a positive integer")
    return ((np.arange(int(steps), dtype=np.float64) + 0.5) / int(steps)).astype(np.float32)


def entry_rows(n_bonds_directed, n_fbonds_directed):
    """How rows map to entries.  From the per-molecule directed-row counts: ``(bond_first, bond_index, bond_count, fbond_first,
    fbond_index, fbond_count, fbond_other)`` -- ``*_first``: int64 flat row (over all molecules) of each entry's first directed row, the
    entry's score being rows ``first`` and ``first + 1``; ``*_index``: the entry's index column as ``replica_table`` writes it (bonds: the
    directed row within the molecule, 0, 2, ...; fragment connections: k); ``*_count``: entries per molecule; ``fbond_other``: the flat
    fragment-bond rows that belong to no entry (row 2 (nf // 2) of a molecule with an odd count: the placeholder row)."""
    nb = np.asarray(n_bonds_directed, dtype=np.int64).reshape(-1)
    nf = np.asarray(n_fbonds_directed, dtype=np.int64).reshape(-1)
    if nb.shape != nf.shape or (nb < 0).any() or (nf < 0).any() or (nb % 2).any() or ((nf % 2 == 1) & (nf != 1)).any():
        raise ValueError("entry_rows: one non-negative count per molecule, directed-row counts even (one placeholder fragment-bond row aside)")

    def pairs(counts):
        off = offsets_of(counts)[:-1]
        per = counts // 2
        mol = np.repeat(np.arange(counts.shape[0]), per)
        k = np.arange(int(per.sum())) - np.repeat(offsets_of(per)[:-1], per)
        return off[mol] + 2 * k, k, per, off

    b_first, b_k, b_per, _ = pairs(nb)
    f_first, f_k, f_per, f_off = pairs(nf)
    odd = np.flatnonzero(nf % 2 == 1)
    return (b_first, (2 * b_k).astype(np.int32), b_per, f_first, f_k.astype(np.int32), f_per, f_off[odd] + 2 * f_per[odd])


class GradientAttribution(_KindTables):
    """Result of ``input_gradients`` / ``integrated_gradients``: flat arrays plus per-molecule offsets.  ``result[i]`` is molecule i as
    ``{"pred": float, kind: {"index": [count], "attr": [count]}, "attr_other": float, ...}`` (integrated gradients adds
    ``pred_baseline`` and ``gap``); ``arrays()`` is what the command-line script writes.  ``gradients``: None, or the raw gradient
    tables ``(atoms [N, Ka], bond nodes [E, Kb], fragment-bond nodes [EF, Kf] or None)`` of all molecules, rows molecule-major."""

    def __init__(self, method: str, pred, tables: Dict[str, Dict[str, np.ndarray]], attr_other, pred_baseline=None, gap=None,
                 gradients=None, steps: Optional[int] = None, target: int = 0):
        self.method, self.pred, self.tables, self.attr_other = method, pred, tables, attr_other
        self.pred_baseline, self.gap, self.gradients, self.steps, self.target = pred_baseline, gap, gradients, steps, target
        self.kinds = KIND_ORDER

    def __getitem__(self, i: int) -> dict:
        i = self._index(i)
        out = {"pred": self.pred[i], "attr_other": self.attr_other[i]}
        if self.pred_baseline is not None:
            out["pred_baseline"], out["gap"] = self.pred_baseline[i], self.gap[i]
        return {**out, **self._kind_rows(i)}

    def arrays(self) -> Dict[str, np.ndarray]:
        out = {"method": np.array(self.method), "target": np.array(self.target), "pred": self.pred, "attr_other": self.attr_other,
               "kinds": np.array(self.kinds)}
        if self.steps is not None:
            out["steps"] = np.array(self.steps)
        if self.pred_baseline is not None:
            out["pred_baseline"], out["gap"] = self.pred_baseline, self.gap
        out.update(self._kind_arrays())
        if self.gradients is not None:
            for key, g in zip(TABLE_KEYS, self.gradients):
                if g is not None:
                    out[f"grad_{key}"] = g
        return out


def assemble(lens, row_scores: Sequence[np.ndarray]) -> Tuple[Dict[str, Dict[str, np.ndarray]], np.ndarray]:
    """Per-row scores (atoms [N], directed bonds [E], directed fragment bonds [EF], molecule-major, float32) to the three entry tables
    and ``attr_other`` [n]: pair sums ``row 2k + row 2k + 1`` in float32, rows outside every entry summed per molecule."""
    na, nb, nf = (np.asarray(lens[s], dtype=np.int64) for s in TABLE_SPACES)
    n = na.shape[0]
    a, b, f = (np.asarray(r, dtype=np.float32).reshape(-1) for r in row_scores)
    if a.shape[0] != na.sum() or b.shape[0] != nb.sum() or f.shape[0] != nf.sum():
        raise ValueError("assemble: row scores do not match the molecules' row counts")
    b_first, b_index, b_per, f_first, f_index, f_per, f_other = entry_rows(nb, nf)
    k_atom = np.arange(int(na.sum())) - np.repeat(offsets_of(na)[:-1], na)
    tables = {"atom": {"offsets": offsets_of(na), "index": k_atom.astype(np.int32), "attr": a},
              "bond": {"offsets": offsets_of(b_per), "index": b_index, "attr": b[b_first] + b[b_first + 1]},
              "fbond": {"offsets": offsets_of(f_per), "index": f_index, "attr": f[f_first] + f[f_first + 1]}}
    other = np.zeros(n, dtype=np.float32)
    f_mol = np.repeat(np.arange(n), nf)
    np.add.at(other, f_mol[f_other], f[f_other])
    return tables, other


def completeness_gap(pred, pred_baseline, tables, attr_other) -> np.ndarray:
    """``pred - pred_baseline - sum(attr) - attr_other`` per molecule (float64 sums, float32 result)."""
    n = np.asarray(pred).shape[0]
    total = np.asarray(attr_other, dtype=np.float64).copy()
    for k in KIND_ORDER:
        t = tables[k]
        total += np.bincount(np.repeat(np.arange(n), np.diff(t["offsets"])), weights=t["attr"].astype(np.float64), minlength=n)
    return (np.asarray(pred, dtype=np.float64) - np.asarray(pred_baseline, dtype=np.float64) - total).astype(np.float32)


def _check_model(model, what: str):
    from .model import FragNetFineTune
    if not isinstance(model, FragNetFineTune):
        raise ValueError(f"{what}: {type(model).__name__} is not a FragNetFineTune (CDRP, DTA and gcn2 models are out of scope)")
    variant = getattr(model.pretrain, "variant", None)
    if variant not in ("gat2", "gat2_lite"):
        raise NotImplementedError(f"{what}: the engine differentiates its inputs for model_version gat2 and gat2_lite (got {variant!r})")
    device = engine_device(model, what)
    if not model.pretrain.use_engine:
        raise ValueError(f"{what}: the fused row dots come from the engine (use_engine=False has no such output)")
    return device, variant


def _column(out, rows: int, target: int):
    out = out.reshape(rows, -1)
    if not 0 <= target < out.shape[1]:
        raise IndexError(f"target {target}: the model has {out.shape[1]} output column(s)")
    return out[:, target]


def _backward_dots(model, batch, leaves, deltas, target: int, keep_dx: bool):
    """One evaluation forward and backward of ``batch`` with ``leaves`` as its three tables: (logit column [B], row dots, gradients)."""
    import torch
    from . import engine
    for key, t in zip(TABLE_KEYS, leaves):
        batch[key] = t.requires_grad_(True)
    rows = int(batch.offsets.shape[1]) - 1
    with torch.enable_grad():
        engine.arm_input_dots(deltas, keep_dx=keep_dx)
        try:
            col = _column(model(batch), rows, target)
            grads = torch.autograd.grad(col.sum(), [batch[k] for k in TABLE_KEYS], allow_unused=True)      # ones on the target column
        finally:
            dots = engine.take_input_dots()
    if dots is None:
        raise RuntimeError("the backward pass did not run the engine's input-gradient call")
    return col.detach().float(), dots, grads


def input_gradients(model, source, target: int = 0, batch_size: int = 512, return_gradients: bool = False) -> GradientAttribution:
    """Gradient x input of logit column ``target`` for every molecule of ``source`` (a ``FlatMolStore`` or a list of ``MolRecord``): one
    evaluation forward and one backward per batch of ``batch_size`` molecules, the backward seeded with ones on that column.  The scores
    are the fused row dots ``<dL/dx row, x row>``; ``return_gradients=True`` also returns the three raw gradient tables."""
    import torch
    device, variant = _check_model(model, "input_gradients")
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    store = _as_store(source, device)
    lens = store._host_lengths()
    preds, rows, grads = [], ([], [], []), ([], [], [])
    with evaluation(model):
        for _, _, batch in store_batches(store, batch_size):
            xs = [batch[k].detach().float().contiguous() for k in TABLE_KEYS]
            leaves = [x.clone() for x in xs]
            col, dots, g = _backward_dots(model, batch, leaves, xs if variant == "gat2" else (xs[0], xs[1], None), target, return_gradients)
            preds.append(col)
            for k in range(3):
                rows[k].append(dots[k] if dots[k] is not None else torch.zeros(xs[k].shape[0], dtype=torch.float32, device=device))
                grads[k].append(g[k])
        pred = torch.cat(preds).cpu().numpy()
        row_h = [torch.cat(r).cpu().numpy() for r in rows]
        grad_h = None
        if return_gradients:
            grad_h = tuple(None if any(t is None for t in g) else torch.cat(g, 0).cpu().numpy() for g in grads)
    tables, other = assemble(lens, row_h)
    return GradientAttribution("grad_x_input", pred, tables, other, gradients=grad_h, target=target)


def check_baseline(baseline, widths: Sequence[int], device):
    """``baseline`` of ``integrated_gradients`` as three float32 row vectors on ``device``: None (zeros), or a triple of 1-d arrays /
    tensors ``[Ka]``, ``[Kb]``, ``[Kf]``; a tensor must live on the CPU or on ``device``."""
    import torch
    if baseline is None:
        return [torch.zeros(w, dtype=torch.float32, device=device) for w in widths]
    if not isinstance(baseline, (tuple, list)) or len(baseline) != 3:
        raise ValueError("baseline: None (zeros) or three row vectors (atoms [Ka], bond nodes [Kb], fragment-bond nodes [Kf])")
    out = []
    for v, w, key in zip(baseline, widths, TABLE_KEYS):
        if torch.is_tensor(v) and v.device.type != "cpu" and v.device != torch.device(device):
            raise ValueError(f"baseline of {key}: a tensor on {v.device}, the model is on {device}")
        out.append(row_vector(v, w, device, f"baseline of {key}", "features"))
    return out


def ig_plan(lens, steps: int, max_rows: int):
    """The replica plan of integrated gradients: every (molecule, step) pair is one replica costing the molecule's atom + directed-bond
    rows, chunked molecule-major by ``attribution.plan_chunks`` (a molecule's steps may span chunks)."""
    n = np.asarray(lens["atom"]).shape[0]
    return plan_chunks(np.asarray(lens["atom"]) + np.asarray(lens["edge"]), np.full(n, int(steps), dtype=np.int64), max_rows)


def integrated_gradients(model, source, steps: int = 32, baseline=None, target: int = 0, max_rows: int = DEFAULT_MAX_ROWS,
                         batch_size: int = 512) -> GradientAttribution:
    """Integrated gradients of logit column ``target`` along the straight path from ``baseline`` (None: zeros; or three row vectors
    broadcast over the rows) to the molecule's three node tables, midpoint rule with ``steps`` nodes.  Every (molecule, step) pair is a
    molecule of an ordinary evaluation batch (collated with repeated indices, chunks of at most ``max_rows`` atom + directed-bond
    rows) whose tables are ``x0 + alpha_j (x - x0)``; its backward's fused row dots with ``delta = x - x0`` are the step's scores.  The
    steps of a row are added in ascending j and divided by ``steps``."""
    import torch
    device, variant = _check_model(model, "integrated_gradients")
    alphas = midpoint_alphas(steps)
    steps = int(steps)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    store = _as_store(source, device)
    lens = store._host_lengths()
    widths = [int(store.t[k].shape[1]) for k in STORE_KEYS]
    base = check_baseline(baseline, widths, device)
    chunks = ig_plan(lens, steps, max_rows)
    counts = [np.asarray(lens[s], dtype=np.int64) for s in TABLE_SPACES]
    offs = [offsets_of(c) for c in counts]
    totals = [int(o[-1]) for o in offs]
    live = (True, True, variant == "gat2")
    with evaluation(model):
        with torch.no_grad():
            pred, pred0 = [], []
            for b, e, batch in store_batches(store, batch_size):
                pred.append(_column(model(batch), e - b, target).float())
                batch = store.collate(np.arange(b, e))
                for key, x0 in zip(TABLE_KEYS, base):
                    batch[key] = x0.expand(batch[key].shape[0], -1).contiguous()
                pred0.append(_column(model(batch), e - b, target).float())
            pred, pred0 = torch.cat(pred).cpu().numpy(), torch.cat(pred0).cpu().numpy()
        # every step's row scores, [steps, rows of all molecules] per table, then the sum over the steps in ascending j
        per_step = [torch.zeros((steps, t), dtype=torch.float32, device=device) for t in totals]
        alpha_d = torch.from_numpy(alphas).to(device)
        for chunk in chunks:
            mols, step = chunk_replicas(chunk)          # a replica's number is its step
            batch = store.collate(mols)
            step_d = torch.from_numpy(step).to(device)
            leaves, deltas, slots = [], [], []
            for k, key in enumerate(TABLE_KEYS):
                x = batch[key].detach().float()
                c = counts[k][mols]
                row_rep = torch.repeat_interleave(torch.arange(len(mols), device=device), torch.from_numpy(c).to(device), output_size=int(c.sum()))
                if row_rep.shape[0] != x.shape[0]:
                    raise RuntimeError(f"integrated_gradients: {key} has {x.shape[0]} rows, the store's lengths give {row_rep.shape[0]}")
                delta = (x - base[k]).contiguous()
                leaves.append(torch.addcmul(base[k].expand_as(x), alpha_d[step_d[row_rep]].unsqueeze(1), delta).contiguous())
                deltas.append(delta if live[k] else None)
                # destination of the replica's rows in per_step[k]: row (step, first row of the molecule + row within the molecule)
                dest = np.repeat(step * totals[k] + offs[k][mols] - offsets_of(c)[:-1], c) + np.arange(int(c.sum()))
                slots.append(torch.from_numpy(dest).to(device))
            _, dots, _ = _backward_dots(model, batch, leaves, deltas, target, False)
            for k in range(3):
                if dots[k] is not None:
                    per_step[k].view(-1)[slots[k]] = dots[k]
        row_h = []
        for t in per_step:
            acc = t[0].clone()
            for j in range(1, steps):
                acc += t[j]
            row_h.append((acc / steps).cpu().numpy())
    tables, other = assemble(lens, row_h)
    gap = completeness_gap(pred, pred0, tables, other)
    return GradientAttribution("ig", pred, tables, other, pred_baseline=pred0, gap=gap, steps=steps, target=target)
