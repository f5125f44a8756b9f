"""Attributions for the two pair models, ``cdrp.CDRPModel`` and ``dta.DTAModel2``: which genes of a cell line, which residues of a
protein and which atoms / bonds / fragment connections of the drug a prediction rests on.

Both pair heads are affine -- ``fc2(fc1(cat(a, b)))`` has nothing between the two Linears -- so with ``v = fc1.weight^T fc2.weight``
split at column 256 into ``v_d`` and ``v_s``

    out = <drug_enc, v_d> + <second_enc, v_s> + const,        const = <fc2.weight, fc1.bias> + fc2.bias        (``pair_vectors``)

and each side is explained on its own: the second input's attribution does not depend on the drug and runs no encoder pass.

* ``cell_line_attributions`` -- the CDRP cell-line tower (gene_dim -> 1024 -> 256 -> 64 -> 256, a ReLU after every Linear) is
  non-linear: gradient x input or integrated gradients of ``s(c) = <cell_enc(c), v_s>`` with respect to the genes, on the tower's HIP
  kernels (``ops.cell_path_attributions``: fn_cdrp_gene_fwd_path_f32 forms the path rows in its loads, fn_cdrp_gene_dx_f32 is the input
  gradient folded over the path; neither the path rows nor the per-node gradients exist in memory).
* ``protein_attributions`` -- the DTA protein tower (embedding -> convolution -> Linear, no activation) is linear in the embedded
  tensor, so gradient x input per residue is exact and collapses to a ``[L, V]`` lookup table.
* ``drug_attributions`` -- the drug side is the engine's existing input-gradient path with ``<pooled, v_d>`` as the head.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .attribution import DEFAULT_MAX_ROWS, _Result, row_vector
from .gradient_attribution import GradientAttribution, input_gradients, integrated_gradients, midpoint_alphas
from .model import FragNetFineTune

DRUG_WIDTH = 256          # of the pooled read-out: the pair heads' first 256 input columns
METHODS = ("ig", "grad_x_input")


def pair_vectors(model):
    """``(v_d [256], v_s [second width], const)`` of a pair model's affine head, float32 tensors on the parameters' device and a float:
    ``model(batch) = <drug_enc, v_d> + <second_enc, v_s> + const``.  The products are taken in float64."""
    fc1, fc2 = getattr(model, "fc1", None), getattr(model, "fc2", None)
    if not (isinstance(fc1, torch.nn.Linear) and isinstance(fc2, torch.nn.Linear)) or fc2.out_features != 1 \
            or fc1.out_features != fc2.in_features or fc1.in_features <= DRUG_WIDTH or fc1.bias is None or fc2.bias is None:
        raise ValueError(f"{type(model).__name__}: not a pair model (fc2(fc1(cat(drug_enc, second_enc))) with one output column)")
    with torch.no_grad():
        w2 = fc2.weight.detach().double()
        v = (w2 @ fc1.weight.detach().double()).reshape(-1)
        const = float((w2 @ fc1.bias.detach().double()).reshape(()) + fc2.bias.detach().double().reshape(()))
        return v[:DRUG_WIDTH].float().contiguous(), v[DRUG_WIDTH:].float().contiguous(), const


# ----------------------------------------------------------------------------------------------------------------- the cell-line side
def plan_cell_chunks(n_cells: int, steps: int, max_rows: int) -> List[Tuple[int, int]]:
    """``[first, end)`` ranges of cell lines such that ``cells * steps <= max_rows`` in every chunk (a cell line's path nodes stay
    together: fn_cdrp_gene_dx_f32 folds them in one launch)."""
    if n_cells < 0 or steps < 1 or max_rows < 1:
        raise ValueError("plan_cell_chunks: n_cells >= 0, steps >= 1, max_rows >= 1")
    per = max_rows // steps
    if per < 1:
        raise ValueError(f"plan_cell_chunks: one cell line's {steps} path nodes do not fit max_rows = {max_rows}")
    return [(c, min(n_cells, c + per)) for c in range(0, n_cells, per)]


class CellLineAttribution(_Result):
    """Result of ``cell_line_attributions``: ``attr`` float32 [C, gene_dim], ``score`` [C] (= ``<cell_enc, v_s>``), and for integrated
    gradients ``score_baseline`` [C] and ``gap = score - score_baseline - sum_k attr`` [C] (None for gradient x input).  ``result[c]``
    is cell line c as a dict; ``arrays()`` is what the command-line script writes."""
    _per_item = "attr"

    def __init__(self, method: str, attr, score, score_baseline=None, gap=None, steps: Optional[int] = None):
        self.method, self.attr, self.score, self.score_baseline, self.gap, self.steps = method, attr, score, score_baseline, gap, steps

    def __getitem__(self, c: int) -> dict:
        c = self._index(c)
        out = {"attr": self.attr[c], "score": self.score[c]}
        if self.score_baseline is not None:
            out["score_baseline"], out["gap"] = self.score_baseline[c], self.gap[c]
        return out

    def arrays(self) -> Dict[str, np.ndarray]:
        out = {"method": np.array(self.method), "side": np.array("cell_line"), "attr": self.attr, "score": self.score}
        if self.steps is not None:
            out["steps"] = np.array(self.steps)
        if self.score_baseline is not None:
            out["score_baseline"], out["gap"] = self.score_baseline, self.gap
        return out


def _gene_baseline(baseline, width: int, device):
    return None if baseline is None else row_vector(baseline, width, device, "baseline", "genes")


def cell_line_attributions(model, gene_expr, method: str = "ig", steps: int = 32, baseline=None,
                           max_rows: int = ops.DENSE_MAX_ROWS) -> CellLineAttribution:
    """Attributions of ``s(c) = <cell_enc(c), v_s>`` -- the cell line's whole share of a ``CDRPModel`` prediction -- to the genes of
    ``gene_expr`` (int64 [C, gene_dim], one row per distinct cell line; a tensor or an array).

    ``method="grad_x_input"``: ``attr = gene * d s / d gene``, one forward and backward of the tower.  ``method="ig"``: integrated
    gradients along the straight path from ``baseline`` (None: zeros; or a row vector [gene_dim]) to the cell line, midpoint rule with
    ``steps`` nodes (``gradient_attribution.midpoint_alphas``), a cell line's nodes added in ascending order.  Cell lines are chunked so
    that ``cells * steps <= max_rows`` (default and upper limit ``ops.DENSE_MAX_ROWS``).  Everything runs on the tower's HIP kernels; a
    tower whose widths they do not take raises ValueError -- there is no other path."""
    # (drug_attributions' two refusals of ``method`` / ``baseline``: each driver has refusals of its own between them, so they stay apart)
    if method not in METHODS:
        raise ValueError(f"method: one of {METHODS} (got {method!r})")
    tower = getattr(getattr(model, "cell_model", None), "predictor", None)
    if tower is None:
        raise ValueError(f"cell_line_attributions: {type(model).__name__} has no cell-line tower (a cdrp.CDRPModel is wanted)")
    linears = list(tower)
    device = linears[0].weight.device
    max_rows = int(max_rows)
    if not 1 <= max_rows <= ops.DENSE_MAX_ROWS:
        raise ValueError(f"max_rows: 1 .. {ops.DENSE_MAX_ROWS} (the tower's kernels reduce over all rows of a call)")
    gene = gene_expr if torch.is_tensor(gene_expr) else torch.as_tensor(np.asarray(gene_expr))
    if gene.dtype != torch.int64 or gene.dim() != 2 or gene.shape[1] != linears[0].in_features:
        raise ValueError(f"gene_expr: int64 [cell lines, {linears[0].in_features}] (got {gene.dtype} {tuple(gene.shape)})")
    if method == "grad_x_input":
        if baseline is not None:
            raise ValueError("baseline: gradient x input has none (method='ig' takes one)")
        alphas, n_steps = np.ones(1, dtype=np.float32), None
    else:
        alphas = midpoint_alphas(steps)
        n_steps = int(steps)
    chunks = plan_cell_chunks(gene.shape[0], alphas.shape[0], max_rows)
    _, v_s, _ = pair_vectors(model)
    if v_s.shape[0] != linears[-1].out_features:
        raise ValueError(f"cell_line_attributions: fc1 takes {v_s.shape[0]} columns behind the drug's, the tower gives {linears[-1].out_features}")
    if not ops.cell_tower_ok(gene, max_rows, linears):
        raise ValueError("cell_line_attributions: the tower's kernels take Linears with a bias whose widths behind gene_dim are multiples of "
                         "4; this tower has no kernel path, and there is no other")
    base = _gene_baseline(baseline, gene.shape[1], "cpu" if device.type != "cuda" else device)
    if device.type != "cuda":          # (attribution.engine_device's refusal, for the tower's device and in this driver's words)
        raise _lib.FragnetHipError("cell_line_attributions runs on the GPU kernels; there is no CPU fallback")
    gene = gene.to(device).contiguous()
    alpha_d, one = torch.from_numpy(alphas).to(device), torch.ones(1, dtype=torch.float32, device=device)
    attrs, scores = [], []
    with torch.no_grad():
        for c0, c1 in chunks:
            g = gene[c0:c1]
            attrs.append(ops.cell_path_attributions(g, linears, v_s, alpha_d, base)[0])
            scores.append(ops.cell_path_scores(g, linears, v_s, one).reshape(-1))
        C = gene.shape[0]
        attr = torch.cat(attrs).cpu().numpy() if attrs else np.zeros((0, gene.shape[1]), dtype=np.float32)
        score = torch.cat(scores).cpu().numpy() if scores else np.zeros(0, dtype=np.float32)
        if method == "grad_x_input":
            return CellLineAttribution(method, attr, score)
        # the path's start is the same point for every cell line: one row, alpha = 0
        s0 = ops.cell_path_scores(torch.zeros((1, gene.shape[1]), dtype=torch.int64, device=device), linears, v_s, torch.zeros_like(one), base)
        score0 = np.full(C, float(s0.reshape(-1)[0]), dtype=np.float32)
    gap = (score.astype(np.float64) - score0.astype(np.float64) - attr.astype(np.float64).sum(1)).astype(np.float32)
    return CellLineAttribution(method, attr, score, score0, gap, n_steps)


# ----------------------------------------------------------------------------------------------------------------- the protein side
class ProteinAttribution(_Result):
    """Result of ``protein_attributions``: ``attr`` float32 [P, L] per residue position, ``attr_other`` [P] (the bias terms), ``score``
    [P] (= ``<xt, v_s>`` from the tower's own forward) and ``table`` [L, V], the lookup ``attr[p, c] = table[c, tokens[p, c]]``."""

    _per_item = "attr"

    def __init__(self, attr, attr_other, score, table):
        self.method, self.attr, self.attr_other, self.score, self.table = "grad_x_input", attr, attr_other, score, table

    def __getitem__(self, p: int) -> dict:
        p = self._index(p)
        return {"attr": self.attr[p], "attr_other": self.attr_other[p], "score": self.score[p]}

    def arrays(self) -> Dict[str, np.ndarray]:
        return {"method": np.array(self.method), "side": np.array("protein"), "attr": self.attr, "attr_other": self.attr_other, "score": self.score,
                "table": self.table}


def protein_table(model, v_s):
    """``(T [L, V], other)`` of a ``DTAModel2``: ``<xt, v_s> = sum_c T[c, token_c] + other`` for tokens inside ``[0, V)``.  With
    ``g = reshape(fc1_xt.weight^T v_s, [F, J])``:  ``Gm[v, f, k] = sum_j g[f, j] E[v, j + k]``,  ``T[c, v] = sum_{f, k} Wconv[f, c, k]
    Gm[v, f, k]``,  ``other = sum_f bconv[f] sum_j g[f, j] + <fc1_xt.bias, v_s>``.  In the parameters' dtype, on their device."""
    E, conv, fc = model.embedding_xt.weight.detach(), model.conv_xt_1, model.fc1_xt
    Wc = conv.weight.detach()
    (V, D), (F_, L, KS) = E.shape, Wc.shape
    J = D - KS + 1
    if fc.in_features != F_ * J or conv.bias is None or fc.bias is None or tuple(conv.stride) != (1,) or tuple(conv.dilation) != (1,) \
            or conv.groups != 1 or conv.padding not in ((0,), "valid"):
        raise ValueError("protein_table: embedding -> plain Conv1d over the embedding axis -> Linear is wanted (DTAModel2's protein tower)")
    v_s = v_s.to(E.dtype)
    g = (fc.weight.detach().t() @ v_s).reshape(F_, J)
    Gm = torch.einsum("fj,vkj->vfk", g, E.unfold(1, J, 1))                  # E.unfold: [V, KS, J], window k = E[v, k : k + J]
    T = torch.einsum("fck,vfk->cv", Wc, Gm)
    other = (conv.bias.detach() * g.sum(1)).sum() + (fc.bias.detach() * v_s).sum()
    return T, other


def _protein_xt(model, tokens):
    """fc1_xt's output for ``tokens``: the model's own tower on the GPU, the same layers in torch elsewhere (a token outside [0, V) embeds
    as zeros, as the tower's histogram kernel counts it)."""
    if tokens.is_cuda:
        return ops.protein_tower(tokens, model.embedding_xt, model.conv_xt_1, model.fc1_xt)
    E = model.embedding_xt.weight
    inside = (tokens >= 0) & (tokens < E.shape[0])
    emb = E[tokens.clamp(0, E.shape[0] - 1)] * inside.unsqueeze(-1).to(E.dtype)
    return model.fc1_xt(torch.nn.functional.conv1d(emb, model.conv_xt_1.weight, model.conv_xt_1.bias).flatten(1))


def protein_attributions(model, tokens) -> ProteinAttribution:
    """Per-residue attributions of ``<xt, v_s>`` -- the protein's whole share of a ``DTAModel2`` prediction -- for ``tokens`` (int64
    [P, L]).  The tower is linear in the embedded tensor, so gradient x input on it, summed over a position's embedding row, is EXACT
    (no path, no quadrature) and equals one entry of ``protein_table``: ``attr[p, c] = T[c, tokens[p, c]]``, 0 for a token outside
    ``[0, V)``; ``attr_other`` is the bias terms, so that ``score = sum_c attr + attr_other``.  These are a few small matrix products
    on constants of the model and one gather, written in plain torch ops on the model's device: no kernel is wanted here."""
    if not all(hasattr(model, k) for k in ("embedding_xt", "conv_xt_1", "fc1_xt")):
        raise ValueError(f"protein_attributions: {type(model).__name__} has no protein tower (a dta.DTAModel2 is wanted)")
    device = model.embedding_xt.weight.device
    tok = tokens if torch.is_tensor(tokens) else torch.as_tensor(np.asarray(tokens))
    L = model.conv_xt_1.weight.shape[1]
    if tok.dtype != torch.int64 or tok.dim() != 2 or tok.shape[1] != L:
        raise ValueError(f"tokens: int64 [proteins, {L}] (got {tok.dtype} {tuple(tok.shape)})")
    tok = tok.to(device).contiguous()
    _, v_s, _ = pair_vectors(model)
    with torch.no_grad():
        T, other = protein_table(model, v_s)
        V = T.shape[1]
        inside = (tok >= 0) & (tok < V)
        attr = T.unsqueeze(0).expand(tok.shape[0], -1, -1).gather(2, tok.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1) * inside.to(T.dtype)
        score = _protein_xt(model, tok) @ v_s.to(T.dtype) if tok.shape[0] else torch.zeros(0, dtype=T.dtype, device=device)
    f32 = lambda t: t.float().cpu().numpy()
    return ProteinAttribution(f32(attr), np.full(tok.shape[0], float(other), dtype=np.float32), f32(score), f32(T))


# ----------------------------------------------------------------------------------------------------------------- the drug side
class LinearScoreHead(nn.Module):
    """``enc -> <enc, v>`` [B, 1] as a prediction head: one Linear(len(v), 1) with a zero bias, on the head kernels (``ops.mlp_head``).
    The owning model sets ``rng`` and ``live_rows`` as on every head."""
    rng, live_rows = None, None

    def __init__(self, v):
        super().__init__()
        self.lin = nn.Linear(v.numel(), 1).to(v.device)
        self.lin.weight.data.copy_(v.detach().reshape(1, -1))
        self.lin.bias.data.zero_()
        self.lin.requires_grad_(False)

    def forward(self, enc):
        return ops.mlp_head(enc, [self.lin], 0.0, False, self.rng, self.live_rows)


class DrugScorer(FragNetFineTune):
    """A pair model's drug encoder under the head ``<pooled, v_d>``, as the ``FragNetFineTune`` the engine's input-gradient functions
    take (``gradient_attribution._check_model`` goes on refusing the pair models themselves): the SAME ``pretrain`` module, no copy,
    in the mode the pair model's encoder is in."""

    def __init__(self, drug_model, v_d):
        nn.Module.__init__(self)
        self.pretrain = drug_model.pretrain
        self.fthead = LinearScoreHead(v_d)
        self.fthead.rng = self.pretrain.rng
        self.train(drug_model.training)


def drug_attributions(model, records, method: str = "ig", steps: int = 32, baseline=None, target: int = 0, max_rows: int = DEFAULT_MAX_ROWS,
                      batch_size: int = 512) -> GradientAttribution:
    """Atom, bond and fragment-connection attributions of the drug's share ``<drug_enc, v_d>`` of a pair model's prediction
    (``cdrp.CDRPModel`` or ``dta.DTAModel2``).  ``records``: the pair records (their molecule part is read) or a ``FlatMolStore``.
    Runs ``model.drug_model``'s encoder on the engine under the head ``<pooled, v_d>`` through ``gradient_attribution.input_gradients``
    (``method="grad_x_input"``) or ``integrated_gradients`` (``method="ig"``, with ``steps``, ``baseline`` and ``max_rows`` as there).

    The result's ``pred`` (and ``pred_baseline``) is the scalar ``<drug_enc, v_d>``, NOT the model's prediction: the second input's share
    and the constant of ``pair_vectors`` are not in it.  The head has one column: ``target`` must be 0."""
    if method not in METHODS:          # (cell_line_attributions' two refusals, in its words: see the note there)
        raise ValueError(f"method: one of {METHODS} (got {method!r})")
    drug = getattr(model, "drug_model", None)
    if drug is None or not hasattr(drug, "pretrain"):
        raise ValueError(f"drug_attributions: {type(model).__name__} has no drug encoder (a cdrp.CDRPModel or dta.DTAModel2 is wanted)")
    v_d, _, _ = pair_vectors(model)
    scorer = DrugScorer(drug, v_d)
    if method == "grad_x_input":
        if baseline is not None:
            raise ValueError("baseline: gradient x input has none (method='ig' takes one)")
        return input_gradients(scorer, records, target=target, batch_size=batch_size)
    return integrated_gradients(scorer, records, steps=steps, baseline=baseline, target=target, max_rows=max_rows, batch_size=batch_size)
