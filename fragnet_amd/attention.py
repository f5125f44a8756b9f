"""Attention weights of every molecule of a dataset on the engine: the second interpretability view of the reference's app
(fragnet/vizualize/viz.py ``calc_weights``, ``vizualize_atom_weights``, ``frag_weight_highlight``), which runs its Viz model on a
batch of ONE molecule and reads the last layer's four ``summed_attn_weights_*`` tensors.

Here the molecules are collated into ordinary evaluation batches; each batch is one read-out pass of the engine (a
``viz_model.FragNetFineTuneViz`` in ``eval()`` mode -> fn_encoder_forward_attn) and the four ``[n, H]`` tensors are split back per
molecule by the offsets table of the collated batch.  Attention never crosses molecules, so a molecule's rows do not depend on the
batch it ran in.  Every tensor has a row for every node (viz_model's shape contract: the reference's own tensors are prefixes).
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from .attribution import _as_store, _Result, engine_device, evaluation, offsets_of, store_batches

LEVELS = ("atoms", "bonds", "frags", "fbonds")
LEVEL_SPACE = {"atoms": "atom", "bonds": "edge", "frags": "frag", "fbonds": "fedge"}       # rows of plan.SPACES / CollatedBatch.offsets


def bond_weights(bonds: np.ndarray) -> np.ndarray:
    """viz.py:684-687 on one molecule's ``[2 n_bonds, H]`` rows: ``a1 = w[::2]; a2 = w[1::2]; (a1 + a2 / 2).sum(1)`` -- the
    precedence is the reference's (only the second direction is halved)."""
    bonds = np.asarray(bonds)
    return (bonds[::2] + bonds[1::2] / 2).sum(1)


def split_rows(rows: np.ndarray, offsets) -> List[np.ndarray]:
    """``rows[offsets[i] : offsets[i + 1]]`` per molecule; ``offsets`` are the batch's cumulative counts of the tensor's index space."""
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != rows.shape[0]:
        raise ValueError(f"split_rows: offsets must rise from 0 to the {rows.shape[0]} rows of the tensor")
    return [rows[offsets[i]: offsets[i + 1]] for i in range(offsets.size - 1)]


class AttentionWeights(_Result):
    """Result of ``attention_weights``: ``pred [n_mols, n_classes]`` and, per level in ``LEVELS``, the flat rows ``[total, H]`` with
    the per-molecule offsets ``[n_mols + 1]``.  ``result[i]`` is molecule i as a dict: ``pred [n_classes]``, ``atoms [n_atoms, H]``,
    ``bonds [2 n_bonds, H]``, ``frags [n_frags, H]``, ``fbonds [2 n_cnx, H]``, the head sums the app draws ``atom_weights``
    (viz.py:733), ``frag_weights`` (viz.py:859), and ``bond_weights [n_bonds]`` (viz.py:684-687)."""

    def __init__(self, pred: np.ndarray, rows: Dict[str, np.ndarray], offsets: Dict[str, np.ndarray]):
        self.pred, self.rows, self.offsets = pred, rows, offsets

    def __getitem__(self, i: int) -> dict:
        i = self._index(i)
        out = {"pred": self.pred[i]}
        for k in LEVELS:
            out[k] = self.rows[k][int(self.offsets[k][i]): int(self.offsets[k][i + 1])]
        out["atom_weights"] = out["atoms"].sum(1)
        out["frag_weights"] = out["frags"].sum(1)
        out["bond_weights"] = bond_weights(out["bonds"])
        return out

    def arrays(self) -> Dict[str, np.ndarray]:
        """A flat dict for ``np.savez``: ``pred``, and per level k ``k`` [total, H] and ``k_offsets`` [n_mols + 1]; the drawn sums
        ``atom_weights`` [total atoms], ``frag_weights`` [total fragments] (offsets: the level's) and ``bond_weights`` with
        ``bond_weights_offsets`` (one entry per bond = pair of directed rows)."""
        out = {"pred": self.pred}
        for k in LEVELS:
            out[k] = self.rows[k]
            out[f"{k}_offsets"] = self.offsets[k]
        out["atom_weights"] = self.rows["atoms"].sum(1)
        out["frag_weights"] = self.rows["frags"].sum(1)
        per_mol = [bond_weights(r) for r in split_rows(self.rows["bonds"], self.offsets["bonds"])]
        out["bond_weights"] = np.concatenate(per_mol) if per_mol else np.zeros(0, np.float32)
        out["bond_weights_offsets"] = offsets_of([len(r) for r in per_mol])
        return out


def assemble(preds: List[np.ndarray], tensors: List[Dict[str, np.ndarray]], offsets: List[Dict[str, np.ndarray]]) -> AttentionWeights:
    """Batches -> one result: per batch the predictions ``[B, n_classes]``, the four ``[n, H]`` tensors and, per level, the batch's
    cumulative per-molecule counts ``[B + 1]``.  Rows stay in molecule order, so the flat offsets are the running sums."""
    rows, offs = {}, {}
    for k in LEVELS:
        for t, o in zip(tensors, offsets):
            split_rows(t[k], o[k])            # validates
        rows[k] = np.concatenate([t[k] for t in tensors], 0)
        offs[k] = offsets_of(np.concatenate([np.diff(np.asarray(o[k], dtype=np.int64)) for o in offsets]))
    return AttentionWeights(np.concatenate(preds, 0), rows, offs)


def attention_weights(model, source, batch_size: int = 512) -> AttentionWeights:
    """Attention weights of every molecule of ``source`` (a ``FlatMolStore`` or a list of ``MolRecord``) under ``model``: a
    ``viz_model.FragNetFineTuneViz`` (or ``FragNetPreTrainViz``) on the GPU.  One read-out pass per batch of ``batch_size`` molecules."""
    import torch
    from .plan import SPACES
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    enc = getattr(model, "pretrain", None)
    if enc is None or not getattr(enc.layers[-1], "return_attentions", False):
        raise ValueError("attention_weights: a Viz model (viz_model.FragNetFineTuneViz / FragNetPreTrainViz), whose last layer reads the attentions out")
    store = _as_store(source, engine_device(model, "attention_weights"))
    preds, tensors, offsets = [], [], []
    with evaluation(model), torch.no_grad():
        for b, e, batch in store_batches(store, batch_size):
            out = model(batch)
            if len(out) != 5:
                raise ValueError("attention_weights: the model must return (prediction, attn_atoms, attn_frags, attn_bonds, attn_fbonds)")
            pred, attn = out[0], dict(zip(("atoms", "frags", "bonds", "fbonds"), out[1:]))
            preds.append(pred.reshape(e - b, -1).float())
            tensors.append({k: attn[k].float() for k in LEVELS})
            offsets.append(batch.offsets)
        # (copied to the host once every batch is queued: no synchronisation between the passes)
        preds = [t.cpu().numpy() for t in preds]
        tensors = [{k: v.cpu().numpy() for k, v in t.items()} for t in tensors]
        offsets = [{k: off[SPACES.index(LEVEL_SPACE[k])] for k in LEVELS} for off in (o.cpu().numpy() for o in offsets)]
    return assemble(preds, tensors, offsets)
