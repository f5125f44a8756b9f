"""Nearest neighbours in the space the encoder learned: the example-based view next to the attribution drivers, and the
applicability-domain distance of a screened molecule.

Two levels.  ``"mol"``: the pooled read-out cat(sum of atoms, sum of fragments) [B, 256], exactly what ``model.pooled`` hands to the
head.  ``"frag"``: the encoder's final ``x_frags`` rows, 128 wide, one per fragment -- FragNet's fragments are first-class rows.

``embed`` runs the engine's no-backward pass batch by batch and yields the rows; ``nearest`` embeds the queries once, then makes one
encoder pass per library batch, each followed by one ``ops.TopK.update`` (csrc/topk.hip: similarity tile and top-k selection in one
kernel).  Neither the library's embeddings nor any [queries, library] score matrix is ever held.  The lists do not depend on how the
library is cut into batches as far as the kernel goes; the encoder's own rows may differ in the last bit with batch composition.
"""
from __future__ import annotations

from typing import Dict, NamedTuple

import numpy as np

from .attribution import _as_store, _Result, engine_device, evaluation, offsets_of, store_batches

LEVELS = ("mol", "frag")
LEVEL_WIDTH = {"mol": 256, "frag": 128}


class EmbeddedBatch(NamedTuple):
    first: int              # molecules first .. end of the source
    end: int
    rows: "object"          # device tensor [end - first, 256] ("mol") or [fragments of the batch, 128] ("frag")
    offsets: np.ndarray     # int64 [end - first + 1]: rows offsets[i] : offsets[i + 1] are molecule first + i's (host side)


def _level(level) -> str:
    if level not in LEVELS:
        raise ValueError(f"unknown level {level!r}: one of {', '.join(LEVELS)}")
    return level


def _batch_size(batch_size) -> int:
    if not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError("batch_size must be positive")
    return batch_size


def _encoder(model, who: str):
    """(encoder, "gat" | "gcn") of a finetune or pretrain model of the gat2 family or gcn2; pair models are refused by name."""
    from . import gcn
    from .model import FragNet
    if hasattr(model, "drug_model"):
        raise ValueError(f"{who}: {type(model).__name__} is a pair model (CDRP / DTA): embeddings of pair models are out of scope; "
                         "hand in its drug encoder's finetune or pretrain model instead")
    enc = getattr(model, "pretrain", None)
    if isinstance(enc, FragNet):
        return enc, "gat"
    if isinstance(enc, gcn.FragNet):
        return enc, "gcn"
    raise ValueError(f"{who}: {type(model).__name__} has no `.pretrain` encoder of the gat2 family (gat2, gat2_lite, gat2_edge) or gcn2")


def _rows(enc, family: str, batch, level: str):
    from . import ops
    from .model import pooled
    from .plan import gcn_plan_for
    if family == "gcn":
        x_atoms, x_frags = enc(batch)
        return x_frags if level == "frag" else ops.pool_cat(x_atoms, x_frags, gcn_plan_for(batch))
    x_atoms, x_frags = enc(batch, edge_outputs=False)[:2]
    return x_frags if level == "frag" else pooled(x_atoms, x_frags, batch)


def row_offsets(store, level: str) -> np.ndarray:
    """int64 [n_mols + 1]: first embedding row of every molecule of the store -- the molecule itself for ``"mol"``, its first fragment
    for ``"frag"`` (from the store's host-side lengths: no synchronisation)."""
    if _level(level) == "mol":
        return np.arange(len(store) + 1, dtype=np.int64)
    return offsets_of(store._host_lengths()["frag"])


def _embed_store(model, store, level: str, batch_size: int, who: str):
    import torch
    enc, family = _encoder(model, who)
    offsets = row_offsets(store, level)
    for b, e, batch in store_batches(store, batch_size):
        with evaluation(model), torch.no_grad():          # no_grad: the engine takes its no-backward pass
            rows = _rows(enc, family, batch, level)
        local = offsets[b: e + 1] - offsets[b]
        if rows.shape != (int(local[-1]), LEVEL_WIDTH[level]):
            raise ValueError(f"{who}: the encoder returned {tuple(rows.shape)} rows for molecules {b}..{e}, expected "
                             f"({int(local[-1])}, {LEVEL_WIDTH[level]})")
        yield EmbeddedBatch(b, e, rows, local)


def embed(model, source, level: str, batch_size: int = 512):
    """Yields an ``EmbeddedBatch`` per batch of ``batch_size`` consecutive molecules of ``source`` (a ``FlatMolStore`` or a list of
    ``MolRecord``): the ``level`` rows of ``model``'s encoder in evaluation mode.  ``model``: any finetune or pretrain model whose
    ``.pretrain`` is an encoder of the gat2 family (gat2, gat2_lite, gat2_edge) or gcn2, on the GPU."""
    _level(level), _batch_size(batch_size)
    _encoder(model, "embed")
    store = _as_store(source, engine_device(model, "embed"))
    return _embed_store(model, store, level, batch_size, "embed")


def embed_all(model, source, level: str, batch_size: int = 512):
    """``(rows [total, width] on the device, offsets int64 [n_mols + 1] on the host)``: every batch of ``embed`` gathered."""
    import torch
    parts = list(embed(model, source, level, batch_size))
    rows = torch.cat([p.rows for p in parts], 0)
    return rows, offsets_of(np.concatenate([np.diff(p.offsets) for p in parts]))


def rows_to_mol_frag(index, offsets):
    """Global embedding rows -> ``(molecule, row inside the molecule)`` through the molecules' first rows ``offsets`` [n_mols + 1];
    molecules without rows own none.  An empty slot (-1) maps to (-1, -1)."""
    index, offsets = np.asarray(index, dtype=np.int64), np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("rows_to_mol_frag: offsets must rise from 0")
    if ((index < -1) | (index >= offsets[-1])).any():
        raise ValueError(f"rows_to_mol_frag: a row outside -1 .. {int(offsets[-1]) - 1}")
    mol = np.searchsorted(offsets, index, side="right") - 1
    frag = index - offsets[np.maximum(mol, 0)]
    empty = index < 0
    return np.where(empty, -1, mol), np.where(empty, -1, frag)


class Neighbours(_Result):
    """Result of ``nearest``.  ``score`` / ``index`` [n_q, k]: per query row the best ``k`` library rows, best first (``index`` is the
    global library row, -1 where the library had fewer than k candidates; then ``score`` is -inf, +inf for ``"l2"``); ``mol`` [n_q, k]
    the library molecule of that row.  Level ``"mol"``: a query row is a query molecule and ``index == mol``.  Level ``"frag"``: a
    query row is a fragment -- ``query_mol`` / ``query_frag`` [n_q] name it, ``frag`` [n_q, k] is the neighbour's fragment number inside
    its molecule, ``query_offsets`` / ``library_offsets`` the molecules' first rows.  ``result[i]`` is query MOLECULE i as a dict of its
    rows: ``score``, ``index``, ``mol`` ([k] for ``"mol"``, [its fragments, k] for ``"frag"``, there with ``frag``)."""

    def __init__(self, level: str, metric: str, score: np.ndarray, index: np.ndarray, query_offsets: np.ndarray,
                 library_offsets: np.ndarray):
        self.level, self.metric = _level(level), metric
        self.score, self.index = np.asarray(score), np.asarray(index, dtype=np.int64)
        self.query_offsets = np.asarray(query_offsets, dtype=np.int64)
        self.library_offsets = np.asarray(library_offsets, dtype=np.int64)
        if self.score.shape != self.index.shape or self.score.ndim != 2 or self.score.shape[0] != self.query_offsets[-1]:
            raise ValueError(f"Neighbours: score {self.score.shape} / index {self.index.shape} do not match the "
                             f"{int(self.query_offsets[-1])} query rows")
        self.mol, self.frag = rows_to_mol_frag(self.index, self.library_offsets)
        rows = np.arange(self.score.shape[0], dtype=np.int64)
        self.query_mol, self.query_frag = rows_to_mol_frag(rows, self.query_offsets)

    def __len__(self):
        return self.query_offsets.shape[0] - 1

    def __getitem__(self, i: int) -> dict:
        i = self._index(i)
        lo, hi = int(self.query_offsets[i]), int(self.query_offsets[i + 1])
        rows = slice(lo, hi) if self.level == "frag" else lo
        out = {"score": self.score[rows], "index": self.index[rows], "mol": self.mol[rows]}
        if self.level == "frag":
            out["frag"] = self.frag[rows]
        return out

    def domain_distance(self) -> np.ndarray:
        """The applicability-domain number, [query molecules]: the best score of each query molecule -- of its one row for ``"mol"``,
        the best over its fragments for ``"frag"`` (a molecule without rows, or a library without candidates: the empty score)."""
        smaller = self.metric == "l2"
        out = np.full(len(self), np.inf if smaller else -np.inf, dtype=self.score.dtype)
        best = self.score[:, 0]
        for i in range(len(self)):
            part = best[int(self.query_offsets[i]): int(self.query_offsets[i + 1])]
            if part.size:
                out[i] = part.min() if smaller else part.max()
        return out

    def arrays(self) -> Dict[str, np.ndarray]:
        """A flat dict for ``np.savez``: ``score``, ``index``, ``mol`` [n_q, k], ``domain_distance`` [query molecules], ``level``,
        ``metric``; for ``"frag"`` also ``frag`` [n_q, k], ``query_mol``, ``query_frag`` [n_q], ``query_offsets``, ``library_offsets``."""
        out = {"score": self.score, "index": self.index, "mol": self.mol, "domain_distance": self.domain_distance(),
               "level": np.array(self.level), "metric": np.array(self.metric)}
        if self.level == "frag":
            out.update(frag=self.frag, query_mol=self.query_mol, query_frag=self.query_frag, query_offsets=self.query_offsets,
                       library_offsets=self.library_offsets)
        return out


def _aux(rows, metric: int):
    """What ``ops.TopK.update`` wants next to the rows: nothing for dot, reciprocal norms for cosine, squared norms for l2."""
    from . import ops
    if metric == 0:
        return None
    return ops.rows_rnorm(rows) if metric == 1 else (rows * rows).sum(1)


def nearest(model, queries, library, level: str = "mol", k: int = 8, metric: str = "cosine", batch_size: int = 512,
            exclude_self: bool = False) -> Neighbours:
    """The ``k`` nearest library rows of every query row in ``model``'s embedding space (``embed``), under ``metric``: ``"cosine"``,
    ``"dot"`` (larger is better) or ``"l2"`` (squared distance, smaller is better).  ``queries`` / ``library``: a ``FlatMolStore`` or a
    list of ``MolRecord`` each.  The queries are embedded once and held ([n_q, width]); the library is embedded batch by batch, each
    batch folded into the lists by one ``ops.TopK.update`` and dropped.  ``exclude_self=True`` needs ``queries is library`` and skips
    each row's own id.  Ties go to the smaller library row."""
    import torch
    from . import ops
    _level(level), _batch_size(batch_size)
    k, m = ops.topk_k(k), ops.topk_metric(metric)
    metric = next(name for name, v in ops.TOPK_METRICS.items() if v == m)
    if exclude_self and queries is not library:
        raise ValueError("nearest: exclude_self=True skips each row's own id, so it needs `queries is library` (the same object)")
    _encoder(model, "nearest")
    device = engine_device(model, "nearest")
    q_store = _as_store(queries, device)
    lib_store = q_store if library is queries else _as_store(library, device)
    q_parts = list(_embed_store(model, q_store, level, batch_size, "nearest"))
    q = torch.cat([p.rows for p in q_parts], 0).contiguous()
    q_offsets, lib_offsets = row_offsets(q_store, level), row_offsets(lib_store, level)
    del q_parts
    q_aux = _aux(q, m)
    exclude = torch.arange(q.shape[0], dtype=torch.int64, device=device) if exclude_self else None
    top = ops.TopK(int(q.shape[0]), k, m, device)
    for part in _embed_store(model, lib_store, level, batch_size, "nearest"):
        top.update(q, part.rows, int(lib_offsets[part.first]), q_aux, _aux(part.rows, m), exclude)
    score, index = top.result()
    return Neighbours(level, metric, score.cpu().numpy(), index.cpu().numpy(), q_offsets, lib_offsets)
