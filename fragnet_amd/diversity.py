"""Diverse subsets and cluster splits in the space the encoder learned: greedy k-centre (farthest-point selection; MaxMin picking to
cheminformatics users) over the embedding rows of ``neighbours.embed_all``, on the GPU (ops.KCenter, csrc/kcenter.hip: one launch per
pick, nothing synchronises with the host between picks).

``select`` picks ``k`` rows that cover a source -- molecules (level ``"mol"``, the pooled 256-wide read-outs) or fragments (``"frag"``,
the 128-wide fragment rows) -- and labels every row with its nearest pick; the coverage radius after every pick comes with it.  With
``seeds`` or ``init_distance`` it answers "which k rows are least like what I already have".  ``Diverse.split`` hands whole clusters to
train / valid / test: a structure split without RDKit, where the reference splits by Murcko scaffold (fragnet/dataset/splitters.py).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from .attribution import _as_store, _Result, engine_device
from .neighbours import _batch_size, _encoder, _level, embed_all, row_offsets, rows_to_mol_frag

MAX_SEED_ROWS = 4096        # a seed costs one pass over the rows; a larger set goes in as a distance (init_distance)


class Diverse(_Result):
    """Result of ``select``.  ``picked`` [k]: the chosen embedding rows in pick order; ``mol`` / ``frag`` [k] the molecule of each and
    the row's number inside it (level ``"mol"``: ``picked == mol``, ``frag`` 0).  ``radius`` [k + 1]: ``radius[t]`` is the distance of
    pick t to the centres before it when it was picked -- the coverage radius of those (+inf for the first pick of an unseeded run) --
    and ``radius[k]`` the largest distance left, the coverage radius of everything chosen.  ``distance`` [N]: every row's distance to its
    nearest centre (0 for a pick); ``label`` [N]: that centre -- an index into ``picked``; in a seeded run ``-1 - s`` for seed row ``s``; in
    a run with ``init_distance`` -1 for a row no centre came closer to than that.  ``offsets`` [molecules + 1]: the molecules' first rows.  ``result[t]`` is pick t as
    a dict (``row``, ``mol``, ``frag``, ``radius``, ``members``: the rows labelled with it)."""
    _per_item = "picked"

    def __init__(self, level: str, metric: str, picked, radius, distance, label, offsets):
        self.level, self.metric = _level(level), metric
        self.picked, self.radius = np.asarray(picked, dtype=np.int64).reshape(-1), np.asarray(radius, dtype=np.float32).reshape(-1)
        self.distance, self.label = np.asarray(distance, dtype=np.float32).reshape(-1), np.asarray(label, dtype=np.int64).reshape(-1)
        self.offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        n = int(self.offsets[-1]) if self.offsets.size else -1
        if self.radius.shape[0] != self.picked.shape[0] + 1 or self.distance.shape != (n,) or self.label.shape != (n,):
            raise ValueError(f"Diverse: {self.picked.shape[0]} picks need radius [{self.picked.shape[0] + 1}] and distance / label [{n}] "
                             f"(the rows of offsets); got {self.radius.shape}, {self.distance.shape}, {self.label.shape}")
        if (self.label >= self.picked.shape[0]).any():
            raise ValueError("Diverse: a label beyond the picks")
        self.mol, self.frag = rows_to_mol_frag(self.picked, self.offsets)

    def __getitem__(self, t: int) -> dict:
        t = self._index(t)
        return {"row": int(self.picked[t]), "mol": int(self.mol[t]), "frag": int(self.frag[t]), "radius": float(self.radius[t]),
                "members": np.flatnonzero(self.label == t)}

    def arrays(self) -> Dict[str, np.ndarray]:
        """A flat dict for ``np.savez``: ``picked``, ``mol``, ``frag`` [k], ``radius`` [k + 1], ``distance``, ``label`` [N], ``offsets``
        [molecules + 1], ``level``, ``metric``."""
        return {"picked": self.picked, "mol": self.mol, "frag": self.frag, "radius": self.radius, "distance": self.distance,
                "label": self.label, "offsets": self.offsets, "level": np.array(self.level), "metric": np.array(self.metric)}

    def split(self, fractions=(0.8, 0.1, 0.1)) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Train / valid / test molecule indices, sorted, a partition of ``range(N)`` made of WHOLE clusters (the groups of equal
        ``label``; the rows of a seed, and the rows without a centre, are a group each).  Clusters are taken largest first, ties by the
        smallest member, and dealt out by the filling rule of the reference's scaffold split (splitters.py:100-114): a cluster goes to
        train unless train would then pass ``fractions[0] * N``; else to valid unless train + valid would then pass
        ``(fractions[0] + fractions[1]) * N``; else to test.  Level ``"mol"`` only: a fragment split would cut molecules apart."""
        if self.level != "mol":
            raise ValueError('Diverse.split: clusters of fragment rows cut molecules apart; select with level="mol" to split a store')
        fractions = tuple(float(f) for f in fractions)
        if len(fractions) != 3 or min(fractions) < 0 or abs(sum(fractions) - 1.0) > 1e-6:
            raise ValueError(f"Diverse.split: three non-negative fractions that add up to 1, got {fractions!r}")
        n = self.label.shape[0]
        order = np.argsort(self.label, kind="stable")                  # members of a cluster in ascending order, clusters side by side
        cuts = np.flatnonzero(np.diff(self.label[order])) + 1
        clusters = np.split(order, cuts) if n else []
        clusters.sort(key=lambda c: (-c.shape[0], int(c[0])))
        train_cutoff, valid_cutoff = fractions[0] * n, (fractions[0] + fractions[1]) * n
        parts, sizes = ([], [], []), [0, 0, 0]
        for c in clusters:
            if sizes[0] + c.shape[0] <= train_cutoff:
                to = 0
            elif sizes[0] + sizes[1] + c.shape[0] <= valid_cutoff:
                to = 1
            else:
                to = 2
            parts[to].append(c)
            sizes[to] += c.shape[0]
        return tuple(np.sort(np.concatenate(p)) if p else np.zeros(0, dtype=np.int64) for p in parts)


def _check_k(k, n: int, what: str) -> int:
    if not isinstance(k, int) or isinstance(k, bool) or k < 0:
        raise ValueError(f"select: k must be a non-negative integer, got {k!r}")
    if k > n:
        raise ValueError(f"select: k = {k} exceeds the {n} {what} of the source")
    return k


def select(model, source, k: int, level: str = "mol", metric: str = "l2", first=0, seeds=None, init_distance=None,
           batch_size: int = 512) -> Diverse:
    """``k`` rows of ``source`` (a ``FlatMolStore`` or a list of ``MolRecord``) that cover it in ``model``'s embedding space
    (``neighbours.embed_all``; the same models are accepted, pair models are refused by name): greedy k-centre under ``metric`` --
    ``"l2"`` (squared distance, summed directly, never as |x|^2 + |c|^2 - 2 x.c) or ``"cosine"`` (1 - cosine, at least 0); ``"dot"``
    is no distance.  Each pick is the row farthest from the centres so far, ties to the smaller row; ``first`` is the row the run
    starts from (``None``: the arg-max, row 0 of an unseeded run).  The [N, width] rows are held on the device; nothing is read back
    between picks.

    ``seeds``: a store or record list whose rows (at most ``MAX_SEED_ROWS``) are centres before the first pick -- the picks are then the
    rows least like the seeds.  ``init_distance``: an fp32 [N] vector every row's distance starts from instead of +inf (a negative value counts as 0), for a
    larger set, e.g. ``neighbours.nearest(model, source, train, metric="l2", k=1).score[:, 0]``.  Those values come from the
    nearest-neighbour kernel's expanded form q_sq + lib_sq - 2 dot and differ in the last bits from the direct sums here; rows no centre
    comes closer to keep label -1.  With either (not both), ``first`` stays at its default and the arg-max decides."""
    import torch
    from . import ops
    _level(level), _batch_size(batch_size)
    m = ops.kcenter_metric(metric)
    metric = next(name for name, v in ops.KCENTER_METRICS.items() if v == m)
    if seeds is not None and init_distance is not None:
        raise ValueError("select: seeds or init_distance, not both (label -1 is seed row 0 with the one and `no centre` with the other); "
                         "fold the seeds into the distance instead")
    given = seeds is not None or init_distance is not None
    if given and first not in (0, None):
        raise ValueError("select: with seeds or init_distance the first pick is the row farthest from them; leave `first` at its default")
    if first is not None and (not isinstance(first, int) or isinstance(first, bool) or first < 0):
        raise ValueError(f"select: first must be a row number or None, got {first!r}")
    _encoder(model, "select")
    from .dataset import FlatMolStore
    if not isinstance(source, FlatMolStore):
        source = list(source)
    if len(source) == 0:
        raise ValueError("select: no molecules")
    store = source if isinstance(source, FlatMolStore) else FlatMolStore.from_records(source)
    offsets = row_offsets(store, level)
    n = int(offsets[-1])
    k = _check_k(k, n, "molecules" if level == "mol" else "fragment rows")
    if not given and first is not None and first >= max(n, 1):
        raise ValueError(f"select: first = {first} is no row of the source ({n} rows)")
    device = engine_device(model, "select")
    store = _as_store(store, device)
    rows, _ = embed_all(model, store, level, batch_size)
    rows = rows.contiguous()
    if init_distance is not None:
        init_distance = torch.as_tensor(init_distance).to(device)
        if init_distance.dtype != torch.float32 or init_distance.shape != (n,):
            raise ValueError(f"select: init_distance must be float32 [{n}], got {init_distance.dtype} {tuple(init_distance.shape)}")
    seed_rows = None
    if seeds is not None:
        too_many = len(seeds) > MAX_SEED_ROWS                  # (a molecule has at least one row: refused before the store is built)
        seed_store = None if too_many else _as_store(seeds, device)
        n_seed = len(seeds) if too_many else int(row_offsets(seed_store, level)[-1])
        if n_seed > MAX_SEED_ROWS:
            raise ValueError(f"select: {n_seed}{' or more' if too_many else ''} seed rows; a seed costs one pass over the source, so at most {MAX_SEED_ROWS} are folded "
                             "in -- hand a larger set in as init_distance (the distance of every source row to its nearest row of the set, "
                             'e.g. neighbours.nearest(model, source, seeds, metric="l2", k=1).score[:, 0])')
        seed_rows = embed_all(model, seed_store, level, batch_size)[0].contiguous()
    s = 0 if seed_rows is None else int(seed_rows.shape[0])
    kc = ops.KCenter(n, int(rows.shape[1]), m, device, cap=s + k, init_distance=init_distance)
    aux = ops.rows_rnorm(rows) if m == 1 else None
    if s:
        kc.seed(rows, seed_rows, ops.rows_rnorm(seed_rows) if m == 1 else None, aux)
    kc.pick(rows, k, None if given else first, aux)
    picked, radius, mind, label = (t.cpu().numpy() for t in kc.result())
    label = label.astype(np.int64)
    label = np.where(label >= s, label - s, np.where(label >= 0, -1 - label, -1))
    return Diverse(level, metric, picked[s:], radius[s:], np.abs(mind), label, offsets)
