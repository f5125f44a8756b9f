"""The chemical-space map of a store and the Mahalanobis applicability domain, in the space the encoder learned: the data-set level
view next to the per-molecule pictures (attention read-outs, leave-one-out, Shapley) and the neighbour / diversity drivers.

``fit`` sweeps a source once (``neighbours.embed``) and keeps nothing but the fp64 moments of the rows (ops.Moments, csrc/moments.hip:
count, column sums, Gram matrix; no [n, d] temporary, no library GEMM, one order of addition).  The host turns the moments into a PCA
in float64 numpy (``solve``).  ``EmbeddingSpace.transform`` gives PCA coordinates, ``EmbeddingSpace.mahalanobis`` the squared
Mahalanobis distance to the fitted distribution -- both one ``ops.rows_project`` launch per batch of rows.  ``map`` puts the two
together for a library and optional queries.

Levels as everywhere: ``"mol"`` the pooled 256-wide read-outs, ``"frag"`` the 128-wide fragment rows.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from .attribution import _as_store, _Result, engine_device
from .neighbours import LEVEL_WIDTH, _batch_size, _embed_store, _encoder, _level, row_offsets, rows_to_mol_frag

WIDTH_LEVEL = {w: name for name, w in LEVEL_WIDTH.items()}


def chain_gamma(terms: int) -> float:
    """Higham's gamma of an fp32 chain of ``terms`` fused multiply-adds: ``terms u / (1 - terms u)``, u = 2^-24."""
    t = terms * 2.0 ** -24
    return t / (1.0 - t)


def _moments_chunk() -> int:
    from . import _lib
    return _lib.MOMENTS_CHUNK


def sign_components(v: np.ndarray) -> np.ndarray:
    """The columns of ``v`` signed so that each one's entry of largest magnitude is positive; on ties the lowest index decides."""
    v = np.array(v, dtype=np.float64)
    for c in range(v.shape[1]):
        if v[int(np.argmax(np.abs(v[:, c]))), c] < 0:          # argmax: the first of equal magnitudes
            v[:, c] = -v[:, c]
    return v


class EmbeddingSpace:
    """A fitted embedding space.  ``n`` rows of ``width`` at ``level``; ``mean`` [width]; ``eigenvalues`` [width] of the covariance
    (divisor n), descending; ``components`` [width, width], column c the unit direction of eigenvalue c, signed so that its entry of
    largest magnitude is positive; ``floor`` the a-priori bound of the moments kernel on an eigenvalue's error,
    ``gamma (trace(cov) + |sum / n|^2)`` with ``gamma = L u / (1 - L u)``, L = FN_MOMENTS_CHUNK, u = 2^-24; ``rank`` the number of
    eigenvalues above it; ``explained_variance_ratio`` [width].  ``shift`` / ``sum`` / ``gram`` are the moments it was solved from:
    ``sum`` and ``gram`` of ``row - shift``.  Everything is float64 numpy on the host."""

    def __init__(self, n: int, level: str, shift, total, gram, chunk: Optional[int] = None):
        self.level = _level(level)
        self.width = LEVEL_WIDTH[self.level]
        self.shift = np.asarray(shift, dtype=np.float64).reshape(-1)
        self.sum, self.gram = np.asarray(total, dtype=np.float64).reshape(-1), np.asarray(gram, dtype=np.float64)
        if self.shift.shape != (self.width,) or self.sum.shape != (self.width,) or self.gram.shape != (self.width, self.width):
            raise ValueError(f"EmbeddingSpace: level {level!r} needs shift and sum [{self.width}] and gram [{self.width}, {self.width}]; got "
                             f"{self.shift.shape}, {self.sum.shape}, {self.gram.shape}")
        if not isinstance(n, (int, np.integer)) or n < 2:
            raise ValueError(f"EmbeddingSpace: a covariance needs at least 2 rows, got {n!r}")
        if not (np.isfinite(self.sum).all() and np.isfinite(self.gram).all() and np.isfinite(self.shift).all()):
            raise ValueError("EmbeddingSpace: the moments are not finite (a NaN or an infinity among the embedding rows)")
        self.n = int(n)
        m = self.sum / self.n
        self.mean = self.shift + m
        cov = self.gram / self.n - np.outer(m, m)
        cov = 0.5 * (cov + cov.T)                       # (gram is symmetric bit for bit; this keeps eigh's input so after the outer product)
        w, v = np.linalg.eigh(cov)
        order = np.argsort(-w, kind="stable")
        self.eigenvalues, self.components = w[order], sign_components(v[:, order])
        gamma = chain_gamma(_moments_chunk() if chunk is None else chunk)
        self.floor = float(gamma * (np.trace(cov) + m @ m))
        self.rank = int((self.eigenvalues > self.floor).sum())
        trace = float(self.eigenvalues.sum())
        self.explained_variance_ratio = self.eigenvalues / trace if trace > 0 else np.zeros_like(self.eigenvalues)
        self._cache = {}

    # ---- host side
    def directions(self, k: int) -> np.ndarray:
        """``components[:, :k]`` -- the projection matrix of ``transform``; k > rank is refused."""
        if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 1:
            raise ValueError(f"k must be a positive integer, got {k!r}")
        if k > self.rank:
            raise ValueError(f"k = {k} exceeds the rank {self.rank} of the fitted space: the directions behind it are below the moments' "
                             f"own error bound ({self.floor:.3e})")
        return self.components[:, :k]

    def whitening(self) -> np.ndarray:
        """``V_r Lambda_r^-1/2`` [width, rank]: the rows' squared norm after it is the squared Mahalanobis distance."""
        if self.rank < 1:
            raise ValueError("the fitted space has rank 0: every eigenvalue is below the moments' own error bound")
        return self.components[:, :self.rank] / np.sqrt(self.eigenvalues[:self.rank])

    # ---- device side
    def _device_pair(self, key, matrix, device):
        import torch
        if (key, device) not in self._cache:
            self._cache[(key, device)] = (torch.as_tensor(np.ascontiguousarray(matrix), dtype=torch.float32).to(device).contiguous(),
                                          torch.as_tensor(self.mean, dtype=torch.float32).to(device).contiguous())
        return self._cache[(key, device)]

    def _batches(self, rows_or_source, model, batch_size: int, who: str):
        import torch
        if torch.is_tensor(rows_or_source):
            if rows_or_source.dim() != 2 or rows_or_source.shape[1] != self.width:
                raise ValueError(f"{who}: rows must be [rows, {self.width}] (level {self.level!r}), got {tuple(rows_or_source.shape)}")
            yield rows_or_source
            return
        if model is None:
            raise ValueError(f"{who}: a source of molecules needs the model that embeds them (model=...); a device row table does not")
        _encoder(model, who)
        store = _as_store(rows_or_source, engine_device(model, who))
        for part in _embed_store(model, store, self.level, _batch_size(batch_size), who):
            yield part.rows

    def _project(self, rows_or_source, model, batch_size, who, key, matrix, want_rows: bool):
        import torch
        from . import ops
        outs = []
        for rows in self._batches(rows_or_source, model, batch_size, who):
            rows = ops._f32c(rows, f"{who}: rows")             # (CPU rows are refused before anything is put on a device)
            W, mean = self._device_pair(key, matrix, rows.device)
            out, sq = ops.rows_project(rows, W, mean, want_rows=want_rows, want_sq=not want_rows)
            outs.append(out if want_rows else sq)
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def transform(self, rows_or_source, k: int = 2, model=None, batch_size: int = 512):
        """PCA coordinates [rows, k] on the device, fp32: ``(row - mean) @ components[:, :k]`` by ``ops.rows_project``, mean and
        components rounded to fp32.  ``rows_or_source``: a device row table [rows, width], or a store / record list with ``model``.
        k > rank is refused.  A row's coordinates depend on that row alone: a slice gives the same bits as the whole table."""
        return self._project(rows_or_source, model, batch_size, "transform", ("pca", int(k)), self.directions(k), True)

    def mahalanobis(self, rows_or_source, model=None, batch_size: int = 512):
        """Squared Mahalanobis distance [rows] of every row to the fitted distribution, on the device, fp32: the squared norm of
        ``(row - mean) @ V_r Lambda_r^-1/2`` (``ops.rows_project`` with ``want_sq`` alone: no [rows, rank] table is written).  This is
        the PSEUDO-inverse form: the ``width - rank`` directions whose eigenvalue is below ``floor`` are dropped, not divided by, so a
        row's distance ignores its component outside the fitted rows' span.  Over the fitted rows the mean is ``rank``."""
        return self._project(rows_or_source, model, batch_size, "mahalanobis", ("maha", self.rank), self.whitening(), False)


def solve(n: int, shift, total, gram, level: Optional[str] = None, chunk: Optional[int] = None) -> EmbeddingSpace:
    """The host half of ``fit``: float64 moments of ``row - shift`` over ``n`` rows -> ``EmbeddingSpace``.  ``level``: by the width when
    not named."""
    if level is None:
        width = int(np.asarray(total).reshape(-1).shape[0])
        if width not in WIDTH_LEVEL:
            raise ValueError(f"rows of {width} floats belong to no level ({', '.join(f'{w}: {name}' for w, name in WIDTH_LEVEL.items())})")
        level = WIDTH_LEVEL[width]
    return EmbeddingSpace(n, level, shift, total, gram, chunk)


def _fit_batches(batches, level: str, device, keep: bool):
    """Moments of the row batches (one ``Moments.update`` each; the first non-empty batch's fp32 column mean is the shift, which keeps
    ``gram / n - m m^T`` free of cancellation) and ONE device -> host copy.  ``keep``: also returns the batches, concatenated."""
    import torch
    from . import ops
    mom, shift, kept = ops.Moments(LEVEL_WIDTH[level], device), None, []
    for rows in batches:
        if keep:
            kept.append(rows)
        if rows.shape[0] == 0:
            continue
        if shift is None:
            shift = rows.mean(0)
        mom.update(rows, shift)
    n, total, gram = mom.result()
    if n < 2:
        raise ValueError(f"fit: a covariance needs at least 2 rows, the source has {n}")
    d = mom.d
    host = torch.cat([total, gram.reshape(-1), shift.double()]).cpu().numpy()
    space = EmbeddingSpace(n, level, host[d + d * d:], host[:d], host[d: d + d * d].reshape(d, d))
    return space, (torch.cat(kept, 0) if keep else None)


def _rows_level(rows, level, who: str) -> str:
    from . import ops
    rows = ops._f32c(rows, f"{who}: rows")
    if rows.dim() != 2 or rows.shape[1] not in WIDTH_LEVEL:
        raise ValueError(f"{who}: a row table must be [rows, 256] (level \"mol\") or [rows, 128] (\"frag\"), got {tuple(rows.shape)}")
    if level is not None and LEVEL_WIDTH[_level(level)] != rows.shape[1]:
        raise ValueError(f"{who}: level {level!r} has rows of {LEVEL_WIDTH[level]} floats, the table has {rows.shape[1]}")
    return WIDTH_LEVEL[int(rows.shape[1])]


def fit(model, source=None, level: Optional[str] = None, batch_size: int = 512) -> EmbeddingSpace:
    """The embedding space of ``source`` (a ``FlatMolStore`` or a list of ``MolRecord``) under ``model`` -- any finetune or pretrain model
    of the gat2 family or gcn2, on the GPU; pair models are refused by name -- at ``level`` (default ``"mol"``): one ``neighbours.embed``
    sweep, one ``ops.Moments.update`` per batch, one device -> host copy at the end, then the float64 eigen-decomposition on the host.
    ``fit(rows)``: a device row table [n, 256] or [n, 128] instead of (model, source), folded in as one batch.  Fewer than 2 rows and
    non-finite moments are refused."""
    import torch
    _batch_size(batch_size)
    if torch.is_tensor(model):
        if source is not None:
            raise ValueError("fit: a row table comes alone (fit(rows)); a source of molecules comes with its model (fit(model, source))")
        level = _rows_level(model, level, "fit")
        return _fit_batches([model.contiguous()], level, model.device, False)[0]
    level = _level("mol" if level is None else level)
    _encoder(model, "fit")
    if source is None:
        raise ValueError("fit: no source of molecules")
    device = engine_device(model, "fit")
    store = _as_store(source, device)
    return _fit_batches((p.rows for p in _embed_store(model, store, level, batch_size, "fit")), level, device, False)[0]


class ChemMap(_Result):
    """Result of ``map``.  ``coords`` [N, k] / ``d2`` [N]: PCA coordinates and squared Mahalanobis distance of the library's rows in the
    space fitted on them (``space``); ``mol`` / ``frag`` [N] the molecule of each row and the row's number inside it, ``offsets``
    [molecules + 1] the molecules' first rows.  ``domain_cutoff``: the ``quantile`` of the library's own ``d2``.  With queries:
    ``query_coords`` [Q, k], ``query_d2`` [Q], ``inside`` [Q] (``query_d2 <= domain_cutoff``), ``query_mol`` / ``query_frag`` [Q],
    ``query_offsets``; without, those are empty.  ``result[i]`` is library row i as a dict."""
    _per_item = "coords"

    def __init__(self, space: EmbeddingSpace, quantile: float, coords, d2, offsets, query_coords=None, query_d2=None, query_offsets=None):
        self.space, self.level, self.quantile = space, space.level, float(quantile)
        if not 0.0 <= self.quantile <= 1.0:
            raise ValueError(f"quantile must be in [0, 1], got {quantile!r}")
        self.coords, self.d2 = np.asarray(coords, dtype=np.float32), np.asarray(d2, dtype=np.float32).reshape(-1)
        self.offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        if self.coords.ndim != 2 or self.coords.shape[0] != self.d2.shape[0] or self.offsets.size < 1 or self.offsets[-1] != self.d2.shape[0]:
            raise ValueError(f"ChemMap: coords {self.coords.shape} / d2 {self.d2.shape} do not match the rows of offsets")
        self.k = int(self.coords.shape[1])
        if query_coords is None:
            query_coords, query_d2, query_offsets = np.zeros((0, self.k)), np.zeros(0), np.zeros(1)
        self.query_coords, self.query_d2 = np.asarray(query_coords, dtype=np.float32), np.asarray(query_d2, dtype=np.float32).reshape(-1)
        self.query_offsets = np.asarray(query_offsets, dtype=np.int64).reshape(-1)
        if self.query_coords.shape != (self.query_d2.shape[0], self.k) or self.query_offsets[-1] != self.query_d2.shape[0]:
            raise ValueError(f"ChemMap: query_coords {self.query_coords.shape} / query_d2 {self.query_d2.shape} do not match the query rows")
        self.domain_cutoff = float(np.quantile(self.d2.astype(np.float64), self.quantile)) if self.d2.size else float("nan")
        self.inside = self.query_d2 <= self.domain_cutoff
        self.mol, self.frag = rows_to_mol_frag(np.arange(self.d2.shape[0]), self.offsets)
        self.query_mol, self.query_frag = rows_to_mol_frag(np.arange(self.query_d2.shape[0]), self.query_offsets)

    def __getitem__(self, i: int) -> dict:
        i = self._index(i)
        return {"coords": self.coords[i], "d2": float(self.d2[i]), "mol": int(self.mol[i]), "frag": int(self.frag[i])}

    def arrays(self) -> Dict[str, np.ndarray]:
        """A flat dict for ``np.savez``: the fields above plus the fitted space (``n``, ``mean``, ``eigenvalues``, ``components``,
        ``rank``, ``floor``, ``explained_variance_ratio``), ``level`` and ``quantile``."""
        s = self.space
        return {"coords": self.coords, "d2": self.d2, "mol": self.mol, "frag": self.frag, "offsets": self.offsets,
                "query_coords": self.query_coords, "query_d2": self.query_d2, "query_mol": self.query_mol, "query_frag": self.query_frag,
                "query_offsets": self.query_offsets, "inside": self.inside, "domain_cutoff": np.array(self.domain_cutoff),
                "quantile": np.array(self.quantile), "level": np.array(self.level), "n": np.array(s.n), "mean": s.mean,
                "eigenvalues": s.eigenvalues, "components": s.components, "rank": np.array(s.rank), "floor": np.array(s.floor),
                "explained_variance_ratio": s.explained_variance_ratio}


def map(model, library, queries=None, level: str = "mol", k: int = 2, quantile: float = 0.95, batch_size: int = 512) -> ChemMap:      # noqa: A001
    """The chemical-space map of ``library`` under ``model``: the space is fitted on the library (``fit``: one sweep, whose rows are held
    on the device as ``diversity.select`` holds them), then the library's and the ``queries``' rows get ``k`` PCA coordinates and their
    squared Mahalanobis distance.  ``domain_cutoff`` is the ``quantile`` of the library's own distances -- the caller's choice, not a
    measured number -- and ``inside`` says which query rows are at or below it."""
    _level(level), _batch_size(batch_size)
    if not isinstance(quantile, (int, float)) or isinstance(quantile, bool) or not 0.0 <= quantile <= 1.0:
        raise ValueError(f"map: quantile must be in [0, 1], got {quantile!r}")
    if not isinstance(k, int) or isinstance(k, bool) or k < 1:
        raise ValueError(f"map: k must be a positive integer, got {k!r}")
    _encoder(model, "map")
    device = engine_device(model, "map")
    lib_store = _as_store(library, device)
    space, rows = _fit_batches((p.rows for p in _embed_store(model, lib_store, level, batch_size, "map")), level, device, True)
    space.directions(k)                                        # (k > rank is refused before anything is projected)

    def placed(batches):                                       # each batch embedded once, projected twice
        import torch
        both = [(space.transform(r, k), space.mahalanobis(r)) for r in batches]
        return torch.cat([c for c, _ in both], 0).cpu().numpy(), torch.cat([d for _, d in both], 0).cpu().numpy()

    coords, d2 = placed([rows.contiguous()])
    q = (None, None, None)
    if queries is not None:
        q_store = lib_store if queries is library else _as_store(queries, device)
        q = (*placed(p.rows for p in _embed_store(model, q_store, level, batch_size, "map")), row_offsets(q_store, level))
    return ChemMap(space, quantile, coords, d2, row_offsets(lib_store, level), *q)
