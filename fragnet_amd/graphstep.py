"""Static-shape training step replayed as ONE hipGraph.

An eager step of the hot path is ~200 kernel launches plus the Python around them and is bound by the host
(2.0 ms wall for 1.6 ms of GPU work at ESOL batch 512).  Kernel sizes, however, depend on the batch only through
six counts (atoms, directed bonds, bond-graph edges, fragments, fragment edges, fragment-bond-graph edges), so a
step over buffers of FIXED capacity can be captured once -- graph plan, encoder, pooling, head, loss, backward,
gradient gather -- and replayed with one launch per step.  Every batch (the dict of the reference's
``collate_fn``, dataset/data.py:931-948) is copied into the fixed buffers by one staging kernel
(``fn_stage_padded``) which also fills the tails with PADDING:

* padding rows carry zero features;
* padding index values point at the last ``slack`` slots of the target index space (atoms, bond nodes,
  fragments, fragment edges, molecules), which are guaranteed to be padding themselves, spread round-robin so
  that no padding node collects a large in-degree.

Padding therefore forms extra, disconnected "molecules" behind the real ones: real rows of every level see
exactly the edges they had, the loss is weighted by a 1/0 molecule mask, and padding rows receive zero
upstream gradient -- outputs, loss and parameter gradients of the real batch are unchanged
(tests/test_graphstep.py checks this against the oracle on CPU and against the eager path on the GPU).
Batches that do not fit the capacities fall back to the eager step, sharing optimiser and RNG state.

The all-reduce and the Adam update stay outside the graph (one RCCL call + one kernel) so the N>1 path is the
same collective as in the eager step.

``PairGraphedTrainStep`` is the same step for the pair models (cdrp.CDRPModel, dta.DTAModel2): the second input's int64 rows are
staged too, and the pair head's fused loss reads the real-row count the staging launch wrote instead of a weight vector.
``FactoredPairGraphedTrainStep`` is that step on FACTORED pair batches: two more index spaces (pairs, distinct second inputs) with
capacities of their own (``FactoredPairShapes``), and the pair orderings built inside the graph.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, Iterable, Optional

import torch

from . import _lib
from .plan import LIVE_MOLS_KEY, PLAN_KEY, REAL_ATOMS_KEY, REAL_MOLS_KEY, SPACES, CollatedBatch, prezeroed_plans

# field -> (index space of the ragged axis, layout, index space its VALUES point into)
FIELDS = {
    "x_atoms": ("atom", "rows", None), "batch": ("atom", "ids", "mol"), "atom_to_frag_ids": ("atom", "ids", "frag"),
    "edge_index": ("edge", "cols", "atom"), "edge_attr": ("edge", "rows", None), "node_features_bonds": ("edge", "rows", None),
    "edge_index_bonds_graph": ("bedge", "cols", "edge"), "edge_attr_bonds": ("bedge", "rows", None),
    "x_frags": ("frag", "rows", None), "frag_batch": ("frag", "ids", "mol"),
    "frag_index": ("fedge", "cols", "frag"), "cnx_attr": ("fedge", "rows", None), "node_features_fbonds": ("fedge", "rows", None),
    "edge_index_fbonds": ("fbedge", "cols", "fedge"), "edge_attr_fbonds": ("fbedge", "rows", None),
    "y": ("mol", "rows", None),
    # pretrain targets (collate_fn_pt, dataset/data.py:1028-1030)
    "bnd_lngth": ("edge", "rows", None), "bnd_angl": ("atom", "rows", None), "dh_angl": ("edge", "rows", None),
}
COUNT_FIELD = {"atom": "x_atoms", "edge": "node_features_bonds", "bedge": "edge_attr_bonds", "frag": "x_frags",
               "fedge": "node_features_fbonds", "fbedge": "edge_attr_fbonds", "mol": "y"}
# the second input of a pair model (data.collate_fn_cdrp / collate_fn_dta: one int64 row per pair), staged through FN_STAGE_ROWS_I64 with
# zero rows behind the real ones.  A table of its own: FIELDS is what a property batch may carry
PAIR_FIELDS = {"gene_expr": ("mol", "rows_i64", None), "protein": ("mol", "rows_i64", None)}
MASK_KEY = "mol_weight"           # float32 [mol cap]: 1 for real molecules, 0 for padding
MASKS = {"mol": MASK_KEY, "atom": "atom_weight", "edge": "edge_weight"}     # 1/0 weights of the mean losses
SCALE_KEY = "loss_scales"         # float32 [2]: (per-edge, per-atom) rank weights of the pretrain loss, 1 on one GPU
_OFFSETS = object()               # StaticBatch: the staged field whose source is the batch's offsets table, not one of its keys


# "thread_local": HIP calls of OTHER threads (the collective library's watchdog, a data-loader thread) do not invalidate
# a capture in progress; everything the captured step itself does runs on the capturing thread
_CAPTURE_MODE = "thread_local"


def _gat_limit(heads: int) -> int:
    """Padding in-degree that stays on the kernels' one-pass path (in-degree <= 2 * 32/heads, self loop included)."""
    return max(2, min(12, (2 * (32 // heads) * 3) // 4))


def _pairs(heads: int):
    g = _gat_limit(heads)
    # node space -> [(item space whose values point into it, max padding items per padding node)]
    return [("edge", [("bedge", g)]), ("fedge", [("fbedge", g)]), ("atom", [("edge", g)]),
            ("frag", [("fedge", g), ("atom", 32)]), ("mol", [("atom", 64), ("frag", 64)])]


def batch_counts(batch: Dict[str, torch.Tensor]) -> Dict[str, int]:
    return {sp: int(batch[f].shape[0]) for sp, f in COUNT_FIELD.items()}


def _up(x: int, q: int = 64) -> int:
    return (x + q - 1) // q * q


class StaticShapes:
    """Capacities per index space + the number of trailing slots of each node space reserved for padding."""

    def __init__(self, cap: Dict[str, int], slack: Dict[str, int], heads: int = 4, lower: Optional[Dict[str, int]] = None,
                 max_per_mol: Optional[Dict[str, int]] = None):
        self.cap, self.slack, self.heads = dict(cap), dict(slack), heads
        self.lower = dict(lower) if lower else {sp: 0 for sp in cap}       # fewest real items a batch is expected to bring
        # largest molecule the one-launch plan builder's LDS tile is sized for (None: batches carry no such bound)
        self.max_per_mol = dict(max_per_mol) if max_per_mol else None

    @classmethod
    def from_counts(cls, counts: Iterable[Dict[str, int]], margin: float = 0.03, heads: int = 4, spread_sigmas: float = 4.0) -> "StaticShapes":
        counts = list(counts)
        mx = {sp: max(c[sp] for c in counts) for sp in COUNT_FIELD}
        mn = {sp: min(c[sp] for c in counts) for sp in COUNT_FIELD}
        # a small index space varies far more from batch to batch than the margin allows for (fragment-bond-graph edges of ESOL-shape
        # batches of 512: 8.5 k ... 10.4 k, +-5 % one sigma): with three or more sample batches the bounds also cover mean +- 4 sigma
        # (spread_sigmas = 0: the sample IS the data that will run -- a benchmark pool sized from itself -- so max / min are exact)
        if len(counts) >= 3 and spread_sigmas > 0:
            for sp in COUNT_FIELD:
                v = [float(c[sp]) for c in counts]
                mean = sum(v) / len(v)
                sd = (sum((x - mean) ** 2 for x in v) / (len(v) - 1)) ** 0.5
                mx[sp] = max(mx[sp], int(math.ceil((mean + spread_sigmas * sd) / (1.0 + margin)))) if sp != "mol" else mx[sp]
                mn[sp] = min(mn[sp], max(0, int((mean - spread_sigmas * sd) / (1.0 - margin)))) if sp != "mol" else mn[sp]
        lower = {sp: int(mn[sp] * (1.0 - margin)) for sp in COUNT_FIELD}
        cap, slack = {}, {}
        for sp in ("bedge", "fbedge"):
            cap[sp] = _up(int(math.ceil(mx[sp] * (1.0 + margin))))
        for node, sources in _pairs(heads):
            need = max(-(-(cap[item] - lower[item]) // lim) for item, lim in sources)
            slack[node] = max(8, need)
            grow = 0.0 if node == "mol" else margin
            cap[node] = _up(int(math.ceil(mx[node] * (1.0 + grow))) + slack[node], 8)
            if node == "mol":       # the batch size is exact: every slot the rounding added is padding too (the head skips them)
                slack[node] = cap[node] - mx[node]
        return cls(cap, slack, heads, lower)

    @classmethod
    def from_batches(cls, batches, margin: float = 0.03, heads: int = 4, spread_sigmas: float = 4.0) -> "StaticShapes":
        batches = list(batches)
        shapes = cls.from_counts([batch_counts(b) for b in batches], margin, heads, spread_sigmas)
        bounds = [getattr(b, "max_per_mol", None) for b in batches]
        if bounds and all(m is not None for m in bounds):       # CollatedBatches: room for molecules half as large again
            shapes.max_per_mol = {sp: (1 if sp == "mol" else _up(int(1.5 * max(m[sp] for m in bounds)) + 8, 8)) for sp in SPACES}
        return shapes

    def fits(self, counts: Dict[str, int], max_per_mol: Optional[Dict[str, int]] = None) -> bool:
        if self.max_per_mol is not None and max_per_mol is not None and any(max_per_mol[sp] > self.max_per_mol[sp] for sp in SPACES):
            return False        # a molecule larger than the plan builder's tile was sized for
        for sp, n in counts.items():
            if n > self.cap[sp] - self.slack.get(sp, 0):
                return False
        for node, sources in _pairs(self.heads):
            for item, lim in sources:
                if self.cap[item] - counts[item] > lim * self.slack[node]:
                    return False
        return True

    def capacity(self, space: str) -> int:
        """Rows a staged field of ``space`` has (a subclass may know index spaces outside ``cap``)."""
        return self.cap[space]

    def pad_rule(self, target: str):
        """(pad_hi, pad_mod): padding position i of a field pointing into ``target`` holds pad_hi - (i - n_real) % pad_mod."""
        return self.cap[target] - 1, self.slack[target]

    def pad_info(self) -> Dict[str, Dict[str, int]]:
        """CollatedBatch.pad of a batch staged into these shapes (plan.GraphPlan.from_batch -> fn_plan_build_mol)."""
        return {"cap": dict(self.cap), "mod": dict(self.slack),
                "hint": {sp: self.cap[sp] - self.lower.get(sp, 0) for sp in self.cap}}

    def __repr__(self):
        return f"StaticShapes(cap={self.cap}, slack={self.slack})"


def pad_batch(batch: Dict[str, torch.Tensor], shapes: StaticShapes) -> Dict[str, torch.Tensor]:
    """Reference implementation of the staging kernel with torch ops (any device): the padded batch dict."""
    counts = batch_counts(batch)
    if not shapes.fits(counts):
        raise ValueError(f"batch {counts} does not fit {shapes}")
    out = {}
    for name, (space, layout, target) in FIELDS.items():
        if name not in batch:
            continue
        src, cap, n = batch[name], shapes.cap[space], counts[space]
        if layout == "rows":
            dst = src.new_zeros((cap,) + tuple(src.shape[1:]))
            dst[:n] = src
        else:
            hi, mod = shapes.pad_rule(target)
            pad = hi - (torch.arange(cap, device=src.device, dtype=torch.long) - n) % mod
            if layout == "ids":
                dst = pad.clone()
                dst[:n] = src
            else:
                dst = pad.repeat(2, 1)
                dst[:, :n] = src
        out[name] = dst
    for space, key in MASKS.items():
        w = torch.zeros(shapes.cap[space], dtype=torch.float32, device=batch["y"].device)
        w[: counts[space]] = 1.0
        out[key] = w
    if isinstance(batch, CollatedBatch) and batch.offsets is not None:      # the staged offsets table (FN_STAGE_OFFSETS)
        out = batch.like(out)
        B, cap = counts["mol"], shapes.cap["mol"]
        off = batch.offsets.new_empty((len(SPACES), cap + 1))
        off[:, : B + 1] = batch.offsets
        off[:, B + 1:] = batch.offsets[:, B:]
        out.offsets, out.pad = off, shapes.pad_info()
        if shapes.max_per_mol is not None:
            out.max_per_mol = shapes.max_per_mol
    return out


def pad_pair_batch(batch: Dict[str, torch.Tensor], shapes: StaticShapes) -> Dict[str, torch.Tensor]:
    """``pad_batch`` of a one-record-per-pair batch: the second input's int64 rows (PAIR_FIELDS) with zero rows behind the real ones, up to
    the ``mol`` capacity -- that of ``y``."""
    out = pad_batch(batch, shapes)
    for name in PAIR_FIELDS:
        if name in batch:
            src = batch[name]
            dst = src.new_zeros((shapes.cap["mol"],) + tuple(src.shape[1:]))
            dst[: src.shape[0]] = src
            out[name] = dst
    return out


# A FACTORED pair batch (data.collate_fn_*_factored) has two index spaces the encoder knows nothing of: ``pair`` (its M pairs: y and the
# two pair lists) and ``second`` (its C distinct second inputs).  Neither is in plan.SPACES or in the offsets table; nothing points INTO
# them through a padded index, so they need no slack: a capacity each (FactoredPairShapes).  ``y`` takes the place of FIELDS' entry.
PAIR_SPACES = ("pair", "second")
FACTORED_PAIR_FIELDS = {"y": ("pair", "rows", None), "gene_expr": ("second", "rows_i64", None), "protein": ("second", "rows_i64", None),
                        "pair_drug": ("pair", "vec_i64", None), "pair_second": ("pair", "vec_i64", None)}
REAL_PAIRS_KEY = "_real_pairs"    # StaticBatch.add_count("pair"): device-side count of the real pairs of a staged factored batch


def factored_batch_counts(batch: Dict[str, torch.Tensor]) -> Dict[str, int]:
    """``batch_counts`` of a factored pair batch: the molecule count is the one the batch carries (``plan.N_MOLS_KEY``; ``y`` has one
    entry per PAIR), plus the two spaces of PAIR_SPACES."""
    from .plan import batch_n_mols
    counts = {sp: int(batch[f].shape[0]) for sp, f in COUNT_FIELD.items() if sp != "mol"}
    counts["mol"] = batch_n_mols(batch)
    counts["pair"] = int(batch["y"].shape[0])
    counts["second"] = int(next(batch[k] for k in PAIR_FIELDS if k in batch).shape[0])
    return counts


class FactoredPairShapes(StaticShapes):
    """``StaticShapes`` plus ``pair_cap`` and ``second_cap``.  ``cap`` / ``slack`` keep plan.SPACES' seven entries (the plan builder's
    padding rule reads them); the ``mol`` space holds the U DISTINCT drugs, which vary from batch to batch like any other count."""

    def __init__(self, cap, slack, heads: int = 4, lower=None, max_per_mol=None, pair_cap: int = 0, second_cap: int = 0):
        super().__init__(cap, slack, heads, lower, max_per_mol)
        self.pair_cap, self.second_cap = int(pair_cap), int(second_cap)

    @classmethod
    def from_batches(cls, batches, margin: float = 0.03, heads: int = 4, spread_sigmas: float = 4.0) -> "FactoredPairShapes":
        """Capacities from sample factored batches.  The encoder's spaces as ``StaticShapes.from_counts`` sizes them, except that the real
        room of ``mol`` grows by the margin too (there the batch size is exact; here U is not): the slack it computed -- what
        ``fits``' padding rule needs -- stays and only grows with the rounding.  ``pair`` and ``second``: the largest count, plus the
        margin, rounded up to 8."""
        batches = list(batches)
        counts = [factored_batch_counts(b) for b in batches]
        base = StaticShapes.from_counts([{sp: c[sp] for sp in COUNT_FIELD} for c in counts], margin, heads, spread_sigmas)
        cap, slack = dict(base.cap), dict(base.slack)
        real = int(math.ceil(max(c["mol"] for c in counts) * (1.0 + margin)))
        cap["mol"] = _up(real + slack["mol"], 8)
        slack["mol"] = cap["mol"] - real
        room = {sp: _up(int(math.ceil(max(c[sp] for c in counts) * (1.0 + margin))), 8) for sp in PAIR_SPACES}
        shapes = cls(cap, slack, heads, base.lower, pair_cap=room["pair"], second_cap=room["second"])
        bounds = [getattr(b, "max_per_mol", None) for b in batches]
        if bounds and all(m is not None for m in bounds):
            shapes.max_per_mol = {sp: (1 if sp == "mol" else _up(int(1.5 * max(m[sp] for m in bounds)) + 8, 8)) for sp in SPACES}
        return shapes

    def capacity(self, space: str) -> int:
        return {"pair": self.pair_cap, "second": self.second_cap}[space] if space in PAIR_SPACES else self.cap[space]

    def fits(self, counts: Dict[str, int], max_per_mol: Optional[Dict[str, int]] = None) -> bool:
        """``counts`` of ``factored_batch_counts`` (the encoder's seven alone are accepted too: ``pad_batch`` asks with those)."""
        if counts.get("pair", 0) > self.pair_cap or counts.get("second", 0) > self.second_cap:
            return False
        return super().fits({sp: n for sp, n in counts.items() if sp not in PAIR_SPACES}, max_per_mol)

    def __repr__(self):
        return f"FactoredPairShapes(cap={self.cap}, slack={self.slack}, pair_cap={self.pair_cap}, second_cap={self.second_cap})"


def pad_factored_pair_batch(batch: Dict[str, torch.Tensor], shapes: FactoredPairShapes) -> Dict[str, torch.Tensor]:
    """``pad_batch`` of a factored pair batch, the torch counterpart of what FactoredPairGraphedTrainStep stages: the encoder's fields
    and masks padded over the U distinct drugs, ``y`` and the two pair lists with zeros up to ``pair_cap``, the second input's int64 rows
    with zero rows up to ``second_cap``, and ``plan.N_MOLS_KEY`` = the ``mol`` capacity.  The pair orderings are left out: the step builds
    them on the GPU from the staged lists."""
    from .data import PAIR_ORDER_KEYS
    from .plan import N_MOLS_KEY
    counts = factored_batch_counts(batch)
    if not shapes.fits(counts):
        raise ValueError(f"batch {counts} does not fit {shapes}")
    mols = {k: v for k, v in batch.items() if k not in FACTORED_PAIR_FIELDS and k not in PAIR_ORDER_KEYS and k != N_MOLS_KEY}
    mols["y"] = batch["y"].new_zeros(counts["mol"])          # pad_batch counts molecules by it; replaced below
    out = pad_batch(batch.like(mols) if isinstance(batch, CollatedBatch) else mols, shapes)
    for name, (space, _, _) in FACTORED_PAIR_FIELDS.items():
        if name in batch:
            src = batch[name]
            dst = src.new_zeros((shapes.capacity(space),) + tuple(src.shape[1:]))
            dst[: src.shape[0]] = src
            out[name] = dst
    out[N_MOLS_KEY] = shapes.cap["mol"]
    return out


ADAM_RIDER = os.environ.get("FRAGNET_ADAM_RIDER", "1") != "0"      # the head's Adam slice rides in the encoder backward's last launch (A/B: 0)


def masked_regr_loss(out: torch.Tensor, y: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """MSELoss()(out.view(-1), y) of train/utils.py:341 restricted to the molecules with weight 1."""
    if out.is_cuda:
        from . import ops
        return ops.masked_mse(out, y, w)              # loss + its gradient from one kernel
    d = out.reshape(w.shape[0], -1) - y.reshape(w.shape[0], -1)
    return (d * d * w[:, None]).sum() / (w.sum() * d.shape[1])


def masked_bce_loss(out: torch.Tensor, y: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """compute_bce_loss (train/utils.py:297-304): targets <= -0.5 are missing labels; padding molecules too."""
    if out.is_cuda:
        from . import ops
        return ops.masked_bce(out, y, w)
    y = y.reshape(out.shape)
    valid = (y > -0.5) & (w[:, None] > 0)
    mat = torch.nn.functional.binary_cross_entropy_with_logits(out, y.clamp(min=0.0), reduction="none")
    return torch.where(valid, mat, torch.zeros_like(mat)).sum() / valid.sum()


def masked_pretrain_loss(outputs, sb: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The reference's pretrain loss (pretrain_utils.py:9-31: 2*MSE(dihedral) + MSE(angle) + MSE(energy); the
    bond-length term is overwritten there before use) over a padded batch, with the rank weights of
    parallel.weighted_loss_scale applied to the per-edge and per-atom means."""
    from . import ops
    _, ba, da, graph_rep = outputs
    if da.is_cuda:       # 2 * sc0 * MSE(dihedral) + sc1 * MSE(angle) + MSE(energy) and its gradients: two launches
        return ops.masked_mse_multi([(2.0, 0), (1.0, 1), (1.0, -1)], sb[SCALE_KEY],
                                    da, sb["dh_angl"], sb[MASKS["edge"]], ba, sb["bnd_angl"], sb[MASKS["atom"]],
                                    graph_rep, sb["y"], sb[MASK_KEY])
    sc = sb[SCALE_KEY]
    l_dh = ops.masked_mse(da, sb["dh_angl"], sb[MASKS["edge"]]) * sc[0]
    return l_dh + ops.masked_mse(ba, sb["bnd_angl"], sb[MASKS["atom"]]) * sc[1] + l_dh \
        + ops.masked_mse(graph_rep, sb["y"], sb[MASK_KEY])


class StaticBatch:
    """Fixed-capacity device buffers for one batch + the single-launch staging call."""

    def __init__(self, shapes: StaticShapes, example: Dict[str, torch.Tensor], extra_fields: Optional[dict] = None, counts_of=None):
        """``extra_fields``: a table in FIELDS' form of fields staged behind FIELDS' own (PAIR_FIELDS for a pair model); an entry under one
        of FIELDS' names takes that field's place.  ``counts_of``: batch -> the real count of every index space a staged field lives in
        (``batch_counts`` when None)."""
        self._counts_of = counts_of or batch_counts
        dev = example["x_atoms"].device
        if dev.type != "cuda":
            raise _lib.FragnetHipError("StaticBatch stages batches on the GPU (fn_stage_padded); there is no CPU path")
        self.shapes, self.device = shapes, dev
        self._extra = dict(extra_fields or {})
        # the padded batch keeps the example's layout promise for its real molecules (the fused kernels treat the padding
        # molecules, whose items point round-robin at the reserved slots, separately: REAL_MOLS_KEY)
        self.collated = isinstance(example, CollatedBatch)
        self.t: Dict[str, torch.Tensor] = CollatedBatch() if self.collated else {}
        # per-molecule offsets table of the staged batch: drives the one-launch plan builder (fn_plan_build_mol)
        self.with_offsets = self.collated and example.offsets is not None and example.offsets.is_cuda and shapes.max_per_mol is not None
        if self.with_offsets:
            self.t.offsets = torch.zeros((len(SPACES), shapes.cap["mol"] + 1), dtype=torch.int32, device=dev)
            self.t.max_per_mol, self.t.pad = dict(shapes.max_per_mol), shapes.pad_info()
        # the staging table, in the launch's order: data fields (FIELDS order, then ``extra_fields``'), the three masks, the real-molecule count, the offsets table,
        # add_count's counts, then set_bumps' bumps and zero regions.  ``_refresh``: one entry per field that changes with the batch, all that
        # load() walks -- (the field, the index space whose real count is its n_real, its src: a batch key, _OFFSETS, or None)
        self._fields = (_lib.StageField * _lib.FN_MAX_STAGE_FIELDS)()
        self.n_fields = 0
        self._refresh = []
        for name, (space, layout, target) in {**FIELDS, **self._extra}.items():
            if name not in example:
                continue
            src, cap = example[name], shapes.capacity(space)
            if layout == "vec_i64":          # an int64 vector whose padding nobody reads: zeros behind the real entries
                if src.dtype != torch.int64 or src.dim() != 1:
                    raise TypeError(f"{name}: expected an int64 vector, got {src.dtype} {tuple(src.shape)}")
                self.t[name] = torch.zeros(cap, dtype=torch.int64, device=dev)
                self._append(_lib.STAGE_ROWS_I64, self.t[name].data_ptr(), cap, 1, refresh=(space, name))
            elif layout == "rows_i64":
                if src.dtype != torch.int64 or src.dim() != 2:
                    raise TypeError(f"{name}: expected int64 rows [n, width], got {src.dtype} {tuple(src.shape)}")
                self.t[name] = torch.zeros((cap, src.shape[1]), dtype=torch.int64, device=dev)
                self._append(_lib.STAGE_ROWS_I64, self.t[name].data_ptr(), cap, int(src.shape[1]), refresh=(space, name))
            elif layout == "rows":
                if src.dtype != torch.float32:
                    raise TypeError(f"{name}: expected float32 rows, got {src.dtype}")
                self.t[name] = torch.zeros((cap,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
                width = int(src[0].numel()) if src.dim() > 1 else 1
                self._append(_lib.STAGE_ROWS, self.t[name].data_ptr(), cap, max(width, 1), refresh=(space, name))
            else:
                if src.dtype != torch.int64:
                    raise TypeError(f"{name}: expected int64 indices, got {src.dtype}")
                hi, mod = shapes.pad_rule(target)
                self.t[name] = torch.zeros((cap,) if layout == "ids" else (2, cap), dtype=torch.int64, device=dev)
                self._append(_lib.STAGE_IDS if layout == "ids" else _lib.STAGE_COLS, self.t[name].data_ptr(), cap, pad_hi=hi, pad_mod=mod,
                             refresh=(space, name))
        for space, key in MASKS.items():
            self.t[key] = torch.zeros(shapes.cap[space], dtype=torch.float32, device=dev)
            self._append(_lib.STAGE_MASK, self.t[key].data_ptr(), shapes.cap[space], refresh=(space, None))
        self.t[SCALE_KEY] = torch.ones(2, dtype=torch.float32, device=dev)
        # device-side copy of the number of real molecules: the fused encoder kernels skip the padding behind them
        self.t[REAL_MOLS_KEY] = torch.zeros(1, dtype=torch.int32, device=dev)
        self._append(_lib.STAGE_COUNT, self.t[REAL_MOLS_KEY].data_ptr(), 1, refresh=("mol", None))
        if self.with_offsets:
            self._append(_lib.STAGE_OFFSETS, self.t.offsets.data_ptr(), shapes.cap["mol"], len(SPACES), refresh=("mol", _OFFSETS))
        # molecule rows behind capacity - slack are padding in every batch that fits: the prediction head skips them
        self.t[LIVE_MOLS_KEY] = shapes.cap["mol"] - shapes.slack["mol"]
        self.counts: Optional[Dict[str, int]] = None
        self._n_static = self.n_fields       # set_bumps rewinds to here

    def _append(self, kind, dst, cap, width=1, pad_hi=0, pad_mod=1, src=None, n_real=0, refresh=None) -> int:
        """Fill the next entry of the staging table; its index.  ``refresh`` = (space, src source): load() rewrites n_real and src."""
        if self.n_fields >= _lib.FN_MAX_STAGE_FIELDS:
            raise ValueError(f"too many batch fields for one staging launch (its table holds FN_MAX_STAGE_FIELDS = {_lib.FN_MAX_STAGE_FIELDS})")
        i, f = self.n_fields, self._fields[self.n_fields]
        f.src, f.dst, f.n_real, f.cap, f.width, f.kind, f.pad_hi, f.pad_mod = src, dst, n_real, cap, width, kind, pad_hi, pad_mod
        if refresh is not None:
            self._refresh.append((f,) + refresh)
        self.n_fields += 1
        return i

    def add_count(self, space: str, key: str) -> torch.Tensor:
        """One more device-side count written by the staging launch: ``self.t[key]`` = int32 [1], the number of REAL rows of ``space``
        in the staged batch (the masked-atom sampler reads the real atom count there).  Before set_bumps."""
        if self.n_fields != self._n_static:
            raise RuntimeError("add_count comes before set_bumps")
        self.t[key] = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._n_static = self._append(_lib.STAGE_COUNT, self.t[key].data_ptr(), 1, refresh=(space, None)) + 1
        return self.t[key]

    def set_bumps(self, bumps, zeros=()):
        """Extra work of the staging launch in front of every replay of a captured step.  ``bumps`` = [(int64 device tensor
        [1], increment)]: counters it advances (FN_STAGE_BUMP: the step's Philox block counter and optimiser step count);
        ``zeros`` = [(device pointer, int32 count)]: workspaces it zeroes (FN_STAGE_ZERO: those of the plans built inside the
        graph).  The graph then needs no launch of its own for either."""
        self.n_fields = self._n_static
        for t, inc in bumps:
            self._append(_lib.STAGE_BUMP, t.data_ptr(), 1, n_real=int(inc))
        for ptr, n in zeros:
            self._append(_lib.STAGE_ZERO, int(ptr), int(n))

    def load(self, batch: Dict[str, torch.Tensor]) -> bool:
        """Stage ``batch`` (GPU tensors); False when it does not fit the capacities (nothing is written then)."""
        counts = self._counts_of(batch)
        if not self.shapes.fits(counts, getattr(batch, "max_per_mol", None)):
            return False
        if self.collated and not isinstance(batch, CollatedBatch):
            return False        # no layout promise: the caller's eager step takes the general kernels
        off = batch.offsets if self.with_offsets else None
        if self.with_offsets:
            if off is None or not off.is_cuda or batch.max_per_mol is None:
                return False
            off = off if off.is_contiguous() else off.contiguous()
        keep = [off]            # alive until the launch has run
        for f, space, key in self._refresh:
            if key is _OFFSETS:
                f.src = off.data_ptr()
            elif key is not None:
                src = batch[key]
                if not src.is_cuda:
                    raise _lib.FragnetHipError(f"{key} must live on the GPU to be staged (got {src.device})")
                if key in self._extra and tuple(src.shape[1:]) != tuple(self.t[key].shape[1:]):
                    raise ValueError(f"{key}: rows of {tuple(src.shape[1:])}, the captured step was built for {tuple(self.t[key].shape[1:])}")
                if not src.is_contiguous():
                    src = src.contiguous()
                    keep.append(src)
                f.src = src.data_ptr()
            f.n_real = counts[space]
        _lib.call("fn_stage_padded", self._fields, self.n_fields, torch.cuda.current_stream(self.device).cuda_stream)
        self.counts, self._keep = counts, keep
        return True


def _warm_up(device, fn, warmup: int):
    """``fn`` ``warmup`` times on a side stream (a capture must not be the first run of anything), joined and finished."""
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)


class ReplayCounter:
    """One Philox stream inside a captured step: the stream, its device word (``word``: int64 [1], added by the kernels to every offset
    they are handed), the host offset the capture started from (``base``: the offsets baked into the graph count from it), the blocks
    one step draws (``per_step``, fixed by the static shapes) and whether the staging launch in front of every replay moves the word on
    (``staged``: the single-graph step; the two-graph step advances the word inside its first graph).

    Invariant: between replays the device counter is ONE STEP BEHIND when ``staged`` is set -- the staging launch in front of every
    replay moves it on, which is why it starts at -per_step: the first replay sees 0 -- so anything that replays without staging (or
    stages without replaying) must go through GraphedTrainStep.replay(), and a step that runs outside the graph goes through eager()."""

    def __init__(self, stream, word: torch.Tensor, what: str = "Philox"):
        self.stream, self.word, self.what = stream, word, what
        stream.dev = word
        self.base, self.per_step, self.staged = 0, 0, False

    def mark(self):
        self.base = self.stream.offset           # a warm-up step, or the capture, starts here

    def drawn(self) -> int:
        return self.stream.offset - self.base

    def measure(self):
        self.per_step = self.drawn()             # a warm-up step that began at mark() has run: every step draws what it drew

    def check(self):
        if self.drawn() != self.per_step:
            raise RuntimeError(f"the captured step drew a different number of {self.what} blocks than the warm-up steps")

    def stage(self):
        """The staging launch moves the word from now on: its (tensor, increment) bump entry, or None for a step that draws nothing."""
        self.staged = True
        if not self.per_step:
            return None
        self.word -= self.per_step
        return self.word, self.per_step

    @staticmethod
    @contextlib.contextmanager
    def eager(*counters: "ReplayCounter"):
        """Around a step that runs outside the graph: it draws from the base offsets the captured step has baked in -- the word, which the
        eager kernels add as well, makes them this step's own -- and afterwards the word has moved past all it drew: fallback steps and
        replays never share Philox blocks.  The host offsets come back as they were.  Several counters: each half in the order given."""
        held = [(c, c.stream.offset, c.per_step if c.staged else 0) for c in counters]      # (.., host offset, blocks the word is behind)
        for c, _, behind in held:
            c.stream.offset = c.base
            if behind:                           # the staging launch would have moved it on
                c.word += behind
        yield
        for c, after, behind in held:
            if c.drawn() - behind:
                c.word += c.drawn() - behind
            c.stream.offset = after


class GraphedTrainStep:
    """zero_grad + forward + loss + backward + gradient gather as one hipGraph; all-reduce + Adam after it.

    ``model``: FragNetFineTune / FragNetPreTrain (fragnet_amd.model) in train mode; ``opt``: parallel.FlatAdam over its
    live parameters; ``loss``: "regr" (MSE, train/utils.py:341), "clsf" (masked BCE, train/utils.py:297) or "pretrain"
    (pretrain_utils.py:9-31 on the collate_fn_pt batch).
    """

    LOSS_KINDS = ("regr", "clsf", "pretrain")
    EXTRA_FIELDS: Optional[dict] = None      # StaticBatch's ``extra_fields``
    COUNTS_OF = staticmethod(batch_counts)   # StaticBatch's ``counts_of``

    def __init__(self, model, opt, shapes: StaticShapes, example: Dict[str, torch.Tensor], loss: str = "regr",
                 group=None, warmup: int = 3, overlap: Optional[bool] = None, capture_adam: bool = True,
                 force_distributed: bool = False):
        """``overlap=True``: capture the step as TWO graphs -- (forward + loss + head backward) and (encoder backward) -- and
        start an asynchronous all-reduce of the head's gradients (83 % of the bytes for FTHead3) between them, so that it
        runs on RCCL's stream beside the encoder's backward pass; the encoder's own, small slice follows the second graph.
        Off by default: on this stack an async collective costs ~95 us of stream fork/join against ~20 us for a blocking
        one (tools/allreduce_probe.py), which eats what the overlap hides at 8 MB of gradients (DESIGN.md section 7 and HISTORY.md section 7)."""
        self.model, self.opt, self.shapes, self.group = model, opt, shapes, group
        # force_distributed: run the N>1 step sequence (graph replay -> RCCL all-reduce -> Adam outside the graph, rank loss
        # weights through an all-reduce) even in a 1-rank process group, so that one GPU can test it
        self.force_distributed = bool(force_distributed)
        if self.force_distributed:
            opt.force_collective = True
        self.loss_kind = loss
        if loss not in self.LOSS_KINDS:
            raise ValueError(f"unknown loss kind {loss!r}")
        self._masked = {"regr": masked_regr_loss, "clsf": masked_bce_loss}.get(loss)
        self.static = StaticBatch(shapes, example, self.EXTRA_FIELDS, self.COUNTS_OF)
        self.device = self.static.device
        self._extend_static()
        if loss == "pretrain" and "dh_angl" not in example:
            raise ValueError("pretrain step needs the collate_fn_pt batch (bnd_lngth, bnd_angl, dh_angl)")
        if loss == "pretrain" and hasattr(getattr(model, "head", None), "need_bond_length"):
            model.head.need_bond_length = False      # the loss never reads the bond-length prediction (pretrain_utils.py:17-24)
        self.rng = self._encoder().rng
        # [Philox blocks consumed, Adam steps done]: the staging launch in front of every replay moves both on (FN_STAGE_BUMP).  The first
        # word is the dropout stream's (``rng.dev``), the second the step count the captured Adam reads (_sync_adam_state)
        self._counters = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.rng_counter = ReplayCounter(self.rng, self._counters[0:1])
        import torch.distributed as dist
        # the ranks exchange gradients and loss weights: more than one of them, or a 1-rank group made to (force_distributed)
        self._distributed = dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or self.force_distributed)
        # one rank, fused HIP Adam: the update is captured too (step count and learning rate live in device memory)
        self.adam_in_graph = bool(capture_adam) and not self._distributed and not self.force_distributed and getattr(opt, "opt", 1) is None
        self._lr_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._lr_host, self._dev_steps = None, -1
        self.graph = self.graph_b = None             # torch.cuda.CUDAGraph: the step; the encoder backward of a two-graph step
        self.loss: Optional[torch.Tensor] = None
        self.replays = self.fallbacks = 0
        # a masked-atom model (FragNetPreTrainMasked2) draws its row mask inside the step, from a stream of its own: the sampler launch is
        # captured behind the staging / plan launches, reads the real atom count the staging launch writes, and its device word is kept
        # exactly like the dropout stream's (a second ReplayCounter)
        self.mask_rng = getattr(model, "mask_rng", None) if loss == "pretrain" else None
        self.mask_counter: Optional[ReplayCounter] = None
        self.keep_mask: Optional[torch.Tensor] = None      # the latest step's mask (uint8 [atom capacity]): a persistent buffer, for tests and tools
        if self.mask_rng is not None:
            self.mask_counter = ReplayCounter(self.mask_rng, torch.zeros(1, dtype=torch.int64, device=self.device), "mask")
            self.static.add_count("atom", REAL_ATOMS_KEY)
            self.keep_mask = model.keep_buffer = torch.ones(shapes.cap["atom"], dtype=torch.uint8, device=self.device)
        self._stream_counters = [c for c in (self.rng_counter, self.mask_counter) if c is not None]      # dropout first: the order of their launches
        from . import ops
        self._unit = ops.unit_grad(self.static.device)
        self.head_off = self._head_offset()
        self.split = bool(overlap) and self.head_off is not None
        self._rider_lo: Optional[int] = None         # set by the warm-up steps of _capture: where the Adam slice that may ride starts
        self._capture(example, warmup)

    # -- pieces
    def _extend_static(self):
        """What a subclass stages beyond the field tables (``StaticBatch.add_count``, buffers of its own in ``static.t``); before the capture."""

    def _encoder(self):
        """The FragNet encoder whose dropout stream the step owns."""
        return self.model.pretrain

    def _stage(self, batch) -> bool:
        """Stage ``batch`` for a replay; False: it takes the eager step (nothing was written)."""
        return self.static.load(batch)

    def _head_offset(self) -> Optional[int]:
        """Offset of the head's parameters in the optimiser's flat buffer if they are its contiguous tail (model =
        encoder ``pretrain`` + ``fthead``, regression / classification loss), else None (single-graph step)."""
        head = getattr(self.model, "fthead", None)
        if self.loss_kind == "pretrain" or head is None or not hasattr(self.model, "pretrain"):
            return None
        ids = {id(p) for p in head.parameters()}
        first = None
        for p, off in zip(self.opt.params, self.opt.offsets):
            if id(p) in ids:
                if first is None:
                    first = off
            elif first is not None:
                return None                                  # an encoder parameter after a head parameter
        return first

    def _head_grads_in_place(self) -> bool:
        base, es, ids = self.opt.grad.data_ptr(), self.opt.grad.element_size(), {id(p) for p in self.model.fthead.parameters()}
        for p, off in zip(self.opt.params, self.opt.offsets):
            if id(p) in ids and (p.grad is None or p.grad.data_ptr() != base + off * es):
                return False
        return True

    def _static_loss(self, predict):
        """The staged batch without a plan (every step builds its own, inside the graph) -> ``predict(batch)`` -> the loss.  A
        predictor-stack head is told the targets first (``loss_spec``): its last Linear, the loss and that Linear's backward then
        share one launch (ops.mlp_head) and the predictions come back with the loss attached; every other head, and a stack the
        fused launch does not cover, goes through the loss kernel of its own."""
        sb = self.static.t
        sb.pop(PLAN_KEY, None)
        if self.loss_kind == "pretrain":            # single-graph step only: a pretrain model has no head to split at
            return masked_pretrain_loss(predict(sb), sb)
        y, w, head = sb["y"], sb[MASK_KEY], getattr(self.model, "fthead", None)
        armed = head is not None and hasattr(head, "loss_spec") and y.is_cuda
        if armed:
            head.loss_spec = (_lib.LOSS_MSE if self.loss_kind == "regr" else _lib.LOSS_BCE, y, w)
        try:
            out = predict(sb)
        finally:
            if armed:
                head.loss_spec = None
        fused = getattr(out, "_fragnet_loss", None)
        if fused is not None and fused[1] is y and fused[2] is w:
            return fused[0]
        return self._masked(out, y, w)

    def _part_a(self):
        """forward, loss, and the backward pass of loss + head; leaves d loss / d pooled in ``leaf.grad``."""
        from .model import _KEEP_EDGE_OUTPUTS, pooled
        pooled_t = leaf = None

        def head_on_leaf(sb):
            nonlocal pooled_t, leaf
            x_atoms, x_frags, _, _ = self.model.pretrain(sb, edge_outputs=_KEEP_EDGE_OUTPUTS)
            pooled_t = pooled(x_atoms, x_frags, sb)
            leaf = pooled_t.detach().requires_grad_(True)
            self.model.fthead.live_rows = sb.get(LIVE_MOLS_KEY)
            return self.model.fthead(leaf)
        loss = self._static_loss(head_on_leaf)
        loss.backward(gradient=self._unit)
        return loss, pooled_t, leaf

    def _part_b(self, pooled_t, leaf):
        pooled_t.backward(leaf.grad)
        self.opt.gather_grads()

    def _fwd_bwd_static(self, ride_adam: bool = False):
        """forward, loss, backward, gradients gathered.  ``ride_adam`` (the captured single-graph step with Adam inside): the
        head's slice of the Adam update -- its gradients are complete once the head's backward has run -- rides in the encoder
        backward's last launch; returns (loss, first element of the flat buffer that rode, or None)."""
        loss = self._static_loss(self.model)
        rode = None
        if ride_adam and ADAM_RIDER and self._rider_lo is not None:
            from . import engine
            keep = self.opt.adam_slice(self._counters[1:2], self._lr_dev, self._rider_lo)
            engine.arm_adam_rider(keep)
            try:
                loss.backward(gradient=self._unit)
            finally:
                if engine.adam_rider_taken():
                    rode = self._rider_lo
        else:
            loss.backward(gradient=self._unit)      # persistent 1.0: no fill launch, masked_mse skips the multiply
        self.opt.gather_grads()
        return loss, rode

    def _capture(self, example, warmup: int):
        if not self.model.training:
            raise RuntimeError("GraphedTrainStep captures a TRAINING step: call model.train() first")
        if not self._stage(example):
            raise ValueError(f"the example batch {self.COUNTS_OF(example)} does not fit {self.shapes}")

        def warm_step():
            self.opt.zero_grad()
            for c in self._stream_counters:
                c.mark()
            if self.split:
                _, pooled_t, leaf = self._part_a()
                if not self._head_grads_in_place():      # e.g. a non-ReLU head (torch's own backward): one graph
                    self.split = False
                self._part_b(pooled_t, leaf)
            else:
                self._fwd_bwd_static()
                # may the head's Adam slice ride in the encoder's backward?  Only if its gradients sit in the flat buffer already
                # when that backward starts (the fused head writes them there) and its parameters are the buffer's tail
                off = self._head_offset()
                self._rider_lo = off if (off is not None and off % 4 == 0 and self._head_grads_in_place()) else None
            for c in self._stream_counters:
                c.measure()                              # Philox blocks one step draws (fixed by the static shapes)
        _warm_up(self.device, warm_step, warmup)
        self.opt.zero_grad()
        if self.split:
            self.adam_in_graph = False
        self._sync_adam_state()
        graph = torch.cuda.CUDAGraph()
        for c in self._stream_counters:
            c.mark()
        if self.split:
            pool = torch.cuda.graph_pool_handle()
            with torch.cuda.graph(graph, pool=pool, capture_error_mode=_CAPTURE_MODE):
                loss, pooled_t, leaf = self._part_a()
                consumed = self.rng_counter.drawn()
                if consumed:
                    self.rng.advance_device(consumed)
            self.graph_b = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_b, pool=pool, capture_error_mode=_CAPTURE_MODE):
                self._part_b(pooled_t, leaf)
            del pooled_t, leaf
        else:
            # plans built inside the capture skip their zeroing launch: the staging launch zeroes their workspaces (below)
            with prezeroed_plans() as pz, torch.cuda.graph(graph, capture_error_mode=_CAPTURE_MODE):
                loss, rode = self._fwd_bwd_static(ride_adam=self.adam_in_graph)
                for c in self._stream_counters:
                    c.check()
                # fresh dropout masks and the next Adam step number on every replay: the staging launch in front of the replay
                # advances the counters (FN_STAGE_BUMP), so the graph has no launch of its own for them
                if self.adam_in_graph:
                    self.opt.adam_in_graph(self._counters[1:2], self._lr_dev, 0, rode)      # what did not ride in the backward
            bumps = [c.stage() for c in self._stream_counters]
            if self.adam_in_graph:
                bumps.insert(1, (self._counters[1:2], 1))        # the table's order: dropout blocks, Adam steps, mask blocks
            self._captured_plans = pz.plans          # keep their arenas (the regions below) alive with the graph
            self.static.set_bumps([b for b in bumps if b is not None], zeros=[r for plan in pz.plans for r in plan.zero_regions])
        self.graph, self.loss = graph, loss.detach()

    def _sync_adam_state(self):
        """Device copies of the optimiser's step count and learning rate follow the host values (an eager fallback step,
        a scheduler or a restored checkpoint may have moved them)."""
        if not self.adam_in_graph:
            return
        if self._dev_steps != self.opt.steps:
            self._counters[1:2].fill_(self.opt.steps)
            self._dev_steps = self.opt.steps
        lr = float(self.opt.hyper["lr"])
        if self._lr_host != lr:
            self._lr_dev.fill_(lr)
            self._lr_host = lr

    def _rank_scales(self, batch) -> Optional[torch.Tensor]:
        """(per-edge, per-atom) loss weights local_count * world / global_count as a device tensor (no host sync)."""
        if self.loss_kind != "pretrain" or not self._distributed:
            return None
        import torch.distributed as dist
        local = torch.tensor([float(batch["dh_angl"].shape[0]), float(batch["bnd_angl"].shape[0])], device=self.device)
        total = local.clone()
        dist.all_reduce(total, op=dist.ReduceOp.SUM, group=self.group)
        return (local * dist.get_world_size(self.group) / total).to(torch.float32)

    def _eager_loss(self, batch):
        if self.loss_kind == "pretrain":
            from .train import pretrain_loss
            sc = self._rank_scales(batch)
            return pretrain_loss(self.model(batch), batch, (1.0, 1.0) if sc is None else (sc[0], sc[1]))
        out = self.model(batch)
        w = torch.ones(batch["y"].shape[0], dtype=torch.float32, device=out.device)
        return self._masked(out, batch["y"], w)

    def _eager(self, batch):
        self.opt.zero_grad()
        with ReplayCounter.eager(*self._stream_counters):
            loss = self._eager_loss(batch)
            loss.backward()
            if self.split:
                # the ranks that replay the two graphs issue two slice all-reduces (head, then encoder): a rank that fell back to
                # the eager step must issue the same collectives, in the same order and sizes
                self.opt.gather_grads()
                self.opt.all_reduce_slice(self.head_off, None, self.group)
                self.opt.all_reduce_slice(0, self.head_off, self.group)
                self.opt.apply_gathered(self.group, reduced=True)
            else:
                self.opt.step(self.group)
        return loss.detach()

    def _count_adam_step(self):      # the update ran inside the graph: the host's counts follow the device word the staging launch moved
        self.opt.steps += 1
        self._dev_steps += 1

    def replay(self, batch: Dict[str, torch.Tensor]) -> bool:
        """Stage ``batch`` and replay the captured graph(s) -- always as a pair: the staging launch zeroes the plan workspaces
        and advances the Philox / step counters the graph reads.  No collective, no optimiser step outside the graph (tools
        that time or profile the captured part use this instead of ``static.load`` + ``graph.replay``).  False: the batch does
        not fit the capacities (nothing ran)."""
        self._sync_adam_state()
        if not self._stage(batch):
            return False
        self.graph.replay()
        if self.graph_b is not None:
            self.graph_b.replay()
        if self.adam_in_graph:
            self._count_adam_step()
        self.replays += 1
        return True

    def __call__(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """One optimiser step on ``batch``.  Returns the loss (a tensor that the next call overwrites)."""
        self._sync_adam_state()                      # before the staging launch: it bumps the step counter
        if not self._stage(batch):
            self.fallbacks += 1
            return self._eager(batch)
        sc = self._rank_scales(batch)
        if sc is not None:
            self.static.t[SCALE_KEY].copy_(sc)
        self.graph.replay()
        if self.adam_in_graph:
            self._count_adam_step()
        elif self.split:
            head = self.opt.all_reduce_slice(self.head_off, None, self.group, async_op=True)     # beside graph_b
            self.graph_b.replay()
            rest = self.opt.all_reduce_slice(0, self.head_off, self.group, async_op=True)
            for work in (head, rest):
                if work is not None:
                    work.wait()                     # stream-side wait, the host does not block
            self.opt.apply_gathered(self.group, reduced=True)
        else:
            self.opt.apply_gathered(self.group)
        self.replays += 1
        return self.loss


class PairGraphedTrainStep(GraphedTrainStep):
    """``GraphedTrainStep`` for a pair model (cdrp.CDRPModel, dta.DTAModel2) on the one-record-per-pair batches of
    ``data.collate_fn_cdrp`` / ``data.collate_fn_dta``: encoder, second-input tower, pair head with its fused MSE, backward, gradient
    gather and (one rank, fused Adam) the update as ONE hipGraph.  What differs from the property step, and nothing else:

    * staged fields: FIELDS' sixteen encoder fields and ``y``, plus ``gene_expr`` / ``protein`` (PAIR_FIELDS: int64 rows in the ``mol``
      space, zero rows behind the real ones);
    * the encoder is ``model.drug_model.pretrain``: its Philox stream is the step's ``ReplayCounter``;
    * the step is ``model(staged, loss=(LOSS_MSE, y, None, real-row word))``: the pair head's fused launch reads the count the staging
      launch wrote (plan.REAL_MOLS_KEY), takes the mean over the real pairs and hands the padding rows a zero gradient, so the tower
      and the encoder see none either.  Padding molecules and padding rows of the tower are computed, not skipped;
    * ``target_norm = (mean, sdev)`` (the DTA trainer sets it, per call): what is staged as ``y`` is ``(y - mean) / (sdev + 1e-5)``,
      computed in front of the staging launch -- the graph never sees the two numbers, so they may change between calls;
    * a factored batch (it carries ``data.PAIR_DRUG_KEY``), a grid batch and a batch beyond the capacities take the eager step on the
      same optimiser and RNG state (``fallbacks``).  A grid batch has no target: its eager step raises.

    Single graph and single rank only: ``overlap=True`` and a process group of more than one rank raise ValueError."""

    LOSS_KINDS = ("pair",)
    EXTRA_FIELDS = PAIR_FIELDS

    def __init__(self, model, opt, shapes: StaticShapes, example: Dict[str, torch.Tensor], group=None, warmup: int = 3,
                 overlap: Optional[bool] = None, capture_adam: bool = True):
        who = type(self).__name__
        if overlap:
            raise ValueError(f"{who} captures one graph: overlap=True (the two-graph step) is not built for pair models")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            raise ValueError(f"{who} is single-GPU: the process group has more than one rank")
        if not hasattr(getattr(model, "drug_model", None), "pretrain"):
            raise TypeError(f"{who} takes a pair model (cdrp.CDRPModel / dta.DTAModel2): model.drug_model.pretrain is its encoder")
        if not any(k in example for k in PAIR_FIELDS):
            raise ValueError(f"the example is no pair batch: none of {tuple(PAIR_FIELDS)} in it")
        self.target_norm = None                      # None: y as the batch has it; (mean, sdev): (y - mean) / (sdev + 1e-5)
        self._y_keep = None
        super().__init__(model, opt, shapes, example, loss="pair", group=group, warmup=warmup, overlap=False, capture_adam=capture_adam)

    def _encoder(self):
        return self.model.drug_model.pretrain

    def _target(self, batch) -> torch.Tensor:
        if self.target_norm is None:
            return batch["y"]
        mean, sdev = self.target_norm
        return (batch["y"] - mean) / (sdev + 1e-5)           # trainer_dta.py:42, the statement of TrainerFineTuneDTA._loss

    @staticmethod
    def _one_row_per_pair(batch) -> bool:
        from .data import PAIR_DRUG_KEY, PAIR_GRID_KEY
        return PAIR_DRUG_KEY not in batch and not batch.get(PAIR_GRID_KEY)

    def _stage(self, batch) -> bool:
        if not self._one_row_per_pair(batch):
            return False
        if self.target_norm is not None:
            staged = batch.like(dict(batch)) if isinstance(batch, CollatedBatch) else dict(batch)
            staged["y"] = self._y_keep = self._target(batch)     # alive until the next call: the staging launch reads it
            batch = staged
        return self.static.load(batch)

    def _static_loss(self, predict):
        sb = self.static.t
        sb.pop(PLAN_KEY, None)
        _, loss = predict(sb, loss=(_lib.LOSS_MSE, sb["y"], None, sb[REAL_MOLS_KEY]))
        return loss              # never None: ops._pair_apply refuses a count where the fused launch does not apply

    def _eager_loss(self, batch):
        from .data import PAIR_GRID_KEY
        if batch.get(PAIR_GRID_KEY):
            raise ValueError("a grid batch has no target and no training step")
        y = self._target(batch)
        out, loss = self.model(batch, loss=(_lib.LOSS_MSE, y, None))
        return loss if loss is not None else torch.nn.functional.mse_loss(out.view(-1), y)


class FactoredPairGraphedTrainStep(PairGraphedTrainStep):
    """``PairGraphedTrainStep`` on FACTORED batches (``data.collate_fn_cdrp_factored`` / ``collate_fn_dta_factored``): the encoder on the
    U distinct drugs, the second tower on the C distinct rows, the pair orderings (``ops.pair_orderings_both``: one launch, no host
    read), the factored pair head with its fused MSE, backward, gradient gather and the update as ONE hipGraph.  ``shapes``: a
    ``FactoredPairShapes``.  What differs from the sibling:

    * staged fields: FIELDS' encoder fields in their own spaces (``mol`` = the distinct drugs), and FACTORED_PAIR_FIELDS: ``y`` and the two
      pair lists in the ``pair`` space, ``gene_expr`` / ``protein`` in the ``second`` space, zeros behind the real entries; two device
      counts, the real molecules (plan.REAL_MOLS_KEY) and the real pairs (REAL_PAIRS_KEY).  One staging launch; a table beyond
      FN_MAX_STAGE_FIELDS raises;
    * the staged batch carries ``plan.N_MOLS_KEY`` = the ``mol`` capacity and four persistent ordering buffers (``data.PAIR_ORDER_KEYS``)
      that the orderings launch fills under the real-pair count: a padding pair is in no segment, so the head's backward needs no count
      (csrc/pair_factored.hip) and padding rows of both towers receive exact zeros;
    * the step is ``model(staged, loss=(LOSS_MSE, y, None, real-pair word))``; the forward's 4-byte memset of its arrival counter is
      captured as a memset node;
    * a one-record-per-pair batch is accepted: it is staged (and, beyond the capacities, run eagerly) through ``data.as_factored``;
    * a grid batch and a batch beyond any capacity -- ``mol``, ``pair``, ``second`` or an encoder space -- take the eager factored step
      on the same optimiser and Philox state (``fallbacks``); a grid batch has no target: its eager step raises."""

    EXTRA_FIELDS = FACTORED_PAIR_FIELDS
    COUNTS_OF = staticmethod(factored_batch_counts)

    def __init__(self, model, opt, shapes: FactoredPairShapes, example: Dict[str, torch.Tensor], group=None, warmup: int = 3,
                 overlap: Optional[bool] = None, capture_adam: bool = True):
        from . import ops
        from .data import PAIR_GRID_KEY
        if not isinstance(shapes, FactoredPairShapes):
            raise TypeError("FactoredPairGraphedTrainStep takes FactoredPairShapes (capacities of the pair and second spaces too)")
        if example.get(PAIR_GRID_KEY):
            raise ValueError("a grid batch has no target and no training step")
        over = {k: v for k, v in (("mol", shapes.cap["mol"]), ("pair", shapes.pair_cap), ("second", shapes.second_cap)) if v > ops.DENSE_MAX_ROWS}
        if over:
            raise ValueError(f"FactoredPairGraphedTrainStep: capacities {over} are beyond the factored pair head's {ops.DENSE_MAX_ROWS} rows")
        super().__init__(model, opt, shapes, self._factored(example), group=group, warmup=warmup, overlap=overlap, capture_adam=capture_adam)

    @staticmethod
    def _factored(batch):
        from .data import PAIR_DRUG_KEY, as_factored
        return batch if PAIR_DRUG_KEY in batch else as_factored(batch)

    def _extend_static(self):
        from .data import PAIR_ORDER_KEYS
        from .plan import N_MOLS_KEY
        st, sh = self.static, self.shapes
        st.add_count("pair", REAL_PAIRS_KEY)
        sizes = (sh.cap["mol"] + 1, sh.pair_cap, sh.second_cap + 1, sh.pair_cap)
        for key, n in zip(PAIR_ORDER_KEYS, sizes):
            st.t[key] = torch.zeros(n, dtype=torch.int32, device=st.device)
        st.t[N_MOLS_KEY] = sh.cap["mol"]

    def _stage(self, batch) -> bool:
        from .data import PAIR_GRID_KEY
        if batch.get(PAIR_GRID_KEY):
            return False
        batch = self._factored(batch)
        if self.target_norm is not None:
            staged = batch.like(dict(batch)) if isinstance(batch, CollatedBatch) else dict(batch)
            staged["y"] = self._y_keep = self._target(batch)     # alive until the next call: the staging launch reads it
            batch = staged
        return self.static.load(batch)

    def _static_loss(self, predict):
        from . import ops
        from .data import PAIR_DRUG_KEY, PAIR_ORDER_KEYS, PAIR_SECOND_KEY
        sb = self.static.t
        sb.pop(PLAN_KEY, None)
        ops.pair_orderings_both(sb[PAIR_DRUG_KEY], sb[PAIR_SECOND_KEY], self.shapes.cap["mol"], self.shapes.second_cap,
                                real_pairs=sb[REAL_PAIRS_KEY], out=tuple(sb[k] for k in PAIR_ORDER_KEYS))
        _, loss = predict(sb, loss=(_lib.LOSS_MSE, sb["y"], None, sb[REAL_PAIRS_KEY]))
        return loss              # never None: ops._pair_apply refuses a count where the fused launch does not apply

    def _eager_loss(self, batch):
        from .data import PAIR_GRID_KEY
        return super()._eager_loss(batch if batch.get(PAIR_GRID_KEY) else self._factored(batch))


class GraphedForward:
    """Inference counterpart of GraphedTrainStep: stage + plan build + ``model(batch)`` (eval mode, no autograd) as one
    hipGraph over static shapes.  ``__call__`` returns the predictions of the real molecules (a view of a buffer the next
    call overwrites); batches beyond the capacities run eagerly.  Useful when the host is the bottleneck (small batches,
    busy CPU); on an idle host the eager forward is already GPU-bound and the staging copy makes this path 5-10 % slower
    (745 k vs 784 k molecules/s at 512 molecules, 1.15 M vs 1.27 M at 8192), so bench.py's forward sweep stays eager."""

    def __init__(self, model, shapes: StaticShapes, example: Dict[str, torch.Tensor], warmup: int = 2):
        if model.training:
            raise RuntimeError("GraphedForward captures an inference pass: call model.eval() first")
        self.model, self.shapes = model, shapes
        self.static = StaticBatch(shapes, example)
        self.device = self.static.device
        self.replays = self.fallbacks = 0
        if not self.static.load(example):
            raise ValueError(f"the example batch {batch_counts(example)} does not fit {self.shapes}")
        with torch.no_grad():
            _warm_up(self.device, self._run, warmup)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode=_CAPTURE_MODE):
            self.out = self._run()

    def _run(self):
        sb = self.static.t
        sb.pop(PLAN_KEY, None)
        return self.model(sb)

    def __call__(self, batch: Dict[str, torch.Tensor]):
        n = batch[COUNT_FIELD["mol"]].shape[0] if COUNT_FIELD["mol"] in batch else int(batch["batch"].max()) + 1
        if not self.static.load(batch):
            self.fallbacks += 1
            batch.pop(PLAN_KEY, None)
            with torch.no_grad():
                return self.model(batch)
        self.graph.replay()
        self.replays += 1
        out = self.out
        return tuple(o[:n] if torch.is_tensor(o) and o.shape[0] == self.shapes.cap["mol"] else o for o in out) \
            if isinstance(out, tuple) else out[:n]

