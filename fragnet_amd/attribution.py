"""Leave-one-out attributions on the engine: the reference's masking interpretability (fragnet/vizualize/viz.py:
``calc_atom_contributions``, ``calc_bond_contributions``, ``calc_fbond_contributions``, ``get_all_contributions``) as batched
evaluation passes.

The reference zeroes the rows of ONE atom, bond or fragment connection in every layer of a deep copy of the model, predicts a
batch of one again and reports ``pred_no_mask - pred_mask``: one forward per element, ~57 for a 26-atom molecule.  Here every
masked replica of every molecule is a molecule of an ordinary evaluation batch: the replica list is collated with repeated
molecule indices, one launch (fn_loo_row_masks_u8) writes the three byte masks of the batch, and the model runs its masked
evaluation pass (batch keys ``mask_atoms`` / ``mask_bonds`` / ``mask_fbonds`` -> fn_encoder_forward_masked).

Replica order and indices are viz.py's: atoms ``0 .. n-1``; bonds by their first directed row ``0, 2, 4, ...`` (the reference's
``bond_index`` column: ``bond_mask`` zeroes rows ``i, i + 1``); fragment connections ``k = 0 .. EF/2 - 1`` (rows ``2k, 2k + 1``).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

KIND_NONE, KIND_ATOM, KIND_BOND, KIND_FBOND = 0, 1, 2, 3
KINDS = {"atom": KIND_ATOM, "bond": KIND_BOND, "fbond": KIND_FBOND}
KIND_ORDER = ("atom", "bond", "fbond")
DEFAULT_MAX_ROWS = 1 << 18       # atom + directed-bond rows of one replica batch: ~3000 ESOL-size replicas


def _kinds(kinds: Sequence[str]) -> Tuple[str, ...]:
    kinds = tuple(kinds)
    for k in kinds:
        if k not in KINDS:
            raise ValueError(f"kinds: {k!r} is not one of {KIND_ORDER}")
    if len(set(kinds)) != len(kinds) or not kinds:
        raise ValueError("kinds: a non-empty selection without repeats")
    return tuple(k for k in KIND_ORDER if k in kinds)          # viz.py's order whatever the caller's


def replica_table(n_atoms, n_bonds_directed, n_fbonds_directed, kinds=KIND_ORDER) -> List[np.ndarray]:
    """Per molecule the int32 array [count, 2] of its replicas ``(kind, index)``, kinds as KIND_*: atoms ``0 .. n-1``, then bonds
    by directed row index ``0, 2, ...``, then fragment connections ``0 .. EF/2 - 1``.  The arguments are per-molecule counts
    (directed rows for the two edge spaces).  A molecule with one fragment has no fragment-connection replica: the featuriser gives
    it no connection row, or a single placeholder row (a self edge), and viz.py:1107-1110 returns an empty frame for it."""
    kinds = _kinds(kinds)
    na, nb, nf = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (n_atoms, n_bonds_directed, n_fbonds_directed))
    if not (na.shape == nb.shape == nf.shape):
        raise ValueError("replica_table: one count per molecule in each of the three arguments")
    if (na < 0).any() or (nb < 0).any() or (nf < 0).any() or (nb % 2).any() or ((nf % 2 == 1) & (nf != 1)).any():
        raise ValueError("replica_table: counts must be non-negative, directed-row counts even (one placeholder fragment-bond row aside)")
    out = []
    for a, b, f in zip(na.tolist(), nb.tolist(), nf.tolist()):
        parts = []
        if "atom" in kinds:
            parts.append(np.stack([np.full(a, KIND_ATOM), np.arange(a)], 1))
        if "bond" in kinds:
            parts.append(np.stack([np.full(b // 2, KIND_BOND), np.arange(0, b, 2)], 1))
        if "fbond" in kinds:
            parts.append(np.stack([np.full(f // 2, KIND_FBOND), np.arange(f // 2)], 1))
        out.append(np.concatenate(parts, 0).astype(np.int32).reshape(-1, 2))
    return out


def local_index(table: np.ndarray) -> np.ndarray:
    """(kind, local index) as fn_loo_row_masks_u8 takes them: a bond by its pair number ``k`` (rows 2k, 2k + 1), not by its row."""
    out = np.array(table, dtype=np.int32, copy=True).reshape(-1, 2)
    bond = out[:, 0] == KIND_BOND
    out[bond, 1] //= 2
    return out


def plan_chunks(rows_per_mol, replicas_per_mol, max_rows: int) -> List[List[Tuple[int, int, int]]]:
    """Splits the replica list (molecule-major) into chunks of at most ``max_rows`` rows, a replica of molecule i costing
    ``rows_per_mol[i]``.  A chunk is a list of spans ``(molecule, first replica, end replica)``; a molecule's replicas may span
    chunks; a chunk holds at least one replica even where a single molecule exceeds the budget."""
    if max_rows < 1:
        raise ValueError("max_rows must be positive")
    chunks, cur, used = [], [], 0
    for i, (rows, count) in enumerate(zip(np.asarray(rows_per_mol).tolist(), np.asarray(replicas_per_mol).tolist())):
        rows = max(int(rows), 1)
        r = 0
        while r < count:
            fit = (max_rows - used) // rows
            if fit <= 0:
                if cur:
                    chunks.append(cur)
                    cur, used = [], 0
                    continue
                fit = 1                      # an empty chunk takes one replica whatever it costs
            take = min(fit, count - r)
            cur.append((i, r, r + take))
            used += take * rows
            r += take
    if cur:
        chunks.append(cur)
    return chunks


class Attribution:
    """Result of ``leave_one_out``: flat arrays plus per-molecule offsets (``arrays()`` is what the command-line script writes);
    ``result[i]`` is molecule i as a dict ``{"pred_no_mask": [n_classes], kind: {"index": [count], "pred_mask": [count,
    n_classes], "attr": [count, n_classes]}}`` -- the reference's DataFrame columns as arrays."""

    def __init__(self, pred_no_mask: np.ndarray, kinds: Tuple[str, ...], tables: Dict[str, Dict[str, np.ndarray]]):
        self.pred_no_mask, self.kinds, self.tables = pred_no_mask, kinds, tables

    def __len__(self):
        return self.pred_no_mask.shape[0]

    def __getitem__(self, i: int) -> dict:
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        i %= len(self)
        out = {"pred_no_mask": self.pred_no_mask[i]}
        for k in self.kinds:
            t = self.tables[k]
            lo, hi = int(t["offsets"][i]), int(t["offsets"][i + 1])
            out[k] = {"index": t["index"][lo:hi], "pred_mask": t["pred_mask"][lo:hi], "attr": t["attr"][lo:hi]}
        return out

    def arrays(self) -> Dict[str, np.ndarray]:
        out = {"pred_no_mask": self.pred_no_mask, "kinds": np.array(self.kinds)}
        for k in self.kinds:
            for name, v in self.tables[k].items():
                out[f"{k}_{name}"] = v
        return out


def _as_store(source, device):
    from .dataset import FlatMolStore
    if isinstance(source, FlatMolStore):
        return source if source.device == device else source.to(device)
    records = list(source)
    if not records:
        raise ValueError("leave_one_out: no molecules")
    return FlatMolStore.from_records(records).to(device)


def build_row_masks(batch, replicas_dev, status):
    """The three uint8 masks of a collated replica batch, written by one launch.  ``replicas_dev``: int32 [B, 2] (kind, local index)
    on the batch's device; ``status``: int32 [1] device word that collects FN_STATUS_BAD_REPLICA."""
    import torch
    from . import _lib
    from .plan import SPACES, _stream_ptr
    off = batch.offsets
    if off is None or not off.is_cuda:
        raise ValueError("build_row_masks: a collated batch with its offsets table on the GPU (data.batch_to / FlatMolStore.collate)")
    dev = off.device
    B = off.shape[1] - 1
    if replicas_dev.shape != (B, 2) or replicas_dev.dtype != torch.int32 or not replicas_dev.is_contiguous() or replicas_dev.device != dev:
        raise ValueError(f"build_row_masks: replicas must be a contiguous int32 [{B}, 2] tensor on {dev}")
    N, E, EF = batch["x_atoms"].shape[0], batch["node_features_bonds"].shape[0], batch["node_features_fbonds"].shape[0]
    pad = lambda n: (n + 15) // 16 * 16
    buf = torch.empty(pad(N) + pad(E) + pad(EF), dtype=torch.uint8, device=dev)      # one allocation, every mask 16-byte aligned
    masks = (buf[:N], buf[pad(N): pad(N) + E], buf[pad(N) + pad(E): pad(N) + pad(E) + EF])
    rows = [off[SPACES.index(s)] for s in ("atom", "edge", "fedge")]
    _lib.call("fn_loo_row_masks_u8", replicas_dev.data_ptr(), B, *(r.data_ptr() for r in rows), masks[0].data_ptr(), N,
              masks[1].data_ptr(), E, masks[2].data_ptr(), EF, status.data_ptr(), _stream_ptr(dev))
    return masks


def leave_one_out(model, source, kinds=KIND_ORDER, max_rows: int = DEFAULT_MAX_ROWS, batch_size: int = 512) -> Attribution:
    """Leave-one-out attributions of every molecule of ``source`` (a ``FlatMolStore`` or a list of ``MolRecord``) under ``model``
    (a ``FragNetFineTune`` on the GPU, model_version gat2, any head, any ``n_classes``).  The unmasked predictions run in evaluation
    batches of ``batch_size`` molecules; the replicas in chunks of at most ``max_rows`` atom + directed-bond rows."""
    import torch
    from .model import MASK_KEYS
    kinds = _kinds(kinds)
    enc = getattr(model, "pretrain", None)
    if enc is None or getattr(enc, "variant", None) != "gat2":
        raise ValueError(f"leave_one_out: masks exist for model_version gat2 (got {getattr(enc, 'variant', type(model).__name__)!r})")
    device = next(model.parameters()).device
    if device.type != "cuda":
        from . import _lib
        raise _lib.FragnetHipError("leave_one_out runs on the GPU engine; there is no CPU fallback")
    store = _as_store(source, device)
    n = len(store)
    lens = store._host_lengths()
    table = replica_table(lens["atom"], lens["edge"], lens["fedge"], kinds)
    counts = np.array([t.shape[0] for t in table], dtype=np.int64)
    chunks = plan_chunks(lens["atom"] + lens["edge"], counts, max_rows)
    first = np.concatenate([[0], np.cumsum(counts)])
    total = int(first[-1])
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            base = []
            for b in range(0, n, batch_size):
                base.append(model(store.collate(np.arange(b, min(n, b + batch_size)))).reshape(min(n, b + batch_size) - b, -1).float())
            base = torch.cat(base, 0)
            n_classes = base.shape[1]
            pred_mask = torch.empty((total, n_classes), dtype=torch.float32, device=device)
            attr = torch.empty_like(pred_mask)
            status = torch.zeros(1, dtype=torch.int32, device=device)
            for chunk in chunks:
                mols = np.concatenate([np.full(r1 - r0, i, dtype=np.int64) for i, r0, r1 in chunk])
                reps = np.concatenate([local_index(table[i][r0:r1]) for i, r0, r1 in chunk], 0)
                slots = torch.from_numpy(np.concatenate([np.arange(first[i] + r0, first[i] + r1) for i, r0, r1 in chunk])).to(device)
                batch = store.collate(mols)
                masks = build_row_masks(batch, torch.from_numpy(np.ascontiguousarray(reps)).to(device), status)
                for key, m in zip(MASK_KEYS, masks):
                    batch[key] = m
                pm = model(batch).reshape(len(mols), -1).float()
                pred_mask[slots] = pm
                attr[slots] = base[torch.from_numpy(mols).to(device)] - pm
            if int(status.item()):
                raise IndexError("leave_one_out: a replica index lies outside its molecule (FN_STATUS_BAD_REPLICA)")
            base_h, pred_h, attr_h = base.cpu().numpy(), pred_mask.cpu().numpy(), attr.cpu().numpy()
    finally:
        model.train(was_training)
    flat = np.concatenate(table, 0) if total else np.zeros((0, 2), np.int32)
    mol_of = np.repeat(np.arange(n), counts)
    tables = {}
    for k in kinds:
        sel = flat[:, 0] == KINDS[k]
        per_mol = np.bincount(mol_of[sel], minlength=n)
        tables[k] = {"offsets": np.concatenate([[0], np.cumsum(per_mol)]).astype(np.int64), "index": flat[sel, 1].astype(np.int32),
                     "pred_mask": pred_h[sel], "attr": attr_h[sel]}
    return Attribution(base_h, kinds, tables)
