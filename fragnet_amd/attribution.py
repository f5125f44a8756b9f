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


# ================================================================================================ fragment contributions
# The reference's fragment contribution (fragnet/vizualize/model_attr.py ``get_attr_image``): mask one fragment, predict again, report
# ``pred_no_mask - pred_mask``.  Its mask sits BEHIND the encoder -- with ``apply_mask=True`` the fragment's rows of the encoder's final
# x_atoms are set to 0.0 just before the two pools (model_attr.py:186-205, :251-263, :285-292), x_frags stays -- so every replica of a
# molecule shares the molecule's encoder pass: one pass per molecule, a read-out that leaves a group of atoms out of the atom sum
# (ops.pool_cat_groups) and one head call over the unmasked and the replica rows.
def flat_group_table(flat, atom_off):
    """The replica table of all molecules at once.  ``flat``: int64 [N], the group id of every atom of every molecule (< 0: in no
    group); ``atom_off``: int64 [n + 1], first atom of every molecule.  Returns ``(molecule [R], id [R], n_atoms [R], count [n])``: one
    replica per molecule and distinct id >= 0, molecule-major, ids ascending within a molecule."""
    flat, atom_off = np.asarray(flat, dtype=np.int64), np.asarray(atom_off, dtype=np.int64)
    n = atom_off.shape[0] - 1
    mol = np.repeat(np.arange(n, dtype=np.int64), np.diff(atom_off))
    keep = flat >= 0
    if not keep.all():
        flat, mol = flat[keep], mol[keep]
    if flat.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, np.zeros(n, dtype=np.int64)
    span = int(flat.max()) + 1
    if n * span <= max(1 << 16, 8 * flat.size):           # small ids (fragment numbers): a histogram over (molecule, id), no sort
        hist = np.bincount(mol * span + flat, minlength=n * span)
        key = np.flatnonzero(hist)
        rep_mol, ids, sizes = key // span, key % span, hist[key]
    else:                                                  # arbitrary ids: sort the (molecule, id) pairs
        order = np.lexsort((flat, mol))
        mol, flat = mol[order], flat[order]
        new = np.ones(flat.size, dtype=bool)
        new[1:] = (mol[1:] != mol[:-1]) | (flat[1:] != flat[:-1])
        starts = np.flatnonzero(new)
        rep_mol, ids, sizes = mol[starts], flat[starts], np.diff(np.append(starts, flat.size))
    return rep_mol.astype(np.int64), ids.astype(np.int64), sizes.astype(np.int64), np.bincount(rep_mol, minlength=n).astype(np.int64)


def _group_array(g, what):
    g = g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)
    if g.ndim != 1 or g.dtype.kind not in "iu":
        raise ValueError(f"{what}: one integer id per atom as a 1-d integer array (got dtype {g.dtype}, shape {g.shape})")
    return g


def group_table(atom_groups) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """Per molecule (ids, n_atoms): the distinct group ids >= 0 of its int array ``[n_atoms]`` in ascending order -- one replica each --
    and the number of atoms that carry each.  An id < 0 marks an atom that is in no group."""
    arrays = [_group_array(g, f"groups[{i}]") for i, g in enumerate(atom_groups)]
    if not arrays:
        return [], []
    atom_off = np.concatenate([[0], np.cumsum([g.shape[0] for g in arrays])]).astype(np.int64)
    _, ids, sizes, counts = flat_group_table(np.concatenate(arrays) if arrays else np.zeros(0, np.int64), atom_off)
    cut = np.cumsum(counts)[:-1]
    return np.split(ids, cut), np.split(sizes, cut)


def _flat_groups(groups, n_atoms) -> np.ndarray:
    """The caller's ``groups`` (one int array [n_atoms] per molecule) as one int64 array, checked against the molecules' sizes."""
    groups = list(groups)
    if len(groups) != len(n_atoms):
        raise ValueError(f"groups: one array per molecule ({len(n_atoms)} molecules, {len(groups)} arrays)")
    arrays = []
    for i, (g, k) in enumerate(zip(groups, n_atoms)):
        g = _group_array(g, f"groups[{i}]")
        if g.shape[0] != int(k):
            raise ValueError(f"groups[{i}]: {g.shape[0]} ids for a molecule of {int(k)} atoms")
        arrays.append(g)
    return np.concatenate(arrays).astype(np.int64)


class FragmentAttribution:
    """Result of ``fragment_contributions``.  ``result[i]`` is molecule i as ``{"pred_no_mask": [C], "group": [count] ids, "n_atoms":
    [count], "pred_mask": [count, C], "attr": [count, C]}``; ``arrays()`` the flat arrays plus per-molecule offsets that the command-line
    script writes; ``atom_weights(i)`` the reference's ``add_atom_weights``.  ``atom_group`` / ``atom_offsets``: every atom's group id,
    flat, and the first atom of every molecule."""

    def __init__(self, pred_no_mask, offsets, group, n_atoms, pred_mask, attr, atom_group, atom_offsets):
        self.pred_no_mask, self.offsets, self.group, self.n_atoms = pred_no_mask, offsets, group, n_atoms
        self.pred_mask, self.attr, self.atom_group, self.atom_offsets = pred_mask, attr, atom_group, atom_offsets

    def __len__(self):
        return self.pred_no_mask.shape[0]

    def _index(self, i: int) -> int:
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        return i % len(self)

    def __getitem__(self, i: int) -> dict:
        i = self._index(i)
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        return {"pred_no_mask": self.pred_no_mask[i], "group": self.group[lo:hi], "n_atoms": self.n_atoms[lo:hi],
                "pred_mask": self.pred_mask[lo:hi], "attr": self.attr[lo:hi]}

    def atom_weights(self, i: int) -> np.ndarray:
        """[n_atoms of molecule i, C]: every atom carries its group's attribution, an atom in no group 0 (model_attr.py:767-781)."""
        i = self._index(i)
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        g = self.atom_group[int(self.atom_offsets[i]): int(self.atom_offsets[i + 1])]
        out = np.zeros((g.shape[0], self.attr.shape[1]), dtype=self.attr.dtype)
        if hi > lo:
            pos = np.minimum(np.searchsorted(self.group[lo:hi], g), hi - lo - 1)          # the molecule's ids are ascending
            hit = self.group[lo:hi][pos] == g
            out[hit] = self.attr[lo:hi][pos[hit]]
        return out

    def arrays(self) -> Dict[str, np.ndarray]:
        return {"pred_no_mask": self.pred_no_mask, "offsets": self.offsets, "group": self.group, "n_atoms": self.n_atoms,
                "pred_mask": self.pred_mask, "attr": self.attr, "atom_offsets": self.atom_offsets, "atom_group": self.atom_group}


def _store_fragment_table(store):
    """(fragment map of every atom on the host, its replica table ``flat_group_table``) of a ``FlatMolStore``: derived once and kept on
    the store, like its host-side lengths and offsets (the store is immutable)."""
    import torch
    hit = getattr(store, "_frag_table_cpu", None)
    if hit is None:
        flat = store.t["atom_id_frag_id"].to("cpu", torch.long).numpy()
        hit = store._frag_table_cpu = (flat, flat_group_table(flat, store._host_offsets()["atom"]))
    return hit


def _contribution_kind(model) -> str:
    from . import cdrp, dta
    from .model import FragNetFineTune, FragNetPreTrain
    if isinstance(model, FragNetFineTune):
        return "property"
    if isinstance(model, FragNetPreTrain):
        return "energy"
    if isinstance(model, cdrp.CDRPModel):
        return "drp"
    if isinstance(model, dta.DTAModel2):
        return "dta"
    raise ValueError(f"fragment_contributions: {type(model).__name__} is not one of FragNetFineTune, FragNetPreTrain, cdrp.CDRPModel, "
                     "dta.DTAModel2")


def _contribution_rows(kind, model, batch, atom_group, row_mol, row_group):
    """One encoder pass, one leave-group-out read-out and one head call: the predictions [rows, C] of ``row_mol`` / ``row_group``."""
    import torch
    from . import ops
    from .plan import plan_for
    encoder = (model.drug_model if kind in ("drp", "dta") else model).pretrain
    x_atoms, x_frags = encoder(batch, edge_outputs=False)[:2]
    enc = ops.pool_cat_groups(x_atoms, x_frags, plan_for(batch), atom_group, row_mol, row_group, check=False)      # rows checked by the caller
    if kind == "property":
        model.fthead.live_rows = None
        out = model.fthead(enc)
    elif kind == "energy":
        out = model.head._tower(model.head.FC_layers, enc)
    else:
        rows = row_mol.to(torch.long)
        if kind == "drp":         # the second tower once per molecule, expanded to the rows
            out = ops.pair_head(enc, model.cell_model(batch["gene_expr"]).index_select(0, rows), model.fc1, model.fc2)
        else:
            xt = ops.protein_tower(batch["protein"].reshape(-1, model.in_channels), model.embedding_xt, model.conv_xt_1, model.fc1_xt)
            out = ops.pair_head_dta(enc, xt.index_select(0, rows), model.fc1, model.fc2)
    return out.reshape(row_mol.shape[0], -1).float()


def fragment_contributions(model, source, groups=None, batch_size: int = 512) -> FragmentAttribution:
    """Fragment contributions ``pred_no_mask - pred_mask`` of every molecule of ``source`` under ``model`` on the GPU: a
    ``FragNetFineTune`` (any head, ``n_classes``, ``model_version``), a ``cdrp.CDRPModel``, a ``dta.DTAModel2`` or a
    ``FragNetPreTrain`` (its 4th output, the energy).  ``source``: a ``FlatMolStore`` (plain models) or a list of ``MolRecord`` -- the
    only form for the pair models, whose records carry ``gene_expr`` / ``protein``.  ``groups=None``: one replica per fragment
    (``atom_id_frag_id``), in fragment order; else one int array ``[n_atoms]`` of local group ids per molecule (< 0: the atom is in no
    group), one replica per distinct id >= 0 in ascending order.  Per chunk of ``batch_size`` molecules: one evaluation encoder pass,
    one read-out whose rows are the chunk's unmasked rows followed by its replica rows, one head call over all of them."""
    import torch
    from . import data
    kind = _contribution_kind(model)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    from .dataset import FlatMolStore
    store = records = None
    if isinstance(source, FlatMolStore):
        if kind in ("drp", "dta"):
            raise ValueError(f"fragment_contributions: a {type(model).__name__} takes a list of records (they carry "
                             f"{'gene_expr' if kind == 'drp' else 'protein'}), not a FlatMolStore")
        store = source
        n_atoms = store._host_lengths()["atom"]
        if groups is None:
            flat = _store_fragment_table(store)[0]
    else:
        records = list(source)
        if not records:
            raise ValueError("fragment_contributions: no molecules")
        n_atoms = np.array([int(r.x_atoms.shape[0]) for r in records], dtype=np.int64)
        if groups is None:
            flat = torch.cat([r.atom_id_frag_id for r in records]).to(torch.long).numpy()
    if groups is not None:
        flat = _flat_groups(groups, n_atoms)
    n = len(n_atoms)
    atom_off = np.concatenate([[0], np.cumsum(n_atoms)]).astype(np.int64)
    if store is not None and groups is None:
        rep_mol, ids, sizes, counts = _store_fragment_table(store)[1]
    else:
        rep_mol, ids, sizes, counts = flat_group_table(flat, atom_off)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    R = int(offsets[-1])
    device = next(model.parameters()).device
    if device.type != "cuda":
        from . import _lib
        raise _lib.FragnetHipError("fragment_contributions runs on the GPU engine; there is no CPU fallback")
    if kind in ("drp", "dta"):
        collate = data.collate_fn_cdrp if kind == "drp" else data.collate_fn_dta
    else:
        store = _as_store(source if store is not None else records, device)
    # every chunk's rows in ONE upload: [row groups int64 | row molecules int32 | atom groups int64], rows chunk-major, a chunk's B
    # unmasked rows (group -1) in front of its replica rows; chunks are runs of molecules, so each takes contiguous slices.  The atom
    # groups are not uploaded where they are the fragment map of a store that lives on the device.
    starts = list(range(0, n, batch_size))
    N = int(atom_off[-1])
    frag_map = store.t["atom_id_frag_id"] if store is not None and groups is None else None
    on_device = frag_map is not None and frag_map.dtype == torch.long and frag_map.is_contiguous() and frag_map.device == device
    words = (n + R) + (n + R + 1) // 2
    host = np.empty(words + (0 if on_device else N), dtype=np.int64)
    row_group_h, row_mol_h = host[: n + R], host[n + R: words].view(np.int32)[: n + R]
    if not on_device:
        host[words:] = flat
    row0 = []
    for b in starts:
        e = min(n, b + batch_size)
        r0, lo, hi = b + int(offsets[b]), int(offsets[b]), int(offsets[e])
        row0.append(r0)
        row_group_h[r0: r0 + e - b] = -1
        row_group_h[r0 + e - b: r0 + e - b + hi - lo] = ids[lo:hi]
        row_mol_h[r0: r0 + e - b] = np.arange(e - b)
        row_mol_h[r0 + e - b: r0 + e - b + hi - lo] = rep_mol[lo:hi] - b          # in [0, B) by construction: ops' own check is skipped
    dev_buf = torch.from_numpy(host).to(device)
    row_group_d, row_mol_d = dev_buf[: n + R], dev_buf[n + R: words].view(torch.int32)[: n + R]
    atom_group_d = frag_map if on_device else dev_buf[words:]
    was_training = model.training
    model.eval()
    preds = []
    try:
        with torch.no_grad():
            for b, r0 in zip(starts, row0):
                e = min(n, b + batch_size)
                rows = e - b + int(offsets[e] - offsets[b])
                batch = store.collate(np.arange(b, e)) if store is not None else data.batch_to(collate(records[b:e]), device)
                preds.append(_contribution_rows(kind, model, batch, atom_group_d[int(atom_off[b]): int(atom_off[e])], row_mol_d[r0: r0 + rows],
                                                row_group_d[r0: r0 + rows]))
            pred_h = (preds[0] if len(preds) == 1 else torch.cat(preds, 0)).cpu().numpy()
    finally:
        model.train(was_training)
    unmasked = np.zeros(n + R, dtype=bool)
    for b, r0 in zip(starts, row0):
        unmasked[r0: r0 + min(n, b + batch_size) - b] = True
    base_h, masked_h = pred_h[unmasked], pred_h[~unmasked]
    return FragmentAttribution(base_h, offsets, ids, sizes, masked_h, base_h[rep_mol] - masked_h, flat, atom_off)
