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

from contextlib import contextmanager
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


def chunk_replicas(chunk) -> Tuple[np.ndarray, np.ndarray]:
    """``(molecule of every replica, its number among its molecule's replicas)``, int64, of one chunk of ``plan_chunks``."""
    mols = np.concatenate([np.full(r1 - r0, i, dtype=np.int64) for i, r0, r1 in chunk])
    return mols, np.concatenate([np.arange(r0, r1, dtype=np.int64) for _, r0, r1 in chunk])


# ====================================== what the drivers of this module, gradient_attribution.py, pair_attribution.py and attention.py share
def offsets_of(counts) -> np.ndarray:
    """int64 ``[len(counts) + 1]``: 0, then the running sums of ``counts`` -- entry i is where item i's rows start in a flat array."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    out = np.zeros(counts.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=out[1:])
    return out


def batch_ranges(n: int, batch_size: int) -> List[Tuple[int, int]]:
    """``(first, end)`` of the batches of ``batch_size`` consecutive items that cover ``0 .. n``, the last one shorter."""
    return [(b, min(n, b + batch_size)) for b in range(0, n, batch_size)]


def store_batches(store, batch_size: int):
    """``(first, end, collated batch)`` per batch of ``batch_size`` consecutive molecules of a ``FlatMolStore``, collated when reached."""
    for b, e in batch_ranges(len(store), batch_size):
        yield b, e, store.collate(np.arange(b, e))


@contextmanager
def evaluation(model):
    """``model`` in ``eval()`` mode inside the block, back in the mode it came in on the way out, through an exception too.  Gradient
    mode is the caller's: input_gradients and the chunk loop of integrated_gradients differentiate inside this block."""
    mode = model.training
    model.eval()
    try:
        yield model
    finally:
        model.train(mode)


def engine_device(model, who: str):
    """The device of ``model``'s parameters if it is a GPU; else the drivers' refusal in ``who``'s name.  (pair_attribution's
    cell_line_attributions words its own: it runs kernels, not the engine, and on its tower's device.)"""
    device = next(model.parameters()).device
    if device.type != "cuda":
        from . import _lib
        raise _lib.FragnetHipError(f"{who} runs on the GPU engine; there is no CPU fallback")
    return device


def row_vector(v, width: int, device, prefix: str, unit: str):
    """``v`` -- a 1-d array or tensor of ``width`` real numbers -- as a contiguous float32 tensor on ``device``; the refusals start with
    ``prefix`` and count the entries in ``unit``."""
    import torch
    v = v.detach() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
    if v.dim() != 1 or v.shape[0] != width:
        raise ValueError(f"{prefix}: a row vector of {width} {unit} (got shape {tuple(v.shape)})")
    if not (v.dtype.is_floating_point or v.dtype in (torch.int32, torch.int64, torch.uint8, torch.bool)):
        raise ValueError(f"{prefix}: a real-valued vector (got {v.dtype})")
    return v.to(device=device, dtype=torch.float32).contiguous()


class PackedUpload:
    """Arrays of several dtypes that reach the device in ONE copy.  ``parts``: ``(numpy dtype, count)`` each; ``host`` holds a numpy view
    per part into one int64 buffer, every part on an 8-byte boundary, for the caller to fill in place; ``to(device)`` copies the buffer
    once and returns the matching views of the device tensor."""

    def __init__(self, parts):
        self._counts, self._first = [int(count) for _, count in parts], [0]
        for dt, count in parts:          # a part's first int64 word (plain ints: this runs once per chunk of fragment_shapley)
            self._first.append(self._first[-1] + (np.dtype(dt).itemsize * int(count) + 7) // 8)
        self.buffer = np.empty(self._first[-1], dtype=np.int64)
        self.host = [self._part(self.buffer, k, np.dtype(dt)) for k, (dt, _) in enumerate(parts)]

    def _part(self, buffer, k, dtype):
        return buffer[self._first[k]: self._first[k + 1]].view(dtype)[: self._counts[k]]

    def to(self, device):
        import torch
        dev = torch.from_numpy(self.buffer).to(device)
        return [self._part(dev, k, torch.from_numpy(h).dtype) for k, h in enumerate(self.host)]


def kept_on_store(store, name: str, derive):
    """``derive()``, computed at the first call and kept on the ``FlatMolStore`` as attribute ``name``, like its host-side lengths and
    offsets (the store is immutable)."""
    hit = getattr(store, name, None)
    if hit is None:
        hit = derive()
        setattr(store, name, hit)
    return hit


class _Result:
    """What the result classes share: ``len(result)`` is the first axis of the array that ``_per_item`` names, and ``_index(i)`` is
    ``i`` checked against it, a negative one counted from the end."""
    _per_item = "pred"

    def __len__(self):
        return getattr(self, self._per_item).shape[0]

    def _index(self, i: int) -> int:
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        return i % len(self)


class _KindTables(_Result):
    """A result with ``kinds`` and per kind ``tables[kind] = {"offsets": [n + 1], name: [total, ...], ...}``: flat arrays, molecule i's rows
    at ``offsets[i] : offsets[i + 1]`` (``_kind_rows(i)``: per kind those rows of every array of its table)."""

    def _kind_rows(self, i: int) -> Dict[str, Dict[str, np.ndarray]]:
        out = {}
        for k in self.kinds:
            t = self.tables[k]
            lo, hi = int(t["offsets"][i]), int(t["offsets"][i + 1])
            out[k] = {name: v[lo:hi] for name, v in t.items() if name != "offsets"}
        return out

    def _kind_arrays(self) -> Dict[str, np.ndarray]:
        return {f"{k}_{name}": v for k in self.kinds for name, v in self.tables[k].items()}


class Attribution(_KindTables):
    """Result of ``leave_one_out``: flat arrays plus per-molecule offsets (``arrays()`` is what the command-line script writes);
    ``result[i]`` is molecule i as a dict ``{"pred_no_mask": [n_classes], kind: {"index": [count], "pred_mask": [count,
    n_classes], "attr": [count, n_classes]}}`` -- the reference's DataFrame columns as arrays."""
    _per_item = "pred_no_mask"

    def __init__(self, pred_no_mask: np.ndarray, kinds: Tuple[str, ...], tables: Dict[str, Dict[str, np.ndarray]]):
        self.pred_no_mask, self.kinds, self.tables = pred_no_mask, kinds, tables

    def __getitem__(self, i: int) -> dict:
        i = self._index(i)
        return {"pred_no_mask": self.pred_no_mask[i], **self._kind_rows(i)}

    def arrays(self) -> Dict[str, np.ndarray]:
        return {"pred_no_mask": self.pred_no_mask, "kinds": np.array(self.kinds), **self._kind_arrays()}


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
    device = engine_device(model, "leave_one_out")
    store = _as_store(source, device)
    n = len(store)
    lens = store._host_lengths()
    table = replica_table(lens["atom"], lens["edge"], lens["fedge"], kinds)
    counts = np.array([t.shape[0] for t in table], dtype=np.int64)
    chunks = plan_chunks(lens["atom"] + lens["edge"], counts, max_rows)
    first = offsets_of(counts)
    total = int(first[-1])
    flat = np.concatenate(table, 0) if total else np.zeros((0, 2), np.int32)
    flat_local = local_index(flat)
    with evaluation(model), torch.no_grad():
        base = torch.cat([model(batch).reshape(e - b, -1).float() for b, e, batch in store_batches(store, batch_size)], 0)
        n_classes = base.shape[1]
        pred_mask = torch.empty((total, n_classes), dtype=torch.float32, device=device)
        attr = torch.empty_like(pred_mask)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        for chunk in chunks:
            mols, rep = chunk_replicas(chunk)
            slots_h = first[mols] + rep          # the replicas' rows of the flat table, and of the result
            slots = torch.from_numpy(slots_h).to(device)
            batch = store.collate(mols)
            masks = build_row_masks(batch, torch.from_numpy(flat_local[slots_h]).to(device), status)
            for key, m in zip(MASK_KEYS, masks):
                batch[key] = m
            pm = model(batch).reshape(len(mols), -1).float()
            pred_mask[slots] = pm
            attr[slots] = base[torch.from_numpy(mols).to(device)] - pm
        if int(status.item()):
            raise IndexError("leave_one_out: a replica index lies outside its molecule (FN_STATUS_BAD_REPLICA)")
        base_h, pred_h, attr_h = base.cpu().numpy(), pred_mask.cpu().numpy(), attr.cpu().numpy()
    mol_of = np.repeat(np.arange(n), counts)
    tables = {}
    for k in kinds:
        sel = flat[:, 0] == KINDS[k]
        tables[k] = {"offsets": offsets_of(np.bincount(mol_of[sel], minlength=n)), "index": flat[sel, 1].astype(np.int32),
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
    atom_off = offsets_of([g.shape[0] for g in arrays])
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


class _GroupResult(_Result):
    """A result per group of atoms.  Rows ``offsets[i] : offsets[i + 1]`` of ``group`` (ids, ascending) and ``n_atoms`` are molecule
    i's groups; ``atom_group`` / ``atom_offsets``: every atom's group id, flat, and the first atom of every molecule.  ``_per_group`` names
    the array ``[R, C]`` that ``atom_weights`` spreads over the atoms."""

    def _set_groups(self, offsets, group, n_atoms, atom_group, atom_offsets):
        self.offsets, self.group, self.n_atoms, self.atom_group, self.atom_offsets = offsets, group, n_atoms, atom_group, atom_offsets

    def atom_weights(self, i: int) -> np.ndarray:
        """[n_atoms of molecule i, C]: every atom carries its group's attribution, an atom in no group 0 (model_attr.py:767-781)."""
        return _spread_to_atoms(getattr(self, self._per_group), self.group, self.offsets, self.atom_group, self.atom_offsets, self._index(i))


class FragmentAttribution(_GroupResult):
    """Result of ``fragment_contributions``.  ``result[i]`` is molecule i as ``{"pred_no_mask": [C], "group": [count] ids, "n_atoms":
    [count], "pred_mask": [count, C], "attr": [count, C]}``; ``arrays()`` the flat arrays plus per-molecule offsets that the command-line
    script writes; ``atom_weights(i)`` the reference's ``add_atom_weights``.  ``atom_group`` / ``atom_offsets``: every atom's group id,
    flat, and the first atom of every molecule."""
    _per_item, _per_group = "pred_no_mask", "attr"

    def __init__(self, pred_no_mask, offsets, group, n_atoms, pred_mask, attr, atom_group, atom_offsets):
        self._set_groups(offsets, group, n_atoms, atom_group, atom_offsets)
        self.pred_no_mask, self.pred_mask, self.attr = pred_no_mask, pred_mask, attr

    def __getitem__(self, i: int) -> dict:
        i = self._index(i)
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        return {"pred_no_mask": self.pred_no_mask[i], "group": self.group[lo:hi], "n_atoms": self.n_atoms[lo:hi],
                "pred_mask": self.pred_mask[lo:hi], "attr": self.attr[lo:hi]}

    def arrays(self) -> Dict[str, np.ndarray]:
        return {"pred_no_mask": self.pred_no_mask, "offsets": self.offsets, "group": self.group, "n_atoms": self.n_atoms,
                "pred_mask": self.pred_mask, "attr": self.attr, "atom_offsets": self.atom_offsets, "atom_group": self.atom_group}


def _store_fragment_table(store):
    """(fragment map of every atom on the host, its replica table ``flat_group_table``) of a ``FlatMolStore``: derived once and kept on
    the store (``kept_on_store``)."""
    import torch

    def derive():
        flat = store.t["atom_id_frag_id"].to("cpu", torch.long).numpy()
        return flat, flat_group_table(flat, store._host_offsets()["atom"])
    return kept_on_store(store, "_frag_table_cpu", derive)


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


def _contribution_rows(kind, model, batch, read_out, row_mol, head_rows=None):
    """One encoder pass, one read-out ``read_out(x_atoms, x_frags, plan) -> [rows, 256]`` and the head over its rows -- one call, or
    slices of at most ``head_rows`` rows: the predictions [rows, C] of the read-out's rows, row r a row of molecule ``row_mol[r]``."""
    import torch
    from . import ops
    from .plan import plan_for
    encoder = (model.drug_model if kind in ("drp", "dta") else model).pretrain
    x_atoms, x_frags = encoder(batch, edge_outputs=False)[:2]
    enc = read_out(x_atoms, x_frags, plan_for(batch))
    second = None                 # the pair models' second tower: once per molecule, expanded to the rows
    if kind == "drp":
        second = model.cell_model(batch["gene_expr"])
    elif kind == "dta":
        second = ops.protein_tower(batch["protein"].reshape(-1, model.in_channels), model.embedding_xt, model.conv_xt_1, model.fc1_xt)
    total = int(row_mol.shape[0])
    step = total if head_rows is None else int(head_rows)
    outs = []
    for lo in range(0, max(total, 1), max(step, 1)):
        part = enc[lo: lo + step] if step < total else enc
        if kind == "property":
            model.fthead.live_rows = None
            out = model.fthead(part)
        elif kind == "energy":
            out = model.head._tower(model.head.FC_layers, part)
        else:
            rows = row_mol[lo: lo + step].to(torch.long)
            if kind == "drp":
                out = ops.pair_head(part, second.index_select(0, rows), model.fc1, model.fc2)
            else:
                out = ops.pair_head_dta(part, second.index_select(0, rows), model.fc1, model.fc2)
        outs.append(out.reshape(part.shape[0], -1).float())
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


def _group_source(who, kind, model, source, groups):
    """What the fragment-level calls share: ``(store or None, records or None, collate or None, flat group id of every atom, first atom
    of every molecule, flat_group_table, the model's device)`` of ``source`` under ``groups``; refuses a model that is not on the GPU."""
    import torch
    from . import data
    from .dataset import FlatMolStore
    store = records = None
    if isinstance(source, FlatMolStore):
        if kind in ("drp", "dta"):
            raise ValueError(f"{who}: a {type(model).__name__} takes a list of records (they carry "
                             f"{'gene_expr' if kind == 'drp' else 'protein'}), not a FlatMolStore")
        store = source
        n_atoms = store._host_lengths()["atom"]
        if groups is None:
            flat = _store_fragment_table(store)[0]
    else:
        records = list(source)
        if not records:
            raise ValueError(f"{who}: no molecules")
        n_atoms = np.array([int(r.x_atoms.shape[0]) for r in records], dtype=np.int64)
        if groups is None:
            flat = torch.cat([r.atom_id_frag_id for r in records]).to(torch.long).numpy()
    if groups is not None:
        flat = _flat_groups(groups, n_atoms)
    atom_off = offsets_of(n_atoms)
    if store is not None and groups is None:
        table = _store_fragment_table(store)[1]
    else:
        table = flat_group_table(flat, atom_off)
    device = engine_device(model, who)          # (behind the table: a source or groups that are wrong are refused on any device)
    collate = None
    if kind in ("drp", "dta"):
        collate = data.collate_fn_cdrp if kind == "drp" else data.collate_fn_dta
    else:
        store = _as_store(source if store is not None else records, device)
    return store, records, collate, flat, atom_off, table, device


def fragment_contributions(model, source, groups=None, batch_size: int = 512) -> FragmentAttribution:
    """Fragment contributions ``pred_no_mask - pred_mask`` of every molecule of ``source`` under ``model`` on the GPU: a
    ``FragNetFineTune`` (any head, ``n_classes``, ``model_version``), a ``cdrp.CDRPModel``, a ``dta.DTAModel2`` or a
    ``FragNetPreTrain`` (its 4th output, the energy).  ``source``: a ``FlatMolStore`` (plain models) or a list of ``MolRecord`` -- the
    only form for the pair models, whose records carry ``gene_expr`` / ``protein``.  ``groups=None``: one replica per fragment
    (``atom_id_frag_id``), in fragment order; else one int array ``[n_atoms]`` of local group ids per molecule (< 0: the atom is in no
    group), one replica per distinct id >= 0 in ascending order.  Per chunk of ``batch_size`` molecules: one evaluation encoder pass,
    one read-out whose rows are the chunk's unmasked rows followed by its replica rows, one head call over all of them."""
    import torch
    from . import data, ops
    kind = _contribution_kind(model)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    store, records, collate, flat, atom_off, table, device = _group_source("fragment_contributions", kind, model, source, groups)
    (rep_mol, ids, sizes, counts), n = table, atom_off.shape[0] - 1
    offsets = offsets_of(counts)
    R = int(offsets[-1])
    # every chunk's rows in ONE upload: [row groups int64 | row molecules int32 | atom groups int64], rows chunk-major, a chunk's B
    # unmasked rows (group -1) in front of its replica rows; chunks are runs of molecules, so each takes contiguous slices.  The atom
    # groups are not uploaded where they are the fragment map of a store that lives on the device.
    chunks = batch_ranges(n, batch_size)
    frag_map = store.t["atom_id_frag_id"] if store is not None and groups is None else None
    on_device = frag_map is not None and frag_map.dtype == torch.long and frag_map.is_contiguous() and frag_map.device == device
    upload = PackedUpload([(np.int64, n + R), (np.int32, n + R)] + ([] if on_device else [(np.int64, int(atom_off[-1]))]))
    row_group_h, row_mol_h = upload.host[:2]
    if not on_device:
        upload.host[2][:] = flat
    unmasked = np.zeros(n + R, dtype=bool)
    for b, e in chunks:
        r0, lo, hi = b + int(offsets[b]), int(offsets[b]), int(offsets[e])          # the chunk's first row: its molecules' and replicas' sum
        unmasked[r0: r0 + e - b] = True
        row_group_h[r0: r0 + e - b] = -1
        row_group_h[r0 + e - b: r0 + e - b + hi - lo] = ids[lo:hi]
        row_mol_h[r0: r0 + e - b] = np.arange(e - b)
        row_mol_h[r0 + e - b: r0 + e - b + hi - lo] = rep_mol[lo:hi] - b          # in [0, B) by construction: ops' own check is skipped
    row_group_d, row_mol_d, *rest = upload.to(device)
    atom_group_d = frag_map if on_device else rest[0]
    preds = []
    with evaluation(model), torch.no_grad():
        for b, e in chunks:
            r0 = b + int(offsets[b])
            rows = e - b + int(offsets[e] - offsets[b])
            batch = store.collate(np.arange(b, e)) if store is not None else data.batch_to(collate(records[b:e]), device)
            rm, rg, ag = row_mol_d[r0: r0 + rows], row_group_d[r0: r0 + rows], atom_group_d[int(atom_off[b]): int(atom_off[e])]
            preds.append(_contribution_rows(kind, model, batch, lambda xa, xf, plan: ops.pool_cat_groups(xa, xf, plan, ag, rm, rg, check=False),
                                            rm))          # rows built and checked here, on the host
        pred_h = (preds[0] if len(preds) == 1 else torch.cat(preds, 0)).cpu().numpy()
    base_h, masked_h = pred_h[unmasked], pred_h[~unmasked]
    return FragmentAttribution(base_h, offsets, ids, sizes, masked_h, base_h[rep_mol] - masked_h, flat, atom_off)


# ================================================================================================ fragment Shapley values
# fragment_contributions reports leave-one-out numbers; with a non-linear head they do not add up to pred - v(no fragment).  The Shapley
# values of the set function v(S) = prediction with the atoms of every group OUTSIDE S zeroed behind the encoder do: sum_f phi_f =
# v(all) - v(none).  The mask sits behind the encoder, so a coalition costs one pooled sum (ops.pool_cat_coalitions) and one head row.
DEFAULT_SHAPLEY_ROWS = 1 << 16
_WEIGHTS, _PREFIX_ROWS = {}, {}


def shapley_weights(F: int):
    """The exact-mode template of F groups, cached: ``(without [F, 2^(F-1)], with [F, 2^(F-1)], weight [F, 2^(F-1)])`` -- for group f
    the masks S without f in ascending order, S | 1 << f, and s! (F - s - 1)! / F! with s = |S|.  A mask is its own row index."""
    hit = _WEIGHTS.get(F)
    if hit is None:
        if not 1 <= F <= 30:
            raise ValueError(f"shapley_weights: 1 <= F <= 30 (got {F})")
        from math import factorial
        masks = np.arange(1 << F, dtype=np.int64)
        size = np.zeros(1 << F, dtype=np.int64)
        for f in range(F):
            size += (masks >> f) & 1
        by_size = np.array([factorial(s) * factorial(F - s - 1) / factorial(F) for s in range(F)], dtype=np.float64)
        without = np.stack([masks[((masks >> f) & 1) == 0] for f in range(F)])
        hit = _WEIGHTS[F] = (without, without | (np.int64(1) << np.arange(F, dtype=np.int64))[:, None], by_size[size[without]])
    return hit


def shapley_exact(values: np.ndarray, F: int) -> np.ndarray:
    """phi [M, F, C] (float64) of M set functions on F groups from their values [M, 2^F, C], row index = mask:
    phi_f = sum over S without f of s! (F - s - 1)! / F! (v(S + f) - v(S))."""
    v = np.asarray(values, dtype=np.float64)
    if F == 0:
        return np.zeros((v.shape[0], 0, v.shape[2]), dtype=np.float64)
    without, with_f, w = shapley_weights(F)
    return np.einsum("fs,mfsc->mfc", w, v[:, with_f] - v[:, without])


def draw_permutations(F: int, samples: int, seed: int, molecule: int) -> np.ndarray:
    """[samples, F]: samples / 2 permutations of the groups from ``np.random.default_rng([seed, molecule])``, each followed by its
    reverse (antithetic pairs) -- a function of the molecule's own index and F alone."""
    rng = np.random.default_rng([int(seed), int(molecule)])
    half = np.stack([rng.permutation(F) for _ in range(samples // 2)]).astype(np.int64).reshape(samples // 2, F)
    out = np.empty((samples, F), dtype=np.int64)
    out[0::2], out[1::2] = half, half[:, ::-1]
    return out


def _full_mask(F: int) -> np.uint64:
    return np.uint64((1 << F) - 1)


def permutation_masks(perms: np.ndarray) -> np.ndarray:
    """The rows of a sampled molecule: uint64 [2 + K (F - 1)] -- the empty coalition, the full one, then per permutation its F - 1
    interior prefixes {pi_0}, {pi_0, pi_1}, ..."""
    K, F = perms.shape
    bits = np.left_shift(np.uint64(1), perms.astype(np.uint64))
    prefixes = np.bitwise_or.accumulate(bits, axis=1)[:, : max(F - 1, 0)]
    return np.concatenate([np.array([0, _full_mask(F)], dtype=np.uint64), prefixes.reshape(-1)])


def shapley_sampled(values: np.ndarray, perms: np.ndarray, paired: bool):
    """(phi [F, C], stderr [F, C]) from the values [2 + K (F - 1), C] of ``permutation_masks(perms)``: the mean marginal of every group
    over the K permutations; the standard error over the K / 2 means of consecutive pairs (``paired``: the antithetic draw) or over the K
    permutations (a caller's design); NaN where there is a single one."""
    v = np.asarray(values, dtype=np.float64)
    K, F = perms.shape
    rows = _PREFIX_ROWS.get((K, F))
    if rows is None:            # [K, F + 1]: row 0 (empty), the permutation's interior prefixes, row 1 (full)
        rows = np.empty((K, F + 1), dtype=np.int64)
        rows[:, 0], rows[:, F] = 0, 1
        rows[:, 1:F] = 2 + np.arange(K * (F - 1), dtype=np.int64).reshape(K, F - 1)
        _PREFIX_ROWS[(K, F)] = rows
    steps = v[rows]                                                   # [K, F + 1, C]
    marginal = np.take_along_axis(steps[:, 1:] - steps[:, :-1], np.argsort(perms, axis=1)[:, :, None], axis=1)      # by group
    units = 0.5 * (marginal[0::2] + marginal[1::2]) if paired else marginal
    if units.shape[0] > 1:
        stderr = units.std(axis=0, ddof=1) / np.sqrt(units.shape[0])
    else:
        stderr = np.full(marginal.shape[1:], np.nan)
    return marginal.mean(axis=0), stderr


def plan_coalition_chunks(rows_per_mol, batch_size: int, max_rows: int) -> List[Tuple[int, int]]:
    """Runs ``(first molecule, end molecule)`` of at most ``batch_size`` molecules whose rows sum to at most ``max_rows``; a molecule's
    rows are never split, so one that alone needs more than ``max_rows`` is refused."""
    if batch_size < 1 or max_rows < 1:
        raise ValueError("batch_size and max_rows must be positive")
    rows = np.asarray(rows_per_mol, dtype=np.int64)
    big = np.flatnonzero(rows > max_rows)
    if big.size:
        raise ValueError(f"fragment_shapley: molecule {int(big[0])} alone needs {int(rows[big[0]])} coalition rows, more than max_rows = {max_rows} "
                         "(lower exact_max or samples, or raise max_rows)")
    chunks, b, used = [], 0, 0
    for i, r in enumerate(rows.tolist()):
        if i > b and (i - b == batch_size or used + r > max_rows):
            chunks.append((b, i))
            b, used = i, 0
        used += r
    if len(rows):
        chunks.append((b, len(rows)))
    return chunks


def coalition_design(counts, additive=False, exact_max=10, samples=256, permutations=None):
    """``(mode [n], permutations {molecule: [K, F]}, rows [n])``: per molecule its mode -- ``"exact"`` (F <= exact_max: all 2^F masks, the
    row index is the mask), ``"sampled"`` (the antithetic draw, made when the molecule's chunk is built, or the caller's
    ``permutations[i]``), ``"additive"`` (an additive v: the empty row, the full row and all-but-one per group) -- and its number of rows."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    n = counts.shape[0]
    if samples < 2 or samples % 2:
        raise ValueError(f"fragment_shapley: samples must be even and positive, permutations come in antithetic pairs (got {samples})")
    if exact_max < 0:
        raise ValueError("fragment_shapley: exact_max must not be negative")
    if n and counts.max() > 64:
        i = int(np.argmax(counts > 64))
        raise ValueError(f"fragment_shapley: molecule {i} has {int(counts[i])} groups; a coalition mask holds 64")
    if additive:
        return np.full(n, "additive"), {}, 2 + counts
    exact = counts <= exact_max
    mode = np.where(exact, "exact", "sampled")
    rows = np.where(exact, np.left_shift(np.int64(1), np.minimum(counts, 62)), 2 + samples * (counts - 1))
    given = {}
    for i, perms in dict(permutations or {}).items():
        if not 0 <= int(i) < n:
            raise ValueError(f"fragment_shapley: permutations names molecule {i}; there are {n}")
        F, perms = int(counts[i]), np.asarray(perms)
        if perms.ndim != 2 or perms.shape[1] != F or perms.shape[0] < 1 or perms.dtype.kind not in "iu" or \
                (np.sort(perms, axis=1) != np.arange(F)).any():
            raise ValueError(f"fragment_shapley: permutations[{i}] must be an int array [K, {F}] whose rows are permutations of 0..{F - 1}")
        given[int(i)] = perms.astype(np.int64)
        mode[i], rows[i] = "sampled", 2 + perms.shape[0] * max(F - 1, 0)
    return mode, given, rows.astype(np.int64)


def _shapley_host(counts, evaluate, additive=False, batch_size=512, exact_max=10, samples=256, seed=0, permutations=None,
                  max_rows=DEFAULT_SHAPLEY_ROWS, return_values=False):
    """Everything of ``fragment_shapley`` that runs on the host: the design, the chunks, the rows of every chunk and the reduction in
    float64.  ``evaluate(first molecule, end molecule, row_mol int32 [rows] (chunk-local, non-decreasing), row_mask uint64 [rows])``
    returns the values [rows, C] of a chunk.  Molecules in exact mode are handled per F, all at once; only the others one by one."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    n = counts.shape[0]
    mode, given, rows = coalition_design(counts, additive, exact_max, samples, permutations)
    chunks = plan_coalition_chunks(rows, batch_size, max_rows)
    offsets = offsets_of(counts)
    is_exact = mode == "exact"
    pred = base = phi = stderr = None
    exact = mode != "sampled"
    values = [None] * n if return_values else None
    for b, e in chunks:
        first = offsets_of(rows[b:e])
        row_mol = np.repeat(np.arange(e - b, dtype=np.int32), rows[b:e])
        row_mask = (np.arange(first[-1], dtype=np.int64) - np.repeat(first[:-1], rows[b:e])).astype(np.uint64)      # exact mode: the row index
        others = (b + np.flatnonzero(~is_exact[b:e])).tolist()
        perms_of = {}
        for i in others:
            F, lo = int(counts[i]), int(first[i - b])
            if additive:
                full = _full_mask(F)
                row_mask[lo], row_mask[lo + 1] = 0, full
                row_mask[lo + 2: lo + 2 + F] = full ^ np.left_shift(np.uint64(1), np.arange(F, dtype=np.uint64))
            else:
                perms_of[i] = given[i] if i in given else draw_permutations(F, samples, seed, i)
                row_mask[lo: lo + int(rows[i])] = permutation_masks(perms_of[i])
        v = np.asarray(evaluate(b, e, row_mol, row_mask))
        if v.ndim != 2 or v.shape[0] != first[-1]:
            raise ValueError(f"fragment_shapley: {first[-1]} rows went in, values of shape {v.shape} came back")
        if phi is None:
            C = v.shape[1]
            pred, base = np.empty((n, C), dtype=v.dtype), np.empty((n, C), dtype=v.dtype)
            phi, stderr = np.zeros((int(offsets[-1]), C), dtype=np.float64), np.zeros((int(offsets[-1]), C), dtype=np.float64)
        v64 = v.astype(np.float64)
        local = np.arange(b, e)
        for F in np.unique(counts[b:e][is_exact[b:e]]).tolist():          # all exact molecules of one F at once
            sel = local[is_exact[b:e] & (counts[b:e] == F)]
            at = first[sel - b][:, None] + np.arange(1 << F)
            pred[sel], base[sel] = v[at[:, -1]], v[at[:, 0]]
            if F:
                phi[(offsets[sel][:, None] + np.arange(F)).reshape(-1)] = shapley_exact(v64[at], F).reshape(-1, v.shape[1])
        for i in others:
            F, lo, g0 = int(counts[i]), int(first[i - b]), int(offsets[i])
            base[i], pred[i] = v[lo], v[lo + 1]
            if additive:
                phi[g0: g0 + F] = v64[lo + 1] - v64[lo + 2: lo + 2 + F]
            else:
                phi[g0: g0 + F], stderr[g0: g0 + F] = shapley_sampled(v64[lo: lo + int(rows[i])], perms_of[i], paired=i not in given)
        if return_values:
            for i in range(b, e):
                lo = int(first[i - b])
                values[i] = {"mask": row_mask[lo: lo + int(rows[i])].copy(), "value": v[lo: lo + int(rows[i])].copy()}
    return dict(pred=pred, base=base, offsets=offsets, phi=phi, stderr=stderr, exact=exact, values=values, rows=rows, chunks=chunks)


def _spread_to_atoms(table, group, offsets, atom_group, atom_offsets, i):
    """[n_atoms of molecule i, C]: every atom carries its group's row of ``table``, an atom in no group 0 (model_attr.py:767-781)."""
    lo, hi = int(offsets[i]), int(offsets[i + 1])
    g = atom_group[int(atom_offsets[i]): int(atom_offsets[i + 1])]
    out = np.zeros((g.shape[0], table.shape[1]), dtype=table.dtype)
    if hi > lo:
        pos = np.minimum(np.searchsorted(group[lo:hi], g), hi - lo - 1)          # the molecule's ids are ascending
        hit = group[lo:hi][pos] == g
        out[hit] = table[lo:hi][pos[hit]]
    return out


class FragmentShapley(_GroupResult):
    """Result of ``fragment_shapley``.  ``pred [n, C]`` = v(all groups), ``base [n, C]`` = v(no group); rows ``offsets[i] : offsets[i + 1]``
    of ``group`` / ``n_atoms`` / ``phi`` / ``stderr`` (float64 ``[R, C]``) are molecule i's groups in ascending order; ``exact [n]``: the
    molecule's values are exact (``stderr`` 0), not a permutation sample.  ``result[i]`` is molecule i as a dict, ``atom_weights(i)`` its
    phi spread over its atoms, ``arrays()`` what the command-line script writes.  ``values`` (``return_values=True``): per molecule
    ``{"mask": uint64 [rows], "value": [rows, C]}``, every evaluated coalition."""

    _per_group = "phi"

    def __init__(self, pred, base, offsets, group, n_atoms, phi, stderr, exact, atom_group, atom_offsets, values=None):
        self._set_groups(offsets, group, n_atoms, atom_group, atom_offsets)
        self.pred, self.base, self.phi, self.stderr, self.exact, self.values = pred, base, phi, stderr, exact, values

    def __getitem__(self, i: int) -> dict:
        i = self._index(i)
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        return {"pred": self.pred[i], "base": self.base[i], "group": self.group[lo:hi], "n_atoms": self.n_atoms[lo:hi],
                "phi": self.phi[lo:hi], "stderr": self.stderr[lo:hi], "exact": bool(self.exact[i])}

    def arrays(self) -> Dict[str, np.ndarray]:
        return {"pred": self.pred, "base": self.base, "offsets": self.offsets, "group": self.group, "n_atoms": self.n_atoms, "phi": self.phi,
                "stderr": self.stderr, "exact": self.exact, "atom_offsets": self.atom_offsets, "atom_group": self.atom_group}


def atom_bits(flat, atom_off, table) -> np.ndarray:
    """int8 [N]: for every atom the position of its group among its molecule's groups (ascending ids: the order of ``flat_group_table``),
    -1 for an atom in no group."""
    rep_mol, ids, _, counts = table
    flat = np.asarray(flat, dtype=np.int64)
    n = atom_off.shape[0] - 1
    out = np.full(flat.shape[0], -1, dtype=np.int8)
    keep = np.flatnonzero(flat >= 0)
    if keep.size:
        span = int(ids.max()) + 1
        if n * span >= 1 << 62:
            raise ValueError("fragment_shapley: group ids too large to index (molecules x largest id must stay below 2^62)")
        mol = np.repeat(np.arange(n, dtype=np.int64), np.diff(atom_off))[keep]
        first = offsets_of(counts)
        pos = np.searchsorted(rep_mol * span + ids, mol * span + flat[keep]) - first[mol]
        if counts.max() > 64:
            i = int(np.argmax(counts > 64))
            raise ValueError(f"fragment_shapley: molecule {i} has {int(counts[i])} groups; a coalition mask holds 64")
        out[keep] = pos.astype(np.int8)
    return out


def fragment_shapley(model, source, groups=None, batch_size: int = 512, exact_max: int = 10, samples: int = 256, seed: int = 0,
                     permutations=None, max_rows: int = DEFAULT_SHAPLEY_ROWS, return_values: bool = False) -> FragmentShapley:
    """Shapley values of the fragments (or ``groups``) of every molecule of ``source`` under ``model`` on the GPU; models, sources and
    the ``groups`` convention are ``fragment_contributions``'.  The set function: v(S) = the prediction with the atoms of every group
    outside S zeroed behind the encoder (ungrouped atoms and the fragment rows always stay); ``pred`` = v(all), ``base`` = v(none), and
    sum_f phi_f = pred - base.

    A molecule with F <= ``exact_max`` groups is enumerated (2^F rows, phi exact); one with more is sampled: ``samples`` permutations in
    antithetic pairs from ``np.random.default_rng([seed, molecule index])`` -- so its answer does not depend on ``batch_size``, on its
    neighbours or on chunking -- phi the mean marginal, ``stderr`` the standard error over the pair means.  ``permutations={molecule:
    int array [K, F]}`` replaces the draw for those molecules whatever their F (``stderr`` then over the K permutations).  At most 64
    groups per molecule.

    The pair models (``cdrp.CDRPModel``, ``dta.DTAModel2``): their head is ``fc2(fc1(cat(enc, second)))`` with nothing between the two
    Linears, so v is ADDITIVE in the groups and a group's Shapley value is its leave-one-out contribution v(all) - v(all but f).  Nothing
    is enumerated for them: rows full, empty and all-but-one per group, flagged exact.

    Per chunk (a run of at most ``batch_size`` molecules whose rows sum to at most ``max_rows``; a molecule's rows are never split): one
    evaluation encoder pass, ONE coalition read-out, head calls over slices of ``ops.DENSE_MAX_ROWS`` rows, one upload of the rows.  The
    reduction over rows runs on the host in float64."""
    import torch
    from . import data, ops
    kind = _contribution_kind(model)
    additive = kind in ("drp", "dta")
    design_args = dict(additive=additive, batch_size=batch_size, exact_max=exact_max, samples=samples, seed=seed, permutations=permutations,
                       max_rows=max_rows, return_values=return_values)
    store, records, collate, flat, atom_off, table, device = _group_source("fragment_shapley", kind, model, source, groups)
    rep_mol, ids, sizes, counts = table
    if store is not None and groups is None:          # the fragment map of a store: derived once and kept on it, like its replica table
        bits = kept_on_store(store, "_frag_bits_cpu", lambda: atom_bits(flat, atom_off, table))
    else:
        bits = atom_bits(flat, atom_off, table)

    def evaluate(b, e, row_mol, row_mask):
        R, N = row_mol.shape[0], int(atom_off[e] - atom_off[b])
        upload = PackedUpload([(np.int64, R), (np.int32, R), (np.int8, N)])          # one upload: [masks | molecules | atom bits]
        upload.host[0][:] = row_mask.view(np.int64)
        upload.host[1][:] = row_mol
        upload.host[2][:] = bits[int(atom_off[b]): int(atom_off[e])]
        mask_d, mol_d, bit_d = upload.to(device)
        batch = store.collate(np.arange(b, e)) if store is not None else data.batch_to(collate(records[b:e]), device)
        read_out = lambda xa, xf, plan: ops.pool_cat_coalitions(xa, xf, plan, bit_d, mol_d, mask_d, check=False)      # rows built here
        return _contribution_rows(kind, model, batch, read_out, mol_d, head_rows=ops.DENSE_MAX_ROWS).cpu().numpy()

    with evaluation(model), torch.no_grad():
        r = _shapley_host(counts, evaluate, **design_args)
    return FragmentShapley(r["pred"], r["base"], r["offsets"], ids, sizes, r["phi"], r["stderr"], r["exact"], flat, atom_off, r["values"])
