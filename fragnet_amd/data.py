"""Batch assembly: per-molecule records -> the 16/19-key batch dict the model consumes.

Counterpart of the reference's ``collate_fn`` / ``collate_fn_pt``
(fragnet/dataset/data.py:877-948, 951-1032) and its five ``get_incr_*`` helpers
(data.py:11-113).  Same keys, dtypes and integer values (bit-exact; pinned by
tests/golden/collate_*.npz), but the per-molecule offsets are one ``cumsum`` +
``repeat_interleave`` per index space instead of Python loops over ``torch.cat``.

Index spaces and what offsets them:
  atoms        edge_index              += sum of previous x_atoms.size(0)
  fragments    frag_index, a2f         += sum of previous n_frags
  bond nodes   edge_index_bonds_graph  += sum of previous node_features_bonds.size(0)
  fbond nodes  edge_index_fbonds       += sum of previous node_feautures_fbondg.size(0)

The reference accumulates the first three offsets in float32 and casts to int64 at the
end (data.py:883,933-942); that is exact only below 2**24 nodes, so this collate refuses
larger batches instead of reproducing index collisions.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch

from .plan import N_MOLS_KEY, CollatedBatch, batch_n_mols, mol_offsets

_F32_EXACT = 1 << 24


def _offsets(counts: Sequence[int], reps: Sequence[int]) -> torch.Tensor:
    """For molecule i: (sum of counts[:i]) repeated reps[i] times, int64."""
    c = torch.as_tensor(list(counts), dtype=torch.long)
    r = torch.as_tensor(list(reps), dtype=torch.long)
    start = torch.cumsum(c, 0) - c
    return torch.repeat_interleave(start, r)


def _collate_common(data_list: List) -> Dict[str, torch.Tensor]:
    if len(data_list) == 0:
        raise ValueError("collate_fn: empty data_list")
    n_atoms = [int(d.x_atoms.size(0)) for d in data_list]
    n_frags = [int(d.n_frags.item()) for d in data_list]
    n_bnodes = [int(d.node_features_bonds.size(0)) for d in data_list]
    n_fbnodes = [int(d.node_feautures_fbondg.size(0)) for d in data_list]
    if max(sum(n_atoms), sum(n_frags), sum(n_bnodes)) >= _F32_EXACT:
        raise ValueError("batch exceeds 2**24 nodes: the reference's float32 offsets are inexact there")

    e = [int(d.edge_index.shape[1]) for d in data_list]
    ef = [int(d.frag_index.shape[1]) for d in data_list]
    eb = [int(d.edge_index_bonds.shape[1]) for d in data_list]
    efb = [int(d.edge_index_fbondg.shape[1]) for d in data_list]

    cat0 = lambda name: torch.cat([getattr(d, name) for d in data_list], dim=0)
    cat1 = lambda name: torch.cat([getattr(d, name) for d in data_list], dim=1)

    mol_id = torch.arange(len(data_list), dtype=torch.long)
    out = CollatedBatch({
        "x_atoms": cat0("x_atoms"),
        "edge_index": cat1("edge_index").to(torch.long) + _offsets(n_atoms, e),
        "frag_index": cat1("frag_index").to(torch.long) + _offsets(n_frags, ef),
        "x_frags": cat0("x_frags"),
        "edge_attr": cat0("edge_attr"),
        "cnx_attr": cat0("cnx_attr"),
        "batch": torch.repeat_interleave(mol_id, torch.as_tensor(n_atoms)),
        "frag_batch": torch.repeat_interleave(mol_id, torch.as_tensor(n_frags)),
        "atom_to_frag_ids": cat0("atom_id_frag_id").to(torch.long) + _offsets(n_frags, n_atoms),
        "node_features_bonds": cat0("node_features_bonds"),
        "edge_index_bonds_graph": cat1("edge_index_bonds").to(torch.long) + _offsets(n_bnodes, eb),
        "edge_attr_bonds": cat0("edge_attr_bonds"),
        "node_features_fbonds": cat0("node_feautures_fbondg"),
        "edge_index_fbonds": cat1("edge_index_fbondg").to(torch.long) + _offsets(n_fbnodes, efb),
        "edge_attr_fbonds": cat0("edge_attr_fbondg"),
    })
    # the cumulative counts as a table (plan.CollatedBatch): the one-launch graph-plan builder is driven by it
    per_mol = {"atom": n_atoms, "edge": e, "bedge": eb, "frag": n_frags, "fedge": ef, "fbedge": efb}
    out.offsets = mol_offsets({k: torch.as_tensor(v, dtype=torch.long) for k, v in per_mol.items()})
    out.max_per_mol = {k: max(v) for k, v in per_mol.items()}
    out.max_per_mol["mol"] = 1
    if getattr(data_list[0], "positions", None) is not None:      # one conformer per record: the geometry keys can be derived from it (batch_to)
        out["positions"] = cat0("positions").to(torch.float)
    return out


def collate_fn(data_list: List) -> Dict[str, torch.Tensor]:
    """Finetune batch dict (16 keys) -- reference data.py:877-948."""
    out = _collate_common(data_list)
    out["y"] = torch.cat([d.y for d in data_list], dim=0).type(torch.float)
    return out


def collate_fn_pt(data_list: List) -> Dict[str, torch.Tensor]:
    """Pretrain batch dict (19 keys) -- reference data.py:951-1032."""
    out = _collate_common(data_list)
    out["bnd_lngth"] = torch.cat([d.bnd_lngth for d in data_list], dim=0)
    out["bnd_angl"] = torch.cat([d.bnd_angl for d in data_list], dim=0)
    out["dh_angl"] = torch.cat([d.dh_angl for d in data_list], dim=0)
    out["y"] = torch.cat([d.y for d in data_list], dim=0).type(torch.float)
    return out


BATCH_KEYS_FT = (
    "x_atoms", "edge_index", "frag_index", "x_frags", "edge_attr", "cnx_attr", "batch",
    "frag_batch", "atom_to_frag_ids", "node_features_bonds", "edge_index_bonds_graph",
    "edge_attr_bonds", "node_features_fbonds", "edge_index_fbonds", "edge_attr_fbonds", "y",
)
BATCH_KEYS_PT = BATCH_KEYS_FT[:-1] + ("bnd_lngth", "bnd_angl", "dh_angl", "y")


def batch_to(batch: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """``batch[k] = batch[k].to(device)`` for every key -- reference train/utils.py:335-336.  A batch collated from a
    store without its bond-graph index (dataset.FlatMolStore.without_bond_graph_index) gets ``edge_index_bonds_graph``
    rebuilt from ``edge_index`` once it is on the GPU (ops.bond_graph)."""
    out = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
    if isinstance(batch, CollatedBatch):         # the layout promise (and the offsets table) travels with the batch
        out = batch.like(out)
        if out.offsets is not None:
            out.offsets = out.offsets.to(device)
    if "edge_index_bonds_graph" not in out and "edge_index" in out and out["edge_index"].is_cuda:
        from . import ops
        out["edge_index_bonds_graph"] = ops.bond_graph(out["edge_index"], out["batch"], batch_n_mols(out))
    if "edge_index_fbonds" not in out and "frag_index" in out and out["frag_index"].is_cuda:
        from . import ops
        eifb = ops.bond_graph(out["frag_index"], out["frag_batch"], batch_n_mols(out), fragments=True)
        out["edge_index_fbonds"] = eifb
        out["edge_attr_fbonds"] = out["node_features_fbonds"][eifb[0]] + out["node_features_fbonds"][eifb[1]]
    if "positions" in out and out["positions"].is_cuda and "edge_index_bonds_graph" in out:
        # a batch collated from a store that keeps coordinates instead of the tensors derived from them (FlatMolStore.without_geometry)
        from . import ops
        if "edge_attr_bonds" not in out:
            out["edge_attr_bonds"] = ops.bond_cos(out["positions"], out["edge_index"], out["edge_index_bonds_graph"])
        if "bnd_lngth" not in out:
            m = getattr(out, "max_per_mol", None)
            out["bnd_lngth"], out["bnd_angl"], out["dh_angl"] = ops.pretrain_geometry(
                out["positions"], out["edge_index"], out["batch"], batch_n_mols(out),
                max_per_mol=(m["atom"], m["edge"]) if m else None)
    return out


def collate_fn_cdrp(data_list: List) -> Dict[str, torch.Tensor]:
    """Cancer-drug-response batch dict (17 keys) -- reference data.py:1112-1187: the finetune batch plus ``gene_expr`` [B, gene_dim],
    each record's ``gene_expr.view(1, -1)`` stacked and cast with ``.type(torch.long)`` exactly as the reference does (truncation toward
    zero; the model casts it back with ``.float()``, and the tower's first kernel reads the int64 rows directly)."""
    out = _collate_common(data_list)
    out["y"] = torch.cat([d.y for d in data_list], dim=0).type(torch.float)
    out["gene_expr"] = torch.cat([d.gene_expr.view(1, -1) for d in data_list], dim=0).type(torch.long)
    return out


BATCH_KEYS_CDRP = BATCH_KEYS_FT + ("gene_expr",)


DTA_VOCAB = 26           # nn.Embedding(25 + 1, 300) of DTAModel2: token 0 is the padding behind a sequence, 1..25 the residues


def collate_fn_dta(data_list: List) -> Dict[str, torch.Tensor]:
    """Drug-target-affinity batch dict (17 keys) -- reference data.py:1035-1109: the finetune batch plus ``protein`` [B, length], each
    record's ``protein.view(1, -1)`` stacked and cast with ``.type(torch.long)`` exactly as the reference does.  A token outside
    [0, 25] raises ValueError here, on the host: the reference's nn.Embedding raises for it, the protein-tower kernels cannot (they
    skip such a position instead of indexing with it)."""
    out = _collate_common(data_list)
    out["y"] = torch.cat([d.y for d in data_list], dim=0).type(torch.float)
    protein = torch.cat([d.protein.view(1, -1) for d in data_list], dim=0).type(torch.long)
    if protein.numel() and (int(protein.min()) < 0 or int(protein.max()) >= DTA_VOCAB):
        raise ValueError(f"collate_fn_dta: protein tokens must lie in [0, {DTA_VOCAB - 1}] (got {int(protein.min())} .. {int(protein.max())})")
    out["protein"] = protein
    return out


BATCH_KEYS_DTA = BATCH_KEYS_FT + ("protein",)


# ------------------------------------------------------------------------------------ factored pair batches
# A drug-response or drug-target table has many rows over few distinct drugs and second inputs.  A factored batch holds every distinct
# input ONCE -- the molecule keys describe the U distinct drugs, ``gene_expr`` / ``protein`` the C distinct second inputs, both in order
# of first occurrence -- and says which pair uses which: ``pair_drug`` [M], ``pair_second`` [M] (int64), ``y`` [M] in data_list order.
# The models then run the encoder on U molecules, the tower on C rows and the factored pair head (ops.pair_head_factored).
PAIR_DRUG_KEY, PAIR_SECOND_KEY = "pair_drug", "pair_second"
PAIR_ORDER_KEYS = ("pair_drug_rowptr", "pair_drug_perm", "pair_second_rowptr", "pair_second_perm")      # int32: ops.pair_orderings
PAIR_GRID_KEY = "_pair_grid"         # python bool: no pair lists, the models return every drug against every second input, [U, C]

# every tensor _collate_common reads from a record
_MOL_FIELDS = ("x_atoms", "n_frags", "node_features_bonds", "node_feautures_fbondg", "edge_index", "frag_index", "edge_index_bonds",
               "edge_index_fbondg", "x_frags", "edge_attr", "cnx_attr", "atom_id_frag_id", "edge_attr_bonds", "edge_attr_fbondg", "positions")


def _digest(tensors) -> bytes:
    """A content key: dtype, shape and bytes of every tensor (None: absent).  ``smiles`` plays no part: synthetic records leave it empty."""
    import hashlib
    h = hashlib.blake2b(digest_size=16)
    for t in tensors:
        if t is None:
            h.update(b"-;")
            continue
        t = t.detach().cpu().contiguous()
        h.update(f"{t.dtype}{tuple(t.shape)};".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.digest()


def _first_occurrence(keys):
    """(indices of the first occurrence of every distinct key, in order; for every key the position of its first occurrence in that list)"""
    seen, first, which = {}, [], []
    for i, k in enumerate(keys):
        if k not in seen:
            seen[k] = len(first)
            first.append(i)
        which.append(seen[k])
    return first, torch.as_tensor(which, dtype=torch.long)


def _orderings_host(pair_list: torch.Tensor, n_rows: int):
    """ops.pair_orderings on the host: a stable sort of the pair list, so ascending pair index inside a row."""
    perm = torch.sort(pair_list, stable=True)[1].to(torch.int32)
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.bincount(pair_list, minlength=n_rows), 0)
    return rowptr, perm


def _check_tokens(protein, who):
    if protein.numel() and (int(protein.min()) < 0 or int(protein.max()) >= DTA_VOCAB):
        raise ValueError(f"{who}: protein tokens must lie in [0, {DTA_VOCAB - 1}] (got {int(protein.min())} .. {int(protein.max())})")


def _collate_factored(data_list: List, field: str, key: str, who: str) -> Dict[str, torch.Tensor]:
    if len(data_list) == 0:
        raise ValueError(f"{who}: empty data_list")
    rows = [getattr(d, field).view(1, -1).type(torch.long) for d in data_list]          # exactly what collate_fn_cdrp / _dta emit
    first_d, pair_drug = _first_occurrence([_digest(getattr(d, f, None) for f in _MOL_FIELDS) for d in data_list])
    first_s, pair_second = _first_occurrence([_digest((r,)) for r in rows])
    out = _collate_common([data_list[i] for i in first_d])
    out["y"] = torch.cat([d.y for d in data_list], dim=0).type(torch.float)
    second = torch.cat([rows[i] for i in first_s], dim=0)
    if key == "protein":
        _check_tokens(second, who)
    out[key] = second
    out[PAIR_DRUG_KEY], out[PAIR_SECOND_KEY] = pair_drug, pair_second
    for k, v in zip(PAIR_ORDER_KEYS, _orderings_host(pair_drug, len(first_d)) + _orderings_host(pair_second, len(first_s))):
        out[k] = v
    out[N_MOLS_KEY] = len(first_d)
    return out


def collate_fn_cdrp_factored(data_list: List) -> Dict[str, torch.Tensor]:
    """``collate_fn_cdrp`` without the copies: the molecule keys hold the U DISTINCT drugs of ``data_list`` and ``gene_expr`` [C, gene_dim]
    its C distinct cell lines, each in order of first occurrence; ``pair_drug`` / ``pair_second`` [M] int64 say which pair uses which,
    ``y`` [M] is in ``data_list`` order.  Distinct means different CONTENT: every tensor the collate reads from the record for a drug,
    the int64 row as ``collate_fn_cdrp`` emits it (after the truncating cast) for a cell line; ``smiles`` is not looked at.  Also carried:
    the pair orderings of the head's backward (``PAIR_ORDER_KEYS``) and the molecule count (``plan.N_MOLS_KEY``: ``y`` has M entries)."""
    return _collate_factored(data_list, "gene_expr", "gene_expr", "collate_fn_cdrp_factored")


def collate_fn_dta_factored(data_list: List) -> Dict[str, torch.Tensor]:
    """``collate_fn_dta`` without the copies (``collate_fn_cdrp_factored``): ``protein`` [C, length] holds the distinct token rows.  A token
    outside [0, 25] raises ValueError, as in ``collate_fn_dta``."""
    return _collate_factored(data_list, "protein", "protein", "collate_fn_dta_factored")


def pair_grid_batch(drug_records: List, second_rows, kind: str) -> Dict[str, torch.Tensor]:
    """A screening batch: U drug records and C second inputs (``kind`` "cdrp": gene-expression rows, "dta": token rows; a [C, n] tensor or
    a list of rows), no pair lists and no ``y``.  ``CDRPModel`` / ``DTAModel2`` return [U, C] for it: every drug against every second input."""
    if kind not in ("cdrp", "dta"):
        raise ValueError(f"pair_grid_batch: kind must be 'cdrp' or 'dta' (got {kind!r})")
    out = _collate_common(list(drug_records))
    if torch.is_tensor(second_rows) and second_rows.dim() == 2:
        second = second_rows.type(torch.long)
    else:
        second = torch.cat([torch.as_tensor(r).view(1, -1) for r in second_rows], dim=0).type(torch.long)
    if kind == "dta":
        _check_tokens(second, "pair_grid_batch")
    out["gene_expr" if kind == "cdrp" else "protein"] = second
    out[PAIR_GRID_KEY] = True
    out[N_MOLS_KEY] = len(drug_records)
    return out


def as_factored(batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """An already collated pair batch (``collate_fn_cdrp`` / ``collate_fn_dta``: one molecule and one second row per pair) with the
    identity pair lists, so that the models take the factored path on it.  The tensors are shared, not copied."""
    M = int(batch["y"].shape[0])
    dev = batch["y"].device
    out = batch.like(dict(batch)) if isinstance(batch, CollatedBatch) else dict(batch)
    out[PAIR_DRUG_KEY] = torch.arange(M, dtype=torch.long, device=dev)
    out[PAIR_SECOND_KEY] = torch.arange(M, dtype=torch.long, device=dev)
    rowptr, perm = torch.arange(M + 1, dtype=torch.int32, device=dev), torch.arange(M, dtype=torch.int32, device=dev)
    for k, v in zip(PAIR_ORDER_KEYS, (rowptr, perm, rowptr, perm)):
        out[k] = v
    out[N_MOLS_KEY] = M
    return out
