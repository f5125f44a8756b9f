"""Deterministic synthetic molecule generator (SURVEY.md §8d "Concrete synthetic inputs").

There is no RDKit and no dataset in the build image, so "ESOL-shape" is *defined* by
this generator: a random valence-capped heavy-atom tree, 0-2 ring closures, explicit H
atoms, the bond graph / fragment graph / fragment-bond graph built by the same rules the
reference's offline featuriser uses, and random features of the reference's widths.

Topology rules restated from the reference (no code copied):
  * directed ``edge_index``: every bond twice, (a->b, b->a) interleaved
    -- reference fragnet/dataset/feature_utils.py:285-296
  * bond graph: ordered pairs (i, j) of directed bonds sharing exactly one atom
    -- reference fragnet/dataset/data.py:116-128; two-atom components get the pair of
    mutual edges with attribute 1 -- data.py:157-182,192-195
  * fragments numbered by smallest atom index (RDKit ``GetMolFrags`` order);
    ``atom_id_frag_id`` in atom order -- fragnet/dataset/fragments.py:205-252
  * one connection per cut bond, both directions; a single-fragment molecule gets the
    one self connection (0, 0) -- data.py:505-538, fragments.py:230-234;
    disconnected components are linked by extra connections -- fragments.py:236-240,274-300
  * fragment-bond graph: 2-node special case, otherwise "share exactly one fragment"
    -- data.py:131-154; its edge attribute is the sum of the two node features -- data.py:291-303

A record is a ``MolRecord`` with the attribute names of the reference's per-molecule
``Data`` object (data.py:437-480) so that the reference's own ``collate_fn`` can consume
it when golden vectors are generated.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

ATOM_F = 167   # exps/ft/esol/e1pt4.yaml:8
EDGE_F = 17    # exps/ft/esol/e1pt4.yaml:10
CNX_F = 6      # fedge_in / fbond_edge_in, e1pt4.yaml:11-12

# name -> (mu heavy atoms, p_cut, n_tasks)   -- SURVEY.md §8d profiles
PROFILES = {
    "esol": (10.5, 0.35, 0),
    "tox21": (14.5, 0.35, 12),
    "synth40": (16.0, 0.78, 0),
}


@dataclass
class MolRecord:
    """Per-molecule tensors, attribute names as in the reference ``Data`` item."""
    x_atoms: torch.Tensor                # [n, 167] f32
    edge_index: torch.Tensor             # [2, e]  i64   row0=src,row1=dst
    edge_attr: torch.Tensor              # [e, 17] f32
    frag_index: torch.Tensor             # [2, ef] i64
    cnx_attr: torch.Tensor               # [ef, 6] f32
    x_frags: torch.Tensor                # [f, 167] f32
    atom_id_frag_id: torch.Tensor        # [n] i64
    n_frags: torch.Tensor                # [1] i64
    node_features_bonds: torch.Tensor    # [e, 17] f32
    edge_index_bonds: torch.Tensor       # [2, eb] i32
    edge_attr_bonds: torch.Tensor        # [eb, 1] f32
    node_feautures_fbondg: torch.Tensor  # [ef, 6] f32   (sic: reference spelling)
    edge_index_fbondg: torch.Tensor      # [2, efb] i32
    edge_attr_fbondg: torch.Tensor       # [efb, 6] f32
    y: torch.Tensor                      # [1] or [1, T] f32
    bnd_lngth: Optional[torch.Tensor] = None   # [e, 1]
    bnd_angl: Optional[torch.Tensor] = None    # [n, 1]
    dh_angl: Optional[torch.Tensor] = None     # [e, 1]
    smiles: str = ""
    positions: Optional[torch.Tensor] = None   # [n, 3] f32: one conformer (attach_positions)


def bond_graph_pairs(ends: np.ndarray) -> np.ndarray:
    """Ordered pairs (i, j), i-major, of rows of ``ends`` ([k, 2]) sharing exactly one id."""
    k = ends.shape[0]
    if k == 0:
        return np.zeros((2, 0), dtype=np.int64)
    a = ends[:, 0][:, None]
    b = ends[:, 1][:, None]
    c = ends[:, 0][None, :]
    d = ends[:, 1][None, :]
    # |set(b_i) & set(b_j)| for 2-element lists (elements of one row may coincide: self edge)
    same_i = (ends[:, 0] == ends[:, 1])
    n_common = np.zeros((k, k), dtype=np.int64)
    # distinct elements of row i that also occur in row j
    in_j_a = (a == c) | (a == d)
    in_j_b = (b == c) | (b == d)
    n_common = in_j_a.astype(np.int64) + (in_j_b & ~same_i[:, None]).astype(np.int64)
    ii, jj = np.nonzero(n_common == 1)
    return np.stack([ii, jj]).astype(np.int64)


def fbond_graph_pairs(ends: np.ndarray) -> np.ndarray:
    """Fragment-bond graph: the reference's 2-node special case, else 'share exactly one'."""
    k = ends.shape[0]
    if k == 2:
        rows = [[], []]
        for i in range(2):
            for j in range(2):
                if not (ends[i, 0] == ends[j, 0] and ends[i, 1] == ends[j, 1]):
                    rows[0].append(i)
                    rows[1].append(j)
        return np.asarray(rows, dtype=np.int64).reshape(2, -1)
    return bond_graph_pairs(ends)


def _components(n: int, bonds: List[tuple]) -> np.ndarray:
    """Connected-component label per atom, components numbered by smallest atom index."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in bonds:
        ra, rb = find(a), find(b)
        if ra != rb:
            if ra < rb:
                parent[rb] = ra
            else:
                parent[ra] = rb
    roots = np.array([find(i) for i in range(n)])
    _, labels = np.unique(roots, return_inverse=True)   # roots are the smallest members
    return labels.astype(np.int64)


def _multi_hot(rng, rows: int, width: int, ones: int) -> np.ndarray:
    out = np.zeros((rows, width), dtype=np.float32)
    if rows:
        cols = np.argsort(rng.random((rows, width)), axis=1)[:, :ones]
        np.put_along_axis(out, cols, 1.0, axis=1)
    return out


def make_topology(rng, mu: float, p_cut: float, p_salt: float = 0.0):
    """Returns (n_atoms, bonds[list of (a,b)], cut[list of bool per bond])."""
    n_heavy = max(2, int(rng.poisson(mu)))
    cap = rng.choice([4, 3, 2, 1], size=n_heavy, p=[0.70, 0.10, 0.15, 0.05])
    cap[0] = max(cap[0], 1)
    deg = np.zeros(n_heavy, dtype=np.int64)
    bonds: List[tuple] = []
    for i in range(1, n_heavy):
        free = np.nonzero(deg[:i] < cap[:i])[0]
        if free.size == 0:           # every earlier atom is saturated: widen the newest one
            j = i - 1
            cap[j] = deg[j] + 1
        else:
            j = int(free[rng.integers(free.size)])
        bonds.append((j, i))
        deg[j] += 1
        deg[i] += 1
        cap[i] = max(cap[i], 1)
    n_tree = len(bonds)
    in_ring = [False] * n_tree
    # 0-2 ring closures between non-adjacent atoms with free valence
    for _ in range(int(rng.integers(0, 3))):
        free = np.nonzero(deg < cap)[0]
        if free.size < 2:
            break
        a, b = (int(v) for v in rng.choice(free, size=2, replace=False))
        if a > b:
            a, b = b, a
        if (a, b) in bonds or (b, a) in bonds:
            continue
        # tree path a..b becomes cyclic: those bonds may no longer be cut
        par = {}
        for k, (p, c) in enumerate(bonds[:n_tree]):
            par[c] = (p, k)
        anc_a = {a: None}
        x = a
        while x in par:
            x = par[x][0]
            anc_a[x] = None
        y = b
        path_b = []
        while y not in anc_a:
            p, k = par[y]
            path_b.append(k)
            y = p
        x = a
        while x != y:
            p, k = par[x]
            in_ring[k] = True
            x = p
        for k in path_b:
            in_ring[k] = True
        bonds.append((a, b))
        in_ring.append(True)
        deg[a] += 1
        deg[b] += 1
    n_heavy_bonds = len(bonds)
    cut = [(not in_ring[k]) and (rng.random() < p_cut) for k in range(n_heavy_bonds)]
    # explicit hydrogens fill the remaining valence
    n = n_heavy
    for a in range(n_heavy):
        for _ in range(int(cap[a] - deg[a])):
            bonds.append((a, n))
            cut.append(False)
            n += 1
    salt_atoms = 0
    if p_salt > 0 and rng.random() < p_salt:
        if rng.random() < 0.5:        # lone counter-ion (no bonds)
            # must not be the last atom: the reference rejects a molecule whose last atom
            # has no bond (data.py:368-371).  Insert by swapping ids with the last atom.
            salt_atoms = 1
        else:                          # two-atom component (one-bond fragment)
            bonds.append((n, n + 1))
            cut.append(False)
            n += 2
    if salt_atoms:
        # new atom takes the id of the current last atom; the last atom moves to the end
        last = n - 1
        ion = last
        moved = n
        bonds = [((moved if a == last else a), (moved if b == last else b)) for a, b in bonds]
        n += 1
        _ = ion
    return n, bonds, cut


def make_molecule(rng, mu: float = 10.5, p_cut: float = 0.35, n_tasks: int = 0,
                  pretrain_targets: bool = False, p_salt: float = 0.0,
                  topology=None) -> MolRecord:
    if topology is None:
        n, bonds, cut = make_topology(rng, mu, p_cut, p_salt)
    else:
        n, bonds, cut = topology
    nb = len(bonds)
    e = 2 * nb
    src = np.empty(e, dtype=np.int64)
    dst = np.empty(e, dtype=np.int64)
    barr = np.asarray(bonds, dtype=np.int64).reshape(nb, 2)
    src[0::2], dst[0::2] = barr[:, 0], barr[:, 1]
    src[1::2], dst[1::2] = barr[:, 1], barr[:, 0]
    edge_index = np.stack([src, dst])
    ends = edge_index.T.copy()                      # bond-graph node k = directed edge k

    # ---- bond graph
    eib = bond_graph_pairs(ends)
    cos = rng.uniform(-1.0, 1.0, size=eib.shape[1])
    mol_comp = _components(n, bonds)
    comp_size = np.bincount(mol_comp, minlength=mol_comp.max() + 1)
    extra = [[], []]
    for k in range(nb):
        a, b = bonds[k]
        if comp_size[mol_comp[a]] == 2:
            extra[0] += [2 * k, 2 * k + 1]
            extra[1] += [2 * k + 1, 2 * k]
    if extra[0]:
        eib = np.concatenate([eib, np.asarray(extra, dtype=np.int64)], axis=1)
        cos = np.concatenate([cos, np.ones(len(extra[0]))])

    # ---- fragments
    kept = [bonds[k] for k in range(nb) if not cut[k]]
    a2f = _components(n, kept)
    n_frags = int(a2f.max()) + 1
    cnx: List[tuple] = [(int(a2f[bonds[k][0]]), int(a2f[bonds[k][1]])) for k in range(nb) if cut[k]]
    if not cnx and n_frags == 1:
        cnx = [(0, 0)]
    n_mol_comp = int(mol_comp.max()) + 1
    if n_mol_comp > 1:
        frag_comp = np.zeros(n_frags, dtype=np.int64)
        frag_comp[a2f] = mol_comp
        have = {tuple(sorted(c)) for c in cnx}
        for ci in range(n_mol_comp):
            for cj in range(ci + 1, n_mol_comp):
                for fi in np.nonzero(frag_comp == ci)[0]:
                    for fj in np.nonzero(frag_comp == cj)[0]:
                        if tuple(sorted((int(fi), int(fj)))) not in have:
                            cnx.append((int(fi), int(fj)))
    one_hot_c = np.zeros((len(cnx), CNX_F), dtype=np.float32)
    one_hot_c[np.arange(len(cnx)), rng.integers(0, CNX_F, size=len(cnx))] = 1.0
    if n_frags == 1 and len(cnx) == 1 and cnx[0] == (0, 0):
        frag_index = np.asarray([[0], [0]], dtype=np.int64)
        cnx_attr = one_hot_c
    else:
        fs, fd, rows = [], [], []
        for k, (a, b) in enumerate(cnx):
            fs += [a, b]
            fd += [b, a]
            rows += [k, k]
        frag_index = np.asarray([fs, fd], dtype=np.int64)
        cnx_attr = one_hot_c[rows]
    fends = frag_index.T.copy()
    eifb = fbond_graph_pairs(fends)
    ea_fb = cnx_attr[eifb[0]] + cnx_attr[eifb[1]] if eifb.shape[1] else np.zeros((0, CNX_F), np.float32)

    # ---- features
    x_atoms = _multi_hot(rng, n, ATOM_F, 10)
    bond_feat = _multi_hot(rng, nb, EDGE_F, 5)
    edge_attr = np.repeat(bond_feat, 2, axis=0)
    x_frags = np.zeros((n_frags, ATOM_F), dtype=np.float32)
    np.add.at(x_frags, a2f, x_atoms)
    if n_tasks:
        y = rng.integers(-1, 2, size=(1, n_tasks)).astype(np.float32)
    else:
        y = rng.normal(size=(1,)).astype(np.float32)

    t = torch.from_numpy
    rec = MolRecord(
        x_atoms=t(x_atoms), edge_index=t(edge_index), edge_attr=t(edge_attr),
        frag_index=t(frag_index), cnx_attr=t(cnx_attr.astype(np.float32)), x_frags=t(x_frags),
        atom_id_frag_id=t(a2f), n_frags=torch.tensor([n_frags], dtype=torch.long),
        node_features_bonds=t(edge_attr.copy()),
        edge_index_bonds=t(eib.astype(np.int32)),
        edge_attr_bonds=t(cos.astype(np.float32).reshape(-1, 1)),
        node_feautures_fbondg=t(cnx_attr.astype(np.float32).copy()),
        edge_index_fbondg=t(eifb.astype(np.int32)),
        edge_attr_fbondg=t(ea_fb.astype(np.float32)),
        y=t(y),
    )
    if pretrain_targets:
        rec.bnd_lngth = t(rng.uniform(0.8, 2.5, size=(e, 1)).astype(np.float32))
        rec.bnd_angl = t(rng.uniform(0.0, 4.0, size=(n, 1)).astype(np.float32))
        rec.dh_angl = t(rng.uniform(-1.0, 1.0, size=(e, 1)).astype(np.float32))
    return rec


def synth_molecules(B: int, seed: int, profile: str = "esol", pretrain_targets: bool = False,
                    p_salt: float = 0.0) -> List[MolRecord]:
    mu, p_cut, n_tasks = PROFILES[profile]
    rng = np.random.default_rng(seed)
    return [make_molecule(rng, mu, p_cut, n_tasks, pretrain_targets, p_salt) for _ in range(B)]


def attach_gene_expr(mols: List[MolRecord], gene_dim: int, seed: int, pinned=()) -> List[MolRecord]:
    """Gives every record a ``gene_expr`` float vector [gene_dim] drawn from N(0, 2.5) -- the cell-line input of a cancer-drug-response
    record (reference dataset/cdrp.py; collate_fn_cdrp truncates it to int64: negatives, zeros and values up to about +-8).  ``pinned``:
    values written over the leading entries of the FIRST record (fixtures place truncation cases there).  Returns ``mols``."""
    rng = np.random.default_rng(seed)
    for i, m in enumerate(mols):
        v = rng.normal(0.0, 2.5, size=gene_dim).astype(np.float32)
        if i == 0:
            v[:len(pinned)] = np.asarray(pinned, dtype=np.float32)
        m.gene_expr = torch.from_numpy(v)
    return mols


def attach_protein(mols: List[MolRecord], seed: int, length: int = 1000, pinned=None) -> List[MolRecord]:
    """Gives every record a ``protein`` float vector [length] -- the target input of a drug-target-affinity record as the reference's
    dataset/dta.py (CreateData.encode_protein) writes it: residue tokens 1..25 over a prefix of random length, 0 behind it.  The first
    record is full length.  ``pinned``: {record index: sequence of tokens}, written over that record's vector (zero-padded; fixtures place
    their edge cases there).  Returns ``mols``."""
    rng = np.random.default_rng(seed)
    pinned = {int(k): v for k, v in dict(pinned or {}).items()}
    for i, m in enumerate(mols):
        n = length if i == 0 else int(rng.integers(1, length + 1))
        v = np.zeros(length, dtype=np.float32)
        v[:n] = rng.integers(1, 26, size=n)
        if i in pinned:
            seq = np.asarray(pinned[i], dtype=np.float32)
            v[:] = 0.0
            v[:len(seq)] = seq
        m.protein = torch.from_numpy(v)
    return mols


def pair_records(n_pairs: int, n_drugs: int, n_seconds: int, kind: str, seed: int, gene_dim: int = 903, length: int = 1000) -> List[MolRecord]:
    """``n_pairs`` (drug, second input, y) records over exactly ``n_drugs`` distinct drugs and ``n_seconds`` distinct second inputs
    (``kind`` "cdrp": ``gene_expr`` rows that stay distinct after collate_fn_cdrp's truncating cast; "dta": ``protein`` token rows) -- the
    shape of a real drug-response or drug-target table, as the reference's dataset/cdrp.py builds it: one record per table row, so a
    repeated drug is a deep COPY with equal content, not a shared object.  Every drug and every second input occurs at least once;
    ``y`` is a pair effect, a drug effect plus a second-input effect plus noise."""
    import copy
    if kind not in ("cdrp", "dta"):
        raise ValueError(f"pair_records: kind must be 'cdrp' or 'dta' (got {kind!r})")
    if min(n_drugs, n_seconds) < 1 or n_pairs < max(n_drugs, n_seconds):
        raise ValueError("pair_records: n_pairs >= max(n_drugs, n_seconds) >= 1, so that every input can occur")
    rng = np.random.default_rng(seed)
    drugs = synth_molecules(n_drugs, seed=seed + 1, profile="esol")
    holders = [copy.deepcopy(drugs[0]) for _ in range(n_seconds)]
    field = "gene_expr" if kind == "cdrp" else "protein"
    for attempt in range(64):          # distinct AFTER the int64 cast: redraw in the (vanishingly rare) event of a collision
        if kind == "cdrp":
            attach_gene_expr(holders, gene_dim, seed + 2 + attempt)
        else:
            attach_protein(holders, seed + 2 + attempt, length=length)
        rows = {tuple(getattr(h, field).type(torch.long).tolist()) for h in holders}
        if len(rows) == n_seconds:
            break
    else:
        raise RuntimeError("pair_records: could not draw distinct second inputs")
    seconds = [getattr(h, field) for h in holders]
    # every input once, then uniform draws; shuffled so that first occurrences are not in index order
    du = np.concatenate([np.arange(n_drugs), rng.integers(0, n_drugs, size=n_pairs - n_drugs)])
    sc = np.concatenate([np.arange(n_seconds), rng.integers(0, n_seconds, size=n_pairs - n_seconds)])
    du, sc = rng.permutation(du), rng.permutation(sc)
    e_d, e_s = rng.normal(0.0, 1.0, size=n_drugs), rng.normal(0.0, 1.0, size=n_seconds)
    out = []
    for u, c in zip(du, sc):
        rec = copy.deepcopy(drugs[int(u)])
        setattr(rec, field, seconds[int(c)].clone())
        rec.y = torch.tensor([e_d[u] + e_s[c] + 0.1 * rng.normal()], dtype=torch.float32).reshape(drugs[0].y.shape)
        out.append(rec)
    return out


# ----------------------------------------------------------------------------------------
# Geometry from one conformer: the bond-graph edge attribute and the three pretraining targets as the reference's featuriser derives
# them (dataset/data.py:185-211 get_edge_attr_bond_graph, :224-260 get_bond_angle_dhangle), restated from their definitions:
#   u_e = (p[src] - p[dst]) / |p[src] - p[dst]|,  sigma_e = u_x + u_y + u_z,  S_a = sum of sigma_e over the bonds leaving a, ascending e
#   bnd_lngth[e] = |p[src] - p[dst]|^2     (squared: the reference takes no root)
#   bnd_angl[a]  = 3 S_a^2                 (the reference sums the unit vectors of an atom over ALL components into one scalar)
#   dh_angl[e]   = S_src S_dst (3 - sigma_e^2)
#   cos[j]       = 1 for the two directions of one bond, else the clamped dot product of the unit vectors from the shared atom
# ----------------------------------------------------------------------------------------
def geometry_from_positions(positions, edge_index, edge_index_bonds=None, dtype=np.float32):
    """Host evaluation (NumPy, ``dtype`` arithmetic) of what ops.bond_cos / ops.pretrain_geometry compute on the GPU, for one molecule or
    a whole batch (ids only have to be consistent).  Returns a dict of torch tensors: ``bnd_lngth`` [e, 1], ``bnd_angl`` [n, 1],
    ``dh_angl`` [e, 1] and, when ``edge_index_bonds`` [2, eb] is given, ``edge_attr_bonds`` [eb, 1]."""
    p = np.asarray(positions, dtype=dtype).reshape(-1, 3)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    src, dst = ei
    n = p.shape[0]
    d = p[src] - p[dst]
    l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = d / np.sqrt(l2)[:, None]
    sigma = (u[:, 0] + u[:, 1]) + u[:, 2]
    S = np.zeros(n, dtype=dtype)
    np.add.at(S, src, sigma)                                  # unbuffered, in edge order
    out = {"bnd_lngth": l2.reshape(-1, 1), "bnd_angl": (dtype(3.0) * (S * S)).reshape(-1, 1),
           "dh_angl": ((S[src] * S[dst]) * (dtype(3.0) - sigma * sigma)).reshape(-1, 1)}
    if edge_index_bonds is not None:
        n1, n2 = np.asarray(edge_index_bonds, dtype=np.int64).reshape(2, -1)
        a1, b1, a2, b2 = src[n1], dst[n1], src[n2], dst[n2]
        rev = (a1 == b2) & (b1 == a2)
        first = (a1 == a2) | (a1 == b2)                       # the shared atom is bond 1's source, else its destination
        c = np.where(first, a1, b1)
        o0 = np.where(first, b1, a1)
        o1 = np.where(c == a2, b2, a2)
        with np.errstate(divide="ignore", invalid="ignore"):
            v0, v1 = p[o0] - p[c], p[o1] - p[c]
            u0 = v0 / np.sqrt((v0 * v0).sum(1))[:, None]
            u1 = v1 / np.sqrt((v1 * v1).sum(1))[:, None]
        cos = np.clip((u0[:, 0] * u1[:, 0] + u0[:, 1] * u1[:, 1]) + u0[:, 2] * u1[:, 2], -1.0, 1.0)
        out["edge_attr_bonds"] = np.where(rev, dtype(1.0), cos).reshape(-1, 1)
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in out.items()}


def _place_atoms(rng, n: int, edge_index: np.ndarray) -> np.ndarray:
    """Breadth-first placement: a component starts at an origin drawn from N(0, 3^2) at its lowest atom; every newly reached neighbour
    (ascending id) sits U(0.9, 1.6) from its parent in a uniformly random direction, redrawn while it lands within 0.5 of a placed atom."""
    nbrs = [[] for _ in range(n)]
    for a, b in zip(edge_index[0].tolist(), edge_index[1].tolist()):
        nbrs[a].append(b)
    pos = np.zeros((n, 3))
    placed = np.zeros(n, dtype=bool)

    def put(a, draw):
        for _ in range(10000):
            cand = draw()
            if not placed.any() or np.min(np.linalg.norm(pos[placed] - cand, axis=1)) >= 0.5:
                pos[a], placed[a] = cand, True
                return
        raise RuntimeError("attach_positions: no free place for an atom")

    def beside(parent):
        v = rng.normal(size=3)
        return pos[parent] + rng.uniform(0.9, 1.6) * v / np.linalg.norm(v)

    for root in range(n):
        if placed[root]:
            continue
        put(root, lambda: rng.normal(0.0, 3.0, size=3))
        queue = [root]
        while queue:
            a = queue.pop(0)
            for b in sorted(set(nbrs[a])):
                if not placed[b]:
                    put(b, lambda: beside(a))
                    queue.append(b)
    return pos.astype(np.float32)


def attach_positions(mols: List[MolRecord], seed: int) -> List[MolRecord]:
    """Gives every record ``positions`` [n, 3] (one synthetic conformer; an RNG of its own, so synth_molecules' stream is untouched) and
    OVERWRITES ``edge_attr_bonds`` -- and ``bnd_lngth`` / ``bnd_angl`` / ``dh_angl`` where the record has them -- with the values
    geometry_from_positions derives from those positions, so that a store with and one without the derived tensors describe the same
    molecules.  Ring-closure bonds get whatever length the placement leaves them.  Returns ``mols``."""
    rng = np.random.default_rng(seed)
    for m in mols:
        ei = m.edge_index.numpy()
        pos = _place_atoms(rng, int(m.x_atoms.shape[0]), ei)
        geo = geometry_from_positions(pos, ei, m.edge_index_bonds.numpy())
        m.positions = torch.from_numpy(pos)
        m.edge_attr_bonds = geo["edge_attr_bonds"]
        if m.bnd_lngth is not None:
            m.bnd_lngth, m.bnd_angl, m.dh_angl = geo["bnd_lngth"], geo["bnd_angl"], geo["dh_angl"]
    return mols


# ----------------------------------------------------------------------------------------
# The one molecule whose fragmentation the reference publishes:
# CC[NH+](CCCl)CCOc1cccc2ccccc12.[Cl-] with explicit H (41 atoms, 7 fragments),
# fragnet/notebooks/FragNet.ipynb cell 34 (atom -> fragment map), cell 28 (bond list),
# cells 43/46 (11 connections and the fragment-bond node order).
# ----------------------------------------------------------------------------------------
NOTEBOOK_ATOMS_IN_FRAGS = {
    0: [0, 1, 20, 21, 22, 23, 24],
    1: [2, 25],
    2: [3, 4, 5, 26, 27, 28, 29],
    3: [6, 7, 30, 31, 32, 33],
    4: [8],
    5: [9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 34, 35, 36, 37, 38, 39, 40],
    6: [19],
}
# heavy-atom bonds 0..19 then X-H bonds (notebook cell 28 lists (index, atom1, atom2))
NOTEBOOK_BONDS = [
    (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (2, 6), (6, 7), (7, 8), (8, 9), (9, 10),
    (10, 11), (11, 12), (12, 13), (13, 14), (14, 15), (15, 16), (16, 17), (17, 18),
    (18, 9), (18, 13),
    (0, 20), (0, 21), (0, 22), (1, 23), (1, 24), (2, 25), (3, 26), (3, 27), (4, 28),
    (4, 29), (6, 30), (6, 31), (7, 32), (7, 33), (10, 34), (11, 35), (12, 36), (14, 37),
    (15, 38), (16, 39), (17, 40),
]
# fragment-bond nodes 0,2,4,...,20 (begin, end) -- notebook cell 46; odd nodes are the reverses
NOTEBOOK_CONNECTIONS = [(4, 3), (4, 5), (0, 1), (2, 1), (3, 1), (0, 6), (1, 6), (2, 6), (3, 6), (4, 6), (5, 6)]


def notebook_molecule(seed: int = 7, pretrain_targets: bool = False) -> MolRecord:
    """Topology of the notebook molecule with random features (no RDKit here)."""
    rng = np.random.default_rng(seed)
    n = 41
    a2f = np.empty(n, dtype=np.int64)
    for f, atoms in NOTEBOOK_ATOMS_IN_FRAGS.items():
        a2f[atoms] = f
    bonds = list(NOTEBOOK_BONDS)
    # a bond is "cut" iff its atoms sit in different fragments (5 BRICS bonds)
    cut = [bool(a2f[a] != a2f[b]) for a, b in bonds]
    rec = make_molecule(rng, n_tasks=0, pretrain_targets=pretrain_targets, topology=(n, bonds, cut))
    # impose the published connection order (BRICS bonds first, then the iso links)
    fs, fd = [], []
    for a, b in NOTEBOOK_CONNECTIONS:
        fs += [a, b]
        fd += [b, a]
    frag_index = np.asarray([fs, fd], dtype=np.int64)
    one_hot = np.zeros((len(NOTEBOOK_CONNECTIONS), CNX_F), dtype=np.float32)
    one_hot[np.arange(len(NOTEBOOK_CONNECTIONS)), rng.integers(0, CNX_F, size=len(NOTEBOOK_CONNECTIONS))] = 1.0
    cnx_attr = np.repeat(one_hot, 2, axis=0)
    eifb = fbond_graph_pairs(frag_index.T.copy())
    rec.frag_index = torch.from_numpy(frag_index)
    rec.cnx_attr = torch.from_numpy(cnx_attr)
    rec.node_feautures_fbondg = torch.from_numpy(cnx_attr.copy())
    rec.edge_index_fbondg = torch.from_numpy(eifb.astype(np.int32))
    rec.edge_attr_fbondg = torch.from_numpy(cnx_attr[eifb[0]] + cnx_attr[eifb[1]])
    assert torch.equal(rec.atom_id_frag_id, torch.from_numpy(a2f))
    return rec
