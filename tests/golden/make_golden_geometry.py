#!/usr/bin/env python3
"""Generates tests/golden/geometry_b8.npz: eight molecules with atom coordinates, and what the REFERENCE's featuriser derives from
them (same rules as make_golden.py: run where the reference is, only numbers go into the fixture):

    python tests/golden/make_golden_geometry.py

The molecules: make_golden.edge_case_molecules() -- one fragment, two fragments, a lone counter-ion (an atom without a bond, not
the last atom), a two-atom component beside a larger one (one-bond fragment), two heavy atoms, the notebook molecule (two fused
rings and an ion) -- with coordinates from synth.attach_positions, plus two hand-placed ones: a molecule of two atoms (its
bond-graph rows are the reversed pair only) and a degree-4 centre at the origin whose first two neighbours lie on the x axis, one on
each side (a collinear triple: the dot product of the two unit vectors is exactly -1, the clamp's boundary).

    pos, edge_index, batch, edge_index_bonds_graph, n_atoms, n_edges, n_bedges      the inputs, collated by the reference's collate_fn_pt
    bnd_lngth, bnd_angl, dh_angl      fp32, as returned by the reference's own get_bond_angle_dhangle (fragnet/dataset/data.py:224-260)
                                      per molecule, on a stand-in conformer whose GetPositions() returns the coordinates, then
                                      concatenated by collate_fn_pt
    cos                               float64.  The reference takes the bond-graph edge attribute from RDKit (GetAngleRad, then np.cos,
                                      data.py:185-211) and RDKit is not installed where this runs, so this ONE quantity is not
                                      reference-generated: it is a float64 NumPy evaluation of that definition, written here pair by
                                      pair -- 1 for the two directions of one bond, else the dot product, clamped to [-1, 1], of the two
                                      normalised difference vectors from the shared atom.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import edge_case_molecules, install_stubs, quiet  # noqa: E402


class Conformer:
    """What get_bond_angle_dhangle asks of an RDKit conformer."""

    def __init__(self, pos):
        self.pos = np.asarray(pos, dtype=np.float64)

    def GetPositions(self):
        return self.pos


def cos_float64(pos, edge_index, pairs):
    p = np.asarray(pos, dtype=np.float64)
    out = np.empty(pairs.shape[1], dtype=np.float64)
    for j in range(pairs.shape[1]):
        b1 = tuple(int(v) for v in edge_index[:, pairs[0, j]])
        b2 = tuple(int(v) for v in edge_index[:, pairs[1, j]])
        if b1 == (b2[1], b2[0]):
            out[j] = 1.0
            continue
        (c,) = set(b1) & set(b2)
        o0, o1 = sorted(set(b1 + b2) - {c})
        v0, v1 = p[o0] - p[c], p[o1] - p[c]
        out[j] = min(1.0, max(-1.0, float(np.dot(v0 / np.linalg.norm(v0), v1 / np.linalg.norm(v1)))))
    return out


def hand_placed():
    from fragnet_amd import synth
    rng = np.random.default_rng(23)
    two = synth.make_molecule(rng, topology=(2, [(0, 1)], [False]))
    two.positions = torch.tensor([[0.25, -1.0, 0.5], [1.0, -0.25, 1.5]])
    star = synth.make_molecule(rng, topology=(5, [(0, 1), (0, 2), (0, 3), (0, 4)], [False] * 4))
    star.positions = torch.tensor([[0.0, 0.0, 0.0], [1.25, 0.0, 0.0], [-1.5, 0.0, 0.0], [0.0, 1.0, 0.5], [0.25, -0.5, 1.0]])
    return [two, star]


def main():
    install_stubs()
    with quiet():
        from fragnet.dataset import data as ref_data
    from fragnet_amd import synth
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)

    mols = synth.attach_positions(edge_case_molecules(), seed=41) + hand_placed()
    assert len(mols) == 8
    for m in mols:
        bl, ba, dh = ref_data.get_bond_angle_dhangle(Conformer(m.positions.numpy()), m.x_atoms, m.edge_index)
        m.bnd_lngth, m.bnd_angl, m.dh_angl = bl.reshape(-1, 1), ba.reshape(-1, 1), dh.reshape(-1, 1)      # data.py:478-480
    batch = ref_data.collate_fn_pt(mols)
    pos = torch.cat([m.positions for m in mols]).numpy()
    ei, eib = batch["edge_index"].numpy(), batch["edge_index_bonds_graph"].numpy()
    store = {"pos": pos.astype(np.float32), "edge_index": ei.astype(np.int64), "batch": batch["batch"].numpy().astype(np.int64),
             "edge_index_bonds_graph": eib.astype(np.int64),
             "n_atoms": np.asarray([m.x_atoms.shape[0] for m in mols], dtype=np.int64),
             "n_edges": np.asarray([m.edge_index.shape[1] for m in mols], dtype=np.int64),
             "n_bedges": np.asarray([m.edge_index_bonds.shape[1] for m in mols], dtype=np.int64),
             "bnd_lngth": batch["bnd_lngth"].numpy().astype(np.float32), "bnd_angl": batch["bnd_angl"].numpy().astype(np.float32),
             "dh_angl": batch["dh_angl"].numpy().astype(np.float32), "cos": cos_float64(pos, ei, eib)}
    assert store["bnd_lngth"].shape == (ei.shape[1], 1) and store["bnd_angl"].shape == (pos.shape[0], 1)
    np.savez_compressed(os.path.join(HERE, "geometry_b8.npz"), **store)
    print("geometry_b8 written:", {k: v.shape for k, v in store.items()}, "cos range", store["cos"].min(), store["cos"].max())


if __name__ == "__main__":
    main()
