"""Geometry from atom coordinates, host side (the geometry half): synth.geometry_from_positions against the fixture
tests/golden/geometry_b8.npz (the reference's own get_bond_angle_dhangle for the three pretraining targets, a float64 evaluation of
the definition for the cosines -- tests/golden/make_golden_geometry.py), synth.attach_positions, the ``positions`` field of
dataset.FlatMolStore and the argument checks of the two new entry points.  The kernels themselves: tests/test_gpu_geometry.py.

Tolerances: the targets against the reference's fp32 values with |a - b| <= 1e-4 (1 + |b|), the project's parity bar; the cosines
against float64 with atol 1e-5 (two differences, two norms and one dot product in fp32 stay well under 32 * 2^-24 ~ 2e-6)."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

TARGETS = ("bnd_lngth", "bnd_angl", "dh_angl")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "geometry_b8.npz")))


def parity(got, want):
    """max |a - b| / (1 + |b|)"""
    a, b = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert a.shape == b.shape
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if a.size else 0.0


def _mols(n=12, seed=11, pretrain_targets=True):
    from fragnet_amd import synth
    return synth.attach_positions(synth.synth_molecules(n, seed=seed, profile="esol", pretrain_targets=pretrain_targets, p_salt=0.3), seed=3)


def test_fixture_holds_the_structural_cases(gold):
    na, ne, nb = gold["n_atoms"], gold["n_edges"], gold["n_bedges"]
    assert len(na) == 8 and int(na.sum()) == gold["pos"].shape[0] and int(ne.sum()) == gold["edge_index"].shape[1]
    assert (int(na[6]), int(ne[6]), int(nb[6])) == (2, 2, 2)                       # the two-atom molecule: reversed-pair rows only
    deg = np.bincount(gold["edge_index"][0], minlength=int(na.sum()))
    ions = np.nonzero(deg == 0)[0]
    assert ions.size >= 2 and all(gold["batch"][i] == gold["batch"][i + 1] for i in ions)      # lone ions, never a molecule's last atom
    assert int(deg.max()) == 4
    assert int((gold["cos"] == -1.0).sum()) == 8 and int((gold["cos"] == 1.0).sum()) == 4      # the collinear triple; two one-bond fragments
    assert np.all(np.abs(gold["cos"]) <= 1.0)


def test_host_geometry_reproduces_the_fixture(gold):
    from fragnet_amd import synth
    got = synth.geometry_from_positions(gold["pos"], gold["edge_index"], gold["edge_index_bonds_graph"])
    for k in TARGETS:
        err = parity(got[k].numpy(), gold[k])
        print(k, "parity error", err)
        assert got[k].dtype == torch.float32 and err <= 1e-4, (k, err)
    cos = got["edge_attr_bonds"].numpy()[:, 0]
    err = float(np.max(np.abs(cos.astype(np.float64) - gold["cos"])))
    print("cos max abs error", err)
    assert err <= 1e-5
    assert np.all(np.abs(cos) <= 1.0) and np.all(cos[gold["cos"] == 1.0] == 1.0) and np.all(cos[gold["cos"] == -1.0] == -1.0)
    deg = np.bincount(gold["edge_index"][0], minlength=gold["pos"].shape[0])
    assert np.all(got["bnd_angl"].numpy()[deg == 0] == 0.0)


def test_attach_positions_leaves_the_molecule_stream_alone():
    from fragnet_amd import synth
    fields = [f for f in synth.MolRecord.__dataclass_fields__ if f not in ("smiles", "positions")]
    before = synth.synth_molecules(6, seed=21, profile="esol", pretrain_targets=True, p_salt=0.3)
    kept = [{f: getattr(m, f).clone() for f in fields} for m in before]
    synth.attach_positions(before, seed=5)
    after = synth.synth_molecules(6, seed=21, profile="esol", pretrain_targets=True, p_salt=0.3)
    for m, k in zip(after, kept):
        assert m.positions is None
        for f in fields:
            assert torch.equal(getattr(m, f), k[f]), f
    # what it writes: positions, and the four tensors derived from them; nothing else of the record changes
    for m, k in zip(before, kept):
        assert m.positions.dtype == torch.float32 and tuple(m.positions.shape) == (m.x_atoms.shape[0], 3)
        geo = synth.geometry_from_positions(m.positions.numpy(), m.edge_index.numpy(), m.edge_index_bonds.numpy())
        for f in fields:
            want = geo[f] if f in geo else k[f]
            assert torch.equal(getattr(m, f), want), f
    again = synth.attach_positions(synth.synth_molecules(6, seed=21, profile="esol", pretrain_targets=True, p_salt=0.3), seed=5)
    assert all(torch.equal(a.positions, b.positions) for a, b in zip(again, before))


def test_no_bonded_pair_is_closer_than_the_placement_allows():
    from fragnet_amd import synth
    mols = synth.attach_positions(synth.synth_molecules(200, seed=8, profile="esol", p_salt=0.3), seed=9)
    for m in mols:
        s, d = m.edge_index
        if s.numel():
            assert float((m.positions[s] - m.positions[d]).norm(dim=1).min()) >= 0.5


def test_positions_travel_with_the_store(tmp_path):
    from fragnet_amd.dataset import FlatMolStore
    mols = _mols()
    store = FlatMolStore.from_records(mols)
    want = torch.cat([m.positions for m in mols])
    assert torch.equal(store.t["positions"], want) and store.has_pretrain_targets
    path = str(tmp_path / "geom.pt")
    store.save(path)
    back = FlatMolStore.load(path)
    assert set(back.t) == set(store.t) and all(torch.equal(back.t[k], store.t[k]) for k in store.t)
    rep = store.replicate(3)
    assert torch.equal(rep.t["positions"], want.repeat(3, 1))
    i = len(mols) + 4                                                   # molecule 4 of the second copy
    assert torch.equal(rep.collate([i])["positions"], mols[4].positions)
    assert FlatMolStore.from_records(_mols(pretrain_targets=False)).without_geometry().has_pretrain_targets


def test_without_geometry_drops_exactly_the_four_tensors():
    from fragnet_amd import synth
    from fragnet_amd.dataset import FlatMolStore
    store = FlatMolStore.from_records(_mols())
    lean = store.without_geometry()
    assert set(store.t) - set(lean.t) == {"edge_attr_bonds", "bnd_lngth", "bnd_angl", "dh_angl"} and set(lean.t) <= set(store.t)
    assert torch.equal(lean.bond_graph_edges(), store.bond_graph_edges())
    a, b = lean.without_bond_graph_index(), store.without_bond_graph_index().without_geometry()
    assert set(a.t) == set(b.t) == set(lean.t) - set(FlatMolStore.DERIVED)
    assert torch.equal(a.bond_graph_edges(), store.bond_graph_edges())
    with pytest.raises(ValueError, match="positions"):
        FlatMolStore.from_records(synth.synth_molecules(3, seed=1)).without_geometry()


def test_coincident_bonded_atoms_are_refused():
    from fragnet_amd.dataset import FlatMolStore
    mols = _mols(4)
    s, d = (int(v) for v in mols[2].edge_index[:, 0])
    mols[2].positions[s] = mols[2].positions[d] + 5e-4          # closer than 1e-3 (in one coordinate)
    mols[2].positions[s, 1:] = mols[2].positions[d, 1:]
    with pytest.raises(ValueError, match="closer"):
        FlatMolStore.from_records(mols)
    mols[2].positions[s, 0] = mols[2].positions[d, 0] + 0.01   # far enough: accepted
    FlatMolStore.from_records(mols)


def test_cpu_collate_of_a_dropped_geometry_store_omits_the_derived_keys():
    from fragnet_amd import data, synth
    from fragnet_amd.dataset import FlatMolStore
    mols = _mols()
    store = FlatMolStore.from_records(mols)
    idx = [7, 2, 11, 0, 5]
    full = store.collate(idx, pretrain=True)
    lean = store.without_geometry().collate(idx, pretrain=True)
    assert set(full) - set(lean) == {"edge_attr_bonds", "bnd_lngth", "bnd_angl", "dh_angl"} and set(lean) <= set(full)
    for k in lean:
        assert lean[k].dtype == full[k].dtype and torch.equal(lean[k], full[k]), k
    assert torch.equal(lean.offsets, full.offsets)
    # the record-list collates pass the coordinates through, and the store's batch is theirs
    for fn, pt in ((data.collate_fn, False), (data.collate_fn_pt, True)):
        want = fn([mols[i] for i in idx])
        got = store.collate(idx, pretrain=pt)
        assert set(got) == set(want) and "positions" in want
        for k in want:
            assert torch.equal(got[k], want[k]), k
    assert "positions" not in data.collate_fn(synth.synth_molecules(2, seed=1))


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    assert lib.fn_bond_cos_f32(None, None, None, 4, 6, 8, None, None) == _lib.FN_EINVAL
    assert lib.fn_bond_cos_f32(None, None, None, -1, 6, 8, None, None) == _lib.FN_EINVAL
    assert lib.fn_bond_cos_f32(None, None, None, 4, 6, -8, None, None) == _lib.FN_EINVAL
    assert lib.fn_pretrain_geometry_f32(None, None, None, 4, 6, 1, 4, 6, None, None, None, None) == _lib.FN_EINVAL
    assert lib.fn_pretrain_geometry_f32(None, None, None, 4, -6, 1, 4, 6, None, None, None, None) == _lib.FN_EINVAL
    assert lib.fn_pretrain_geometry_f32(None, None, None, 4, 6, -1, 4, 6, None, None, None, None) == _lib.FN_EINVAL
    # the largest molecule the per-molecule staging takes: 1024 atoms, 4096 directed bonds; a caller that states more is refused up front
    assert (_lib.FN_GEOM_MAX_ATOMS, _lib.FN_GEOM_MAX_BONDS) == (1024, 4096)
    for atoms, bonds in ((1025, 8), (8, 4097)):
        assert lib.fn_pretrain_geometry_f32(None, None, None, 4000, 6000, 1, atoms, bonds, None, None, None, None) == _lib.FN_EUNSUPPORTED
        assert b"FN_GEOM_MAX" in lib.fn_last_error()


def test_ops_refuse_cpu_tensors():
    from fragnet_amd import _lib, ops
    pos, ei = torch.zeros(3, 3), torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(_lib.FragnetHipError):
        ops.bond_cos(pos, ei, torch.tensor([[0, 1], [1, 0]]))
    with pytest.raises(_lib.FragnetHipError):
        ops.pretrain_geometry(pos, ei, torch.zeros(3, dtype=torch.long), 1)
