"""Geometry from atom coordinates on the GPU (csrc/geometry.hip through ops.bond_cos / ops.pretrain_geometry): against the fixture
tests/golden/geometry_b8.npz (the reference's own get_bond_angle_dhangle for the three targets, a float64 evaluation of the definition
for the cosines), and the four ways a store can keep or drop its derived tensors collated to the same batch.

Tolerances, as in tests/test_geometry_host.py: the targets against fp32 values with |a - b| <= 1e-4 (1 + |b|), the cosines with atol 1e-5.
Observed on the MI355X (fixture batch): bnd_lngth 0, bnd_angl 3.6e-7, dh_angl 2.4e-6, cos 1.7e-7; the step's loss 124.956833 on both stores."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = ("bnd_lngth", "bnd_angl", "dh_angl")
GEOMETRY = TARGETS + ("edge_attr_bonds",)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def parity(got, want):
    a, b = got.detach().double().cpu().numpy(), np.asarray(want.detach().cpu().numpy() if torch.is_tensor(want) else want, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if a.size else 0.0


def abs_err(got, want):
    a, b = got.detach().double().cpu().numpy(), np.asarray(want.detach().cpu().numpy() if torch.is_tensor(want) else want, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "geometry_b8.npz")))
    g["dev"] = {k: torch.from_numpy(g[k]).to(DEV) for k in ("pos", "edge_index", "batch", "edge_index_bonds_graph")}
    return g


def _run(dev, pos=None, max_per_mol=None):
    """(cos [Eb, 1], bnd_lngth, bnd_angl, dh_angl) of the fixture batch, optionally at other coordinates."""
    from fragnet_amd import ops
    pos = dev["pos"] if pos is None else pos
    cos = ops.bond_cos(pos, dev["edge_index"], dev["edge_index_bonds_graph"])
    return (cos,) + tuple(ops.pretrain_geometry(pos, dev["edge_index"], dev["batch"], 8, max_per_mol=max_per_mol))


@pytest.fixture(scope="module")
def on_fixture(gold):
    out = _run(gold["dev"], max_per_mol=(int(gold["n_atoms"].max()), int(gold["n_edges"].max())))
    torch.cuda.synchronize()
    return out


def test_ops_reproduce_the_fixture(gold, on_fixture):
    cos, *targets = on_fixture
    for k, got in zip(TARGETS, targets):
        err = parity(got, gold[k])
        print(k, "parity error", err)
        assert got.dtype == torch.float32 and err <= 1e-4, (k, err)
    err = abs_err(cos[:, 0], gold["cos"])
    print("cos max abs error", err)
    assert cos.dtype == torch.float32 and tuple(cos.shape) == (gold["cos"].shape[0], 1) and err <= 1e-5
    c = cos[:, 0].cpu().numpy()
    ei, eib = gold["edge_index"], gold["edge_index_bonds_graph"]
    rev = (ei[0][eib[0]] == ei[1][eib[1]]) & (ei[1][eib[0]] == ei[0][eib[1]])
    assert int(rev.sum()) == 4 and np.all(c[rev] == 1.0)                            # the two directions of one bond: exactly 1
    assert np.all(np.abs(c) <= 1.0) and np.all(c[gold["cos"] == -1.0] == -1.0)      # the collinear triple sits on the clamp's boundary
    deg = np.bincount(ei[0], minlength=gold["pos"].shape[0])
    assert int((deg == 0).sum()) >= 2 and np.all(targets[1].cpu().numpy()[deg == 0] == 0.0)      # lone ions: exactly 0


def test_ops_are_bit_reproducible_and_size_the_molecules_themselves(gold, on_fixture):
    again = _run(gold["dev"])                   # max_per_mol=None: the op reads the largest molecule back from the batch vector
    for a, b in zip(on_fixture, again):
        assert torch.equal(a, b)


def test_translation_changes_nothing(gold, on_fixture):
    shift = torch.tensor([1.5, -0.75, 0.625], device=DEV)
    moved = _run(gold["dev"], gold["dev"]["pos"] + shift)
    assert abs_err(moved[0], on_fixture[0]) <= 1e-5
    for k, a, b in zip(TARGETS, moved[1:], on_fixture[1:]):
        assert parity(a, b) <= 1e-4, k


def test_rotation_keeps_lengths_and_cosines(gold, on_fixture):
    """Only those two: bnd_angl and dh_angl sum the COMPONENTS of unit vectors, so they are not rotation-invariant (nor are the reference's)."""
    q, r = np.linalg.qr(np.random.default_rng(2).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    pos = torch.from_numpy((gold["pos"].astype(np.float64) @ q.T).astype(np.float32)).to(DEV)
    turned = _run(gold["dev"], pos)
    assert abs_err(turned[0], on_fixture[0]) <= 1e-5
    assert parity(turned[1], on_fixture[1]) <= 1e-4


# ---------------------------------------------------------------------------------------- stores
@pytest.fixture(scope="module")
def stores():
    from fragnet_amd import synth
    from fragnet_amd.dataset import FlatMolStore
    mols = synth.attach_positions(synth.synth_molecules(70, seed=11, profile="esol", pretrain_targets=True, p_salt=0.2), seed=13)
    cpu = FlatMolStore.from_records(mols)
    idx = torch.randperm(70, generator=torch.Generator().manual_seed(4))[:37]      # store rows and batch rows differ
    full = cpu.to(DEV)
    want = full.collate(idx, pretrain=True)
    return {"cpu": cpu, "full": full, "idx": idx, "want": want}


def _same_batch(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if k in TARGETS:
            assert parity(got[k], want[k]) <= 1e-4, k
        elif k == "edge_attr_bonds":
            assert abs_err(got[k], want[k]) <= 1e-5, k
        else:
            assert torch.equal(got[k], want[k]), k                                  # every integer tensor, and the floats that are copies
    assert torch.equal(got.offsets, want.offsets) and got.max_per_mol == want.max_per_mol


@pytest.mark.parametrize("drop", ["geometry", "index", "geometry+index", "index+geometry"])
def test_stores_without_derived_tensors_collate_the_same_batch(stores, drop):
    full, idx, want = stores["full"], stores["idx"], stores["want"]
    N, E, Eb = want["x_atoms"].shape[0], want["edge_index"].shape[1], want["edge_index_bonds_graph"].shape[1]
    assert E % 64 and Eb % 64 and Eb % 256 and "positions" in want and getattr(want, "_keep", None) is not None, (N, E, Eb)
    store = {"geometry": lambda: full.without_geometry(), "index": lambda: full.without_bond_graph_index(),
             "geometry+index": lambda: full.without_geometry().without_bond_graph_index(),
             "index+geometry": lambda: full.without_bond_graph_index().without_geometry()}[drop]()
    got = store.collate(idx, pretrain=True)
    _same_batch(got, want)
    ft = store.collate(idx)                                      # the targets are filled for a pretraining batch only
    assert set(ft) == set(want) - set(TARGETS) and torch.equal(ft["edge_attr_bonds"], got["edge_attr_bonds"])
    if drop == "geometry":
        # the store still holds its bond-graph index: the batch came from the one-launch collate, not from the torch path --
        # which builds the same batch, bit for bit
        from fragnet_amd import dataset
        assert getattr(got, "_keep", None) is not None and getattr(ft, "_keep", None) is not None
        dataset.FUSED_COLLATE = False
        try:
            slow = store.collate(idx, pretrain=True)
        finally:
            dataset.FUSED_COLLATE = True
        assert getattr(slow, "_keep", None) is None and set(slow) == set(got)
        for k in got:
            assert torch.equal(slow[k], got[k]), k


def test_batch_to_fills_the_geometry_of_a_cpu_collated_batch(stores):
    from fragnet_amd import data
    idx = stores["idx"]
    lean_cpu = stores["cpu"].without_geometry()
    host = lean_cpu.collate(idx, pretrain=True)
    assert not set(GEOMETRY) & set(host)
    got = data.batch_to(host, DEV)
    want = lean_cpu.to(DEV).collate(idx, pretrain=True)
    assert set(got) == set(want) >= set(GEOMETRY)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_pretrain_step_on_a_geometry_store(stores):
    """One eager pretraining step (train.pretrain_loss) on the batch of a store that keeps coordinates only: the loss of the batch of
    the full store, within 1e-4."""
    from fragnet_amd import train
    from fragnet_amd.model import FragNetPreTrain
    torch.manual_seed(3)
    model = FragNetPreTrain(num_layer=1, drop_ratio=0.0, edge_features=17).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    want = stores["want"]
    ref_loss = float(train.pretrain_loss(model(dict(want)), want).detach())
    batch = stores["full"].without_geometry().collate(stores["idx"], pretrain=True)
    loss = train.pretrain_loss(model(dict(batch)), batch)
    print("loss", float(loss.detach()), "full store", ref_loss)
    assert abs(float(loss.detach()) - ref_loss) <= 1e-4
    before = [p.detach().clone() for p in model.parameters()]
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
