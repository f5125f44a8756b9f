"""The chemical-space map on the GPU (fragnet_amd/chemspace.py): ``fit`` through the model against ``fit`` on the rows
``neighbours.embed_all`` returns, the moments against the float64 reference of tests/moments_ref.py, the two identities of a PCA that
hold whatever the eigenvectors inside a near-degenerate eigenspace are (variance of coordinate c = eigenvalue c; mean squared
Mahalanobis distance of the fitted rows = rank) at the project's parity bar 1e-4 + 1e-4 |ref|, and ``map``."""
import numpy as np
import pytest
import torch

from fragnet_amd import _lib, chemspace as cs, neighbours as nb, synth
from fragnet_amd.dataset import FlatMolStore
from tests import moments_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [("gat2", "mol"), ("gat2", "frag"), ("gcn2", "mol"), ("gcn2", "frag")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture(scope="module")
def mols():
    return synth.synth_molecules(48, seed=33, profile="esol")


@pytest.fixture(scope="module")
def store(mols):
    return FlatMolStore.from_records(mols).to(DEV)


@pytest.fixture(scope="module")
def models():
    from fragnet_amd.gcn import FragNetFineTune as GCN
    from fragnet_amd.model import FragNetFineTune
    torch.manual_seed(0)
    gat = FragNetFineTune().to(DEV)                   # the default gat2 finetune model, randomly initialised
    torch.manual_seed(3)
    return {"gat2": gat, "gcn2": GCN(num_layer=2, h1=8, h2=8, h3=8, h4=8, edge_features=17).to(DEV)}


@pytest.fixture(scope="module")
def fitted(models, store):
    """Per case: the rows of one whole-store batch, the space fitted on them as a row table, and the space fitted through the model."""
    out = {}
    for name, level in CASES:
        rows, offsets = nb.embed_all(models[name], store, level, len(store))
        out[name, level] = (rows.contiguous(), offsets, cs.fit(rows.contiguous()), cs.fit(models[name], store, level=level, batch_size=len(store)))
    return out


def close(value, ref):
    return np.abs(value - ref) <= 1e-4 + 1e-4 * np.abs(ref)


@pytest.mark.parametrize("name,level", CASES)
def test_fit_through_the_model_equals_fit_on_the_rows(name, level, fitted, models, store):
    rows, offsets, by_rows, by_model = fitted[name, level]
    assert by_model.n == by_rows.n == rows.shape[0] == offsets[-1] and by_model.level == by_rows.level == level
    for field in ("shift", "sum", "gram", "mean", "eigenvalues", "components"):      # one batch, one call: the same moments bit for bit
        assert np.array_equal(getattr(by_model, field), getattr(by_rows, field)), field
    assert by_model.rank == by_rows.rank >= 2 and models[name].training
    # the moments against float64, inside the kernel's own bound
    x, shift = rows.cpu().numpy(), by_rows.shift.astype(np.float32)
    assert np.array_equal(shift.astype(np.float64), by_rows.shift)
    ref_sum, ref_gram = R.moments(x, shift)
    b_sum, b_gram = R.moments_bound(x, shift, _lib.MOMENTS_CHUNK)
    assert (np.abs(by_rows.gram - ref_gram) <= b_gram).all() and (np.abs(by_rows.sum - ref_sum) <= b_sum).all()
    # batch by batch: other chunks, other encoder batches -- the bound still holds against the rows of the same batching
    small = cs.fit(models[name], store, level=level, batch_size=7)
    x7 = nb.embed_all(models[name], store, level, 7)[0].cpu().numpy()
    shift7 = small.shift.astype(np.float32)
    ref_sum, ref_gram = R.moments(x7, shift7)
    b_sum, b_gram = R.moments_bound(x7, shift7, _lib.MOMENTS_CHUNK)
    assert small.n == by_rows.n and (np.abs(small.gram - ref_gram) <= b_gram).all() and (np.abs(small.sum - ref_sum) <= b_sum).all()
    mean64 = x.astype(np.float64).mean(0)
    assert close(by_rows.mean, mean64).all() and close(small.mean, x7.astype(np.float64).mean(0)).all()


@pytest.mark.parametrize("name,level", CASES)
def test_coordinates_have_the_eigenvalues_as_variances_and_mean_d2_is_the_rank(name, level, fitted):
    rows, _, space, _ = fitted[name, level]
    k = min(space.rank, 6)
    coords = space.transform(rows, k=k)
    assert coords.shape == (rows.shape[0], k) and coords.dtype == torch.float32 and coords.is_cuda
    c = coords.double().cpu().numpy()
    var = (c * c).mean(0)
    d2 = space.mahalanobis(rows)
    mean_d2 = float(d2.double().mean())
    print(f"{name} {level}: n {space.n} rank {space.rank} floor {space.floor:.3e} eig[:k] {space.eigenvalues[:k]} var {var} "
          f"eig[rank-1] {space.eigenvalues[space.rank - 1]:.3e} mean d2 {mean_d2:.6f}")
    assert close(var, space.eigenvalues[:k]).all()
    assert close(c.mean(0), 0.0).all()
    assert d2.shape == (rows.shape[0],) and (d2 >= 0).all()
    assert close(mean_d2, float(space.rank))
    # a slice of the rows, and a copy of a row, get the same bits as the whole table
    assert torch.equal(space.transform(rows[5:23], k=k), coords[5:23]) and torch.equal(space.mahalanobis(rows[5:23]), d2[5:23])
    twin = torch.cat([rows[9:10], rows[:3]], 0)
    assert torch.equal(space.transform(twin, k=k)[0], coords[9]) and torch.equal(space.mahalanobis(twin)[0], d2[9])
    with pytest.raises(ValueError, match="exceeds the rank"):
        space.transform(rows, k=space.rank + 1) if space.rank < space.width else space.directions(space.width + 1)


@pytest.mark.parametrize("name,level", [("gat2", "mol"), ("gcn2", "frag")])
def test_map_fills_every_field(name, level, fitted, models, store, mols):
    rows, offsets, space, _ = fitted[name, level]
    model = models[name]
    res = cs.map(model, store, queries=store, level=level, k=2, quantile=0.9, batch_size=len(store))
    n = rows.shape[0]
    assert len(res) == n and res.coords.shape == (n, 2) and res.d2.shape == (n,) and res.k == 2 and res.level == level
    assert np.array_equal(res.space.gram, space.gram) and res.space.rank == space.rank
    assert np.array_equal(res.coords, space.transform(rows, k=2).cpu().numpy()) and np.array_equal(res.d2, space.mahalanobis(rows).cpu().numpy())
    assert np.array_equal(res.offsets, offsets) and np.array_equal(res.offsets[res.mol] + res.frag, np.arange(n))
    # queries that are the library: every query row gets its library row's coordinates and distance bit for bit
    assert np.array_equal(res.query_coords, res.coords) and np.array_equal(res.query_d2, res.d2) and np.array_equal(res.query_offsets, res.offsets)
    assert res.domain_cutoff == np.quantile(res.d2.astype(np.float64), 0.9) and np.array_equal(res.inside, res.query_d2 <= res.domain_cutoff)
    assert 0 < res.inside.sum() < n
    arrays = res.arrays()
    assert all(np.asarray(v).size > 0 for v in arrays.values()) and arrays["components"].shape == (space.width, space.width)
    # other queries, in batches; none at all
    few = cs.map(model, store, queries=mols[3:9], level=level, k=1, batch_size=5)
    assert few.query_coords.shape == (few.query_offsets[-1], 1) and few.inside.shape == (few.query_offsets[-1],) and len(few.query_offsets) == 7
    assert np.isfinite(few.query_d2).all() and np.isfinite(few.coords).all()
    alone = cs.map(model, store, level=level, batch_size=16)
    assert alone.query_d2.shape == (0,) and alone.coords.shape == (n, 2)
    with pytest.raises(ValueError, match="exceeds the rank"):
        cs.map(model, mols[:4], level="mol", k=4)


def test_refusals_on_the_device(models, store):
    class Pair(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.drug_model = inner

    with pytest.raises(ValueError, match="pair model"):
        cs.fit(Pair(models["gat2"]), store)
    with pytest.raises(ValueError, match="at least 2 rows"):
        cs.fit(torch.zeros(1, 256, device=DEV))
    with pytest.raises(ValueError, match="not finite"):
        cs.fit(torch.full((4, 128), float("nan"), device=DEV))
    space = cs.fit(torch.randn(300, 128, device=DEV, generator=torch.Generator(DEV).manual_seed(1)))
    assert space.rank == 128 and space.level == "frag"
    with pytest.raises(ValueError, match=r"\[rows, 128\]"):
        space.transform(torch.zeros(3, 256, device=DEV))
    with pytest.raises(ValueError, match="needs the model"):
        space.mahalanobis(store)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        space.transform(torch.zeros(3, 128))
