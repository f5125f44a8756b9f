"""Diverse subsets on the GPU (fragnet_amd/diversity.py, scripts/diverse_subset_gat2.py): ``select`` is a valid greedy selection
(tests/kcenter_ref.check_selection at the project's parity bar 1e-4 + 1e-4 |ref|) against float64 distances of the rows
``neighbours.embed_all`` returns for the same batching -- not sequence equality: near-ties among embeddings make that a test of
rounding -- the picks map back to molecules and fragments, seeds are honoured, and ``split`` deals whole clusters."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fragnet_amd import diversity as dv, neighbours as nb, synth
from fragnet_amd.dataset import FlatMolStore
from tests import kcenter_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture(scope="module")
def mols():
    out = synth.synth_molecules(39, seed=21, profile="esol")
    return out + [out[4]]                             # molecule 4 a second time: row 39 is its twin, at distance 0 of it


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


def rows64(model, source, level, batch_size):
    return nb.embed_all(model, source, level, batch_size)[0].double().cpu().numpy()


def check(res, x64, k, metric, seeds64=None):
    """``res`` against float64 distances of the rows it was computed from; returns the float64 seed-first arrays' worst radius error."""
    s = 0 if seeds64 is None else seeds64.shape[0]
    n = x64.shape[0]
    assert res.picked.shape == (k,) and res.radius.shape == (k + 1,) and res.distance.shape == res.label.shape == (n,)
    picked = np.concatenate([np.full(s, -1), res.picked])
    radius = np.concatenate([np.full(s, np.nan), res.radius])
    label = np.where(res.label >= 0, res.label + s, -1 - res.label) if s else res.label          # seeded: -1 - s is seed row s
    return R.check_selection(x64, picked, radius, label, 1e-4, R.METRICS[metric], seeds=seeds64)


@pytest.mark.parametrize("name,level,metric", [("gat2", "mol", "l2"), ("gat2", "frag", "cosine"), ("gat2", "frag", "l2"), ("gcn2", "mol", "cosine")])
def test_select_is_a_valid_greedy_selection_for_every_batching(name, level, metric, store, models):
    model = models[name]
    for batch_size in (7, len(store)):
        x64 = rows64(model, store, level, batch_size)
        res = dv.select(model, store, 9, level=level, metric=metric, batch_size=batch_size)
        worst = check(res, x64, 9, metric)
        print(f"{name} {level} {metric} batch {batch_size}: max |radius - float64| = {worst:.3e}")
        assert len(res) == 9 and res.picked[0] == 0 and np.isposinf(res.radius[0]) and (np.diff(res.radius[1:]) <= 0).all()
        assert (res.distance[res.picked] == 0).all() and not np.signbit(res.distance).any()
        offsets = nb.row_offsets(store, level)
        assert np.array_equal(res.offsets, offsets)
        assert np.array_equal(offsets[res.mol] + res.frag, res.picked) and (res.frag < np.diff(offsets)[res.mol]).all()
        if level == "mol":
            assert np.array_equal(res.mol, res.picked) and (res.frag == 0).all()
            assert res.label[39] == res.label[4] and not (4 in res.picked and 39 in res.picked)      # the twin shares its cluster
        item = res[3]
        assert item["row"] == res.picked[3] and item["row"] in item["members"]
    assert model.training                             # the mode it came in is restored


def test_first_row_and_arg_max_start(store, models):
    model = models["gat2"]
    x64 = rows64(model, store, "mol", len(store))
    res = dv.select(model, store, 5, first=11)
    assert res.picked[0] == 11
    check(res, x64, 5, "l2")
    assert dv.select(model, store, 5, first=None).picked[0] == 0              # every row at +inf: the smallest row
    everything = dv.select(model, store, len(store))
    assert sorted(everything.picked.tolist()) == list(range(len(store))) and everything.radius[-1] == 0
    assert everything.radius[-2] <= 1e-4 * (1 + np.abs(x64).max() ** 2)       # the last pick is the twin of a row picked before it
    none = dv.select(model, store, 0)
    assert len(none) == 0 and (none.label == -1).all() and np.isposinf(none.distance).all()


def test_seeds_and_initial_distances(mols, store, models):
    model = models["gat2"]
    seeds = synth.synth_molecules(4, seed=77, profile="esol") + [mols[9]]
    for level in ("mol", "frag"):
        x64, s64 = rows64(model, store, level, 16), rows64(model, seeds, level, 16)
        res = dv.select(model, store, 6, level=level, seeds=seeds, batch_size=16)
        check(res, x64, 6, "l2", s64)
        assert np.isfinite(res.radius).all()
        if level == "mol":
            assert res.label[9] == -1 - 4 and res.distance[9] <= 1e-4 * (1 + (s64[4] ** 2).sum()) and 9 not in res.picked
    # a distance to another set handed in: rows nothing comes closer to keep label -1
    near = nb.nearest(model, store, seeds, metric="l2", k=1, batch_size=16).score[:, 0]
    res = dv.select(model, store, 6, init_distance=near, batch_size=16)
    x64 = rows64(model, store, "mol", 16)
    R.check_selection(x64, res.picked, res.radius, res.label, 1e-4, 0, init=np.maximum(near, 0).astype(np.float64))
    assert res.label[9] == -1 and (res.label[res.picked] == np.arange(6)).all() and res.radius[0] == near.max()
    with pytest.raises(ValueError, match=r"float32 \[40\]"):
        dv.select(model, store, 2, init_distance=near[:5])
    big = synth.synth_molecules(2, seed=5, profile="esol") * (dv.MAX_SEED_ROWS // 2 + 1)
    with pytest.raises(ValueError, match="init_distance"):
        dv.select(model, store, 2, seeds=big)
    with pytest.raises(ValueError, match="not both"):
        dv.select(model, store, 2, seeds=seeds, init_distance=near)


def test_split_partitions_the_store_by_whole_clusters(store, models):
    res = dv.select(models["gat2"], store, 8)
    train, valid, test = res.split((0.6, 0.2, 0.2))
    assert sorted(np.concatenate([train, valid, test]).tolist()) == list(range(len(store)))
    for part in (train, valid, test):
        assert (np.diff(part) > 0).all()
        for c in range(8):
            members = np.flatnonzero(res.label == c)
            assert members.size and (np.isin(members, part).all() or not np.isin(members, part).any())
    assert len(train) <= 0.6 * len(store)
    with pytest.raises(ValueError, match='level="mol"'):
        dv.select(models["gat2"], store, 3, level="frag").split()


def test_script_writes_the_documented_arrays(tmp_path, mols):
    from fragnet_amd import train
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import diverse_subset_gat2
    finally:
        sys.path.pop(0)
    config = os.path.join(ROOT, "exps", "ft", "esol_synth", "config.yaml")
    FlatMolStore.from_records(mols).save(str(tmp_path / "data.pt"))
    FlatMolStore.from_records(mols[:3]).save(str(tmp_path / "seeds.pt"))
    torch.manual_seed(11)
    model = diverse_subset_gat2.build_model(train.load_config(config, config=config))
    torch.save(model.state_dict(), str(tmp_path / "ft.pt"))
    out = str(tmp_path / "diverse.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "diverse_subset_gat2.py"), "--config", config, "--checkpoint",
                        str(tmp_path / "ft.pt"), "--data", str(tmp_path / "data.pt"), "--seeds", str(tmp_path / "seeds.pt"), "--out", out,
                        "--k", "6", "--metric", "cosine", "--split", "0.5", "0.25", "0.25", "--batch-size", "16"], capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "6 of 40 rows (40 molecules) picked" in r.stdout and "split" in r.stdout
    z = np.load(out)
    data, seeds = (FlatMolStore.load(str(tmp_path / name), device=DEV) for name in ("data.pt", "seeds.pt"))
    res = dv.select(model.to(DEV), data, 6, metric="cosine", seeds=seeds, batch_size=16)
    assert set(z.files) == set(res.arrays()) | {"train", "valid", "test"}
    for name in ("picked", "mol", "frag", "label", "offsets"):
        np.testing.assert_array_equal(z[name], res.arrays()[name])
    np.testing.assert_allclose(z["radius"], res.radius, rtol=0, atol=1e-6)
    np.testing.assert_allclose(z["distance"], res.distance, rtol=0, atol=1e-6)
    assert str(z["level"]) == "mol" and str(z["metric"]) == "cosine"
    for name, part in zip(("train", "valid", "test"), res.split((0.5, 0.25, 0.25))):
        np.testing.assert_array_equal(z[name], part)
    assert z["label"][:3].tolist() == [-1, -2, -3]    # the first three molecules ARE the seeds
