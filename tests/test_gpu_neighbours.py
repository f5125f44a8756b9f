"""Nearest neighbours in embedding space on the GPU (fragnet_amd/neighbours.py, scripts/neighbours_gat2.py): the embeddings are the
encoder's own rows bit for bit, and the lists meet the conditions of tests/topk_ref.check_lists (sorted, distinct, every score within
1e-4 + 1e-4 |ref| of the float64 score of that row, no better row left outside) against float64 scores of the embeddings ``embed``
returned -- not bit equality across batch sizes: the encoder's rows may differ in the last bit with batch composition.

Squared L2 is evaluated as q_sq + lib_sq - 2 dot (the kernel's contract), which cancels: its fp32 error does not scale with the
distance but with the terms.  Each term carries a relative error of at most about sqrt(256) roundings of 2^-24 (a chain or a tree over
at most 256 products), and rows embedded in another batch may differ by one unit in the last place, 2^-23 relative, which enters the
distance twice.  ``l2_atol`` = 1e-4 + 2^-19 (max q_sq + max lib_sq) covers both (2^-19 = 32 x 2^-24) and is used for the l2 cases only;
neighbouring scores of these molecules lie orders of magnitude further apart.
Observed on the MI355X: cosine within 6e-7 of float64, dot within 5e-5, squared L2 within 1.2e-3 under an l2_atol of 9.2e-3."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fragnet_amd import neighbours as nb, synth
from fragnet_amd.attribution import evaluation
from fragnet_amd.dataset import FlatMolStore
from tests import topk_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(num_layer=2, h1=8, h2=8, h3=8, h4=8, edge_features=17)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture(scope="module")
def mols():
    out = synth.synth_molecules(37, seed=21, profile="esol")
    return out + [out[4]]                             # molecule 4 a second time: row 37 is its twin


def make_model(variant="gat2", seed=0):
    from fragnet_amd.model import FragNetFineTune
    torch.manual_seed(seed)
    return FragNetFineTune(**SMALL, variant=variant).to(DEV)


@pytest.fixture(scope="module")
def model():
    return make_model()


@pytest.fixture(scope="module")
def store(mols):
    return FlatMolStore.from_records(mols).to(DEV)


@pytest.mark.parametrize("variant", ["gat2", "gat2_lite", "gat2_edge"])
def test_embeddings_are_the_encoders_rows(variant, store, model):
    from fragnet_amd.model import pooled
    m = model if variant == "gat2" else make_model(variant)
    batch = store.collate(np.arange(len(store)))
    with evaluation(m), torch.no_grad():
        x_atoms, x_frags = m.pretrain(batch, edge_outputs=False)[:2]
        want_mol, want_frag = pooled(x_atoms, x_frags, batch).clone(), x_frags.clone()
    got_mol, mol_off = nb.embed_all(m, store, "mol", batch_size=len(store))
    got_frag, frag_off = nb.embed_all(m, store, "frag", batch_size=len(store))
    assert got_mol.shape == (len(store), 256) and torch.equal(got_mol, want_mol)
    assert got_frag.shape[1] == 128 and torch.equal(got_frag, want_frag)
    assert mol_off.tolist() == list(range(len(store) + 1))
    assert np.array_equal(frag_off, batch.offsets.cpu().numpy()[3].astype(np.int64))          # plan.SPACES[3] = "frag"
    assert m.training                                                                          # the mode it came in is restored
    parts = list(nb.embed(m, store, "frag", batch_size=7))
    assert [(p.first, p.end) for p in parts] == [(b, min(b + 7, len(store))) for b in range(0, len(store), 7)]
    assert all(p.rows.shape[0] == p.offsets[-1] and p.offsets[0] == 0 for p in parts)
    assert sum(p.rows.shape[0] for p in parts) == got_frag.shape[0]


def l2_atol(q, lib):
    return 1e-4 + 2.0 ** -19 * float((q * q).sum(1).max() + (lib * lib).sum(1).max())


def _reference_scores(model, store, level, metric, want_atol=False):
    rows, _ = nb.embed_all(model, store, level, batch_size=len(store))
    rows = rows.double().cpu().numpy()
    ref = R.scores(rows, rows, R.METRICS[metric])
    return (ref, l2_atol(rows, rows) if metric == "l2" else 1e-4) if want_atol else ref


@pytest.mark.parametrize("level,metric", [("mol", "cosine"), ("mol", "l2"), ("frag", "cosine"), ("frag", "dot")])
def test_lists_against_float64_scores_for_every_batching(level, metric, store, model):
    ref, atol = _reference_scores(model, store, level, metric, want_atol=True)
    m = R.METRICS[metric]
    for batch_size in (3, 7, len(store)):
        res = nb.nearest(model, store, store, level=level, k=9, metric=metric, batch_size=batch_size)
        assert res.score.shape == (ref.shape[0], 9) and len(res) == len(store)
        worst = R.check_lists(res.score, res.index, ref, m, atol=atol)
        print(f"{level} {metric} batch {batch_size}: max |score - float64| = {worst:.3e} (atol {atol:.3e})")
    if metric == "cosine":
        assert np.abs(res.score[:, 0] - 1).max() <= 1e-5          # the best neighbour of a row of the library is itself, or a twin
        own = np.arange(ref.shape[0])
        assert ((res.index[:, 0] == own) | (np.abs(ref[own, res.index[:, 0]] - 1) <= 1e-5)).all()
        assert np.array_equal(res.domain_distance()[:3], [res.score[res.query_offsets[i]: res.query_offsets[i + 1], 0].max() for i in range(3)])


def test_exclude_self_finds_the_twin_first(store, model):
    res = nb.nearest(model, store, store, level="mol", k=4, metric="cosine", batch_size=7, exclude_self=True)
    assert (res.index != np.arange(len(store))[:, None]).all()
    assert res.index[4, 0] == 37 and res.index[37, 0] == 4
    assert abs(res.score[4, 0] - 1) <= 1e-5 and res[4]["mol"][0] == 37
    ref = _reference_scores(model, store, "mol", "cosine")
    R.check_lists(res.score, res.index, ref, 1, exclude=np.arange(len(store)))
    frag = nb.nearest(model, store, store, level="frag", k=3, metric="l2", exclude_self=True)
    rows = np.arange(frag.score.shape[0])
    assert (frag.index != rows[:, None]).all()
    lo, hi = frag.query_offsets[4], frag.query_offsets[5]
    twin = frag.library_offsets[37]
    assert np.array_equal(frag.index[lo:hi, 0], twin + np.arange(hi - lo))                    # fragment j of molecule 4 -> fragment j of its twin
    assert np.array_equal(frag.mol[lo:hi, 0], np.full(hi - lo, 37)) and np.array_equal(frag.frag[lo:hi, 0], np.arange(hi - lo))
    assert np.array_equal(frag.query_mol[lo:hi], np.full(hi - lo, 4))


def test_queries_from_another_source(mols, store, model):
    queries = synth.synth_molecules(5, seed=77, profile="esol") + [mols[9]]
    res = nb.nearest(model, queries, store, level="mol", k=32, metric="l2", batch_size=16)
    q, lib = (nb.embed_all(model, src, "mol")[0].double().cpu().numpy() for src in (queries, store))
    atol = l2_atol(q, lib)
    assert len(res) == 6 and res.score.shape == (6, 32) and res.index[5, 0] == 9 and abs(res.score[5, 0]) <= atol
    R.check_lists(res.score, res.index, R.scores(q, lib, 2), 2, atol=atol)
    few = nb.nearest(model, queries, mols[:3], level="mol", k=5, metric="dot")                # a library smaller than k: empty slots
    assert (few.index[:, 3:] == -1).all() and np.isneginf(few.score[:, 3:]).all() and (few.mol[:, 3:] == -1).all()
    assert (np.sort(few.index[:, :3], axis=1) == np.arange(3)).all()


def test_gcn2_encoder_hands_back_the_same_pair(store):
    from fragnet_amd.gcn import FragNetFineTune as GCN
    torch.manual_seed(3)
    m = GCN(num_layer=2, h1=8, h2=8, h3=8, h4=8, edge_features=17).to(DEV)
    res = nb.nearest(m, store, store, level="mol", k=3, metric="cosine", batch_size=16)
    R.check_lists(res.score, res.index, _reference_scores(m, store, "mol", "cosine"), 1)


def test_script_writes_the_documented_arrays(tmp_path, mols):
    from fragnet_amd import train
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import neighbours_gat2
    finally:
        sys.path.pop(0)
    config = os.path.join(ROOT, "exps", "ft", "esol_synth", "config.yaml")
    FlatMolStore.from_records(mols).save(str(tmp_path / "lib.pt"))
    FlatMolStore.from_records(mols[:6]).save(str(tmp_path / "q.pt"))
    torch.manual_seed(11)
    model = neighbours_gat2.build_model(train.load_config(config, config=config))
    torch.save(model.state_dict(), str(tmp_path / "ft.pt"))
    out = str(tmp_path / "nn.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "neighbours_gat2.py"), "--config", config, "--checkpoint",
                        str(tmp_path / "ft.pt"), "--queries", str(tmp_path / "q.pt"), "--library", str(tmp_path / "lib.pt"), "--out", out,
                        "--level", "frag", "--k", "5", "--metric", "cosine", "--batch-size", "16"], capture_output=True, text=True, cwd=ROOT,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "6 query molecules" in r.stdout
    z = np.load(out)
    res = nb.nearest(model.to(DEV), FlatMolStore.load(str(tmp_path / "q.pt"), device=DEV), FlatMolStore.load(str(tmp_path / "lib.pt"), device=DEV),
                     level="frag", k=5, metric="cosine", batch_size=16)
    assert set(z.files) == set(res.arrays())
    for name in ("index", "mol", "frag", "query_mol", "query_frag", "query_offsets", "library_offsets"):
        np.testing.assert_array_equal(z[name], res.arrays()[name])
    np.testing.assert_allclose(z["score"], res.score, rtol=0, atol=1e-6)
    assert str(z["level"]) == "frag" and str(z["metric"]) == "cosine" and z["domain_distance"].shape == (6,)
