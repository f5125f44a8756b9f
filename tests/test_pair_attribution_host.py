"""Host-side checks of fragnet_amd.pair_attribution (no GPU): chunk planning, the affine split of the two pair heads, the protein
lookup table against float64 autograd, the fixture's own consistency, and the argument refusals."""
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

SMALL = dict(n_classes=1, num_layer=1, num_heads=4, drop_ratio=0.0, h1=8, h2=8, h3=8, h4=8, act="relu", fthead="FTHead3")


def _cdrp(seed=0, gene_dim=903):
    from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
    torch.manual_seed(seed)
    return CDRPModel(FragNetFineTuneBase(**SMALL), gene_dim, "cpu")


def _dta(seed=0):
    from fragnet_amd.dta import DTAModel2, FragNetFineTuneBase
    torch.manual_seed(seed)
    return DTAModel2(FragNetFineTuneBase(**SMALL))


# ------------------------------------------------------------------------------- chunk planning
def test_cell_chunks_keep_a_cell_lines_nodes_together():
    from fragnet_amd.pair_attribution import plan_cell_chunks
    assert plan_cell_chunks(10, 3, 10) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert plan_cell_chunks(1000, 32, 4096) == [(c, min(1000, c + 128)) for c in range(0, 1000, 128)]
    assert plan_cell_chunks(5, 1, 4096) == [(0, 5)]
    assert plan_cell_chunks(4, 8, 8) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert plan_cell_chunks(0, 8, 64) == []
    for n, steps, rows in ((7, 5, 17), (129, 32, 4096), (3, 4096, 4096)):
        chunks = plan_cell_chunks(n, steps, rows)
        assert [c for a, b in chunks for c in range(a, b)] == list(range(n))
        assert all(0 < (b - a) * steps <= rows for a, b in chunks)
    with pytest.raises(ValueError, match="do not fit"):
        plan_cell_chunks(4, 9, 8)
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError):
            plan_cell_chunks(*bad)


# ------------------------------------------------------------------------------- the affine split
@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_pair_head_is_the_sum_of_two_dots_and_a_constant(kind):
    from fragnet_amd.pair_attribution import pair_vectors
    model = _cdrp(3) if kind == "cdrp" else _dta(3)
    width = 256 if kind == "cdrp" else 300
    v_d, v_s, const = pair_vectors(model)
    assert v_d.shape == (256,) and v_s.shape == (width,) and v_d.dtype == v_s.dtype == torch.float32
    g = torch.Generator().manual_seed(5)
    drug, second = torch.randn(7, 256, generator=g), torch.randn(7, width, generator=g)
    with torch.no_grad():
        out = model.fc2(model.fc1(torch.cat((drug, second), 1))).reshape(-1)
    split = drug @ v_d + second @ v_s + const
    assert float((out - split).abs().max()) <= 1e-5


def test_pair_vectors_refuses_other_models():
    from fragnet_amd.pair_attribution import pair_vectors
    with pytest.raises(ValueError, match="not a pair model"):
        pair_vectors(torch.nn.Linear(4, 4))
    m = _cdrp()
    m.fc2 = torch.nn.Linear(128, 2)
    with pytest.raises(ValueError, match="not a pair model"):
        pair_vectors(m)


# ------------------------------------------------------------------------------- the protein table
def test_protein_table_matches_float64_autograd_on_the_embedded_tensor():
    """gradient x input through F.embedding -> F.conv1d -> F.linear in float64, an out-of-range token among the tokens: it has no
    embedding row (zeros here, as the tower's histogram kernel counts it) and gets no attribution."""
    from fragnet_amd.pair_attribution import pair_vectors, protein_attributions
    F = torch.nn.functional
    model = _dta(4).double()
    g = torch.Generator().manual_seed(9)
    tokens = torch.randint(0, 26, (3, 1000), generator=g)
    tokens[1, 1:] = 0
    tokens[0, 5], tokens[2, 999], tokens[2, 0] = 26, -1, 31
    v_s = pair_vectors(model)[1].double()
    E = model.embedding_xt.weight.detach()
    inside = (tokens >= 0) & (tokens < 26)
    emb = (F.embedding(tokens.clamp(0, 25), E) * inside.unsqueeze(-1)).requires_grad_(True)
    xt = F.linear(F.conv1d(emb, model.conv_xt_1.weight, model.conv_xt_1.bias).flatten(1), model.fc1_xt.weight, model.fc1_xt.bias)
    score = xt @ v_s
    (grad,) = torch.autograd.grad(score.sum(), emb)
    want = (grad * emb.detach()).sum(-1)
    got = protein_attributions(model, tokens)
    assert got.attr.shape == (3, 1000) and got.table.shape == (1000, 26) and len(got) == 3
    np.testing.assert_allclose(got.attr, want.numpy(), rtol=1e-5, atol=1e-7 * float(want.abs().max()))
    assert got.attr[0, 5] == 0.0 and got.attr[2, 999] == 0.0 and got.attr[2, 0] == 0.0
    np.testing.assert_allclose(got.score, score.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(got.attr.astype(np.float64).sum(1) + got.attr_other, got.score, atol=1e-4)
    assert set(got.arrays()) == {"method", "side", "attr", "attr_other", "score", "table"} and got[1]["attr"].shape == (1000,)


def test_fixture_is_consistent_with_itself():
    """tests/golden/pair_attr.npz: the lookup table reproduces the per-protein attributions, completeness holds in float64, and the gap
    of integrated gradients shrinks from 8 to 64 nodes on the CPU oracle."""
    z = np.load(os.path.join(GOLDEN, "pair_attr.npz"))
    cfg = json.loads(str(z["cfg"]))
    assert cfg["steps"] == [8, 64] and cfg["margin"] == 1e-4
    tok, table = z["dta/tokens"], z["dta/table"]
    assert tok.shape == (3, 1000) and table.shape == (1000, 26)
    np.testing.assert_allclose(table[np.arange(1000)[None, :], tok], z["dta/attr"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(z["dta/attr"].sum(1) + z["dta/attr_other"], z["dta/score"], rtol=0, atol=1e-12)
    assert z["cdrp/gene"].shape == (5, 903) and z["cdrp/gene"].dtype == np.int64 and bool(np.any(z["cdrp/baseline"] != 0))
    for name, attr, s0 in (("zero", "cdrp/ig8_zero_attr", "cdrp/score_zero"), ("base", "cdrp/ig8_base_attr", "cdrp/score_base")):
        gaps = z["cdrp/gap_" + name]
        np.testing.assert_allclose(z["cdrp/score"] - z[s0] - z[attr].sum(1), gaps[0], rtol=0, atol=1e-12)
        assert np.abs(gaps[1]).max() < np.abs(gaps[0]).max()


# ------------------------------------------------------------------------------- refusals
def test_cell_line_attributions_refuse_bad_arguments_before_touching_the_gpu():
    from fragnet_amd import _lib
    from fragnet_amd.pair_attribution import cell_line_attributions
    model, gene = _cdrp(), torch.zeros((2, 903), dtype=torch.int64)
    for kw, match in ((dict(method="shap"), "method"), (dict(steps=0), "steps"), (dict(max_rows=4097), "max_rows"), (dict(max_rows=0), "max_rows"),
                      (dict(steps=64, max_rows=32), "do not fit"), (dict(method="grad_x_input", baseline=np.zeros(903)), "baseline"),
                      (dict(baseline=np.zeros(3)), "baseline"), (dict(baseline=np.zeros((1, 903))), "baseline")):
        with pytest.raises(ValueError, match=match):
            cell_line_attributions(model, gene, **kw)
    for bad in (gene.float(), gene[:, :900], gene[0]):
        with pytest.raises(ValueError, match="gene_expr"):
            cell_line_attributions(model, bad)
    with pytest.raises(ValueError, match="cell-line tower"):
        cell_line_attributions(_dta(), gene)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        cell_line_attributions(model, gene)


def test_cell_line_attributions_refuse_a_tower_without_a_kernel_path():
    """widths the tower's kernels do not take: ValueError, never a quiet torch fallback"""
    from fragnet_amd.pair_attribution import cell_line_attributions
    model, gene = _cdrp(), torch.zeros((2, 903), dtype=torch.int64)
    model.cell_model.predictor[1] = torch.nn.Linear(1024, 254)
    model.cell_model.predictor[2] = torch.nn.Linear(254, 64)
    with pytest.raises(ValueError, match="no kernel path"):
        cell_line_attributions(model, gene)
    model = _cdrp()
    model.cell_model.predictor[3] = torch.nn.Linear(64, 256, bias=False)
    with pytest.raises(ValueError, match="no kernel path"):
        cell_line_attributions(model, gene)


def test_protein_and_drug_attributions_refuse_bad_arguments():
    from fragnet_amd import _lib, synth
    from fragnet_amd.pair_attribution import drug_attributions, protein_attributions
    dta = _dta()
    with pytest.raises(ValueError, match="protein tower"):
        protein_attributions(_cdrp(), torch.zeros((1, 1000), dtype=torch.int64))
    for bad in (torch.zeros((1, 999), dtype=torch.int64), torch.zeros((1, 1000)), torch.zeros(1000, dtype=torch.int64)):
        with pytest.raises(ValueError, match="tokens"):
            protein_attributions(dta, bad)
    mols = synth.synth_molecules(2, seed=1)
    with pytest.raises(ValueError, match="method"):
        drug_attributions(dta, mols, method="shap")
    with pytest.raises(ValueError, match="baseline"):
        drug_attributions(dta, mols, method="grad_x_input", baseline=(np.zeros(167), np.zeros(17), np.zeros(6)))
    with pytest.raises(ValueError, match="drug encoder"):
        drug_attributions(torch.nn.Linear(2, 2), mols)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        drug_attributions(dta, mols, method="grad_x_input")


def test_gradient_attribution_still_refuses_the_pair_models():
    from fragnet_amd import gradient_attribution as ga
    from fragnet_amd import synth
    with pytest.raises(ValueError, match="out of scope"):
        ga.input_gradients(_cdrp(), synth.synth_molecules(1, seed=1))


def test_drug_scorer_shares_the_encoder_and_keeps_its_mode():
    from fragnet_amd.pair_attribution import DrugScorer, pair_vectors
    model = _cdrp()
    model.eval()
    scorer = DrugScorer(model.drug_model, pair_vectors(model)[0])
    assert scorer.pretrain is model.drug_model.pretrain and not scorer.training and not model.drug_model.pretrain.training
    assert scorer.fthead.rng is model.drug_model.pretrain.rng
    assert torch.equal(scorer.fthead.lin.weight.reshape(-1), pair_vectors(model)[0]) and float(scorer.fthead.lin.bias.abs().sum()) == 0.0
    assert not any(p.requires_grad for p in scorer.fthead.parameters())
    model.train()
    assert DrugScorer(model.drug_model, pair_vectors(model)[0]).training and model.drug_model.pretrain.training


# ------------------------------------------------------------------------------- the command-line script
def _script():
    import importlib.util
    from tests.conftest import ROOT
    spec = importlib.util.spec_from_file_location("attribute_pair_gat2", os.path.join(ROOT, "scripts", "attribute_pair_gat2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_refuses_bad_command_lines():
    script = _script()
    base = ["--config", "c.yaml", "--checkpoint", "m.pt", "--data", "d.pkl"]
    for bad in (["--model", "dta", "--side", "second", "--method", "ig", "--out", "x.npz"], ["--model", "cdrp", "--side", "second", "--out", "x.txt"],
                ["--model", "cdrp", "--side", "second", "--steps", "0", "--out", "x.npz"], ["--model", "gcn", "--side", "drug", "--out", "x.npz"]):
        with pytest.raises(SystemExit):
            script.parse_args(base + bad)
    args = script.parse_args(base + ["--model", "cdrp", "--side", "second", "--method", "ig", "--out", "x.npz"])
    assert (args.steps, args.max_rows, args.method) == (32, None, "ig")


def test_script_writes_the_residue_attributions_of_a_dta_dataset(tmp_path):
    """the protein side is plain torch ops, so the whole script runs on the CPU: records that share a protein are attributed once"""
    import pickle
    from fragnet_amd import synth, train
    from tests.conftest import ROOT
    script = _script()
    config = os.path.join(ROOT, "exps", "ft", "dta_synth", "config.yaml")
    torch.manual_seed(1)
    model = script.build_model(train.load_config(config, config=config), "dta", "cpu")
    ckpt, data, out = (str(tmp_path / n) for n in ("ft.pt", "test.pkl", "res.npz"))
    torch.save(model.state_dict(), ckpt)
    recs = synth.attach_protein(synth.synth_molecules(4, seed=3), 4, length=1000)
    recs[3].protein = recs[1].protein.clone()
    with open(data, "wb") as f:
        pickle.dump(recs, f)
    script.main(["--model", "dta", "--side", "second", "--config", config, "--checkpoint", ckpt, "--data", data, "--out", out, "--device", "cpu"])
    z = np.load(out)
    assert z["rows"].tolist() == [0, 1, 2, 1] and z["attr"].shape == (3, 1000) and z["table"].shape == (1000, 26)
    assert str(z["side"]) == "protein" and str(z["method"]) == "grad_x_input"
    np.testing.assert_allclose(z["attr"].astype(np.float64).sum(1) + z["attr_other"], z["score"], atol=1e-4)
