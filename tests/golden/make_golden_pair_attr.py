#!/usr/bin/env python3
"""Generates tests/golden/pair_attr.npz: attributions of the two pair models computed with the REFERENCE's own classes in float64 on
the CPU (needs the reference checkout that make_golden.py names; run where that exists):
    python tests/golden/make_golden_pair_attr.py

The models are the reference's CDRPModel (with its MLP) and DTAModel2 around its FragNetFineTuneBase, loaded as make_golden_cdrp.py /
make_golden_dta.py load them, with their constructor arguments.  The fixture stores no weights: the DTA model is dta_b5.npz's (same
seed; its parameter checksums are checked here), the CDRP model is cdrp_b5's constructor under the first seed from cdrp_b5's on whose
tower biases clear the margin below (``cfg`` names both; ``cdrp/pkeys``, ``cdrp/psums`` are its parameter checksums).  Everything is
evaluated on ``.double()`` copies; the file holds inputs and expected numbers only.

  v = fc1.weight^T fc2.weight, v_d = v[:256], v_s = v[256:]                 (plain float64 products, not fragnet_amd's)

CDRP, 5 cell lines (``cdrp/gene`` int64 [5, 903]) and the drugs of cdrp_b5's batch:
  s(x) = <tower(x), v_s>, the tower being the reference MLP's own ``predictor`` layers, relu(l(v)) in its forward's order, on float64
  rows (its forward casts to float32, so its layers are called directly).
  cdrp/gxi_attr                        gene * ds/dgene
  cdrp/ig8_zero_attr, ig8_base_attr    integrated gradients, midpoint rule with 8 nodes (the float32 values (j + 1/2) / 8), from zeros
                                       and from ``cdrp/baseline`` (float32 [903], N(0, 1))
  cdrp/score, score_zero, score_base   s at the cell lines, at zeros, at the baseline
  cdrp/gap_zero, gap_base              [2, 5]: score - score_baseline - sum(attr) at 8 and at 64 nodes
  drug/pred, drug/rows_*               <drug_enc, v_d> per molecule and (gradient . input) per row of the three node tables
EVERY pre-activation of every row evaluated for a stored value -- the 5 cell lines, their 2 x 8 path nodes, the two baselines -- is at
least MARGIN = 1e-4 away from zero (asserted; a cell line or baseline that fails is redrawn from the next seed): float32 then takes the
same side of every ReLU, and the float64 numbers are the target of a float32 computation up to round-off.

DTA, 3 proteins (``dta/tokens`` int64 [3, 1000], tokens 0..25):
  dta/attr [3, 1000]      gradient x input of <xt, v_s> on the EMBEDDED tensor (autograd through F.embedding -> the reference's Conv1d ->
                          Linear), summed over each position's embedding row
  dta/attr_other [3], dta/score [3]     score - sum(attr) (the bias terms) and <xt, v_s>
  dta/table [1000, 26]    the same attribution for 26 proteins of one repeated token each: position c, token v
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_cdrp as mc  # noqa: E402
import make_golden_dta as md  # noqa: E402

sys.path.insert(0, mg.REPO)
from tests import inputgrad_common as ic  # noqa: E402

NAME = "pair_attr"
MARGIN = 1e-4
N_CELLS, N_PROT, STEPS, STEPS_FINE = 5, 3, 8, 64
CELL_SEED, BASE_SEED, PROT_SEED = 7100, 7200, 7300


def alphas(steps):
    return ((np.arange(steps, dtype=np.float64) + 0.5) / steps).astype(np.float32).astype(np.float64)


def pair_vectors(model):
    v = (model.fc2.weight.detach().double() @ model.fc1.weight.detach().double()).reshape(-1)
    return v[:256], v[256:]


def checksums_match(model, case):
    z = np.load(os.path.join(HERE, case + ".npz"))
    keys, sums = mg.param_checksums(model)
    assert keys == json.loads(str(z["pkeys"])) and np.array_equal(np.asarray(sums), z["psums"]), f"{case}: not the model of the fixture"


class Tower:
    """The reference MLP's layers on float64 rows, with the smallest |pre-activation| seen."""

    def __init__(self, mlp):
        self.layers = list(copy.deepcopy(mlp).double().predictor)

    def __call__(self, x):
        lo = float("inf")
        for layer in self.layers:
            z = layer(x)
            lo = min(lo, float(z.detach().abs().min()))
            x = torch.nn.functional.relu(z)
        return x, lo


def path_rows(x, x0, steps):
    return x0 + torch.from_numpy(alphas(steps)).unsqueeze(1) * (x - x0)


def ig(tower, v_s, x, x0, steps):
    """(attr [K], smallest |pre-activation| on the nodes)"""
    rows = path_rows(x, x0, steps).requires_grad_(True)
    enc, lo = tower(rows)
    (g,) = torch.autograd.grad((enc @ v_s).sum(), rows)
    acc = g[0].clone()
    for j in range(1, steps):
        acc = acc + g[j]
    return (x - x0) * (acc / steps), lo


def cdrp_cells(model, store):
    tower, (_, v_s) = Tower(model.cell_model), pair_vectors(model)
    score = lambda x: float((tower(x.unsqueeze(0))[0].detach() @ v_s)[0])
    zero = torch.zeros(mc.GENE_DIM, dtype=torch.float64)
    assert tower(zero.unsqueeze(0))[1] >= MARGIN
    seed = BASE_SEED
    while True:
        base = torch.from_numpy(np.random.default_rng(seed).normal(0.0, 1.0, size=mc.GENE_DIM).astype(np.float32))
        if tower(base.double().unsqueeze(0))[1] >= MARGIN:
            break
        seed += 1
    print(f"  baseline: seed {seed}")
    base64 = base.double()
    genes, out, seed = [], {k: [] for k in ("gxi", "ig0", "igb", "score", "gap0", "gapb", "gap0f", "gapbf")}, CELL_SEED
    while len(genes) < N_CELLS:
        gene = torch.from_numpy(np.random.default_rng(seed).normal(0.0, 2.5, size=mc.GENE_DIM).astype(np.float32)).type(torch.long)
        seed += 1
        x = gene.double()
        leaf = x.clone().unsqueeze(0).requires_grad_(True)
        enc, lo_x = tower(leaf)
        (g,) = torch.autograd.grad((enc @ v_s).sum(), leaf)
        gxi = x * g[0]
        ig0, lo_0 = ig(tower, v_s, x, zero, STEPS)
        igb, lo_b = ig(tower, v_s, x, base64, STEPS)
        if min(lo_x, lo_0, lo_b) < MARGIN:
            continue
        print(f"  cell line {len(genes)}: seed {seed - 1}, smallest |pre-activation| {min(lo_x, lo_0, lo_b):.3e}")
        s = score(x)
        genes.append(gene)
        out["gxi"].append(gxi), out["ig0"].append(ig0), out["igb"].append(igb), out["score"].append(s)
        out["gap0"].append(s - score(zero) - float(ig0.sum())), out["gapb"].append(s - score(base64) - float(igb.sum()))
        out["gap0f"].append(s - score(zero) - float(ig(tower, v_s, x, zero, STEPS_FINE)[0].sum()))
        out["gapbf"].append(s - score(base64) - float(ig(tower, v_s, x, base64, STEPS_FINE)[0].sum()))
    for a, b, what in ((out["gap0"], out["gap0f"], "zero"), (out["gapb"], out["gapbf"], "non-zero")):
        worst8, worst64 = max(abs(v) for v in a), max(abs(v) for v in b)
        print(f"  {what} baseline: max|gap| {worst8:.3e} at {STEPS} nodes, {worst64:.3e} at {STEPS_FINE}")
        assert worst64 < worst8, "the gap does not shrink with the nodes: choose other seeds"
    stack = lambda k: torch.stack(out[k]).numpy()
    store.update({"cdrp/gene": torch.stack(genes).numpy(), "cdrp/baseline": base.numpy(), "cdrp/gxi_attr": stack("gxi"),
                  "cdrp/ig8_zero_attr": stack("ig0"), "cdrp/ig8_base_attr": stack("igb"), "cdrp/score": np.asarray(out["score"]),
                  "cdrp/score_zero": np.asarray(score(zero)), "cdrp/score_base": np.asarray(score(base64)),
                  "cdrp/gap_zero": np.asarray([out["gap0"], out["gap0f"]]), "cdrp/gap_base": np.asarray([out["gapb"], out["gapbf"]])})


def cdrp_drug(model, batch, mols, store):
    v_d, _ = pair_vectors(model)
    drug = copy.deepcopy(model.drug_model).double().eval()
    b = {k: (v.double() if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in batch.items()}
    leaves = [b[k].clone().requires_grad_(True) for k in ic.TABLE_KEYS]
    for k, t in zip(ic.TABLE_KEYS, leaves):
        b[k] = t
    with mg.quiet():
        pred = drug(b) @ v_d
    grads = torch.autograd.grad(pred.sum(), leaves)
    store["drug/pred"] = pred.detach().numpy()
    for name, g, x in zip(("atom", "bond", "fbond"), grads, leaves):
        store[f"drug/rows_{name}"] = (g * x.detach()).sum(1).numpy()
    store["drug/n_atoms"] = np.asarray([m.x_atoms.shape[0] for m in mols], dtype=np.int64)
    store["drug/n_bonds"] = np.asarray([m.node_features_bonds.shape[0] for m in mols], dtype=np.int64)
    store["drug/n_fbonds"] = np.asarray([m.node_feautures_fbondg.shape[0] for m in mols], dtype=np.int64)


def dta_proteins(model, store):
    m = copy.deepcopy(model).double()
    _, v_s = pair_vectors(m)

    def attributions(tokens):
        emb = torch.nn.functional.embedding(tokens, m.embedding_xt.weight).detach().requires_grad_(True)
        xt = torch.nn.functional.linear(m.conv_xt_1(emb).view(-1, m.fc1_xt_dim), m.fc1_xt.weight, m.fc1_xt.bias)
        s = xt @ v_s
        (g,) = torch.autograd.grad(s.sum(), emb)
        return (g * emb.detach()).sum(-1), s.detach()

    rng = np.random.default_rng(PROT_SEED)
    tokens = np.zeros((N_PROT, 1000), dtype=np.int64)
    for i, n in enumerate((1000, 1, 417)):
        tokens[i, :n] = rng.integers(1, 26, size=n)
    attr, s = attributions(torch.from_numpy(tokens))
    table, _ = attributions(torch.arange(26).unsqueeze(1).expand(26, 1000).contiguous())
    assert float((attr - table.t().gather(1, torch.from_numpy(tokens).t()).t()).abs().max()) < 1e-12
    store.update({"dta/tokens": tokens, "dta/attr": attr.numpy(), "dta/score": s.numpy(), "dta/attr_other": (s - attr.sum(1)).numpy(),
                  "dta/table": table.t().contiguous().numpy()})


def main():
    mg.install_stubs()
    with mg.quiet():
        from fragnet.model.gat import gat2 as ref_gat2
        from fragnet.model.cdrp.model import CDRPModel
        from fragnet.model.dta.model import DTAModel2           # reseeds torch and numpy at import
        from fragnet.dataset import data as ref_data
    from fragnet_amd import synth
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    store = {}

    Base, seed = mc.reference_base_class(ref_gat2), mc.SEED
    while True:                                                  # the zero row is the tower's biases: only another draw of the weights moves it
        torch.manual_seed(seed)
        with mg.quiet():
            cdrp = CDRPModel(Base(**mc.CTOR), mc.GENE_DIM, "cpu")
        if Tower(cdrp.cell_model)(torch.zeros(1, mc.GENE_DIM, dtype=torch.float64))[1] >= MARGIN:
            break
        seed += 1
    print(f"  CDRP model: seed {seed}")
    mg.zero_dead_bias(cdrp.drug_model)
    cdrp.eval()
    keys, sums = mg.param_checksums(cdrp)
    store.update({"cfg": np.asarray(json.dumps({"cdrp": {"ctor": mc.CTOR, "gene_dim": mc.GENE_DIM, "seed": seed, "mol_seed": mc.MOL_SEED},
                                                "dta": "dta_b5", "margin": MARGIN, "steps": [STEPS, STEPS_FINE]})),
                  "cdrp/pkeys": np.asarray(json.dumps(keys)), "cdrp/psums": sums})
    cdrp_cells(cdrp, store)
    mols = synth.attach_gene_expr(synth.synth_molecules(5, seed=mc.MOL_SEED, profile="esol"), mc.GENE_DIM, mc.GENE_SEED, mc.PINNED)
    cdrp_drug(cdrp, ref_data.collate_fn_cdrp(mols), mols, store)

    torch.manual_seed(md.SEED)
    with mg.quiet():
        dta = DTAModel2(md.reference_base_class(ref_gat2)(**md.CTOR))
    mg.zero_dead_bias(dta.drug_model)
    checksums_match(dta, "dta_b5")
    dta.eval()
    dta_proteins(dta, store)

    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print(f"{NAME}.npz: {size / 1024:.1f} KiB")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
