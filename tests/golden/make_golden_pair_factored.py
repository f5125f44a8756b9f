#!/usr/bin/env python3
"""Generates tests/golden/cdrp_pairs_u3c3.npz and tests/golden/dta_pairs_u3c3.npz by running the REFERENCE's two pair models on a batch
that really repeats its inputs (needs the reference checkout that make_golden.py names; run where that exists):
    python tests/golden/make_golden_pair_factored.py

Each case: 7 (drug, second input, y) records drawn from 3 drugs x 3 second inputs, collated the reference's way -- one molecule and one
gene / token row PER PAIR (collate_fn_cdrp / collate_fn_dta) -- through the reference model, num_layer 2, num_heads 4, drop_ratio 0,
model.train(), MSE against y.  The pair lists are PAIR_DRUG / PAIR_SECOND below: drug 0 occurs in 4 pairs, drug 1 in 2, drug 2 in 1
(seven pairs cannot hold 4 + 2 + 2), every second input at least twice.  Layout as make_golden_cdrp.py / make_golden_dta.py write it
(logits, loss, drug_enc, the second encoding, sampled gradients, cfg and seed); the cfg also holds the pair lists and the seeds from which
``records`` rebuilds the seven records, so that a test can collate the same records the factored way.  The reference is imported only
when this file is run; ``records`` needs fragnet_amd.synth alone.
"""
import copy
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

GENE_DIM = 903
PAIR_DRUG = [0, 1, 0, 0, 2, 1, 0]
PAIR_SECOND = [0, 1, 2, 1, 0, 2, 0]
Y = [0.8, -1.1, 0.3, 1.7, -0.4, 0.1, -2.0]
SEED = 7
CASES = {"cdrp": dict(name="cdrp_pairs_u3c3", mol_seed=5100, second_seed=5101),
         "dta": dict(name="dta_pairs_u3c3", mol_seed=6100, second_seed=6101)}
CTOR = dict(n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=2, num_heads=4, drop_ratio=0.0,
            h1=32, h2=64, h3=64, h4=32, act="relu", emb_dim=128, fthead="FTHead3")


def records(kind, mol_seed, second_seed, pair_drug=PAIR_DRUG, pair_second=PAIR_SECOND, y=Y):
    """The case's records: deep copies of 3 synthetic ESOL-profile molecules, each with a clone of one of 3 second inputs and its own y"""
    from fragnet_amd import synth
    drugs = synth.synth_molecules(3, seed=mol_seed, profile="esol")
    holders = [copy.deepcopy(drugs[0]) for _ in range(3)]
    if kind == "cdrp":
        synth.attach_gene_expr(holders, GENE_DIM, second_seed, (-0.7, 2.9, -1.5))
        seconds = [h.gene_expr for h in holders]
    else:
        synth.attach_protein(holders, second_seed, length=1000, pinned={1: [7]})
        seconds = [h.protein for h in holders]
    out = []
    for u, c, t in zip(pair_drug, pair_second, y):
        rec = copy.deepcopy(drugs[u])
        setattr(rec, "gene_expr" if kind == "cdrp" else "protein", seconds[c].clone())
        rec.y = torch.tensor([t], dtype=torch.float32).reshape(drugs[0].y.shape)
        out.append(rec)
    return out


def main():
    sys.path.insert(0, HERE)
    import make_golden as mg
    import make_golden_cdrp
    import make_golden_dta
    mg.install_stubs()
    with mg.quiet():
        from fragnet.model.gat import gat2 as ref_gat2
        from fragnet.model.cdrp.model import CDRPModel
        from fragnet.model.dta.model import DTAModel2           # reseeds torch and numpy at import
        from fragnet.dataset import data as ref_data
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    for kind, case in CASES.items():
        recs = records(kind, case["mol_seed"], case["second_seed"])
        if kind == "cdrp":
            Base = make_golden_cdrp.reference_base_class(ref_gat2)
            batch = ref_data.collate_fn_cdrp(recs)
        else:
            Base = make_golden_dta.reference_base_class(ref_gat2)
            batch = ref_data.collate_fn_dta(recs)
        torch.manual_seed(SEED)
        with mg.quiet():
            model = CDRPModel(Base(**CTOR), GENE_DIM, "cpu") if kind == "cdrp" else DTAModel2(Base(**CTOR))
        mg.zero_dead_bias(model.drug_model)
        model.train()
        kept = {}
        second = (model.cell_model, "cell_enc") if kind == "cdrp" else (model.fc1_xt, "prot_enc")
        hooks = [model.drug_model.register_forward_hook(lambda m, i, o: kept.__setitem__("drug_enc", o.detach().clone())),
                 second[0].register_forward_hook(lambda m, i, o, k=second[1]: kept.__setitem__(k, o.detach().clone()))]
        with mg.quiet():
            out = model(batch)
        for h in hooks:
            h.remove()
        loss = torch.nn.functional.mse_loss(out.view(-1), batch["y"])
        loss.backward()
        cfg = {"kind": kind, "ctor": CTOR, "gene_dim": GENE_DIM, "seed": SEED, "loss": "mse", "mol_seed": case["mol_seed"],
               "second_seed": case["second_seed"], "pair_drug": PAIR_DRUG, "pair_second": PAIR_SECOND, "y": Y}
        mg.save_case(case["name"], cfg, batch, model, {"logits": out, **kept}, loss, [])
        size = os.path.getsize(os.path.join(HERE, case["name"] + ".npz"))
        print(f"{case['name']}.npz: {size} bytes")
        assert size < (1 << 20)


if __name__ == "__main__":
    main()
