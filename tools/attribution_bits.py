"""Bit fingerprints of the attribution drivers (fragnet_amd/attribution.py, gradient_attribution.py, pair_attribution.py, attention.py):
one line per case, the case name and a SHA-256 over every entry of ``result.arrays()`` in key order (name, shape, dtype, bytes), then
over molecule -1 as ``result[-1]`` gives it.  Run it on two checkouts and diff the outputs: a change of the drivers' HOST code that is
meant to leave the numbers alone must leave every line alone.  The companion of tools/engine_bits.py, whose ``digest`` and
``record_calls`` it uses.

    python tools/attribution_bits.py > bits.txt
    python tools/attribution_bits.py --calls > calls.txt        # per case the library's fn_* entry points in call order
    python tools/attribution_bits.py --time > times.txt         # per case: median, min and max seconds of 5 calls after a warm-up
    python tools/attribution_bits.py --time --only=protein,attention_bs5        # (any mode) these cases alone

Cases: 24 synthetic molecules (profile esol; the pair cases 24 records), fixed seeds, models with ``drop_ratio`` 0.1 left in training
mode -- a driver that forgot ``eval()`` shows as a changed fingerprint.  Every public driver, with the arguments that make it split its
work: a ``max_rows`` under which a molecule's replicas or steps span chunks, batch sizes that do not divide 24.  ``--time`` runs the
same cases on 512 molecules with a host clock around the whole call (the result arrives as numpy, so the device has finished)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

import engine_bits as eb
from fragnet_amd import attention, attribution, cdrp, dta, synth
from fragnet_amd import gradient_attribution as ga
from fragnet_amd import model as M
from fragnet_amd import pair_attribution as pa
from fragnet_amd import viz_model as V
from fragnet_amd.dataset import FlatMolStore

DEV = eb.DEV
CTOR = dict(n_classes=2, num_layer=2, num_heads=4, drop_ratio=0.1, h1=32, h2=32, h3=32, h4=32, act="relu", fthead="FTHead3")
GENE_DIM = 903
REPEATS = 5


def build(make, seed=0):
    """A model in TRAINING mode on the device: the drivers are to switch to evaluation themselves, and to switch back."""
    torch.manual_seed(seed)
    return make().to(DEV).train()


def flat(prefix, x):
    if isinstance(x, dict):
        return [it for k, v in x.items() for it in flat(f"{prefix}.{k}", v)]
    return [(prefix, x)]


def items_of(res):
    items = list(res.arrays().items()) + flat("last", res[-1])
    for i, v in enumerate(getattr(res, "values", None) or ()):
        items += flat(f"values{i}", v)
    return items


def cases(n):
    mols = synth.synth_molecules(n, seed=17, profile="esol")
    store = FlatMolStore.from_records(mols).to(DEV)

    def groups_of(recs):          # ids 0, 7, 14 by atom number; every fifth atom in no group
        return [np.where(np.arange(k) % 5 == 4, -1, np.arange(k) % 3 * 7).astype(np.int64) for k in (int(r.x_atoms.shape[0]) for r in recs)]
    drp_recs = synth.pair_records(n, max(n // 3, 1), max(n // 4, 1), "cdrp", seed=5, gene_dim=GENE_DIM)
    dta_recs = synth.pair_records(n, max(n // 3, 1), max(n // 4, 1), "dta", seed=6)
    gene = torch.cat([r.gene_expr.view(1, -1) for r in drp_recs]).type(torch.long)
    tokens = torch.cat([r.protein.view(1, -1) for r in dta_recs]).type(torch.long)

    gat2 = build(lambda: M.FragNetFineTune(**CTOR))
    lite = build(lambda: M.FragNetFineTuneLite(**CTOR))
    energy = build(lambda: M.FragNetPreTrain(num_layer=2, drop_ratio=0.1, edge_features=17), seed=2)
    drp = build(lambda: cdrp.CDRPModel(cdrp.FragNetFineTuneBase(**CTOR), GENE_DIM, DEV), seed=3)
    dtam = build(lambda: dta.DTAModel2(dta.FragNetFineTuneBase(**CTOR)), seed=4)
    viz = build(lambda: V.FragNetFineTuneViz(**dict(CTOR, edge_features=17)), seed=5)
    base3 = [np.linspace(0.0, 0.5, int(store.t[k].shape[1]), dtype=np.float32) for k in ga.STORE_KEYS]
    gene_base = np.linspace(-1.0, 1.0, GENE_DIM).astype(np.float32)
    lens = store._host_lengths()
    # a max_rows of three replicas of the largest molecule: replicas and steps span chunks (--time: of 128, or the chunks' fixed cost is all)
    small = (3 if n == 24 else 128) * int((lens["atom"] + lens["edge"]).max())

    loo, fc, fs = attribution.leave_one_out, attribution.fragment_contributions, attribution.fragment_shapley
    out = [
        ("loo_all", gat2, lambda m: loo(m, store)),
        ("loo_all_small_chunks_bs7", gat2, lambda m: loo(m, store, max_rows=small, batch_size=7)),
        ("loo_bond_atom_records", gat2, lambda m: loo(m, mols, kinds=("bond", "atom"), max_rows=small)),
        ("loo_fbond", gat2, lambda m: loo(m, store, kinds=("fbond",))),
    ]
    for name, model, recs in (("property", gat2, mols), ("energy", energy, mols), ("drp", drp, drp_recs), ("dta", dtam, dta_recs)):
        groups = groups_of(recs)
        if recs is mols:          # (the pair models take records only: theirs carry the second input)
            out.append((f"frag_{name}_store_bs7", model, lambda m: fc(m, store, batch_size=7)))
            out.append((f"frag_{name}_store_groups", model, lambda m, g=groups: fc(m, store, groups=g, batch_size=7)))
        out.append((f"frag_{name}_records_bs7", model, lambda m, recs=recs: fc(m, recs, batch_size=7)))
        out.append((f"frag_{name}_records_groups", model, lambda m, recs=recs, g=groups: fc(m, recs, groups=g, batch_size=7)))
    groups = groups_of(mols)
    F1 = np.unique(mols[1].atom_id_frag_id.numpy()).size
    perms = {1: np.stack([np.arange(F1), np.arange(F1)[::-1], np.roll(np.arange(F1), 1)])}          # molecule 1 by a caller's design
    out += [
        ("shapley_exact_store", gat2, lambda m: fs(m, store, exact_max=6, samples=8)),
        ("shapley_exact_small_chunks", gat2, lambda m: fs(m, store, exact_max=6, samples=8, batch_size=5, max_rows=1 << 9, return_values=True)),
        ("shapley_sampled_records", gat2, lambda m: fs(m, mols, exact_max=2, samples=8, seed=3, batch_size=7)),
        ("shapley_permutations", gat2, lambda m: fs(m, store, exact_max=6, samples=8, permutations=perms)),
        ("shapley_groups", gat2, lambda m: fs(m, store, groups=groups, exact_max=2, samples=8)),
        ("shapley_energy", energy, lambda m: fs(m, store, exact_max=6, samples=8, batch_size=7)),
        ("shapley_additive_drp", drp, lambda m: fs(m, drp_recs, batch_size=7, return_values=True)),
        ("shapley_additive_dta", dtam, lambda m: fs(m, dta_recs, batch_size=7)),
        ("gxi_gat2", gat2, lambda m: ga.input_gradients(m, store, target=1, batch_size=7)),
        ("gxi_gat2_gradients_records", gat2, lambda m: ga.input_gradients(m, mols, return_gradients=True)),
        ("gxi_lite_gradients", lite, lambda m: ga.input_gradients(m, store, batch_size=7, return_gradients=True)),
        ("ig_gat2_steps5", gat2, lambda m: ga.integrated_gradients(m, store, steps=5, target=1)),
        ("ig_gat2_steps5_small_chunks", gat2, lambda m: ga.integrated_gradients(m, store, steps=5, max_rows=small, batch_size=7)),
        ("ig_gat2_baseline_records", gat2, lambda m: ga.integrated_gradients(m, mols, steps=5, baseline=base3, max_rows=small)),
        ("ig_lite_steps5", lite, lambda m: ga.integrated_gradients(m, store, steps=5, baseline=[torch.from_numpy(b) for b in base3])),
        ("cell_gxi", drp, lambda m: pa.cell_line_attributions(m, gene, method="grad_x_input")),
        ("cell_ig_two_chunks", drp, lambda m: pa.cell_line_attributions(m, gene, method="ig", steps=5, max_rows=5 * ((n + 1) // 2))),
        ("cell_ig_baseline", drp, lambda m: pa.cell_line_attributions(m, gene, method="ig", steps=5, baseline=gene_base)),
        ("protein", dtam, lambda m: pa.protein_attributions(m, tokens)),
        ("drug_gxi_drp", drp, lambda m: pa.drug_attributions(m, drp_recs, method="grad_x_input", batch_size=7)),
        ("drug_ig_drp", drp, lambda m: pa.drug_attributions(m, drp_recs, method="ig", steps=5, max_rows=small)),
        ("drug_gxi_dta", dtam, lambda m: pa.drug_attributions(m, dta_recs, method="grad_x_input")),
        ("drug_ig_dta", dtam, lambda m: pa.drug_attributions(m, dta_recs, method="ig", steps=5, baseline=base3, batch_size=7)),
        ("attention_bs5", viz, lambda m: attention.attention_weights(m, store, batch_size=5)),
        ("attention_records", viz, lambda m: attention.attention_weights(m, mols)),
    ]
    return out


def main(argv):
    timed = "--time" in argv
    if "--calls" in argv:
        eb.record_calls()
    only = [a.split("=", 1)[1].split(",") for a in argv if a.startswith("--only=")]
    for name, model, run in cases(512 if timed else 24):
        if only and name not in only[0]:
            continue
        if not timed:
            res = run(model)
            assert model.training, f"{name}: the driver left the model in evaluation mode"
            eb.report(name, items_of(res))
            continue
        run(model)
        took = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            run(model)
            took.append(time.perf_counter() - t0)
        print(f"{name:34s} {statistics.median(took):.6f} {min(took):.6f} {max(took):.6f}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
