#!/usr/bin/env python3
"""Generates tests/golden/attr_loo_b6.npz with the REFERENCE's own Python: leave-one-out predictions of its FragNetFineTune, one
molecule and one mask at a time, as fragnet/vizualize/viz.py's ``_mask_prediction*`` loops set the per-layer attributes.  Same
loading of the reference as make_golden.py (whose stand-ins it imports); its gat2.py prints on every masked forward, hence quiet().
Run here only:
    python tests/golden/make_golden_attr.py

The model is the scaled one of tests/attr_common.py (FTHead3 64/128/128/64, relu, 2 layers, 4 heads, seed 5; last Linear x 100,
attention vectors x 4) on synth.synth_molecules(6, seed=4100, profile="esol").  The file holds numbers only:
    cfg                           json: ctor, seeds, scalings
    pkeys, psums                  state-dict keys and (sum, abs-sum) checksums of the SCALED model
    m<i>/pred_no_mask             [n_classes]
    m<i>/<kind>_index, m<i>/<kind>_pred_mask      kind in atom, bond, fbond
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_stubs, param_checksums, quiet, zero_dead_bias  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import attr_common as ac  # noqa: E402


def main():
    install_stubs()
    with quiet():
        from fragnet.model.gat import gat2 as ref_gat2
        from fragnet.dataset import data as ref_data
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    ctor = dict(atom_features=167, frag_features=167, edge_features=17, emb_dim=128, **ac.CTOR)
    with quiet():
        model = ac.build(ref_gat2, ctor, ac.SEED, scaled=True)
    zero_dead_bias(model)

    def run(m, b):
        with quiet():
            return m(b)

    recs = ac.scalar_loo(model, ac.molecules(), ref_data.collate_fn, run)
    store = {"cfg": np.asarray(json.dumps({"ctor": ctor, "seed": ac.SEED, "mol_seed": ac.MOL_SEED, "n_mols": ac.N_MOLS, "profile": "esol",
                                           "head_scale": ac.HEAD_SCALE, "att_scale": ac.ATT_SCALE}))}
    keys, sums = param_checksums(model)
    store["pkeys"], store["psums"] = np.asarray(json.dumps(keys)), sums
    for i, rec in enumerate(recs):
        store[f"m{i}/pred_no_mask"] = rec["pred_no_mask"].astype(np.float32)
        for kind in ac.MASK_ATTR:
            store[f"m{i}/{kind}_index"] = rec[kind]["index"]
            store[f"m{i}/{kind}_pred_mask"] = rec[kind]["pred_mask"]
    path = os.path.join(HERE, "attr_loo_b6.npz")
    np.savez_compressed(path, **store)
    print(f"attr_loo_b6: {os.path.getsize(path) / 1024:.1f} KiB, {sum(len(r[k]['index']) for r in recs for k in ac.MASK_ATTR)} replicas")


if __name__ == "__main__":
    main()
