#!/usr/bin/env python3
"""Generates tests/golden/attn_readout_b6.npz with the REFERENCE's own Python: the last layer's four ``summed_attn_weights_*``
tensors (``scatter_add(attn_probs, source)``, gat2.py:165, 219, 268, 312) and the logits of its FragNetFineTune on ONE collated
batch.  ``return_attentions = True`` is set on the reference's last FragNetLayerA and a forward hook on that layer records the
8-tuple and hands the first four on, so the model's own forward runs unchanged: the reference's layer code, without importing
vizualize/model.py and its drawing dependencies.  Same loading of the reference as make_golden_attr.py.  Run here only:
    python tests/golden/make_golden_viz.py

The models are the scaled one of tests/attr_common.py (FTHead3 64/128/128/64, relu, 2 layers, seed 5; last Linear x 100, attention
vectors x 4, so the weights are far from uniform) with 4 heads (case ``h4``) and with 2 heads (case ``h2``), on
synth.synth_molecules(6, seed=4100, profile="esol").  The file holds numbers only:
    cfg                              json: seeds, scalings, per case the ctor
    <case>/pkeys, <case>/psums       state-dict keys and (sum, abs-sum) checksums of the SCALED model
    <case>/logits                    [6, n_classes]
    <case>/attn_atoms, attn_frags, attn_bonds, attn_fbonds     [rows, heads], rows = source.max() + 1 of the level
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
from tests.viz_common import CASES, NAMES, last_layer_readout  # noqa: E402

def main():
    install_stubs()
    with quiet():
        from fragnet.model.gat import gat2 as ref_gat2
        from fragnet.dataset import data as ref_data
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)

    def run(m, b):
        with quiet():
            return m(b)

    batch = ref_data.collate_fn(ac.molecules())
    store, ctors = {}, {}
    for case, heads in CASES.items():
        ctor = dict(atom_features=167, frag_features=167, edge_features=17, emb_dim=128, **dict(ac.CTOR, num_heads=heads))
        with quiet():
            model = ac.build(ref_gat2, ctor, ac.SEED, scaled=True)
        zero_dead_bias(model)
        logits, attn = last_layer_readout(model, batch, run)
        keys, sums = param_checksums(model)
        store[f"{case}/pkeys"], store[f"{case}/psums"] = np.asarray(json.dumps(keys)), sums
        store[f"{case}/logits"] = logits.detach().numpy().astype(np.float32)
        for name, t in zip(NAMES, attn):
            store[f"{case}/{name}"] = t.numpy().astype(np.float32)
        ctors[case] = ctor
    store["cfg"] = np.asarray(json.dumps({"ctor": ctors, "seed": ac.SEED, "mol_seed": ac.MOL_SEED, "n_mols": ac.N_MOLS, "profile": "esol",
                                          "head_scale": ac.HEAD_SCALE, "att_scale": ac.ATT_SCALE}))
    path = os.path.join(HERE, "attn_readout_b6.npz")
    np.savez_compressed(path, **store)
    print(f"attn_readout_b6: {os.path.getsize(path) / 1024:.1f} KiB; rows " +
          ", ".join(f"{c}/{n} {store[f'{c}/{n}'].shape}" for c in CASES for n in NAMES))


if __name__ == "__main__":
    main()
