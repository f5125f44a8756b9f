#!/usr/bin/env python3
"""Writes a synthetic cancer-drug-response dataset: pickled lists of per-molecule records (the reference's on-disk format,
dataset.load_pickle_dataset), each an ESOL-shape synthetic molecule with a ``gene_expr`` float vector [gene_dim] ~ N(0, 2.5) and a
scalar response ``y``.  Stands in for the reference's data_create pipeline for CDRP (RDKit + GDSC tables, not available here).

    python scripts/make_synthetic_cdrp_dataset.py --out finetune_data/cdrp_synth"""
import argparse
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fragnet_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True, help="output directory")
ap.add_argument("--gene-dim", type=int, default=903)
ap.add_argument("--n", type=int, nargs=3, default=[512, 64, 64], metavar=("TRAIN", "VAL", "TEST"))
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--drugs", type=int, default=0, help="distinct drugs per split (0: every record its own, the default)")
ap.add_argument("--cells", type=int, default=0, help="distinct cell lines per split (0: every record its own, the default)")
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)
for split, n, s in zip(("train", "val", "test"), args.n, (0, 1, 2)):
    if args.drugs or args.cells:      # a table of (drug, cell line, y) rows over few distinct entities (synth.pair_records)
        mols = synth.pair_records(n, min(n, args.drugs or n), min(n, args.cells or n), "cdrp", args.seed * 3 + s, gene_dim=args.gene_dim)
    else:
        mols = synth.attach_gene_expr(synth.synth_molecules(n, seed=args.seed * 3 + s, profile="esol"), args.gene_dim, args.seed * 3 + s + 100)
    path = os.path.join(args.out, f"{split}.pkl")
    with open(path, "wb") as f:
        pickle.dump(mols, f)
    print(f"{split}: {n} records (gene_dim {args.gene_dim}) -> {path}")
