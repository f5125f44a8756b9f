#!/usr/bin/env python3
"""Writes a synthetic drug-target-affinity dataset: pickled lists of per-molecule records (the reference's on-disk format,
dataset.load_pickle_dataset), each an ESOL-shape synthetic molecule with a ``protein`` float vector [1000] (residue tokens 1..25 over a
prefix of random length, 0 behind it) and a scalar affinity ``y``.  Stands in for the reference's data_create pipeline for DTA (RDKit +
the Davis / KIBA tables, not available here).

    python scripts/make_synthetic_dta_dataset.py --out finetune_data/dta_synth"""
import argparse
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fragnet_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True, help="output directory")
ap.add_argument("--n", type=int, nargs=3, default=[512, 64, 64], metavar=("TRAIN", "VAL", "TEST"))
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--drugs", type=int, default=0, help="distinct drugs per split (0: every record its own, the default)")
ap.add_argument("--proteins", type=int, default=0, help="distinct proteins per split (0: every record its own, the default)")
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)
for split, n, s in zip(("train", "val", "test"), args.n, (0, 1, 2)):
    if args.drugs or args.proteins:   # a table of (drug, protein, y) rows over few distinct entities (synth.pair_records)
        mols = synth.pair_records(n, min(n, args.drugs or n), min(n, args.proteins or n), "dta", args.seed * 3 + s)
    else:
        mols = synth.attach_protein(synth.synth_molecules(n, seed=args.seed * 3 + s, profile="esol"), args.seed * 3 + s + 100)
    path = os.path.join(args.out, f"{split}.pkl")
    with open(path, "wb") as f:
        pickle.dump(mols, f)
    print(f"{split}: {n} records (protein length 1000) -> {path}")
