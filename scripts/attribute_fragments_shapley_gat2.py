#!/usr/bin/env python3
"""Fragment Shapley values of a trained model for a whole dataset (fragnet_amd/attribution.py ``fragment_shapley``): the attribution of
the set function v(S) = prediction with the atoms of every fragment outside S zeroed behind the encoder -- the mask of the reference's
fragnet/vizualize/model_attr.py -- that adds up: sum of a molecule's phi = pred - base.  One encoder pass per molecule.

    python scripts/attribute_fragments_shapley_gat2.py --config exps/ft/esol_synth/config.yaml --checkpoint exps/ft/esol_synth/ft.pt \\
        --data finetune_data/esol_synth/test.pt --out frag_shapley.npz --prop-type property

Model, data and ``--prop-type`` are attribute_fragments_gat2.py's.  A molecule with at most ``--exact-max`` fragments is enumerated (2^F
coalitions, exact values); one with more is sampled with ``--samples`` permutations in antithetic pairs, seeded by ``--seed`` and the
molecule's index.  ``--max-rows`` bounds the coalition rows of one encoder pass.  The ``.npz`` holds ``pred [n_mols, C]`` (every fragment
present), ``base`` (none), ``offsets [n_mols + 1]``, ``group`` (fragment id), ``n_atoms``, ``phi`` and ``stderr`` (float64; rows
``offsets[i] : offsets[i + 1]`` are molecule i's fragments), ``exact [n_mols]`` and ``atom_group`` / ``atom_offsets``.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from attribute_fragments_gat2 import PROP_TYPES, build_model  # noqa: E402  (one model per --prop-type, built in one place)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="finetune YAML (property, drp, dta) or pretrain YAML (energy)")
    ap.add_argument("--checkpoint", required=True, help="state_dict of the trained model")
    ap.add_argument("--data", required=True, help="flat store (.pt) or pickled list of molecule records")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--prop-type", required=True, choices=PROP_TYPES)
    ap.add_argument("--batch-size", type=int, default=512, help="molecules per encoder pass, at most")
    ap.add_argument("--exact-max", type=int, default=10, help="molecules with at most this many fragments are enumerated")
    ap.add_argument("--samples", type=int, default=256, help="permutations per sampled molecule (even: antithetic pairs)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the permutation draw")
    ap.add_argument("--max-rows", type=int, default=1 << 16, help="coalition rows per encoder pass, at most")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.batch_size < 1 or args.max_rows < 1:
        ap.error("--batch-size and --max-rows must be positive")
    if args.samples < 2 or args.samples % 2:
        ap.error("--samples must be even and positive")
    if args.exact_max < 0:
        ap.error("--exact-max must not be negative")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    if args.prop_type in ("drp", "dta") and args.data.endswith(".pt"):
        ap.error(f"--prop-type {args.prop_type}: --data must be a pickled list of records (a flat store carries no "
                 f"{'gene_expr' if args.prop_type == 'drp' else 'protein'})")
    return args


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    import fragnet_amd
    from fragnet_amd import attribution, train
    from fragnet_amd.dataset import load_source
    cfg = train.load_config(args.config, config=args.config)
    fragnet_amd.prefer_rocblas_for_dense_heads()
    device = torch.device(args.device)
    model = build_model(cfg, args.prop_type, device)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model.to(device)
    res = attribution.fragment_shapley(model, load_source(args.data, device), batch_size=args.batch_size, exact_max=args.exact_max,
                                       samples=args.samples, seed=args.seed, max_rows=args.max_rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **res.arrays())
    print(f"{len(res)} molecules, {int(res.offsets[-1])} fragments, {int(res.exact.sum())} molecules exact -> {args.out}")


if __name__ == "__main__":
    main()
