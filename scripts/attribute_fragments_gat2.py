#!/usr/bin/env python3
"""Fragment contributions of a trained model (the reference's fragnet/vizualize/model_attr.py ``get_attr_image``: zero one fragment's
atom rows behind the encoder, predict again, report ``pred_no_mask - pred_mask``) for a whole dataset, one encoder pass per molecule
(fragnet_amd/attribution.py ``fragment_contributions``).

    python scripts/attribute_fragments_gat2.py --config exps/ft/esol_synth/config.yaml --checkpoint exps/ft/esol_synth/ft.pt \\
        --data finetune_data/esol_synth/test.pt --out frag_attr.npz --prop-type property

``--prop-type``: ``property`` (FragNetFineTune, finetune YAML), ``drp`` (CDRPModel, CDRP YAML with ``gene_dim``), ``dta`` (DTAModel2),
``energy`` (FragNetPreTrain's 4th output, pretrain YAML).  ``--checkpoint`` is a plain state_dict, ``--data`` a flat store (``.pt``) or a
pickled list of per-molecule records -- the only form for ``drp`` / ``dta``, whose records carry ``gene_expr`` / ``protein``.  The
``.npz`` holds flat arrays plus per-molecule offsets: ``pred_no_mask [n_mols, C]``, ``offsets [n_mols + 1]``, ``group`` (fragment id),
``n_atoms``, ``pred_mask``, ``attr`` -- rows ``offsets[i] : offsets[i + 1]`` are molecule i's fragments -- and ``atom_group`` /
``atom_offsets``, every atom's fragment.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROP_TYPES = ("property", "drp", "dta", "energy")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="finetune YAML (property, drp, dta) or pretrain YAML (energy)")
    ap.add_argument("--checkpoint", required=True, help="state_dict of the trained model")
    ap.add_argument("--data", required=True, help="flat store (.pt) or pickled list of molecule records")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--prop-type", required=True, choices=PROP_TYPES)
    ap.add_argument("--batch-size", type=int, default=512, help="molecules per encoder pass")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    if args.prop_type in ("drp", "dta") and args.data.endswith(".pt"):
        ap.error(f"--prop-type {args.prop_type}: --data must be a pickled list of records (a flat store carries no "
                 f"{'gene_expr' if args.prop_type == 'drp' else 'protein'})")
    return args


def build_model(cfg, prop_type="property", device="cuda:0"):
    """The model of the finetune / CDRP / DTA / pretrain drivers, from the same YAML fields."""
    from fragnet_amd import cdrp, dta, train
    from fragnet_amd.model import FragNetFineTune, FragNetPreTrain
    if prop_type == "energy":
        return FragNetPreTrain(**train.pretrain_model_kwargs(cfg))
    kw = train.finetune_model_kwargs(cfg)
    if prop_type == "property":
        return FragNetFineTune(variant=cfg.model_version, **kw)
    if prop_type == "drp":
        return cdrp.CDRPModel(cdrp.FragNetFineTuneBase(**kw), int(cfg.gene_dim), device)
    return dta.DTAModel2(dta.FragNetFineTuneBase(**kw))


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
    res = attribution.fragment_contributions(model, load_source(args.data, device), batch_size=args.batch_size)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **res.arrays())
    print(f"{len(res)} molecules, {int(res.offsets[-1])} fragment replicas -> {args.out}")


if __name__ == "__main__":
    main()
