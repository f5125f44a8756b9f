#!/usr/bin/env python3
"""Leave-one-out atom, bond and fragment-connection attributions of a finetuned model (the reference's
fragnet/vizualize/viz.py ``get_all_contributions``: mask one element in every layer, predict again, report
``pred_no_mask - pred_mask``) for a whole dataset, batched on the engine (fragnet_amd/attribution.py).

    python scripts/attribute_gat2.py --config exps/ft/esol_synth/config.yaml --checkpoint exps/ft/esol_synth/ft.pt \\
        --data finetune_data/esol_synth/test.pt --out attr.npz

``--config`` is the finetune YAML (the model's shape is read from it, as scripts/finetune_gat2.py does), ``--checkpoint`` a plain
state_dict, ``--data`` a flat store (``.pt``) or a pickled list of per-molecule records.  The ``.npz`` holds flat arrays plus
per-molecule offsets: ``pred_no_mask [n_mols, n_classes]``, and per kind k in atom / bond / fbond ``k_offsets [n_mols + 1]``,
``k_index``, ``k_pred_mask``, ``k_attr`` -- rows ``k_offsets[i] : k_offsets[i + 1]`` are molecule i's.  ``bond_index`` is the
directed row of the bond (the reference's ``bond_index`` column), ``fbond_index`` the fragment connection's number.  Atom and bond
type columns need RDKit and are the caller's to join.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    from fragnet_amd import attribution
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="finetune YAML (exps/ft/*/config.yaml)")
    ap.add_argument("--checkpoint", required=True, help="state_dict of the finetuned model (finetune.chkpoint_name)")
    ap.add_argument("--data", required=True, help="flat store (.pt) or pickled list of molecule records")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--kinds", nargs="+", default=list(attribution.KIND_ORDER), choices=list(attribution.KIND_ORDER))
    ap.add_argument("--max-rows", type=int, default=attribution.DEFAULT_MAX_ROWS, help="atom + directed-bond rows per replica batch")
    ap.add_argument("--batch-size", type=int, default=512, help="molecules per unmasked evaluation batch")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if len(set(args.kinds)) != len(args.kinds):
        ap.error("--kinds: each kind once")
    if args.max_rows < 1 or args.batch_size < 1:
        ap.error("--max-rows and --batch-size must be positive")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    return args


def build_model(cfg):
    from fragnet_amd import train
    from fragnet_amd.model import FragNetFineTune
    if cfg.model_version != "gat2":
        raise SystemExit(f"model_version {cfg.model_version!r}: the masks (and so the attributions) exist for gat2 only")
    return FragNetFineTune(**train.finetune_model_kwargs(cfg), variant=cfg.model_version)


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
    model = build_model(cfg)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model.to(device)
    res = attribution.leave_one_out(model, load_source(args.data, device), kinds=args.kinds, max_rows=args.max_rows,
                                    batch_size=args.batch_size)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **res.arrays())
    n_rep = sum(int(res.tables[k]["offsets"][-1]) for k in res.kinds)
    print(f"{len(res)} molecules, {n_rep} masked replicas ({', '.join(res.kinds)}) -> {args.out}")


if __name__ == "__main__":
    main()
