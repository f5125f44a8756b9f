#!/usr/bin/env python3
"""Attention weights of a finetuned model for a whole dataset (the reference's fragnet/vizualize/viz.py ``calc_weights``: the last
layer's ``summed_attn_weights_atoms / _frags / _bonds / _fbonds`` of ``FragNetFineTuneViz``), batched on the engine
(fragnet_amd/attention.py).

    python scripts/attention_gat2.py --config exps/ft/esol_synth/config.yaml --checkpoint exps/ft/esol_synth/ft.pt \\
        --data finetune_data/esol_synth/test.pt --out attn.npz

``--config`` is the finetune YAML (the model's shape is read from it, as scripts/finetune_gat2.py does), ``--checkpoint`` a plain
state_dict of the finetuned ``FragNetFineTune`` (the Viz class has its keys), ``--data`` a flat store (``.pt``) or a pickled list of
per-molecule records.  The ``.npz`` holds ``pred [n_mols, n_classes]`` and, per level k in atoms / bonds / frags / fbonds, ``k``
``[total rows, heads]`` with ``k_offsets [n_mols + 1]`` -- rows ``k_offsets[i] : k_offsets[i + 1]`` are molecule i's, one row per atom,
directed bond, fragment, directed fragment connection -- plus the sums the app draws: ``atom_weights``, ``frag_weights`` (head sums)
and ``bond_weights`` with ``bond_weights_offsets`` (viz.py:684-687, one value per bond).  Drawing needs RDKit and is the caller's.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="finetune YAML (exps/ft/*/config.yaml)")
    ap.add_argument("--checkpoint", required=True, help="state_dict of the finetuned model (finetune.chkpoint_name)")
    ap.add_argument("--data", required=True, help="flat store (.pt) or pickled list of molecule records")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--batch-size", type=int, default=512, help="molecules per read-out pass")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    return args


def build_model(cfg):
    from fragnet_amd import train
    from fragnet_amd.viz_model import FragNetFineTuneViz
    if cfg.model_version != "gat2":
        raise SystemExit(f"model_version {cfg.model_version!r}: the attention read-out exists for gat2 only")
    return FragNetFineTuneViz(**train.finetune_model_kwargs(cfg))          # (the Viz class takes no ``variant``)


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    import fragnet_amd
    from fragnet_amd import attention, train
    from fragnet_amd.dataset import load_source
    cfg = train.load_config(args.config, config=args.config)
    fragnet_amd.prefer_rocblas_for_dense_heads()
    device = torch.device(args.device)
    model = build_model(cfg)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model.to(device)
    res = attention.attention_weights(model, load_source(args.data, device), batch_size=args.batch_size)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **res.arrays())
    print(f"{len(res)} molecules, {', '.join(f'{int(res.offsets[k][-1])} {k}' for k in attention.LEVELS)} rows -> {args.out}")


if __name__ == "__main__":
    main()
