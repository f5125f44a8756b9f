#!/usr/bin/env python3
"""A diverse subset of a store in the embedding space of a finetuned model -- greedy k-centre (farthest-point / MaxMin picking) on the
engine (fragnet_amd/diversity.py) -- and, with ``--split``, a train / valid / test split of the store by the clusters around the picks.

    python scripts/diverse_subset_gat2.py --config exps/ft/esol_synth/config.yaml --checkpoint exps/ft/esol_synth/ft.pt \\
        --data finetune_data/esol_synth/train.pt --k 64 --split 0.8 0.1 0.1 --out diverse.npz

``--config`` is the finetune YAML (the model's shape and ``model_version`` -- gat2, gat2_lite, gat2_edge or gcn2 -- are read from it, as
scripts/neighbours_gat2.py does), ``--checkpoint`` a plain state_dict of the finetuned model, ``--data`` a flat store (``.pt``) or a
pickled list of per-molecule records.  ``--level mol`` picks among the pooled 256-wide read-outs, ``--level frag`` among the 128-wide
fragment rows.  ``--seeds STORE``: its rows are centres before the first pick, so the picks are the rows of ``--data`` least like them.
The ``.npz`` holds ``picked`` / ``mol`` / ``frag`` ``[k]`` (pick order), ``radius`` ``[k + 1]`` (the coverage radius before every pick, and
after the last), ``distance`` / ``label`` ``[rows]`` (every row's distance to and number of its nearest pick; ``-1 - s`` for seed row
``s``), ``offsets`` ``[molecules + 1]``, ``level``, ``metric``, and with ``--split`` (level ``mol`` only) the sorted molecule indices
``train`` / ``valid`` / ``test``: whole clusters, dealt out largest first by the filling rule of the reference's scaffold split.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neighbours_gat2 import build_model          # noqa: E402  (one model builder for the embedding scripts)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="finetune YAML (exps/ft/*/config.yaml)")
    ap.add_argument("--checkpoint", required=True, help="state_dict of the finetuned model (finetune.chkpoint_name)")
    ap.add_argument("--data", required=True, help="flat store (.pt) or pickled list of molecule records")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--k", type=int, required=True, help="rows to pick")
    ap.add_argument("--level", default="mol", choices=("mol", "frag"), help="pooled read-outs [256] or fragment rows [128]")
    ap.add_argument("--metric", default="l2", choices=("l2", "cosine"))
    ap.add_argument("--seeds", help="flat store (.pt) or pickled record list whose rows are centres before the first pick")
    ap.add_argument("--split", type=float, nargs=3, metavar=("TRAIN", "VALID", "TEST"), help="fractions of a cluster split (level mol)")
    ap.add_argument("--batch-size", type=int, default=512, help="molecules per encoder pass")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if args.k < 0:
        ap.error("--k must not be negative")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    if args.split is not None and args.level != "mol":
        ap.error("--split needs --level mol")
    if args.split is not None and (min(args.split) < 0 or abs(sum(args.split) - 1) > 1e-6):
        ap.error("--split takes three non-negative fractions that add up to 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    import fragnet_amd
    from fragnet_amd import diversity, train
    from fragnet_amd.dataset import load_source
    cfg = train.load_config(args.config, config=args.config)
    fragnet_amd.prefer_rocblas_for_dense_heads()
    device = torch.device(args.device)
    model = build_model(cfg)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model.to(device)
    data = load_source(args.data, device)
    seeds = load_source(args.seeds, device) if args.seeds else None
    res = diversity.select(model, data, args.k, level=args.level, metric=args.metric, seeds=seeds, batch_size=args.batch_size)
    out = res.arrays()
    if args.split is not None:
        out.update(zip(("train", "valid", "test"), res.split(args.split)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    sizes = ", split " + " / ".join(str(out[name].shape[0]) for name in ("train", "valid", "test")) if args.split is not None else ""
    print(f"{len(res)} of {res.distance.shape[0]} rows ({len(res.offsets) - 1} molecules) picked, level {args.level}, {args.metric}, "
          f"coverage radius {float(res.radius[-1]):.6g}{sizes} -> {args.out}")


if __name__ == "__main__":
    main()
