#!/usr/bin/env python3
"""Gradient attributions of a finetuned model for a whole dataset: gradient x input, or integrated gradients, of one output column
with respect to the atom, bond-node and fragment-connection feature tables, batched on the engine
(fragnet_amd/gradient_attribution.py).  The companion of scripts/attribute_gat2.py (leave-one-out masking): same inputs, entries
in the same order.

    python scripts/attribute_gradients_gat2.py --config exps/ft/esol_synth/config.yaml --checkpoint exps/ft/esol_synth/ft.pt \\
        --data finetune_data/esol_synth/test.pt --method ig --steps 32 --out ig.npz

``--config`` is the finetune YAML (model_version gat2 or gat2_lite), ``--checkpoint`` a plain state_dict, ``--data`` a flat store
(``.pt``) or a pickled list of per-molecule records.  The ``.npz`` holds flat arrays plus per-molecule offsets: ``pred [n_mols]`` (the
``--target`` column), ``attr_other [n_mols]``, and per kind k in atom / bond / fbond ``k_offsets [n_mols + 1]``, ``k_index``,
``k_attr`` -- rows ``k_offsets[i] : k_offsets[i + 1]`` are molecule i's, indexed as attribute_gat2.py indexes them.  ``--method ig``
adds ``pred_baseline``, ``gap`` (= pred - pred_baseline - all attributions: the completeness remainder) and ``steps``; the baseline
is zeros.  ``--gradients`` (grad_x_input only) adds the raw gradient tables ``grad_<table>``.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

METHODS = ("grad_x_input", "ig")


def parse_args(argv=None):
    from fragnet_amd import attribution
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="finetune YAML (exps/ft/*/config.yaml)")
    ap.add_argument("--checkpoint", required=True, help="state_dict of the finetuned model (finetune.chkpoint_name)")
    ap.add_argument("--data", required=True, help="flat store (.pt) or pickled list of molecule records")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--method", default="grad_x_input", choices=METHODS)
    ap.add_argument("--steps", type=int, default=32, help="ig: nodes of the midpoint rule")
    ap.add_argument("--target", type=int, default=0, help="output column that is differentiated")
    ap.add_argument("--gradients", action="store_true", help="grad_x_input: also write the raw gradient tables")
    ap.add_argument("--max-rows", type=int, default=attribution.DEFAULT_MAX_ROWS, help="ig: atom + directed-bond rows per replica batch")
    ap.add_argument("--batch-size", type=int, default=512, help="molecules per evaluation batch")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.max_rows < 1 or args.batch_size < 1:
        ap.error("--steps, --max-rows and --batch-size must be positive")
    if args.target < 0:
        ap.error("--target must not be negative")
    if args.gradients and args.method != "grad_x_input":
        ap.error("--gradients goes with --method grad_x_input")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    return args


def build_model(cfg):
    from fragnet_amd import train
    from fragnet_amd.model import FragNetFineTune
    if cfg.model_version not in ("gat2", "gat2_lite"):
        raise SystemExit(f"model_version {cfg.model_version!r}: the engine differentiates its inputs for gat2 and gat2_lite")
    return FragNetFineTune(**train.finetune_model_kwargs(cfg), variant=cfg.model_version)


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    import fragnet_amd
    from fragnet_amd import gradient_attribution as ga
    from fragnet_amd import train
    from fragnet_amd.dataset import load_source
    cfg = train.load_config(args.config, config=args.config)
    fragnet_amd.prefer_rocblas_for_dense_heads()
    device = torch.device(args.device)
    model = build_model(cfg)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model.to(device)
    source = load_source(args.data, device)
    if args.method == "ig":
        res = ga.integrated_gradients(model, source, steps=args.steps, target=args.target, max_rows=args.max_rows, batch_size=args.batch_size)
    else:
        res = ga.input_gradients(model, source, target=args.target, batch_size=args.batch_size, return_gradients=args.gradients)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **res.arrays())
    n_ent = sum(int(res.tables[k]["offsets"][-1]) for k in res.kinds)
    extra = f", {args.steps} steps, max |gap| {float(np.abs(res.gap).max()):.3e}" if args.method == "ig" else ""
    print(f"{len(res)} molecules, {n_ent} attributed entries ({args.method}, column {args.target}{extra}) -> {args.out}")


if __name__ == "__main__":
    main()
