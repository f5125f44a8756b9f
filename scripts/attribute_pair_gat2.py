#!/usr/bin/env python3
"""Attributions of a finetuned pair model -- cancer drug response (``--model cdrp``) or drug-target affinity (``--model dta``) -- for a
whole dataset (fragnet_amd/pair_attribution.py).  The pair heads are affine, so a prediction is ``<drug_enc, v_d> + <second_enc, v_s> +
const`` and each side is explained on its own.

    python scripts/attribute_pair_gat2.py --model cdrp --side second --config exps/ft/cdrp_synth/config.yaml \\
        --checkpoint exps/ft/cdrp_synth/ft.pt --data finetune_data/cdrp_synth/test.pkl --method ig --steps 32 --out genes.npz

``--config`` is the finetune YAML of scripts/finetune_cdrp.py / finetune_dta.py, ``--checkpoint`` a plain state_dict, ``--data`` a pickled
list of pair records.

``--side second``: the cell lines' genes (cdrp: ``--method grad_x_input`` or ``ig``, zero baseline) or the proteins' residues (dta: the
tower is linear, gradient x input is exact and the only method).  Records that share a cell line / protein are attributed once:
``rows [n_records]`` maps a record to its row of ``attr [n_distinct, gene_dim or length]``; ``score`` is ``<second_enc, v_s>``.  cdrp
with ig adds ``score_baseline``, ``gap`` and ``steps``; dta adds ``attr_other`` (the bias terms) and ``table [length, 26]``.
``--side drug``: atoms, bonds and fragment connections of every record's molecule, laid out as scripts/attribute_gradients_gat2.py
writes them; ``pred`` is the scalar ``<drug_enc, v_d>``, not the model's prediction.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

METHODS = ("grad_x_input", "ig")


def parse_args(argv=None):
    from fragnet_amd import attribution, ops
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, choices=("cdrp", "dta"))
    ap.add_argument("--side", required=True, choices=("second", "drug"))
    ap.add_argument("--config", required=True, help="finetune YAML (exps/ft/*/config.yaml)")
    ap.add_argument("--checkpoint", required=True, help="state_dict of the finetuned pair model (finetune.chkpoint_name)")
    ap.add_argument("--data", required=True, help="pickled list of pair records")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--method", default="grad_x_input", choices=METHODS)
    ap.add_argument("--steps", type=int, default=32, help="ig: nodes of the midpoint rule")
    ap.add_argument("--max-rows", type=int, default=None, help=f"ig: rows per launch (cell lines * steps, at most {ops.DENSE_MAX_ROWS}; drug side: "
                    f"atom + directed-bond rows per replica batch, default {attribution.DEFAULT_MAX_ROWS})")
    ap.add_argument("--batch-size", type=int, default=512, help="drug side: molecules per evaluation batch")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.batch_size < 1 or (args.max_rows is not None and args.max_rows < 1):
        ap.error("--steps, --max-rows and --batch-size must be positive")
    if args.model == "dta" and args.side == "second" and args.method != "grad_x_input":
        ap.error("--model dta --side second: the protein tower is linear, gradient x input is exact (--method grad_x_input)")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    return args


def build_model(cfg, kind, device):
    from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
    from fragnet_amd.dta import DTAModel2
    from fragnet_amd.train import finetune_model_kwargs
    if cfg.model_version != "gat2":
        raise SystemExit(f"model_version {cfg.model_version!r}: the pair models run model_version gat2")
    drug = FragNetFineTuneBase(**finetune_model_kwargs(cfg))
    return CDRPModel(drug, int(cfg.gene_dim), device) if kind == "cdrp" else DTAModel2(drug)


def distinct_rows(records, field):
    """(int64 [n_distinct, width] in order of first appearance, row of every record) of the records' second input, cast as the collate
    functions cast it."""
    import numpy as np
    import torch
    table = torch.cat([getattr(r, field).view(1, -1) for r in records], dim=0).type(torch.long).numpy()
    seen, rows, keep = {}, np.empty(len(records), dtype=np.int64), []
    for i, row in enumerate(table):
        key = row.tobytes()
        if key not in seen:
            seen[key] = len(keep)
            keep.append(i)
        rows[i] = seen[key]
    return torch.from_numpy(table[keep]), rows


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from fragnet_amd import attribution, ops, train
    from fragnet_amd import pair_attribution as pa
    from fragnet_amd.dataset import load_pickle_dataset
    cfg = train.load_config(args.config, config=args.config)
    device = torch.device(args.device)
    model = build_model(cfg, args.model, device)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model.to(device).eval()
    records = load_pickle_dataset(args.data)
    if args.side == "drug":
        res = pa.drug_attributions(model, records, method=args.method, steps=args.steps, batch_size=args.batch_size,
                                   max_rows=args.max_rows or attribution.DEFAULT_MAX_ROWS)
        arrays = res.arrays()
        what = f"{len(res)} molecules, {sum(int(res.tables[k]['offsets'][-1]) for k in res.kinds)} attributed entries"
    else:
        second, rows = distinct_rows(records, "gene_expr" if args.model == "cdrp" else "protein")
        if args.model == "cdrp":
            res = pa.cell_line_attributions(model, second, method=args.method, steps=args.steps, max_rows=args.max_rows or ops.DENSE_MAX_ROWS)
        else:
            res = pa.protein_attributions(model, second)
        arrays = dict(res.arrays(), rows=rows)
        what = f"{len(records)} records, {len(res)} distinct {'cell lines' if args.model == 'cdrp' else 'proteins'} x {res.attr.shape[1]}"
    gap = arrays.get("gap")
    extra = f", {args.steps} steps, max |gap| {float(np.abs(gap).max()):.3e}" if gap is not None and gap.size else ""
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print(f"{what} ({args.model}, {args.side} side, {args.method}{extra}) -> {args.out}")


if __name__ == "__main__":
    main()
