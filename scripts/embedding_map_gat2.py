#!/usr/bin/env python3
"""The chemical-space map of a library in the embedding space of a finetuned model, and the Mahalanobis applicability domain of a set
of query molecules in it, on the engine (fragnet_amd/chemspace.py).

    python scripts/embedding_map_gat2.py --config exps/ft/esol_synth/config.yaml --checkpoint exps/ft/esol_synth/ft.pt \\
        --library finetune_data/esol_synth/train.pt --queries finetune_data/esol_synth/test.pt --out map.npz

``--config`` is the finetune YAML (the model's shape and ``model_version`` -- gat2, gat2_lite, gat2_edge or gcn2 -- are read from it, as
scripts/finetune_gat2.py does), ``--checkpoint`` a plain state_dict of the finetuned model, ``--library`` / ``--queries`` a flat store
(``.pt``) or a pickled list of per-molecule records each; ``--queries`` may be left out.  ``--level mol`` maps the pooled 256-wide
read-outs, ``--level frag`` the 128-wide fragment rows.  The space (PCA of the library's rows) is fitted on the library.  The ``.npz``
holds ``coords`` ``[library rows, k]`` and ``d2`` ``[library rows]`` (PCA coordinates, squared Mahalanobis distance), ``mol`` / ``frag``
/ ``offsets``, the same with ``query_`` in front for the queries, ``domain_cutoff`` (the ``--quantile`` of the library's own ``d2``),
``inside`` ``[query rows]``, and the fitted space: ``n``, ``mean``, ``eigenvalues``, ``components``, ``rank``, ``floor``,
``explained_variance_ratio``.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VERSIONS = ("gat2", "gat2_lite", "gat2_edge", "gcn2")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="finetune YAML (exps/ft/*/config.yaml)")
    ap.add_argument("--checkpoint", required=True, help="state_dict of the finetuned model (finetune.chkpoint_name)")
    ap.add_argument("--library", required=True, help="flat store (.pt) or pickled list of molecule records: the space is fitted on it")
    ap.add_argument("--queries", default=None, help="flat store (.pt) or pickled list of molecule records (optional)")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--level", default="mol", choices=("mol", "frag"), help="pooled read-outs [256] or fragment rows [128]")
    ap.add_argument("--k", type=int, default=2, help="PCA coordinates per row, 1..width (at most the rank of the fitted space)")
    ap.add_argument("--quantile", type=float, default=0.95, help="the library's own quantile of d2 that bounds the domain")
    ap.add_argument("--batch-size", type=int, default=512, help="molecules per encoder pass")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be positive")
    if not 1 <= args.k <= (256 if args.level == "mol" else 128):
        ap.error("--k must be in 1..256 (--level mol) or 1..128 (--level frag)")
    if not 0.0 <= args.quantile <= 1.0:
        ap.error("--quantile must be in [0, 1]")
    if not args.out.endswith(".npz"):
        ap.error("--out must end in .npz")
    return args


def build_model(cfg):
    from fragnet_amd import train
    if cfg.model_version not in VERSIONS:
        raise SystemExit(f"model_version {cfg.model_version!r}: embeddings exist for {', '.join(VERSIONS)}")
    kw = train.finetune_model_kwargs(cfg)
    if cfg.model_version == "gcn2":          # (the graph-convolution baseline takes no num_heads, scripts/finetune_gat2.py)
        from fragnet_amd.gcn import FragNetFineTune as FragNetFineTuneGCN
        del kw["num_heads"]
        return FragNetFineTuneGCN(**kw)
    from fragnet_amd.model import FragNetFineTune
    return FragNetFineTune(**kw, variant=cfg.model_version)


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    import fragnet_amd
    from fragnet_amd import chemspace, train
    from fragnet_amd.dataset import load_source
    cfg = train.load_config(args.config, config=args.config)
    fragnet_amd.prefer_rocblas_for_dense_heads()
    device = torch.device(args.device)
    model = build_model(cfg)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model.to(device)
    library = load_source(args.library, device)
    queries = None
    if args.queries is not None:
        queries = library if os.path.abspath(args.queries) == os.path.abspath(args.library) else load_source(args.queries, device)
    res = chemspace.map(model, library, queries, level=args.level, k=args.k, quantile=args.quantile, batch_size=args.batch_size)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **res.arrays())
    print(f"{len(res.offsets) - 1} library molecules ({len(res)} rows), rank {res.space.rank} of {res.space.width}, "
          f"{100 * res.space.explained_variance_ratio[:args.k].sum():.1f} % of the variance in {args.k} coordinates; "
          f"{len(res.query_offsets) - 1} query molecules ({res.query_d2.shape[0]} rows), {int(res.inside.sum())} inside the "
          f"{args.quantile:g} quantile (d2 <= {res.domain_cutoff:.4g}), level {args.level} -> {args.out}")


if __name__ == "__main__":
    main()
