#!/usr/bin/env python3
"""Counterpart of the reference's fragnet/train/pretrain/pretrain_gat2.py: same CLI and YAML schema
(exps/pt/unimol_exp1s4/config.yaml), data parallel over the GPUs of one node with one flat all-reduce per step."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fragnet_amd import parallel, train
from fragnet_amd.dataset import FlatMolStore
from fragnet_amd.model import FragNetPreTrain, FragNetPreTrainMasked2


def build_model(args):
    """The reference's dispatch on ``model_version`` (pretrain_gat2.py:97-128).  gat2 (or no key): FragNetPreTrain; gat2_masked2:
    FragNetPreTrainMasked2 with ``pretrain.mask_ratio`` (optional, 0.15 = the reference's literal 0.85 kept); gat2_masked: refused, the
    reference's class cannot train; anything else: refused (the reference would fail later, with ``model`` unbound)."""
    pt = args.pretrain
    version = args.get("model_version") or "gat2"
    kw = train.pretrain_model_kwargs(args)
    if version == "gat2":
        return FragNetPreTrain(**kw)
    if version == "gat2_masked2":
        ratio = pt.get("mask_ratio")
        return FragNetPreTrainMasked2(**kw, mask_ratio=0.15 if ratio is None else float(ratio))
    if version == "gat2_masked":
        raise SystemExit("model_version gat2_masked: the reference's FragNetPreTrainMasked.forward returns None (pretrain_heads.py:174-184 "
                         "ends without a return), so it cannot be trained there either; use gat2_masked2")
    raise SystemExit(f"model_version {version!r}: pretrain_gat2 knows gat2, gat2_masked2 (and refuses gat2_masked)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config.yaml")
    cli = ap.parse_args()
    args = train.load_config(cli.config, config=cli.config)
    train.seed_everything(args.seed)
    import fragnet_amd
    fragnet_amd.prefer_rocblas_for_dense_heads()
    fragnet_amd.tune_library_gemms()
    rank, local_rank, world = parallel.init_distributed()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    exp_dir = args["exp_dir"]
    os.makedirs(exp_dir, exist_ok=True)
    pt = args.pretrain
    model = build_model(args)
    if pt.get("saved_checkpoint"):
        model.load_state_dict(torch.load(pt.saved_checkpoint, map_location="cpu"))
    model.to(device)
    model.pretrain.rng.rank = rank
    if hasattr(model, "mask_rng"):
        model.mask_rng.rank = rank          # data-parallel ranks draw different masks
    # pretrain.data: list of directories holding train.pt / val.pt flat stores (the reference splits 90/10 itself,
    # pretrain_gat2.py:141; the synthetic stores come pre-split)
    d0 = pt.data[0]
    train_store = FlatMolStore.load(os.path.join(d0, "train.pt"), device=device)
    val_store = FlatMolStore.load(os.path.join(d0, "val.pt"), device=device)
    train_loader = train.StoreLoader(train_store, pt.batch_size, shuffle=True, drop_last=True, pretrain=True, seed=args.seed,
                                     rank=rank, world=world)
    val_loader = train.StoreLoader(val_store, pt.batch_size, pretrain=True)
    trainer = train.PretrainTrainer()
    probe = next(iter(train_loader))
    optimizer = train.make_optimizer(model, float(pt.lr), probe, lambda mdl, b: train.pretrain_loss(mdl(b), b))
    graph_step = None
    if pt.get("graph_step", True):      # whole-step hipGraph over static shapes; `pretrain.graph_step: false` = eager step
        from fragnet_amd import graphstep
        sample = [probe] + [b for _, b in zip(range(7), iter(train_loader))]
        shapes = graphstep.StaticShapes.from_batches(sample, margin=0.05, heads=pt.num_heads)
        model.train()
        graph_step = graphstep.GraphedTrainStep(model, optimizer, shapes, probe, loss="pretrain")
    stopper = train.EarlyStopping(patience=pt.es_patience, verbose=rank == 0, chkpoint_name=pt.chkpoint_name)
    every = int(pt.get("valdiate_every", 5))          # sic: the reference's key
    log = open(os.path.join(exp_dir, "log.jsonl"), "a") if rank == 0 else None
    for epoch in range(pt.n_epochs):
        train_loss = trainer.train(model, train_loader, optimizer, graph_step=graph_step)
        rec = {"epoch": epoch, "Loss/train": train_loss}
        if epoch % every == 0:
            val_loss = trainer.validate(val_loader, model)
            rec["Loss/val"] = val_loss
            if rank == 0:
                stopper(val_loss, model)
        if rank == 0:
            print(rec)
            log.write(json.dumps(rec) + "\n")
            log.flush()
        stop = torch.tensor([int(stopper.early_stop)], device=device)
        if world > 1:
            torch.distributed.broadcast(stop, 0)
        if int(stop):
            break
