#!/usr/bin/env python3
"""Counterpart of the reference's fragnet/train/finetune/finetune_cdrp.py: same CLI (--config X.yaml), same YAML schema (gene_dim,
finetune.*, pretrain.chkpoint_name -> model.drug_model.pretrain), same checkpoint format (plain state_dict), on the MI355X path.
Datasets are pickled lists of per-molecule records with a ``gene_expr`` vector (scripts/make_synthetic_cdrp_dataset.py writes synthetic ones).

    python scripts/finetune_cdrp.py --config exps/ft/cdrp_synth/config.yaml
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.utils.data import DataLoader

from fragnet_amd import data, train
from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
from fragnet_amd.dataset import load_pickle_dataset
from fragnet_amd.model import FragNetPreTrain


class _OnDevice:
    """a DataLoader whose batches arrive on the GPU (data.batch_to keeps the collate's layout promise)"""

    def __init__(self, loader, device):
        self.loader, self.device, self.dataset = loader, device, loader.dataset

    def __iter__(self):
        return (data.batch_to(b, self.device) for b in self.loader)

    def __len__(self):
        return len(self.loader)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config.yaml")
    cli = ap.parse_args()
    args = train.load_config(cli.config, config=cli.config)
    train.seed_everything(args.seed)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    exp_dir = args["exp_dir"]
    os.makedirs(exp_dir, exist_ok=True)
    ft = args.finetune
    if args.model_version != "gat2":
        raise SystemExit("CDRP: model_version gat2 is on the accelerated path")
    if ft.target_type != "regr":
        raise SystemExit("CDRP: target_type regr only")
    want_graph_step = train.check_pair_graph_step(ft)      # finetune.graph_step: true -- the training step as one hipGraph (graphstep.PairGraphedTrainStep)
    # finetune.factored_graph_step: true -- factored batches AND their training step as one hipGraph (graphstep.FactoredPairGraphedTrainStep)
    want_factored_step = train.check_factored_pair_graph_step(ft)
    model = CDRPModel(FragNetFineTuneBase(**train.finetune_model_kwargs(args)), int(args.gene_dim), device)
    pt = args.pretrain
    if pt.get("chkpoint_name") and os.path.exists(str(pt.chkpoint_name)):
        modelpt = FragNetPreTrain(**train.pretrain_model_kwargs(args))
        modelpt.load_state_dict(torch.load(pt.chkpoint_name, map_location="cpu"))
        model.drug_model.pretrain.load_state_dict(modelpt.pretrain.state_dict())
        print("loaded pretrained encoder", pt.chkpoint_name)
    model.to(device)
    sets = {k: load_pickle_dataset(ft[k].path) for k in ("train", "val", "test")}
    # finetune.factored_pairs: true -- every distinct drug and second input of a batch goes through its encoder once
    # (data.collate_fn_cdrp_factored); with drop_ratio > 0 a training step then draws one dropout mask per distinct drug, not per pair
    collate = data.collate_fn_cdrp_factored if ft.get("factored_pairs") or want_factored_step else data.collate_fn_cdrp
    train_loader = _OnDevice(DataLoader(sets["train"], collate_fn=collate, batch_size=ft.batch_size, shuffle=True, drop_last=True), device)
    val_loader = _OnDevice(DataLoader(sets["val"], collate_fn=collate, batch_size=64, shuffle=False), device)
    test_loader = _OnDevice(DataLoader(sets["test"], collate_fn=collate, batch_size=64, shuffle=False), device)
    trainer = train.TrainerFineTuneCDRP(target_type=ft.target_type)
    optimizer = train.make_optimizer(model, float(ft.lr), next(iter(train_loader)), lambda mdl, b: trainer._loss(mdl, b))
    graph_step = train.make_pair_graph_step(model, optimizer, train_loader, int(ft.model.num_heads)) if want_graph_step else None
    if want_factored_step:
        graph_step = train.make_factored_pair_graph_step(model, optimizer, train_loader, int(ft.model.num_heads))
    step_kw = {} if graph_step is None else {"graph_step": graph_step}      # absent by default: the launch-by-launch step, as ever
    # finetune.device_metrics: true -- validation and test scores from the metrics kernels (no host read per batch), Pearson and CI in the final lines
    device_metrics = bool(ft.get("device_metrics"))
    stopper = train.EarlyStopping(patience=ft.es_patience, verbose=True, chkpoint_name=ft.chkpoint_name)
    log = open(os.path.join(exp_dir, "log.jsonl"), "a")
    for epoch in range(ft.n_epochs):
        train_loss = trainer.train(model=model, loader=train_loader, optimizer=optimizer, scheduler=None, device=device, val_loader=val_loader,
                                   label_mean=None, label_sdev=None, **step_kw)
        if device_metrics:
            val_loss = trainer.evaluate(model=model, loader=val_loader, device=device)["mse"]
        else:
            val_loss, _, _ = trainer.test(model=model, loader=val_loader, device=device, label_mean=None, label_sdev=None)
        print("epoch: ", epoch, train_loss, val_loss, "" if graph_step is None else f"(graph replays {graph_step.replays}, eager fallbacks {graph_step.fallbacks})")
        log.write(json.dumps({"epoch": epoch, "Loss/train": train_loss, "Loss/val": val_loss}) + "\n")
        log.flush()
        stopper(val_loss, model)
        if stopper.early_stop:
            print("Early stopping")
            break
    model.load_state_dict(torch.load(ft.chkpoint_name, map_location=device))
    for name, loader in (("val_res", val_loader), ("test_res", test_loader)):
        if device_metrics:
            acc = train.save_predictions_on_device(trainer, loader, model, exp_dir, name, ft.loss, args.seed, device=device)
            print(f"{name} rmse: {acc} pearson: {trainer.last_metrics['pearson']} ci: {trainer.last_metrics['ci']}")
            continue
        acc = train.save_predictions(trainer, loader, model, exp_dir, name, ft.loss, args.seed)
        print(f"{name} rmse: {acc}")
