"""Training loops, config and checkpoint handling with the reference's semantics.

Counterparts of
  fragnet/train/utils.py:13-56      EarlyStopping (checkpoint = plain ``state_dict`` on every improvement)
  fragnet/train/utils.py:297-304    compute_bce_loss (masked BCE-with-logits)
  fragnet/train/utils.py:307-492    TrainerFineTune (train_regr / train_clsf_bce / validate / test)
  fragnet/train/pretrain/pretrain_utils.py:4-56   pretrain Trainer (2*MSE(dihedral)+MSE(angle)+MSE(energy): the
                                    bond-length term is overwritten before use there, reproduced here)
  fragnet/train/finetune/finetune_gat2.py:17-26,68-288 / pretrain/pretrain_gat2.py:79-183   drivers (see scripts/)
Config: one YAML per run with ``${key}`` interpolation and attribute + item access (the reference uses OmegaConf,
which is not installed in the build image; PyYAML + a 20-line resolver cover the schema of exps/**.yaml).

Loss values returned by ``train`` follow the reference's normalisation quirk: the sum of per-batch MEAN losses
divided by the number of molecules in the dataset (train/utils.py:351).
"""
from __future__ import annotations

import os
import pickle
import random
import re
from typing import Dict, Iterable, Optional

import numpy as np
import torch
import yaml

from . import _lib, parallel
from .dataset import BatchSampler, FlatMolStore


# ------------------------------------------------------------------------------------ config
class Config(dict):
    """dict with attribute access, recursively (args.finetune.model.h1 and args['exp_dir'] both work)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def _wrap(node):
    if isinstance(node, dict):
        return Config({k: _wrap(v) for k, v in node.items()})
    if isinstance(node, list):
        return [_wrap(v) for v in node]
    return node


def _resolve(node, root):
    if isinstance(node, dict):
        for k in node:
            node[k] = _resolve(node[k], root)
    elif isinstance(node, list):
        return [_resolve(v, root) for v in node]
    elif isinstance(node, str):
        def sub(mt):
            cur = root
            for part in mt.group(1).split("."):
                cur = cur[part]
            return str(cur)
        for _ in range(8):
            new = re.sub(r"\$\{([^}]+)\}", sub, node)
            if new == node:
                break
            node = new
    return node


def load_config(path: str, **overrides) -> Config:
    with open(path) as f:
        cfg = _wrap(yaml.safe_load(f))
    cfg.update(overrides)
    return _resolve(cfg, cfg)


def finetune_model_kwargs(cfg: Config) -> dict:
    """The fourteen constructor arguments that a finetune YAML gives a model -- ``FragNetFineTune`` and its Viz, GCN (which takes no
    ``num_heads``) and pair-model ``FragNetFineTuneBase`` relatives.  ``variant`` (``cfg.model_version``) is the caller's to add: not
    every class takes one."""
    m = cfg.finetune.model
    return dict(n_classes=m.n_classes, atom_features=cfg.atom_features, frag_features=cfg.frag_features, edge_features=cfg.edge_features,
                num_layer=m.num_layer, drop_ratio=m.drop_ratio, num_heads=m.num_heads, emb_dim=m.emb_dim, h1=m.h1, h2=m.h2, h3=m.h3,
                h4=m.h4, act=m.act, fthead=m.fthead)


def pretrain_model_kwargs(cfg: Config) -> dict:
    """The constructor arguments that a YAML's ``pretrain`` section and feature widths give ``FragNetPreTrain`` and its masked relatives."""
    pt = cfg.pretrain
    return dict(num_layer=pt.num_layer, drop_ratio=pt.drop_ratio, num_heads=pt.num_heads, emb_dim=pt.emb_dim,
                atom_features=cfg.atom_features, frag_features=cfg.frag_features, edge_features=cfg.edge_features,
                fedge_in=cfg.fedge_in, fbond_edge_in=cfg.fbond_edge_in)


def seed_everything(seed: int):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)


# ------------------------------------------------------------------------------------ early stopping / checkpoints
class EarlyStopping:
    def __init__(self, patience=7, verbose=False, delta=0, chkpoint_name="gnn_best.pt"):
        self.patience, self.verbose, self.delta, self.chkpoint_name = patience, verbose, delta, chkpoint_name
        self.counter, self.best_score, self.early_stop, self.val_loss_min = 0, None, False, float("inf")

    def __call__(self, val_loss, model):
        score = -val_loss
        if self.best_score is None or not (score < self.best_score + self.delta):
            self.best_score = score
            self.save_checkpoint(val_loss, model)
            self.counter = 0
        else:
            self.counter += 1
            if self.verbose:
                print(f"EarlyStopping counter: {self.counter} out of {self.patience}")
            if self.counter >= self.patience:
                self.early_stop = True

    def save_checkpoint(self, val_loss, model):
        if self.verbose:
            print(f"Validation loss decreased ({self.val_loss_min:.6f} --> {val_loss:.6f}).  Saving model ...")
        os.makedirs(os.path.dirname(os.path.abspath(self.chkpoint_name)), exist_ok=True)
        torch.save(model.state_dict(), self.chkpoint_name)
        self.val_loss_min = val_loss


# ------------------------------------------------------------------------------------ losses
def compute_bce_loss(prediction, target):
    valid = target > -0.5
    mat = torch.nn.functional.binary_cross_entropy_with_logits(prediction, target, reduction="none")
    return torch.where(valid, mat, torch.zeros_like(mat)).sum() / valid.sum()


def pretrain_loss(outputs, batch, scales=(1.0, 1.0)):
    """loss_lngth(:= MSE(dihedral)) + loss_angle + loss_lngth + loss_E.  ``scales`` = (per-edge, per-atom) weights
    that make rank-averaged gradients equal the global-mean gradients (parallel.weighted_loss_scale)."""
    _, ba, da, graph_rep = outputs
    mse = torch.nn.functional.mse_loss
    l_dh = mse(da, batch["dh_angl"]) * scales[0]
    return l_dh + mse(ba, batch["bnd_angl"]) * scales[1] + l_dh + mse(graph_rep.view(-1), batch["y"])


# ------------------------------------------------------------------------------------ loaders
class StoreLoader:
    """Iterates batch dicts from a FlatMolStore (on the GPU when the store lives there)."""

    def __init__(self, store: FlatMolStore, batch_size: int, shuffle=False, drop_last=False, pretrain=False, seed=0,
                 device=None, rank=0, world=1, prefetch=False):
        self.store, self.pretrain, self.device = store, pretrain, device
        self.sampler = BatchSampler(len(store), batch_size, shuffle, drop_last, seed, rank, world)
        self.dataset = store            # len(loader.dataset) is what the reference normalises losses by
        # prefetch (off by default): batch k + 1 is collated on a side stream while the consumer's step on batch k runs.  Measured on the
        # captured ESOL step: 0.894 ms per step against 0.836 with the collate's one launch simply in front of the step on the same stream
        # -- the second queue costs more than the 40 us it hides
        self.prefetch = bool(prefetch) and store.device.type == "cuda" and (device is None or torch.device(device) == store.device)
        self._side = None

    def __iter__(self):
        if self.prefetch:
            yield from self._iter_prefetch()
            return
        for idx in self.sampler:
            batch = self.store.collate(idx, pretrain=self.pretrain)       # host indices: the store sizes the batch without a device read-back
            if self.device is not None and batch["x_atoms"].device != torch.device(self.device):
                batch = {k: v.to(self.device, non_blocking=True) for k, v in batch.items()}
            yield batch

    def _iter_prefetch(self):
        dev = self.store.device
        if self._side is None:
            self._side = torch.cuda.Stream(dev)
        side = self._side

        def produce(idx):
            with torch.cuda.stream(side):
                b = self.store.collate(idx, pretrain=self.pretrain)
                ev = torch.cuda.Event()
                ev.record(side)
            return b, ev

        it = iter(self.sampler)
        try:
            nxt = produce(next(it))
        except StopIteration:
            return
        while nxt is not None:
            (batch, ev), nxt = nxt, None
            try:
                nxt = produce(next(it))           # enqueued before the consumer enqueues its step on `batch`
            except StopIteration:
                pass
            main = torch.cuda.current_stream(dev)
            main.wait_event(ev)
            # the tensors were allocated on the side stream and are read on the consumer's: the caching allocator must not hand their
            # memory to a later collate before that stream is done with them
            for v in list(batch.values()) + [getattr(batch, "offsets", None)] + list(getattr(batch, "_keep", ())):
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(main)
            yield batch

    def __len__(self):
        return len(self.sampler)


# ------------------------------------------------------------------------------------ trainers
def _on(batch, device):
    """The reference's trainers move every batch to ``device`` themselves (train/utils.py:335-336); so do these."""
    if device is None or batch["x_atoms"].device == torch.device(device):
        return batch
    return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}


class TrainerFineTune:
    def __init__(self, target_pos=None, target_type="regr", n_multi_task_heads=0):
        self.target_type = target_type
        if target_type == "regr":
            self.loss_fn = torch.nn.MSELoss()
        elif target_type == "clsf":
            self.loss_fn = compute_bce_loss
        else:
            raise NotImplementedError(f"target_type {target_type!r} is outside the FragNet gat2 hot path")

    def _loss(self, model, batch):
        out = model(batch)
        if self.target_type == "regr":
            return self.loss_fn(out.view(-1), batch["y"])
        return self.loss_fn(out, batch["y"].view(out.shape))

    @staticmethod
    def _shard_scale(batch):
        """local molecules * world / global molecules: rank-averaged gradients of per-rank MEAN losses then equal the gradient
        of the global mean when a batch does not divide evenly over the ranks (1.0 on a single rank)."""
        d = parallel.dist
        if not (d.is_available() and d.is_initialized()) or d.get_world_size() == 1:
            return 1.0
        return parallel.weighted_loss_scale(batch["y"].shape[0], batch["y"].device)

    def train(self, model, loader, optimizer, scheduler=None, device=None, val_loader=None, graph_step=None):
        """``optimizer``: torch.optim.Optimizer or parallel.FlatAdam.  ``graph_step``: a graphstep.GraphedTrainStep over
        the same model and optimiser -- every batch then costs one staging kernel, one hipGraph replay and the Adam
        kernel (batches beyond its capacities take the eager step inside it)."""
        model.train()
        total = 0.0
        losses = []
        for batch in loader:
            batch = _on(batch, device)
            if graph_step is not None:
                losses.append(graph_step(batch).clone())
                continue
            optimizer.zero_grad()
            loss = self._loss(model, batch)
            scale = self._shard_scale(batch)
            (loss * scale if scale != 1.0 else loss).backward()
            optimizer.step()
            losses.append(loss.detach())
        if losses:
            total = float(torch.stack(losses).sum())        # one synchronisation per epoch, not per step
        if scheduler:
            scheduler.step()
        return total / len(loader.dataset)

    @torch.no_grad()
    def validate(self, model, loader, device=None):
        model.eval()
        losses = [self._loss(model, _on(batch, device)) for batch in loader]
        return float(torch.stack(losses).sum()) / len(loader.dataset) if losses else 0.0

    @torch.no_grad()
    def test(self, model, loader, device=None):
        """regr: (mse, true, pred); clsf: (-mean ROC-AUC over tasks with both classes, true, pred) -- a LOSS, lower is
        better, exactly as the reference's test_clsf_bce returns it (train/utils.py:494-521), so a reference-style
        ``early_stopping(val_loss, model)`` loop keeps the best model."""
        model.eval()
        true, pred = [], []
        for batch in loader:
            batch = _on(batch, device)
            out = model(batch)
            true.append(batch["y"].reshape(out.shape[0], -1).cpu())
            pred.append(out.reshape(out.shape[0], -1).cpu())
        t, p = torch.cat(true).numpy(), torch.cat(pred).numpy()
        if self.target_type == "regr":
            return float(((t.ravel() - p.ravel()) ** 2).mean()), t.ravel(), p.ravel()
        from sklearn.metrics import roc_auc_score
        aucs = []
        for c in range(t.shape[1]):
            ok = t[:, c] > -0.5
            if ok.any() and len(np.unique(t[ok, c])) == 2:
                aucs.append(roc_auc_score(t[ok, c], p[ok, c]))
        return -float(np.mean(aucs)) if aucs else float("nan"), t, p

    # ---- the same evaluation with the metrics computed on the device (csrc/metrics.hip): no host read per batch, one at the end
    def _eval_norm(self, label_mean, label_sdev):
        """(shift, scale) applied to the model's output before it is compared with ``y``; only the DTA trainer de-normalises."""
        return 0.0, 1.0

    @torch.no_grad()
    def _eval_on_device(self, model, loader, device, label_mean, label_sdev):
        """-> (metrics dict, true, pred): the two as device tensors [rows, C] (classification) or [rows * C, 1] (regression, which
        ``test`` scores over all elements alike), ``pred`` de-normalised.  The model is put back into the mode it came in."""
        from . import metrics, ops
        shift, scale = self._eval_norm(label_mean, label_sdev)
        was_training = model.training
        model.eval()
        try:
            true = pred = None
            total, filled = len(loader.dataset), 0
            for batch in loader:
                batch = _on(batch, device)
                out = model(batch)
                rows = out.shape[0]
                out = out.reshape(rows, -1)
                if pred is None:
                    pred = torch.empty((total, out.shape[1]), dtype=torch.float32, device=out.device)
                    true = torch.empty_like(pred)
                if filled + rows > total:
                    raise ValueError(f"evaluate: the loader yields more than len(loader.dataset) = {total} rows")
                pred[filled:filled + rows].copy_(out)
                true[filled:filled + rows].copy_(batch["y"].reshape(rows, -1))
                filled += rows
        finally:
            model.train(was_training)
        if pred is None:
            raise ValueError("evaluate: the loader is empty")
        true, pred = true[:filled], pred[:filled]
        if self.target_type == "clsf":
            counts = ops.pair_concordance(pred, true, metrics.CLSF_LABEL_FLOOR).cpu()          # the one synchronisation
            auc = metrics.concordance_per_column(counts)
            neg_auc = -metrics.roc_auc(counts)
            return {"score": neg_auc, "neg_auc": neg_auc, "auc": auc}, true, pred
        true, pred = true.reshape(-1, 1), pred.reshape(-1, 1)
        sums = ops.regression_sums(pred, true, scale=scale, shift=shift)
        if (shift, scale) != (0.0, 1.0):
            # what the sums launch computed per element, now in place for the pair counts and the caller: an fp32 product, then an
            # fp32 sum -- the bits of numpy's ``p * float32(sdev) + float32(mean)`` in ``TrainerFineTuneDTA.test``
            pred = pred.mul(scale).add_(shift)
        counts = ops.pair_concordance(pred, true)
        both = torch.cat([sums.view(torch.uint8).reshape(-1), counts.view(torch.uint8).reshape(-1)]).cpu().numpy()       # the one synchronisation
        n_sums = sums.numel() * 8
        sums_h, counts_h = both[:n_sums].view(np.float64).reshape(sums.shape), both[n_sums:].view(np.int64).reshape(counts.shape)
        res = {k: float(v[0]) for k, v in metrics.regression_metrics(sums_h).items()}
        res["ci"] = metrics.concordance_index(counts_h)
        res["score"] = res["mse"]
        return res, true, pred

    def evaluate(self, model, loader, device=None, label_mean=None, label_sdev=None):
        """``test``'s pass with the metrics computed on the device: every batch's output and ``y`` go into their slice of two
        preallocated ``[len(loader.dataset), C]`` device buffers with no host read, one launch pair per metric table follows
        (ops.pair_concordance, ops.regression_sums), and the tables are copied back once.  Returns a dict --
        classification: ``neg_auc`` (``test``'s score: minus the mean ROC-AUC over the columns with both classes, NaN when none has)
        and ``auc`` (per column, NaN where undefined); regression: ``mse``, ``rmse``, ``mae``, ``pearson``, ``r2``, ``ci`` (the
        concordance index), in float64 from fp64 sums over all elements -- ``test``'s own mse is an fp32 numpy mean and differs from
        it at the 1e-7 level.  ``score`` is ``test``'s first return value either way.  A NaN prediction in a valid classification
        row raises.  The model's training / eval mode is left as it was."""
        return self._eval_on_device(model, loader, device, label_mean, label_sdev)[0]

    def test_on_device(self, model, loader, device=None, label_mean=None, label_sdev=None):
        """``(score, true, pred)`` as ``test`` returns them -- the arrays bit for bit, copied back once at the end -- with the score
        from ``evaluate``, whose whole dict is kept as ``self.last_metrics``."""
        res, true, pred = self._eval_on_device(model, loader, device, label_mean, label_sdev)
        self.last_metrics = res
        t, p = true.cpu().numpy(), pred.cpu().numpy()
        if self.target_type == "regr":
            t, p = t.ravel(), p.ravel()
        return res["score"], t, p


class TrainerFineTuneCDRP(TrainerFineTune):
    """The reference's ``trainer_cdrp.TrainerFineTune`` for a ``cdrp.CDRPModel`` (regression, MSE on ``model(batch).view(-1)``): the
    loops are ``TrainerFineTune``'s.  A training step takes the model's fused-loss call (last Linear pair, loss and its gradient in one
    launch).  ``label_mean`` / ``label_sdev`` are what the reference's driver passes and its trainer never reads; accepted and ignored."""

    def __init__(self, target_pos=None, target_type="regr", n_multi_task_heads=0):
        if target_type != "regr":
            raise NotImplementedError(f"target_type {target_type!r} is outside the FragNet gat2 hot path")
        super().__init__(target_pos=target_pos, target_type=target_type, n_multi_task_heads=n_multi_task_heads)

    def _loss(self, model, batch):
        if model.training and torch.is_grad_enabled():
            out, loss = model(batch, loss=(_lib.LOSS_MSE, batch["y"], None))
            if loss is not None:
                return loss
        else:
            out = model(batch)
        return self.loss_fn(out.view(-1), batch["y"])

    def train(self, model, loader, optimizer, scheduler=None, device=None, val_loader=None, label_mean=None, label_sdev=None, graph_step=None):
        """``graph_step``: a graphstep.PairGraphedTrainStep over the same model and optimiser (``TrainerFineTune.train``)."""
        return super().train(model, loader, optimizer, scheduler=scheduler, device=device, val_loader=val_loader, graph_step=graph_step)

    def validate(self, model, loader, device=None, label_mean=None, label_sdev=None):
        return super().validate(model, loader, device=device)

    def test(self, model, loader, device=None, label_mean=None, label_sdev=None):
        return super().test(model, loader, device=device)


class TrainerFineTuneDTA(TrainerFineTune):
    """The reference's ``trainer_dta.TrainerFineTune`` for a ``dta.DTAModel2`` (regression only).  Unlike the CDRP trainer this one USES
    ``label_mean`` / ``label_sdev``: ``train`` fits ``(y - mean) / (sdev + 1e-5)`` (trainer_dta.py:42), ``validate`` and ``test``
    de-normalise the output (``out * sdev + mean``) and compare it with the raw ``y`` (trainer_dta.py:65, 83).  A training step takes the
    model's fused-loss call on the normalised target.  Returned losses are sums of per-batch losses over ``len(loader.dataset)``, as in
    the reference.  The defaults mean = 0, sdev = 1 leave everything but the 1e-5 as it is."""

    def __init__(self, target_pos=None, target_type="regr", n_multi_task_heads=0):
        if target_type != "regr":
            raise NotImplementedError(f"target_type {target_type!r} is outside the FragNet gat2 hot path")
        super().__init__(target_pos=target_pos, target_type=target_type, n_multi_task_heads=n_multi_task_heads)
        self._norm = (0.0, 1.0)

    def _loss(self, model, batch):
        mean, sdev = self._norm
        if model.training and torch.is_grad_enabled():
            y = (batch["y"] - mean) / (sdev + 1e-5)
            out, loss = model(batch, loss=(_lib.LOSS_MSE, y, None))
            if loss is not None:
                return loss
            return self.loss_fn(out.view(-1), y)
        return self.loss_fn(model(batch).view(-1) * sdev + mean, batch["y"])

    @staticmethod
    def _stats(label_mean, label_sdev):
        return (0.0 if label_mean is None else float(label_mean), 1.0 if label_sdev is None else float(label_sdev))

    def _eval_norm(self, label_mean, label_sdev):
        return self._stats(label_mean, label_sdev)

    def train(self, model, loader, optimizer, scheduler=None, device=None, val_loader=None, label_mean=None, label_sdev=None, graph_step=None):
        """``graph_step``: a graphstep.PairGraphedTrainStep over the same model and optimiser.  It stages the NORMALISED target, computed
        from this call's ``label_mean`` / ``label_sdev`` in front of its staging launch: the two may change from call to call."""
        self._norm = self._stats(label_mean, label_sdev)
        if graph_step is not None:
            graph_step.target_norm = self._norm
        return super().train(model, loader, optimizer, scheduler=scheduler, device=device, val_loader=val_loader, graph_step=graph_step)

    def validate(self, model, loader, device=None, label_mean=None, label_sdev=None):
        self._norm = self._stats(label_mean, label_sdev)
        return super().validate(model, loader, device=device)

    def test(self, model, loader, device=None, label_mean=None, label_sdev=None):
        """(mse, true, pred) with ``pred`` de-normalised."""
        mean, sdev = self._stats(label_mean, label_sdev)
        _, t, p = super().test(model, loader, device=device)
        p = p * np.float32(sdev) + np.float32(mean)
        return float(((t - p) ** 2).mean()), t, p


class PretrainTrainer:
    def __init__(self, loss_fn=None):
        self.loss_fn = loss_fn

    def train(self, model, loader, optimizer, device=None, graph_step=None):
        model.train()
        losses = []
        for batch in loader:
            batch = _on(batch, device)
            if graph_step is not None:          # graphstep.GraphedTrainStep(..., loss="pretrain")
                losses.append(graph_step(batch).clone())
                continue
            optimizer.zero_grad()
            scales = (1.0, 1.0)
            if parallel.dist.is_available() and parallel.dist.is_initialized() and parallel.dist.get_world_size() > 1:
                dev = batch["x_atoms"].device
                scales = (parallel.weighted_loss_scale(batch["dh_angl"].shape[0], dev),
                          parallel.weighted_loss_scale(batch["bnd_angl"].shape[0], dev))
            loss = pretrain_loss(model(batch), batch, scales)
            loss.backward()
            optimizer.step()
            losses.append(loss.detach())
        return float(torch.stack(losses).sum()) / len(loader.dataset) if losses else 0.0

    @torch.no_grad()
    def validate(self, loader, model, device=None):
        model.eval()
        losses = [pretrain_loss(model(b), b) for b in (_on(batch, device) for batch in loader)]
        return float(torch.stack(losses).sum()) / len(loader.dataset) if losses else 0.0


def make_optimizer(model, lr: float, probe_batch: Optional[Dict[str, torch.Tensor]] = None, loss_of=None):
    """parallel.FlatAdam over the live parameters when a probe batch is given (GPU path), else torch Adam."""
    if probe_batch is None:
        return torch.optim.Adam(model.parameters(), lr=lr)

    def probe():
        was = model.training
        model.train()
        loss_of(model, probe_batch).backward()
        model.train(was)
    return parallel.FlatAdam.for_live_parameters(model, probe, lr=lr)


def check_pair_graph_step(ft) -> bool:
    """``finetune.graph_step`` of the pair drivers (scripts/finetune_cdrp.py, finetune_dta.py): absent means off.  The captured step
    covers one-record-per-pair batches only, so together with ``finetune.factored_pairs`` it is a configuration error."""
    if not ft.get("graph_step"):
        return False
    if ft.get("factored_pairs"):
        raise SystemExit("finetune.graph_step and finetune.factored_pairs exclude each other: the captured pair step takes one-record-per-pair "
                         "batches (a factored batch would run eagerly, every step)")
    return True


def make_pair_graph_step(model, optimizer, train_loader, heads: int):
    """The drivers' ``graphstep.PairGraphedTrainStep``: capacities from eight training batches (margin 5 %), captured on the first."""
    from . import graphstep
    sample = [b for _, b in zip(range(8), iter(train_loader))]
    shapes = graphstep.StaticShapes.from_batches(sample, margin=0.05, heads=heads)
    model.train()
    return graphstep.PairGraphedTrainStep(model, optimizer, shapes, sample[0])


def check_factored_pair_graph_step(ft) -> bool:
    """``finetune.factored_graph_step`` of the pair drivers: absent means off.  It selects the factored collate AND the captured step
    built for it (graphstep.FactoredPairGraphedTrainStep), so together with ``finetune.graph_step`` -- the captured step on
    one-record-per-pair batches -- it is a configuration error."""
    if not ft.get("factored_graph_step"):
        return False
    if ft.get("graph_step"):
        raise SystemExit("finetune.factored_graph_step and finetune.graph_step exclude each other: each captures the training step, the "
                         "first on factored batches, the second on one-record-per-pair batches")
    return True


def make_factored_pair_graph_step(model, optimizer, train_loader, heads: int):
    """The drivers' ``graphstep.FactoredPairGraphedTrainStep``: capacities from eight training batches (margin 5 %; the numbers of distinct
    drugs and second inputs vary from batch to batch, so those two grow by it as well), captured on the first."""
    from . import graphstep
    sample = [b for _, b in zip(range(8), iter(train_loader))]
    shapes = graphstep.FactoredPairShapes.from_batches(sample, margin=0.05, heads=heads)
    model.train()
    return graphstep.FactoredPairGraphedTrainStep(model, optimizer, shapes, sample[0])


def save_predictions(trainer, loader, model, exp_dir, save_name="test_res", loss_type="mse", seed=123):
    score, true, pred = trainer.test(model=model, loader=loader)
    acc = score ** 0.5 if loss_type == "mse" else score
    os.makedirs(exp_dir, exist_ok=True)
    with open(os.path.join(exp_dir, f"{save_name}_{seed}.pkl"), "wb") as f:
        pickle.dump({"acc": acc, "true": true, "pred": pred, "smiles": getattr(loader.dataset, "smiles", None)}, f)
    return acc


def save_predictions_on_device(trainer, loader, model, exp_dir, save_name="test_res", loss_type="mse", seed=123, **test_kw):
    """``save_predictions`` with the pass and the score from ``trainer.test_on_device`` (``finetune.device_metrics`` of the drivers);
    the pickle is the same.  ``trainer.last_metrics`` holds every metric of the pass afterwards."""
    class _OnDevice:
        @staticmethod
        def test(model, loader):
            return trainer.test_on_device(model=model, loader=loader, **test_kw)
    return save_predictions(_OnDevice, loader, model, exp_dir, save_name, loss_type, seed)
