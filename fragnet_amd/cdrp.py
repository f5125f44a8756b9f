"""Cancer drug response prediction (CDRP): the reference's third application of FragNet, on the MI355X path.

Counterpart of ``fragnet/model/cdrp/model.py`` (``MLP``, ``CDRPModel``) and of the ``FragNetFineTuneBase`` class that
``fragnet/train/finetune/finetune_cdrp.py:65-106`` defines for it.  Same module tree, attribute creation order and constructor
signatures, so a reference checkpoint loads with ``load_state_dict(strict=True)`` and the same ``torch.manual_seed`` gives the same
initial parameters (tests/golden/cdrp_b5.npz pins both).

On GPU tensors ``CDRPModel.forward`` is: encoder engine -> pooled [B, 256] read-out, cell-line tower (``ops.cell_tower``) and pair head
(``ops.pair_head``), all hand-written HIP (csrc/cdrp.hip beside the encoder's kernels): no library GEMM and no ``torch.cat``.  There is
no CPU path, as everywhere in fragnet_amd.
"""
from __future__ import annotations

import torch.nn as nn

from . import ops
from .data import PAIR_DRUG_KEY, PAIR_GRID_KEY, PAIR_ORDER_KEYS, PAIR_SECOND_KEY
from .model import FragNet, FTHead1, FTHead2, FTHead3, FTHead4, pooled


class FragNetFineTuneBase(nn.Module):
    """The drug encoder of a CDRP model: ``pretrain`` (FragNet) and a ``fthead`` that is built but never called -- the reference builds
    it too, so the state-dict keys and the order of the initialisation draws stay the reference's.  ``forward`` returns the pooled
    read-out cat(sum of atoms, sum of fragments) [B, 256]."""

    def __init__(self, n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=4, num_heads=4, drop_ratio=0.15,
                 h1=256, h2=256, h3=256, h4=256, act="celu", emb_dim=128, fthead="FTHead3"):
        super().__init__()
        self.pretrain = FragNet(num_layer=num_layer, drop_ratio=drop_ratio, num_heads=num_heads, emb_dim=emb_dim,
                                atom_features=atom_features, frag_features=frag_features, edge_features=edge_features)
        if fthead == "FTHead1":
            self.fthead = FTHead1(n_classes=n_classes)
        elif fthead == "FTHead2":
            self.fthead = FTHead2(n_classes=n_classes)
        elif fthead == "FTHead3":
            self.fthead = FTHead3(n_classes=n_classes, h1=h1, h2=h2, h3=h3, h4=h4, drop_ratio=drop_ratio, act=act)
        elif fthead == "FTHead4":
            self.fthead = FTHead4(n_classes=n_classes, h1=h1, drop_ratio=drop_ratio, act=act)

    def forward(self, batch):
        x_atoms, x_frags, _, _ = self.pretrain(batch, edge_outputs=False)
        return pooled(x_atoms, x_frags, batch)


class MLP(nn.Module):
    """The cell-line tower: Linear gene_dim -> 1024 -> 256 -> 64 -> 256 with a ReLU after every Linear (the last one included), on the
    int64 ``gene_expr`` rows of ``collate_fn_cdrp``."""

    def __init__(self, gene_dim=903, device="cuda"):
        super().__init__()
        self.device = device
        dims = [gene_dim, 1024, 256, 64, 256]
        self.predictor = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])

    def forward(self, v):
        return ops.cell_tower(v, self.predictor)


class CDRPModel(nn.Module):
    def __init__(self, drug_model, gene_dim, device):
        super().__init__()
        self.drug_model = drug_model
        self.fc1 = nn.Linear(256 + 256, 128)
        self.fc2 = nn.Linear(128, 1)
        self.cell_model = MLP(gene_dim, device)

    def forward(self, batch, loss=None):
        """``loss = (_lib.LOSS_MSE, y, None)``: the fused-loss call of a training step (``ops.pair_head``); returns ``(out, loss)``, ``loss``
        None where the fused launch does not apply.  ``(_lib.LOSS_MSE, y, None, real_rows)``: a batch staged to static shapes
        (graphstep.PairGraphedTrainStep), the mean over its first ``*real_rows`` rows.
        A factored batch (``data.collate_fn_cdrp_factored``, ``data.as_factored``: it carries ``pair_drug``) runs the encoder on its U distinct drugs, the tower on its C distinct cell lines and ``ops.pair_head_factored``: [M, 1]
        in pair order.  A grid batch (``data.pair_grid_batch``) returns every drug against every cell line, [U, C]."""
        drug_enc = self.drug_model(batch)
        cell_enc = self.cell_model(batch["gene_expr"])
        if batch.get(PAIR_GRID_KEY):
            return ops.pair_head_grid(drug_enc, cell_enc, self.fc1, self.fc2)
        if PAIR_DRUG_KEY in batch:
            return ops.pair_head_factored(drug_enc, cell_enc, batch[PAIR_DRUG_KEY], batch[PAIR_SECOND_KEY], self.fc1, self.fc2, loss=loss,
                                          orderings=pair_orderings_of(batch), check=False)
        return ops.pair_head(drug_enc, cell_enc, self.fc1, self.fc2, loss=loss)


def pair_orderings_of(batch):
    """The pair orderings a factored batch carries (``data.PAIR_ORDER_KEYS``), None where it has none: the head then builds them."""
    return tuple(batch[k] for k in PAIR_ORDER_KEYS) if all(k in batch for k in PAIR_ORDER_KEYS) else None
