"""The reference's attention-read-out models (fragnet/vizualize/model.py:45-280) on the MI355X kernels:

  FragNetViz              :45-143    the encoder; its last layer is built with ``return_attentions=True``
  FragNetFineTuneViz      :146-201   (prediction, attn_atoms, attn_frags, attn_bonds, attn_fbonds)
  FragNetFineTuneBaseViz  :205-250   the readout cat(sum of atoms, sum of fragments) per molecule
  FragNetPreTrainViz      :256-280   (graph_rep, attn_atoms, attn_frags, attn_bonds, attn_fbonds)

Constructor signatures, defaults (``edge_features`` is 16 for the finetune and pretrain classes and 17 for the other two, as there),
construction order (= RNG order), return tuples and state-dict keys are the reference's: ``pretrain.layers.{i}.*``, ``fthead.*``,
``head.*``, so ``load_state_dict`` of a FragNetFineTune / FragNetPreTrain checkpoint works with ``strict=True``.  As there, ``num_layer``
counts a first, ``num_layer - 2`` inner and a last layer (``num_layer=1`` builds two).

The four attention tensors are the LAST layer's ``scatter_add(attn_probs, source)`` (gat2.py:219, 312, 165, 268): per node of a
level and head, the attention its out-edges receive.  ``FragNet.route(batch, attn=True)`` decides the way: in ``eval()`` mode, with no
gradient required, the whole model is ONE engine pass ("engine-attn": ``FragNet._engine(..., attn_readout=True)`` ->
fn_encoder_forward_attn, the plain evaluation pass plus one launch).  In training mode, with a gradient required, with
``use_engine=False`` or with a per-layer mask attribute set, the encoder runs level by level ("levels": ``FragNet._levels``, the route
``return_attentions`` always took); both routes return the same tensors.

SHAPE CONTRACT.  Every attention tensor here is ``[n, num_heads]`` with a row for EVERY node of its level: atoms ``[N, H]``,
fragments ``[F, H]``, directed bonds ``[E, H]``, directed fragment connections ``[EF, H]``.  The reference's ``scatter_add`` is
called without ``dim_size`` and stops at ``source.max() + 1``, so its tensor can be shorter (trailing nodes without out-edges: the
last fragment of a batch whose last molecule has one fragment, trailing bonds that are no source in the bond graph); it is a PREFIX
of the tensor returned here, and the rows beyond it are exactly zero.
"""
from __future__ import annotations

import torch.nn as nn

from . import ops
from .model import FragNet, FragNetLayerA, FTHead1, FTHead2, FTHead3, FTHead4, PretrainTask, pooled
from .plan import LIVE_MOLS_KEY, plan_for


class FragNetViz(FragNet):
    """fragnet/vizualize/model.py:45-143.  ``forward(batch)`` returns the 8-tuple ``(x_atoms, x_frags, edge_features, fedge_features,
    attn_atoms, attn_frags, attn_bonds, attn_fbonds)``; the attention tensors follow the module's shape contract (a row per node)."""

    def __init__(self, num_layer, drop_ratio=0.2, emb_dim=128, atom_features=167, frag_features=167, edge_features=17, fedge_in=6,
                 fbond_edge_in=6, num_heads=4):
        nn.Module.__init__(self)
        self.variant = "gat2"
        self.num_layer = num_layer
        self.dropout = nn.Dropout(p=drop_ratio)
        self.act = nn.ReLU()
        self.layers = nn.ModuleList()
        self.rng = ops.PhiloxStream()
        self.use_engine = True      # False: always level by level (the A/B of the two routes)
        self.layers.append(FragNetLayerA(atom_in=atom_features, atom_out=emb_dim, frag_in=frag_features, frag_out=emb_dim,
                                         edge_in=edge_features, fedge_in=fedge_in, fbond_edge_in=fbond_edge_in, edge_out=emb_dim,
                                         num_heads=num_heads))
        for _ in range(num_layer - 2):
            self.layers.append(FragNetLayerA(atom_in=emb_dim, atom_out=emb_dim, frag_in=emb_dim, frag_out=emb_dim, edge_in=emb_dim,
                                             edge_out=emb_dim, fedge_in=emb_dim, fbond_edge_in=fbond_edge_in, num_heads=num_heads))
        self.layers.append(FragNetLayerA(atom_in=emb_dim, atom_out=emb_dim, frag_in=emb_dim, frag_out=emb_dim, edge_in=emb_dim,
                                         edge_out=emb_dim, fedge_in=emb_dim, fbond_edge_in=fbond_edge_in, num_heads=num_heads,
                                         return_attentions=True))

    def forward(self, batch):
        plan = plan_for(batch)
        if self.route(batch, attn=True) == "engine-attn":
            outs = self._engine(batch, plan, attn_readout=True)
            return outs[:4] + outs[5:]
        for layer in self.layers:
            layer.lite = False
        x, attn = self._levels(batch, plan)
        if attn is None:
            raise ValueError("FragNetViz: no layer has return_attentions set")
        return x + tuple(attn)


def _make_head(fthead, n_classes, h1, h2, h3, h4, drop_ratio, act):
    if fthead == "FTHead1":
        return FTHead1(n_classes=n_classes)
    if fthead == "FTHead2":
        return FTHead2(n_classes=n_classes)
    if fthead == "FTHead3":
        return FTHead3(n_classes=n_classes, h1=h1, h2=h2, h3=h3, h4=h4, drop_ratio=drop_ratio, act=act)
    if fthead == "FTHead4":
        return FTHead4(n_classes=n_classes, h1=h1, drop_ratio=drop_ratio, act=act)
    return None


class FragNetFineTuneViz(nn.Module):
    """fragnet/vizualize/model.py:146-201: ``forward(batch)`` returns ``(prediction, attn_atoms, attn_frags, attn_bonds,
    attn_fbonds)``, the attention tensors with a row per node (module docstring: the reference's are prefixes of them)."""

    def __init__(self, n_classes=1, atom_features=167, frag_features=167, edge_features=16, num_layer=4, num_heads=4, drop_ratio=0.15,
                 h1=256, h2=256, h3=256, h4=256, act="celu", emb_dim=128, fthead="FTHead3"):
        super().__init__()
        self.pretrain = FragNetViz(num_layer=num_layer, drop_ratio=drop_ratio, num_heads=num_heads, emb_dim=emb_dim,
                                   atom_features=atom_features, frag_features=frag_features, edge_features=edge_features)
        head = _make_head(fthead, n_classes, h1, h2, h3, h4, drop_ratio, act)
        if head is not None:         # (any other name: no head, as in the reference -- forward then fails)
            self.fthead = head
            self.fthead.rng = self.pretrain.rng

    @property
    def use_engine(self):
        return self.pretrain.use_engine

    @use_engine.setter
    def use_engine(self, value):
        self.pretrain.use_engine = bool(value)

    def forward(self, batch):
        x_atoms, x_frags, _, _, attn_atoms, attn_frags, attn_bonds, attn_fbonds = self.pretrain(batch)
        self.fthead.live_rows = batch.get(LIVE_MOLS_KEY)
        return self.fthead(pooled(x_atoms, x_frags, batch)), attn_atoms, attn_frags, attn_bonds, attn_fbonds


class FragNetFineTuneBaseViz(nn.Module):
    """fragnet/vizualize/model.py:205-250: the head is constructed (checkpoints load) and not applied; ``forward(batch)`` returns the
    readout ``cat(sum of atom rows, sum of fragment rows)`` [n_mols, 256]."""

    def __init__(self, n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=4, num_heads=4, drop_ratio=0.15,
                 h1=256, h2=256, h3=256, h4=256, act="celu", emb_dim=128, fthead="FTHead3"):
        super().__init__()
        self.pretrain = FragNetViz(num_layer=num_layer, drop_ratio=drop_ratio, num_heads=num_heads, emb_dim=emb_dim,
                                   atom_features=atom_features, frag_features=frag_features, edge_features=edge_features)
        head = _make_head(fthead, n_classes, h1, h2, h3, h4, drop_ratio, act)
        if head is not None:
            self.fthead = head
            self.fthead.rng = self.pretrain.rng

    use_engine = FragNetFineTuneViz.use_engine

    def forward(self, batch):
        outs = self.pretrain(batch)
        return pooled(outs[0], outs[1], batch)


class FragNetPreTrainViz(nn.Module):
    """fragnet/vizualize/model.py:256-280: ``forward(batch)`` returns ``(graph_rep, attn_atoms, attn_frags, attn_bonds,
    attn_fbonds)``, the attention tensors with a row per node."""

    def __init__(self, num_layer=4, drop_ratio=0.15, num_heads=4, emb_dim=128, atom_features=167, frag_features=167, edge_features=16):
        super().__init__()
        self.pretrain = FragNetViz(num_layer=num_layer, drop_ratio=drop_ratio, num_heads=num_heads, emb_dim=emb_dim,
                                   atom_features=atom_features, frag_features=frag_features, edge_features=edge_features)
        self.head = PretrainTask(128, 1)

    use_engine = FragNetFineTuneViz.use_engine

    def forward(self, batch):
        plan_for(batch, edge_ends=self.head.need_bond_length)
        x_atoms, x_frags, x_edge, _, attn_atoms, attn_frags, attn_bonds, attn_fbonds = self.pretrain(batch)
        graph_rep = self.head(x_atoms, x_frags, x_edge, batch)[3]
        return graph_rep, attn_atoms, attn_frags, attn_bonds, attn_fbonds
