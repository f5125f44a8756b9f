"""FragNet's graph-convolution baseline (model_version gcn2) on the MI355X kernels.

Module API, constructor signatures, parameter names and construction order (= RNG order = state-dict order) are the reference's
fragnet/model/gcn/gcn2.py, so the same seed gives the same weights and reference checkpoints load with ``strict=True``:
  FragNetLayer     gcn2.py:11-71
  FragNet          gcn2.py:76-130
  FragNetFineTune  gcn2.py:159-194

``forward`` is not the reference's op list.  A layer is
  h        = atom_embed(x_atoms)                                       ops.linear128 (model._project)
  x_atoms' = D^-1/2 (A + I) D^-1/2 h                                    ops.gcn_aggregate on the plan's atom level (loop items), coef = deg^-1/2
  x_frags  = scatter_add(x_atoms', atom_to_frag_ids)                   ops.segment_sum
  x_frags' = frag_mlp(sum over the fragment graph's in-edges)          ops.gcn_aggregate without coefficients, ops.frag_mlp
and relu(dropout(.)) between layers rides in the aggregate's launch.  What the reference computes and never reads is not computed:
``edge_embed(edge_attr)`` (gcn2.py:46), and the fragment half of every layer but the last (gcn2.py:59 overwrites the incoming ``x_frags``,
so only the last layer's is ever read).  The parameters the reference constructs and never calls (``frag_embed``, ``edge_embed``,
``frag_message_mlp``, ``atom_mlp``, ``batch_norms``, the top-level ``lin1``) are constructed too and stay without gradient, exactly as
there.  Dropout masks are this project's Philox stream, not torch's.  GPU tensors only: there is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .model import FTHead3, FTHead4, _project, _two_layer
from .plan import LIVE_MOLS_KEY, GraphPlan, gcn_plan_for

_LAYER_PLANS = {}      # tiny cache for direct layer calls: index-tensor identity -> (GraphPlan, coefficient table)


def _plan_from_indices(N, F_, edge_index, frag_index, a2f):
    key = tuple((t.data_ptr(), tuple(t.shape), t._version) for t in (edge_index, frag_index, a2f))
    hit = _LAYER_PLANS.get(key)
    if hit is None:
        if len(_LAYER_PLANS) >= 4:
            _LAYER_PLANS.clear()
        plan = GraphPlan([
            dict(kind="gat", name="atom", dst=edge_index[1], src=edge_index[0], n=N, n_loops=N),
            dict(kind="gat", name="frag", dst=frag_index[1], src=frag_index[0], n=F_, n_loops=0),
            dict(kind="seg", name="a2f", key=a2f, n_seg=F_),
        ], edge_index.device)
        hit = _LAYER_PLANS[key] = plan
    return hit


def _coef(plan):
    """deg^-1/2 of the plan's atom level, once per plan (the same table for every layer and both directions)"""
    coef = getattr(plan, "gcn_coef", None)
    if coef is None:
        coef = plan.gcn_coef = ops.gcn_coef(plan.levels["atom"])
    return coef


class FragNetLayer(nn.Module):
    def __init__(self, atom_in=128, atom_out=128, frag_in=128, frag_out=128, edge_in=128, edge_out=128):
        super().__init__()
        if atom_out != 128:
            raise ValueError("the gfx950 kernels are specialised for emb_dim = 128 (every reference config)")
        self.atom_embed = nn.Linear(atom_in, atom_out, bias=True)
        # constructed-but-unused block (kept for RNG order and checkpoint compatibility)
        self.frag_embed = nn.Linear(frag_in, frag_out)
        self.edge_embed = nn.Linear(edge_in, edge_out)
        self.frag_message_mlp = nn.Linear(atom_out * 2, atom_out)
        self.atom_mlp = _two_layer(atom_out)
        # live again
        self.frag_mlp = _two_layer(atom_out)

    def forward(self, x_atoms, edge_index, edge_attr, frag_index, x_frags, atom_to_frag_ids):
        """The reference's 6-argument layer signature (gcn2.py:31-36): the raw rows of both halves.  ``edge_attr`` and ``x_frags`` are
        accepted and ignored, as they are never read there (gcn2.py:46, 59)."""
        plan = _plan_from_indices(x_atoms.shape[0], x_frags.shape[0], edge_index, frag_index, atom_to_frag_ids)
        atoms_new = self.atoms(x_atoms, plan)
        return atoms_new, self.frags(atoms_new, plan)

    def atoms(self, x_atoms, plan, act=None, raw=None):
        """gcn2.py:45-58: the normalised neighbour sum of the projected atoms; ``act`` / ``raw`` as ``ops.gcn_aggregate``"""
        return ops.gcn_aggregate(_project(x_atoms, self.atom_embed), plan.levels["atom"], _coef(plan), act=act, raw=raw)

    def frags(self, atoms_new, plan):
        """gcn2.py:59-68 from the raw atom rows: atom -> fragment sum, plain sum over the fragment graph, ``frag_mlp``"""
        x_frags = ops.segment_sum(atoms_new, plan.segs["a2f"], plan)
        return ops.frag_mlp(ops.gcn_aggregate(x_frags, plan.levels["frag"]), self.frag_mlp[0], self.frag_mlp[2])


class FragNet(nn.Module):
    def __init__(self, num_layer, drop_ratio=0, emb_dim=128, atom_features=45, frag_features=45, edge_features=12):
        super().__init__()
        self.num_layer = num_layer
        self.dropout = nn.Dropout(p=drop_ratio)
        self.act = nn.ReLU()
        self.layers = nn.ModuleList()
        self.layers.append(FragNetLayer(atom_in=atom_features, atom_out=emb_dim, frag_in=frag_features, frag_out=emb_dim,
                                        edge_in=edge_features, edge_out=emb_dim))
        for _ in range(num_layer - 1):
            self.layers.append(FragNetLayer(atom_in=emb_dim, atom_out=emb_dim, frag_in=emb_dim, frag_out=emb_dim,
                                            edge_in=edge_features, edge_out=emb_dim))
        self.batch_norms = nn.ModuleList()      # constructed, never called (gcn2.py:95-97)
        for _ in range(num_layer):
            self.batch_norms.append(nn.BatchNorm1d(emb_dim))
        self.rng = ops.PhiloxStream()

    def forward(self, batch):
        plan = gcn_plan_for(batch)
        p, train = self.dropout.p, self.training
        x_atoms = ops.dropout_act(batch["x_atoms"], p, train, False, self.rng)
        # batch["x_frags"] is dead in the reference too: every layer overwrites it with the atom -> fragment sum before first use
        # (gcn2.py:59); so is the fragment half of every layer but the last, whose result the next layer overwrites the same way
        for layer in self.layers[:-1]:
            x_atoms = layer.atoms(x_atoms, plan, act=(p, train, True, self.rng))
        last = self.layers[-1]
        raw, x_atoms = last.atoms(x_atoms, plan, act=(p, train, True, self.rng), raw=True)
        x_frags = ops.dropout_act(last.frags(raw, plan), p, train, True, self.rng)
        return x_atoms, x_frags


class FragNetFineTune(nn.Module):
    def __init__(self, n_classes=1, atom_features=167, frag_features=167, edge_features=16, num_layer=4, drop_ratio=.15,
                 emb_dim=128, h1=256, h2=256, h3=256, h4=256, act="celu", fthead="FTHead3"):
        super().__init__()
        self.pretrain = FragNet(num_layer=num_layer, drop_ratio=drop_ratio, emb_dim=emb_dim, atom_features=atom_features,
                                frag_features=frag_features, edge_features=edge_features)
        self.lin1 = nn.Linear(emb_dim * 2, emb_dim * 2)      # constructed, never called (gcn2.py:169)
        self.dropout = nn.Dropout(p=0.15)
        self.activation = nn.ReLU()
        if fthead == "FTHead3":
            self.fthead = FTHead3(n_classes=n_classes, h1=h1, h2=h2, h3=h3, h4=h4, drop_ratio=drop_ratio, act=act)
        elif fthead == "FTHead4":
            self.fthead = FTHead4(n_classes=n_classes, h1=h1, drop_ratio=drop_ratio, act=act)
        else:
            raise ValueError(f"fthead {fthead!r}: gcn2 builds FTHead3 or FTHead4 (gcn2.py:173-180)")
        self.fthead.rng = self.pretrain.rng

    def forward(self, batch):
        x_atoms, x_frags = self.pretrain(batch)
        self.fthead.live_rows = batch.get(LIVE_MOLS_KEY)
        return self.fthead(ops.pool_cat(x_atoms, x_frags, gcn_plan_for(batch)))
