"""The reference's fragment-contribution models (fragnet/vizualize/model_attr.py) on the MI355X kernels:

  FragNetFineTune         :143-208   the finetune model; ``apply_mask=True`` zeroes the rows ``atom_mask == 1`` of the encoder's final x_atoms
  FragNetFineTuneBaseViz  :212-263   the drug encoder of a CDRP / DTA model with the same mask, returning the pooled read-out
  FragNetPreTrain         :269-295   the pretrain model with the same mask; all four outputs come from the masked rows
  collate_fn, collate_fn_cdrp  :302-462   the finetune / CDRP batch plus ``atom_mask`` int32 [N] from each record's ``atom_mask``

Constructor signatures (``apply_mask=False, mask_all_layers=False`` included), construction order (= RNG order) and state-dict keys are
the reference's, so its checkpoints load with ``strict=True``.  The mask sits behind the encoder: the masked rows are replaced out of
place just before ``pooled()``; nothing inside the encoder sees it.

This is the literal path: one encoder pass per replica, as ``get_attr_image`` runs it on the records ``create_data`` copies per
fragment.  ``attribution.fragment_contributions`` computes the same numbers with one encoder pass per molecule.

``mask_all_layers=True`` is not implemented: the reference zeroes the rows between the layers but not inside them
(model_attr.py:116-117, 133-134), which is neither the engine's row masks (zero in every layer, inside included) nor anything
``get_attr_image`` sets.
"""
from __future__ import annotations

import torch

from . import cdrp, data, model
from .model import pooled


def _refuse_mask_all_layers(mask_all_layers):
    if mask_all_layers:
        raise NotImplementedError("mask_all_layers=True (model_attr.py:116-117, 133-134: rows zeroed between the layers, not inside them) "
                                  "is not implemented; get_attr_image never sets it")


def _masked(x_atoms, batch):
    """``x_atoms[atom_mask == 1] = 0.0`` (model_attr.py:189-191), out of place."""
    mask = batch["atom_mask"]
    if mask.shape != (x_atoms.shape[0],):
        raise ValueError(f"atom_mask must hold one entry per atom ([{x_atoms.shape[0]}]), got {tuple(mask.shape)}")
    return x_atoms.masked_fill((mask == 1).unsqueeze(1), 0.0)


class FragNetFineTune(model.FragNetFineTune):
    def __init__(self, n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=4, num_heads=4, drop_ratio=0.15,
                 h1=256, h2=256, h3=256, h4=256, act="celu", emb_dim=128, fthead="FTHead3", apply_mask=False, mask_all_layers=False,
                 variant="gat2"):
        """``variant``: this project's model_version switch, as on ``model.FragNetFineTune`` (the mask sits behind the encoder, so it
        holds for gat2_lite and gat2_edge too)."""
        _refuse_mask_all_layers(mask_all_layers)
        super().__init__(n_classes=n_classes, atom_features=atom_features, frag_features=frag_features, edge_features=edge_features,
                         num_layer=num_layer, num_heads=num_heads, drop_ratio=drop_ratio, h1=h1, h2=h2, h3=h3, h4=h4, act=act,
                         emb_dim=emb_dim, fthead=fthead, variant=variant)
        self.apply_mask = apply_mask

    def forward(self, batch):
        if not self.apply_mask:
            return super().forward(batch)
        x_atoms, x_frags, _, _ = self.pretrain(batch, edge_outputs=False)
        self.fthead.live_rows = None
        return self.fthead(pooled(_masked(x_atoms, batch), x_frags, batch))


class FragNetFineTuneBaseViz(cdrp.FragNetFineTuneBase):
    def __init__(self, n_classes=1, atom_features=167, frag_features=167, edge_features=17, num_layer=4, num_heads=4, drop_ratio=0.15,
                 h1=256, h2=256, h3=256, h4=256, act="celu", emb_dim=128, fthead="FTHead3", apply_mask=False, mask_all_layers=False):
        _refuse_mask_all_layers(mask_all_layers)
        super().__init__(n_classes=n_classes, atom_features=atom_features, frag_features=frag_features, edge_features=edge_features,
                         num_layer=num_layer, num_heads=num_heads, drop_ratio=drop_ratio, h1=h1, h2=h2, h3=h3, h4=h4, act=act,
                         emb_dim=emb_dim, fthead=fthead)
        self.apply_mask = apply_mask

    def forward(self, batch):
        if not self.apply_mask:
            return super().forward(batch)
        x_atoms, x_frags, _, _ = self.pretrain(batch, edge_outputs=False)
        return pooled(_masked(x_atoms, batch), x_frags, batch)


class FragNetPreTrain(model.FragNetPreTrain):
    def __init__(self, num_layer=4, drop_ratio=0.15, num_heads=4, emb_dim=128, atom_features=167, frag_features=167, edge_features=16,
                 apply_mask=False):
        super().__init__(num_layer=num_layer, drop_ratio=drop_ratio, num_heads=num_heads, emb_dim=emb_dim, atom_features=atom_features,
                         frag_features=frag_features, edge_features=edge_features)
        self.apply_mask = apply_mask

    def forward(self, batch):
        if not self.apply_mask:
            return super().forward(batch)
        from .plan import plan_for
        plan_for(batch, edge_ends=self.head.need_bond_length)
        x_atoms, x_frags, e_edge, _ = self.pretrain(batch)
        return self.head(_masked(x_atoms, batch), x_frags, e_edge, batch)


def _atom_mask(data_list):
    return torch.cat([d.atom_mask for d in data_list], dim=0).type(torch.int)


def collate_fn(data_list):
    """``data.collate_fn`` plus ``atom_mask`` int32 [N] (model_attr.py:302-380)."""
    out = data.collate_fn(data_list)
    out["atom_mask"] = _atom_mask(data_list)
    return out


def collate_fn_cdrp(data_list):
    """``data.collate_fn_cdrp`` plus ``atom_mask`` int32 [N] (model_attr.py:383-462)."""
    out = data.collate_fn_cdrp(data_list)
    out["atom_mask"] = _atom_mask(data_list)
    return out
