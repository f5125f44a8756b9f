"""Drug-target affinity (DTA): the reference's second pair application of FragNet, on the MI355X path.

Counterpart of ``fragnet/model/dta/model.py`` (``DTAModel2``, the model its driver builds: ``from dta_model.model import DTAModel2 as
DTAModel``) and of the ``FragNetFineTuneBase`` class that ``fragnet/train/finetune/finetune_dta.py:64-105`` defines for it -- the same
class as the CDRP driver's, re-exported here.  Same module tree and attribute creation order, so a reference checkpoint loads with
``load_state_dict(strict=True)`` and the same ``torch.manual_seed`` gives the same initial parameters (tests/golden/dta_b5.npz pins
both).  Unlike the reference's module, importing this one does not touch the random generators.

On GPU tensors ``DTAModel2.forward`` is: encoder engine -> pooled [B, 256] read-out, protein tower (``ops.protein_tower``: the
convolution over the embedded tokens in its histogram form, then Linear(9376, 300)) and pair head (``ops.pair_head_dta``), all
hand-written HIP (csrc/dta.hip beside the encoder's kernels): no library convolution or GEMM, no embedding gather and no ``torch.cat``.
There is no CPU path, as everywhere in fragnet_amd.
"""
from __future__ import annotations

import torch.nn as nn

from . import ops
from .cdrp import FragNetFineTuneBase, pair_orderings_of  # noqa: F401  (finetune_dta.py:64-105 defines the same class)
from .data import PAIR_DRUG_KEY, PAIR_GRID_KEY, PAIR_SECOND_KEY


class DTAModel2(nn.Module):
    def __init__(self, drug_model):
        super().__init__()
        self.drug_model = drug_model
        self.fc1 = nn.Linear(256 + 300, 128)
        self.fc2 = nn.Linear(128, 1)

        num_features = 25
        prot_emb_dim = 300
        self.in_channels = 1000
        n_filters = 32
        kernel_size = 8
        prot_output_dim = 300

        self.embedding_xt = nn.Embedding(num_features + 1, prot_emb_dim)
        # holds the parameters only: the convolution runs inside ops.protein_tower
        self.conv_xt_1 = nn.Conv1d(in_channels=self.in_channels, out_channels=n_filters, kernel_size=kernel_size)
        intermediate_dim = prot_emb_dim - kernel_size + 1
        self.fc1_xt_dim = n_filters * intermediate_dim
        self.fc1_xt = nn.Linear(self.fc1_xt_dim, prot_output_dim)

    def forward(self, batch, loss=None):
        """``loss = (_lib.LOSS_MSE, y, None)``: the fused-loss call of a training step (``ops.pair_head_dta``); returns ``(out, loss)``,
        ``loss`` None where the fused launch does not apply.  ``(_lib.LOSS_MSE, y, None, real_rows)``: a batch staged to static shapes
        (graphstep.PairGraphedTrainStep), the mean over its first ``*real_rows`` rows.  A factored batch (``data.collate_fn_dta_factored``, ``data.as_factored``)
        runs the encoder on its U distinct drugs, the tower on its C distinct proteins and ``ops.pair_head_dta_factored``: [M, 1] in pair
        order.  A grid batch (``data.pair_grid_batch``) returns every drug against every protein, [U, C]."""
        drug_enc = self.drug_model(batch)
        tokens = batch["protein"].reshape(-1, self.in_channels)
        xt = ops.protein_tower(tokens, self.embedding_xt, self.conv_xt_1, self.fc1_xt)
        if batch.get(PAIR_GRID_KEY):
            return ops.pair_head_dta_grid(drug_enc, xt, self.fc1, self.fc2)
        if PAIR_DRUG_KEY in batch:
            return ops.pair_head_dta_factored(drug_enc, xt, batch[PAIR_DRUG_KEY], batch[PAIR_SECOND_KEY], self.fc1, self.fc2, loss=loss,
                                              orderings=pair_orderings_of(batch), check=False)
        return ops.pair_head_dta(drug_enc, xt, self.fc1, self.fc2, loss=loss)


class DTAModel(nn.Module):
    """The reference's transformer-tower variant (8 encoder layers over the 1000 positions), which its driver does not use."""

    def __init__(self, drug_model=None):
        raise NotImplementedError("DTAModel (the transformer protein tower) is outside the FragNet gat2 hot path; the reference's "
                                  "driver builds DTAModel2")
