"""CPU-side checks of the cancer-drug-response (CDRP) surface: collate_fn_cdrp against the reference's batch, CDRPModel's module tree
and initialisation against the reference's (tests/golden/cdrp_b5.npz, written by tests/golden/make_golden_cdrp.py), the ``fragnet.*``
import paths of the reference's finetune_cdrp.py, the trainer's keyword set, and the fixture's size."""
import inspect
import os
import sys

import pytest
import torch

from tests.conftest import GOLDEN, ROOT
from tests.helpers import check_params_match, load_case

CASE = "cdrp_b5"


def _records(cfg):
    from fragnet_amd import synth
    mols = synth.synth_molecules(5, seed=cfg["mol_seed"], profile="esol")
    return synth.attach_gene_expr(mols, cfg["gene_dim"], cfg["gene_seed"], cfg["pinned"])


def test_collate_fn_cdrp_reproduces_the_reference_batch():
    from fragnet_amd import data
    cfg, want, _, _, _, _ = load_case(CASE)
    mols = _records(cfg)
    got = data.collate_fn_cdrp(mols)
    assert tuple(got.keys()) == data.BATCH_KEYS_CDRP and set(want) == set(data.BATCH_KEYS_CDRP)
    for k in data.BATCH_KEYS_CDRP:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k           # integer tensors bit-exact; the float ones are copies of the same records
    ge = got["gene_expr"]
    assert ge.dtype == torch.int64 and ge.shape == (5, cfg["gene_dim"]) and cfg["gene_dim"] % 4 == 3
    # the hand-placed -0.7, 2.9, -1.5: .type(torch.long) truncates toward zero
    assert mols[0].gene_expr[:3].tolist() == pytest.approx([-0.7, 2.9, -1.5])
    assert ge[0, :3].tolist() == [0, 2, -1]
    assert torch.equal(ge, torch.stack([m.gene_expr for m in mols]).type(torch.long))
    assert int(ge.min()) < 0 < int(ge.max()) and bool((ge == 0).any())


def test_cdrp_model_matches_reference_module_tree_and_init():
    from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase, MLP
    cfg, _, _, _, pkeys, psums = load_case(CASE)
    torch.manual_seed(cfg["seed"])
    model = CDRPModel(FragNetFineTuneBase(**cfg["ctor"]), cfg["gene_dim"], "cpu")
    assert list(model._modules) == ["drug_model", "fc1", "fc2", "cell_model"]
    assert isinstance(model.cell_model, MLP) and [tuple(l.weight.shape) for l in model.cell_model.predictor] == \
        [(1024, cfg["gene_dim"]), (256, 1024), (64, 256), (256, 64)]
    check_params_match(model, pkeys, psums)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    torch.manual_seed(cfg["seed"] + 1)
    other = CDRPModel(FragNetFineTuneBase(**cfg["ctor"]), cfg["gene_dim"], "cpu")
    other.load_state_dict(sd, strict=True)
    check_params_match(other, pkeys, psums)
    # the reference's constructor signature (finetune_cdrp.py:65-67)
    names = list(inspect.signature(FragNetFineTuneBase.__init__).parameters)[1:]
    assert names == ["n_classes", "atom_features", "frag_features", "edge_features", "num_layer", "num_heads", "drop_ratio", "h1", "h2", "h3",
                     "h4", "act", "emb_dim", "fthead"]


@pytest.fixture
def _this_repo_first():
    sys.path.insert(0, ROOT)
    for k in [k for k in sys.modules if k == "fragnet" or k.startswith("fragnet.")]:
        del sys.modules[k]
    yield
    sys.path.remove(ROOT)


def test_cdrp_driver_imports_resolve_to_fragnet_amd(_this_repo_first):
    import fragnet_amd.cdrp
    import fragnet_amd.data
    import fragnet_amd.train
    from fragnet.model.cdrp.model import CDRPModel, MLP
    from fragnet.dataset.data import collate_fn_cdrp
    from fragnet.train.finetune.trainer_cdrp import TrainerFineTune
    assert CDRPModel is fragnet_amd.cdrp.CDRPModel and MLP is fragnet_amd.cdrp.MLP
    assert collate_fn_cdrp is fragnet_amd.data.collate_fn_cdrp
    assert TrainerFineTune is fragnet_amd.train.TrainerFineTuneCDRP
    trainer = TrainerFineTune(target_pos=None, target_type="regr", n_multi_task_heads=0)
    # the keyword set of the reference's driver (finetune_cdrp.py: trainer.train / validate / test)
    for fn, kws in ((trainer.train, ("model", "loader", "optimizer", "scheduler", "device", "val_loader", "label_mean", "label_sdev")),
                    (trainer.validate, ("model", "loader", "device", "label_mean", "label_sdev")),
                    (trainer.test, ("model", "loader", "device", "label_mean", "label_sdev"))):
        params = inspect.signature(fn).parameters
        assert all(k in params for k in kws), fn
    for kind in ("clsf", "clsf_ms"):
        with pytest.raises(NotImplementedError, match="outside the FragNet gat2 hot path"):
            TrainerFineTune(target_type=kind)


def test_cdrp_model_refuses_cpu_tensors():
    from fragnet_amd import _lib
    from fragnet_amd.cdrp import MLP
    with pytest.raises(_lib.FragnetHipError):
        MLP(7, "cpu")(torch.zeros((2, 7), dtype=torch.int64))


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, CASE + ".npz")) < (1 << 20)
