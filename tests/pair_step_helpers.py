"""What the captured-pair-step tests share (tests/test_pair_graphstep_host.py, tests/test_gpu_pair_graphstep.py): synthetic CDRP / DTA
records and batches -- the few lines of ``_records`` / ``_batch`` of tests/test_gpu_cdrp.py and tests/test_gpu_dta.py, with the device
as an argument -- and the small models of the step-level tests.  Test infrastructure only."""
import torch

GENE_DIM = 903
KINDS = ("cdrp", "dta")
SECOND = {"cdrp": "gene_expr", "dta": "protein"}
SMALL = dict(n_classes=1, num_layer=2, num_heads=4, drop_ratio=0.0, h1=32, h2=64, h3=64, h4=32, act="relu", fthead="FTHead3")


def records(kind, n, seed):
    from fragnet_amd import synth
    mols = synth.synth_molecules(n, seed=seed, profile="esol")
    return synth.attach_gene_expr(mols, GENE_DIM, seed + 1) if kind == "cdrp" else synth.attach_protein(mols, seed + 1)


def batch(kind, n, seed, device=None):
    from fragnet_amd import data
    b = (data.collate_fn_cdrp if kind == "cdrp" else data.collate_fn_dta)(records(kind, n, seed))
    return b if device is None else data.batch_to(b, device)


def model(kind, device, seed=0, drop=0.0):
    from fragnet_amd.cdrp import CDRPModel, FragNetFineTuneBase
    from fragnet_amd.dta import DTAModel2
    torch.manual_seed(seed)
    base = FragNetFineTuneBase(**dict(SMALL, drop_ratio=drop))
    m = CDRPModel(base, GENE_DIM, device) if kind == "cdrp" else DTAModel2(base)
    return m.to(device).train()


class Loader(list):
    """pre-collated batches with the ``dataset`` attribute the trainers normalise by"""
    dataset = ()
