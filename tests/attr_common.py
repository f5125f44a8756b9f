"""Shared by the attribution tests and tests/golden/make_golden_attr.py: the model of the issue's checks, its scaled form, and the
leave-one-out loop over any FragNetFineTune-shaped model that takes the reference's per-layer scalar mask attributes (the oracle,
the reference itself), one molecule and one mask at a time as fragnet/vizualize/viz.py does."""
import numpy as np
import torch

CTOR = dict(n_classes=1, num_layer=2, num_heads=4, drop_ratio=0.0, h1=64, h2=128, h3=128, h4=64, act="relu", fthead="FTHead3")
SEED, MOL_SEED, N_MOLS = 5, 4100, 6
HEAD_SCALE, ATT_SCALE = 100.0, 4.0
ATOL = RTOL = 1e-4                       # the project's logit / encoder-output tolerance
MASK_ATTR = {"atom": "atom_mask_individual", "bond": "bond_mask", "fbond": "frag_bond_mask"}


def molecules(n=N_MOLS, seed=MOL_SEED, profile="esol"):
    from fragnet_amd import synth
    return synth.synth_molecules(n, seed=seed, profile=profile)


def build(module, ctor=CTOR, seed=SEED, scaled=False):
    """``module.FragNetFineTune(**ctor)`` under ``seed``; ``scaled``: last Linear x HEAD_SCALE, the four attention vectors x ATT_SCALE."""
    torch.manual_seed(seed)
    model = module.FragNetFineTune(**ctor)
    if scaled:
        scale_model(model)
    model.eval()
    return model


def last_linear(model):
    lins = [m for m in model.fthead.modules() if isinstance(m, torch.nn.Linear)]
    return lins[-1]


def scale_model(model):
    with torch.no_grad():
        lin = last_linear(model)
        lin.weight.mul_(HEAD_SCALE)
        lin.bias.mul_(HEAD_SCALE)
        for layer in model.pretrain.layers:
            for name in ("a_b", "a", "f", "f_a_b"):
                getattr(layer, name).mul_(ATT_SCALE)


def replicas_of(n_atoms, n_bonds, n_fbonds):
    """viz.py's loops: (kind, value of the layer attribute, reported index)."""
    return ([("atom", i, i) for i in range(n_atoms)] + [("bond", i, i) for i in range(0, n_bonds, 2)]
            + [("fbond", k, k) for k in range(n_fbonds // 2)])


def set_mask(model, kind, value):
    for layer in model.pretrain.layers:
        setattr(layer, MASK_ATTR[kind], value)


def scalar_loo(model, mols, collate, run=None):
    """Per molecule ``{"pred_no_mask": [C], kind: {"index", "pred_mask" [count, C]}}`` with one forward per masked element."""
    run = run or (lambda m, b: m(b))
    out = []
    for mol in mols:
        b = collate([mol])
        with torch.no_grad():
            base = run(model, b).reshape(-1).clone()
        rec = {"pred_no_mask": base.numpy().copy()}
        C = base.numel()
        reps = replicas_of(b["x_atoms"].shape[0], b["node_features_bonds"].shape[0], b["node_features_fbonds"].shape[0])
        for kind in MASK_ATTR:
            idx, preds = [], []
            for k, value, index in reps:
                if k != kind:
                    continue
                set_mask(model, kind, value)
                try:
                    with torch.no_grad():
                        preds.append(run(model, b).reshape(-1).numpy().copy())
                finally:
                    set_mask(model, kind, None)
                idx.append(index)
            rec[kind] = {"index": np.asarray(idx, dtype=np.int32), "pred_mask": np.asarray(preds, dtype=np.float32).reshape(len(idx), C)}
        out.append(rec)
    return out


def attr_tolerance(pred_no_mask):
    """Each prediction is held to ATOL + RTOL |.|, so a difference of two to twice that."""
    return 2.0 * (ATOL + RTOL * np.abs(pred_no_mask))
