#!/usr/bin/env python3
"""Generates tests/golden/frag_shapley.npz with the REFERENCE's own fragment-contribution models (fragnet/vizualize/model_attr.py, run with
``apply_mask=True``) on one record per COALITION of fragments (needs the reference checkout that make_golden.py names; run where that
exists):
    python tests/golden/make_golden_fragshap.py

The set function: v(S) = the reference's prediction of the record whose ``atom_mask`` is 1 on the atoms of every group OUTSIDE S (the
reference zeroes those atom rows behind its encoder; the fragment rows stay).  Every coalition of every molecule is evaluated: 2^F records
per molecule, all records of a case collated into batches by model_attr's own collate.  The cases are three of make_golden_fragattr.py's --
the same models, seeds, molecules and groups, with that generator's stubs, ``with_mask`` and ``groups_of``; its ``pair`` is a local function
of its ``main`` and is repeated here:
    property          28 groups (F = 6, 4, 4, 8, 2, 4): 372 rows
    property_groups   atom index % 3, atoms with index % 7 == 0 in no group (they are in every coalition): 6 x 8 = 48 rows
    energy            model_attr.FragNetPreTrain, its 4th output: 372 rows

The file holds numbers and a JSON of constructor arguments only:
    cfg                     json: per case ctor, seed, scaling, fragments per molecule
    <case>/mask             int64 [rows, 2]: (molecule, mask), molecule-major, masks ascending; bit k = the molecule's k-th group id
    <case>/value            [rows, C] fp32
    <case>/phi              float64 [R, C]: the Shapley values of those values, by the definition (every order of the groups)
"""
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_fragattr as mgf  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import attr_common as ac  # noqa: E402

NAME = "frag_shapley"
CASES = ("property", "property_groups", "energy")
# share of (molecule, group) entries whose |phi| exceeds 10 x the attribution tolerance, asserted on these reference values
MIN_SHARE = {"property": 0.75, "property_groups": 0.75, "energy": 0.5}
RECORDS_PER_BATCH = 64


def shapley_by_orders(values, F):
    """phi [F, C] in float64 from v [2^F, C] (row index = mask) by the definition: the mean marginal over all F! orders."""
    v = np.asarray(values, dtype=np.float64)
    phi = np.zeros((F, v.shape[1]), dtype=np.float64)
    count = 0
    for order in itertools.permutations(range(F)):
        m = 0
        for f in order:
            phi[f] += v[m | (1 << f)] - v[m]
            m |= 1 << f
        count += 1
    return phi / count


def coalition_records(case, mols):
    """(records, int64 [rows, 2] (molecule, mask)): per molecule every mask 0 .. 2^F - 1; atom_mask = 1 on the groups outside the mask."""
    recs, table = [], []
    for i, m in enumerate(mols):
        g = mgf.groups_of(case, m)
        ids = np.unique(g[g >= 0]).tolist()
        for mask in range(1 << len(ids)):
            out = [gid for k, gid in enumerate(ids) if not (mask >> k) & 1]
            recs.append(mgf.with_mask(m, np.nonzero(np.isin(g, out))[0]))
            table.append((i, mask))
    return recs, np.asarray(table, dtype=np.int64).reshape(-1, 2)


def main():
    mgf.install_stubs()
    with mg.quiet():
        from fragnet.vizualize import model_attr as ref_attr
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)

    def masked_model(make, seed, scaled):
        """make_golden_fragattr.py's ``pair``, the apply_mask=True half."""
        torch.manual_seed(seed)
        with mg.quiet():
            masked = make(True)
        mg.zero_dead_bias(masked)
        if scaled:
            ac.scale_model(masked)
        return masked.eval()

    ft_ctor = dict(atom_features=167, frag_features=167, edge_features=17, emb_dim=128, **ac.CTOR)
    cases = {
        "property": dict(seed=ac.SEED, scaled=True, ctor=ft_ctor, make=lambda m: ref_attr.FragNetFineTune(**ft_ctor, apply_mask=m)),
        "property_groups": dict(seed=ac.SEED, scaled=True, ctor=ft_ctor, make=lambda m: ref_attr.FragNetFineTune(**ft_ctor, apply_mask=m)),
        "energy": dict(seed=5, scaled=False, ctor=mgf.ENERGY_CTOR, output=3,
                       make=lambda m: ref_attr.FragNetPreTrain(**mgf.ENERGY_CTOR, apply_mask=m)),
    }
    cfg = {"head_scale": ac.HEAD_SCALE, "att_scale": ac.ATT_SCALE, "mol_seed": ac.MOL_SEED, "profile": "esol", "cases": {}}
    store = {}
    for name in CASES:
        c = cases[name]
        mols = ac.molecules()
        recs, table = coalition_records(name, mols)
        model = masked_model(c["make"], c["seed"], c["scaled"])
        pick = (lambda o: o[c["output"]]) if "output" in c else (lambda o: o)
        parts = []
        with torch.no_grad(), mg.quiet():
            for lo in range(0, len(recs), RECORDS_PER_BATCH):
                chunk = recs[lo: lo + RECORDS_PER_BATCH]
                parts.append(pick(model(ref_attr.collate_fn(chunk))).reshape(len(chunk), -1).numpy().astype(np.float32))
        value = np.concatenate(parts, 0)
        groups = [int(np.log2((table[:, 0] == i).sum())) for i in range(len(mols))]
        phi, big, worst = [], [], 0.0
        for i, F in enumerate(groups):
            v = value[table[:, 0] == i]
            p = shapley_by_orders(v, F)
            worst = max(worst, float(np.abs(p.sum(0) - (v[-1].astype(np.float64) - v[0])).max()))
            phi.append(p)
            big.append((np.abs(p) > 10 * ac.attr_tolerance(v[-1].astype(np.float64))).all(axis=1))
        phi, big = np.concatenate(phi, 0), np.concatenate(big)
        store[f"{name}/mask"], store[f"{name}/value"], store[f"{name}/phi"] = table, value, phi
        cfg["cases"][name] = {"ctor": c["ctor"], "seed": c["seed"], "scaled": c["scaled"], "n_mols": len(mols), "groups": groups}
        print(f"{name}: {len(mols)} molecules, groups {groups}, {len(recs)} rows, {int(big.sum())}/{len(big)} Shapley values above 10 x tolerance, "
              f"efficiency gap {worst:.1e}")
        assert big.mean() >= MIN_SHARE[name], name
    store["cfg"] = np.asarray(json.dumps(cfg))
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **store)
    print(f"{NAME}.npz: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
