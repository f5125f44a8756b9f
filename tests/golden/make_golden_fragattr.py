#!/usr/bin/env python3
"""Generates tests/golden/frag_attr.npz with the REFERENCE's own fragment-contribution models: fragnet/vizualize/model_attr.py's
``FragNetFineTune``, ``FragNetFineTuneBaseViz`` (under the reference's ``CDRPModel`` and ``DTAModel2``) and ``FragNetPreTrain``, run
unmasked and with ``apply_mask=True`` on the replicated records, as ``get_attr_image`` runs them (needs the reference checkout that
make_golden.py names; run where that exists):
    python tests/golden/make_golden_fragattr.py

model_attr.py imports IPython, omegaconf, rdkit.Chem.Draw and more at module level; besides make_golden.py's stand-ins this generator
installs a meta-path finder that answers any IPython / omegaconf / rdkit / streamlit / torch_geometric / lmdb submodule that is not in
``sys.modules`` yet with an import-only mock package.  The dead per-layer ``bias`` is zeroed as in the other generators.

Replicas are built as ``create_data`` builds them (model_attr.py:734-761): one copy of the record per group with ``atom_mask[atoms of the
group] = 1`` (a shallow copy: only ``atom_mask`` differs), all replicas of a case collated into ONE batch by model_attr's own collate.
The groups are the fragments (``atom_id_frag_id``) except in ``property_groups``.

Cases (molecules from fragnet_amd.synth; built in main()):
    property          the scaled model of tests/attr_common.py (CTOR, seed 5) on synth_molecules(6, seed=4100, "esol"): 28 replicas
    property_groups   the same model and molecules, groups[i] = atom index % 3, atoms with index % 7 == 0 in no group: 18 replicas
    energy            model_attr.FragNetPreTrain(num_layer=2, drop_ratio=0, num_heads=4, edge_features=17), seed 5, unscaled; 4th output
    drp               CDRPModel(model_attr.FragNetFineTuneBaseViz(**make_golden_cdrp.CTOR), 903, "cpu"), seed 7, that generator's molecules
                      and gene rows: 12 replicas
    dta               DTAModel2 over the same class with make_golden_dta's CTOR / seeds / proteins; ``protein`` is added to model_attr.collate_fn's
                      batch exactly as the reference's collate_fn_dta builds it: 11 replicas, three molecules with a single fragment

The file holds numbers and a JSON of constructor arguments only:
    cfg                          json: per case ctor, seeds, scalings, molecule recipe
    <case>/pkeys, <case>/psums   state-dict keys and (sum, abs-sum) checksums
    <case>/pred_no_mask          [B, C]
    <case>/replica               int64 [R, 2]: (molecule, group)
    <case>/pred_mask             [R, C]
"""
import copy
import importlib.abc
import importlib.machinery
import json
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_cdrp as mgc  # noqa: E402
import make_golden_dta as mgd  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import attr_common as ac  # noqa: E402

NAME = "frag_attr"
MOCKED_ROOTS = ("IPython", "omegaconf", "rdkit", "streamlit", "torch_geometric", "lmdb")
ENERGY_CTOR = dict(num_layer=2, drop_ratio=0.0, num_heads=4, edge_features=17)
# share of replicas whose |pred_no_mask - pred_mask| exceeds 10 x the attribution tolerance, asserted on these reference values
MIN_SHARE = {"property": 0.75, "property_groups": 0.75, "energy": 0.5, "drp": 0.75, "dta": 0.75}


class _MockFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Any submodule of MOCKED_ROOTS that nothing has installed: an import-only MagicMock package."""

    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in MOCKED_ROOTS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        m = mock.MagicMock(name=spec.name)
        m.__path__, m.__name__, m.__spec__, m.__loader__ = [], spec.name, spec, self
        return m

    def exec_module(self, module):
        pass


def install_stubs():
    mg.install_stubs()
    for name, m in list(sys.modules.items()):          # make_golden's mocks are plain modules: as packages their submodules resolve
        if name.split(".")[0] in MOCKED_ROOTS and isinstance(m, mock.MagicMock):
            m.__path__ = []
    sys.meta_path.insert(0, _MockFinder())


def groups_of(case, mol):
    n = int(mol.x_atoms.shape[0])
    if case == "property_groups":
        g = np.arange(n) % 3
        g[np.arange(n) % 7 == 0] = -1
        return g.astype(np.int64)
    return mol.atom_id_frag_id.numpy().astype(np.int64)


def with_mask(mol, atoms):
    rec = copy.copy(mol)                       # shallow: every tensor shared, atom_mask its own
    mask = torch.zeros(mol.x_atoms.shape[0], dtype=torch.int)
    mask[torch.as_tensor(atoms, dtype=torch.long)] = 1
    rec.atom_mask = mask
    return rec


def replicas(case, mols):
    """(unmasked records, replica records, int64 [R, 2] (molecule, group)), the groups of a molecule in ascending order."""
    plain = [with_mask(m, []) for m in mols]
    recs, table = [], []
    for i, m in enumerate(mols):
        g = groups_of(case, m)
        for gid in np.unique(g[g >= 0]).tolist():
            recs.append(with_mask(m, np.nonzero(g == gid)[0]))
            table.append((i, gid))
    return plain, recs, np.asarray(table, dtype=np.int64).reshape(-1, 2)


def main():
    install_stubs()
    with mg.quiet():
        from fragnet.vizualize import model_attr as ref_attr
        from fragnet.model.cdrp.model import CDRPModel
        from fragnet.model.dta.model import DTAModel2                 # reseeds torch and numpy at import
    from fragnet_amd import synth
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)

    def pair(make, seed, scaled=False):
        """(unmasked model, apply_mask=True model) with the same weights, as the reference loads one checkpoint into both."""
        torch.manual_seed(seed)
        with mg.quiet():
            masked = make(True)
        enc = masked.drug_model if hasattr(masked, "drug_model") else masked
        mg.zero_dead_bias(enc)
        if scaled:
            ac.scale_model(masked)
        with mg.quiet():
            plain = make(False)
        plain.load_state_dict(masked.state_dict())
        return plain.eval(), masked.eval()

    def with_protein(collate):
        def run(recs):
            b = collate(recs)
            b["protein"] = torch.cat([i.protein.view(1, -1) for i in recs], dim=0).type(torch.long)      # data.py:1089, 1108
            return b
        return run

    ft_ctor = dict(atom_features=167, frag_features=167, edge_features=17, emb_dim=128, **ac.CTOR)
    esol = lambda: ac.molecules()
    cases = {
        "property": dict(mols=esol, collate=ref_attr.collate_fn, seed=ac.SEED, scaled=True, ctor=ft_ctor,
                         make=lambda m: ref_attr.FragNetFineTune(**ft_ctor, apply_mask=m)),
        "property_groups": dict(mols=esol, collate=ref_attr.collate_fn, seed=ac.SEED, scaled=True, ctor=ft_ctor,
                                make=lambda m: ref_attr.FragNetFineTune(**ft_ctor, apply_mask=m)),
        "energy": dict(mols=esol, collate=ref_attr.collate_fn, seed=5, scaled=False, ctor=ENERGY_CTOR, output=3,
                       make=lambda m: ref_attr.FragNetPreTrain(**ENERGY_CTOR, apply_mask=m)),
        "drp": dict(mols=lambda: synth.attach_gene_expr(synth.synth_molecules(5, seed=mgc.MOL_SEED, profile="esol"), mgc.GENE_DIM,
                                                        mgc.GENE_SEED, mgc.PINNED),
                    collate=ref_attr.collate_fn_cdrp, seed=mgc.SEED, scaled=False, ctor=mgc.CTOR,
                    make=lambda m: CDRPModel(ref_attr.FragNetFineTuneBaseViz(**mgc.CTOR, apply_mask=m), mgc.GENE_DIM, "cpu")),
        "dta": dict(mols=lambda: synth.attach_protein(synth.synth_molecules(5, seed=mgd.MOL_SEED, profile="esol"), mgd.PROT_SEED, length=1000,
                                                      pinned=mgd.PINNED),
                    collate=with_protein(ref_attr.collate_fn), seed=mgd.SEED, scaled=False, ctor=mgd.CTOR,
                    make=lambda m: DTAModel2(ref_attr.FragNetFineTuneBaseViz(**mgd.CTOR, apply_mask=m))),
    }
    cfg = {"head_scale": ac.HEAD_SCALE, "att_scale": ac.ATT_SCALE, "cases": {}}
    store = {}
    for name, c in cases.items():
        mols = c["mols"]()
        plain_recs, recs, table = replicas(name, mols)
        plain, masked = pair(c["make"], c["seed"], c["scaled"])
        pick = (lambda o: o[c["output"]]) if "output" in c else (lambda o: o)
        with torch.no_grad(), mg.quiet():
            base = pick(plain(c["collate"](plain_recs))).reshape(len(mols), -1).numpy().astype(np.float32)
            pm = pick(masked(c["collate"](recs))).reshape(len(recs), -1).numpy().astype(np.float32)
        keys, sums = mg.param_checksums(masked)
        store[f"{name}/pkeys"], store[f"{name}/psums"] = np.asarray(json.dumps(keys)), sums
        store[f"{name}/pred_no_mask"], store[f"{name}/replica"], store[f"{name}/pred_mask"] = base, table, pm
        attr = base[table[:, 0]] - pm
        big = (np.abs(attr) > 10 * ac.attr_tolerance(base[table[:, 0]])).all(axis=1)
        cfg["cases"][name] = {"ctor": c["ctor"], "seed": c["seed"], "scaled": c["scaled"], "n_mols": len(mols),
                              "atoms": [int(m.x_atoms.shape[0]) for m in mols], "fragments": [int(m.n_frags) for m in mols]}
        print(f"{name}: {len(mols)} molecules, {len(recs)} replicas, atoms {cfg['cases'][name]['atoms']}, fragments "
              f"{cfg['cases'][name]['fragments']}, {int(big.sum())}/{len(big)} attributions above 10 x tolerance")
        assert big.mean() >= MIN_SHARE[name], name
    cfg.update(mol_seed=ac.MOL_SEED, profile="esol", cdrp=dict(mol_seed=mgc.MOL_SEED, gene_seed=mgc.GENE_SEED, gene_dim=mgc.GENE_DIM,
               pinned=list(mgc.PINNED)), dta=dict(mol_seed=mgd.MOL_SEED, prot_seed=mgd.PROT_SEED, pinned={str(k): v for k, v in mgd.PINNED.items()}))
    store["cfg"] = np.asarray(json.dumps(cfg))
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **store)
    print(f"{NAME}.npz: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
