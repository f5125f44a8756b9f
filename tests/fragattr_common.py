"""Shared by the fragment-contribution tests: the fixture tests/golden/frag_attr.npz (tests/golden/make_golden_fragattr.py), this
project's models of its five cases with the fixture's weights, their molecules and groups, and the literal replicated records."""
import copy
import json
import os

import numpy as np
import torch

from tests import attr_common as ac
from tests.helpers import GOLDEN, check_params_match

CASES = ("property", "property_groups", "energy", "drp", "dta")
# share of replicas whose reference attribution exceeds 10 x its tolerance: the condition that makes the fixture's masks matter
MIN_SHARE = {"property": 0.75, "property_groups": 0.75, "energy": 0.5, "drp": 0.75, "dta": 0.75}
REPLICAS = {"property": 28, "property_groups": 18, "energy": 28, "drp": 12, "dta": 11}

_FIXTURE = {}


def fixture():
    if not _FIXTURE:
        z = np.load(os.path.join(GOLDEN, "frag_attr.npz"))
        _FIXTURE.update({k: z[k] for k in z.files})
        _FIXTURE["cfg"] = json.loads(str(z["cfg"]))
    return _FIXTURE


def reference(case):
    """(pred_no_mask [B, C], replica [R, 2] (molecule, group), pred_mask [R, C]) as the reference computed them."""
    z = fixture()
    return z[f"{case}/pred_no_mask"], z[f"{case}/replica"], z[f"{case}/pred_mask"]


def assert_the_masks_matter(case):
    """The issue's condition on the fixture's own values."""
    base, rep, pm = reference(case)
    assert rep.shape == (REPLICAS[case], 2) and pm.shape[0] == REPLICAS[case]
    rows = base[rep[:, 0]].astype(np.float64)
    big = (np.abs(rows - pm) > 10 * ac.attr_tolerance(rows)).all(axis=1)
    assert big.mean() >= MIN_SHARE[case], (case, int(big.sum()), len(big))


def molecules(case):
    from fragnet_amd import synth
    cfg = fixture()["cfg"]
    if case == "drp":
        c = cfg["cdrp"]
        return synth.attach_gene_expr(synth.synth_molecules(5, seed=c["mol_seed"], profile="esol"), c["gene_dim"], c["gene_seed"], c["pinned"])
    if case == "dta":
        c = cfg["dta"]
        return synth.attach_protein(synth.synth_molecules(5, seed=c["mol_seed"], profile="esol"), c["prot_seed"], length=1000,
                                    pinned={int(k): v for k, v in c["pinned"].items()})
    return ac.molecules(cfg["cases"][case]["n_mols"], cfg["mol_seed"], cfg["profile"])


def groups(case, mols):
    """None (the fragments) or the custom groups of ``property_groups``: atom index % 3, atoms with index % 7 == 0 in no group."""
    if case != "property_groups":
        return None
    out = []
    for m in mols:
        g = np.arange(int(m.x_atoms.shape[0])) % 3
        g[np.arange(g.shape[0]) % 7 == 0] = -1
        out.append(g.astype(np.int64))
    return out


def build(case, device=None, apply_mask=True):
    """The drop-in model of the case (fragnet_amd.attr_model under cdrp.CDRPModel / dta.DTAModel2) with the fixture's weights: same seed
    and construction order, checked against the fixture's state-dict keys and checksums."""
    from fragnet_amd import attr_model, cdrp, dta
    z = fixture()
    c = z["cfg"]["cases"][case]
    torch.manual_seed(c["seed"])
    if case in ("property", "property_groups"):
        model = attr_model.FragNetFineTune(**c["ctor"], apply_mask=apply_mask)
    elif case == "energy":
        model = attr_model.FragNetPreTrain(**c["ctor"], apply_mask=apply_mask)
    elif case == "drp":
        model = cdrp.CDRPModel(attr_model.FragNetFineTuneBaseViz(**c["ctor"], apply_mask=apply_mask), z["cfg"]["cdrp"]["gene_dim"], device or "cpu")
    else:
        model = dta.DTAModel2(attr_model.FragNetFineTuneBaseViz(**c["ctor"], apply_mask=apply_mask))
    if c["scaled"]:
        ac.scale_model(model)
    check_params_match(model, json.loads(str(z[f"{case}/pkeys"])), z[f"{case}/psums"])
    model.eval()
    return model.to(device) if device is not None else model


def atom_groups(case, mols):
    g = groups(case, mols)
    return g if g is not None else [m.atom_id_frag_id.numpy().astype(np.int64) for m in mols]


def literal_replicas(mols, atom_group_arrays):
    """The records ``create_data`` builds (model_attr.py:734-761): one shallow copy per group with ``atom_mask[its atoms] = 1``, groups
    in ascending order; and the int64 [R, 2] table (molecule, group)."""
    recs, table = [], []
    for i, (m, g) in enumerate(zip(mols, atom_group_arrays)):
        for gid in np.unique(g[g >= 0]).tolist():
            rec = copy.copy(m)
            rec.atom_mask = torch.from_numpy((g == gid).astype(np.int32))
            recs.append(rec)
            table.append((i, gid))
    return recs, np.asarray(table, dtype=np.int64).reshape(-1, 2)


def literal_collate(case):
    """The collate of the literal path: attr_model's, plus ``protein`` as data.collate_fn_dta builds it for the DTA case."""
    from fragnet_amd import attr_model, data
    if case == "drp":
        return attr_model.collate_fn_cdrp
    if case == "dta":
        def run(recs):
            out = data.collate_fn_dta(recs)
            out["atom_mask"] = torch.cat([r.atom_mask for r in recs], dim=0).type(torch.int)
            return out
        return run
    return attr_model.collate_fn


def close(got, ref, what, scale=1.0):
    """|got - ref| <= scale (ATOL + RTOL |ref|): the project's prediction tolerance."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    err = np.abs(got - ref) - scale * (ac.ATOL + ac.RTOL * np.abs(ref))
    assert (err <= 0).all(), f"{what}: worst excess over the tolerance {err.max():.3e}"
