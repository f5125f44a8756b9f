"""Host side of the fragment contributions (fragnet_amd/attribution.py ``fragment_contributions``, fragnet_amd/attr_model.py and the
alias fragnet/vizualize/model_attr.py): the replica table, the refusals, the result class, the drop-in classes' state-dict keys against
the reference fixture tests/golden/frag_attr.npz, and the fixture's consistency with the oracle."""
import importlib
import json
import sys

import numpy as np
import pytest
import torch

from tests import attr_common as ac
from tests import fragattr_common as fc
from tests.conftest import ROOT


# ------------------------------------------------------------------------------------------------ replica table
def test_replica_table_from_fragment_maps_and_custom_groups():
    from fragnet_amd import attribution as attr
    frag_maps = [np.array([0, 0, 1, 2, 2, 1]), np.array([0, 0, 0]), np.array([1, 0, 1, 0])]            # the second molecule has one fragment
    ids, sizes = attr.group_table(frag_maps)
    assert [u.tolist() for u in ids] == [[0, 1, 2], [0], [0, 1]]
    assert [c.tolist() for c in sizes] == [[2, 2, 2], [3], [2, 2]]
    # custom groups: ascending order whatever the order of appearance, ungrouped atoms (< 0) in no replica, an id no atom carries (3)
    # has no replica, a molecule whose atoms are all ungrouped has none
    ids, sizes = attr.group_table([np.array([5, -1, 2, 5, -7, 4]), np.array([-1, -1]), np.array([7])])
    assert [u.tolist() for u in ids] == [[2, 4, 5], [], [7]]
    assert [c.tolist() for c in sizes] == [[1, 1, 2], [], [1]]
    assert all(u.dtype == np.int64 and c.dtype == np.int64 for u, c in zip(ids, sizes))
    # ids too large for the histogram take the sorting path: the same table
    big = [np.array([5, -1, 2, 5, -7, 4]) * 10 ** 12, np.array([-1, -1]), np.array([7])]
    ids, sizes = attr.group_table(big)
    assert [u.tolist() for u in ids] == [[2 * 10 ** 12, 4 * 10 ** 12, 5 * 10 ** 12], [], [7]] and [c.tolist() for c in sizes] == [[1, 1, 2], [], [1]]
    assert attr.group_table([]) == ([], [])
    mol, gid, cnt, per = attr.flat_group_table(np.array([1, 1, 0, -1, 3]), np.array([0, 3, 3, 5]))
    assert (mol.tolist(), gid.tolist(), cnt.tolist(), per.tolist()) == ([0, 0, 2], [0, 1, 3], [1, 2, 1], [2, 0, 1])


def test_replica_table_of_the_fixture_molecules_is_the_reference_order():
    from fragnet_amd import attribution as attr
    for case in fc.CASES:
        mols = fc.molecules(case)
        ids, _ = attr.group_table(fc.atom_groups(case, mols))
        table = np.array([(i, g) for i, u in enumerate(ids) for g in u.tolist()], dtype=np.int64).reshape(-1, 2)
        np.testing.assert_array_equal(table, fc.reference(case)[1])
        np.testing.assert_array_equal(fc.literal_replicas(mols, fc.atom_groups(case, mols))[1], table)


# ------------------------------------------------------------------------------------------------ refusals
def test_groups_of_the_wrong_length_or_dtype_are_refused():
    from fragnet_amd import attribution as attr
    from fragnet_amd.model import FragNetFineTune
    mols = ac.molecules(2)
    model = FragNetFineTune(**ac.CTOR)
    n = [int(m.x_atoms.shape[0]) for m in mols]
    with pytest.raises(ValueError, match="one array per molecule"):
        attr.fragment_contributions(model, mols, groups=[np.zeros(n[0], dtype=np.int64)])
    with pytest.raises(ValueError, match=f"for a molecule of {n[1]} atoms"):
        attr.fragment_contributions(model, mols, groups=[np.zeros(n[0], dtype=np.int64), np.zeros(n[1] + 1, dtype=np.int64)])
    with pytest.raises(ValueError, match="integer"):
        attr.fragment_contributions(model, mols, groups=[np.zeros(k, dtype=np.float32) for k in n])
    with pytest.raises(ValueError, match="1-d"):
        attr.fragment_contributions(model, mols, groups=[np.zeros((k, 1), dtype=np.int64) for k in n])


def test_a_cpu_model_and_an_unsupported_class_are_refused():
    from fragnet_amd import _lib, attribution as attr, cdrp
    from fragnet_amd.dataset import FlatMolStore
    from fragnet_amd.model import FragNetFineTune
    mols = ac.molecules(2)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        attr.fragment_contributions(FragNetFineTune(**ac.CTOR), mols)
    with pytest.raises(ValueError, match="Linear is not one of"):
        attr.fragment_contributions(torch.nn.Linear(2, 2), mols)
    pair = cdrp.CDRPModel(cdrp.FragNetFineTuneBase(**ac.CTOR), 16, "cpu")
    with pytest.raises(ValueError, match="list of records"):
        attr.fragment_contributions(pair, FlatMolStore.from_records(mols))
    with pytest.raises(_lib.FragnetHipError):
        from fragnet_amd import ops
        ops.pool_cat_groups(torch.zeros(3, 128), torch.zeros(1, 128), None, torch.zeros(3, dtype=torch.int64),
                            torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ the result class
def _result():
    from fragnet_amd.attribution import FragmentAttribution
    atom_groups = [np.array([2, -1, 0, 2, 0], dtype=np.int64), np.array([-1, -1], dtype=np.int64), np.array([4, 4, 4], dtype=np.int64)]
    pred_no_mask = np.array([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0]], dtype=np.float32)
    pred_mask = np.array([[0.5, 9.0], [0.25, 12.0], [1.0, 40.0]], dtype=np.float32)            # molecule 0: groups 0, 2; molecule 2: group 4
    mol_of = np.array([0, 0, 2])
    return FragmentAttribution(pred_no_mask, np.array([0, 2, 2, 3], dtype=np.int64), np.array([0, 2, 4], dtype=np.int64),
                               np.array([2, 2, 3], dtype=np.int64), pred_mask, pred_no_mask[mol_of] - pred_mask, np.concatenate(atom_groups),
                               np.array([0, 5, 7, 10], dtype=np.int64))


def test_fragment_attribution_indexing_arrays_and_atom_weights():
    res = _result()
    assert len(res) == 3
    m0, m1 = res[0], res[1]
    assert m0["group"].tolist() == [0, 2] and m0["n_atoms"].tolist() == [2, 2] and m0["pred_no_mask"].tolist() == [1.0, 10.0]
    np.testing.assert_array_equal(m0["attr"], [[0.5, 1.0], [0.75, -2.0]])
    assert m1["group"].shape == (0,) and m1["pred_mask"].shape == (0, 2) and m1["attr"].shape == (0, 2)
    np.testing.assert_array_equal(res[-1]["attr"], res[2]["attr"])
    with pytest.raises(IndexError):
        res[3]
    # every atom its group's attribution, ungrouped atoms 0 (the reference's add_atom_weights)
    np.testing.assert_array_equal(res.atom_weights(0), [[0.75, -2.0], [0.0, 0.0], [0.5, 1.0], [0.75, -2.0], [0.5, 1.0]])
    np.testing.assert_array_equal(res.atom_weights(1), np.zeros((2, 2), dtype=np.float32))
    np.testing.assert_array_equal(res.atom_weights(2), [[2.0, -10.0]] * 3)
    a = res.arrays()
    assert sorted(a) == ["atom_group", "atom_offsets", "attr", "group", "n_atoms", "offsets", "pred_mask", "pred_no_mask"]
    assert a["offsets"].tolist() == [0, 2, 2, 3] and a["atom_offsets"].tolist() == [0, 5, 7, 10]
    assert a["atom_group"].tolist() == [2, -1, 0, 2, 0, -1, -1, 4, 4, 4]
    np.testing.assert_array_equal(a["attr"], a["pred_no_mask"][np.repeat(np.arange(3), np.diff(a["offsets"]))] - a["pred_mask"])


# ------------------------------------------------------------------------------------------------ the drop-in classes
@pytest.fixture
def _this_repo_first():
    sys.path.insert(0, ROOT)
    for k in [k for k in sys.modules if k == "fragnet" or k.startswith("fragnet.")]:
        del sys.modules[k]
    yield
    sys.path.remove(ROOT)


def test_the_alias_module_resolves_to_the_drop_in_classes(_this_repo_first):
    from fragnet_amd import attr_model
    mod = importlib.import_module("fragnet.vizualize.model_attr")
    assert mod.__file__.startswith(ROOT)
    for name in ("FragNetFineTune", "FragNetFineTuneBaseViz", "FragNetPreTrain", "collate_fn", "collate_fn_cdrp"):
        assert getattr(mod, name) is getattr(attr_model, name)


def test_state_dict_keys_and_weights_of_the_five_cases_are_the_reference_s():
    """Same seed and construction order give the reference's weights (checksums), so its checkpoints load strictly."""
    from fragnet_amd import attr_model, cdrp, dta
    z = fc.fixture()
    for case in fc.CASES:
        model = fc.build(case)                              # checks keys and checksums against the fixture
        assert list(model.state_dict()) == json.loads(str(z[f"{case}/pkeys"]))
        enc = model.drug_model if case in ("drp", "dta") else model
        assert enc.apply_mask is True
    assert isinstance(fc.build("drp"), cdrp.CDRPModel) and isinstance(fc.build("dta"), dta.DTAModel2)
    assert isinstance(fc.build("energy", apply_mask=False), attr_model.FragNetPreTrain)


def test_mask_all_layers_is_refused_and_collates_add_the_atom_mask():
    from fragnet_amd import attr_model, data
    for cls in (attr_model.FragNetFineTune, attr_model.FragNetFineTuneBaseViz):
        with pytest.raises(NotImplementedError, match=r"model_attr\.py:116-117"):
            cls(**ac.CTOR, apply_mask=True, mask_all_layers=True)
    mols = fc.molecules("drp")[:3]
    recs, table = fc.literal_replicas(mols, fc.atom_groups("drp", mols))
    for collate, plain, keys in ((attr_model.collate_fn, data.collate_fn, data.BATCH_KEYS_FT), (attr_model.collate_fn_cdrp, data.collate_fn_cdrp, data.BATCH_KEYS_CDRP)):
        got, want = collate(recs), plain(recs)
        assert tuple(got) == keys + ("atom_mask",)
        assert got["atom_mask"].dtype == torch.int32 and got["atom_mask"].shape == (got["x_atoms"].shape[0],)
        for k in keys:
            assert torch.equal(got[k], want[k]), k
        per_replica = torch.split(got["atom_mask"], [int(r.x_atoms.shape[0]) for r in recs])
        for (i, gid), m in zip(table, per_replica):
            np.testing.assert_array_equal(m.numpy() == 1, fc.atom_groups("drp", mols)[i] == gid)


# ------------------------------------------------------------------------------------------------ the fixture itself
@pytest.mark.parametrize("case", fc.CASES)
def test_the_fixture_s_masks_matter(case):
    fc.assert_the_masks_matter(case)


def test_the_fixture_agrees_with_the_oracle_pooling_without_the_fragment_s_rows():
    """oracle/fragnet_ref.py's encoder on the CPU ONCE for the six molecules, then per replica: the fragment's rows zeroed, the two
    sums, the head -- the identity the engine path rests on -- gives the reference's ``property`` numbers within the tolerance."""
    from fragnet_amd import data
    from oracle import fragnet_ref as R
    torch.set_num_threads(4)
    cfg = fc.fixture()["cfg"]["cases"]["property"]
    gold = ac.build(R, cfg["ctor"], cfg["seed"], scaled=True)
    mols = fc.molecules("property")
    batch = data.collate_fn(mols)
    base, rep, pm = fc.reference("property")
    with torch.no_grad():
        x_atoms, x_frags = gold.pretrain(batch)[:2]
        fc.close(gold.fthead(R.pool_cat(x_atoms, x_frags, batch)).numpy(), base, "pred_no_mask")
        first = np.concatenate([[0], np.cumsum([int(m.x_atoms.shape[0]) for m in mols])])
        rows = []
        for i, gid in rep.tolist():
            xz = x_atoms.clone()
            own = torch.from_numpy(mols[i].atom_id_frag_id.numpy() == gid)
            xz[first[i]: first[i + 1]][own] = 0.0
            rows.append(gold.fthead(R.pool_cat(xz, x_frags, batch))[i])
        fc.close(torch.stack(rows).numpy(), pm, "pred_mask")
