"""Fragment contributions on the engine: the leave-group-out read-out (fn_pool_cat_groups_f32, ops.pool_cat_groups), the batched API
(fragnet_amd/attribution.py ``fragment_contributions``), the literal drop-in models (fragnet_amd/attr_model.py) and the script.

Expected values: ``fn_pool_cat_f32`` bit for bit for the kernel; the reference's own numbers (tests/golden/frag_attr.npz: its model_attr
classes unmasked and with ``apply_mask=True`` on the replicated records) and this project's literal path on the GPU for the API.
Tolerances are the project's (tests/attr_common.py): |got - ref| <= 1e-4 + 1e-4 |ref| for a prediction, twice that (on |pred_no_mask|)
for a difference of two.  That the fixture's masks matter is asserted on the reference's values (tests/fragattr_common.py): share of
replicas with |attribution| > 10 x tolerance: property 26/28, property_groups 18/18, energy 21/28, drp 12/12, dta 11/11."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attr_common as ac
from tests import fragattr_common as fc
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _kernel_inputs(order):
    """Random encoder outputs on a collated batch of 7 molecules (atoms 26, 31, 12, 51, 36, 34 and a seventh) in ``order``."""
    from fragnet_amd import data
    from fragnet_amd.plan import plan_for
    mols = ac.molecules(7)
    assert 12 in [int(m.x_atoms.shape[0]) for m in mols] and max(int(m.x_atoms.shape[0]) for m in mols) > 8
    mols = [mols[i] for i in order]
    batch = data.batch_to(data.collate_fn(mols), DEV)
    g = torch.Generator().manual_seed(3)
    xa = torch.randn(batch["x_atoms"].shape[0], 128, generator=g).to(DEV)
    xf = torch.randn(batch["x_frags"].shape[0], 128, generator=g).to(DEV)
    groups = [m.atom_id_frag_id.numpy().astype(np.int64) for m in mols]
    return mols, batch, plan_for(batch), xa, xf, groups


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5, 6), (4, 2, 6, 0, 5, 3, 1)], ids=["in-order", "permuted"])
def test_the_read_out_equals_pool_cat_bit_for_bit(order):
    from fragnet_amd import ops
    mols, batch, plan, xa, xf, groups = _kernel_inputs(order)
    B = len(mols)
    first = np.concatenate([[0], np.cumsum([g.shape[0] for g in groups])])
    plain = ops.pool_cat(xa, xf, plan)
    reps = [(i, gid) for i, g in enumerate(groups) for gid in np.unique(g).tolist()]
    # the unmasked rows, every fragment row, a foreign id per molecule (no atom of it carries 99) -- in one call
    row_mol = list(range(B)) + [i for i, _ in reps] + list(range(B))
    row_group = [-1] * B + [gid for _, gid in reps] + [99] * B
    atom_group = _dev(np.concatenate(groups), np.int64)
    out = ops.pool_cat_groups(xa, xf, plan, atom_group, _dev(row_mol, np.int32), _dev(row_group, np.int64))
    assert out.shape == (len(row_mol), 256) and not out.requires_grad
    assert torch.equal(out[:B], plain), "unmasked rows differ from fn_pool_cat_f32"
    assert torch.equal(out[B + len(reps):], plain), "a group id foreign to the molecule must give the unmasked row"
    for r, (i, gid) in enumerate(reps):
        xz = xa.clone()
        xz[first[i]: first[i + 1]][torch.from_numpy(groups[i] == gid).to(DEV)] = 0.0
        want = ops.pool_cat(xz, xf, plan)[i]
        assert torch.equal(out[B + r], want), f"molecule {i} fragment {gid}: differs from fn_pool_cat_f32 of the zeroed table"
        assert torch.equal(out[B + r, 128:], plain[i, 128:])
    assert any(not torch.equal(out[B + r, :128], plain[i, :128]) for r, (i, _) in enumerate(reps))
    # rows in shuffled and repeated order: the same bytes per row
    perm = np.random.default_rng(5).permutation(np.concatenate([np.arange(len(row_mol)), np.arange(0, len(row_mol), 3)]))
    again = ops.pool_cat_groups(xa, xf, plan, atom_group, _dev(np.asarray(row_mol)[perm], np.int32), _dev(np.asarray(row_group)[perm], np.int64))
    assert torch.equal(again, out[torch.from_numpy(perm).to(DEV)])
    # a group that covers a whole molecule: the atoms' half is exactly 0.0, the fragments' half unchanged; ungrouped atoms (< 0) stay in
    # every row, the unmasked one (row_group -1) included
    whole = np.concatenate([np.zeros_like(g) if i % 2 == 0 else np.where(np.arange(g.shape[0]) % 2 == 0, -1, 1) for i, g in enumerate(groups)])
    got = ops.pool_cat_groups(xa, xf, plan, _dev(whole, np.int64), _dev(list(range(B)) * 2, np.int32), _dev([0] * B + [-1] * B, np.int64))
    for i in range(B):
        assert torch.equal(got[i, 128:], plain[i, 128:])
        if i % 2 == 0:
            assert bool((got[i, :128] == 0.0).all())
        else:
            assert torch.equal(got[i], plain[i]), "group 0 is foreign to a molecule whose ids are -1 and 1"
    assert torch.equal(got[B:], plain), "row_group -1 must not leave the atoms with id -1 out"
    # R == 0
    empty = ops.pool_cat_groups(xa, xf, plan, atom_group, torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    assert empty.shape == (0, 256) and empty.dtype == torch.float32 and empty.device == xa.device


def test_the_op_validates_its_rows_on_the_host():
    from fragnet_amd import ops
    mols, batch, plan, xa, xf, groups = _kernel_inputs(range(7))
    atom_group = _dev(np.concatenate(groups), np.int64)
    one = lambda v, t: _dev([v], t)
    for bad in (7, -1):
        with pytest.raises(IndexError, match="row_mol"):
            ops.pool_cat_groups(xa, xf, plan, atom_group, one(bad, np.int32), one(0, np.int64))
    with pytest.raises(ValueError, match="row_mol"):
        ops.pool_cat_groups(xa, xf, plan, atom_group, one(0, np.int64), one(0, np.int64))
    with pytest.raises(ValueError, match="row_group"):
        ops.pool_cat_groups(xa, xf, plan, atom_group, one(0, np.int32), _dev([0, 0], np.int64))
    with pytest.raises(ValueError, match="atom_group"):
        ops.pool_cat_groups(xa, xf, plan, atom_group[:-1], one(0, np.int32), one(0, np.int64))
    with pytest.raises(ValueError, match="feature tables"):
        ops.pool_cat_groups(xa[:-1], xf, plan, atom_group, one(0, np.int32), one(0, np.int64))


def test_the_library_refuses_bad_arguments_without_touching_the_output():
    """FN_EINVAL through fail() before any launch: null descriptors / buffers, an n_seg mismatch, R < 0; a 7.0-filled output stays."""
    from fragnet_amd import _lib, ops
    from fragnet_amd.plan import _stream_ptr
    mols, batch, plan, xa, xf, groups = _kernel_inputs(range(7))
    lib = _lib.load()
    atom_group = _dev(np.concatenate(groups), np.int64)
    row_mol, row_group = _dev([0, 1], np.int32), _dev([0, -1], np.int64)
    out = torch.full((2, 256), 7.0, device=DEV)
    a, f = ops._seg_struct(plan.segs["mol_atoms"]), ops._seg_struct(plan.segs["mol_frags"])
    short = ops._seg_struct(plan.segs["mol_frags"])
    short.n_seg -= 1
    no_rowptr = ops._seg_struct(plan.segs["mol_atoms"])
    no_rowptr.rowptr = None
    st = _stream_ptr(xa.device)
    good = dict(xa=xa.data_ptr(), xf=xf.data_ptr(), a=C.byref(a), f=C.byref(f), ag=atom_group.data_ptr(), rm=row_mol.data_ptr(),
                rg=row_group.data_ptr(), R=2, out=out.data_ptr())
    for change in (dict(a=None), dict(f=None), dict(f=C.byref(short)), dict(R=-1), dict(rm=None), dict(rg=None), dict(ag=None), dict(xa=None),
                   dict(xf=None), dict(out=None), dict(a=C.byref(no_rowptr))):
        k = {**good, **change}
        rc = lib.fn_pool_cat_groups_f32(k["xa"], k["xf"], k["a"], k["f"], k["ag"], k["rm"], k["rg"], k["R"], k["out"], st)
        assert rc == _lib.FN_EINVAL, change
        assert b"fn_pool_cat_groups_f32" in lib.fn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert lib.fn_pool_cat_groups_f32(None, None, C.byref(a), C.byref(f), None, None, None, 0, None, st) == 0          # R == 0: nothing to do
    k = good
    assert lib.fn_pool_cat_groups_f32(k["xa"], k["xf"], k["a"], k["f"], k["ag"], k["rm"], k["rg"], k["R"], k["out"], st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[1], ops.pool_cat(xa, xf, plan)[1])


# ------------------------------------------------------------------------------------------------ 2. the reference fixture
def _contributions(case, **kw):
    from fragnet_amd import attribution as attr
    model = fc.build(case, DEV)
    mols = fc.molecules(case)
    return attr.fragment_contributions(model, mols, groups=fc.groups(case, mols), **kw), model, mols


_RESULTS = {}          # case -> (result, model, molecules): computed once, shared by the fixture and the literal-path checks


def _shared(case):
    if case not in _RESULTS:
        _RESULTS[case] = _contributions(case)
    return _RESULTS[case]


def _table(res):
    return np.array([(i, g) for i in range(len(res)) for g in res[i]["group"].tolist()], dtype=np.int64).reshape(-1, 2)


@pytest.mark.parametrize("case", fc.CASES)
def test_fragment_contributions_match_the_reference_fixture(case):
    fc.assert_the_masks_matter(case)
    base, rep, pm = fc.reference(case)
    res, _, mols = _shared(case)
    a = res.arrays()
    print(f"{case}: max |pred_no_mask - ref| {np.abs(a['pred_no_mask'] - base).max():.3e}, max |pred_mask - ref| {np.abs(a['pred_mask'] - pm).max():.3e}")
    assert len(res) == len(mols)
    np.testing.assert_array_equal(_table(res), rep)
    fc.close(a["pred_no_mask"], base, f"{case}: pred_no_mask")
    fc.close(a["pred_mask"], pm, f"{case}: pred_mask")
    rows = base[rep[:, 0]].astype(np.float64)
    err = np.abs(a["attr"].astype(np.float64) - (rows - pm)) - ac.attr_tolerance(rows)
    assert a["attr"].shape == pm.shape and (err <= 0).all(), f"{case}: attr off by {err.max():.3e} over the tolerance"
    sizes = np.concatenate([np.unique(g[g >= 0], return_counts=True)[1] for g in fc.atom_groups(case, mols)])
    np.testing.assert_array_equal(a["n_atoms"], sizes)
    w = res.atom_weights(0)
    g0 = fc.atom_groups(case, mols)[0]
    assert w.shape == (g0.shape[0], pm.shape[1]) and bool((w[g0 < 0] == 0).all())
    np.testing.assert_array_equal(w[g0 == res[0]["group"][0]], np.repeat(res[0]["attr"][:1], int((g0 == res[0]["group"][0]).sum()), 0))


# ------------------------------------------------------------------------------------------------ 3. the literal path on the GPU
def _literal(case, model, mols, groups):
    from fragnet_amd import data
    recs, table = fc.literal_replicas(mols, groups)
    with torch.no_grad():
        out = model(data.batch_to(fc.literal_collate(case)(recs), DEV))
    out = out[3] if case == "energy" else out
    return out.reshape(len(recs), -1).float().cpu().numpy(), table


@pytest.mark.parametrize("case", fc.CASES)
def test_the_literal_models_agree_with_fragment_contributions(case):
    """The drop-in classes with apply_mask=True on the replicated, collated batch (one encoder pass per replica) against the one pass
    per molecule: the prediction tolerance -- the encoder runs on other batch compositions, so bit equality is not claimed."""
    res, model, mols = _shared(case)
    pm, table = _literal(case, model, mols, fc.atom_groups(case, mols))
    np.testing.assert_array_equal(_table(res), table)
    fc.close(res.pred_mask, pm, f"{case}: pred_mask against the literal path")
    fc.close(pm, fc.reference(case)[2], f"{case}: the literal path against the reference")


@pytest.mark.parametrize("name,ctor,profile,seed", [("gat2_lite", dict(ac.CTOR, variant="gat2_lite"), "esol", 11),
                                                     ("tox21-12", dict(ac.CTOR, n_classes=12), "tox21", 7)])
def test_other_model_versions_and_multi_task_heads_against_the_literal_path(name, ctor, profile, seed):
    from fragnet_amd import attr_model, attribution as attr
    from fragnet_amd.dataset import FlatMolStore
    torch.manual_seed(seed)
    model = attr_model.FragNetFineTune(**ctor, apply_mask=True)
    ac.scale_model(model)
    model = model.to(DEV).eval()
    mols = ac.molecules(4, seed=4300, profile=profile)
    res = attr.fragment_contributions(model, FlatMolStore.from_records(mols).to(DEV))
    groups = [m.atom_id_frag_id.numpy().astype(np.int64) for m in mols]
    pm, table = _literal("property", model, mols, groups)
    assert res.pred_no_mask.shape == (4, ctor["n_classes"]) and res.pred_mask.shape == pm.shape
    np.testing.assert_array_equal(_table(res), table)
    fc.close(res.pred_mask, pm, f"{name}: pred_mask against the literal path")
    model.apply_mask = False
    with torch.no_grad():
        from fragnet_amd import data
        base = model(data.batch_to(data.collate_fn(mols), DEV))
    fc.close(res.pred_no_mask, base.reshape(4, -1).cpu().numpy(), f"{name}: pred_no_mask")
    rows = res.pred_no_mask[table[:, 0]].astype(np.float64)
    assert (np.abs(rows - pm) > 10 * ac.attr_tolerance(rows)).any(axis=1).mean() >= 0.5, "the masks do not matter for this model"


# ------------------------------------------------------------------------------------------------ 4. one encoder pass per chunk
class _Counting:
    """Stands in for the loaded library: counts the calls of every fn_* entry point (fn_last_error aside)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("fn_") or name == "fn_last_error":
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


def test_one_encoder_pass_and_one_read_out_per_chunk(monkeypatch):
    from fragnet_amd import _lib, attribution as attr
    from fragnet_amd.dataset import FlatMolStore
    model = fc.build("property", DEV)
    store = FlatMolStore.from_records(fc.molecules("property")).to(DEV)
    proxy = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    model.train()
    one = attr.fragment_contributions(model, store)
    assert model.training, "the training flag is restored"
    calls = list(proxy.calls)
    assert calls.count("fn_encoder_forward") == 1 and calls.count("fn_pool_cat_groups_f32") == 1
    assert "fn_encoder_forward_masked" not in calls and "fn_pool_cat_f32" not in calls
    proxy.calls.clear()
    two = attr.fragment_contributions(model.eval(), store, batch_size=4)
    calls = list(proxy.calls)
    assert calls.count("fn_encoder_forward") == 2 and calls.count("fn_pool_cat_groups_f32") == 2
    assert "fn_encoder_forward_masked" not in calls
    np.testing.assert_array_equal(two.offsets, one.offsets)
    np.testing.assert_array_equal(two.group, one.group)
    fc.close(two.pred_no_mask, one.pred_no_mask, "pred_no_mask, two chunks against one")
    fc.close(two.pred_mask, one.pred_mask, "pred_mask, two chunks against one")
    fc.close(one.pred_mask, fc.reference("property")[2], "pred_mask (a FlatMolStore source) against the reference")


# ------------------------------------------------------------------------------------------------ 5. a molecule without groups
def test_a_molecule_whose_atoms_are_all_ungrouped_has_no_replica():
    from fragnet_amd import attribution as attr
    model = fc.build("property", DEV)
    mols = fc.molecules("property")[:3]
    n = [int(m.x_atoms.shape[0]) for m in mols]
    groups = [np.full(n[0], -1, dtype=np.int64), np.arange(n[1], dtype=np.int64) % 2, np.full(n[2], -3, dtype=np.int64)]
    res = attr.fragment_contributions(model, mols, groups=groups)
    assert res.offsets.tolist() == [0, 0, 2, 2]
    for i in (0, 2):
        assert res[i]["group"].shape == (0,) and res[i]["pred_mask"].shape == (0, 1) and res[i]["attr"].shape == (0, 1)
        assert res.atom_weights(i).shape == (n[i], 1) and not res.atom_weights(i).any()
    fc.close(res.pred_no_mask, fc.reference("property")[0][:3], "pred_no_mask")
    none = attr.fragment_contributions(model, mols[:1], groups=groups[:1])
    assert none.pred_mask.shape == (0, 1) and none.attr.shape == (0, 1) and none.group.shape == (0,) and none.pred_no_mask.shape == (1, 1)


# ------------------------------------------------------------------------------------------------ 6. the script
def _script():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import attribute_fragments_gat2
    finally:
        sys.path.pop(0)
    return attribute_fragments_gat2


@pytest.mark.parametrize("prop_type,config", [("property", ("exps", "ft", "esol_synth", "config.yaml")), ("energy", ("exps", "pt", "synth", "config.yaml"))])
def test_script_writes_the_arrays_fragment_contributions_returns(tmp_path, prop_type, config):
    from fragnet_amd import attribution as attr, synth, train
    from fragnet_amd.dataset import FlatMolStore
    mod = _script()
    config = os.path.join(ROOT, *config)
    FlatMolStore.from_records(synth.synth_molecules(24, seed=2, profile="esol")).save(str(tmp_path / "test.pt"))
    torch.manual_seed(11)
    model = mod.build_model(train.load_config(config, config=config), prop_type)
    torch.save(model.state_dict(), str(tmp_path / "model.pt"))
    out = str(tmp_path / "frag.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "attribute_fragments_gat2.py"), "--config", config, "--checkpoint",
                        str(tmp_path / "model.pt"), "--data", str(tmp_path / "test.pt"), "--out", out, "--prop-type", prop_type, "--batch-size", "16"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = attr.fragment_contributions(model.to(DEV), FlatMolStore.load(str(tmp_path / "test.pt"), device=DEV))
    assert f"24 molecules, {int(res.offsets[-1])} fragment replicas -> {out}" in r.stdout
    z = np.load(out)
    want = res.arrays()
    assert sorted(z.files) == sorted(want)
    for k in ("offsets", "group", "n_atoms", "atom_group", "atom_offsets"):
        np.testing.assert_array_equal(z[k], want[k])
    fc.close(z["pred_no_mask"], want["pred_no_mask"], "pred_no_mask")
    fc.close(z["pred_mask"], want["pred_mask"], "pred_mask")
    np.testing.assert_allclose(z["attr"], z["pred_no_mask"][np.repeat(np.arange(24), np.diff(z["offsets"]))] - z["pred_mask"], atol=1e-6)
