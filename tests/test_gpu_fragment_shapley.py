"""Fragment Shapley values on the engine: the coalition read-out (fn_pool_cat_coalitions_f32, ops.pool_cat_coalitions), the batched API
(fragnet_amd/attribution.py ``fragment_shapley``) and the script.

Expected values: ``fn_pool_cat_f32`` and ``fn_pool_cat_groups_f32`` bit for bit for the kernel; for the API the reference's own numbers
(tests/golden/frag_shapley.npz: its model_attr classes with ``apply_mask=True`` on one record per coalition, and the Shapley values of
those numbers by the definition) and this project's literal path on the GPU.  Tolerances are the project's (tests/attr_common.py): |got -
ref| <= 1e-4 + 1e-4 |ref| for a prediction; twice that for a Shapley value -- a group's weights sum to 1 over its 2^(F-1) differences of
two predictions, so an error t on every value moves phi by at most 2 t."""
import ctypes as C
import copy
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attr_common as ac
from tests import fragattr_common as fc
from tests import fragshap_common as sc
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# FN_TUNE_COALITION_STAGED: one workgroup per row; the tiled form with every run staged, with runs of >= 16 rows staged (the default's
# rule), with no run staged; the default (here one workgroup per row: fewer than 64 rows per molecule on average)
FORMS = {"rows": 0, "tiled, every run staged": 2, "tiled, long runs staged": 17, "tiled, global memory": 1 << 30, "default": 1}
KEY = 34
FULL64 = 2 ** 64 - 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def _masks(values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64).copy()).to(DEV)


# ------------------------------------------------------------------------------------------------ a. the read-out
ATOMS = (0, 1, 2, 8, 9, 17, 40, 130)          # 130: larger than the kernel's staging area (112 atoms); 40 (22 rows): a long run
GROUPS = (0, 1, 2, 1, 2, 3, 7, 64)
FRAGS = (0, 1, 2, 1, 3, 9, 4, 17)


def _read_out_inputs():
    """Eight hand-built molecules whose atom and fragment rows are interleaved in the tables (the pooling order is the plan's, not the
    table's): atom j of a molecule with F groups is in group j % F, every fifth atom of the molecules with 9, 40 and 130 atoms in no
    group; the molecule with 8 atoms has one group that holds all of them."""
    from fragnet_amd.plan import GraphPlan
    rng = np.random.default_rng(11)
    B = len(ATOMS)
    batch = rng.permutation(np.repeat(np.arange(B), ATOMS))
    frag_batch = rng.permutation(np.repeat(np.arange(B), FRAGS))
    bit = np.full(batch.shape[0], -1, dtype=np.int8)
    for m in range(B):
        where = np.flatnonzero(batch == m)
        j = np.arange(where.shape[0])
        b = (j % max(GROUPS[m], 1)).astype(np.int8)
        if ATOMS[m] in (9, 40, 130):
            b[(j % 5 == 4) & (j >= GROUPS[m])] = -1          # every group keeps an atom
        bit[where] = b if GROUPS[m] else -1
    plan = GraphPlan([dict(kind="seg", name="mol_atoms", key=_dev(batch, np.int64), n_seg=B),
                      dict(kind="seg", name="mol_frags", key=_dev(frag_batch, np.int64), n_seg=B)], torch.device(DEV))
    g = torch.Generator().manual_seed(3)
    xa = torch.randn(batch.shape[0], 128, generator=g).to(DEV)
    xf = torch.randn(frag_batch.shape[0], 128, generator=g).to(DEV)
    rows = []          # (molecule, mask), molecule-major
    for m in range(B):
        F = GROUPS[m]
        full = (1 << F) - 1
        masks = [0, full] + [full ^ (1 << k) for k in range(F)] + [1 << k for k in range(F)]
        masks += [int.from_bytes(rng.bytes(8), "little") & full for _ in range(6)]
        rows += [(m, k) for k in masks]
    return batch, bit, plan, xa, xf, rows


def _call(lib, xa, xf, plan, bit_d, row_mol_d, mask_d, R, out):
    from fragnet_amd import ops
    from fragnet_amd.plan import _stream_ptr
    a, f = ops._seg_struct(plan.segs["mol_atoms"]), ops._seg_struct(plan.segs["mol_frags"])
    return lib.fn_pool_cat_coalitions_f32(xa.data_ptr(), xf.data_ptr(), C.byref(a), C.byref(f), bit_d.data_ptr(), row_mol_d.data_ptr(),
                                          mask_d.data_ptr(), R, out.data_ptr(), _stream_ptr(xa.device))


def test_the_read_out_equals_pool_cat_bit_for_bit_in_every_form():
    from fragnet_amd import _lib, ops
    batch, bit, plan, xa, xf, rows = _read_out_inputs()
    lib = _lib.load()
    R = len(rows)
    assert R > 3 * 64 and sum(1 for m, _ in rows if m == 7) > 128, "several tiles of 64 rows, a molecule whose rows cross tile boundaries"
    assert (7, 1 << 63) in rows and (7, FULL64 ^ (1 << 63)) in rows and (3, 0) in rows
    bit_d, row_mol_d, mask_d = _dev(bit, np.int8), _dev([m for m, _ in rows], np.int32), _masks([k for _, k in rows])
    plain = ops.pool_cat(xa, xf, plan)
    # expected rows: fn_pool_cat_f32 of the table with the left-out atom rows overwritten by 0.0
    want = torch.empty(R, 256, device=DEV)
    for r, (m, k) in enumerate(rows):
        out_of = (batch == m) & np.array([b >= 0 and not (k >> int(b)) & 1 for b in bit])
        xz = xa.clone()
        xz[torch.from_numpy(out_of).to(DEV)] = 0.0
        want[r] = ops.pool_cat(xz, xf, plan)[m]
    results = {}
    try:
        for name, form in FORMS.items():
            _lib.call("fn_set_tuning", KEY, form)
            out = torch.full((R + 3, 256), 7.0, device=DEV)          # three sentinel rows behind the result
            assert _call(lib, xa, xf, plan, bit_d, row_mol_d, mask_d, R, out) == 0
            torch.cuda.synchronize()
            assert bool((out[R:] == 7.0).all()), f"{name}: rows behind the result were written"
            results[name] = out[:R]
            bad = [rows[r] for r in range(R) if not torch.equal(out[r], want[r])]
            assert not bad, f"{name}: {len(bad)} rows differ from fn_pool_cat_f32 of the zeroed table, first (molecule, mask) {bad[0]}"
    finally:
        _lib.call("fn_set_tuning", KEY, 1)
    assert all(torch.equal(results[name], results["rows"]) for name in FORMS), "the forms against each other"
    out = ops.pool_cat_coalitions(xa, xf, plan, bit_d, row_mol_d, mask_d)          # the default form through ops
    assert out.shape == (R, 256) and not out.requires_grad and torch.equal(out, want)
    # against the two older read-outs, row by row
    group_d = _dev(bit, np.int64)
    for r, (m, k) in enumerate(rows):
        F = GROUPS[m]
        full = (1 << F) - 1
        assert torch.equal(out[r, 128:], plain[m, 128:]), "the fragments' half is never masked"
        if k == full:
            assert torch.equal(out[r], plain[m]), f"molecule {m}: the full row is not fn_pool_cat_f32's"
        elif F and bin(full ^ k).count("1") == 1:
            left = (full ^ k).bit_length() - 1
            loo = ops.pool_cat_groups(xa, xf, plan, group_d, _dev([m], np.int32), _dev([left], np.int64))
            assert torch.equal(out[r], loo[0]), f"molecule {m}: all-but-{left} is not fn_pool_cat_groups_f32's row"
    empty_of = {m: out[rows.index((m, 0))] for m in range(len(ATOMS))}
    assert bool((empty_of[3][:128] == 0.0).all()) and bool((empty_of[1][:128] == 0.0).all()), "mask 0 with every atom grouped: exactly 0.0"
    assert bool((empty_of[0] == 0.0).all()), "a molecule without atoms and fragments"
    assert bool((empty_of[6][:128] != 0.0).any()), "ungrouped atoms are in the empty coalition"
    only63 = out[rows.index((7, 1 << 63))]
    assert not torch.equal(only63, empty_of[7]) and not torch.equal(only63, plain[7])
    # R == 0
    none = ops.pool_cat_coalitions(xa, xf, plan, bit_d, torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    assert none.shape == (0, 256) and none.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ b. refusals
def test_refusals_leave_the_output_untouched():
    from fragnet_amd import _lib, ops
    from fragnet_amd.plan import _stream_ptr
    batch, bit, plan, xa, xf, rows = _read_out_inputs()
    lib = _lib.load()
    bit_d, row_mol_d, mask_d = _dev(bit, np.int8), _dev([1, 2], np.int32), _masks([1, 3])
    out = torch.full((2, 256), 7.0, device=DEV)
    a, f = ops._seg_struct(plan.segs["mol_atoms"]), ops._seg_struct(plan.segs["mol_frags"])
    short = ops._seg_struct(plan.segs["mol_frags"])
    short.n_seg -= 1
    no_rowptr = ops._seg_struct(plan.segs["mol_atoms"])
    no_rowptr.rowptr = None
    none_a, none_f = ops._seg_struct(plan.segs["mol_atoms"]), ops._seg_struct(plan.segs["mol_frags"])
    none_a.n_seg = none_f.n_seg = 0          # a batch without molecules
    st = _stream_ptr(xa.device)
    good = dict(xa=xa.data_ptr(), xf=xf.data_ptr(), a=C.byref(a), f=C.byref(f), ab=bit_d.data_ptr(), rm=row_mol_d.data_ptr(),
                mk=mask_d.data_ptr(), R=2, out=out.data_ptr())
    run = lambda k: lib.fn_pool_cat_coalitions_f32(k["xa"], k["xf"], k["a"], k["f"], k["ab"], k["rm"], k["mk"], k["R"], k["out"], st)
    for change in (dict(a=None), dict(f=None), dict(f=C.byref(short)), dict(R=-1), dict(rm=None), dict(mk=None), dict(ab=None), dict(xa=None),
                   dict(xf=None), dict(out=None), dict(a=C.byref(no_rowptr)), dict(a=C.byref(none_a), f=C.byref(none_f))):
        assert run({**good, **change}) == _lib.FN_EINVAL, change
        assert b"fn_pool_cat_coalitions_f32" in lib.fn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert lib.fn_pool_cat_coalitions_f32(None, None, C.byref(a), C.byref(f), None, None, None, 0, None, st) == 0          # R == 0: nothing to do
    assert run(good) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    # ops: rows and bits are validated on the host
    one = lambda v, t: _dev([v], t)
    for bad in (len(ATOMS), -1):
        with pytest.raises(IndexError, match="row_mol"):
            ops.pool_cat_coalitions(xa, xf, plan, bit_d, one(bad, np.int32), one(0, np.int64))
    with pytest.raises(ValueError, match="non-decreasing"):
        ops.pool_cat_coalitions(xa, xf, plan, bit_d, _dev([2, 1], np.int32), _dev([0, 0], np.int64))
    too_wide = bit.copy()
    too_wide[5] = 64
    with pytest.raises(IndexError, match="atom_bit"):
        ops.pool_cat_coalitions(xa, xf, plan, _dev(too_wide, np.int8), one(0, np.int32), one(0, np.int64))
    with pytest.raises(ValueError, match="row_mol"):
        ops.pool_cat_coalitions(xa, xf, plan, bit_d, one(0, np.int64), one(0, np.int64))
    with pytest.raises(ValueError, match="row_mask"):
        ops.pool_cat_coalitions(xa, xf, plan, bit_d, one(0, np.int32), _dev([0, 0], np.int64))
    with pytest.raises(ValueError, match="atom_bit"):
        ops.pool_cat_coalitions(xa, xf, plan, _dev(bit, np.int64), one(0, np.int32), one(0, np.int64))
    with pytest.raises(ValueError, match="feature tables"):
        ops.pool_cat_coalitions(xa[:-1], xf, plan, bit_d, one(0, np.int32), one(0, np.int64))


# ------------------------------------------------------------------------------------------------ c. the reference fixture
_RESULTS = {}          # case -> (result, model, molecules): computed once, shared


def _shared(case):
    if case not in _RESULTS:
        from fragnet_amd import attribution as attr
        model = fc.build(case, DEV)
        mols = fc.molecules(case)
        _RESULTS[case] = (attr.fragment_shapley(model, mols, groups=fc.groups(case, mols), return_values=True), model, mols)
    return _RESULTS[case]


def _efficiency(res):
    """max over molecules and classes of |sum_f phi_f - (pred - base)| - 1e-9 max(1, max |v|): float64 round-off of at most 5 120 terms."""
    worst = -np.inf
    for i in range(len(res)):
        m = res[i]
        gap = np.abs(m["phi"].sum(axis=0) - (m["pred"].astype(np.float64) - m["base"].astype(np.float64))).max()
        scale = max(1.0, float(np.abs(res.values[i]["value"]).max())) if res.values is not None else max(1.0, float(np.abs(m["pred"]).max()), float(np.abs(m["base"]).max()))
        worst = max(worst, gap - 1e-9 * scale)
    return worst


@pytest.mark.parametrize("case", sc.CASES)
def test_values_and_shapley_values_match_the_reference_fixture(case):
    mask, value, phi, groups = sc.reference(case)
    res, _, mols = _shared(case)
    assert len(res) == len(mols) and np.diff(res.offsets).tolist() == groups and res.exact.all() and not res.stderr.any()
    got_mask = np.concatenate([np.stack([np.full(v["mask"].shape[0], i, dtype=np.int64), v["mask"].astype(np.int64)], 1) for i, v in enumerate(res.values)])
    np.testing.assert_array_equal(got_mask, mask)
    got = np.concatenate([v["value"] for v in res.values])
    print(f"{case}: max |value - ref| {np.abs(got - value).max():.3e}, max |phi - ref| {np.abs(res.phi - phi).max():.3e}, max |phi| {np.abs(phi).max():.3f}")
    fc.close(got, value, f"{case}: values")
    fc.close(res.phi, phi, f"{case}: phi", scale=2.0)
    assert res.phi.dtype == np.float64 and _efficiency(res) <= 0.0
    for i, v in enumerate(res.values):
        np.testing.assert_array_equal(res.pred[i], v["value"][-1])
        np.testing.assert_array_equal(res.base[i], v["value"][0])
    ids = [np.unique(g[g >= 0]) for g in fc.atom_groups(case, mols)]
    np.testing.assert_array_equal(res.group, np.concatenate(ids))
    w = res.atom_weights(0)
    g0 = fc.atom_groups(case, mols)[0]
    assert w.shape == (g0.shape[0], phi.shape[1]) and bool((w[g0 < 0] == 0).all())
    np.testing.assert_array_equal(w[g0 == res[0]["group"][0]], np.repeat(res[0]["phi"][:1], int((g0 == res[0]["group"][0]).sum()), 0))


# ------------------------------------------------------------------------------------------------ d. the literal path on the GPU
@pytest.mark.parametrize("name,ctor,profile,seed", [("gat2_lite", dict(ac.CTOR, variant="gat2_lite"), "esol", 11),
                                                     ("tox21-12", dict(ac.CTOR, n_classes=12), "tox21", 7)])
def test_the_literal_models_on_replicated_records_agree(name, ctor, profile, seed):
    """The drop-in classes with apply_mask=True, run literally: one record per evaluated coalition, atom_mask = 1 on the atoms of the
    groups outside it, one encoder pass per record."""
    from fragnet_amd import attr_model, attribution as attr, data
    from fragnet_amd.dataset import FlatMolStore
    torch.manual_seed(seed)
    model = attr_model.FragNetFineTune(**ctor, apply_mask=True)
    ac.scale_model(model)
    model = model.to(DEV).eval()
    mols = ac.molecules(4, seed=4300, profile=profile)
    res = attr.fragment_shapley(model, FlatMolStore.from_records(mols).to(DEV), exact_max=6, samples=4, return_values=True)
    recs = []
    for i, m in enumerate(mols):
        g = m.atom_id_frag_id.numpy().astype(np.int64)
        ids = np.unique(g)
        for k in res.values[i]["mask"].tolist():
            rec = copy.copy(m)
            rec.atom_mask = torch.from_numpy(np.isin(g, [gid for p, gid in enumerate(ids.tolist()) if not (k >> p) & 1]).astype(np.int32))
            recs.append(rec)
    assert 16 <= len(recs) <= 1024
    with torch.no_grad():
        literal = torch.cat([model(data.batch_to(attr_model.collate_fn(recs[lo: lo + 256]), DEV)).reshape(len(recs[lo: lo + 256]), -1).float()
                             for lo in range(0, len(recs), 256)]).cpu().numpy()
    got = np.concatenate([v["value"] for v in res.values])
    assert got.shape == (len(recs), ctor["n_classes"])
    fc.close(got, literal, f"{name}: values against the literal path")
    assert _efficiency(res) <= 0.0
    spread = np.concatenate([np.abs(v["value"] - v["value"][1 if not res.exact[i] else -1]).max(axis=1) for i, v in enumerate(res.values)])
    assert (spread > 10 * (ac.ATOL + ac.RTOL * np.abs(got).max())).mean() >= 0.5, "the masks do not matter for this model"


# ------------------------------------------------------------------------------------------------ e. modes and degenerate molecules
def test_sampling_with_all_permutations_equals_exact_mode():
    from fragnet_amd import attribution as attr
    exact, model, mols = _shared("property")
    pick = [i for i in range(len(mols)) if int(np.diff(exact.offsets)[i]) in (2, 4)]          # F = 4, 4, 2, 4
    assert [int(np.diff(exact.offsets)[i]) for i in pick] == [4, 4, 2, 4]
    every = {j: np.array(list(itertools.permutations(range(4)))) for j, i in enumerate(pick) if int(np.diff(exact.offsets)[i]) == 4}
    res = attr.fragment_shapley(model, [mols[i] for i in pick], exact_max=2, permutations=every, return_values=True)
    assert res.exact.tolist() == [False, False, True, False]
    assert [v["mask"].shape[0] for v in res.values] == [2 + 24 * 3, 2 + 24 * 3, 4, 2 + 24 * 3]
    want = np.concatenate([exact[i]["phi"] for i in pick])
    fc.close(res.phi, want, "phi, all 24 permutations against the enumeration", scale=2.0)
    assert _efficiency(res) <= 0.0
    # F = 3 (custom groups), every molecule sampled
    exact3, model3, mols3 = _shared("property_groups")
    every3 = {i: np.array(list(itertools.permutations(range(3)))) for i in range(len(mols3))}
    res3 = attr.fragment_shapley(model3, mols3, groups=fc.groups("property_groups", mols3), exact_max=2, permutations=every3)
    assert not res3.exact.any()
    fc.close(res3.phi, exact3.phi, "phi, all 6 permutations against the enumeration (F = 3)", scale=2.0)
    # the default draw on F = 3: efficient whatever the sample
    drawn = attr.fragment_shapley(model3, mols3, groups=fc.groups("property_groups", mols3), exact_max=2, samples=4, seed=1)
    assert not drawn.exact.any() and _efficiency(drawn) <= 0.0 and np.isfinite(drawn.stderr).all()


def test_degenerate_molecules():
    from fragnet_amd import attribution as attr
    _, model, mols = _shared("property")
    mols = mols[:3]
    n = [int(m.x_atoms.shape[0]) for m in mols]
    groups = [np.full(n[0], -1, dtype=np.int64), np.full(n[1], 5, dtype=np.int64), np.arange(n[2], dtype=np.int64) % 2]
    res = attr.fragment_shapley(model, mols, groups=groups, return_values=True)
    assert res.offsets.tolist() == [0, 0, 1, 3] and res.group.tolist() == [5, 0, 1] and res.exact.all()
    assert res[0]["phi"].shape == (0, 1) and res.atom_weights(0).shape == (n[0], 1) and not res.atom_weights(0).any()
    np.testing.assert_array_equal(res.pred[0], res.base[0])          # nothing to leave out: one row
    assert res.values[0]["mask"].tolist() == [0]
    np.testing.assert_array_equal(res[1]["phi"][0], res.pred[1].astype(np.float64) - res.base[1].astype(np.float64))          # one group: phi = pred - base
    fc.close(res.pred, sc.reference("property")[1][[63, 79, 95]], "pred against the reference's full rows")


# ------------------------------------------------------------------------------------------------ f. the pair models
@pytest.mark.parametrize("case", ["drp", "dta"])
def test_pair_models_are_additive_and_answer_from_one_pass(case):
    from fragnet_amd import attribution as attr
    model = fc.build(case, DEV)
    mols = fc.molecules(case)
    res = attr.fragment_shapley(model, mols, return_values=True)
    loo = attr.fragment_contributions(model, mols)
    counts = np.diff(res.offsets)
    assert res.exact.all() and [v["mask"].shape[0] for v in res.values] == (counts + 2).tolist()
    np.testing.assert_array_equal(res.offsets, loo.offsets)
    np.testing.assert_array_equal(res.group, loo.group)
    fc.close(res.pred, loo.pred_no_mask, f"{case}: pred")
    fc.close(res.phi, loo.attr, f"{case}: phi against the leave-one-out contributions")
    for i in range(len(res)):          # the additivity the shortcut claims: the leave-one-out values add up to pred - base
        m = res[i]
        gap = np.abs(m["phi"].sum(axis=0) - (m["pred"].astype(np.float64) - m["base"]))
        tol = 2 * max(int(counts[i]), 1) * (ac.ATOL + ac.RTOL * np.maximum(np.abs(m["pred"]), np.abs(m["base"])))
        print(f"{case} molecule {i}: F {int(counts[i])}, efficiency gap {gap.max():.3e}, bound {tol.min():.3e}")
        assert (gap <= tol).all(), (case, i, gap, tol)


# ------------------------------------------------------------------------------------------------ g. launches per chunk
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


def test_one_encoder_pass_one_read_out_per_chunk_and_bounded_head_slices(monkeypatch):
    from fragnet_amd import _lib, attribution as attr, ops
    from fragnet_amd.dataset import FlatMolStore
    model = fc.build("property", DEV)
    store = FlatMolStore.from_records(fc.molecules("property")).to(DEV)
    proxy = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    head_rows = []
    hook = model.fthead.register_forward_pre_hook(lambda mod, args: head_rows.append(int(args[0].shape[0])))
    try:
        model.train()
        one = attr.fragment_shapley(model, store)
        assert model.training, "the training flag is restored"
        calls = list(proxy.calls)
        assert calls.count("fn_encoder_forward") == 1 and calls.count("fn_pool_cat_coalitions_f32") == 1
        assert "fn_encoder_forward_masked" not in calls and "fn_pool_cat_f32" not in calls and "fn_pool_cat_groups_f32" not in calls
        assert head_rows == [372]
        proxy.calls.clear()
        head_rows.clear()
        monkeypatch.setattr(ops, "DENSE_MAX_ROWS", 100)
        two = attr.fragment_shapley(model.eval(), store, max_rows=256)          # 64 + 16 + 16 | 256 | 4 + 16 rows
        calls = list(proxy.calls)
        assert calls.count("fn_encoder_forward") == 3 and calls.count("fn_pool_cat_coalitions_f32") == 3
        assert head_rows == [96, 100, 100, 56, 20]
    finally:
        hook.remove()
    np.testing.assert_array_equal(two.offsets, one.offsets)
    fc.close(two.phi, one.phi, "phi, three chunks against one", scale=2.0)
    fc.close(one.phi, sc.reference("property")[2], "phi (a FlatMolStore source) against the reference", scale=2.0)
    with pytest.raises(ValueError, match="molecule 3 alone needs 256"):
        attr.fragment_shapley(model, store, max_rows=255)


# ------------------------------------------------------------------------------------------------ h. the script
def test_script_writes_the_arrays_fragment_shapley_returns(tmp_path):
    from fragnet_amd import attribution as attr, synth, train
    from fragnet_amd.dataset import FlatMolStore
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import attribute_fragments_shapley_gat2 as mod
    finally:
        sys.path.pop(0)
    config = os.path.join(ROOT, "exps", "ft", "esol_synth", "config.yaml")
    FlatMolStore.from_records(synth.synth_molecules(24, seed=2, profile="esol")).save(str(tmp_path / "test.pt"))
    torch.manual_seed(11)
    model = mod.build_model(train.load_config(config, config=config), "property")
    torch.save(model.state_dict(), str(tmp_path / "model.pt"))
    out = str(tmp_path / "shap.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "attribute_fragments_shapley_gat2.py"), "--config", config, "--checkpoint",
                        str(tmp_path / "model.pt"), "--data", str(tmp_path / "test.pt"), "--out", out, "--prop-type", "property", "--batch-size", "16",
                        "--exact-max", "4", "--samples", "8", "--seed", "3", "--max-rows", "4096"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = attr.fragment_shapley(model.to(DEV), FlatMolStore.load(str(tmp_path / "test.pt"), device=DEV), batch_size=16, exact_max=4, samples=8, seed=3,
                                max_rows=4096)
    assert f"24 molecules, {int(res.offsets[-1])} fragments, {int(res.exact.sum())} molecules exact -> {out}" in r.stdout
    assert 0 < int(res.exact.sum()) < 24, "both modes ran"
    z = np.load(out)
    want = res.arrays()
    assert sorted(z.files) == sorted(want)
    for k in ("offsets", "group", "n_atoms", "atom_group", "atom_offsets", "exact"):
        np.testing.assert_array_equal(z[k], want[k])
    fc.close(z["pred"], want["pred"], "pred")
    fc.close(z["base"], want["base"], "base")
    fc.close(z["phi"], want["phi"], "phi", scale=2.0)
    np.testing.assert_allclose(np.add.reduceat(z["phi"], z["offsets"][:-1][np.diff(z["offsets"]) > 0], axis=0),
                               (z["pred"].astype(np.float64) - z["base"])[np.diff(z["offsets"]) > 0], rtol=0, atol=1e-9 * max(1.0, float(np.abs(z["pred"]).max())))
