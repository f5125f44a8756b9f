"""Row masks as a per-batch input of the engine's evaluation pass (fn_encoder_forward_masked, fn_loo_row_masks_u8) and the batched
leave-one-out attribution built on them (fragnet_amd/attribution.py, scripts/attribute_gat2.py).

Expected values: the oracle (oracle/fragnet_ref.py) run on the CPU, one molecule and one scalar mask on every layer at a time -- the
reference's own form of it -- and the reference's fixture tests/golden/attr_loo_b6.npz.  Tolerances are the project's:
|got - ref| <= 1e-4 + 1e-4 |ref| for encoder outputs and predictions, twice that for a difference of two predictions.

The inputs make the masks matter (asserted below on the ORACLE's values, never on the code under test): with freshly initialised
weights most scalar attributions lie below the logit tolerance, so the encoder outputs are compared directly (test 1), and the
end-to-end checks use a model whose last Linear is x 100 and whose attention vectors are x 4 (tests/attr_common.py).
Measured on the CPU for that model and synth.synth_molecules(6, seed=4100, profile="esol") (190 atom, 187 bond, 22 fragment-bond
replicas): share of attributions above 10 x their tolerance: atoms 0.94, bonds 0.75, fragment bonds 0.45."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attr_common as ac
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _pair(scaled, ctor=ac.CTOR, seed=ac.SEED):
    """(oracle on the CPU, this project's model on the GPU) with the same weights."""
    from fragnet_amd import model as M
    from oracle import fragnet_ref as R
    gold = ac.build(R, ctor, seed, scaled=scaled)
    net = M.FragNetFineTune(**ctor)
    net.load_state_dict(gold.state_dict())
    return gold, net.to(DEV).eval()


def _store(mols):
    from fragnet_amd.dataset import FlatMolStore
    return FlatMolStore.from_records(mols).to(DEV)


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref) - (ac.ATOL + ac.RTOL * np.abs(ref))
    assert got.shape == ref.shape and (err <= 0).all(), f"{what}: worst excess over the tolerance {err.max():.3e}"


def _replica_batches(store, max_rows):
    """[(batch with masks, [(molecule, kind, reported index)])] for every replica of the store, in chunks."""
    from fragnet_amd import attribution as attr
    from fragnet_amd.model import MASK_KEYS
    lens = store._host_lengths()
    table = attr.replica_table(lens["atom"], lens["edge"], lens["fedge"])
    chunks = attr.plan_chunks(lens["atom"] + lens["edge"], [t.shape[0] for t in table], max_rows)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = []
    for chunk in chunks:
        mols = np.concatenate([np.full(r1 - r0, i) for i, r0, r1 in chunk])
        reps = np.concatenate([table[i][r0:r1] for i, r0, r1 in chunk], 0)
        batch = store.collate(mols)
        masks = attr.build_row_masks(batch, torch.from_numpy(attr.local_index(reps)).to(DEV), status)
        for key, m in zip(MASK_KEYS, masks):
            batch[key] = m
        out.append((batch, [(int(i), ("atom", "bond", "fbond")[k - 1], int(x)) for i, (k, x) in zip(mols, reps)]))
    assert int(status.item()) == 0
    return out


_ORACLE_OUTPUTS = {}          # (molecule, kind, index) -> the oracle's four encoder outputs: computed once, shared by the cases below


@pytest.mark.parametrize("fuse_rowdots,colaunch", [(1, 2), (1, 0), (0, 2), (0, 0)], ids=["default", "no-colaunch", "no-fused-rowdots", "neither"])
def test_masked_encoder_outputs_match_the_oracle_with_scalar_masks(fuse_rowdots, colaunch):
    """Test 1 of the issue: every replica's four encoder outputs against the oracle on that molecule alone with that scalar mask
    on every layer; the masked element's own rows are exactly 0.0.  Condition on the inputs (oracle values), taken on the two
    outputs a finetune head pools (out_atoms, out_frags): every atom and bond replica moves one of them by >= 10 x tolerance;
    every fragment-bond replica too, except exact no-ops -- both outputs identical to the unmasked ones: the only connection of
    a two-fragment molecule is each fragment's single in-edge, and a softmax over one edge is 1 whatever its term -- at most 1 in
    10 of them.  Measured: minimum over atoms 1040 x, bonds 65 x, fragment bonds 13 x tolerance; 1 of 22 fragment-bond replicas is
    a no-op (its own out_fbond rows still go to zero, which the comparison above checks).
    The cases: the masked pass on the default launches (the two bond levels with the atom projection riding, the row dots in the bond
    level's epilogue, the atom level with the next layer's projections riding) and on the plain launchers it falls back to --
    FN_TUNE_GEMM_COLAUNCH (14) = 0: the masked two-level launch and the masked atom level without riders; FN_TUNE_FUSE_ROWDOTS (7) = 0:
    the bond level without the epilogue and the separate row-dots launch behind a masked level.  Same batch, same tolerances; and the
    same bytes as the default launches: that equality was seen to hold on the commit before these cases existed, for all three."""
    from fragnet_amd import _lib, data
    from fragnet_amd.plan import SPACES
    torch.set_num_threads(8)
    gold, net = _pair(scaled=False)
    mols = ac.molecules()
    ref_cache = _ORACLE_OUTPUTS

    def oracle(i, kind, index):
        key = (i, kind, index)
        if key not in ref_cache:
            b = data.collate_fn([mols[i]])
            if kind is not None:
                ac.set_mask(gold, kind, index)
            try:
                with torch.no_grad():
                    ref_cache[key] = [t.clone().numpy() for t in gold.pretrain(b)]
            finally:
                if kind is not None:
                    ac.set_mask(gold, kind, None)
        return ref_cache[key]

    batches = _replica_batches(_store(mols), max_rows=15000)
    assert 2 <= len(batches) <= 3
    moved = {"atom": [], "bond": [], "fbond": []}
    seen = 0

    def encoder(batch, key7, key14):
        try:
            _lib.call("fn_set_tuning", 7, key7)
            _lib.call("fn_set_tuning", 14, key14)
            with torch.no_grad():
                return [t.cpu().numpy() for t in net.pretrain(batch, edge_outputs=True)]
        finally:
            _lib.call("fn_set_tuning", 7, 1)
            _lib.call("fn_set_tuning", 14, 2)

    for batch, reps in batches:
        outs = encoder(batch, fuse_rowdots, colaunch)
        if (fuse_rowdots, colaunch) != (1, 2):
            for name, o, d in zip(("out_atoms", "out_frags", "out_bond", "out_fbond"), outs, encoder(batch, 1, 2)):
                assert np.array_equal(o, d), f"{name} differs from the default launches' bytes"
        off = batch.offsets.cpu().numpy()
        rows = [off[SPACES.index(s)] for s in ("atom", "frag", "edge", "fedge")]
        for r, (i, kind, index) in enumerate(reps):
            ref = oracle(i, kind, index)
            base = oracle(i, None, None)
            got = [o[sp[r]: sp[r + 1]] for o, sp in zip(outs, rows)]
            for name, g, w in zip(("out_atoms", "out_frags", "out_bond", "out_fbond"), got, ref):
                _close(g, w, f"molecule {i} {kind} {index} {name}")
            own = {"atom": got[0][index: index + 1], "bond": got[2][index: index + 2], "fbond": got[3][2 * index: 2 * index + 2]}[kind]
            assert own.size and (own == 0.0).all(), f"molecule {i} {kind} {index}: the masked rows are not exactly zero"
            ratio = max(float((np.abs(w - b0) / (ac.ATOL + ac.RTOL * np.abs(b0))).max()) for w, b0 in zip(ref[:2], base[:2]))
            same = all(np.array_equal(w, b0) for w, b0 in zip(ref[:2], base[:2]))
            moved[kind].append((ratio, same))
            seen += 1
    assert seen == 399 and {k: len(v) for k, v in moved.items()} == {"atom": 190, "bond": 187, "fbond": 22}
    assert all(r >= 10 for r, _ in moved["atom"]) and all(r >= 10 for r, _ in moved["bond"]), "the inputs do not make the masks matter"
    noop = [same for _, same in moved["fbond"]]
    assert all(r >= 10 for r, same in moved["fbond"] if not same) and sum(noop) * 10 <= len(noop)


def _check_against(res, recs, what, min_share=True):
    """leave_one_out's result against per-molecule records {"pred_no_mask", kind: {"index", "pred_mask"}}; returns nothing.
    The condition on the expected values: at least half of all attributions, and a quarter within each kind, exceed 10 x tolerance."""
    big = {k: [] for k in ac.MASK_ATTR}
    assert len(res) == len(recs)
    for i, rec in enumerate(recs):
        got = res[i]
        base = np.asarray(rec["pred_no_mask"], dtype=np.float64).reshape(-1)
        _close(got["pred_no_mask"], base, f"{what}: molecule {i} pred_no_mask")
        tol = ac.attr_tolerance(base)[None, :]
        for kind in ac.MASK_ATTR:
            np.testing.assert_array_equal(got[kind]["index"], rec[kind]["index"])
            want_pm = np.asarray(rec[kind]["pred_mask"], dtype=np.float64).reshape(len(rec[kind]["index"]), base.size)
            _close(got[kind]["pred_mask"], want_pm, f"{what}: molecule {i} {kind} pred_mask")
            want = base[None, :] - want_pm
            err = np.abs(got[kind]["attr"].astype(np.float64) - want) - tol
            assert got[kind]["attr"].shape == want.shape and (err <= 0).all(), f"{what}: molecule {i} {kind} attr off by {err.max():.3e} over the tolerance"
            big[kind] += list((np.abs(want) > 10 * tol).reshape(-1))
    if min_share:
        shares = {k: float(np.mean(v)) for k, v in big.items()}
        assert all(s >= 0.25 for s in shares.values()) and float(np.mean(sum(big.values(), []))) >= 0.5, shares


def test_leave_one_out_matches_the_oracle_end_to_end():
    """Test 2: the scaled model, leave_one_out against the oracle's pred_no_mask - pred_mask, each held to 2 (1e-4 + 1e-4 |pred_no_mask|)."""
    from fragnet_amd import attribution as attr, data
    torch.set_num_threads(8)
    gold, net = _pair(scaled=True)
    mols = ac.molecules()
    res = attr.leave_one_out(net, mols, max_rows=15000)
    _check_against(res, ac.scalar_loo(gold, mols, data.collate_fn), "oracle")
    empty = [i for i in range(len(res)) if len(res[i]["fbond"]["index"]) == 0]
    for i in empty:
        assert res[i]["fbond"]["attr"].shape == (0, 1)


def test_leave_one_out_matches_the_reference_fixture():
    """Test 3: the same against the reference's own numbers (tests/golden/attr_loo_b6.npz)."""
    from fragnet_amd import attribution as attr
    z = np.load(os.path.join(GOLDEN, "attr_loo_b6.npz"))
    cfg = json.loads(str(z["cfg"]))
    _, net = _pair(scaled=True, ctor={k: v for k, v in cfg["ctor"].items()}, seed=cfg["seed"])
    mols = ac.molecules(cfg["n_mols"], cfg["mol_seed"], cfg["profile"])
    recs = [{"pred_no_mask": z[f"m{i}/pred_no_mask"], **{k: {"index": z[f"m{i}/{k}_index"], "pred_mask": z[f"m{i}/{k}_pred_mask"]} for k in ac.MASK_ATTR}}
            for i in range(cfg["n_mols"])]
    _check_against(attr.leave_one_out(net, _store(mols)), recs, "reference fixture")


def test_chunked_and_one_chunk_runs_agree():
    from fragnet_amd import attribution as attr
    _, net = _pair(scaled=True)
    store = _store(ac.molecules())
    one, many = attr.leave_one_out(net, store, max_rows=10 ** 9), attr.leave_one_out(net, store, max_rows=2000)
    lens = store._host_lengths()
    counts = [t.shape[0] for t in attr.replica_table(lens["atom"], lens["edge"], lens["fedge"])]
    assert len(attr.plan_chunks(lens["atom"] + lens["edge"], counts, 10 ** 9)) == 1 and len(attr.plan_chunks(lens["atom"] + lens["edge"], counts, 2000)) > 6
    for i in range(len(one)):
        for kind in ac.MASK_ATTR:
            _close(many[i][kind]["pred_mask"], one[i][kind]["pred_mask"], f"molecule {i} {kind}")


def test_multi_task_head_against_the_oracle():
    """n_classes = 12 on Tox21-profile molecules: one attribution column per task."""
    from fragnet_amd import attribution as attr, data
    torch.set_num_threads(8)
    ctor = dict(ac.CTOR, n_classes=12)
    gold, net = _pair(scaled=True, ctor=ctor, seed=7)
    mols = ac.molecules(3, seed=4300, profile="tox21")
    res = attr.leave_one_out(net, mols, kinds=("fbond", "atom", "bond"))
    assert res.pred_no_mask.shape == (3, 12)
    _check_against(res, ac.scalar_loo(gold, mols, data.collate_fn), "tox21", min_share=False)


@pytest.mark.parametrize("fthead,act", [("FTHead1", "relu"), ("FTHead2", "relu"), ("FTHead4", "gelu"), ("FTHead3", "celu")])
def test_every_head_runs_masked_batches(fthead, act):
    from fragnet_amd import attribution as attr, data
    torch.set_num_threads(8)
    ctor = dict(ac.CTOR, fthead=fthead, act=act)
    gold, net = _pair(scaled=True, ctor=ctor, seed=9)
    mols = ac.molecules(2, seed=4400)
    _check_against(attr.leave_one_out(net, mols), ac.scalar_loo(gold, mols, data.collate_fn), fthead, min_share=False)


# ------------------------------------------------------------------------------------------------ bit-identity, refusals, status
def _encoder(net, batch, **kw):
    batch.pop("_fragnet_plan", None)
    with torch.no_grad():
        outs = net.pretrain(batch, edge_outputs=True, **kw)
    torch.cuda.synchronize()
    return [t.clone() for t in outs]


def test_zero_masks_absent_masks_and_the_plain_entry_point_return_the_same_bytes():
    from fragnet_amd import data, engine
    from fragnet_amd.model import MASK_KEYS
    _, net = _pair(scaled=False)
    batch = data.batch_to(data.collate_fn(ac.molecules(48, seed=77)), DEV)
    plain = _encoder(net, batch)
    absent = _encoder(net, batch.like({**batch, **{k: None for k in MASK_KEYS}}))
    sizes = (batch["x_atoms"].shape[0], batch["node_features_bonds"].shape[0], batch["node_features_fbonds"].shape[0])
    zeros = _encoder(net, batch.like({**batch, **{k: torch.zeros(n, dtype=torch.uint8, device=DEV) for k, n in zip(MASK_KEYS, sizes)}}))
    only_atoms = _encoder(net, batch.like({**batch, MASK_KEYS[0]: torch.zeros(sizes[0], dtype=torch.uint8, device=DEV)}))
    # fn_encoder_forward_masked with three NULL arrays: the plain pass inside the library
    calls = []
    real = engine._row_mask
    try:
        engine._row_mask = lambda t, n, name: calls.append(name)          # hands the library NULL for every array
        b = batch.like({**batch, MASK_KEYS[0]: torch.zeros(sizes[0], dtype=torch.uint8, device=DEV)})
        null3 = _encoder(net, b)
    finally:
        engine._row_mask = real
    assert calls == list(MASK_KEYS)
    for name, outs in (("absent", absent), ("all-zero", zeros), ("zero atom mask only", only_atoms), ("three NULL arrays", null3)):
        for k, (a, b) in enumerate(zip(plain, outs)):
            assert torch.equal(a, b), f"{name}: output {k} differs from fn_encoder_forward"


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


@pytest.fixture
def counting(monkeypatch):
    from fragnet_amd import _lib
    proxy = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    return proxy


def _masked_batch(n=12, seed=78):
    from fragnet_amd import attribution as attr, data
    from fragnet_amd.model import MASK_KEYS
    from fragnet_amd.plan import SPACES
    batch = data.batch_to(data.collate_fn(ac.molecules(n, seed=seed)), DEV)
    n_fb = np.diff(batch.offsets.cpu().numpy()[SPACES.index("fedge")])
    kinds = [1 + i % 3 if (i % 3 < 2 or n_fb[i] >= 2) else 1 for i in range(n)]           # a single-fragment molecule has no connection to mask
    assert set(kinds) == {1, 2, 3}
    reps = torch.tensor([[k, 0] for k in kinds], dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    masks = attr.build_row_masks(batch, reps, status)
    assert int(status.item()) == 0
    return batch, batch.like({**batch, **dict(zip(MASK_KEYS, masks))}), reps


def test_a_masked_batch_is_the_engine_plus_one_mask_launch(counting, monkeypatch):
    """Test 5: the C calls of a masked model(batch) are those of an unmasked evaluation batch, with fn_encoder_forward_masked in
    fn_encoder_forward's place, plus the one mask launch; nothing of the per-level path runs."""
    from fragnet_amd import attribution as attr, ops
    _, net = _pair(scaled=False)
    batch, _, reps = _masked_batch()
    for name in ("gat_level", "row_dots_sorted"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the per-level path ran"))
    counting.calls.clear()
    with torch.no_grad():
        batch.pop("_fragnet_plan", None)
        net(batch)
    plain = list(counting.calls)
    assert plain.count("fn_encoder_forward") == 1
    counting.calls.clear()
    with torch.no_grad():
        batch.pop("_fragnet_plan", None)
        masks = attr.build_row_masks(batch, reps, torch.zeros(1, dtype=torch.int32, device=DEV))
        net(batch.like({**batch, "mask_atoms": masks[0], "mask_bonds": masks[1], "mask_fbonds": masks[2]}))
    masked = list(counting.calls)
    assert masked[0] == "fn_loo_row_masks_u8" and masked.count("fn_loo_row_masks_u8") == 1
    assert ["fn_encoder_forward" if c == "fn_encoder_forward_masked" else c for c in masked[1:]] == plain
    assert masked.count("fn_encoder_forward_masked") == 1 and "fn_encoder_forward" not in masked


def test_masked_passes_that_cannot_run_are_refused_before_the_library_is_called(counting):
    from fragnet_amd import model as M
    _, net = _pair(scaled=False)
    _, mb, _ = _masked_batch()
    counting.calls.clear()
    net.train()
    with pytest.raises(RuntimeError, match="evaluation"):
        net.pretrain(mb)
    net.eval()
    with pytest.raises(RuntimeError, match="no backward"):          # parameters require gradients and grad mode is on
        net.pretrain(mb)
    for variant in ("gat2_lite", "gat2_edge"):
        other = M.FragNetFineTune(**dict(ac.CTOR, variant=variant)).to(DEV).eval()
        with torch.no_grad(), pytest.raises(ValueError, match="gat2"):
            other(mb)
    net.pretrain.layers[0].bond_mask = 0
    with torch.no_grad(), pytest.raises(ValueError, match="engine only"):
        net.pretrain(mb)
    net.pretrain.layers[0].bond_mask = None
    with torch.no_grad(), pytest.raises(ValueError, match="uint8"):
        net.pretrain(mb.like({**mb, "mask_atoms": mb["mask_atoms"][:-1]}))
    assert not [c for c in counting.calls if c.startswith("fn_encoder_forward")]


@pytest.mark.parametrize("field,value,code,word", [("training", 1, -1, "training"), ("no_backward", 0, -1, "no_backward"),
                                                    ("variant", 1, -2, "variant"), ("heads", 2, -2, "four heads")])
def test_the_library_refuses_descriptors_a_masked_pass_does_not_exist_for(field, value, code, word, monkeypatch):
    """fn_encoder_forward_masked itself: FN_EINVAL / FN_EUNSUPPORTED with the reason in fn_last_error, outputs untouched."""
    import ctypes as C
    from fragnet_amd import _lib, engine
    _, net = _pair(scaled=False)
    _, mb, _ = _masked_batch()
    lib = _lib.load()
    real = engine._describe
    seen = {}

    def describe(*a, **k):
        e = real(*a, **k)
        setattr(e, field, value)
        return e
    monkeypatch.setattr(engine, "_describe", describe)

    class _Spy(_Counting):
        def __getattr__(self, name):
            fn = _Counting.__getattr__(self, name)
            if name != "fn_encoder_forward_masked":
                return fn

            def call(e, m, oa, of, ob, ofb, st):
                out = torch.full((mb["x_atoms"].shape[0], 128), 7.0, device=DEV)       # a buffer of the library's to leave alone
                seen["rc"] = fn(e, m, out.data_ptr(), of, ob, ofb, st)
                torch.cuda.synchronize()
                seen["untouched"] = bool((out == 7.0).all())
                return seen["rc"]
            return call
    monkeypatch.setattr(_lib, "_lib", _Spy(lib))
    with torch.no_grad(), pytest.raises(_lib.FragnetHipError, match=word):
        net.pretrain(mb)
    assert seen == {"rc": code, "untouched": True}


def test_mask_launch_writes_the_rows_and_flags_out_of_range_replicas():
    from fragnet_amd import _lib, attribution as attr, data
    from fragnet_amd.plan import SPACES
    mols = ac.molecules(40, seed=79)
    batch = data.batch_to(data.collate_fn(mols), DEV)
    off = batch.offsets.cpu().numpy()
    rows = [off[SPACES.index(s)] for s in ("atom", "edge", "fedge")]
    rng = np.random.default_rng(3)
    reps = np.zeros((40, 2), dtype=np.int32)
    want = [np.zeros(r[-1], dtype=np.uint8) for r in rows]
    for i in range(40):
        kind = int(rng.integers(0, 4))
        cnt = [0] + [int(r[i + 1] - r[i]) for r in rows]
        if kind and (cnt[kind] if kind == 1 else cnt[kind] // 2) == 0:
            kind = 0
        if kind == 1:
            idx = int(rng.integers(0, cnt[1]))
            want[0][rows[0][i] + idx] = 1
        elif kind:
            idx = int(rng.integers(0, cnt[kind] // 2))
            want[kind - 1][rows[kind - 1][i] + 2 * idx: rows[kind - 1][i] + 2 * idx + 2] = 1
        else:
            idx = int(rng.integers(0, 99))                      # kind 0 ignores its index
        reps[i] = (kind, idx)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = attr.build_row_masks(batch, torch.from_numpy(reps).to(DEV), status)
    assert int(status.item()) == 0
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    assert sum(int(w.sum()) for w in want) > 20
    # out of range: nothing written for that replica, the status word says so
    for bad in ((1, int(rows[0][1] - rows[0][0])), (2, int(rows[1][1] - rows[1][0]) // 2), (3, 10 ** 6), (1, -1), (4, 0)):
        r2 = reps.copy()
        r2[0] = bad
        status.zero_()
        got = attr.build_row_masks(batch, torch.from_numpy(r2).to(DEV), status)
        assert int(status.item()) == _lib.STATUS_BAD_REPLICA, bad
        for s, (g, w) in enumerate(zip(got, want)):
            w = w.copy()
            w[rows[s][0]: rows[s][1]] = 0
            np.testing.assert_array_equal(g.cpu().numpy(), w)


def test_script_writes_the_tables_leave_one_out_returns(tmp_path):
    """scripts/attribute_gat2.py on a synthetic store with the quick start's config: the .npz read back against a direct call."""
    import yaml
    from fragnet_amd import attribution as attr, synth, train
    from fragnet_amd.dataset import FlatMolStore
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import attribute_gat2
    finally:
        sys.path.pop(0)
    config = os.path.join(ROOT, "exps", "ft", "esol_synth", "config.yaml")
    FlatMolStore.from_records(synth.synth_molecules(24, seed=2, profile="esol")).save(str(tmp_path / "test.pt"))
    torch.manual_seed(11)
    model = attribute_gat2.build_model(train.load_config(config, config=config))
    torch.save(model.state_dict(), str(tmp_path / "ft.pt"))
    out = str(tmp_path / "attr.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "attribute_gat2.py"), "--config", config, "--checkpoint", str(tmp_path / "ft.pt"),
                        "--data", str(tmp_path / "test.pt"), "--out", out, "--max-rows", "30000"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "24 molecules" in r.stdout
    z = np.load(out)
    res = attr.leave_one_out(model.to(DEV), FlatMolStore.load(str(tmp_path / "test.pt"), device=DEV))
    assert list(z["kinds"]) == ["atom", "bond", "fbond"]
    _close(z["pred_no_mask"], res.pred_no_mask, "pred_no_mask")
    for k in res.kinds:
        np.testing.assert_array_equal(z[f"{k}_offsets"], res.tables[k]["offsets"])
        np.testing.assert_array_equal(z[f"{k}_index"], res.tables[k]["index"])
        _close(z[f"{k}_pred_mask"], res.tables[k]["pred_mask"], k)
        assert z[f"{k}_attr"].shape == res.tables[k]["attr"].shape
        np.testing.assert_allclose(z[f"{k}_attr"], z["pred_no_mask"][np.repeat(np.arange(24), np.diff(z[f"{k}_offsets"]))] - z[f"{k}_pred_mask"], atol=1e-6)
