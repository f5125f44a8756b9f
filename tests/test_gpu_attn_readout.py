"""The attention read-out pass of the engine (fn_encoder_forward_attn, csrc/attn_readout.hip), the Viz model classes built on it
(fragnet_amd/viz_model.py) and the batched driver (fragnet_amd/attention.py).

Expected values: the reference's fixture tests/golden/attn_readout_b6.npz and the oracle (oracle/fragnet_ref.py) on the CPU, its last
layer read out through the same forward hook (tests/viz_common.py).  Tolerance: the project's |got - ref| <= 1e-4 + 1e-4 |ref|.
The reference's tensors stop at source.max() + 1 of their level; the engine's have a row per node: compared on the reference's rows,
and the rows beyond must be exactly 0.  The models are the scaled ones of tests/attr_common.py (attention vectors x 4)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import attr_common as ac
from tests import viz_common as vc
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ORDER = ("atoms", "frags", "bonds", "fbonds")          # the order of the models' return tuples and of viz_common.NAMES


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    err = np.abs(got - ref) - (ac.ATOL + ac.RTOL * np.abs(ref))
    worst = err.max() if err.size else -1.0
    print(f"{what}: worst excess over the tolerance {worst:.3e}")
    assert worst <= 0, f"{what}: worst excess over the tolerance {worst:.3e}"


def _close_prefix(got, ref, nodes, what):
    """``ref`` is the reference-shaped tensor (source.max() + 1 rows), ``got`` has a row per node; beyond ``ref`` it is exactly 0."""
    got = np.asarray(got)
    assert got.shape[0] == nodes and ref.shape[0] <= nodes, f"{what}: {got.shape[0]} rows for {nodes} nodes (reference {ref.shape[0]})"
    _close(got[: ref.shape[0]], ref, what)
    assert (got[ref.shape[0]:] == 0).all(), f"{what}: rows beyond the reference's are not zero"


def _ctor(heads):
    return dict(atom_features=167, frag_features=167, edge_features=17, emb_dim=128, **dict(ac.CTOR, num_heads=heads))


_PAIRS = {}


def _pair(heads):
    """(oracle on the CPU, FragNetFineTuneViz on the GPU) with the same scaled weights; built once per head count."""
    if heads not in _PAIRS:
        from fragnet_amd import viz_model as V
        from oracle import fragnet_ref as R
        gold = ac.build(R, _ctor(heads), ac.SEED, scaled=True)
        net = V.FragNetFineTuneViz(**_ctor(heads))
        net.load_state_dict(gold.state_dict(), strict=True)
        _PAIRS[heads] = (gold, net.to(DEV).eval())
    return _PAIRS[heads]


def _nodes(batch):
    return {"atoms": batch["x_atoms"].shape[0], "frags": batch["x_frags"].shape[0], "bonds": batch["node_features_bonds"].shape[0],
            "fbonds": batch["node_features_fbonds"].shape[0]}


def _plain_dict(batch):
    """The same tensors without the collate's promise about their layout: the general plan builder and the general fragment tail."""
    return {k: v for k, v in dict(batch).items() if k != "_fragnet_plan"}


_ORACLE = {}


def _oracle(heads, key, cpu_batch):
    if (heads, key) not in _ORACLE:
        torch.set_num_threads(8)
        logits, attn = vc.last_layer_readout(_pair(heads)[0], cpu_batch, lambda m, b: m(b))
        _ORACLE[(heads, key)] = (logits.numpy(), [t.numpy() for t in attn])
    return _ORACLE[(heads, key)]


def _run(net, batch):
    with torch.no_grad():
        out = net(batch)
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), [t.cpu().numpy() for t in out[1:]]


def _check_against(ref_logits, ref_attn, logits, attn, nodes, what):
    _close(logits.reshape(ref_logits.shape), ref_logits, f"{what} logits")
    for name, got, ref in zip(ORDER, attn, ref_attn):
        assert got.shape[1] == ref.shape[1]
        _close_prefix(got, ref, nodes[name], f"{what} {name}")


@pytest.mark.parametrize("route", ["collated", "plain-dict", "collated-saves"])
@pytest.mark.parametrize("case", list(vc.CASES))
def test_engine_readout_matches_the_reference_fixture_and_the_oracle(case, route, monkeypatch):
    """FragNetFineTuneViz in eval mode = one read-out pass: logits and the four tensors against the reference's fixture and against the
    oracle.  Routes: a collated batch (molecule-resident fragment tail), the same tensors as a plain dict (general tail), and the
    collated batch with no_backward = 0 (an evaluation pass that saves for a backward pass)."""
    from fragnet_amd import data, engine
    heads = vc.CASES[case]
    z = np.load(os.path.join(GOLDEN, "attn_readout_b6.npz"))
    cfg = json.loads(str(z["cfg"]))
    assert cfg["ctor"][case] == _ctor(heads) and (cfg["seed"], cfg["mol_seed"], cfg["n_mols"]) == (ac.SEED, ac.MOL_SEED, ac.N_MOLS)
    _, net = _pair(heads)
    cpu_batch = data.collate_fn(ac.molecules())
    batch = data.batch_to(cpu_batch, DEV)
    if route == "plain-dict":
        batch = _plain_dict(batch)
    seen = []
    real = engine._describe

    def describe(*a, **k):
        e = real(*a, **k)
        seen.append((int(e.no_backward), int(e.mol_contiguous)))
        return e
    monkeypatch.setattr(engine, "_describe", describe)
    if route == "collated-saves":
        monkeypatch.setattr(engine, "_EVAL_SAVES", True)
    logits, attn = _run(net, batch)
    assert seen == [(0 if route == "collated-saves" else 1, 0 if route == "plain-dict" else 1)]
    nodes = _nodes(cpu_batch)
    _check_against(z[f"{case}/logits"], [z[f"{case}/{n}"] for n in vc.NAMES], logits, attn, nodes, f"{route} against the fixture:")
    _check_against(*_oracle(heads, "b6", cpu_batch), logits, attn, nodes, f"{route} against the oracle:")


def _p_slots(e, n_layers, H):
    """Offsets (floats) of the last layer's stored probabilities in an encoder workspace: the head of enc_layout (csrc/encoder.hip) --
    per layer six row buffers, the four probability buffers, and (inner layers) the four activated outputs, in 64-float granules."""
    r64 = lambda n: (n + 63) // 64 * 64
    N, E, F_, EF = e.N, e.E, e.F, e.EF
    used, slots = 0, {}
    for l in range(n_layers):
        for rows in (E, N, EF, F_, E, EF):
            used += r64(rows * 128)
        for name, m in (("bonds", e.bond.m), ("atoms", e.atom.m), ("fbonds", e.fbond.m), ("frags", e.frag.m)):
            slots[(l, name)] = (used, m * H)
            used += r64(m * H)
        if l + 1 < n_layers:
            for rows in (N, F_, E, EF):
                used += r64(rows * 128)
    return {name: slots[(n_layers - 1, name)] for name in ORDER}


@pytest.mark.parametrize("route", ["collated", "plain-dict"])
def test_readout_kernel_equals_attn_by_src_and_the_per_level_route(route, monkeypatch):
    """The one new launch against ops.attn_by_src (k_attn_by_src, one launch per level) fed the probabilities the pass stored: the
    same bits.  And the engine route against the per-level route (use_engine=False) of the same model at the project's tolerance."""
    from fragnet_amd import data, engine, ops
    from fragnet_amd.plan import plan_for
    _, net = _pair(4)
    batch = data.batch_to(data.collate_fn(ac.molecules(24, seed=81)), DEV)
    if route == "plain-dict":
        batch = _plain_dict(batch)
    kept = []
    monkeypatch.setattr(engine, "_KEEP_ATTN_WS", kept)
    with torch.no_grad():
        out = net(batch)
    torch.cuda.synchronize()
    (e, ws), = kept
    levels = plan_for(batch).levels
    for name, lv, got in zip(ORDER, ("atom", "frag", "bond", "fbond"), out[1:]):
        off, size = _p_slots(e, len(net.pretrain.layers), 4)[name]
        assert size == levels[lv].m * 4 and off + size <= ws.numel()
        want = ops.attn_by_src(ws[off: off + size], levels[lv], 4)
        assert got.shape == want.shape == (levels[lv].n, 4)
        assert torch.equal(got, want), f"{name}: the read-out launch and k_attn_by_src differ on the same probabilities"
        assert float(got.sum()) > 0
    net.use_engine = False
    try:
        with torch.no_grad():
            slow = net(batch)
    finally:
        net.use_engine = True
    torch.cuda.synchronize()
    _close(out[0].cpu().numpy(), slow[0].cpu().numpy(), "logits, engine against per-level")
    for name, a, b in zip(ORDER, out[1:], slow[1:]):
        _close(a.cpu().numpy(), b.cpu().numpy(), f"{name}, engine against per-level")


@pytest.mark.parametrize("saves", [False, True], ids=["no_backward-1", "no_backward-0"])
def test_encoder_outputs_of_a_readout_pass_are_the_plain_passes_bits(saves, monkeypatch):
    from fragnet_amd import data, engine, model as M
    _, net = _pair(4)
    plain = M.FragNet(num_layer=2, drop_ratio=0.0, num_heads=4).to(DEV).eval()
    plain.load_state_dict(net.pretrain.state_dict(), strict=True)
    monkeypatch.setattr(engine, "_EVAL_SAVES", saves)
    for as_dict in (False, True):
        batch = data.batch_to(data.collate_fn(ac.molecules(48, seed=77)), DEV)
        batch = _plain_dict(batch) if as_dict else batch
        with torch.no_grad():
            got = [t.clone() for t in net.pretrain(batch)[:4]]
            batch.pop("_fragnet_plan", None)
            want = plain(batch, edge_outputs=True)
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and torch.equal(a, b), f"output {k} of the read-out pass differs from the plain pass (plain dict: {as_dict})"


@pytest.mark.parametrize("heads", [2, 4, 8])
def test_attention_is_conserved_per_level_and_head(heads):
    """Every destination row with at least one in-edge hands out probabilities that sum to 1, so per level and head the by-source
    sums add up to the number of such rows (1e-4 relative).  The counts come from the batch's index tensors."""
    from fragnet_amd import data
    _, net = _pair(heads)
    cpu_batch = data.collate_fn(ac.molecules(32, seed=83))
    _, attn = _run(net, data.batch_to(cpu_batch, DEV))
    fed = {"atoms": cpu_batch["x_atoms"].shape[0],                                    # every atom has its self loop
           "frags": int(torch.unique(cpu_batch["frag_index"][1]).numel()),
           "bonds": int(torch.unique(cpu_batch["edge_index_bonds_graph"][0]).numel()),
           "fbonds": int(torch.unique(cpu_batch["edge_index_fbonds"][0]).numel())}
    for name, t in zip(ORDER, attn):
        total = t.astype(np.float64).sum(0)
        print(name, fed[name], total)
        assert t.shape[1] == heads and fed[name] > 0
        assert (np.abs(total - fed[name]) <= 1e-4 * fed[name]).all(), f"{name}: {total} against {fed[name]} fed rows"


def _edge_batches():
    """name -> CPU batch (a CollatedBatch or a plain dict) of the edge shapes."""
    from fragnet_amd import data, synth
    out = {}
    rng = np.random.default_rng(11)
    single = synth.make_molecule(rng, mu=6, p_cut=0.0)
    assert int(single.n_frags) == 1
    out["single-fragment"] = data.collate_fn([single])
    # the same molecule without its placeholder connection row: EF == 0, a fragment graph and a fragment-bond graph without edges
    b = dict(data.collate_fn([single]))
    b["frag_index"] = b["frag_index"][:, :0].contiguous()
    b["node_features_fbonds"] = b["node_features_fbonds"][:0].contiguous()
    b["edge_index_fbonds"] = b["edge_index_fbonds"][:, :0].contiguous()
    b["edge_attr_fbonds"] = b["edge_attr_fbonds"][:0].contiguous()
    out["single-fragment-EF0"] = b
    chain = lambda n: (n, [(i, i + 1) for i in range(n - 1)], [True] * (n - 1))      # every bond cut: one fragment per atom
    cut = synth.make_molecule(rng, topology=chain(8))
    assert int(cut.n_frags) == 8
    out["fully-cut"] = data.collate_fn([cut])
    big = synth.make_molecule(rng, topology=chain(40))                                # more fragments than the fused tail's LDS class (32)
    assert int(big.n_frags) == 40
    out["beyond-the-lds-tail"] = data.collate_fn([big] + ac.molecules(2))
    # a hand-built fragment level: fragment 0 is the source of 40 edges, the trailing fragments have no edge at all, and the
    # fragment-bond graph over the 44 connection rows has isolated rows too (a plain dict: nothing promises a layout)
    b = dict(data.collate_fn(ac.molecules(20, seed=85)))
    F_ = b["x_frags"].shape[0]
    assert F_ >= 48
    g = torch.Generator().manual_seed(9)
    src = torch.tensor([0] * 40 + [3, 5, 5, 41])                       # (the last fragment is a destination: the reference sizes a level's
    dst = torch.tensor(list(range(1, 41)) + [0, 0, F_ - 1, 2])         # output by destination.max() + 1 and needs every row of it)
    EF = src.numel()
    b["frag_index"] = torch.stack([src, dst])
    b["node_features_fbonds"] = torch.rand(EF, b["node_features_fbonds"].shape[1], generator=g)
    fb_dst = torch.cat([torch.randint(0, 30, (89,), generator=g), torch.tensor([EF - 1])])
    fb_src = torch.randint(0, 36, (90,), generator=g)
    b["edge_index_fbonds"] = torch.stack([fb_dst, fb_src])
    b["edge_attr_fbonds"] = torch.rand(90, b["edge_attr_fbonds"].shape[1], generator=g)
    out["out-degree-40"] = b
    return out


_EDGE = {}


@pytest.mark.parametrize("heads", [2, 4, 8])
@pytest.mark.parametrize("shape", ["single-fragment", "single-fragment-EF0", "fully-cut", "beyond-the-lds-tail", "out-degree-40"])
def test_edge_shapes(shape, heads):
    from fragnet_amd import data
    from fragnet_amd.plan import CollatedBatch
    if not _EDGE:
        _EDGE.update(_edge_batches())
    cpu_batch = _EDGE[shape]
    _, net = _pair(heads)
    batch = data.batch_to(cpu_batch, DEV) if isinstance(cpu_batch, CollatedBatch) else {k: v.to(DEV) for k, v in cpu_batch.items()}
    logits, attn = _run(net, batch)
    nodes = _nodes(cpu_batch)
    if shape == "single-fragment-EF0":
        # the oracle's scatter ops have no form for a level without edges; the atom and bond levels never read the fragment side, so
        # they are the unedited molecule's, and the two empty levels are known: no edge, no attention
        ref_logits, ref_attn = _oracle(heads, "single-fragment", _EDGE["single-fragment"])
        assert attn[1].shape == (1, heads) and (attn[1] == 0).all() and attn[3].shape == (0, heads)
        for k in (0, 2):
            _close_prefix(attn[k], ref_attn[k], nodes[ORDER[k]], f"{shape} {ORDER[k]}")
        assert np.isfinite(logits).all()
        return
    ref_logits, ref_attn = _oracle(heads, shape, cpu_batch)
    if shape == "out-degree-40":
        assert ref_attn[1].shape[0] < nodes["frags"] and ref_attn[3].shape[0] < nodes["fbonds"]      # the reference's tensors are shorter here
    _check_against(ref_logits, ref_attn, logits, attn, nodes, f"{shape} H={heads}:")


class _Counting:
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


@pytest.mark.parametrize("field,value,code,word", [("training", 1, -1, "training"), ("variant", 1, -2, "variant"), ("variant", 2, -2, "variant")])
def test_the_library_refuses_descriptors_a_readout_pass_does_not_exist_for(field, value, code, word, monkeypatch):
    """fn_encoder_forward_attn itself: FN_EINVAL / FN_EUNSUPPORTED with the reason in fn_last_error, before anything is launched:
    outputs and read-out tensors pre-filled with a sentinel stay untouched."""
    from fragnet_amd import _lib, data, engine
    _, net = _pair(4)
    batch = data.batch_to(data.collate_fn(ac.molecules(4, seed=78)), DEV)
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
            if name != "fn_encoder_forward_attn":
                return fn

            def call(e, r, oa, of, ob, ofb, st):
                n = batch["x_atoms"].shape[0]
                out = torch.full((n, 128), 7.0, device=DEV)
                attn = torch.full((n, 4), 7.0, device=DEV)
                r2 = _lib.AttnReadout(attn.data_ptr(), None, None, None)
                seen["rc"] = fn(e, C.byref(r2), out.data_ptr(), of, ob, ofb, st)
                torch.cuda.synchronize()
                seen["untouched"] = bool((out == 7.0).all()) and bool((attn == 7.0).all())
                return seen["rc"]
            return call
    monkeypatch.setattr(_lib, "_lib", _Spy(_lib.load()))
    with torch.no_grad(), pytest.raises(_lib.FragnetHipError, match=word):
        net(batch)
    assert seen == {"rc": code, "untouched": True}


def test_readout_passes_that_cannot_run_are_refused_before_the_library_is_called(monkeypatch):
    """Python side: training mode, a gradient required, another model version, and a read-out together with row masks."""
    from fragnet_amd import _lib, data, engine
    from fragnet_amd.plan import plan_for
    _, net = _pair(4)
    batch = data.batch_to(data.collate_fn(ac.molecules(4, seed=78)), DEV)
    plan = plan_for(batch)
    proxy = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    enc = net.pretrain

    def call(training=False, variant=0, row_masks=None):
        return engine.encoder_forward(enc.layers, plan, batch["x_atoms"], batch["node_features_bonds"], batch["node_features_fbonds"],
                                      plan.sorted_attr("bond", batch["edge_attr_bonds"], defer=True),
                                      plan.sorted_attr("fbond", batch["edge_attr_fbonds"], defer=True), 4, 0.0, training, enc.rng,
                                      variant=variant, row_masks=row_masks, attn_readout=True)
    proxy.calls.clear()
    with torch.no_grad(), pytest.raises(RuntimeError, match="evaluation"):
        call(training=True)
    with pytest.raises(RuntimeError, match="no backward"):                    # parameters require gradients and grad mode is on
        call()
    for variant in (1, 2):
        with torch.no_grad(), pytest.raises(ValueError, match="gat2"):
            call(variant=variant)
    mask = torch.zeros(batch["x_atoms"].shape[0], dtype=torch.uint8, device=DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="masked pass"):
        call(row_masks=(mask, None, None))
    with torch.no_grad(), pytest.raises(ValueError, match="masked pass"):      # the same through the model: a batch that carries masks
        net(batch.like({**batch, "mask_atoms": mask}))
    assert not [c for c in proxy.calls if c.startswith("fn_encoder_forward")]
    with torch.no_grad():                                                    # and the null read-out: three None masks run the pass
        out = call(row_masks=(None, None, None))
    assert len(out) == 9 and proxy.calls.count("fn_encoder_forward_attn") == 1


def test_null_readout_is_the_plain_pass(monkeypatch):
    """fn_encoder_forward_attn with r == NULL and with four NULL pointers: fn_encoder_forward's bits."""
    from fragnet_amd import _lib, data, model as M
    _, net = _pair(4)
    plain = M.FragNet(num_layer=2, drop_ratio=0.0, num_heads=4).to(DEV).eval()
    plain.load_state_dict(net.pretrain.state_dict(), strict=True)
    batch = data.batch_to(data.collate_fn(ac.molecules(12, seed=79)), DEV)
    with torch.no_grad():
        want = [t.clone() for t in plain(batch, edge_outputs=True)]
    lib = _lib.load()
    for null_struct in (True, False):
        class _Swap(_Counting):
            def __getattr__(self, name):
                if name != "fn_encoder_forward":
                    return _Counting.__getattr__(self, name)
                r = _lib.AttnReadout(None, None, None, None)
                return lambda e, *rest: lib.fn_encoder_forward_attn(e, None if null_struct else C.byref(r), *rest)
        monkeypatch.setattr(_lib, "_lib", _Swap(lib))
        batch.pop("_fragnet_plan", None)
        with torch.no_grad():
            got = plain(batch, edge_outputs=True)
        torch.cuda.synchronize()
        monkeypatch.setattr(_lib, "_lib", lib)
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), f"output {k} (null struct: {null_struct})"


def test_pretrain_and_base_viz_classes_run_the_same_pass():
    from fragnet_amd import data, viz_model as V
    _, net = _pair(4)
    batch = data.batch_to(data.collate_fn(ac.molecules(6, seed=80)), DEV)
    with torch.no_grad():
        ft = net(batch)
    pv = V.FragNetPreTrainViz(num_layer=2, drop_ratio=0.0, edge_features=17).to(DEV).eval()
    pv.pretrain.load_state_dict(net.pretrain.state_dict(), strict=True)
    base = V.FragNetFineTuneBaseViz(**_ctor(4)).to(DEV).eval()
    base.load_state_dict(net.state_dict(), strict=True)
    with torch.no_grad():
        batch.pop("_fragnet_plan", None)
        out = pv(batch)
        batch.pop("_fragnet_plan", None)
        cat = base(batch)
    assert len(out) == 5 and out[0].shape[0] == 6 and cat.shape == (6, 256)
    for a, b in zip(out[1:], ft[1:]):
        assert torch.equal(a, b)


def test_driver_in_batches_of_four_equals_one_batch_of_six():
    from fragnet_amd import attention as att
    _, net = _pair(4)
    mols = ac.molecules()
    one = att.attention_weights(net, mols, batch_size=6)
    split = att.attention_weights(net, mols, batch_size=4)
    assert len(one) == len(split) == 6 and not net.training
    lens = [(m.x_atoms.shape[0], m.node_features_bonds.shape[0], int(m.n_frags), m.node_feautures_fbondg.shape[0]) for m in mols]
    for i in range(6):
        a, b = one[i], split[i]
        assert (a["atoms"].shape[0], a["bonds"].shape[0], a["frags"].shape[0], a["fbonds"].shape[0]) == lens[i]
        assert a["atoms"].shape[1] == 4 and a["bond_weights"].shape == (lens[i][1] // 2,)
        for k in ("pred", "atoms", "bonds", "frags", "fbonds", "atom_weights", "frag_weights", "bond_weights"):
            _close(b[k], a[k], f"molecule {i} {k}")
    ref_logits, ref_attn = _oracle(4, "b6", __import__("fragnet_amd.data", fromlist=["collate_fn"]).collate_fn(mols))
    _close(one.pred.reshape(ref_logits.shape), ref_logits, "driver predictions against the oracle")
    _close(one.rows["atoms"], ref_attn[0], "driver atoms against the oracle")
    flat = one.arrays()
    assert flat["atoms"].shape == (sum(l[0] for l in lens), 4) and flat["bond_weights_offsets"][-1] == sum(l[1] for l in lens) // 2
