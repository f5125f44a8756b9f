"""Host side of the attention read-outs (fragnet_amd/viz_model.py, fragnet_amd/attention.py, scripts/attention_gat2.py) and the pin
of the reference's fixture tests/golden/attn_readout_b6.npz (written by tests/golden/make_golden_viz.py) on the CPU: the oracle's last
layer, read out through the same forward hook, against the reference's own four tensors and logits."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fragnet_amd import attention as att
from tests import attr_common as ac
from tests import viz_common as vc
from tests.conftest import GOLDEN, ROOT


def _fixture():
    z = np.load(os.path.join(GOLDEN, "attn_readout_b6.npz"))
    return z, json.loads(str(z["cfg"]))


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    err = np.abs(got - ref) - (ac.ATOL + ac.RTOL * np.abs(ref))
    assert (err <= 0).all(), f"{what}: worst excess over the tolerance {err.max():.3e}"


@pytest.mark.parametrize("case", list(vc.CASES))
def test_oracle_matches_the_reference_attention_fixture(case):
    """The oracle's scaled model has the reference's weights (checksums); its logits and its last layer's four by-source sums on the
    one collated batch are the reference's within the project's 1e-4 + 1e-4 |ref|.  Also what the GPU tests rest on: the weights are
    far from uniform (a uniform softmax would give every source of the bond graph the same sum)."""
    from fragnet_amd import data
    from oracle import fragnet_ref as R
    from tests.helpers import check_params_match
    torch.set_num_threads(1)
    z, cfg = _fixture()
    assert (cfg["seed"], cfg["mol_seed"], cfg["n_mols"], cfg["head_scale"], cfg["att_scale"]) == (ac.SEED, ac.MOL_SEED, ac.N_MOLS, ac.HEAD_SCALE, ac.ATT_SCALE)
    assert cfg["ctor"][case]["num_heads"] == vc.CASES[case]
    model = ac.build(R, cfg["ctor"][case], cfg["seed"], scaled=True)
    check_params_match(model, json.loads(str(z[f"{case}/pkeys"])), z[f"{case}/psums"])
    logits, attn = vc.last_layer_readout(model, data.collate_fn(ac.molecules()), lambda m, b: m(b))
    _close(logits.numpy(), z[f"{case}/logits"], "logits")
    for name, t in zip(vc.NAMES, attn):
        _close(t.numpy(), z[f"{case}/{name}"], name)
        assert z[f"{case}/{name}"].shape[1] == vc.CASES[case]
    spread = z[f"{case}/attn_bonds"].std(0) / z[f"{case}/attn_bonds"].mean(0)
    assert (spread > 0.25).all(), spread


def test_fixture_holds_numbers_only_and_is_small():
    z, _ = _fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "attn_readout_b6.npz")) < 64 * 1024
    for k in z.files:
        assert z[k].dtype.kind in "fiU", k


def test_reference_rows_are_a_prefix_of_a_row_per_node():
    """The shape contract: the reference's scatter_add has no dim_size, so a tensor stops at source.max() + 1 of its level -- the
    fixture's row counts are exactly that, never more than the level's nodes -- and what lies beyond is zero."""
    from fragnet_amd import data
    from oracle import fragnet_ref as R
    torch.set_num_threads(1)
    z, cfg = _fixture()
    batch = data.collate_fn(ac.molecules())
    nodes = {"attn_atoms": batch["x_atoms"].shape[0], "attn_frags": batch["x_frags"].shape[0],
             "attn_bonds": batch["node_features_bonds"].shape[0], "attn_fbonds": batch["node_features_fbonds"].shape[0]}
    source = {"attn_atoms": batch["edge_index"][0], "attn_frags": batch["frag_index"][0],
              "attn_bonds": batch["edge_index_bonds_graph"][1], "attn_fbonds": batch["edge_index_fbonds"][1]}
    for name in vc.NAMES:
        rows = z[f"h4/{name}"].shape[0]
        want = nodes[name] if name == "attn_atoms" else int(source[name].max()) + 1      # (every atom is the source of its self loop)
        assert rows == want <= nodes[name], name
    # a level whose trailing nodes are no edge's source (hand-built: the featuriser's molecules have none): the reference's form of the
    # level stops at source.max() + 1, and a sum with a row per node is that prefix followed by zeros
    g = torch.Generator().manual_seed(3)
    n, H, d = 9, 4, 32
    src = torch.tensor([0, 1, 1, 2, 5, 5, 5, 0])
    dst = torch.tensor([1, 0, 2, 1, 0, 3, 8, 7])
    h = torch.randn(n, H, d, generator=g)
    _, probs, short = R.gat_level_materialised(h, torch.randn(src.numel(), d, generator=g), torch.randn(H, 3 * d, generator=g), dst, src, H)
    assert short.shape == (6, H) and n > 6
    full = torch.zeros(n, H).index_add_(0, src, probs)
    assert torch.equal(full[:6], short) and bool((full[6:] == 0).all()) and bool((full[3:5] == 0).all())


def test_split_by_molecule_on_hand_made_offsets():
    rows = {k: np.arange(n * 2, dtype=np.float32).reshape(n, 2) + 100 * i for i, (k, n) in enumerate(zip(att.LEVELS, (7, 8, 3, 2)))}
    offs = {"atoms": [0, 3, 3, 7], "bonds": [0, 4, 4, 8], "frags": [0, 1, 2, 3], "fbonds": [0, 0, 0, 2]}
    pred = np.asarray([[1.0], [2.0], [3.0]], dtype=np.float32)
    res = att.assemble([pred[:2], pred[2:]],
                       [{k: rows[k][: offs[k][2]] for k in att.LEVELS}, {k: rows[k][offs[k][2]:] for k in att.LEVELS}],
                       [{k: np.asarray(offs[k][:3]) for k in att.LEVELS}, {k: np.asarray(offs[k][2:]) - offs[k][2] for k in att.LEVELS}])
    assert len(res) == 3
    for k in att.LEVELS:
        np.testing.assert_array_equal(res.offsets[k], offs[k])
        np.testing.assert_array_equal(res.rows[k], rows[k])
    m1 = res[1]
    assert m1["atoms"].shape == (0, 2) and m1["bonds"].shape == (0, 2) and m1["fbonds"].shape == (0, 2) and m1["bond_weights"].shape == (0,)
    np.testing.assert_array_equal(m1["frags"], rows["frags"][1:2])
    m2 = res[-1]
    np.testing.assert_array_equal(m2["atoms"], rows["atoms"][3:7])
    np.testing.assert_array_equal(m2["fbonds"], rows["fbonds"])
    np.testing.assert_array_equal(m2["atom_weights"], rows["atoms"][3:7].sum(1))
    np.testing.assert_array_equal(m2["frag_weights"], rows["frags"][2:3].sum(1))
    assert float(m2["pred"][0]) == 3.0
    flat = res.arrays()
    assert set(flat) == {"pred", "atom_weights", "frag_weights", "bond_weights", "bond_weights_offsets"} | set(att.LEVELS) | {f"{k}_offsets" for k in att.LEVELS}
    np.testing.assert_array_equal(flat["bond_weights_offsets"], [0, 2, 2, 4])
    np.testing.assert_array_equal(flat["bond_weights"][2:], m2["bond_weights"])
    with pytest.raises(IndexError):
        res[3]
    with pytest.raises(ValueError):
        att.split_rows(rows["atoms"], [0, 3, 6])                # does not end at the tensor's rows
    with pytest.raises(ValueError):
        att.split_rows(rows["atoms"], [0, 5, 3, 7])             # not monotone


def test_bond_combination_is_the_references_precedence():
    """viz.py:684-687: ``a1 + a2/2`` halves the second direction only."""
    w = np.asarray([[1.0, 2.0], [10.0, 20.0], [3.0, 4.0], [30.0, 40.0]], dtype=np.float32)
    np.testing.assert_array_equal(att.bond_weights(w), [(1 + 5) + (2 + 10), (3 + 15) + (4 + 20)])
    a1, a2 = torch.from_numpy(w)[::2], torch.from_numpy(w)[1::2]
    np.testing.assert_array_equal(att.bond_weights(w), (a1 + a2 / 2).sum(1).numpy())
    assert not np.array_equal(att.bond_weights(w), ((w[::2] + w[1::2]) / 2).sum(1))


def test_viz_classes_have_the_reference_signatures_and_load_checkpoints_strictly():
    import inspect
    from fragnet_amd import model as M, viz_model as V
    sig = lambda c: [(p.name, p.default) for p in inspect.signature(c.__init__).parameters.values() if p.name != "self"]
    E = inspect.Parameter.empty
    assert sig(V.FragNetViz) == [("num_layer", E), ("drop_ratio", 0.2), ("emb_dim", 128), ("atom_features", 167), ("frag_features", 167),
                                 ("edge_features", 17), ("fedge_in", 6), ("fbond_edge_in", 6), ("num_heads", 4)]
    ft = [("n_classes", 1), ("atom_features", 167), ("frag_features", 167), ("edge_features", 16), ("num_layer", 4), ("num_heads", 4),
          ("drop_ratio", 0.15), ("h1", 256), ("h2", 256), ("h3", 256), ("h4", 256), ("act", "celu"), ("emb_dim", 128), ("fthead", "FTHead3")]
    assert sig(V.FragNetFineTuneViz) == ft
    assert sig(V.FragNetFineTuneBaseViz) == [(k, 17 if k == "edge_features" else v) for k, v in ft]
    assert sig(V.FragNetPreTrainViz) == [("num_layer", 4), ("drop_ratio", 0.15), ("num_heads", 4), ("emb_dim", 128), ("atom_features", 167),
                                         ("frag_features", 167), ("edge_features", 16)]
    small = dict(num_layer=3, h1=8, h2=8, h3=8, h4=8, edge_features=17)
    for head in ("FTHead1", "FTHead2", "FTHead3", "FTHead4"):
        src = M.FragNetFineTune(fthead=head, **small)
        for cls in (V.FragNetFineTuneViz, V.FragNetFineTuneBaseViz):
            dst = cls(fthead=head, **small)
            assert list(dst.state_dict()) == list(src.state_dict())
            dst.load_state_dict(src.state_dict(), strict=True)
    pt = M.FragNetPreTrain(num_layer=2, edge_features=17)
    pv = V.FragNetPreTrainViz(num_layer=2, edge_features=17)
    assert list(pv.state_dict()) == list(pt.state_dict())
    pv.load_state_dict(pt.state_dict(), strict=True)
    assert all(k.startswith(("pretrain.layers.", "head.")) for k in pv.state_dict())
    v = V.FragNetViz(num_layer=3)
    assert [l.return_attentions for l in v.layers] == [False, False, True]
    assert len(V.FragNetViz(num_layer=1).layers) == 2              # first + last, as the reference builds it
    # the same seed gives the same weights as the plain encoder (construction order = RNG order)
    torch.manual_seed(3)
    a = M.FragNet(num_layer=2).state_dict()
    torch.manual_seed(3)
    b = V.FragNetViz(num_layer=2).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    m = V.FragNetFineTuneViz(**small)
    assert m.use_engine is True
    m.use_engine = False
    assert m.pretrain.use_engine is False


def test_alias_module_resolves_to_the_viz_classes():
    sys.path.insert(0, ROOT)
    try:
        mod = importlib.import_module("fragnet.vizualize.model")
        from fragnet_amd import viz_model as V
        assert mod.__file__.startswith(ROOT)
        for name in ("FragNetViz", "FragNetFineTuneViz", "FragNetFineTuneBaseViz", "FragNetPreTrainViz"):
            assert getattr(mod, name) is getattr(V, name)
    finally:
        sys.path.remove(ROOT)


def test_cpu_models_and_other_models_are_refused():
    from fragnet_amd import _lib, data
    from fragnet_amd.model import FragNetFineTune
    from fragnet_amd.viz_model import FragNetFineTuneViz
    mols = ac.molecules(2)
    small = dict(num_layer=2, h1=8, h2=8, h3=8, h4=8, edge_features=17)
    with pytest.raises(ValueError, match="Viz model"):
        att.attention_weights(FragNetFineTune(**small), mols)
    with pytest.raises(_lib.FragnetHipError):                      # a CPU model: no fallback
        att.attention_weights(FragNetFineTuneViz(**small), mols)
    with pytest.raises(ValueError):
        att.attention_weights(FragNetFineTuneViz(**small), mols, batch_size=0)
    with pytest.raises(_lib.FragnetHipError), torch.no_grad():
        FragNetFineTuneViz(**small).eval()(data.collate_fn(mols))


SCRIPT = os.path.join(ROOT, "scripts", "attention_gat2.py")


def test_script_argument_handling():
    run = lambda *argv: subprocess.run([sys.executable, SCRIPT, *argv], capture_output=True, text=True, cwd=ROOT)
    r = run("--help")
    assert r.returncode == 0 and "--checkpoint" in r.stdout and "--batch-size" in r.stdout
    base = ["--config", "c.yaml", "--checkpoint", "m.pt", "--data", "d.pt"]
    r = run(*base)
    assert r.returncode == 2 and "--out" in r.stderr
    assert run(*base, "--out", "a.txt").returncode == 2
    assert run(*base, "--out", "a.npz", "--batch-size", "0").returncode == 2
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import attention_gat2
    finally:
        sys.path.pop(0)
    a = attention_gat2.parse_args([*base, "--out", "o/a.npz", "--batch-size", "64"])
    assert (a.batch_size, a.device, a.out) == (64, "cuda:0", "o/a.npz")
