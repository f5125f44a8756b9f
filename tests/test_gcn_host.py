"""CPU-side checks of model_version gcn2 (fragnet_amd/gcn.py): the module tree is the reference's fragnet/model/gcn/gcn2.py -- same
state-dict keys in the same order, same initial values under the same seed (checksums recorded by tests/golden/make_golden_gcn.py) --,
the reference's import path resolves to it, and its graph plan builds no bond-graph task."""
import inspect

import pytest
import torch

from tests.helpers import check_params_match, load_case

CASES = ("ft_gcn2_b6", "ft_gcn2_edge_b6")


@pytest.mark.parametrize("case", CASES)
def test_state_dict_is_the_reference_module_tree(case):
    from fragnet_amd.gcn import FragNetFineTune
    cfg, _, _, grads, pkeys, psums = load_case(case)
    torch.manual_seed(cfg["seed"])
    model = FragNetFineTune(**cfg["ctor"])
    check_params_match(model, pkeys, psums)
    L = cfg["ctor"]["num_layer"]
    # 16 parameter tensors per layer, 5 BatchNorm entries per layer, lin1 and the head
    assert len(pkeys) == 21 * L + 2 + len(model.fthead.state_dict())
    assert sum(k.endswith("num_batches_tracked") for k in pkeys) == L
    # what the fixture holds a gradient for is what this model's forward reads: atom_embed of every layer, the last layer's frag_mlp, the head
    live = set(grads["sum"])
    want = {f"pretrain.layers.{i}.atom_embed.{w}" for i in range(L) for w in ("weight", "bias")}
    want |= {f"pretrain.layers.{L - 1}.frag_mlp.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")}
    want |= {"fthead." + k for k in model.fthead.state_dict()}
    assert live == want


def test_probe_fixture_is_the_documented_run():
    cfg, batch, out, _, pkeys, _ = load_case("ft_gcn2_b6")
    assert cfg["ctor"]["num_layer"] == 3 and cfg["ctor"]["fthead"] == "FTHead3" and cfg["seed"] == 7
    assert len(pkeys) == 75 and batch["y"].shape[0] == 6
    assert abs(float(out["loss"]) - 1.349604) < 5e-7
    edge_cfg, edge_batch, edge_out, _, _, _ = load_case("ft_gcn2_edge_b6")
    assert edge_cfg["ctor"]["fthead"] == "FTHead4" and edge_cfg["ctor"]["act"] != "relu" and edge_cfg["ctor"]["num_layer"] == 2
    deg = torch.bincount(edge_batch["edge_index"][0], minlength=edge_batch["x_atoms"].shape[0])
    assert int((deg == 0).sum()) >= 2                        # atoms without a bond: their only item is the self loop
    for o, L in ((out, 3), (edge_out, 2)):
        assert all(f"layer{i}/{nm}" in o for i in range(L) for nm in ("x_atoms", "x_frags"))


def test_reference_import_path_and_signatures():
    from fragnet.model.gcn import gcn2
    from fragnet_amd import gcn
    assert gcn2.FragNetFineTune is gcn.FragNetFineTune and gcn2.FragNet is gcn.FragNet and gcn2.FragNetLayer is gcn.FragNetLayer
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(gcn.FragNetFineTune.__init__)[1:] == ["n_classes", "atom_features", "frag_features", "edge_features", "num_layer", "drop_ratio",
                                                       "emb_dim", "h1", "h2", "h3", "h4", "act", "fthead"]
    assert names(gcn.FragNet.__init__)[1:] == ["num_layer", "drop_ratio", "emb_dim", "atom_features", "frag_features", "edge_features"]
    assert names(gcn.FragNetLayer.__init__)[1:] == ["atom_in", "atom_out", "frag_in", "frag_out", "edge_in", "edge_out"]
    assert names(gcn.FragNetLayer.forward)[1:] == ["x_atoms", "edge_index", "edge_attr", "frag_index", "x_frags", "atom_to_frag_ids"]
    d = inspect.signature(gcn.FragNetFineTune.__init__).parameters
    assert (d["edge_features"].default, d["num_layer"].default, d["drop_ratio"].default, d["act"].default) == (16, 4, .15, "celu")


def test_reference_checkpoint_layout_loads_strictly():
    """a state dict with the fixture's keys (a reference checkpoint) loads with strict=True, BatchNorm buffers included"""
    from fragnet_amd.gcn import FragNetFineTune
    cfg, _, _, _, pkeys, _ = load_case("ft_gcn2_b6")
    a, b = FragNetFineTune(**cfg["ctor"]), FragNetFineTune(**cfg["ctor"])
    sd = a.state_dict()
    assert list(sd) == pkeys
    b.load_state_dict(sd, strict=True)


def test_reduced_plan_names_no_bond_graph_task():
    from fragnet_amd.plan import GraphPlan
    _, batch, _, _, _, _ = load_case("ft_gcn2_b6")
    specs = GraphPlan.gcn_specs(batch, batch["y"].shape[0])
    assert [(s["kind"], s["name"]) for s in specs] == [("gat", "atom"), ("gat", "frag"), ("seg", "a2f"), ("seg", "mol_atoms"), ("seg", "mol_frags")]
    atom, frag = specs[0], specs[1]
    assert atom["n_loops"] == atom["n"] == batch["x_atoms"].shape[0] and frag["n_loops"] == 0
    bond_graph = (batch["edge_index_bonds_graph"], batch["edge_index_fbonds"])
    for s in specs:
        for t in (s.get("dst"), s.get("src"), s.get("key")):
            assert t is None or all(t.data_ptr() != g.data_ptr() and t.numel() != g[0].numel() for g in bond_graph)
    # the items the reduced plan sorts are a minority of what the full plan does
    items = sum((s["dst"].numel() + s["n_loops"]) * 2 if s["kind"] == "gat" else s["key"].numel() for s in specs)
    full = items + 2 * (bond_graph[0].shape[1] + bond_graph[1].shape[1])
    assert items < full / 2


def test_cpu_tensors_are_refused():
    from fragnet_amd import _lib
    from fragnet_amd.gcn import FragNetFineTune
    cfg, batch, _, _, _, _ = load_case("ft_gcn2_b6")
    with pytest.raises(_lib.FragnetHipError):
        FragNetFineTune(**cfg["ctor"])(dict(batch))


def test_driver_config_selects_gcn2():
    import os
    from fragnet_amd import train
    from tests.conftest import ROOT
    c = train.load_config(os.path.join(ROOT, "exps/ft/esol_synth_gcn2/config.yaml"))
    assert c.model_version == "gcn2" and c.finetune.model.fthead in ("FTHead3", "FTHead4")
    assert c.finetune.chkpoint_name.startswith("exps/ft/esol_synth_gcn2/")
