"""tests/topologies.py on the host: the builders hit the row lengths and molecule classes that tests/test_gpu_engine_topologies.py relies on
(so a change in fragnet_amd.synth cannot quietly move a case off its boundary), and the oracle itself is far more exact on these batches
than the tolerance the GPU tests hold the kernels to."""
import numpy as np
import pytest
import torch

from tests import topologies as T


def _rec(top, seed=0):
    from fragnet_amd import synth
    return synth.make_molecule(np.random.default_rng(seed), topology=top)


@pytest.mark.parametrize("n", [12, 24, 25, 32, 33])
def test_cut_chain_has_n_fragments_and_twice_n_minus_one_edges(n):
    d = T.describe(_rec(T.chain(n)))
    assert (d["atoms"], d["frags"], d["nc"], d["mec"]) == (n, n, n - 1, 2 * (n - 1))
    assert (d["in_atom"], d["in_bond"], d["in_frag"], d["in_fbond"]) == (3, 4, 2, 4)
    d = T.describe(_rec(T.chain(n, cut=False)))
    assert (d["frags"], d["mec"]) == (1, 1)


def test_chains_sit_on_the_tail_classes():
    """24 | 25: the backward's LDS tile at 1 / 2 / 4 heads; 32 | 33: the forward's, and the backward's at eight heads."""
    cls = {(n, h): T.tail_class(T.describe(_rec(T.chain(n))), h) for n in (24, 25, 32, 33) for h in (1, 2, 4, 8)}
    for h in (1, 2, 4):
        assert [cls[n, h] for n in (24, 25, 32, 33)] == [("lds", "lds"), ("lds", "global"), ("lds", "global"), ("global", "global")]
    assert [cls[n, 8] for n in (24, 25, 32, 33)] == [("lds", "lds"), ("lds", "lds"), ("lds", "lds"), ("global", "global")]


@pytest.mark.parametrize("sizes,frags,mec,nc", [((1, 5, 8), 14, 128, 64), ((3, 16), 19, 130, 65), ((8, 8), 16, 156, 78)])
def test_components_sit_on_the_tail_edge_class(sizes, frags, mec, nc):
    d = T.describe(_rec(T.components(sizes)))
    assert (d["frags"], d["mec"], d["nc"]) == (frags, mec, nc)
    if len(sizes) == 2:
        assert nc == (sizes[0] + 1) * (sizes[1] + 1) - 3
    else:
        assert sizes[0] == 1 and nc == (sizes[1] + 2) * (sizes[2] + 2) - 6
    assert T.tail_class(d, 4) == (("lds", "lds") if mec <= 128 else ("global", "global"))
    assert d["fbedges"] > 4000            # why these molecules cannot sit in a batch of the one-launch plan builder


@pytest.mark.parametrize("D", [3, 4, 8, 9, 13, 33])
def test_star_row_lengths(D):
    d = T.describe(_rec(T.star(D)))
    assert (d["atoms"], d["bonds"], d["frags"], d["mec"]) == (D + 1, 2 * D, 1, 1)
    assert (d["in_atom"], d["in_bond"], d["out_atom"], d["out_bond"]) == (D + 1, 2 * (D - 1), D + 1, 2 * (D - 1))
    assert d["bedges"] == 4 * D * (D - 1)
    c = T.describe(_rec(T.star(D, cut_all=True)))
    assert (c["frags"], c["nc"], c["mec"]) == (D + 1, D, 2 * D)
    assert (c["in_atom"], c["in_bond"], c["in_frag"], c["in_fbond"]) == (D + 1, 2 * (D - 1), D, 2 * (D - 1))
    assert (c["out_frag"], c["out_fbond"]) == (D, 2 * (D - 1))


def test_the_values_the_issue_table_names():
    assert T.describe(_rec(T.star(8)))["in_bond"] == 14 and T.describe(_rec(T.star(9)))["in_bond"] == 16
    d = T.describe(_rec(T.star(33, cut_all=True)))
    assert (d["frags"], d["mec"]) == (34, 66)
    assert [T.describe(_rec(T.chain(n)))["mec"] for n in (24, 25, 32, 33)] == [46, 48, 62, 64]


def test_two_atom_molecules():
    d = T.describe(_rec(T.two_atoms()))
    assert (d["atoms"], d["bonds"], d["bedges"], d["frags"], d["mec"], d["fbedges"]) == (2, 2, 2, 1, 1, 1)
    d = T.describe(_rec(T.two_atoms(cut=True)))
    assert (d["atoms"], d["bonds"], d["bedges"], d["frags"], d["mec"], d["fbedges"]) == (2, 2, 2, 2, 2, 2)


@pytest.mark.parametrize("heads", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["edges", "wide"])
def test_batches_hold_the_rows_and_classes_they_claim(name, heads):
    T.assert_batch_claims(name, T.BATCHES[name](), heads)


def test_edges_batch_fits_the_one_launch_plan_builder_and_wide_does_not():
    """The same arithmetic as plan.GraphPlan._build_mol, from the collate's per-molecule maxima (the pretrain plan has two more tasks)."""
    from fragnet_amd.plan import mol_plan_fits, mol_plan_slice_words
    tasks = [("bedge", "edge", 0)] * 2 + [("edge", "atom", 1)] * 2 + [("fbedge", "fedge", 0)] * 2 + [("fedge", "frag", 0)] * 2 + \
            [("atom", "frag", 0), ("atom", "mol", 0), ("frag", "mol", 0)] + [("edge", "atom", 0)] * 2
    fits = {}
    for name in ("edges", "wide"):
        m = T.collate(T.BATCHES[name]()).max_per_mol
        fits[name] = mol_plan_fits(sum(mol_plan_slice_words(m[i] + (m[n] if loops else 0), m[n]) for i, n, loops in tasks))
    assert fits == {"edges": True, "wide": False}


def test_pretrain_records_have_the_same_topology():
    for name in ("edges", "wide"):
        a, b = T.BATCHES[name](), T.BATCHES[name](pretrain_targets=True)
        assert [n for n, _ in a] == [n for n, _ in b]
        for (_, x), (_, y) in zip(a, b):
            assert torch.equal(x.edge_index, y.edge_index) and torch.equal(x.frag_index, y.frag_index) and y.bnd_angl is not None


@pytest.mark.parametrize("heads", [1, 4, 8])
@pytest.mark.parametrize("name", ["edges", "wide"])
def test_float32_oracle_is_a_hundred_times_closer_to_float64_than_the_gpu_tolerance(name, heads):
    """The GPU tests hold the engine to |got - ref| <= 1e-4 + 1e-4 |ref| against the float32 oracle.  On these very batches (rows of up
    to 66 in-edges, 128 on the bond graphs) the float32 oracle stays within a hundredth of that of the float64 oracle with the same
    weights -- logits and every gradient (measured: at most 3.4e-4 of the tolerance) -- so the bar is fair for the kernels at these
    row lengths and summation order on a long row is no excuse for missing it."""
    _, res = T.oracle_finetune(T.collate(T.BATCHES[name]()), heads)
    (l32, g32), (l64, g64) = res["f32"], res["f64"]
    assert set(g32) == set(g64) and len(g64) >= 30
    worst = 0.0
    for what, a, c in [("logits", l32, l64)] + [(n, g32[n], g64[n]) for n in g64]:
        ratio = float(((a.double() - c).abs() / (1e-4 + 1e-4 * c.abs())).max())
        worst = max(worst, ratio)
        assert ratio <= 0.01, f"{what}: float32 oracle off the float64 oracle by {ratio:.3g} of the tolerance"
    print(f"{name}, {heads} heads: worst |f32 - f64| / tolerance = {worst:.3e}")
