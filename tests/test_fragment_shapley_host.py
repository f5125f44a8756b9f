"""Host side of the fragment Shapley values (fragnet_amd/attribution.py ``fragment_shapley``): the weight templates, the axioms on
hand-made set functions, the permutation draw and its reduction, the chunk planner, the refusals and the fixture
tests/golden/frag_shapley.npz's own consistency.  A set function on F groups is an array [2^F, C] whose row index is the mask."""
import itertools

import numpy as np
import pytest
import torch

from tests import attr_common as ac
from tests import fragshap_common as sc


def _table_evaluator(tables):
    """``evaluate`` of attribution._shapley_host over per-molecule tables: rows are looked up by (molecule, mask); records the calls."""
    calls = []

    def evaluate(b, e, row_mol, row_mask):
        assert row_mol.dtype == np.int32 and row_mask.dtype == np.uint64 and (np.diff(row_mol) >= 0).all()
        assert row_mol.min() >= 0 and row_mol.max() < e - b
        calls.append((b, e, row_mol.copy(), row_mask.copy()))
        return np.stack([tables[b + int(m)][int(k)] for m, k in zip(row_mol, row_mask)])
    return evaluate, calls


def _random_tables(counts, C=2, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(1 << int(F), C)) for F in counts]


# ------------------------------------------------------------------------------------------------ the weights
@pytest.mark.parametrize("F", [1, 2, 3, 4, 5])
def test_weight_templates_against_all_orders(F):
    from fragnet_amd import attribution as attr
    v = np.random.default_rng(F).normal(size=(3, 1 << F, 2))
    phi = attr.shapley_exact(v, F)
    assert phi.shape == (3, F, 2) and phi.dtype == np.float64
    for m in range(3):
        np.testing.assert_allclose(phi[m], sc.by_orders(v[m], F), rtol=0, atol=1e-12)
    without, with_f, w = attr.shapley_weights(F)
    assert without.shape == with_f.shape == w.shape == (F, 1 << (F - 1))
    np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-15)          # a group's weights sum to 1
    assert ((with_f ^ without) == (1 << np.arange(F))[:, None]).all()
    assert attr.shapley_weights(F) is attr.shapley_weights(F), "one template per F, cached"


def test_the_axioms_on_hand_made_set_functions():
    from fragnet_amd import attribution as attr
    F = 4
    masks = np.arange(1 << F)
    bit = lambda f: ((masks >> f) & 1).astype(np.float64)
    # groups 0 and 1 interchangeable (v depends on them through their count only), group 3 without effect, all non-additive
    pair = bit(0) + bit(1)
    v = (np.tanh(pair + 2.0 * bit(2)) + 0.3 * pair * bit(2) + 0.7)[:, None] * np.array([1.0, -2.5])
    phi = attr.shapley_exact(v[None], F)[0]
    np.testing.assert_allclose(phi.sum(axis=0), v[-1] - v[0], rtol=0, atol=1e-14)          # efficiency
    np.testing.assert_allclose(phi[0], phi[1], rtol=0, atol=1e-15)                       # symmetry
    assert (phi[3] == 0.0).all(), "a group without effect gets exactly 0"
    assert (np.abs(phi[:3]) > 0.05).all()
    # an additive function: the Shapley value is the leave-one-out difference
    w = np.array([0.5, -1.0, 2.0, 0.25])
    add = (sum(w[f] * bit(f) for f in range(F)) + 3.0)[:, None]
    np.testing.assert_allclose(attr.shapley_exact(add[None], F)[0][:, 0], w, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------ sampled mode
def test_all_permutations_reproduce_exact_mode():
    from fragnet_amd import attribution as attr
    counts = [3, 1, 4, 5, 0]
    tables = _random_tables(counts)
    evaluate, _ = _table_evaluator(tables)
    exact = attr._shapley_host(counts, evaluate)
    assert exact["exact"].all() and not exact["stderr"].any()
    every = {i: np.array(list(itertools.permutations(range(F))), dtype=np.int64).reshape(-1, F) for i, F in enumerate(counts) if F}
    sampled = attr._shapley_host(counts, evaluate, permutations=every)
    assert sampled["exact"].tolist() == [False, False, False, False, True]
    np.testing.assert_allclose(sampled["phi"], exact["phi"], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(sampled["pred"], exact["pred"])
    np.testing.assert_array_equal(sampled["base"], exact["base"])
    first = np.concatenate([[0], np.cumsum(counts)])
    for i, F in enumerate(counts):
        np.testing.assert_allclose(exact["phi"][first[i]: first[i + 1]], sc.by_orders(tables[i], F) if F else np.zeros((0, 2)), rtol=0, atol=1e-12)
        np.testing.assert_array_equal(exact["pred"][i], tables[i][-1])
        np.testing.assert_array_equal(exact["base"][i], tables[i][0])


def test_the_draw_is_antithetic_and_the_rows_are_prefixes():
    from fragnet_amd import attribution as attr
    perms = attr.draw_permutations(7, 10, seed=3, molecule=5)
    assert perms.shape == (10, 7) and (np.sort(perms, axis=1) == np.arange(7)).all()
    np.testing.assert_array_equal(perms[1::2], perms[0::2, ::-1])
    assert len({tuple(p) for p in perms[0::2].tolist()}) > 1
    np.testing.assert_array_equal(perms, attr.draw_permutations(7, 10, seed=3, molecule=5))
    assert (perms != attr.draw_permutations(7, 10, seed=3, molecule=6)).any() and (perms != attr.draw_permutations(7, 10, seed=4, molecule=5)).any()
    masks = attr.permutation_masks(perms)
    assert masks.dtype == np.uint64 and masks.shape == (2 + 10 * 6,) and masks[0] == 0 and masks[1] == 127
    rows = masks[2:].reshape(10, 6)
    for k in range(10):
        assert rows[k].tolist() == [sum(1 << int(g) for g in perms[k, : j + 1]) for j in range(6)]
    # a pair's interior prefixes are complements of each other: prefix j of the reverse = all but prefix F - 2 - j
    np.testing.assert_array_equal(rows[1::2], np.uint64(127) ^ rows[0::2, ::-1])
    # bit 63 is a bit like any other
    wide = attr.permutation_masks(np.arange(64, dtype=np.int64)[None, ::-1])
    assert wide[1] == np.uint64(2 ** 64 - 1) and wide[2] == np.uint64(1 << 63) and wide.shape == (2 + 63,)


def test_sampled_values_are_efficient_and_carry_a_standard_error():
    from fragnet_amd import attribution as attr
    counts = [12]
    rng = np.random.default_rng(1)
    w = rng.normal(size=12)

    def evaluate(b, e, row_mol, row_mask):          # a smooth non-additive function of the mask, computed on demand (2^12 rows are not stored)
        bits = ((row_mask[:, None] >> np.arange(12, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)
        return np.tanh(bits @ w)[:, None]
    r = attr._shapley_host(counts, evaluate, samples=64, seed=9, return_values=True)
    assert not r["exact"][0] and r["rows"].tolist() == [2 + 64 * 11]
    np.testing.assert_allclose(r["phi"].sum(axis=0), r["pred"][0] - r["base"][0], rtol=0, atol=1e-12)      # every permutation telescopes
    assert (r["stderr"] > 0).all() and (r["stderr"] < 0.2).all()
    perms = attr.draw_permutations(12, 64, 9, 0)
    np.testing.assert_array_equal(r["values"][0]["mask"], attr.permutation_masks(perms))
    # the standard error over the 32 pair means, recomputed by hand
    v = {int(m): float(x) for m, x in zip(r["values"][0]["mask"], r["values"][0]["value"][:, 0])}
    marg = np.zeros((64, 12))
    for k, p in enumerate(perms.tolist()):
        m = 0
        for g in p:
            marg[k, g] = v[m | (1 << g)] - v[m]
            m |= 1 << g
    pairs = 0.5 * (marg[0::2] + marg[1::2])
    np.testing.assert_allclose(r["phi"][:, 0], marg.mean(axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["stderr"][:, 0], pairs.std(axis=0, ddof=1) / np.sqrt(32), rtol=0, atol=1e-12)


def test_a_molecule_s_answer_does_not_depend_on_batching_neighbours_or_the_row_budget():
    from fragnet_amd import attribution as attr
    counts = [3, 7, 2, 6, 7]
    tables = _random_tables(counts, seed=4)
    evaluate, calls = _table_evaluator(tables)
    kw = dict(exact_max=4, samples=8, seed=2)
    one = attr._shapley_host(counts, evaluate, **kw)
    assert len(calls) == 1 and one["exact"].tolist() == [True, False, True, False, False]
    for other in (dict(batch_size=2), dict(batch_size=1), dict(max_rows=60), dict(max_rows=50, batch_size=3)):
        calls.clear()
        two = attr._shapley_host(counts, evaluate, **kw, **other)
        assert len(calls) > 1
        for k in ("phi", "stderr", "pred", "base", "exact"):
            np.testing.assert_array_equal(two[k], one[k])
    # other neighbours, the same index: molecule 1 (F = 7) keeps its draw and its values
    counts2 = [5, 7, 1]
    evaluate2, _ = _table_evaluator([_random_tables([5], seed=8)[0], tables[1], _random_tables([1], seed=9)[0]])
    moved = attr._shapley_host(counts2, evaluate2, **kw)
    np.testing.assert_array_equal(moved["phi"][5:12], one["phi"][3:10])
    np.testing.assert_array_equal(moved["stderr"][5:12], one["stderr"][3:10])
    # another index or another seed: another draw
    assert (attr._shapley_host(counts, evaluate, exact_max=4, samples=8, seed=3)["phi"][3:10] != one["phi"][3:10]).any()
    assert (one["phi"][3:10] != one["phi"][18:25]).any()


# ------------------------------------------------------------------------------------------------ refusals and the planner
def test_refusals_of_the_design():
    from fragnet_amd import attribution as attr
    evaluate, calls = _table_evaluator([])
    with pytest.raises(ValueError, match="molecule 1 has 65 groups"):
        attr._shapley_host([3, 65], evaluate)
    for samples in (7, 0, -2):
        with pytest.raises(ValueError, match="samples must be even"):
            attr._shapley_host([3], evaluate, samples=samples)
    with pytest.raises(ValueError, match=r"permutations\[0\]"):
        attr._shapley_host([3], evaluate, permutations={0: np.array([[0, 1, 1]])})
    with pytest.raises(ValueError, match=r"permutations\[0\]"):
        attr._shapley_host([3], evaluate, permutations={0: np.array([[0, 1]])})
    with pytest.raises(ValueError, match="names molecule 4"):
        attr._shapley_host([3], evaluate, permutations={4: np.array([[0, 1, 2]])})
    with pytest.raises(ValueError, match="molecule 1 alone needs 1024 coalition rows"):
        attr._shapley_host([3, 10], evaluate, max_rows=1000)
    assert not calls, "refused before anything is evaluated"
    # 64 groups are fine (sampled): the full mask has all 64 bits
    mode, given, rows = attr.coalition_design([64], samples=2)
    assert mode.tolist() == ["sampled"] and not given and rows.tolist() == [2 + 2 * 63]


def test_the_planner_keeps_molecules_whole_and_within_the_budget():
    from fragnet_amd import attribution as attr
    rng = np.random.default_rng(0)
    rows = rng.integers(1, 200, size=300)
    for batch_size, max_rows in ((512, 1000), (7, 1000), (3, 199), (1, 10 ** 6), (512, 10 ** 6)):
        chunks = attr.plan_coalition_chunks(rows, batch_size, max_rows)
        assert chunks[0][0] == 0 and chunks[-1][1] == 300 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        for b, e in chunks:
            assert 0 < e - b <= batch_size and rows[b:e].sum() <= max_rows
        # greedy: a chunk ends only where the next molecule would not fit
        for (b, e), (_, e2) in zip(chunks, chunks[1:]):
            assert e - b == batch_size or rows[b: e + 1].sum() > max_rows
    assert attr.plan_coalition_chunks([], 4, 10) == []
    assert attr.plan_coalition_chunks([10], 4, 10) == [(0, 1)]
    with pytest.raises(ValueError, match="molecule 2 alone needs 11"):
        attr.plan_coalition_chunks([1, 2, 11], 4, 10)
    with pytest.raises(ValueError, match="positive"):
        attr.plan_coalition_chunks([1], 0, 10)


def test_cpu_models_and_cpu_tensors_are_refused():
    from fragnet_amd import _lib, attribution as attr, ops
    from fragnet_amd.model import FragNetFineTune
    mols = ac.molecules(2)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        attr.fragment_shapley(FragNetFineTune(**ac.CTOR), mols)
    with pytest.raises(ValueError, match="Linear is not one of"):
        attr.fragment_shapley(torch.nn.Linear(2, 2), mols)
    with pytest.raises(ValueError, match="one array per molecule"):
        attr.fragment_shapley(FragNetFineTune(**ac.CTOR), mols, groups=[np.zeros(3, dtype=np.int64)])
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        ops.pool_cat_coalitions(torch.zeros(3, 128), torch.zeros(1, 128), None, torch.zeros(3, dtype=torch.int8),
                                torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64))


def test_atom_bits_are_positions_among_the_molecule_s_groups():
    from fragnet_amd import attribution as attr
    flat = np.array([5, -1, 2, 5, -7, 4, -1, -1, 7, 0, 7], dtype=np.int64)
    atom_off = np.array([0, 6, 8, 11], dtype=np.int64)
    bits = attr.atom_bits(flat, atom_off, attr.flat_group_table(flat, atom_off))
    assert bits.dtype == np.int8 and bits.tolist() == [2, -1, 0, 2, -1, 1, -1, -1, 1, 0, 1]
    big = flat * 10 ** 12          # ids that take flat_group_table's sorting path
    assert attr.atom_bits(big, atom_off, attr.flat_group_table(big, atom_off)).tolist() == bits.tolist()
    with pytest.raises(ValueError, match="molecule 0 has 65 groups"):
        many = np.arange(65, dtype=np.int64)
        attr.atom_bits(many, np.array([0, 65]), attr.flat_group_table(many, np.array([0, 65])))


def test_the_result_class():
    from fragnet_amd.attribution import FragmentShapley
    atom_group = np.array([2, -1, 0, 2, 0, -1, -1, 4, 4, 4], dtype=np.int64)
    phi = np.array([[0.5, 1.0], [0.75, -2.0], [2.0, -10.0]])
    res = FragmentShapley(np.ones((3, 2), np.float32), np.zeros((3, 2), np.float32), np.array([0, 2, 2, 3]), np.array([0, 2, 4]), np.array([2, 2, 3]),
                          phi, np.zeros_like(phi), np.array([True, True, False]), atom_group, np.array([0, 5, 7, 10]))
    assert len(res) == 3 and res[0]["group"].tolist() == [0, 2] and res[1]["phi"].shape == (0, 2) and res[-1]["exact"] is False
    with pytest.raises(IndexError):
        res[3]
    np.testing.assert_array_equal(res.atom_weights(0), [[0.75, -2.0], [0.0, 0.0], [0.5, 1.0], [0.75, -2.0], [0.5, 1.0]])
    np.testing.assert_array_equal(res.atom_weights(1), np.zeros((2, 2)))
    np.testing.assert_array_equal(res.atom_weights(2), [[2.0, -10.0]] * 3)
    assert sorted(res.arrays()) == ["atom_group", "atom_offsets", "base", "exact", "group", "n_atoms", "offsets", "phi", "pred", "stderr"]


# ------------------------------------------------------------------------------------------------ the fixture itself
@pytest.mark.parametrize("case", sc.CASES)
def test_the_fixture_s_shapley_values_matter_and_follow_from_its_values(case):
    from fragnet_amd import attribution as attr
    mask, value, phi, groups = sc.reference(case)
    assert mask.shape == (sc.ROWS[case], 2) and value.shape[0] == sc.ROWS[case] and phi.shape == (sum(groups), value.shape[1])
    assert phi.dtype == np.float64 and value.dtype == np.float32 and mask.dtype == np.int64
    big, entries = sc.share_above_tolerance(case)
    print(f"{case}: {big}/{entries} reference Shapley values above 10 x tolerance")
    assert big / entries >= sc.MIN_SHARE[case]
    first = 0
    for i, F in enumerate(groups):
        rows = mask[:, 0] == i
        np.testing.assert_array_equal(mask[rows, 1], np.arange(1 << F))          # molecule-major, the row index is the mask
        v = value[rows]
        np.testing.assert_allclose(phi[first: first + F], sc.by_orders(v, F), rtol=0, atol=1e-12)
        np.testing.assert_allclose(phi[first: first + F], attr.shapley_exact(v[None], F)[0], rtol=0, atol=1e-12)
        np.testing.assert_allclose(phi[first: first + F].sum(axis=0), v[-1].astype(np.float64) - v[0], rtol=0, atol=1e-12)
        first += F


def test_the_fixture_continues_the_leave_one_out_fixture():
    """Same models and molecules as tests/golden/frag_attr.npz: the full row is its pred_no_mask, the all-but-one rows its pred_mask."""
    from tests import fragattr_common as fc
    for case in sc.CASES:
        mask, value, _, groups = sc.reference(case)
        base, rep, pm = fc.reference(case)
        for i, F in enumerate(groups):
            v = value[mask[:, 0] == i]
            fc.close(v[-1], base[i], f"{case}: v(all) of molecule {i}")
            fc.close(v[((1 << F) - 1) ^ (1 << np.arange(F))], pm[rep[:, 0] == i], f"{case}: all-but-one rows of molecule {i}")
