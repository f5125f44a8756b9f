"""Host checks of the factored pair batches (fragnet_amd/data.py: collate_fn_*_factored, pair_grid_batch, as_factored) and of
synth.pair_records: no GPU needed."""
import copy

import pytest
import torch

from fragnet_amd import data, synth
from fragnet_amd.plan import N_MOLS_KEY, CollatedBatch, batch_n_mols

KINDS = {"cdrp": (data.collate_fn_cdrp, data.collate_fn_cdrp_factored, "gene_expr"),
         "dta": (data.collate_fn_dta, data.collate_fn_dta_factored, "protein")}


def _expand(fb, key):
    """the second-input rows of the duplicated batch a factored one stands for"""
    return fb[key][fb["pair_second"]]


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_expanding_a_factored_batch_reproduces_the_duplicated_collate(kind):
    dup_fn, fac_fn, key = KINDS[kind]
    recs = synth.pair_records(33, 6, 4, kind, 11)
    fb, db = fac_fn(recs), dup_fn(recs)
    pd, ps = fb["pair_drug"], fb["pair_second"]
    assert pd.dtype == ps.dtype == torch.int64 and pd.shape == ps.shape == (33,)
    assert fb[N_MOLS_KEY] == 6 and fb[key].shape[0] == 4
    # order of first occurrence on both sides
    for pl in (pd, ps):
        firsts = [pl.tolist().index(v) for v in range(int(pl.max()) + 1)]
        assert firsts == sorted(firsts)
    assert torch.equal(fb["y"], db["y"])
    assert torch.equal(_expand(fb, key), db[key]) and fb[key].dtype == torch.int64
    # the U distinct drugs, collated the duplicated way in pair order, are the duplicated batch key by key (integers bit-exact)
    first = [pd.tolist().index(u) for u in range(6)]
    distinct = dup_fn([recs[i] for i in first])
    for k, v in distinct.items():
        if k in ("y", key):
            continue
        assert torch.equal(fb[k], v) and fb[k].dtype == v.dtype, k
    again = dup_fn([recs[first[u]] for u in pd.tolist()])
    for k, v in db.items():
        if k not in ("y", key):                              # (the second rows: _expand above)
            assert torch.equal(again[k], v) and again[k].dtype == v.dtype, k
    assert isinstance(fb, CollatedBatch) and fb.offsets.shape[1] == 7


def test_distinctness_is_decided_by_content():
    recs = synth.pair_records(4, 2, 2, "cdrp", 3)
    a = recs[0]
    b = copy.deepcopy(a)                                  # another object, equal content
    c = copy.deepcopy(a)
    c.smiles = "not looked at"
    d = copy.deepcopy(a)
    d.edge_attr = d.edge_attr.clone()
    d.edge_attr[0, 0] += 1.0                              # one value changed
    fb = data.collate_fn_cdrp_factored([a, b, c, d])
    assert fb["pair_drug"].tolist() == [0, 0, 0, 1] and fb[N_MOLS_KEY] == 2
    assert fb["pair_second"].tolist() == [0, 0, 0, 0] and fb["gene_expr"].shape[0] == 1


def test_cell_lines_are_distinct_after_the_truncating_cast():
    recs = synth.pair_records(2, 1, 1, "cdrp", 5)
    a, b, c = recs[0], copy.deepcopy(recs[0]), copy.deepcopy(recs[0])
    a.gene_expr = a.gene_expr.clone()
    a.gene_expr[:3] = torch.tensor([0.2, 2.9, -1.5])
    b.gene_expr = a.gene_expr.clone()
    b.gene_expr[:3] = torch.tensor([0.7, 2.1, -1.9])      # differs only below the int64 truncation: (0, 2, -1) both times
    c.gene_expr = a.gene_expr.clone()
    c.gene_expr[1] = 3.0
    fb = data.collate_fn_cdrp_factored([a, b, c])
    assert fb["pair_second"].tolist() == [0, 0, 1] and fb["gene_expr"].shape[0] == 2
    assert fb["gene_expr"][0, :3].tolist() == [0, 2, -1]


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_pair_orderings_are_stable_sorts_of_the_pair_lists(kind):
    fb = KINDS[kind][1](synth.pair_records(40, 5, 7, kind, 17))
    for side, n in (("pair_drug", 5), ("pair_second", 7)):
        pl, rowptr, perm = fb[side], fb[side + "_rowptr"], fb[side + "_perm"]
        assert rowptr.dtype == perm.dtype == torch.int32 and rowptr.shape == (n + 1,) and perm.shape == (40,)
        assert rowptr[0] == 0 and rowptr[-1] == 40
        for r in range(n):
            seg = perm[rowptr[r]:rowptr[r + 1]].tolist()
            assert seg == [m for m in range(40) if pl[m] == r]          # the pairs of row r, ascending


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_the_molecule_count_is_the_number_of_distinct_drugs(kind):
    dup_fn, fac_fn, _ = KINDS[kind]
    recs = synth.pair_records(12, 3, 2, kind, 23)
    fb = fac_fn(recs)
    assert fb["y"].shape[0] == 12 and batch_n_mols(fb) == 3 == int(fb["batch"].max()) + 1
    assert batch_n_mols(dup_fn(recs)) == 12 and N_MOLS_KEY not in dup_fn(recs)      # existing batches: unchanged
    moved = data.batch_to(fb, "cpu")
    assert batch_n_mols(moved) == 3 and isinstance(moved, CollatedBatch)
    assert batch_n_mols({k: v for k, v in fb.items()}) == 3                          # a plain dict of it (the trainers' _on) keeps the count
    af = data.as_factored(dup_fn(recs))
    assert batch_n_mols(af) == 12 and af["pair_drug"].tolist() == list(range(12)) == af["pair_second"].tolist()
    assert af["pair_drug_rowptr"].tolist() == list(range(13)) and af["pair_drug_perm"].tolist() == list(range(12))


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
def test_pair_grid_batch(kind):
    dup_fn, _, key = KINDS[kind]
    recs = synth.pair_records(6, 3, 4, kind, 29)
    rows = [getattr(r, key) for r in recs[:5]]
    g = data.pair_grid_batch(recs[:3], rows, kind)
    assert "y" not in g and "pair_drug" not in g and g[data.PAIR_GRID_KEY] is True and batch_n_mols(g) == 3
    assert torch.equal(g[key], dup_fn(recs[:5])[key]) and g[key].dtype == torch.int64
    assert torch.equal(g["x_atoms"], dup_fn(recs[:3])["x_atoms"])
    g2 = data.pair_grid_batch(recs[:3], dup_fn(recs[:5])[key], kind)              # a [C, n] tensor instead of a list of rows
    assert torch.equal(g2[key], g[key])
    with pytest.raises(ValueError):
        data.pair_grid_batch(recs[:3], rows, "other")


@pytest.mark.parametrize("kind", ["cdrp", "dta"])
@pytest.mark.parametrize("n_pairs,n_drugs,n_seconds", [(7, 3, 3), (33, 6, 4), (20, 20, 1), (16, 1, 16)])
def test_pair_records_repeat_exactly_the_requested_inputs(kind, n_pairs, n_drugs, n_seconds):
    dup_fn, fac_fn, key = KINDS[kind]
    recs = synth.pair_records(n_pairs, n_drugs, n_seconds, kind, 31)
    assert len(recs) == n_pairs and len({id(r) for r in recs}) == n_pairs and len({id(r.x_atoms) for r in recs}) == n_pairs
    fb = fac_fn(recs)
    assert fb[N_MOLS_KEY] == n_drugs and fb[key].shape[0] == n_seconds
    assert len(set(fb["pair_drug"].tolist())) == n_drugs and len(set(fb["pair_second"].tolist())) == n_seconds
    again = synth.pair_records(n_pairs, n_drugs, n_seconds, kind, 31)
    assert torch.equal(fac_fn(again)["y"], fb["y"])
    with pytest.raises(ValueError):
        synth.pair_records(2, 3, 1, kind, 0)


def test_dta_factored_collate_keeps_the_token_check():
    recs = synth.pair_records(4, 2, 2, "dta", 37)
    recs[2].protein = recs[2].protein.clone()
    recs[2].protein[5] = 26.0
    with pytest.raises(ValueError, match="protein tokens"):
        data.collate_fn_dta_factored(recs)
    with pytest.raises(ValueError, match="protein tokens"):
        data.pair_grid_batch(recs[:1], [recs[2].protein], "dta")


def test_factored_ops_refuse_cpu_tensors():
    from fragnet_amd import _lib, ops
    fc1, fc2 = torch.nn.Linear(512, 128), torch.nn.Linear(128, 1)
    d, s = torch.zeros(2, 256), torch.zeros(3, 256)
    pd, ps = torch.tensor([0, 1, 1]), torch.tensor([2, 0, 1])
    with pytest.raises(_lib.FragnetHipError):
        ops.pair_head_factored(d, s, pd, ps, fc1, fc2)
    with pytest.raises(_lib.FragnetHipError):
        ops.pair_head_grid(d, s, fc1, fc2)
    fc1x = torch.nn.Linear(556, 128)
    with pytest.raises(_lib.FragnetHipError):
        ops.pair_head_dta_factored(d, torch.zeros(3, 300), pd, ps, fc1x, fc2)
    with pytest.raises(_lib.FragnetHipError):
        ops.pair_head_dta_grid(d, torch.zeros(3, 300), fc1x, fc2)
