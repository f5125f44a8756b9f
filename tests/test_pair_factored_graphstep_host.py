"""CPU-side checks of the captured factored pair step's surface (graphstep.FactoredPairShapes, factored_batch_counts,
pad_factored_pair_batch, FACTORED_PAIR_FIELDS; train.check_factored_pair_graph_step): capacity sizing and ``fits`` for the two index
spaces a factored batch adds, the torch counterpart of the staging launch, the size of the staging table, and the drivers' key."""
import pytest
import torch

from fragnet_amd import _lib, data, graphstep, plan, train
from tests import pair_factored_step_helpers as F
from tests import pair_step_helpers as H


@pytest.fixture(scope="module", params=H.KINDS)
def case(request):
    return (request.param,) + F.batches(request.param)


def test_counts_take_the_molecule_count_the_batch_carries(case):
    kind, small, _, _ = case
    for b, (M, U, C) in zip(small, F.SMALL):
        c = graphstep.factored_batch_counts(b)
        assert (c["pair"], c["mol"], c["second"]) == (M, U, C)
        assert graphstep.batch_counts(b)["mol"] == M                       # the property step's count reads y: one entry per PAIR
        assert {k: v for k, v in c.items() if k not in ("mol",) + graphstep.PAIR_SPACES} == \
            {k: v for k, v in graphstep.batch_counts(b).items() if k != "mol"}
        assert c["atom"] == b["x_atoms"].shape[0] and b[plan.N_MOLS_KEY] == U


def test_capacities_of_the_two_new_spaces_and_the_mol_padding_rule(case):
    kind, small, big, shapes = case
    M, U, C = (max(s[i] for s in F.SMALL) for i in range(3))
    assert shapes.pair_cap == 16 and shapes.second_cap == 8                # max + 5 %, rounded up to 8
    assert shapes.capacity("pair") == 16 and shapes.capacity("second") == 8 and shapes.capacity("atom") == shapes.cap["atom"]
    assert set(shapes.cap) == set(plan.SPACES) == set(shapes.pad_info()["cap"])      # the plan builder's tables: the encoder's spaces alone
    real = shapes.cap["mol"] - shapes.slack["mol"]
    assert real == 8 and shapes.cap["mol"] % 8 == 0                        # ceil(7 * 1.05) distinct drugs fit; the rest is slack
    lim = dict(graphstep._pairs(shapes.heads))["mol"]
    for b in small:                                                        # StaticShapes.fits' rule: the padding items find padding molecules
        c = graphstep.factored_batch_counts(b)
        assert shapes.fits(c, b.max_per_mol)
        for item, per in lim:
            assert shapes.cap[item] - c[item] <= per * shapes.slack["mol"]
    assert not shapes.fits(graphstep.factored_batch_counts(big), big.max_per_mol)
    c = graphstep.factored_batch_counts(small[0])
    assert shapes.fits(dict(c, pair=16)) and not shapes.fits(dict(c, pair=17))
    assert shapes.fits(dict(c, second=8)) and not shapes.fits(dict(c, second=9))
    assert shapes.fits(dict(c, mol=real)) and not shapes.fits(dict(c, mol=real + 1))
    assert shapes.fits({k: v for k, v in c.items() if k not in graphstep.PAIR_SPACES})       # pad_batch asks with the encoder's seven


def test_pad_factored_pair_batch(case):
    kind, small, big, shapes = case
    key = H.SECOND[kind]
    for b in small:
        c = graphstep.factored_batch_counts(b)
        padded = graphstep.pad_factored_pair_batch(b, shapes)
        assert padded[plan.N_MOLS_KEY] == shapes.cap["mol"] and plan.batch_n_mols(padded) == shapes.cap["mol"]
        assert not any(k in padded for k in data.PAIR_ORDER_KEYS)
        for name, n, cap in (("y", c["pair"], 16), (data.PAIR_DRUG_KEY, c["pair"], 16), (data.PAIR_SECOND_KEY, c["pair"], 16), (key, c["second"], 8)):
            assert padded[name].shape == (cap,) + tuple(b[name].shape[1:]) and padded[name].dtype == b[name].dtype
            assert torch.equal(padded[name][:n], b[name]) and not bool(padded[name][n:].any()), name
        assert float(padded[graphstep.MASK_KEY].sum()) == c["mol"] and padded[graphstep.MASK_KEY].shape == (shapes.cap["mol"],)
        assert padded["x_atoms"].shape[0] == shapes.cap["atom"] and torch.equal(padded["x_atoms"][: c["atom"]], b["x_atoms"])
        assert padded["batch"].shape == (shapes.cap["atom"],) and int(padded["batch"][c["atom"]:].min()) >= shapes.cap["mol"] - shapes.slack["mol"]
        assert padded.offsets.shape == (len(plan.SPACES), shapes.cap["mol"] + 1)
    with pytest.raises(ValueError, match="does not fit"):
        graphstep.pad_factored_pair_batch(big, shapes)


def test_staging_table_stays_within_its_forty_fields(case):
    kind, small, _, _ = case
    table = {**graphstep.FIELDS, **graphstep.FACTORED_PAIR_FIELDS}
    assert list(table)[: len(graphstep.FIELDS)] == list(graphstep.FIELDS)          # y keeps its place; FIELDS itself is untouched
    assert graphstep.FIELDS["y"] == ("mol", "rows", None) and table["y"][0] == "pair"
    assert table[H.SECOND[kind]] == ("second", "rows_i64", None)
    assert table[data.PAIR_DRUG_KEY][:2] == table[data.PAIR_SECOND_KEY][:2] == ("pair", "vec_i64")
    staged = [n for n in table if n in small[0]]
    assert len(staged) == 19                                               # 15 encoder fields, y, the second input, two pair lists
    static = len(staged) + len(graphstep.MASKS) + 2 + 1                    # + the masks, the two counts, the offsets table
    bumps, zero_regions = 2, 8                                             # Philox and Adam words; room for the captured plans' workspaces
    assert static == 25 and static + bumps + zero_regions <= _lib.FN_MAX_STAGE_FIELDS == 40


def test_drivers_key_and_its_refusal():
    assert train.check_factored_pair_graph_step({}) is False
    assert train.check_factored_pair_graph_step({"factored_graph_step": False, "graph_step": True}) is False
    assert train.check_factored_pair_graph_step({"factored_graph_step": True}) is True
    assert train.check_factored_pair_graph_step({"factored_graph_step": True, "factored_pairs": True}) is True
    with pytest.raises(SystemExit, match="finetune.factored_graph_step.*finetune.graph_step"):
        train.check_factored_pair_graph_step({"factored_graph_step": True, "graph_step": True})
    # the old check is as it was
    assert train.check_pair_graph_step({}) is False and train.check_pair_graph_step({"graph_step": True}) is True
    assert train.check_pair_graph_step({"graph_step": True, "factored_graph_step": True}) is True
    with pytest.raises(SystemExit, match="finetune.graph_step.*finetune.factored_pairs"):
        train.check_pair_graph_step({"graph_step": True, "factored_pairs": True})


def test_step_class_is_a_sibling_on_the_same_machinery():
    cls = graphstep.FactoredPairGraphedTrainStep
    assert issubclass(cls, graphstep.PairGraphedTrainStep)
    for name in ("_capture", "replay", "__call__", "_eager", "_fwd_bwd_static", "_sync_adam_state"):
        assert name not in vars(cls), name
    assert graphstep.PairGraphedTrainStep.EXTRA_FIELDS is graphstep.PAIR_FIELDS           # the sibling stages what it staged
    assert _lib.ABI_VERSION == 12 and _lib.FN_MAX_STAGE_FIELDS == 40
