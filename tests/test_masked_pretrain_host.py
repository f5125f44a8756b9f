"""Masked-atom pretraining (model_version gat2_masked2), the parts that need no GPU: the selection rule's restatement
(tests/row_sample_ref.py), the fixtures of tests/golden/make_golden_masked.py against the oracle, the model classes' keys and
weights, and the driver's dispatch on ``model_version``."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import row_sample_ref as rs
from tests.conftest import ROOT
from tests.helpers import GOLDEN, check_grads, check_params_match, load_case

CASES = ["pt_masked2_b4", "pt_masked2_edge6"]
NAMES = ("bond_length", "bond_angle", "dihedral", "graph_rep")


@pytest.mark.parametrize("keep_frac", [0.0, 0.5, 0.85, 1.0])
def test_exact_count_for_every_n(keep_frac):
    rng = np.random.default_rng(5)
    for n in range(301):
        keys = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        out = rs.select(keys, keep_frac)
        assert int(out.sum()) == int(n * keep_frac) == rs.count(n, keep_frac), n
        # padding rows are kept and do not count
        padded = rs.select(np.concatenate([keys, np.zeros(7, dtype=np.uint32)]), keep_frac, n=n)
        assert np.array_equal(padded[:n], out) and bool(padded[n:].all())


def test_count_is_pythons_int_of_the_double_product():
    assert rs.count(102, 0.85) == 86 and rs.count(93, 0.85) == 79 and rs.count(20, 0.85) == 17 and rs.count(40, 0.85) == 34


def test_equal_keys_keep_the_first_rows():
    for n, kf in ((1, 0.85), (2, 0.85), (40, 0.85), (257, 0.5)):
        out = rs.select(np.full(n, 0xDEADBEEF, dtype=np.uint32), kf)
        k = int(n * kf)
        assert bool(out[:k].all()) and not bool(out[k:].any())


def test_ties_at_the_pivot_are_broken_by_row_index():
    keys = np.array([5, 3, 5, 3, 5, 3, 9, 5], dtype=np.uint32)
    # k = 5: the three 3s, then the 5s of rows 0 and 2
    assert rs.select(keys, 5 / 8).tolist() == [1, 1, 1, 1, 0, 1, 0, 0]


def test_inclusion_frequency_is_uniform():
    """400 fixed seeds at n = 40 (k = 34): every row's keep count within six binomial standard deviations of 400 * 34 / 40."""
    n, seeds = 40, range(1000, 1400)
    hits = np.zeros(n)
    for s in seeds:
        out = rs.sample(n, 0.85, seed=s, offset=3 * s)
        assert int(out.sum()) == 34
        hits += out
    p, m = 34 / 40, len(seeds)
    sd = np.sqrt(m * p * (1 - p))
    assert float(np.abs(hits - m * p).max()) <= 6 * sd, (hits.min(), hits.max(), m * p, sd)


def test_sampler_key_convention():
    """the key of row i is word i % 4 of block offset + i // 4; consecutive draws of (cap + 3) // 4 blocks share none"""
    from tests import philox_ref
    k = rs.keys(10, seed=77, offset=5)
    blocks = philox_ref.philox4x32(np.arange(5, 8, dtype=np.uint64), 77, philox_ref.ROUNDS)
    assert np.array_equal(k, blocks.reshape(-1)[:10])
    assert not np.array_equal(rs.keys(8, 77, 5), rs.keys(8, 77, 7))


@pytest.mark.parametrize("case", CASES)
def test_oracle_on_gated_input_reproduces_the_fixture(case):
    """The reference's FragNetPreTrainMasked2 is its FragNetPreTrain on x_atoms with the masked rows zeroed: the oracle, at
    tests/test_oracle_golden.py's tolerances."""
    from oracle import fragnet_ref as ref
    torch.set_num_threads(1)
    cfg, batch, out, grads, pkeys, psums = load_case(case)
    z = np.load(os.path.join(GOLDEN, case + ".npz"))
    keep = torch.from_numpy(z["keep_atoms"])
    n = batch["x_atoms"].shape[0]
    assert keep.dtype == torch.uint8 and keep.shape == (n,) and int(keep.sum()) == int(n * 0.85)
    torch.manual_seed(cfg["seed"])
    model = ref.FragNetPreTrain(**cfg["ctor"])
    check_params_match(model, pkeys, psums)
    model.train()
    gated = dict(batch)
    gated["x_atoms"] = batch["x_atoms"] * keep[:, None].float()
    outs = model(gated)
    for nm, t in zip(NAMES, outs):
        torch.testing.assert_close(t.detach(), torch.from_numpy(out[nm]), atol=2e-6, rtol=1e-5)
    loss = ref.pretrain_loss(outs, gated)
    assert abs(float(loss) - float(out["loss"])) < 1e-5
    loss.backward()
    check_grads(model, grads, atol=1e-6, rtol=1e-4)
    # and the unmasked outputs the fixture carries are the oracle's on the original batch, far from the masked ones
    torch.manual_seed(cfg["seed"])
    plain = ref.FragNetPreTrain(**cfg["ctor"])
    plain.train()
    worst = 0.0
    for nm, t in zip(NAMES, plain(batch)):
        torch.testing.assert_close(t.detach(), torch.from_numpy(z[f"out_unmasked/{nm}"]), atol=2e-6, rtol=1e-5)
        worst = max(worst, float(np.abs(z[f"out_unmasked/{nm}"] - out[nm]).max()))
    assert worst >= 10 * 1e-4 and abs(worst - cfg["masked_vs_unmasked"]) < 1e-6


@pytest.mark.parametrize("case", CASES)
def test_masked_classes_have_the_plain_models_keys_and_weights(case):
    from fragnet_amd import model as M
    cfg, _, _, _, pkeys, psums = load_case(case)
    for cls in (M.FragNetPreTrainMasked2, M.FragNetPreTrainMasked):
        torch.manual_seed(cfg["seed"])
        m = cls(**cfg["ctor"])
        after_masked = torch.rand(3)
        check_params_match(m, pkeys, psums)
        torch.manual_seed(cfg["seed"])
        plain = M.FragNetPreTrain(**cfg["ctor"])
        after_plain = torch.rand(3)
        assert list(m.state_dict()) == list(plain.state_dict())
        assert torch.equal(after_masked, after_plain)          # the same RNG consumption


def test_masked2_constructor_and_mask_stream():
    import inspect
    from fragnet_amd import model as M, ops
    want = ["num_layer", "drop_ratio", "num_heads", "emb_dim", "atom_features", "frag_features", "edge_features", "fedge_in", "fbond_edge_in"]
    sig = inspect.signature(M.FragNetPreTrainMasked2.__init__)
    plain = inspect.signature(M.FragNetPreTrain.__init__)
    names = list(sig.parameters)[1:]
    assert names == want + ["mask_ratio"] and sig.parameters["mask_ratio"].default == 0.15
    assert [sig.parameters[k].default for k in want] == [plain.parameters[k].default for k in want]
    m = M.FragNetPreTrainMasked2(num_layer=1)
    assert m.keep_frac == 0.85 and isinstance(m.mask_rng, ops.PhiloxStream) and m.mask_rng is not m.pretrain.rng
    # a stream of its own: another key than the dropout stream's under the same torch seed and rank, and rank-aware
    torch.manual_seed(9)
    s_mask, _ = ops.mask_stream(rank=0).take(4)
    s_mask1, _ = ops.mask_stream(rank=1).take(4)
    s_drop, _ = ops.PhiloxStream(rank=0).take(4)
    assert len({s_mask, s_mask1, s_drop}) == 3
    with pytest.raises(ValueError):
        M.FragNetPreTrainMasked2(num_layer=1, mask_ratio=1.5)
    with pytest.raises(NotImplementedError, match=r"pretrain_heads\.py:174-184"):
        M.FragNetPreTrainMasked(num_layer=1)({})


def test_cpu_batches_are_refused_not_masked_on_the_host():
    from fragnet_amd import _lib, data, synth
    from fragnet_amd.model import FragNetPreTrainMasked2
    batch = data.collate_fn_pt(synth.synth_molecules(2, seed=1, pretrain_targets=True))
    with pytest.raises(_lib.FragnetHipError):
        FragNetPreTrainMasked2(num_layer=1)(batch)


def _driver():
    spec = importlib.util.spec_from_file_location("pretrain_gat2_driver", os.path.join(ROOT, "scripts", "pretrain_gat2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _config(tmp_path, version, extra=""):
    from fragnet_amd import train
    text = open(os.path.join(ROOT, "exps", "pt", "synth_masked", "config.yaml")).read()
    assert "model_version: gat2_masked2" in text
    text = text.replace("model_version: gat2_masked2\n", "" if version is None else f"model_version: {version}\n")
    text = text.replace("  num_layer: 4\n", "  num_layer: 1\n" + extra)
    path = tmp_path / "config.yaml"
    path.write_text(text)
    return train.load_config(str(path))


def test_driver_dispatches_on_model_version(tmp_path):
    from fragnet_amd import model as M
    drv = _driver()
    for version in ("gat2", None):
        m = drv.build_model(_config(tmp_path, version))
        assert type(m) is M.FragNetPreTrain
    m = drv.build_model(_config(tmp_path, "gat2_masked2"))
    assert type(m) is M.FragNetPreTrainMasked2 and m.mask_ratio == 0.15 and m.pretrain.dropout.p == 0.2
    text = open(os.path.join(ROOT, "exps", "pt", "synth_masked", "config.yaml")).read().replace("  mask_ratio: 0.15", "  mask_ratio: 0.25")
    p = tmp_path / "ratio.yaml"
    p.write_text(text)
    from fragnet_amd import train
    assert drv.build_model(train.load_config(str(p))).mask_ratio == 0.25
    p.write_text("\n".join(l for l in text.splitlines() if "mask_ratio" not in l) + "\n")
    assert drv.build_model(train.load_config(str(p))).mask_ratio == 0.15
    with pytest.raises(SystemExit, match="returns None"):
        drv.build_model(_config(tmp_path, "gat2_masked"))
    with pytest.raises(SystemExit, match="gat2_lite"):
        drv.build_model(_config(tmp_path, "gat2_lite"))
