"""Host-side parts of the gradient attributions (fragnet_amd/gradient_attribution.py) and self-checks of their fixtures
(tests/golden/input_grad_b6.npz, input_grad_lite_b6.npz, ig_b6.npz, written by tests/golden/make_golden_inputgrad.py from the
reference's own classes).  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import inputgrad_common as ic
from tests.conftest import GOLDEN


def _z(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ------------------------------------------------------------------------------- the alpha table and the chunking
def test_midpoint_alphas():
    from fragnet_amd import gradient_attribution as ga
    a = ga.midpoint_alphas(4)
    assert a.dtype == np.float32 and a.tolist() == [0.125, 0.375, 0.625, 0.875]
    a = ga.midpoint_alphas(32)
    np.testing.assert_array_equal(a, ((np.arange(32) + 0.5) / 32).astype(np.float32))
    assert abs(float(a.astype(np.float64).mean()) - 0.5) < 1e-12 and (np.diff(a) > 0).all()
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            ga.midpoint_alphas(bad)


def test_ig_plan_covers_every_step_once_and_respects_the_budget():
    from fragnet_amd import gradient_attribution as ga
    lens = {"atom": np.array([5, 3, 7]), "edge": np.array([8, 4, 12])}      # rows per replica: 13, 7, 19
    steps = 6
    for max_rows in (1, 20, 40, 1000):
        chunks = ga.ig_plan(lens, steps, max_rows)
        seen = {i: [] for i in range(3)}
        for chunk in chunks:
            used = sum((r1 - r0) * int(lens["atom"][i] + lens["edge"][i]) for i, r0, r1 in chunk)
            n_rep = sum(r1 - r0 for _, r0, r1 in chunk)
            assert used <= max_rows or n_rep == 1          # one replica fits into any chunk
            for i, r0, r1 in chunk:
                seen[i] += list(range(r0, r1))
        assert all(seen[i] == list(range(steps)) for i in range(3))      # every step once, ascending within a molecule
    assert len(ga.ig_plan(lens, steps, 40)) > 1 and any(len({i for i, _, _ in c}) == 1 for c in ga.ig_plan(lens, steps, 40))
    with pytest.raises(ValueError):
        ga.ig_plan(lens, steps, 0)


# ------------------------------------------------------------------------------- rows -> entries
def test_entries_line_up_with_the_replica_table():
    from fragnet_amd import attribution as attr
    from fragnet_amd import gradient_attribution as ga
    na, nb, nf = np.array([4, 1, 6, 2]), np.array([6, 0, 10, 2]), np.array([1, 1, 4, 0])
    lens = {"atom": na, "edge": nb, "fedge": nf}
    rng = np.random.default_rng(0)
    rows = [rng.standard_normal(int(c.sum())).astype(np.float32) for c in (na, nb, nf)]
    tables, other = ga.assemble(lens, rows)
    table = attr.replica_table(na, nb, nf)
    per_mol = ic.entry_sums(*rows, na, nb, nf)
    for i, t in enumerate(table):
        for kind, code, want in zip(attr.KIND_ORDER, (attr.KIND_ATOM, attr.KIND_BOND, attr.KIND_FBOND), per_mol[i][:3]):
            lo, hi = tables[kind]["offsets"][i], tables[kind]["offsets"][i + 1]
            np.testing.assert_array_equal(tables[kind]["index"][lo:hi], t[t[:, 0] == code, 1])        # the index column is replica_table's
            np.testing.assert_array_equal(tables[kind]["attr"][lo:hi], want)                          # pair sums, bit for bit
        assert other[i] == per_mol[i][3]
    # the placeholder row of a one-fragment molecule belongs to no entry: it is attr_other, nothing else is
    assert other[0] == rows[2][0] and other[1] == rows[2][1] and other[2] == 0.0 and other[3] == 0.0
    assert tables["fbond"]["offsets"].tolist() == [0, 0, 0, 2, 2]
    with pytest.raises(ValueError):
        ga.assemble(lens, [rows[0], rows[1][:-1], rows[2]])
    with pytest.raises(ValueError):
        ga.entry_rows(np.array([3]), np.array([0]))            # an odd directed-bond count
    with pytest.raises(ValueError):
        ga.entry_rows(np.array([2]), np.array([3]))            # an odd fragment-bond count that is not the placeholder


def test_completeness_gap_and_result_views():
    from fragnet_amd import gradient_attribution as ga
    na, nb, nf = np.array([2, 3]), np.array([2, 4]), np.array([1, 2])
    rows = [np.arange(5, dtype=np.float32), np.arange(6, dtype=np.float32) * 0.5, np.array([4.0, 1.0, 2.0], dtype=np.float32)]
    tables, other = ga.assemble({"atom": na, "edge": nb, "fedge": nf}, rows)
    pred, pred0 = np.array([10.0, 20.0], dtype=np.float32), np.array([1.0, 2.0], dtype=np.float32)
    gap = ga.completeness_gap(pred, pred0, tables, other)
    np.testing.assert_allclose(gap, [9.0 - (0 + 1) - 0.5 - 4.0, 18.0 - (2 + 3 + 4) - (2.5 + 4.5) - 3.0])
    res = ga.GradientAttribution("ig", pred, tables, other, pred_baseline=pred0, gap=gap, steps=8)
    assert len(res) == 2 and res[1]["bond"]["index"].tolist() == [0, 2] and res[-1]["fbond"]["attr"].tolist() == [3.0]
    arrays = res.arrays()
    assert {"pred", "pred_baseline", "gap", "attr_other", "atom_attr", "bond_index", "fbond_offsets", "steps", "method"} <= set(arrays)
    with pytest.raises(IndexError):
        res[2]


# ------------------------------------------------------------------------------- baseline validation
def test_baseline_validation():
    from fragnet_amd import gradient_attribution as ga
    widths = (167, 17, 6)
    z = ga.check_baseline(None, widths, "cpu")
    assert [tuple(t.shape) for t in z] == [(167,), (17,), (6,)] and all(float(t.abs().sum()) == 0.0 and t.dtype == torch.float32 for t in z)
    ok = ga.check_baseline((np.ones(167), torch.full((17,), 2.0, dtype=torch.float64), [0.5] * 6), widths, "cpu")
    assert all(t.dtype == torch.float32 for t in ok) and float(ok[1][3]) == 2.0 and float(ok[2][5]) == 0.5
    for bad in ((np.ones(167), np.ones(17)),                                  # two vectors
                (np.ones(166), np.ones(17), np.ones(6)),                      # wrong width
                (np.ones((1, 167)), np.ones(17), np.ones(6)),                 # not a row vector
                (np.ones(167), np.ones(17), np.array(["a"] * 6)),             # not numbers
                np.ones(167)):                                                # not a triple
        with pytest.raises((ValueError, TypeError)):
            ga.check_baseline(bad, widths, "cpu")
    with pytest.raises(ValueError, match="model is on"):                      # a tensor on another device than the model's
        ga.check_baseline((torch.ones(167, device="meta"), torch.ones(17), torch.ones(6)), widths, "cpu")


# ------------------------------------------------------------------------------- refusals
def _tiny(cls=None, **kw):
    from fragnet_amd import model as M
    return (cls or M.FragNetFineTune)(num_layer=1, h1=8, h2=8, h3=8, h4=8, **kw)


def test_cpu_model_is_refused():
    from fragnet_amd import _lib, synth
    from fragnet_amd import gradient_attribution as ga
    mols = synth.synth_molecules(2, seed=1)
    with pytest.raises(_lib.FragnetHipError):
        ga.input_gradients(_tiny(), mols)
    with pytest.raises(_lib.FragnetHipError):
        ga.integrated_gradients(_tiny(), mols, steps=2)


def test_gat2_edge_and_other_model_classes_are_refused():
    from fragnet_amd import gradient_attribution as ga
    from fragnet_amd import model as M
    from fragnet_amd import synth
    mols = synth.synth_molecules(2, seed=1)
    with pytest.raises(NotImplementedError, match="gat2_edge"):
        ga.input_gradients(_tiny(M.FragNetFineTuneEdge), mols)
    with pytest.raises(NotImplementedError, match="gat2_edge"):
        ga.integrated_gradients(_tiny(M.FragNetFineTuneEdge), mols)
    for other in (M.FragNetPreTrain(num_layer=1), torch.nn.Linear(2, 2)):
        with pytest.raises(ValueError, match="FragNetFineTune"):
            ga.input_gradients(other, mols)
        with pytest.raises(ValueError, match="FragNetFineTune"):
            ga.integrated_gradients(other, mols)


def test_engine_refuses_what_its_backward_cannot_serve():
    """The refusals happen before anything touches the GPU: encoder_forward raises on the argument combination alone."""
    from fragnet_amd import _lib, engine
    from fragnet_amd import model as M
    tables = (torch.zeros(3, 167, requires_grad=True), torch.zeros(3, 17), torch.zeros(3, 6))
    for cls, variant, p, training, word in ((M.FragNetFineTuneEdge, 2, 0.0, False, "gat2_edge"), (M.FragNetFineTune, 0, 0.1, True, "dropout")):
        layers = _tiny(cls).pretrain.layers
        with pytest.raises(NotImplementedError, match=word):
            engine.encoder_forward(layers, None, *tables, None, None, 4, p, training, None, variant=variant)
        with torch.no_grad():              # nothing to differentiate: the refusal does not apply (the call goes on to its Philox stream / the CPU-tensor check)
            with pytest.raises((AttributeError, _lib.FragnetHipError)):
                engine.encoder_forward(layers, None, *tables, None, None, 4, p, training, None, variant=variant)


def test_engine_refusal_ladder_comes_before_the_plan():
    """Every refusal of encoder_forward's argument ladder, in its order, with CPU tensors and ``plan=None``: none of them touches the
    plan, the library or the GPU."""
    from fragnet_amd import engine
    from fragnet_amd import model as M
    gat2, edge = _tiny().pretrain.layers, _tiny(M.FragNetFineTuneEdge).pretrain.layers
    lite = _tiny(M.FragNetFineTuneLite).pretrain.layers
    for layers in (gat2, edge, lite):
        for p in layers.parameters():
            p.requires_grad_(False)
    plain = (torch.zeros(3, 167), torch.zeros(3, 17), torch.zeros(3, 6))
    wants = (torch.zeros(3, 167, requires_grad=True), torch.zeros(3, 17), torch.zeros(3, 6))
    keep, mask = torch.ones(3, dtype=torch.uint8), (torch.zeros(3, dtype=torch.uint8), None, None)
    live = _tiny().pretrain.layers           # parameters that require a gradient
    rows = [
        # (layers, tables, training, drop_p, keywords, exception, a word of its message)
        (gat2, plain, False, 0.0, dict(row_masks=(None, None)), ValueError, "a triple"),
        (gat2, plain, False, 0.0, dict(keep_atoms=keep, attn_readout=True), ValueError, "does not combine with row masks or the attention read-out"),
        (gat2, plain, False, 0.0, dict(keep_atoms=keep, row_masks=mask), ValueError, "does not combine with row masks or the attention read-out"),
        (lite, plain, False, 0.0, dict(keep_atoms=keep, variant=1), ValueError, "exists for model_version gat2"),
        (gat2, plain, False, 0.0, dict(keep_atoms=keep.float()), ValueError, "contiguous uint8 CUDA tensor of 3 rows"),
        (gat2, plain, False, 0.0, dict(keep_atoms=keep), ValueError, "contiguous uint8 CUDA tensor of 3 rows"),      # a CPU tensor
        (gat2, plain, False, 0.0, dict(attn_readout=True, row_masks=mask), ValueError, "no attention read-out of a masked pass"),
        (lite, plain, False, 0.0, dict(attn_readout=True, variant=1), ValueError, "read-out exists for model_version gat2"),
        (gat2, plain, True, 0.0, dict(attn_readout=True), RuntimeError, "attn_readout: a read-out pass is an evaluation pass"),
        (gat2, wants, False, 0.0, dict(attn_readout=True), RuntimeError, "attn_readout: the read-out pass has no backward"),
        (live, plain, False, 0.0, dict(attn_readout=True), RuntimeError, "attn_readout: the read-out pass has no backward"),
        (gat2, plain, True, 0.0, dict(row_masks=mask), RuntimeError, "row_masks: a masked pass is an evaluation pass"),
        (gat2, wants, False, 0.0, dict(row_masks=mask), RuntimeError, "row_masks: the masked pass has no backward"),
        (live, plain, False, 0.0, dict(row_masks=mask), RuntimeError, "row_masks: the masked pass has no backward"),
        (edge, wants, False, 0.0, dict(variant=2), NotImplementedError, "not for gat2_edge"),
        (gat2, wants, True, 0.1, dict(), NotImplementedError, "a training pass with dropout"),
    ]
    for layers, tables, training, p, kw, exc, word in rows:
        with pytest.raises(exc, match=word):
            engine.encoder_forward(layers, None, *tables, None, None, 4, p, training, None, **kw)
    # keep_atoms with inputs that require a gradient: behind the tensor check, which wants a CUDA vector -- one that says it is
    class _OnGpu(torch.Tensor):
        is_cuda = True
    gpu_keep = keep.as_subclass(_OnGpu)
    with pytest.raises(NotImplementedError, match="no input gradients of a masked pass"):
        engine.encoder_forward(gat2, None, *wants, None, None, 4, 0.0, False, None, keep_atoms=gpu_keep)
    with torch.no_grad():                  # ... and under no_grad the same call goes on to the CPU-tensor check
        from fragnet_amd import _lib
        with pytest.raises(_lib.FragnetHipError):
            engine.encoder_forward(gat2, None, *wants, None, None, 4, 0.0, False, None, keep_atoms=gpu_keep)


# ------------------------------------------------------------------------------- the fixtures' self-checks
@pytest.mark.parametrize("name,tables", [("input_grad_b6", ic.TABLE_KEYS), ("input_grad_lite_b6", ic.TABLE_KEYS[:2])])
def test_gradient_fixture_self_checks(name, tables):
    z = _z(name)
    assert {k[len("grad/"):] for k in z.files if k.startswith("grad/")} == set(tables)
    rows = dict(zip(ic.TABLE_KEYS, (z["n_atoms"].sum(), z["n_bonds"].sum(), z["n_fbonds"].sum())))
    assert (z["n_fbonds"] == 1).any()                                    # a molecule with a single fragment: the placeholder row
    assert z["logits"].shape == (6, 1)
    for key in tables:
        g32, g64 = z[f"grad/{key}"], z[f"grad64/{key}"]
        assert g32.dtype == np.float32 and g64.dtype == np.float64 and g32.shape == g64.shape and g32.shape[0] == rows[key]
        scale = np.abs(g64).max()
        assert scale > 0
        assert np.abs(g32.astype(np.float64) - g64).max() < 2.5e-5 * scale       # the reference's own fp32 error: far inside the bound
        ratio, _ = ic.worst(g32, g64)
        assert ratio < 0.25
        assert ic.worst(np.zeros_like(g32), g32)[0] > 1.0                         # a table of zeros FAILS the bound
        with pytest.raises(AssertionError):
            ic.assert_within(np.zeros_like(g32), g32, key)


def test_gradient_fixture_batch_has_an_atom_without_bonds():
    from fragnet_amd import data
    batch = data.collate_fn(ic.molecules())
    z = _z("input_grad_b6")
    assert batch["x_atoms"].shape[0] == z["n_atoms"].sum() and batch["node_features_bonds"].shape[0] == z["n_bonds"].sum()
    deg = torch.bincount(batch["edge_index"][0], minlength=batch["x_atoms"].shape[0])
    assert bool((deg == 0).any())
    np.testing.assert_array_equal([m.node_feautures_fbondg.shape[0] for m in ic.molecules()], z["n_fbonds"])


def test_fixture_weights_are_the_seeded_model():
    import json
    from fragnet_amd import model as M
    from tests.helpers import check_params_match
    for name, cls in (("input_grad_b6", M.FragNetFineTune), ("input_grad_lite_b6", M.FragNetFineTuneLite)):
        z = _z(name)
        cfg = json.loads(str(z["cfg"]))
        assert cfg["seed"] == ic.SEED and cfg["ctor"] == dict(ic.FEATURES, **ic.CTOR)
        torch.manual_seed(cfg["seed"])
        check_params_match(cls(**ic.CTOR), json.loads(str(z["pkeys"])), z["psums"])


def test_ig_fixture_self_checks():
    z = _z("ig_b6")
    steps = int(z["steps"])
    assert steps in ic.STEP_CHOICES
    pred, pred0, gap, other = z["pred"], z["pred_baseline"], z["gap"], z["attr_other"]
    diff = np.abs(pred.astype(np.float64) - pred0)
    assert (np.abs(gap) <= ic.GAP_FRACTION * diff).all()                          # the recorded gap condition, on every molecule
    import json
    by_steps = {int(k): v for k, v in json.loads(str(z["gap_by_steps"])).items()}
    assert all(by_steps[s] > ic.GAP_FRACTION for s in ic.STEP_CHOICES if s < steps)  # ... and no smaller count met it
    for i in range(6):
        a, b, f = z[f"m{i}/atom"], z[f"m{i}/bond"], z[f"m{i}/fbond"]
        assert a.shape == (z["n_atoms"][i],) and b.shape == (z["n_bonds"][i] // 2,) and f.shape == (z["n_fbonds"][i] // 2,)
        total = a.astype(np.float64).sum() + b.astype(np.float64).sum() + f.astype(np.float64).sum() + other[i]
        assert abs(pred[i] - pred0[i] - total - gap[i]) < 1e-6 * max(1.0, diff[i])  # gap is the identity's remainder
        assert (other[i] != 0) == (z["n_fbonds"][i] % 2 == 1) or other[i] == 0
    flat = np.concatenate([z[f"m{i}/atom"] for i in range(6)])
    assert ic.worst(np.zeros_like(flat), flat)[0] > 1.0                           # zeros fail the bound here too
