"""Shared by the input-gradient tests and tests/golden/make_golden_inputgrad.py: the molecules and the model of the fixtures, the
scale-relative bound every gradient / attribution table is held to, and the entry sums of integrated gradients written out plainly
(loops, no code of fragnet_amd.gradient_attribution: the fixtures must not be made by what they check)."""
import numpy as np
import torch

CTOR = dict(n_classes=1, num_layer=2, num_heads=4, drop_ratio=0.0, h1=64, h2=128, h3=128, h4=64, act="relu", fthead="FTHead3")
FEATURES = dict(atom_features=167, frag_features=167, edge_features=17, emb_dim=128)
SEED, MOL_SEED = 2, 23
TABLE_KEYS = ("x_atoms", "node_features_bonds", "node_features_fbonds")
STEP_CHOICES = (16, 32, 64)
GAP_FRACTION = 0.02          # the recorded step count leaves |gap| <= 2 % of |pred - pred_baseline| on every molecule
RTOL_MAX = RTOL = 1e-4       # |got - ref| <= RTOL_MAX max|ref| + RTOL |ref|: the project's 1e-4, relative to the table's scale
ATOL = 1e-4                  # logits and predictions: the project's plain bound


def molecules():
    """Six synthetic molecules: one fragment only (its fragment-bond table is the single placeholder row), exactly two fragments, a
    salt with a lone counter-ion (an atom without bonds), a salt without one, two heavy atoms, and the notebook molecule."""
    from fragnet_amd import synth
    rng = np.random.default_rng(MOL_SEED)
    mols = [synth.make_molecule(rng, mu=6, p_cut=0.0)]
    while True:
        m = synth.make_molecule(rng, mu=7, p_cut=0.25)
        if int(m.n_frags) == 2:
            mols.append(m)
            break
    for want_ion in (True, False):
        while True:
            m = synth.make_molecule(rng, mu=6, p_cut=0.3, p_salt=1.0)
            deg = torch.bincount(m.edge_index[0], minlength=m.x_atoms.size(0))
            if bool((deg == 0).any()) == want_ion:
                mols.append(m)
                break
    mols.append(synth.make_molecule(rng, mu=0.1, p_cut=0.0))
    mols.append(synth.notebook_molecule())
    return mols


def build(module, ctor=None, seed=SEED):
    torch.manual_seed(seed)
    model = module.FragNetFineTune(**(ctor or CTOR))
    model.eval()
    return model


def bound(ref):
    """The per-element bound of a gradient or attribution table ``ref``."""
    ref = np.asarray(ref, dtype=np.float64)
    return RTOL_MAX * (np.abs(ref).max() if ref.size else 0.0) + RTOL * np.abs(ref)


def worst(got, ref):
    """max over the elements of |got - ref| / bound (<= 1 passes), and max |got - ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0, 0.0
    err = np.abs(got - ref)
    b = bound(ref)
    if not (b > 0).all():                # an all-zero reference: only itself passes
        return (float("inf") if err.any() else 0.0), float(err.max())
    return float((err / b).max()), float(err.max())


def assert_within(got, ref, what):
    ratio, err = worst(got, ref)
    print(f"{what}: max|diff| = {err:.3e}, max|ref| = {float(np.abs(np.asarray(ref)).max()) if np.asarray(ref).size else 0.0:.3e}, worst diff / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: outside 1e-4 max|ref| + 1e-4 |ref| by a factor {ratio:.3g} (max|diff| {err:.3e})"


def entry_sums(rows_a, rows_b, rows_f, n_atoms, n_bonds, n_fbonds):
    """Per molecule ``(atom [na], bond [nb / 2], fbond [nf // 2], other)`` from flat per-row scores: a bond / fragment connection is
    the float32 sum of its directed rows 2k and 2k + 1; ``other`` the rows of no entry (fragment-bond rows from 2 (nf // 2) on)."""
    out, a0, b0, f0 = [], 0, 0, 0
    for na, nb, nf in zip(n_atoms, n_bonds, n_fbonds):
        a = np.asarray(rows_a[a0:a0 + na], dtype=np.float32)
        b = np.asarray([np.float32(rows_b[b0 + 2 * k]) + np.float32(rows_b[b0 + 2 * k + 1]) for k in range(nb // 2)], dtype=np.float32)
        f = np.asarray([np.float32(rows_f[f0 + 2 * k]) + np.float32(rows_f[f0 + 2 * k + 1]) for k in range(nf // 2)], dtype=np.float32)
        other = np.float32(0.0)
        for r in range(2 * (nf // 2), nf):
            other += np.float32(rows_f[f0 + r])
        out.append((a, b, f, other))
        a0, b0, f0 = a0 + na, b0 + nb, f0 + nf
    return out
