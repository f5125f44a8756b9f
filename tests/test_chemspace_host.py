"""Host side of the chemical-space map (fragnet_amd/chemspace.py, ops.Moments, ops.rows_project, scripts/embedding_map_gat2.py,
csrc/moments.hip's argument checks): the binding, every refusal before any device call, and the float64 host solver against
tests/moments_ref.py.  Nothing here needs a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from fragnet_amd import chemspace as cs
from tests import moments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------- the binding and the library's refusals
def test_header_binding():
    from fragnet_amd import _lib, ops
    assert _lib.ABI_VERSION == 12 and _lib.load().fn_abi_version() == 12
    for name in ("fn_moments_scratch_bytes", "fn_rows_moments_f32", "fn_rows_project_f32"):
        assert name in _lib.SIGNATURES and name in _lib.HEADER.functions
    assert [n for n, _ in _lib.Moments._fields_] == ["x", "shift", "sum", "gram", "scratch", "scratch_bytes", "n", "d", "accumulate", "splits"]
    assert [n for n, _ in _lib.Project._fields_] == ["x", "shift", "W", "out", "sq", "n", "d", "k"]
    assert _lib.HEADER.functions["fn_moments_scratch_bytes"][0] is C.c_int64
    assert _lib.MOMENTS_CHUNK % 64 == 0 and _lib.MOMENTS_CHUNK <= 1024 and _lib.MOMENTS_GROUP >= 1
    assert (ops.MOMENTS_CHUNK, ops.MOMENTS_GROUP) == (_lib.MOMENTS_CHUNK, _lib.MOMENTS_GROUP)


def _moments(_lib, **kw):
    fields = dict(x=1 << 20, shift=1 << 21, sum=1 << 22, gram=1 << 23, scratch=1 << 24, scratch_bytes=1 << 40, n=1000, d=256, accumulate=0, splits=0)
    fields.update(kw)
    m = _lib.Moments()
    for name, v in fields.items():
        setattr(m, name, v)
    return m


def _project(_lib, **kw):
    fields = dict(x=1 << 20, shift=1 << 21, W=1 << 22, out=1 << 23, sq=1 << 24, n=1000, d=256, k=2)
    fields.update(kw)
    p = _lib.Project()
    for name, v in fields.items():
        setattr(p, name, v)
    return p


def test_library_refuses_bad_descriptors_before_any_launch():
    from fragnet_amd import _lib
    lib = _lib.load()
    rows_per_slot = _lib.MOMENTS_CHUNK * _lib.MOMENTS_GROUP
    need = lambda **kw: lib.fn_moments_scratch_bytes(C.byref(_moments(_lib, **kw)))                      # noqa: E731
    assert need(n=0) == 0 and need(n=1) == (256 * 256 + 256) * 8 == need(n=rows_per_slot) and need(n=rows_per_slot + 1, d=128) == 2 * (128 * 128 + 128) * 8
    assert need(n=1 << 20) <= 20 << 20                       # 1 M rows of 256: on the order of 10 MB, not a Gram per chunk
    assert need(n=1000, splits=63) == need(n=1000)
    mom = lambda **kw: lib.fn_rows_moments_f32(C.byref(_moments(_lib, **kw)), None)                      # noqa: E731
    assert lib.fn_rows_moments_f32(None, None) == _lib.FN_EINVAL and lib.fn_moments_scratch_bytes(None) == _lib.FN_EINVAL
    for bad in (dict(n=-1), dict(splits=-1), dict(n=1 << 40)):
        assert mom(**bad) == _lib.FN_EINVAL and need(**bad) == _lib.FN_EINVAL, bad
    for d in (0, 64, 127, 192, 512):
        assert mom(d=d) == _lib.FN_EUNSUPPORTED and need(d=d) == _lib.FN_EUNSUPPORTED and b"128 or 256" in lib.fn_last_error()
    for name in ("x", "sum", "gram", "scratch"):
        assert mom(**{name: None}) == _lib.FN_EINVAL and b"null" in lib.fn_last_error(), name
    for name, off in (("x", 8), ("shift", 4), ("scratch", 8), ("sum", 4), ("gram", 4)):
        assert mom(**{name: (1 << 25) + off}) == _lib.FN_EINVAL and b"misaligned" in lib.fn_last_error(), name
    assert mom(scratch_bytes=need() - 1) == _lib.FN_EINVAL and b"scratch" in lib.fn_last_error()
    assert mom(n=0, accumulate=1, x=None, scratch=None, scratch_bytes=0) == 0          # nothing to add: nothing is launched or looked at

    proj = lambda **kw: lib.fn_rows_project_f32(C.byref(_project(_lib, **kw)), None)                     # noqa: E731
    assert lib.fn_rows_project_f32(None, None) == _lib.FN_EINVAL
    for bad in (dict(n=-1), dict(k=0), dict(k=257), dict(k=129, d=128), dict(k=-3), dict(out=None, sq=None), dict(x=None), dict(W=None)):
        assert proj(**bad) == _lib.FN_EINVAL, bad
    assert proj(out=None, sq=None) == _lib.FN_EINVAL and b"neither" in lib.fn_last_error()
    for d in (0, 64, 192, 512):
        assert proj(d=d, k=1) == _lib.FN_EUNSUPPORTED
    for name, off in (("x", 8), ("shift", 8), ("W", 2), ("out", 2), ("sq", 2)):
        assert proj(**{name: (1 << 25) + off}) == _lib.FN_EINVAL and b"misaligned" in lib.fn_last_error(), name
    assert proj(n=0, x=None, W=None) == 0


class _Fake:
    """Stands in for a GPU tensor as far as the Python-side checks look: shape, dtype, device, contiguity.  Its data_ptr is never asked for."""

    def __init__(self, shape, dtype=torch.float32, device="cuda:0"):
        self.shape, self.dtype, self.device, self.is_cuda = torch.Size(shape), dtype, torch.device(device), True

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True

    def data_ptr(self):
        raise AssertionError("a refusal came too late: the device pointer was asked for")


def test_python_side_refusals():
    from fragnet_amd import _lib, ops
    for d in (64, 255, 512, "256"):
        with pytest.raises(_lib.FragnetHipError, match="built for"):
            ops.Moments(d, "cuda:0")
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        ops.Moments(256, "cpu")
    for splits in (-1, 64, 1.5, True):
        with pytest.raises(ValueError, match="splits"):
            ops.Moments(256, "cuda:0", splits=splits)
    # the updates: the checks need no device, so a stand-in for the state is enough
    mom = ops.Moments.__new__(ops.Moments)
    mom.d, mom.device, mom.splits, mom.n, mom.shift, mom._given, mom._updates, mom._scratch = 256, torch.device("cuda:0"), 0, 0, None, None, 0, None
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        mom.update(torch.zeros(4, 256))
    with pytest.raises(TypeError, match="float32"):
        mom.update(_Fake((4, 256), torch.float64))
    with pytest.raises(TypeError, match="float32"):
        mom.update(_Fake((4, 256), torch.float16))
    for shape in ((4, 128), (256,), (2, 2, 256)):
        with pytest.raises(ValueError, match=r"\[n, 256\]"):
            mom.update(_Fake(shape))
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        mom.update(_Fake((4, 256)), torch.zeros(256))
    with pytest.raises(TypeError, match="float32"):
        mom.update(_Fake((4, 256)), _Fake((256,), torch.float64))
    for shape in ((128,), (1, 256), (257,)):
        with pytest.raises(ValueError, match=r"shift must be \[256\]"):
            mom.update(_Fake((4, 256)), _Fake(shape))
    with pytest.raises(ValueError, match="on cuda:0"):
        mom.update(_Fake((4, 256)), _Fake((256,), device="cuda:1"))
    assert mom.n == 0 and mom._updates == 0

    x = _Fake((10, 256))
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        ops.rows_project(torch.zeros(10, 256), _Fake((256, 2)))
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        ops.rows_project(x, torch.zeros(256, 2))
    with pytest.raises(TypeError, match="float32"):
        ops.rows_project(_Fake((10, 256), torch.bfloat16), _Fake((256, 2)))
    with pytest.raises(TypeError, match="float32"):
        ops.rows_project(x, _Fake((256, 2), torch.float64))
    for width in (64, 192, 512):
        with pytest.raises(_lib.FragnetHipError, match="built for"):
            ops.rows_project(_Fake((10, width)), _Fake((width, 2)))
    for shape in ((128, 2), (256,), (2, 256), (256, 2, 1)):
        with pytest.raises(ValueError, match=r"W must be \[256, k\]"):
            ops.rows_project(x, _Fake(shape))
    for k in (0, 257):
        with pytest.raises(ValueError, match=r"k must be in \[1, 256\]"):
            ops.rows_project(x, _Fake((256, k)))
    with pytest.raises(ValueError, match=r"k must be in \[1, 128\]"):
        ops.rows_project(_Fake((10, 128)), _Fake((128, 129)))
    with pytest.raises(ValueError, match=r"shift must be \[256\]"):
        ops.rows_project(x, _Fake((256, 2)), _Fake((128,)))
    with pytest.raises(ValueError, match="nothing is wanted"):
        ops.rows_project(x, _Fake((256, 2)), want_rows=False, want_sq=False)


def test_driver_refusals():
    from fragnet_amd import _lib, synth
    from fragnet_amd.dataset import FlatMolStore
    from fragnet_amd.model import FragNetFineTune
    torch.manual_seed(0)
    model = FragNetFineTune(num_layer=2, h1=8, h2=8, h3=8, h4=8, edge_features=17)
    mols = synth.synth_molecules(6, seed=2, profile="esol")
    store = FlatMolStore.from_records(mols)
    with pytest.raises(ValueError, match="unknown level"):
        cs.fit(model, store, level="atom")
    with pytest.raises(ValueError, match="batch_size"):
        cs.fit(model, store, batch_size=0)
    with pytest.raises(ValueError, match="no source"):
        cs.fit(model)
    with pytest.raises(ValueError, match="comes alone"):
        cs.fit(torch.zeros(4, 256), store)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        cs.fit(torch.zeros(4, 256))
    with pytest.raises(ValueError, match="quantile"):
        cs.map(model, store, quantile=1.5)
    with pytest.raises(ValueError, match="positive integer"):
        cs.map(model, store, k=0)

    class Pair(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.drug_model = model

    for call in (lambda: cs.fit(Pair(), store), lambda: cs.map(Pair(), store)):
        with pytest.raises(ValueError, match="pair model"):
            call()
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):           # everything above was refused before the device was asked for
        cs.fit(model, store)
    with pytest.raises(_lib.FragnetHipError, match="no CPU fallback"):
        cs.map(model, store)


# ---------------------------------------------------------------------------------------- the host solver
def _space(rows, shift=None, level=None):
    """The solver fed with float64 moments of ``rows - shift``."""
    rows = np.asarray(rows, dtype=np.float64)
    shift = np.zeros(rows.shape[1]) if shift is None else np.asarray(shift, dtype=np.float64)
    z = rows - shift
    return cs.solve(rows.shape[0], shift, z.sum(0), z.T @ z, level)


@pytest.mark.parametrize("n,d", [(2000, 128), (3000, 256)])
def test_solver_matches_the_svd_of_the_centred_rows(n, d):
    rng = np.random.default_rng(n)
    rows = rng.standard_normal((n, d)) * np.linspace(3.0, 0.5, d) + rng.standard_normal(d) * 5
    sp = _space(rows, shift=rows[:64].mean(0))
    mean, eig, v = R.pca(rows)
    assert (sp.n, sp.width, sp.level) == (n, d, "mol" if d == 256 else "frag")
    assert np.allclose(sp.mean, mean, rtol=0, atol=1e-12 * np.abs(mean).max())
    assert np.allclose(sp.eigenvalues, eig, rtol=1e-8, atol=0) and (np.diff(sp.eigenvalues) <= 0).all()
    assert sp.rank == d
    lead = 8                                                           # well-separated leading directions: equal to the SVD's, sign included
    assert np.abs(sp.components[:, :lead] - v[:, :lead]).max() < 1e-8
    assert np.allclose(sp.components.T @ sp.components, np.eye(d), atol=1e-12)
    assert np.isclose(sp.explained_variance_ratio.sum(), 1.0) and np.allclose(sp.explained_variance_ratio, eig / eig.sum(), atol=1e-12)
    gamma = cs.chain_gamma(cs._moments_chunk())
    assert np.isclose(sp.floor, gamma * (eig.sum() + mean @ mean - 2 * mean @ sp.shift + sp.shift @ sp.shift), rtol=1e-9)
    # the shift changes nothing but rounding
    sp0 = _space(rows)
    assert np.allclose(sp0.eigenvalues, sp.eigenvalues, rtol=1e-8, atol=0) and np.allclose(sp0.mean, sp.mean, atol=1e-12)


def test_sign_rule():
    v = np.array([[0.1, -0.5, 0.7], [-0.9, 0.5, -0.7], [0.3, 0.2, 0.1]])
    s = cs.sign_components(v)
    assert np.array_equal(s[:, 0], -v[:, 0])                           # largest magnitude -0.9: flipped
    assert np.array_equal(s[:, 1], -v[:, 1])                           # |-0.5| == |0.5|: the lowest index (-0.5) decides
    assert np.array_equal(s[:, 2], v[:, 2])                            # 0.7 before -0.7: stays
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((50, 128))
    sp = _space(rows)
    top = np.abs(sp.components).argmax(0)
    assert (sp.components[top, np.arange(128)] > 0).all()
    mirrored = _space(2 * rows.mean(0) - rows)                         # the rows reflected through their mean: the same covariance, the same signs
    assert np.abs(mirrored.components[:, :5] - sp.components[:, :5]).max() < 1e-9


def test_rank_deficient_table_and_refusals():
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((5, 128))
    sp = _space(rows, shift=rows.mean(0))
    assert 1 <= sp.rank <= 4 and sp.rank == 4
    assert (sp.eigenvalues[4:] <= sp.floor).all() and sp.floor > 0
    with pytest.raises(ValueError, match="exceeds the rank 4"):
        sp.directions(5)
    assert sp.directions(4).shape == (128, 4) and sp.whitening().shape == (128, 4)
    with pytest.raises(ValueError, match="positive integer"):
        sp.directions(0)
    same = np.ones((6, 128))
    with pytest.raises(ValueError, match="rank 0"):
        _space(same).whitening()
    with pytest.raises(ValueError, match="at least 2 rows"):
        _space(rows[:1])
    bad = rows.copy()
    bad[2, 7] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        _space(bad)
    with pytest.raises(ValueError, match="belong to no level"):
        _space(rng.standard_normal((9, 64)))
    with pytest.raises(ValueError, match="needs shift and sum"):
        cs.solve(9, np.zeros(128), np.zeros(128), np.zeros((128, 128)), level="mol")


@pytest.mark.parametrize("n,d", [(5, 128), (90, 128), (700, 256)])
def test_mean_mahalanobis_of_the_fitted_rows_is_the_rank(n, d):
    rng = np.random.default_rng(n + d)
    rows = rng.standard_normal((n, d)) * np.linspace(2.0, 1.0, d) + 3.0
    sp = _space(rows, shift=rows.mean(0))
    assert sp.rank == min(n - 1, d)
    d2 = R.mahalanobis(rows, sp.mean, sp.eigenvalues, sp.components, sp.rank)
    assert np.isclose(d2.mean(), sp.rank, rtol=1e-9)                   # tr(L_r^-1 V_r^T C V_r) = r
    w = sp.whitening()
    assert np.allclose((((rows - sp.mean) @ w) ** 2).sum(1), d2, rtol=1e-9)
    var = (((rows - sp.mean) @ sp.directions(min(3, sp.rank))) ** 2).mean(0)
    assert np.allclose(var, sp.eigenvalues[:var.shape[0]], rtol=1e-9)


def test_map_result_and_arrays_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((7, 128))
    sp = _space(rows)
    offsets, q_offsets = np.array([0, 2, 2, 7]), np.array([0, 1, 3])
    coords, d2 = rng.standard_normal((7, 2)).astype(np.float32), np.arange(7, dtype=np.float32)
    res = cs.ChemMap(sp, 0.5, coords, d2, offsets, rng.standard_normal((3, 2)), [1.0, 3.0, 3.5], q_offsets)
    assert len(res) == 7 and res.k == 2 and res.level == "frag" and res.domain_cutoff == 3.0
    assert res.inside.tolist() == [True, True, False]
    assert res.mol.tolist() == [0, 0, 2, 2, 2, 2, 2] and res.frag.tolist() == [0, 1, 0, 1, 2, 3, 4]
    assert res.query_mol.tolist() == [0, 1, 1] and res.query_frag.tolist() == [0, 0, 1]
    item = res[-1]
    assert (item["mol"], item["frag"], item["d2"]) == (2, 4, 6.0) and np.array_equal(item["coords"], coords[6])
    with pytest.raises(IndexError):
        res[7]
    arrays = res.arrays()
    path = tmp_path / "map.npz"
    np.savez(path, **arrays)
    back = np.load(path)
    assert set(back.files) == set(arrays) >= {"coords", "d2", "query_coords", "query_d2", "inside", "domain_cutoff", "eigenvalues", "components",
                                              "mean", "rank", "floor", "explained_variance_ratio", "n", "level", "quantile"}
    for name, v in arrays.items():
        assert np.array_equal(back[name], v), name
    assert str(back["level"]) == "frag" and int(back["rank"]) == sp.rank and back["coords"].dtype == np.float32
    none = cs.ChemMap(sp, 0.95, coords, d2, offsets)                   # no queries: empty fields, still every field
    assert none.query_coords.shape == (0, 2) and none.inside.shape == (0,) and set(none.arrays()) == set(arrays)
    with pytest.raises(ValueError, match="quantile"):
        cs.ChemMap(sp, 1.5, coords, d2, offsets)
    with pytest.raises(ValueError, match="do not match"):
        cs.ChemMap(sp, 0.5, coords, d2[:6], offsets)
    with pytest.raises(ValueError, match="query rows"):
        cs.ChemMap(sp, 0.5, coords, d2, offsets, np.zeros((3, 2)), np.zeros(2), q_offsets)


# ---------------------------------------------------------------------------------------- the script
def test_script_argument_handling():
    import subprocess
    script = os.path.join(ROOT, "scripts", "embedding_map_gat2.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("--config", "--checkpoint", "--library", "--queries", "--level", "--k", "--quantile", "--out"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import embedding_map_gat2
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--checkpoint", "m.pt", "--library", "l.pt"]
    a = embedding_map_gat2.parse_args([*base, "--out", "o/m.npz"])
    assert (a.level, a.k, a.quantile, a.batch_size, a.queries, a.device) == ("mol", 2, 0.95, 512, None, "cuda:0")
    a = embedding_map_gat2.parse_args([*base, "--queries", "q.pt", "--out", "m.npz", "--level", "frag", "--k", "128", "--quantile", "0.9", "--batch-size", "64"])
    assert (a.level, a.k, a.quantile, a.batch_size, a.queries) == ("frag", 128, 0.9, 64, "q.pt")
    for bad in (["--out", "m.txt"], ["--out", "m.npz", "--k", "0"], ["--out", "m.npz", "--k", "257"], ["--out", "m.npz", "--level", "frag", "--k", "129"],
                ["--out", "m.npz", "--quantile", "1.2"], ["--out", "m.npz", "--batch-size", "0"], ["--out", "m.npz", "--level", "atom"], []):
        with pytest.raises(SystemExit) as e:
            embedding_map_gat2.parse_args([*base, *bad])
        assert e.value.code == 2, bad
