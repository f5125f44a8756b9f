"""Host side of the nearest-neighbour search (fragnet_amd/neighbours.py, ops.TopK, scripts/neighbours_gat2.py, csrc/topk.hip's argument
checks) and the rules of its float64 reference tests/topk_ref.py.  Nothing here needs a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------- the reference's own rules
def test_reference_ties_go_to_the_smaller_index():
    q = np.array([[1.0, 0.0]])
    lib = np.array([[0.5, 9.0], [1.0, 0.0], [0.5, -3.0], [1.0, 7.0], [2.0, 0.0]])
    s, i = R.topk(q, lib, 4, 0)
    assert i.tolist() == [[4, 1, 3, 0]] and s.tolist() == [[2.0, 1.0, 1.0, 0.5]]
    s, i = R.topk(q, lib, 3, 2)                     # squared L2: smaller is better; rows 1 (0) then 4 (1) then 2 (9.25)
    assert i.tolist() == [[1, 4, 2]] and s.tolist() == [[0.0, 1.0, 9.25]]
    s, i = R.topk(q, lib, 2, 0, index_base=2 ** 33)
    assert i.tolist() == [[2 ** 33 + 4, 2 ** 33 + 1]]


def test_reference_padding_and_exclusion():
    q = np.array([[1.0, 0.0], [0.0, 1.0]])
    lib = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    for metric, empty in ((0, -np.inf), (1, -np.inf), (2, np.inf)):
        s, i = R.topk(q, lib, 5, metric)
        assert (i[:, 3:] == -1).all() and (s[:, 3:] == empty).all() and (i[:, :3] >= 0).all()
        s, i = R.topk(q, lib[:0], 2, metric)
        assert (i == -1).all() and (s == empty).all()
    s, i = R.topk(q, lib, 2, 2, exclude=np.array([0, -1]))
    assert i.tolist() == [[2, 1], [1, 2]]           # query 0 skips its own row 0; query 1 (-1: none) keeps row 1
    s, i = R.topk(q, lib, 2, 2, index_base=10, exclude=np.array([10, 11]))
    assert i.tolist() == [[12, 11], [12, 10]]       # exclusion compares global ids
    s, i = R.topk(np.array([[1.0, 0.0]]), np.array([[0.0, 0.0], [2.0, 0.0]]), 2, 1)
    assert i.tolist() == [[1, 0]] and s.tolist() == [[1.0, 0.0]]        # an all-zero row under cosine scores 0


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_reference_chunked_equals_unchunked(metric):
    rng = np.random.default_rng(3)
    q, lib = rng.integers(-2, 3, size=(7, 6)).astype(float), rng.integers(-2, 3, size=(41, 6)).astype(float)
    lib[5] = lib[30]
    want = R.topk(q, lib, 9, metric)
    for chunk in (1, 7, 40):
        got = R.topk(q, lib, 9, metric, chunk=chunk)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (np.diff(want[0], axis=1) == 0).any()      # small integers: ties among the best are there
    R.check_lists(want[0], want[1], R.scores(q, lib, metric), metric)


def test_reference_check_refuses_wrong_lists():
    rng = np.random.default_rng(4)
    q, lib = rng.standard_normal((3, 8)), rng.standard_normal((30, 8))
    sc = R.scores(q, lib, 1)
    s, i = R.topk(q, lib, 4, 1)
    R.check_lists(s, i, sc, 1)
    worst = np.argmin(sc[1])
    bad_i, bad_s = i.copy(), s.copy()
    bad_i[1, 3], bad_s[1, 3] = worst, sc[1, worst]                        # right score of a wrong row: a better row is left outside
    with pytest.raises(AssertionError, match="outside"):
        R.check_lists(bad_s, bad_i, sc, 1)
    bad_i = i.copy()
    bad_i[0, 1] = bad_i[0, 0]
    with pytest.raises(AssertionError):
        R.check_lists(s, bad_i, sc, 1)
    with pytest.raises(AssertionError, match="sorted"):
        R.check_lists(s[:, ::-1], i[:, ::-1], sc, 1)
    off = s.copy()
    off[2, 0] += 1e-3
    with pytest.raises(AssertionError):
        R.check_lists(off, i, sc, 1)


# ---------------------------------------------------------------------------------------- rows -> (molecule, fragment), the result class
def test_rows_map_to_molecule_and_fragment():
    from fragnet_amd.neighbours import rows_to_mol_frag
    offsets = np.array([0, 3, 4, 4, 9])               # 3 fragments, ONE fragment, none, 5
    mol, frag = rows_to_mol_frag(np.array([[0, 2, 3], [4, 8, -1]]), offsets)
    assert mol.tolist() == [[0, 0, 1], [3, 3, -1]] and frag.tolist() == [[0, 2, 0], [0, 4, -1]]
    mol, frag = rows_to_mol_frag(np.arange(5), np.arange(6))            # the "mol" level: a row is its molecule
    assert mol.tolist() == [0, 1, 2, 3, 4] and frag.tolist() == [0] * 5
    with pytest.raises(ValueError):
        rows_to_mol_frag(np.array([9]), offsets)
    with pytest.raises(ValueError):
        rows_to_mol_frag(np.array([0]), np.array([1, 2]))


def test_neighbours_indexing_and_arrays():
    from fragnet_amd.neighbours import Neighbours
    q_off, lib_off = np.array([0, 2, 3, 3]), np.array([0, 3, 4, 4, 9])
    score = np.array([[0.9, 0.5], [0.8, 0.1], [0.7, -np.inf]], dtype=np.float32)
    index = np.array([[3, 0], [8, 2], [4, -1]])
    res = Neighbours("frag", "cosine", score, index, q_off, lib_off)
    assert len(res) == 3
    assert res.query_mol.tolist() == [0, 0, 1] and res.query_frag.tolist() == [0, 1, 0]
    assert res.mol.tolist() == [[1, 0], [3, 0], [3, -1]] and res.frag.tolist() == [[0, 0], [4, 2], [0, -1]]
    first = res[0]
    assert first["score"].shape == (2, 2) and first["mol"].tolist() == [[1, 0], [3, 0]] and first["frag"].tolist() == [[0, 0], [4, 2]]
    assert res[-1]["score"].shape == (0, 2) and res[1]["index"].tolist() == [[4, -1]]
    with pytest.raises(IndexError):
        res[3]
    assert res.domain_distance().tolist() == [np.float32(0.9), np.float32(0.7), -np.inf]
    arrays = res.arrays()
    assert set(arrays) == {"score", "index", "mol", "frag", "domain_distance", "level", "metric", "query_mol", "query_frag",
                           "query_offsets", "library_offsets"}
    assert str(arrays["level"]) == "frag" and str(arrays["metric"]) == "cosine"

    mol = Neighbours("mol", "l2", np.array([[0.0, 2.0], [1.0, 3.0]]), np.array([[0, 1], [1, 0]]), np.arange(3), np.arange(3))
    assert len(mol) == 2 and set(mol[1]) == {"score", "index", "mol"} and mol[1]["index"].tolist() == [1, 0] and mol[1]["score"].shape == (2,)
    assert np.array_equal(mol.mol, mol.index) and mol.domain_distance().tolist() == [0.0, 1.0]
    assert set(mol.arrays()) == {"score", "index", "mol", "domain_distance", "level", "metric"}
    with pytest.raises(ValueError):
        Neighbours("mol", "l2", np.zeros((3, 2)), np.zeros((3, 2), dtype=np.int64), np.arange(3), np.arange(3))
    with pytest.raises(ValueError, match="level"):
        Neighbours("atom", "l2", np.zeros((2, 2)), np.zeros((2, 2), dtype=np.int64), np.arange(3), np.arange(3))


# ---------------------------------------------------------------------------------------- refusals
def _small_model():
    from fragnet_amd.model import FragNetFineTune
    return FragNetFineTune(num_layer=2, h1=8, h2=8, h3=8, h4=8, edge_features=17)


def test_argument_refusals():
    from fragnet_amd import _lib, cdrp, dta, neighbours as nb, ops, synth
    mols, other = synth.synth_molecules(3, seed=1, profile="esol"), synth.synth_molecules(3, seed=2, profile="esol")
    model = _small_model()
    for k in (0, 33, -1, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            nb.nearest(model, mols, mols, k=k)
        with pytest.raises(ValueError, match="k must be"):
            ops.TopK(4, k, "dot", "cuda:0")
    with pytest.raises(ValueError, match="metric"):
        nb.nearest(model, mols, mols, metric="manhattan")
    with pytest.raises(ValueError, match="metric"):
        ops.TopK(4, 3, 3, "cuda:0")
    with pytest.raises(ValueError, match="level"):
        nb.nearest(model, mols, mols, level="atom")
    with pytest.raises(ValueError, match="level"):
        nb.embed(model, mols, "bond")
    with pytest.raises(ValueError, match="batch_size"):
        nb.nearest(model, mols, mols, batch_size=0)
    with pytest.raises(ValueError, match="exclude_self"):
        nb.nearest(model, mols, other, exclude_self=True)
    with pytest.raises(ValueError, match="exclude_self"):
        nb.nearest(model, mols, list(mols), exclude_self=True)           # an equal copy is not the same source
    drug = cdrp.FragNetFineTuneBase(num_layer=2, h1=8, h2=8, h3=8, h4=8)
    for pair in (cdrp.CDRPModel(drug, 16, "cpu"), dta.DTAModel2(drug)):
        with pytest.raises(ValueError, match="pair model"):
            nb.nearest(pair, mols, mols)
        with pytest.raises(ValueError, match=type(pair).__name__):
            nb.embed(pair, mols, "mol")
    with pytest.raises(ValueError, match="Linear"):
        nb.embed(torch.nn.Linear(2, 2), mols, "mol")
    # CPU models and CPU tensors: no fallback
    with pytest.raises(_lib.FragnetHipError):
        nb.nearest(model, mols, mols)
    with pytest.raises(_lib.FragnetHipError):
        nb.embed(model, mols, "frag")
    with pytest.raises(_lib.FragnetHipError):
        ops.TopK(4, 3, "dot", "cpu")
    with pytest.raises(_lib.FragnetHipError):
        ops.rows_rnorm(torch.zeros(3, 128))
    assert [ops.topk_metric(m) for m in ("dot", "cosine", "l2", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]


def _descriptor(_lib, **kw):
    fields = dict(q=None, lib=None, q_aux=None, lib_aux=None, exclude=None, best_score=None, best_index=None, scratch=None,
                  scratch_bytes=0, n_q=4, n_lib=100, index_base=0, d=128, k=8, metric=0, splits=0)
    fields.update(kw)
    t = _lib.Topk()
    for name, v in fields.items():
        setattr(t, name, v)
    return t


def test_library_refuses_bad_descriptors_before_any_launch():
    """Argument errors return before anything is launched, so they can be checked without a GPU (as tests/test_abi.py does)."""
    from fragnet_amd import _lib
    lib = _lib.load()
    assert [name for name, _ in _lib.Topk._fields_] == ["q", "lib", "q_aux", "lib_aux", "exclude", "best_score", "best_index", "scratch",
                                                        "scratch_bytes", "n_q", "n_lib", "index_base", "d", "k", "metric", "splits"]
    ok = _descriptor(_lib)
    need = lib.fn_topk_scratch_bytes(C.byref(ok))
    assert need > 0 and need % (4 * 8 * 12) == 0              # per query: slices x 4 waves x k entries of 4 + 8 bytes
    assert lib.fn_topk_scratch_bytes(C.byref(_descriptor(_lib, splits=2))) == 4 * 2 * 4 * 8 * 12
    assert lib.fn_topk_scratch_bytes(C.byref(_descriptor(_lib, splits=63, n_lib=17))) == 4 * 2 * 4 * 8 * 12     # 17 rows: two tiles
    for bad in (dict(k=0), dict(k=33), dict(n_q=-1), dict(n_lib=-1), dict(splits=-1)):
        assert lib.fn_topk_scratch_bytes(C.byref(_descriptor(_lib, **bad))) == _lib.FN_EINVAL, bad
        assert lib.fn_topk_update_f32(C.byref(_descriptor(_lib, **bad)), None) == _lib.FN_EINVAL, bad
        assert b"fn_topk" in lib.fn_last_error()
    assert lib.fn_topk_update_f32(None, None) == _lib.FN_EINVAL
    assert lib.fn_topk_update_f32(C.byref(_descriptor(_lib, metric=3)), None) == _lib.FN_EINVAL and b"metric" in lib.fn_last_error()
    for d in (0, 64, 192, 512):
        assert lib.fn_topk_update_f32(C.byref(_descriptor(_lib, d=d)), None) == _lib.FN_EUNSUPPORTED, d
    assert lib.fn_topk_update_f32(C.byref(ok), None) == _lib.FN_EINVAL and b"null" in lib.fn_last_error()
    fake = dict(q=1 << 20, lib=1 << 21, best_score=1 << 22, best_index=1 << 23, scratch=1 << 24)       # never dereferenced on the host
    assert lib.fn_topk_update_f32(C.byref(_descriptor(_lib, **fake, scratch_bytes=need - 1)), None) == _lib.FN_EINVAL
    assert b"scratch" in lib.fn_last_error()
    assert lib.fn_topk_update_f32(C.byref(_descriptor(_lib, **fake, scratch_bytes=need, metric=1)), None) == _lib.FN_EINVAL   # no norms
    assert lib.fn_topk_update_f32(C.byref(_descriptor(_lib, **dict(fake, q=(1 << 20) + 4), scratch_bytes=need)), None) == _lib.FN_EINVAL
    assert b"misaligned" in lib.fn_last_error()
    # empty calls launch nothing and succeed, whatever the pointers
    assert lib.fn_topk_update_f32(C.byref(_descriptor(_lib, n_lib=0)), None) == 0
    assert lib.fn_topk_update_f32(C.byref(_descriptor(_lib, n_q=0)), None) == 0
    assert lib.fn_rows_rnorm_f32(None, 0, 128, None, None) == 0
    assert lib.fn_rows_rnorm_f32(None, 3, 128, None, None) == _lib.FN_EINVAL
    assert lib.fn_rows_rnorm_f32(None, -1, 128, None, None) == _lib.FN_EINVAL


# ---------------------------------------------------------------------------------------- the script
SCRIPT = os.path.join(ROOT, "scripts", "neighbours_gat2.py")


def test_script_argument_handling():
    run = lambda *argv: subprocess.run([sys.executable, SCRIPT, *argv], capture_output=True, text=True, cwd=ROOT)
    r = run("--help")
    assert r.returncode == 0 and all(w in r.stdout for w in ("--queries", "--library", "--level", "--metric", "--exclude-self"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import neighbours_gat2
    finally:
        sys.path.pop(0)
    base = ["--config", "c.yaml", "--checkpoint", "m.pt", "--queries", "q.pt", "--library", "l.pt"]
    a = neighbours_gat2.parse_args([*base, "--out", "o/n.npz"])
    assert (a.level, a.k, a.metric, a.batch_size, a.exclude_self, a.device) == ("mol", 8, "cosine", 512, False, "cuda:0")
    a = neighbours_gat2.parse_args(["--config", "c.yaml", "--checkpoint", "m.pt", "--queries", "q.pt", "--library", "./q.pt", "--out", "n.npz",
                                    "--level", "frag", "--k", "32", "--metric", "l2", "--batch-size", "64", "--exclude-self"])
    assert (a.level, a.k, a.metric, a.batch_size, a.exclude_self) == ("frag", 32, "l2", 64, True)
    for bad in (["--out", "n.txt"], ["--out", "n.npz", "--k", "0"], ["--out", "n.npz", "--k", "33"], ["--out", "n.npz", "--batch-size", "0"],
                ["--out", "n.npz", "--metric", "manhattan"], ["--out", "n.npz", "--level", "atom"], ["--out", "n.npz", "--exclude-self"], []):
        with pytest.raises(SystemExit) as e:
            neighbours_gat2.parse_args([*base, *bad])
        assert e.value.code == 2, bad
