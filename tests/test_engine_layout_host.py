"""Workspace sizes of the encoder engine are a contract: fn_encoder_ws_floats / fn_encoder_bwd_ws_floats are pure host
arithmetic over the descriptor and the tuning table (no pointer is dereferenced, nothing is launched), every buffer of the
two workspaces is cut from them in a fixed order, and alignment conditions of the fused paths depend on the addresses that
order gives.  The numbers in tests/golden/engine_ws_sizes.json were recorded from the build BEFORE the engine's host code was
reorganised around the level view; a change of the layout code that moves a buffer shows up here, without a GPU.

``python tests/test_engine_layout_host.py --record FILE`` writes the table of the library on the import path."""
import ctypes as C
import itertools
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_ws_sizes.json")

# key -> (value under test, default to restore); "default" runs the table as the library starts with it
TUNINGS = {"default": None, "22=0": (22, 0, 1), "24=0": (24, 0, 1)}
N, E, F, EF, N_MOLS = 37, 78, 11, 20, 5          # odd on purpose: no count is a multiple of the 64-float granule


def _plan(_lib, n, m, m_real):
    p = _lib.GatPlan()
    p.n, p.m, p.m_real = n, m, m_real
    return p


def _descriptor(_lib, variant, heads, training, drop_p, layers, mol, contiguous, sizes=(N, E, F, EF)):
    n, e, f, ef = sizes
    d = _lib.Encoder()
    d.n_layers, d.heads, d.variant, d.training, d.drop_p = layers, heads, variant, training, drop_p
    d.k_atom0, d.k_bond0, d.k_fbond0, d.k_fattr = 167, 17, 6, 6
    d.N, d.E, d.F, d.EF = n, e, f, ef
    d.bond = _plan(_lib, e, 2 * e - 6 if e else 0, 2 * e - 6 if e else 0)
    d.atom = _plan(_lib, n, e + n, e)                      # the atom graph's edges are the bond nodes, plus one loop per atom
    d.fbond = _plan(_lib, ef, 2 * ef - 6 if ef else 0, 2 * ef - 6 if ef else 0)
    d.frag = _plan(_lib, f, ef, ef)
    d.mol_contiguous = contiguous
    if mol:
        dummy = 0x1000                                     # never dereferenced by the two size functions
        d.n_mols = N_MOLS
        d.mol_atoms.rowptr = d.mol_frags.rowptr = dummy
        d.mol_atoms.n_seg = d.mol_frags.n_seg = N_MOLS
        d.counts_dev = dummy
    return d


def _cases(_lib):
    grid = itertools.product((0, 1, 2), (1, 2, 4, 8), ((0, 0.0), (0, 0.1), (1, 0.0), (1, 0.1)), (1, 3, _lib.FN_MAX_LAYERS), (0, 1), (0, 1))
    for variant, heads, (training, drop_p), layers, mol, contiguous in grid:
        name = f"v{variant}_h{heads}_t{training}_p{drop_p}_L{layers}_mol{mol}_c{contiguous}"
        yield name, _descriptor(_lib, variant, heads, training, drop_p, layers, mol, contiguous)
    # a batch of single-fragment molecules (no fragment connections), and the empty descriptor
    yield "EF0", _descriptor(_lib, 0, 4, 1, 0.1, 3, 1, 1, sizes=(N, E, N_MOLS, 0))
    yield "zero", _descriptor(_lib, 0, 4, 1, 0.0, 2, 0, 0, sizes=(0, 0, 0, 0))


def compute(_lib):
    lib = _lib.load()
    lib.fn_encoder_ws_floats.restype = lib.fn_encoder_bwd_ws_floats.restype = C.c_int64
    lib.fn_encoder_ws_floats.argtypes = lib.fn_encoder_bwd_ws_floats.argtypes = [C.c_void_p]
    out = {}
    for tname, setting in TUNINGS.items():
        try:
            if setting:
                assert lib.fn_set_tuning(setting[0], setting[1]) == 0
            out[tname] = {name: [int(lib.fn_encoder_ws_floats(C.byref(d))), int(lib.fn_encoder_bwd_ws_floats(C.byref(d)))]
                          for name, d in _cases(_lib)}
        finally:
            if setting:
                lib.fn_set_tuning(setting[0], setting[2])
    return out


def test_workspace_sizes_match_the_recorded_layout():
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    with open(GOLDEN) as f:
        want = json.load(f)
    got = compute(_lib)
    assert sorted(got) == sorted(want)
    for tname in want:
        assert sorted(got[tname]) == sorted(want[tname]), tname
        bad = {k: (got[tname][k], v) for k, v in want[tname].items() if got[tname][k] != v}
        assert not bad, f"tuning {tname}: {len(bad)} descriptors changed size, e.g. {sorted(bad.items())[:3]}"
    # the grid is not degenerate: the tuning keys and the descriptor fields it walks do move the sizes
    flat = {t: tuple(map(tuple, want[t].values())) for t in want}
    assert len(set(flat.values())) == len(flat)
    assert len(want["default"]) == 3 * 4 * 4 * 3 * 2 * 2 + 2 and want["default"]["zero"][0] >= 0
    assert len({tuple(v) for v in want["default"].values()}) > 100


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    from fragnet_amd import _lib as lib_module
    with open(sys.argv[2], "w") as fh:
        json.dump(compute(lib_module), fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
