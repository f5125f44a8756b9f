"""fn_set_tuning validates: every live key has a [min, max] range (one table in csrc/fragnet_hip.hip, stated at the FN_TUNE_* defines
of the header), a value outside it is refused with FN_EINVAL and leaves the table as it was, fn_get_tuning reads a key back.

No GPU: the table is host state of the library, which loads without a device.  The refused values are only ever handed to
fn_set_tuning -- a block count of zero divides by zero on the host, FN_TUNE_RD_BLOCKS above FN_MAX_PART makes the columns of the
column-major row-dots partials overlap and the last one run past its buffer; nothing may be launched with them."""
import os
import re

import pytest

from tests import launch_geometry_common as G
from tests.conftest import ROOT

FN_EINVAL = -1
RETIRED = (2, 4, 5, 6, 9, 15, 16, 17, 18, 19, 29)
BLOCK_KEYS = (0, 3, 10, 11, 12, 13, 23)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from fragnet_amd import _lib
    from fragnet_amd.build import build_lib
    build_lib()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "fragnet_hip.h")).read()


def _documented_defaults():
    """The initialiser as the header documents it ("The table at load, in key order")."""
    found = re.search(r"The table at load, in key order[^:]*:\s*\n\s*\*\s*((?:-?\d+,\s*)+-?\d+)", _header())
    assert found, "the header no longer documents the table at load"
    return [int(v) for v in found.group(1).split(",")]


def _count():
    return int(re.search(r"#define FN_TUNE_COUNT (\d+)", _header()).group(1))


def _table(lib):
    return [lib.fn_get_tuning(k) for k in range(_count())]


def test_defaults_at_load_are_the_documented_initialiser(lib):
    want = _documented_defaults()
    assert len(want) == _count() == 35
    assert _table(lib) == want
    # ... which is the initialiser of the source
    src = open(os.path.join(ROOT, "fragnet_amd", "csrc", "fragnet_hip.hip")).read()
    init = re.search(r"int g_tune\[FN_TUNE_COUNT\] = \{([^}]*)\}", src).group(1)
    assert [int(v) for v in init.split(",")] == want
    assert lib.fn_get_tuning(-1) == 0 and lib.fn_get_tuning(_count()) == 0


def test_every_default_and_every_swept_value_is_accepted(lib):
    before = _table(lib)
    try:
        for k, v in enumerate(before):
            assert lib.fn_set_tuning(k, v) == 0, (k, v, lib.fn_last_error())
        swept = G.all_settings()
        assert len(swept) >= 40 and {k for s in swept for k in s} == {0, 1, 3, 10, 11, 12, 13, 21, 22, 23, 24, 25}
        for setting in swept:
            for k, v in setting.items():
                assert lib.fn_set_tuning(k, v) == 0, (k, v, lib.fn_last_error())
                assert lib.fn_get_tuning(k) == v
        # the values the other tests and tools of the project set
        for k, v in [(7, 0), (8, 0), (14, 0), (14, 2), (20, 0), (20, 2), (22, 0), (24, 0), (26, 0), (28, 1), (32, 0), (33, 0), (34, 0), (34, 2),
                     (34, 10 ** 6), (10, 8), (30, 0), (30, 64), (31, 0), (13, 4096), (23, 4096), (12, 1024), (11, 4096), (27, 4)]:
            assert lib.fn_set_tuning(k, v) == 0, (k, v, lib.fn_last_error())
        for k in RETIRED:
            for v in (INT_MIN, -1, 0, 1, INT_MAX):
                assert lib.fn_set_tuning(k, v) == 0, (k, v)
    finally:
        for k, v in enumerate(before):
            assert lib.fn_set_tuning(k, v) == 0
    assert _table(lib) == before


REFUSED = ([(10, 0), (10, -1), (13, 4096 + 1), (0, 0), (0, -5)]
           + [(k, v) for k in BLOCK_KEYS for v in (0, -1, INT_MIN)]
           + [(11, 4097), (12, 1025), (23, 4097), (12, INT_MAX), (23, INT_MAX)]
           + [(21, 0), (21, 100), (21, -23), (27, 0), (27, -1), (27, 4097), (1, -1), (30, -1), (31, -1), (34, -1)]
           + [(k, v) for k in (7, 8, 22, 24, 25, 26, 28, 32, 33) for v in (-1, 2)]
           + [(14, -1), (14, 3), (20, -1), (20, 3)])
REFUSED = list(dict.fromkeys(REFUSED))


@pytest.mark.parametrize("key,value", REFUSED)
def test_out_of_range_values_are_refused_and_change_nothing(lib, key, value):
    from fragnet_amd import _lib
    assert _lib.FN_MAX_PART == 4096
    before = _table(lib)
    assert lib.fn_set_tuning(key, value) == FN_EINVAL
    msg = lib.fn_last_error().decode()
    assert msg.startswith("fn_set_tuning") and re.search(r"\bkey %d\b" % key, msg), msg
    name = re.search(r"#define FN_TUNE_(\w+) %d\b" % key, _header()).group(1)
    assert name in msg, msg
    assert lib.fn_get_tuning(key) == before[key]
    assert _table(lib) == before
    with pytest.raises(_lib.FragnetHipError, match="key %d" % key):
        _lib.call("fn_set_tuning", key, value)
    assert _table(lib) == before


@pytest.mark.parametrize("key", [-1, 35, 1000, INT_MIN])
def test_an_unknown_key_is_refused(lib, key):
    before = _table(lib)
    assert lib.fn_set_tuning(key, 1) == FN_EINVAL
    assert b"unknown key" in lib.fn_last_error()
    assert _table(lib) == before


def test_ranges_at_the_defines_are_the_ranges_of_the_table(lib):
    """The comment at every live key's define states its range as [lo, hi]: lo and hi are accepted, lo - 1 and hi + 1 are refused."""
    text = _header()
    words = {"FN_MAX_PART": 4096, "INT_MAX": INT_MAX, "2^20": 2 ** 20}
    before = _table(lib)
    stated = {}
    for m in re.finditer(r"FN_TUNE_(\w+) \[(\w+|\d+\^\d+), (\w+|\d+\^\d+)\]", text):                  # the two keys named in the opening comment
        stated[int(re.search(r"#define FN_TUNE_%s (\d+)" % m.group(1), text).group(1))] = (m.group(2), m.group(3))
    for m in re.finditer(r"#define FN_TUNE_\w+ (\d+)\b(.*?)(?=#define FN_TUNE_|int fn_set_tuning)", text, flags=re.S):
        r = re.findall(r"\[(\w+|\d+\^\d+), (\w+|\d+\^\d+)\] \*/", m.group(2))
        if r:
            stated[int(m.group(1))] = r[-1]
    live = [k for k in range(_count()) if k not in RETIRED]
    assert sorted(stated) == live, sorted(set(live) ^ set(stated))
    try:
        for k, (lo, hi) in stated.items():
            lo, hi = (words[w] if w in words else int(w) for w in (lo, hi))
            assert lo <= before[k] <= hi, k
            assert lib.fn_set_tuning(k, lo) == 0 and lib.fn_set_tuning(k, hi) == 0, k
            assert lib.fn_set_tuning(k, lo - 1) == FN_EINVAL, k
            if hi < INT_MAX:
                assert lib.fn_set_tuning(k, hi + 1) == FN_EINVAL, k
            assert lib.fn_get_tuning(k) == hi
    finally:
        for k, v in enumerate(before):
            assert lib.fn_set_tuning(k, v) == 0
    assert _table(lib) == before


def test_tuning_context_manager_restores_what_it_found(lib):
    from fragnet_amd import _lib
    from tests.helpers import tuning, tuning_key
    before = _table(lib)
    assert tuning_key("ONE_BLOCKS") == 23 and tuning_key("fwd_blocks_eval") == 10
    assert lib.fn_set_tuning(23, 99) == 0                                   # not the default: the manager restores what it FOUND
    try:
        with tuning({23: 7, 25: 1}, RD_BLOCKS=3):
            assert (lib.fn_get_tuning(23), lib.fn_get_tuning(25), lib.fn_get_tuning(13)) == (7, 1, 3)
            with tuning({23: 40}):
                assert lib.fn_get_tuning(23) == 40
            assert lib.fn_get_tuning(23) == 7
        assert (lib.fn_get_tuning(23), lib.fn_get_tuning(25), lib.fn_get_tuning(13)) == (99, before[25], before[13])
        with pytest.raises(ZeroDivisionError):
            with tuning({12: 3}):
                1 / 0
        assert lib.fn_get_tuning(12) == before[12]
        with pytest.raises(_lib.FragnetHipError):                          # the second value is refused: the first is put back
            with tuning({23: 5, 13: 4097}):
                raise AssertionError("the body must not run")
        assert (lib.fn_get_tuning(23), lib.fn_get_tuning(13)) == (99, before[13])
    finally:
        lib.fn_set_tuning(23, before[23])
    assert _table(lib) == before


def test_swept_values_reach_the_regimes_the_defaults_never_do():
    """Host arithmetic only: at the defaults every level of the 51-molecule batch has one row per half-wave; the swept values of the
    one-pass key cover 1, 2, 3 and >= 8 rows, the single-block launch and a last block with idle half-waves."""
    n = G.EDGES_ROWS["bond"]
    assert G.geometry(n, 768) == (1, 167) and G.geometry(n, 1) == (167, 1)
    geo = [G.geometry(n, v) for v in G.ONE_BLOCKS_VALUES]
    assert {1, 2, 3} <= {r for r, _ in geo} and any(r >= 8 for r, _ in geo) and any(b == 1 for _, b in geo)
    assert any(n % (G.ROWS * r) for r, _ in geo)
