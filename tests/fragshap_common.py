"""Shared by the fragment-Shapley tests: the fixture tests/golden/frag_shapley.npz (tests/golden/make_golden_fragshap.py: the reference's
model_attr classes on one record per coalition) and Shapley values by the definition (all F! orders)."""
import itertools
import json
import os

import numpy as np

from tests import attr_common as ac
from tests.helpers import GOLDEN

CASES = ("property", "property_groups", "energy")
# share of (molecule, group) entries whose reference |phi| exceeds 10 x the attribution tolerance
MIN_SHARE = {"property": 0.75, "property_groups": 0.75, "energy": 0.5}
ROWS = {"property": 372, "property_groups": 48, "energy": 372}

_FIXTURE = {}


def fixture():
    if not _FIXTURE:
        z = np.load(os.path.join(GOLDEN, "frag_shapley.npz"))
        _FIXTURE.update({k: z[k] for k in z.files})
        _FIXTURE["cfg"] = json.loads(str(z["cfg"]))
    return _FIXTURE


def reference(case):
    """(mask int64 [rows, 2] (molecule, mask), value [rows, C] fp32, phi float64 [R, C], groups per molecule)."""
    z = fixture()
    return z[f"{case}/mask"], z[f"{case}/value"], z[f"{case}/phi"], z["cfg"]["cases"][case]["groups"]


def by_orders(values, F):
    """phi [F, C] (float64) of v [2^F, C], row index = mask: the mean marginal over all F! orders of the groups."""
    v = np.asarray(values, dtype=np.float64)
    phi = np.zeros((F, v.shape[1]), dtype=np.float64)
    orders = list(itertools.permutations(range(F)))
    for order in orders:
        m = 0
        for f in order:
            phi[f] += v[m | (1 << f)] - v[m]
            m |= 1 << f
    return phi / len(orders)


def share_above_tolerance(case):
    """(entries above 10 x tolerance, entries): the tolerance of an attribution of the molecule's full prediction v(all)."""
    mask, value, phi, groups = reference(case)
    big = []
    first = 0
    for i, F in enumerate(groups):
        v = value[mask[:, 0] == i]
        big.append((np.abs(phi[first: first + F]) > 10 * ac.attr_tolerance(v[-1].astype(np.float64))).all(axis=1))
        first += F
    big = np.concatenate(big)
    return int(big.sum()), int(big.shape[0])
