"""float64 reference of the nearest-neighbour lists (csrc/topk.hip): scores per metric, then one lexicographic sort.

The order is total: better score first (larger for dot and cosine, smaller for squared L2), and on equal score the smaller global
index.  Empty slots are index -1 with score -inf (+inf for L2).  Nothing here touches the GPU."""
import numpy as np

METRICS = {"dot": 0, "cosine": 1, "l2": 2}


def empty_score(metric):
    return np.inf if metric == 2 else -np.inf


def rnorm(x):
    x = np.asarray(x, dtype=np.float64)
    return 1.0 / np.maximum(np.sqrt((x * x).sum(1)), 1e-12)


def scores(q, lib, metric, q_aux=None, lib_aux=None):
    """[n_q, n_lib] float64.  cosine: dot * (q_aux[i] * lib_aux[j]), the reciprocal norms; l2: (q_aux[i] + lib_aux[j]) - 2 dot, the
    squared norms.  The auxiliary vectors default to their float64 values."""
    q, lib = np.asarray(q, dtype=np.float64), np.asarray(lib, dtype=np.float64)
    dot = q @ lib.T
    if metric == 0:
        return dot
    if metric == 1:
        qa = rnorm(q) if q_aux is None else np.asarray(q_aux, dtype=np.float64)
        la = rnorm(lib) if lib_aux is None else np.asarray(lib_aux, dtype=np.float64)
        return dot * (qa[:, None] * la[None, :])
    if metric == 2:
        qa = (q * q).sum(1) if q_aux is None else np.asarray(q_aux, dtype=np.float64)
        la = (lib * lib).sum(1) if lib_aux is None else np.asarray(lib_aux, dtype=np.float64)
        return (qa[:, None] + la[None, :]) - 2.0 * dot
    raise ValueError(f"metric {metric!r}")


def fresh(n_q, k, metric):
    return np.full((n_q, k), empty_score(metric)), np.full((n_q, k), -1, dtype=np.int64)


def select(score, index, k, metric):
    """The k best of the candidates (score [m], index [m]; index -1 = an empty slot, dropped) as padded lists of length k."""
    score, index = np.asarray(score, dtype=np.float64), np.asarray(index, dtype=np.int64)
    keep = index >= 0
    score, index = score[keep], index[keep]
    order = np.lexsort((index, score if metric == 2 else -score))[:k]
    out_s, out_i = np.full(k, empty_score(metric)), np.full(k, -1, dtype=np.int64)
    out_s[:len(order)], out_i[:len(order)] = score[order], index[order]
    return out_s, out_i


def update(state, sc, index_base, metric, exclude=None):
    """Folds the chunk whose scores are sc [n_q, n_lib] (global ids index_base + j) into state = (score [n_q, k], index [n_q, k])."""
    best_s, best_i = state
    n_q, k = best_s.shape
    ids = index_base + np.arange(sc.shape[1], dtype=np.int64)
    out_s, out_i = np.empty_like(best_s), np.empty_like(best_i)
    for i in range(n_q):
        keep = np.ones(len(ids), dtype=bool) if exclude is None or exclude[i] < 0 else ids != exclude[i]
        out_s[i], out_i[i] = select(np.concatenate([best_s[i], sc[i][keep]]), np.concatenate([best_i[i], ids[keep]]), k, metric)
    return out_s, out_i


def topk(q, lib, k, metric, index_base=0, exclude=None, chunk=None, q_aux=None, lib_aux=None):
    """The lists after the whole library, fed in chunks of `chunk` rows (None: one chunk)."""
    sc = scores(q, lib, metric, q_aux, lib_aux)
    state = fresh(sc.shape[0], k, metric)
    step = sc.shape[1] if not chunk else chunk
    for j0 in range(0, sc.shape[1], max(step, 1)):
        state = update(state, sc[:, j0:j0 + step], index_base + j0, metric, exclude)
    return state


def check_lists(score, index, ref_scores, metric, index_base=0, exclude=None, rtol=1e-4, atol=1e-4):
    """The conditions a list must meet where near-ties make index equality a test of rounding: sorted scores; distinct indices in range;
    every score within atol + rtol |ref| of the reference score of that same index; no row outside the list better than the list's last
    score by more than that tolerance.  ref_scores [n_q, n_lib] float64.  Returns the largest |score - ref| seen."""
    score, index = np.asarray(score, dtype=np.float64), np.asarray(index, dtype=np.int64)
    n_q, n_lib = ref_scores.shape
    sgn = -1.0 if metric == 2 else 1.0
    worst = 0.0
    for i in range(n_q):
        banned = -1 if exclude is None else int(exclude[i])
        n_cand = n_lib - (1 if index_base <= banned < index_base + n_lib else 0)
        n_full = min(score.shape[1], n_cand)
        idx, sc = index[i, :n_full], score[i, :n_full]
        assert (index[i, n_full:] == -1).all() and (score[i, n_full:] == empty_score(metric)).all(), f"query {i}: padding"
        assert (np.diff(sgn * sc) <= 0).all(), f"query {i}: scores not sorted best first: {sc}"
        assert len(set(idx.tolist())) == n_full and (idx >= index_base).all() and (idx < index_base + n_lib).all(), f"query {i}: {idx}"
        assert banned not in idx.tolist(), f"query {i}: the excluded row {banned} is in the list"
        ref = ref_scores[i, idx - index_base]
        tol = atol + rtol * np.abs(ref)
        assert (np.abs(sc - ref) <= tol).all(), f"query {i}: scores {sc} against the reference {ref}"
        worst = max(worst, float(np.abs(sc - ref).max()) if n_full else 0.0)
        if n_full:
            outside = np.ones(n_lib, dtype=bool)
            outside[idx - index_base] = False
            if index_base <= banned < index_base + n_lib:
                outside[banned - index_base] = False
            if outside.any():
                best_out = (sgn * ref_scores[i][outside]).max()
                last = sgn * sc[-1]
                assert best_out <= last + atol + rtol * abs(last), f"query {i}: a row outside the list scores {sgn * best_out}, last is {sc[-1]}"
    return worst
