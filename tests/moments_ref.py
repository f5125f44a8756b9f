"""Float64 numpy references of the moments and projection kernels (csrc/moments.hip) and of the host solver (fragnet_amd/chemspace.py).
``z = x - shift`` is formed in fp32 exactly as the kernels form it (one fp32 subtraction per element); everything after that is float64.
The error bounds are Higham's for an fp32 chain of fused multiply-adds, gamma_t = t u / (1 - t u) with u = 2^-24: derived, not measured."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(terms: int) -> float:
    return terms * U32 / (1.0 - terms * U32)


def z_of(x, shift=None) -> np.ndarray:
    """float64 copy of the fp32 difference the kernels compute."""
    x = np.asarray(x, dtype=np.float32)
    z = x if shift is None else x - np.asarray(shift, dtype=np.float32)[None, :]
    assert z.dtype == np.float32
    return z.astype(np.float64)


def moments(x, shift=None):
    """(sum [d], gram [d, d]) of z in float64."""
    z = z_of(x, shift)
    return z.sum(0), z.T @ z


def moments_bound(x, shift, chunk: int):
    """Entrywise bounds (sum, gram) on |device - float64 reference|: an L-term fp32 chain per chunk, L = min(n, chunk), plus the fp64
    folds of the chunk results (fewer than n additions, 2^-52 each is generous) -- against the sums of magnitudes."""
    z = np.abs(z_of(x, shift))
    n = z.shape[0]
    g = gamma(min(n, chunk)) + n * 2.0 ** -52
    return g * z.sum(0), g * (z.T @ z)


def project(x, W, shift=None):
    """(out [n, k], bound [n, k]) in float64: z @ W and gamma_d |z| @ |W|."""
    z, W = z_of(x, shift), np.asarray(W, dtype=np.float32).astype(np.float64)
    return z @ W, gamma(z.shape[1]) * (np.abs(z) @ np.abs(W))


def sq_of(out):
    """(sq [n], bound [n]) of a device ``out`` [n, k]: its float64 sum of squares and gamma_k of it."""
    o = np.asarray(out, dtype=np.float64)
    s = (o * o).sum(1)
    return s, gamma(o.shape[1]) * s


# ---- the host solver
def pca(rows):
    """float64 reference of the solver through the SVD of the centred rows: (mean, eigenvalues descending [min(n, d) padded with zeros to
    d], components [d, d] whose leading columns are the right singular vectors, signed by the largest-magnitude rule)."""
    rows = np.asarray(rows, dtype=np.float64)
    n, d = rows.shape
    mean = rows.mean(0)
    _, s, vt = np.linalg.svd(rows - mean, full_matrices=n < d)        # vt is [d, d] either way
    eig = np.zeros(d)
    eig[:s.shape[0]] = s ** 2 / n
    v = vt.T.copy()
    for c in range(d):
        if v[int(np.argmax(np.abs(v[:, c]))), c] < 0:
            v[:, c] = -v[:, c]
    return mean, eig, v


def mahalanobis(rows, mean, eigenvalues, components, rank):
    """float64 squared Mahalanobis distance with the pseudo-inverse of the leading ``rank`` directions."""
    t = (np.asarray(rows, dtype=np.float64) - mean) @ components[:, :rank]
    return (t * t / eigenvalues[:rank]).sum(1)
