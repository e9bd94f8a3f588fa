"""The self-Jaccard distance of the k-reciprocal re-rank restated in numpy (reranking.py:86-93 for
every row against every column of one set), and the data the Jaccard clustering tests share.

    jd(i, j) = 1 - tm / (2 - tm),   tm = sum over the nonzero columns c of V_qe[i], ascending, of
                                         min(V_qe[i, c], V_qe[j, c])

with every operation an fp16 numpy operation, so the sum is sequential in fp16.  Both helpers are
checked against the C oracle's `jac` in tests/test_jaccard_ref.py; the sparse one is the reference
where the oracle's dense path is too slow (tests/test_gpu_cluster_jaccard.py, two chunks)."""
import numpy as np


def _f16(a):
    a = np.asarray(a)
    return a.view(np.float16) if a.dtype in (np.uint16, np.int16) else a.astype(np.float16, copy=False)


def jaccard_self_dense(V16):
    """fp16 [N][N] from the dense V_qe (fp16, or its bits as uint16)."""
    V = _f16(V16)
    n = V.shape[0]
    assert V.shape == (n, n)
    out = np.empty((n, n), np.float16)
    for i in range(n):
        tm = np.zeros(n, np.float16)
        for c in np.flatnonzero(V[i]):  # ascending
            tm = tm + np.minimum(V[i, c], V[:, c])  # rows without column c add 0
        out[i] = 1 - tm / (2 - tm)
    return out


def jaccard_self_csr(off, col, val):
    """fp16 [N][N] from V_qe as CSR (off int64 [N + 1], col ascending in every row, val fp16 or its
    bits): row by row over the inverted lists, so a pair without a shared column is never visited
    and keeps jd = 1."""
    off, col, val = np.asarray(off, np.int64), np.asarray(col, np.int64), _f16(val)
    n = len(off) - 1
    row = np.repeat(np.arange(n), np.diff(off))
    order = np.lexsort((row, col))  # the inverted index: by column, rows ascending
    irow, ival = row[order], val[order]
    coff = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=coff[1:])
    out = np.ones((n, n), np.float16)
    tm = np.zeros(n, np.float16)
    for i in range(n):
        touched = []
        for e in range(off[i], off[i + 1]):
            c = col[e]
            r = irow[coff[c]:coff[c + 1]]
            tm[r] = tm[r] + np.minimum(val[e], ival[coff[c]:coff[c + 1]])
            touched.append(r)
        if touched:
            r = np.unique(np.concatenate(touched))
            out[i, r] = 1 - tm[r] / (2 - tm[r])
            tm[r] = 0
    return out


def dense_to_csr(V16):
    """(off, col, val bits) of a dense V_qe given as fp16 bits (-0 is no entry)."""
    V = np.asarray(V16).view(np.uint16)
    nz = (V & 0x7fff) != 0
    off = np.zeros(len(V) + 1, np.int64)
    np.cumsum(nz.sum(1), out=off[1:])
    r, c = np.nonzero(nz)
    return off, c.astype(np.int32), V[r, c]


def identities(n_ids, members, outliers, D, seed=0):
    """fp32 [n_ids * members + outliers][D], L2-normalised: n_ids centres drawn from N(0, 1), every
    member its centre + 0.35 N(0, 1), then the outliers at 1.5 N(0, 1)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_ids, D))
    x = np.repeat(centres, members, axis=0) + 0.35 * rng.standard_normal((n_ids * members, D))
    x = np.concatenate([x, 1.5 * rng.standard_normal((outliers, D))])
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), dtype=np.float32)


def fixture(D):
    """The 232-row set of the Jaccard clustering tests: 24 identities of 8 and 40 outliers."""
    return identities(24, 8, 40, D)
