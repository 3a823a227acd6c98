"""An elimination reference that is NOT a multifrontal algorithm: the whole damped, augmented information matrix
[A b]^T [A b] + lambda D is assembled densely in extended precision (x87 long double, 64-bit mantissa) and factored by ONE
right-looking Cholesky, a row at a time.  The variables are permuted to "frontal keys of front 0, of front 1, ..."; because the
multifrontal factor is that same triangular factor, front i's [R S d] is (rows of its frontal scalars) x (columns of its keys, rhs)
of the dense factor, and delta is the back-substitution of the whole thing.

Plain numpy: no oracle, no product code.  A rank-1 update only visits the columns in which the pivot row is non-zero: an exact
zero contributes nothing, so this is the dense algorithm's arithmetic, not a sparse one's (no symbolic analysis, no tree).

block = 0 is that row-at-a-time form.  block = 16..64 is the blocked right-looking variant for dense fronts of a thousand columns
(the row-at-a-time form needs a minute there): panels of `block` rows, rank-1 steps inside the panel, then ONE trailing update
W[j1:, j1:] -= P^T P per panel (again over the non-zero columns of P only); everything stays np.longdouble.  The residual of the
blocked variant is R^T R - H over the whole upper triangle too, computed block by block on contiguous copies."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "dense_reference needs an extended-precision long double (x86: eps = 1.08e-19)"


def _outer_sub(M, r, j0):
    """M[j0:, j0:] -= r r^T over the non-zero columns of r (r indexed like M's columns; r[:j0] is not read)"""
    nz = j0 + np.flatnonzero(r[j0:])
    if nz.size:
        v = r[nz]
        M[np.ix_(nz, nz)] -= np.multiply.outer(v, v)


def _factor_blocked(H, n, nb):
    """[R d] (n, n + 1): upper Cholesky of the leading n columns of the augmented matrix H, panels of nb rows"""
    W = H.copy()
    for j0 in range(0, n, nb):
        j1 = min(n, j0 + nb)
        for j in range(j0, j1):
            p = W[j, j]
            assert p > 0, f"pivot {j} is not positive"
            W[j, j:] /= np.sqrt(p)
            if j + 1 < j1:
                W[j + 1:j1, j + 1:] -= np.multiply.outer(W[j, j + 1:j1], W[j, j + 1:])
        P = W[j0:j1, j1:]
        nz = np.flatnonzero(P.any(axis=0))
        if nz.size == P.shape[1]:
            P = np.ascontiguousarray(P)
            W[j1:, j1:] -= P.T @ P
        elif nz.size:
            P = np.ascontiguousarray(P[:, nz])
            W[np.ix_(j1 + nz, j1 + nz)] -= P.T @ P
    W[np.tril_indices(n + 1, -1)] = 0
    return W[:n]


def _residual_blockwise(H, R, n, nb=64):
    """max |R^T R - H| over the whole upper triangle of the augmented matrix except the (rhs, rhs) corner (never factored):
    block (I, J), I <= J, is (rows of R above the end of I)[:, I]^T [:, J], on contiguous copies of the column blocks"""
    worst = LD(0)
    cols = [np.ascontiguousarray(R[:min(n, j0 + nb), j0:j0 + nb]) for j0 in range(0, n + 1, nb)]
    live = [c.any(axis=1) for c in cols]  # rows of R that are not all zero within the column block: only they contribute
    for bi, i0 in enumerate(range(0, n + 1, nb)):
        k = cols[bi].shape[0]  # rows of R that reach column block I: R is upper triangular
        for bj in range(bi, len(cols)):
            j0 = bj * nb
            rows = np.flatnonzero(live[bi] & live[bj][:k])
            G = np.ascontiguousarray(cols[bi][rows].T) @ cols[bj][rows] - H[i0:i0 + nb, j0:j0 + nb]
            if bi == bj:
                G = np.triu(G)
            if j0 + G.shape[1] == n + 1 and i0 + G.shape[0] == n + 1:
                G[-1, -1] = 0
            worst = max(worst, np.abs(G).max())
    return worst


def augmented_information(factors, dims, lam, diagonal, fronts, min_diag=1e-6, max_diag=1e32):
    """([A b]^T [A b] + lambda D as an (n + 1, n + 1) long-double matrix, {key: first column}, n) in the fronts' variable order"""
    order = [k for keys, nfk in fronts for k in keys[:nfk]]
    assert sorted(order) == sorted(dims), "the fronts' frontal keys must be a permutation of the variables"
    off, n = {}, 0
    for k in order:
        off[k] = n
        n += dims[k]
    H = np.zeros((n + 1, n + 1), dtype=LD)
    for keys, Ab in factors:
        cols = np.concatenate([np.arange(off[k], off[k] + dims[k]) for k in keys] + [[n]])
        assert Ab.shape[1] == cols.size
        A = np.asarray(Ab, dtype=np.float64).astype(LD)
        H[np.ix_(cols, cols)] += A.T @ A
    if lam > 0.0:
        d = np.diagonal(H)[:n].copy()
        D = np.minimum(np.maximum(d, LD(min_diag)), LD(max_diag)) if diagonal else np.ones(n, dtype=LD)
        H[np.arange(n), np.arange(n)] += LD(lam) * D
    return H, off, n


class FactorView:
    """a factor [R d] (n, n + 1) in the fronts' variable order, read front by front; delta by back-substitution in R's own precision.
    (DenseReference is one; a test can wrap any other factor of the same matrix -- a float64 one with a planted defect -- to put it
    through the same comparison.)"""

    def __init__(self, R, off, dims, fronts):
        self.R, self.off, self.dims, self.fronts, self.n = R, off, dims, fronts, R.shape[0]
        n = self.n
        x = np.zeros(n, dtype=R.dtype)
        for j in range(n - 1, -1, -1):
            x[j] = (R[j, n] - R[j, j + 1:n] @ x[j + 1:]) / R[j, j]
        self._x = x

    def front(self, i):
        """[R S d] of front i: (nf, n_front) in the front's own key order"""
        keys, nfk = self.fronts[i]
        rows = np.concatenate([np.arange(self.off[k], self.off[k] + self.dims[k]) for k in keys[:nfk]])
        cols = np.concatenate([np.arange(self.off[k], self.off[k] + self.dims[k]) for k in keys] + [[self.n]])
        return self.R[np.ix_(rows, cols)]

    def delta(self):
        return {k: self._x[o:o + self.dims[k]] for k, o in self.off.items()}


class DenseReference(FactorView):
    """factors: [(keys, Ab)] with Ab = [A1 .. Ak b] (whitened, float64); dims: {key: dim}; fronts: [(keys, n_frontal_keys)] in front
    order (frontal keys first).  diagonal = False: D = I;  True: D = clamp(diag(A^T A), min_diag, max_diag)."""

    def __init__(self, factors, dims, lam, diagonal, fronts, min_diag=1e-6, max_diag=1e32, block=0):
        assert block == 0 or 16 <= block <= 64
        H, off, n = augmented_information(factors, dims, lam, diagonal, fronts, min_diag, max_diag)
        self.hmax = np.abs(H).max()
        if block:
            R = _factor_blocked(H, n, block)
            self.residual = float(_residual_blockwise(H, R, n) / self.hmax)
        else:
            R = self._factor_by_rows(H, n)
        super().__init__(R, off, dims, fronts)

    def _factor_by_rows(self, H, n):
        # right-looking Cholesky of the upper triangle, in place on a copy: row j is scaled, then subtracted from the trailing block
        W = H.copy()
        for j in range(n):
            p = W[j, j]
            assert p > 0, f"pivot {j} is not positive"
            W[j, j:] /= np.sqrt(p)
            r = W[j].copy()
            r[j] = 0  # the update starts at column j + 1
            _outer_sub(W, r, j + 1)
        W[np.tril_indices(n + 1, -1)] = 0
        R = W[:n]  # (n, n + 1): [R d]
        # residual of the factorisation over the whole augmented matrix except the (rhs, rhs) corner (never factored)
        G = H
        for j in range(n):
            _outer_sub(G, R[j], j)
        G[n, n] = 0
        self.residual = float(np.abs(np.triu(G)).max() / self.hmax)
        return R
