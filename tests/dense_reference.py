"""An elimination reference that is NOT a multifrontal algorithm: the whole damped, augmented information matrix
[A b]^T [A b] + lambda D is assembled densely in extended precision (x87 long double, 64-bit mantissa) and factored by ONE
right-looking Cholesky, a row at a time.  The variables are permuted to "frontal keys of front 0, of front 1, ..."; because the
multifrontal factor is that same triangular factor, front i's [R S d] is (rows of its frontal scalars) x (columns of its keys, rhs)
of the dense factor, and delta is the back-substitution of the whole thing.

Plain numpy: no oracle, no product code.  A rank-1 update only visits the columns in which the pivot row is non-zero: an exact
zero contributes nothing, so this is the dense algorithm's arithmetic, not a sparse one's (no symbolic analysis, no tree)."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "dense_reference needs an extended-precision long double (x86: eps = 1.08e-19)"


def _outer_sub(M, r, j0):
    """M[j0:, j0:] -= r r^T over the non-zero columns of r (r indexed like M's columns; r[:j0] is not read)"""
    nz = j0 + np.flatnonzero(r[j0:])
    if nz.size:
        v = r[nz]
        M[np.ix_(nz, nz)] -= np.multiply.outer(v, v)


class DenseReference:
    """factors: [(keys, Ab)] with Ab = [A1 .. Ak b] (whitened, float64); dims: {key: dim}; fronts: [(keys, n_frontal_keys)] in front
    order (frontal keys first).  diagonal = False: D = I;  True: D = clamp(diag(A^T A), min_diag, max_diag)."""

    def __init__(self, factors, dims, lam, diagonal, fronts, min_diag=1e-6, max_diag=1e32):
        order = [k for keys, nfk in fronts for k in keys[:nfk]]
        assert sorted(order) == sorted(dims), "the fronts' frontal keys must be a permutation of the variables"
        self.off, n = {}, 0
        for k in order:
            self.off[k] = n
            n += dims[k]
        self.n, self.dims, self.fronts = n, dims, fronts
        H = np.zeros((n + 1, n + 1), dtype=LD)
        for keys, Ab in factors:
            cols = np.concatenate([np.arange(self.off[k], self.off[k] + dims[k]) for k in keys] + [[n]])
            assert Ab.shape[1] == cols.size
            A = np.asarray(Ab, dtype=np.float64).astype(LD)
            H[np.ix_(cols, cols)] += A.T @ A
        if lam > 0.0:
            d = np.diagonal(H)[:n].copy()
            D = np.minimum(np.maximum(d, LD(min_diag)), LD(max_diag)) if diagonal else np.ones(n, dtype=LD)
            H[np.arange(n), np.arange(n)] += LD(lam) * D
        hmax = np.abs(H).max()
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
        self.R = W[:n]  # (n, n + 1): [R d]
        # residual of the factorisation over the whole augmented matrix except the (rhs, rhs) corner (never factored)
        G = H
        for j in range(n):
            _outer_sub(G, self.R[j], j)
        G[n, n] = 0
        self.residual = float(np.abs(np.triu(G)).max() / hmax)
        # back-substitution R delta = d
        x = np.zeros(n, dtype=LD)
        for j in range(n - 1, -1, -1):
            x[j] = (self.R[j, n] - self.R[j, j + 1:n] @ x[j + 1:]) / self.R[j, j]
        self._x = x

    def front(self, i):
        """[R S d] of front i: (nf, n_front) in the front's own key order"""
        keys, nfk = self.fronts[i]
        rows = np.concatenate([np.arange(self.off[k], self.off[k] + self.dims[k]) for k in keys[:nfk]])
        cols = np.concatenate([np.arange(self.off[k], self.off[k] + self.dims[k]) for k in keys] + [[self.n]])
        return self.R[np.ix_(rows, cols)]

    def delta(self):
        return {k: self._x[o:o + self.dims[k]] for k, o in self.off.items()}
