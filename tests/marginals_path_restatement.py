"""Long-double restatement of the marginal path walk (csrc/kernels_marginals.hpp) and the dense answers it is held
against.  No device, no library: numpy only.

A Bayes tree is a list of cliques `(slots, n_frontal, parent, RSd)`:
  slots      the clique's variables, the n_frontal frontal ones first, then the separators
  parent     index of the parent clique in the list (-1: a root)
  RSd        nf x n array, [R S d] row-major: R upper triangular (nf x nf), S the separator columns in the order of `slots`, d the last
             column (not read here); what lmgpu_get_front returns, reshaped by front_matrix()
`dims[slot]` is the dimension of a variable.

Column c of Sigma = (R^T R)^-1 restricted to variable v is x with R^T y = e_c, R x = y, and both solves only touch the path from the clique
v is frontal in to its root: y vanishes below it, x is wanted at v only, and every separator on the way is frontal in an ancestor."""
import numpy as np

LD = np.longdouble


def front_matrix(RSd_colmajor, nf, n):
    """lmgpu_get_front's column-major nf x n buffer as the row-major [R S d]"""
    return np.asarray(RSd_colmajor, dtype=np.float64).reshape(n, nf).T.copy()


def clique_of(cliques, slot):
    for i, (slots, nfv, _, _) in enumerate(cliques):
        if slot in list(slots)[:nfv]:
            return i
    raise KeyError(slot)


def path_of(cliques, slot):
    """clique indices from the clique `slot` is frontal in up to its root"""
    out, c = [], clique_of(cliques, slot)
    while c >= 0:
        out.append(c)
        c = cliques[c][2]
    return out


def _solve_upper_transposed(R, B):
    """Y with R^T Y = B (forward substitution), long double"""
    n = R.shape[0]
    Y = np.zeros_like(B)
    for i in range(n):
        Y[i] = (B[i] - R[:i, i] @ Y[:i]) / R[i, i]
    return Y


def _solve_upper(R, B):
    """X with R X = B (back-substitution), long double"""
    n = R.shape[0]
    X = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - R[i, i + 1:] @ X[i + 1:]) / R[i, i]
    return X


def path_marginal(cliques, dims, slot):
    """the dim x dim marginal covariance of `slot`, long double, by the walk along its path"""
    d = dims[slot]
    path = path_of(cliques, slot)
    vec = {}  # variable -> its d_v x d part of the work vectors (all columns at once); only frontal variables of the path ever enter
    for c in path:
        for s in list(cliques[c][0])[:cliques[c][1]]:
            vec[s] = np.zeros((dims[s], d), dtype=LD)
    vec[slot] = np.eye(d, dtype=LD)
    for c in path:  # up: y_F = R^-T b_F, b_S -= S^T y_F
        slots, nfv, _, RSd = cliques[c]
        slots = list(slots)
        A = np.asarray(RSd, dtype=LD)
        nf = sum(dims[s] for s in slots[:nfv])
        Y = _solve_upper_transposed(A[:, :nf], np.vstack([vec[s] for s in slots[:nfv]]))
        o = 0
        for s in slots[:nfv]:
            vec[s] = Y[o:o + dims[s]]
            o += dims[s]
        for s in slots[nfv:]:
            assert s in vec, "a separator variable that is frontal in no ancestor: not a Bayes tree"
            vec[s] = vec[s] - A[:, o:o + dims[s]].T @ Y
            o += dims[s]
    for c in reversed(path):  # down: x_F = R^-1 (y_F - S x_S)
        slots, nfv, _, RSd = cliques[c]
        slots = list(slots)
        A = np.asarray(RSd, dtype=LD)
        nf = sum(dims[s] for s in slots[:nfv])
        rhs = np.vstack([vec[s] for s in slots[:nfv]])
        o = nf
        for s in slots[nfv:]:
            rhs = rhs - A[:, o:o + dims[s]] @ vec[s]
            o += dims[s]
        X = _solve_upper(A[:, :nf], rhs)
        o = 0
        for s in slots[:nfv]:
            vec[s] = X[o:o + dims[s]]
            o += dims[s]
    out = vec[slot]
    return 0.5 * (out + out.T)


def path_offsets(cliques, dims):
    """the compact work vector's tables, as finalize builds them: poff[root] = 0, poff[child] = poff[parent] + nf[parent]; per clique the
    path positions of its separator scalars"""
    nf = [sum(dims[s] for s in list(sl)[:nfv]) for sl, nfv, _, _ in cliques]
    poff = [None] * len(cliques)

    def place(c):
        if poff[c] is None:
            p = cliques[c][2]
            poff[c] = 0 if p < 0 else place(p) + nf[p]
        return poff[c]

    for c in range(len(cliques)):
        place(c)
    where = {}
    for c, (sl, nfv, _, _) in enumerate(cliques):
        o = 0
        for s in list(sl)[:nfv]:
            where[s] = (c, o)
            o += dims[s]
    spos = []
    for sl, nfv, _, _ in cliques:
        row = []
        for s in list(sl)[nfv:]:
            c, o = where[s]
            row += [poff[c] + o + k for k in range(dims[s])]
        spos.append(row)
    return poff, spos


def inverse_ld(M):
    """inverse of a small matrix in long double: Gauss-Jordan with partial pivoting"""
    A = np.array(M, dtype=LD)
    n = A.shape[0]
    B = np.eye(n, dtype=LD)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            B[[k, p]] = B[[p, k]]
        piv = A[k, k]
        A[k] = A[k] / piv
        B[k] = B[k] / piv
        for i in range(n):
            if i != k and A[i, k] != 0:
                f = A[i, k]
                A[i] = A[i] - f * A[k]
                B[i] = B[i] - f * B[k]
    return B


def cholesky_upper_ld(M):
    """R upper triangular with R^T R = M, long double"""
    A = np.array(M, dtype=LD)
    n = A.shape[0]
    R = np.zeros((n, n), dtype=LD)
    for i in range(n):
        v = A[i, i:] - R[:i, i] @ R[:i, i:]
        assert v[0] > 0, "not positive definite"
        R[i, i:] = v / np.sqrt(v[0])
    return R


def random_bayes_tree(tree, dims, seed):
    """A Bayes tree from a random SPD information matrix with a prescribed elimination tree.

    tree: list of (frontal slots, parent index, separator slots) in elimination order (children before parents); a clique's separators
    must lie in its parent's frontals + separators (the running intersection property), which keeps the fill of the Cholesky factor inside
    the prescribed cliques.  The information matrix is a sum of random Gram blocks, one per clique over its variables, plus a diagonal
    shift; it is factored densely in long double in the tree's order and the factor is cut into the cliques' [R S d].
    Returns (cliques, information matrix (long double, variables in slot order), scalar offsets of the slots)."""
    rng = np.random.default_rng(seed)
    nslots = len(dims)
    off = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    N = int(off[-1])
    for fr, par, sep in tree:
        if par >= 0:
            allowed = set(tree[par][0]) | set(tree[par][2])
            assert set(sep) <= allowed and len(sep) > 0, "separator outside the parent clique"
        else:
            assert len(sep) == 0
    info = np.zeros((N, N), dtype=LD)
    for fr, par, sep in tree:
        cols = np.concatenate([np.arange(off[s], off[s + 1]) for s in list(fr) + list(sep)])
        J = rng.normal(size=(len(cols) + 2, len(cols)))
        info[np.ix_(cols, cols)] += (J.T @ J).astype(LD)
    info += LD(0.5) * np.eye(N, dtype=LD)
    # eliminate in the tree's order
    order = [s for fr, _, _ in tree for s in fr]
    assert sorted(order) == list(range(nslots))
    perm = np.concatenate([np.arange(off[s], off[s + 1]) for s in order])
    R = cholesky_upper_ld(info[np.ix_(perm, perm)])
    pos = {}
    o = 0
    for s in order:
        pos[s] = o
        o += dims[s]
    cliques = []
    for fr, par, sep in tree:
        rows = np.concatenate([np.arange(pos[s], pos[s] + dims[s]) for s in fr])
        cols = np.concatenate([np.arange(pos[s], pos[s] + dims[s]) for s in list(fr) + list(sep)])
        rest = np.setdiff1d(np.arange(N), cols)
        assert np.all(R[np.ix_(rows, rest)] == 0), "fill outside the prescribed clique"
        RSd = np.zeros((len(rows), len(cols) + 1), dtype=LD)
        RSd[:, :-1] = R[np.ix_(rows, cols)]
        cliques.append((list(fr) + list(sep), len(fr), par, RSd))
    return cliques, info, off
