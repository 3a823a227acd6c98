"""What ISAM2's many-marginals / cross-covariance / joint-marginal route (csrc/kernels_isam2_marginals.hpp, csrc/isam2_marginals.hpp; DESIGN
section 19) must produce, restated on a GIVEN Bayes tree: an isam2_walk_reference.Tree built from ISAM2.cliques() / OracleISAM2.cliques().
Numpy only; `dtype` np.longdouble is the reference, np.float64 the same arithmetic in working precision (the floor of a tolerance).

Sigma[:, j] is x with R^T y = e_j, R x = y.  y lives on the path of j (the cliques from the one j is frontal in to its root); x at a
variable i needs the cliques of i's path only, and that path is j's from their junction J -- the deepest clique on both -- to the root.
cross_covariance is written as that WALK: up the source's path, down it again, then down the target's branch (the cliques of its path
strictly below J) with y = 0 there.  Nothing here goes through the global R; test_isam2_joint_reference.py holds the walk against the inverse
of R^T R assembled by isam2_walk_reference.global_R.

The work vector is the kernel's: compact positions (a clique owns [poff, poff + nf), poff = the frontal scalars of its ancestors), the
branch's positions are zeroed before the descent because they overlap those of the source's own branch."""
import numpy as np

LD = np.longdouble


def where(tree):
    """{key: index of the clique it is frontal in}"""
    return {k: i for i, c in enumerate(tree.cliques) for k in c["fk"]}


def path(tree, key):
    """the first frontal keys of the cliques from the one `key` is frontal in to its root (cliques named as Tree.shape() names them)"""
    return [tree.cliques[i]["fk"][0] for i in _path(tree, where(tree)[int(key)])]


def junction(tree, i, j):
    """the first frontal key of the deepest clique on the paths of both keys; None: two trees of a forest"""
    w = where(tree)
    on_j = set(_path(tree, w[int(j)]))
    for c in _path(tree, w[int(i)]):
        if c in on_j:
            return tree.cliques[c]["fk"][0]
    return None


def _path(tree, c):
    out = []
    while c >= 0:
        out.append(c)
        c = tree.cliques[c]["parent"]
    return out


def _tables(tree):
    """poff per clique, the path position of every frontal scalar (by its index in the tree's vectors), the separators' positions per clique"""
    poff = [None] * len(tree.cliques)
    pos = np.full(tree.n, -1, dtype=int)
    for i in tree.order:  # parents first
        c = tree.cliques[i]
        p = c["parent"]
        poff[i] = 0 if p < 0 else poff[p] + tree.cliques[p]["nf"]
        pos[c["fx"]] = poff[i] + np.arange(c["nf"])
    spos = [pos[c["sx"]] for c in tree.cliques]
    for i, c in enumerate(tree.cliques):
        assert np.all(spos[i] >= 0) and np.all(spos[i] < poff[i]), "a separator scalar that is frontal in no ancestor: not a Bayes tree"
    return poff, pos, spos


def path_scalars(tree, key):
    """scalars of the key's path: the length the source rule compares"""
    return sum(tree.cliques[c]["nf"] for c in _path(tree, where(tree)[int(key)]))


def _up(c, p0, sp, W, dtype):
    """R^T y_F = b_F row by row, then b_S -= S^T y_F"""
    A, nf = c["rsd"].astype(dtype), c["nf"]
    for i in range(nf):
        W[p0 + i] = (W[p0 + i] - A[:i, i] @ W[p0:p0 + i]) / A[i, i]
    for k, p in enumerate(sp):
        W[p] = W[p] - A[:, nf + k] @ W[p0:p0 + nf]


def _down(c, p0, sp, W, dtype):
    """x_F = R^-1 (y_F - S x_S), row by row from the last"""
    A, nf = c["rsd"].astype(dtype), c["nf"]
    xs = W[sp] if len(sp) else None
    for i in range(nf - 1, -1, -1):
        s = W[p0 + i].copy()
        if xs is not None:
            s = s - A[i, nf:-1] @ xs
        if i + 1 < nf:
            s = s - A[i, i + 1:nf] @ W[p0 + i + 1:p0 + nf]
        W[p0 + i] = s / A[i, i]


def cross_covariance(tree, i, j, dtype=LD):
    """Sigma[i, j], dims[i] x dims[j], j the source; the (i, i) block is symmetrised (its two triangles differ by rounding only).
    Exact zeros when the keys lie in two trees."""
    i, j = int(i), int(j)
    w = where(tree)
    poff, pos, spos = _tables(tree)
    di, dj = tree.dims[i], tree.dims[j]
    pj = _path(tree, w[j])
    pi = _path(tree, w[i])
    on_j = set(pj)
    J = next((c for c in pi if c in on_j), None)
    if J is None:
        return np.zeros((di, dj), dtype=dtype)
    Lj = poff[w[j]] + tree.cliques[w[j]]["nf"]
    Li = poff[w[i]] + tree.cliques[w[i]]["nf"]
    W = np.full((max(Li, Lj), dj), np.nan, dtype=dtype)  # (what the walk does not zero itself it must never read)
    W[:Lj] = 0
    at_j = pos[tree.off[j]:tree.off[j] + dj]
    W[at_j] = np.eye(dj, dtype=dtype)
    for c in pj:
        _up(tree.cliques[c], poff[c], spos[c], W, dtype)
    for c in reversed(pj):
        _down(tree.cliques[c], poff[c], spos[c], W, dtype)
    branch = pi[:pi.index(J)]
    if branch:
        W[poff[J] + tree.cliques[J]["nf"]:Li] = 0
        for c in reversed(branch):
            _down(tree.cliques[c], poff[c], spos[c], W, dtype)
    blk = W[pos[tree.off[i]:tree.off[i] + di]].copy()
    return 0.5 * (blk + blk.T) if i == j else blk


def source_is_first(tree, a, b):
    """the source of an unordered pair: the key with the shorter path (fewer scalars; ties: the smaller key)"""
    return (path_scalars(tree, a), int(a)) < (path_scalars(tree, b), int(b))


def joint_covariance(tree, keys, dtype=LD):
    """the joint marginal covariance of `keys`, blocks in the order given: every off-diagonal block computed once, from the pair's source,
    and mirrored"""
    keys = [int(k) for k in keys]
    off = np.concatenate([[0], np.cumsum([tree.dims[k] for k in keys])]).astype(int)
    M = np.zeros((off[-1], off[-1]), dtype=dtype)
    for a, ka in enumerate(keys):
        M[off[a]:off[a + 1], off[a]:off[a + 1]] = cross_covariance(tree, ka, ka, dtype)
        for b in range(a + 1, len(keys)):
            kb = keys[b]
            blk = cross_covariance(tree, kb, ka, dtype) if source_is_first(tree, ka, kb) else cross_covariance(tree, ka, kb, dtype).T  # Sigma[kb, ka]
            M[off[b]:off[b + 1], off[a]:off[a + 1]] = blk
            M[off[a]:off[a + 1], off[b]:off[b + 1]] = blk.T
    return M
