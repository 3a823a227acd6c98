"""Long-double restatement of the cross-covariance walk (csrc/kernels_marginals.hpp, marginal_cross_kernel) on the
cliques of tests/marginals_path_restatement.py.  No device, no library: numpy only.

Sigma[:, j] is x with R^T y = e_j, R x = y.  y lives on j's path; x at a variable i needs the fronts of i's path only, and that path is
j's from their junction J (the deepest clique on both) up to the root.  So: up j's path, down j's path, then down i's BRANCH (the cliques
of i's path strictly below J) with y = 0 there.

The vector handling is the kernel's: ONE work vector of compact positions (mr.path_offsets: a clique owns [poff, poff + nf), poff depends
on its ancestors only, so the shared part of two paths has the same positions in both), the branch's positions [poff[J] + nf[J], L_i) are
zeroed before the descent because they overlap those of j's own branch, and the targets of one source are taken deepest junction first: a
branch descent destroys x of j's path below its junction, which a target with a junction no deeper does not read.  cross_blocks() asserts
that order; out of order it fails."""
import numpy as np

import marginals_path_restatement as mr

LD = mr.LD


def junction(cliques, slot_a, slot_b):
    """the deepest clique on the paths of both variables; None: different trees"""
    pb = set(mr.path_of(cliques, slot_b))
    for c in mr.path_of(cliques, slot_a):
        if c in pb:
            return c
    return None


def _tables(cliques, dims):
    poff, spos = mr.path_offsets(cliques, dims)
    nf = [sum(dims[s] for s in list(sl)[:nfv]) for sl, nfv, _, _ in cliques]
    depth = [len(mr.path_of(cliques, list(sl)[0])) - 1 for sl, _, _, _ in cliques]
    return poff, spos, nf, depth


def _position(cliques, dims, poff, slot):
    c = mr.clique_of(cliques, slot)
    o = 0
    for s in list(cliques[c][0])[:cliques[c][1]]:
        if s == slot:
            return c, poff[c] + o
        o += dims[s]
    raise KeyError(slot)


def _up(cliques, c, poff, spos, nf, W):
    A = np.asarray(cliques[c][3], dtype=LD)
    p0, n = poff[c], nf[c]
    Y = mr._solve_upper_transposed(A[:, :n], W[p0:p0 + n])
    W[p0:p0 + n] = Y
    for k, p in enumerate(spos[c]):
        W[p] = W[p] - A[:, n + k] @ Y


def _down(cliques, c, poff, spos, nf, W):
    A = np.asarray(cliques[c][3], dtype=LD)
    p0, n = poff[c], nf[c]
    rhs = W[p0:p0 + n].copy()
    for k, p in enumerate(spos[c]):
        rhs = rhs - np.outer(A[:, n + k], W[p])
    W[p0:p0 + n] = mr._solve_upper(A[:, :n], rhs)


def order_targets(cliques, dims, source, targets):
    """the targets deepest junction first (a target in another tree anywhere: it walks nothing); stable"""
    _, _, _, depth = _tables(cliques, dims)

    def key(t):
        J = junction(cliques, t, source)
        return -(depth[J] if J is not None else -1)

    return sorted(targets, key=key)


def cross_blocks(cliques, dims, source, targets):
    """[Sigma[t, source] for t in targets], dims[t] x dims[source], long double, in the order given, which must be deepest junction
    first (AssertionError otherwise).  The block of (source, source) is symmetrised as mr.path_marginal's."""
    poff, spos, nf, _ = _tables(cliques, dims)
    dj = dims[source]
    cj, pj = _position(cliques, dims, poff, source)
    Lw = poff[cj] + nf[cj]
    for t in targets:
        ct, _ = _position(cliques, dims, poff, t)
        Lw = max(Lw, poff[ct] + nf[ct])
    W = np.full((Lw, dj), np.nan, dtype=LD)  # (what the walk does not zero itself it must never read)
    W[:poff[cj] + nf[cj]] = 0
    W[pj:pj + dj] = np.eye(dj, dtype=LD)
    path = mr.path_of(cliques, source)
    for c in path:
        _up(cliques, c, poff, spos, nf, W)
    for c in reversed(path):
        _down(cliques, c, poff, spos, nf, W)
    intact = poff[cj] + nf[cj]  # x of the source's path is intact on the positions below this
    out = []
    for t in targets:
        ct, pt = _position(cliques, dims, poff, t)
        J = junction(cliques, t, source)
        if J is None:
            out.append(np.zeros((dims[t], dj), dtype=LD))
            continue
        shared = poff[J] + nf[J]
        assert shared <= intact, "targets out of order: an earlier branch descent overwrote x of the source's path below this junction"
        if ct != J:
            branch = []
            c = ct
            while c != J:
                branch.append(c)
                c = cliques[c][2]
            W[shared:poff[ct] + nf[ct]] = 0
            intact = min(intact, shared)
            for c in reversed(branch):
                _down(cliques, c, poff, spos, nf, W)
        blk = W[pt:pt + dims[t]].copy()
        out.append(0.5 * (blk + blk.T) if t == source else blk)
    return out


def cross_covariance(cliques, dims, i, j):
    """Sigma[i, j] with j the source"""
    return cross_blocks(cliques, dims, j, [i])[0]


def joint_marginal(cliques, dims, slots):
    """the joint marginal covariance of `slots`, blocks in the order given: every off-diagonal block computed once, from the variable
    with the shorter path (scalars; ties: the smaller slot) as the source, and mirrored"""
    poff, _, nf, _ = _tables(cliques, dims)

    def length(s):
        c = mr.clique_of(cliques, s)
        return poff[c] + nf[c]

    off = np.concatenate([[0], np.cumsum([dims[s] for s in slots])]).astype(int)
    M = np.zeros((off[-1], off[-1]), dtype=LD)
    for a, sa in enumerate(slots):
        M[off[a]:off[a + 1], off[a]:off[a + 1]] = cross_covariance(cliques, dims, sa, sa)
        for b in range(a + 1, len(slots)):
            sb = slots[b]
            first = (length(sa), sa) < (length(sb), sb)
            blk = cross_covariance(cliques, dims, sb, sa) if first else cross_covariance(cliques, dims, sa, sb).T  # Sigma[sb, sa]
            M[off[b]:off[b + 1], off[a]:off[a + 1]] = blk
            M[off[a]:off[a + 1], off[b]:off[b + 1]] = blk.T
    return M
