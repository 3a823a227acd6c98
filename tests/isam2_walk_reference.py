"""What the ISAM2 tree-walk kernels of csrc/isam2.hpp must produce, restated in np.longdouble on a GIVEN Bayes tree: the list
ISAM2.cliques() / OracleISAM2.cliques() returns, [(keys, frontal keys, [R S d] (nf, n), parent index)].  Elimination is not part of it:
the tree is taken bit for bit as its owner holds it, so a deviation found against these functions lies in a walk kernel.

  full_solve          x_F = R^-1 (d - S x_S), parents first                      isam2_wildfire_kernel with threshold <= 0
  wildfire            optimizeWildfireNonRecursive as the kernel's header states it (dirty / keep / descend)
  marginal_covariance the key block of (R^T R)^-1 from the assembled global R      isam2_marginal_kernel
  dogleg_point        gradient, R g, steepest-descent and Newton points, ComputeDoglegPoint / ComputeBlend with the tau selection of
                      is_update_delta_dogleg, and the tree's error at 0 and at the dogleg point
                      isam2_tree_gradient / gradient_gather / tree_rg / dot / gradient_search / blend / tree_error kernels

Every triangular solve is written row by row (numpy.linalg does not take longdouble).  Each function takes `dtype`: np.longdouble is the
reference, np.float64 the same arithmetic in working precision -- the FLOOR a tolerance is built on (`tolerance`).  Vectors are
{key: array}, as getDelta() returns them."""
import numpy as np

LD = np.longdouble
EPS, FACTOR, CAP = 2.2e-16, 16, 1e-9  # the recipe of bt_products_cases / test_gpu_dense_front_edges


class Tree:
    """cliques: [(keys, frontal key count, RSd, parent)]; dims: {key: scalars}.  Scalars are numbered by ascending key (getDelta's order)."""

    def __init__(self, cliques, dims):
        self.dims = {int(k): int(d) for k, d in dims.items()}
        self.keys = sorted(self.dims)
        self.off, o = {}, 0
        for k in self.keys:
            self.off[k] = o
            o += self.dims[k]
        self.n = o
        self.cliques = []
        for keys, nfk, rsd, parent in cliques:
            fk, sk = list(keys[:nfk]), list(keys[nfk:])
            fx = np.concatenate([np.arange(self.off[k], self.off[k] + self.dims[k]) for k in fk]).astype(int)
            sx = np.concatenate([np.arange(self.off[k], self.off[k] + self.dims[k]) for k in sk] + [np.zeros(0, dtype=int)]).astype(int)
            nf, ns = len(fx), len(sx)
            rsd = np.array(rsd, dtype=np.float64)
            assert rsd.shape == (nf, nf + ns + 1), (rsd.shape, nf, ns)
            rsd[:, :nf] = np.triu(rsd[:, :nf])  # what lies below the diagonal of a clique's rows is not part of R
            self.cliques.append(dict(fk=fk, sk=sk, fx=fx, sx=sx, nf=nf, ns=ns, rsd=rsd, parent=int(parent)))
        # parents first
        self.order = []
        kids = {}
        for i, c in enumerate(self.cliques):
            kids.setdefault(c["parent"], []).append(i)
        stack = list(reversed(kids.get(-1, [])))
        while stack:
            i = stack.pop()
            self.order.append(i)
            stack.extend(reversed(kids.get(i, [])))
        assert len(self.order) == len(self.cliques)
        self.children = kids

    def shape(self):
        """[(frontal keys, separator keys, parent's first frontal key or None)], sorted: comparable between two owners of one tree"""
        return sorted((tuple(c["fk"]), tuple(sorted(c["sk"])), None if c["parent"] < 0 else self.cliques[c["parent"]]["fk"][0]) for c in self.cliques)

    def widest(self):
        return max(c["nf"] + c["ns"] for c in self.cliques)

    def vec(self, by_key, dtype=LD):
        x = np.zeros(self.n, dtype=dtype)
        for k, v in by_key.items():
            if int(k) in self.off:
                x[self.off[int(k)]:self.off[int(k)] + self.dims[int(k)]] = v
        return x


def _solve_clique(c, x, dtype):
    """x_F = R^-1 (d - S x_S), row by row from the last"""
    A = c["rsd"].astype(dtype)
    nf = c["nf"]
    xs = x[c["sx"]]
    xf = np.zeros(nf, dtype=dtype)
    for i in range(nf - 1, -1, -1):
        s = A[i, -1] - (A[i, nf:-1] @ xs if c["ns"] else dtype(0)) - (A[i, i + 1:nf] @ xf[i + 1:] if i + 1 < nf else dtype(0))
        xf[i] = s / A[i, i]
    return xf


def full_solve(tree, dtype=LD):
    x = np.zeros(tree.n, dtype=dtype)
    for i in tree.order:
        c = tree.cliques[i]
        x[c["fx"]] = _solve_clique(c, x, dtype)
    return x


def wildfire(tree, delta_before, replaced_keys, threshold, dtype=LD):
    """-> (delta, info): info[i] = dict(visited, dirty, kept, change) of clique i.  delta_before: {key: vector} (a key it lacks is new: 0).
    dirty = replaced (its first frontal key) or a separator key was written in this walk; kept = replaced or change >= threshold or
    threshold <= 0, change = max |x_old - x_new| over the frontal scalars; the children of a clique that is not dirty are not visited."""
    replaced_keys = set(int(k) for k in replaced_keys)
    x = tree.vec(delta_before, dtype)
    changed = set()
    info = [dict(visited=False, dirty=False, kept=False, change=None) for _ in tree.cliques]
    for i in tree.order:
        c = tree.cliques[i]
        if c["parent"] >= 0 and not info[c["parent"]]["dirty"]:
            continue
        replaced = c["fk"][0] in replaced_keys
        dirty = threshold <= 0 or replaced or any(k in changed for k in c["sk"])
        info[i].update(visited=True, dirty=dirty)
        if not dirty:
            continue
        xf = _solve_clique(c, x, dtype)
        change = float(np.max(np.abs(x[c["fx"]] - xf)))
        kept = threshold <= 0 or replaced or change >= threshold
        info[i].update(kept=kept, change=change, replaced=replaced)
        if kept:
            x[c["fx"]] = xf
            changed.update(c["fk"])
    return x, info


def global_R(tree, dtype=LD):
    """(R, position of scalar): the cliques' rows stacked children first, so that R is upper triangular"""
    pos = np.zeros(tree.n, dtype=int)
    p = 0
    for i in reversed(tree.order):
        c = tree.cliques[i]
        pos[c["fx"]] = np.arange(p, p + c["nf"])
        p += c["nf"]
    assert p == tree.n
    R = np.zeros((tree.n, tree.n), dtype=dtype)
    for c in tree.cliques:
        rows = pos[c["fx"]]
        cols = pos[np.concatenate([c["fx"], c["sx"]])]
        R[np.ix_(rows, cols)] = c["rsd"][:, :-1].astype(dtype)
    assert not np.any(np.tril(R, -1))
    return R, pos


def marginal_covariance(tree, key, dtype=LD, R_pos=None):
    """the `key` block of (R^T R)^-1: per column R^T y = e, R x = y"""
    R, pos = R_pos if R_pos is not None else global_R(tree, dtype)
    N, d, o = tree.n, tree.dims[int(key)], tree.off[int(key)]
    out = np.zeros((d, d), dtype=dtype)
    for cidx in range(d):
        y = np.zeros(N, dtype=dtype)
        y[pos[o + cidx]] = 1
        start = int(pos[o + cidx])
        for i in range(start, N):  # (y is zero in front of the unit entry)
            y[i] = (y[i] - R[start:i, i] @ y[start:i]) / R[i, i]
        x = np.zeros(N, dtype=dtype)
        for i in range(N - 1, -1, -1):
            x[i] = (y[i] - R[i, i + 1:] @ x[i + 1:]) / R[i, i]
        out[:, cidx] = x[pos[o:o + d]]
    return out


def tree_error2(tree, x, dtype=LD):
    """sum over the cliques of ||[R S] x - d||^2 (twice the tree's error)"""
    tot = dtype(0)
    for c in tree.cliques:
        A = c["rsd"].astype(dtype)
        e = A[:, :-1] @ x[np.concatenate([c["fx"], c["sx"]])] - A[:, -1]
        tot += e @ e
    return tot


def dogleg_point(tree, radius, dtype=LD):
    """-> dict(g, rg, dx_u, dx_n, dx_d, branch (0 steepest descent, 1 blend, 2 Newton), a, b, nu = ||dx_u||, nn = ||dx_n||, nd = ||dx_d||,
    M0, M1 = the tree's error (half the sum of squares) at 0 and at dx_d)"""
    g = np.zeros(tree.n, dtype=dtype)
    for c in tree.cliques:
        A = c["rsd"].astype(dtype)
        np.add.at(g, np.concatenate([c["fx"], c["sx"]]), -(A[:, :-1].T @ A[:, -1]))
    rg = np.zeros(tree.n, dtype=dtype)
    for c in tree.cliques:
        A = c["rsd"].astype(dtype)
        rg[c["fx"]] = A[:, :-1] @ g[np.concatenate([c["fx"], c["sx"]])]
    dx_u = -((g @ g) / (rg @ rg)) * g
    dx_n = full_solve(tree, dtype)
    uu, nn, un = dx_u @ dx_u, dx_n @ dx_n, dx_u @ dx_n
    dsq = dtype(radius) * dtype(radius)
    a, b, branch = dtype(0), dtype(1), 2
    if dsq < uu:
        a, b, branch = np.sqrt(dsq / uu), dtype(0), 0
    elif dsq < nn:
        qa, qb, qc = uu - 2 * un + nn, 2 * (un - uu), uu - dsq
        sq = np.sqrt(qb * qb - 4 * qa * qc)
        tau1, tau2 = (-qb + sq) / (2 * qa), (-qb - sq) / (2 * qa)
        tau = tau1 if (-EPS <= tau1 <= 1.0 + EPS) else tau2
        a, b, branch = 1 - tau, tau, 1
    dx_d = a * dx_u + b * dx_n
    return dict(g=g, rg=rg, dx_u=dx_u, dx_n=dx_n, dx_d=dx_d, branch=branch, a=a, b=b, nu=float(np.sqrt(uu)), nn=float(np.sqrt(nn)),
                nd=float(np.sqrt(dx_d @ dx_d)), M0=0.5 * tree_error2(tree, np.zeros(tree.n, dtype=dtype), dtype), M1=0.5 * tree_error2(tree, dx_d, dtype))


def radius_after(radius, rho, nd):
    """DoglegOptimizerImpl::Iterate, ONE_STEP_PER_ITERATION, for 0 <= rho: the radius the step leaves"""
    assert rho >= 0
    if rho >= 0.75:
        return max(radius, 3.0 * nd)
    return radius if rho >= 0.25 else 0.5 * radius


def deviation(x, ref):
    """max |x - ref| relative to the largest entry of ref"""
    ref = np.asarray(ref, dtype=LD)
    scale = float(np.max(np.abs(ref))) if ref.size else 1.0
    return float(np.max(np.abs(np.asarray(x, dtype=LD) - ref))) / (scale if scale > 0 else 1.0) if ref.size else 0.0


def tolerance(floor, widest):
    """max(16 x floor, 64 n eps), relative to the largest entry of the compared vector or block; n = the widest clique of the case"""
    return max(FACTOR * floor, 64 * widest * EPS)
