"""The cases, the reference and the restatement for the Dogleg's two products with the Bayes tree (csrc/kernels_bayes.hpp:
bt_lds_forward_kernel, bt_lds_transpose_kernel, bt_gather_kernel, bt_hbm_forward_kernel, bt_hbm_transpose_kernel; the slot table of
bt_build_gather in csrc/lmgpu.hip), read through lmgpu_bt_products.

No graph builder of its own: a case is a named case of lds_front_cases, dense_front_cases or schur_cases (CASES: name -> (module,
development switch or None)).  Two remarks on the set:
  * lds_front_cases has pivots[47] and pivots[48] at n - 1 = 63 and pivots[49] at n - 1 = 65, none at 64: `pair[48,16]` is
    lds_front_cases.tree_case on lds_front_cases.pair(48, 16) -- the builder of every pivots[..] case -- and has n - 1 = 64, the last
    width at which bt_lds_transpose_kernel's lanes make one pass.  children_wide is added for its separators of 63, 64, 65, 127 and 128
    scalars, either side of the second and third pass of the forward kernel's separator loop.
  * a gather leaf is by construction (finalize in csrc/lmgpu.hip) an LDS leaf whose parent is an HBM front, and every schur_cases root is
    an HBM front (n >= 142): there is no "gather leaf under an LDS root".  dims_2_3 is the smallest schur_cases case (174 scalars);
    leaf_degrees is taken beside it for its HBM front of nf = 3 under the HBM root.  Point-like leaves under an LDS root are tiny_sfm
    and children[k].

What each case is for is not a comment but an assertion: EDGES names every edge value of the five kernels and of the slot table, and
test_bt_products_reference.py::test_cases_cover_every_edge computes each from front_info of structure-only handles.

The reference needs no factorisation: from the whitened Jacobians [A b] in np.longdouble the gradient is -A^T b, and
    sum_c ||[R S] x - alpha d||^2 = ||A x - alpha b||^2 - alpha^2 (||b||^2 - ||d||^2)
(R^T R = A^T A, R^T d = A^T b), where ||d||^2 is read from dense_reference.DenseReference at lambda = 0.  ||d||^2 does not depend on
the elimination order, so the reference eliminates one variable per "front", in slot order.

Deviations: gradient = max|g - g_ref| / max|g_ref|; squared norm = |s - s_ref| / s_ref, and s = 0 exactly where s_ref = 0 (x = 0 with
alpha = 0: every term of every kernel is then an exact zero).  Tolerance: the project's recipe max(16 x floor, 64 n 2.2e-16) with n the
width of the case's widest front -- every entry of either product is a sum of rows of at most n terms each of [R S d], which the
elimination suites hold to 64 n eps relative to their largest entry; the floor is what the float64 oracle's own cliques, multiplied out
in float64 numpy, deviate from the reference of the oracle's Jacobians, over the passes the comparison makes (the second pass, after
one Newton step, has the smaller gradient and so the larger floor: g = -A^T b cancels towards the optimum).  16 x floor above 1e-9
fails the case.
"""
import functools

import numpy as np

import dense_front_cases as dc
import lds_front_cases as lc
import schur_cases as sc
from dense_front_cases import BLOCK, CAP, EPS, FACTOR
from dense_reference import LD
from gtsam_personal_amd.graph import POINT2, POSE2, Values

FUSE = ("LMGPU_FUSE_LEVELS", "1")
CASES = {}
for _n in ("staging[31]", "children[3]", "children[4]", "children[5]",  # LDS list length 1, 4, 5, 6
           "bin[24]", "bin[64,74]", "bin[65,73]", "bin[3,135]", "bin[135,3]", "backsub[128,8]", "backsub[129,6]", "pivots[48]", "pivots[49]",
           "children_wide", "deep_chain", "tiny_sfm"):
    CASES[_n] = (lc, None)
CASES["pair[48,16]"] = (None, None)
CASES["fused_level"] = (lc, FUSE)
for _n in ("dims_2_3", "leaf_degrees"):
    CASES[_n] = (sc, None)
for _n in ("medium_batch", "tail[257]", "tail[321]", "chain[576]", "separator[300,138]", "separator[96,600]"):
    CASES[_n] = (dc, None)
# the Dogleg runs also start from one_panel[65] (an HBM front of nf = 65 under an LDS root)
EXTRA = {"one_panel[65]": (dc, None)}

ALPHAS = (0.0, 1.0, -0.5)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "pair[48,16]":
        return lc.tree_case(790, lc.pair(48, 16))
    module, _ = CASES.get(name) or EXTRA[name]
    return module.case(name)


def switch_of(name):
    return (CASES.get(name) or EXTRA[name])[1]


def perturbed(c, scale, seed):
    """the case with every initial value moved by default_rng(seed).normal(0, scale) (a pose: scale * [1, 1, 0.5]), in the order of the
    Values' keys; Pose2 / Point2 graphs only"""
    rng = np.random.default_rng(seed)
    out = Values()
    for k in c["initial"].keys():
        t, v = c["initial"].type(k), np.asarray(c["initial"].at(k), dtype=float)
        assert t in (POSE2, POINT2), t
        out.insert(k, t, v + rng.normal(0, scale * np.array([1.0, 1.0, 0.5]) if t == POSE2 else scale, len(v)))
    return dict(c, initial=out)


# ---------------------------------------------------------------------------------------------------------------- coverage
# edge -> predicate over the summary of the set (see `summary`): every edge value the issue of these kernels lists
def _lds(s, f):
    return any(f(nf, ns) for nf, ns in s["lds"])


def _hbm(s, f):
    return any(f(nf, n) for nf, n in s["hbm"])


EDGES = {
    # bt_lds_forward_kernel / bt_lds_transpose_kernel: four fronts per workgroup
    "LDS list of one front": lambda s: 1 in s["lds_list"],
    "LDS list length 0 mod 4": lambda s: 4 in s["lds_list"],
    "LDS list length 1 mod 4, two workgroups": lambda s: 5 in s["lds_list"],
    "LDS list length 2 mod 4, two workgroups": lambda s: 6 in s["lds_list"],
    # the frontal loop j = i + lane
    "LDS nf = 64 (one pass)": lambda s: _lds(s, lambda nf, ns: nf == 64),
    "LDS nf = 65 (second pass)": lambda s: _lds(s, lambda nf, ns: nf == 65),
    "LDS nf = 128 / 129 (third pass)": lambda s: _lds(s, lambda nf, ns: nf == 128) and _lds(s, lambda nf, ns: nf == 129),
    # the separator loop
    "LDS ns = 0 (root)": lambda s: _lds(s, lambda nf, ns: ns == 0),
    "LDS ns = 64 / 65": lambda s: _lds(s, lambda nf, ns: ns == 64) and _lds(s, lambda nf, ns: ns == 65),
    "LDS ns = 128 / >= 129": lambda s: _lds(s, lambda nf, ns: ns == 128) and _lds(s, lambda nf, ns: ns >= 129),
    # lanes along n - 1 columns
    "LDS n - 1 = 64 / 65": lambda s: _lds(s, lambda nf, ns: nf + ns == 64) and _lds(s, lambda nf, ns: nf + ns == 65),
    "LDS n - 1 = 138 (three passes)": lambda s: _lds(s, lambda nf, ns: nf + ns == 138),
    "LDS nf < n - 1 and nf = n - 1": lambda s: _lds(s, lambda nf, ns: ns > 0 and nf > 64) and _lds(s, lambda nf, ns: ns == 0 and nf > 64),
    "LDS dimensions 6 / 3 / 5": lambda s: {6, 3, 5} <= s["lds_dims"],
    # bt_hbm_forward_kernel / bt_hbm_transpose_kernel
    "HBM n - 1 = 256 / 257": lambda s: _hbm(s, lambda nf, n: n - 1 == 256) and _hbm(s, lambda nf, n: n - 1 == 257),
    "HBM three column blocks": lambda s: _hbm(s, lambda nf, n: n - 1 > 512),
    "HBM nf % 64 = 63 / 0 / 1": lambda s: all(_hbm(s, lambda nf, n, r=r: nf % 64 == r) for r in (63, 0, 1)),
    "HBM one chunk / two / nine": lambda s: all(_hbm(s, lambda nf, n, k=k: (nf + 63) // 64 == k) for k in (1, 2, 9)),
    "HBM ns >> nf": lambda s: _hbm(s, lambda nf, n: n - 1 - nf > 4 * nf),
    "HBM nf = 3": lambda s: _hbm(s, lambda nf, n: nf == 3),
    # bt_build_gather / bt_gather_kernel
    "seven HBM fronts in one table": lambda s: 7 in s["hbm_count"],
    "HBM front under an HBM front": lambda s: s["hbm_under_hbm"],
    "LDS and HBM fronts in one table": lambda s: s["mixed"],
    "gather leaves under an HBM root": lambda s: s["gather_leaves"],
    "a variable in five separators": lambda s: s["max_separators"] >= 5,
    "ntot not a multiple of 256": lambda s: any(n > 256 and n % 256 for n in s["ntot"]),
    "ntot above 256 (two workgroups of the gather)": lambda s: any(n > 256 for n in s["ntot"]),
    "thirteen levels (merged elimination)": lambda s: s["levels"] >= 13,
}


def summary(infos_by_case):
    """infos_by_case: {name: (front_info dicts, front key lists, {key: dim})} -> what EDGES reads"""
    s = dict(lds=set(), hbm=set(), lds_list=set(), hbm_count=set(), lds_dims=set(), ntot=[], hbm_under_hbm=False, mixed=False,
             gather_leaves=False, max_separators=0, levels=0)
    for name, (infos, keys, dims) in infos_by_case.items():
        lds = [f for f in infos if f["cls"] == 0]
        hbm = [f for f in infos if f["cls"] == 1]
        s["lds"] |= {(f["nf"], f["n"] - f["nf"] - 1) for f in lds}
        s["hbm"] |= {(f["nf"], f["n"]) for f in hbm}
        s["lds_list"].add(len(lds))
        s["hbm_count"].add(len(hbm))
        s["ntot"].append(sum(dims.values()))
        s["hbm_under_hbm"] |= any(f["parent"] >= 0 and infos[f["parent"]]["cls"] == 1 for f in hbm)
        s["mixed"] |= bool(lds) and bool(hbm)
        children = {f["parent"] for f in infos}
        s["gather_leaves"] |= any(f["parent"] >= 0 and infos[f["parent"]]["cls"] == 1 and i not in children for i, f in enumerate(infos) if f["cls"] == 0)
        count = {}
        for f, ks in zip(infos, keys):
            for k in ks[f["n_frontal_keys"]:]:
                count[k] = count.get(k, 0) + 1
            if f["cls"] == 0:
                s["lds_dims"] |= {dims[k] for k in ks}
        s["max_separators"] = max([s["max_separators"]] + list(count.values()))
        s["levels"] = max(s["levels"], 1 + max(f["level"] for f in infos))
    return s


# ---------------------------------------------------------------------------------------------------------------- the reference
def slot_offsets(c):
    """({key: first scalar in the packed vectors}, {key: dim}, ntot): packed by slot = in the order of the ordering"""
    dims = sc.var_dims(c)
    off, n = {}, 0
    for k in c["ordering"]:
        off[int(k)] = n
        n += dims[k]
    return off, {int(k): d for k, d in dims.items()}, n


class ProductsReference:
    """-A^T b and ||A x - alpha b||^2 - alpha^2 (||b||^2 - ||d||^2) in np.longdouble from the whitened Jacobians [A b] of every factor"""

    def __init__(self, c, jacobians):
        self.off, self.dims, self.n = slot_offsets(c)
        fk = c["graph"].factor_keys_in_graph_order()
        self.factors = []
        for keys, Ab in zip(fk, jacobians):
            cols = np.concatenate([np.arange(self.off[int(k)], self.off[int(k)] + self.dims[int(k)]) for k in keys])
            Ab = np.asarray(Ab, dtype=np.float64).astype(LD)
            assert Ab.shape[1] == cols.size + 1
            self.factors.append((cols, Ab[:, :-1], Ab[:, -1]))
        self.bb = sum((b @ b for _, _, b in self.factors), LD(0))
        ref = sc.reference(c, jacobians, [([k], 1) for k in c["ordering"]], 0.0, False, block=BLOCK)
        assert ref.residual < 1e-17, ref.residual
        d = ref.R[:, ref.n]
        self.dd = d @ d
        self._newton = ref._x  # (the reference's variable order is the slot order)

    def newton(self):
        """the solution of the undamped system, packed by slot"""
        return self._newton.copy()

    def gradient(self):
        g = np.zeros(self.n, dtype=LD)
        for cols, A, b in self.factors:
            np.subtract.at(g, cols, A.T @ b)
        return g

    def sq_norm(self, x, alpha):
        x, alpha = np.asarray(x).astype(LD), LD(alpha)
        tot = LD(0)
        for cols, A, b in self.factors:
            e = A @ x[cols] - alpha * b
            tot += e @ e
        return tot - alpha * alpha * (self.bb - self.dd)


def gradient_deviation(g, ref_g):
    return float(np.abs(np.asarray(g, dtype=LD) - ref_g).max() / np.abs(ref_g).max())


def norm_deviation(s, ref_s):
    """relative; where the reference is an exact zero the product has to be one too (deviation 0, else infinite)"""
    if ref_s == 0:
        return 0.0 if s == 0 else float("inf")
    return float(abs(LD(s) - ref_s) / abs(ref_s))


def probes(ntot, seed=0):
    """the vectors every comparison uses: one standard-normal x and x = 0, each with every alpha"""
    x = np.random.default_rng(1000 + seed).standard_normal(ntot)
    return [(xv, a) for xv in (x, np.zeros(ntot)) for a in ALPHAS]


def tolerance(floor, widest):
    return max(FACTOR * floor, 64 * widest * EPS)


# ---------------------------------------------------------------------------------------------------------------- cliques, multiplied out
def clique_products(cliques, off, dims, ntot, x, alpha):
    """float64 numpy: (sum_c ||[R S] x - alpha d||^2, - sum_c [R S]^T d) of cliques [(keys, n frontal keys, [R S d], ...)]"""
    g, tot = np.zeros(ntot), 0.0
    for keys, _, rsd, *_ in cliques:
        cols = np.concatenate([np.arange(off[k], off[k] + dims[k]) for k in keys])
        RS, d = rsd[:, :-1], rsd[:, -1]
        g[cols] -= RS.T @ d
        e = RS @ x[cols] - alpha * d
        tot += float(e @ e)
    return tot, g


def oracle_pass(c, newton_steps):
    """the oracle linearized (and solved at lambda = 0) after `newton_steps` full Newton steps: (oracle, Jacobians, cliques)"""
    import oracle_harness as oh
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    for _ in range(newton_steps):
        orc.linearize()
        rc, delta, _, _ = orc.solve(0.0, False)
        assert rc == 0
        orc.retract(delta)
    orc.linearize()
    rc, _, _, _ = orc.solve(0.0, False)
    assert rc == 0
    return orc, [orc.jacobian(g) for g in range(c["graph"].size())], orc.cliques()


@functools.lru_cache(maxsize=None)
def oracle_floor(name, passes=2):
    """dict(gradient, norm): what the oracle's cliques, multiplied out in float64, deviate from the reference of the oracle's own
    Jacobians, worst over the probes and over `passes` linearizations (the start, then after each Newton step)"""
    c = case(name)
    off, dims, ntot = slot_offsets(c)
    out = dict(gradient=0.0, norm=0.0, detail=[])
    for p in range(passes):
        _, jac, cliques = oracle_pass(c, p)
        ref = ProductsReference(c, jac)
        g_ref = ref.gradient()
        fg = fn = 0.0
        for x, alpha in probes(ntot, p):
            s, g = clique_products(cliques, off, dims, ntot, x, alpha)
            fg, fn = max(fg, gradient_deviation(g, g_ref)), max(fn, norm_deviation(s, ref.sq_norm(x, alpha)))
        out["detail"].append((fg, fn))
        out["gradient"], out["norm"] = max(out["gradient"], fg), max(out["norm"], fn)
    return out


# ---------------------------------------------------------------------------------------------------------------- the five loops, restated
DEFECTS = ("forward skips column i + 64 of one row", "forward drops separator columns >= 64", "forward subtracts d with alpha = 0",
           "HBM transpose loses chunk 1 for columns 64 .. 127", "HBM transpose's last column block is not written",
           "gather list misses one separator slot of one clique", "gather uses the slot table of the previous front order")


def restated_fronts(infos, cliques):
    """[dict(keys, nfk, nf, n, cls, rsd)] in the order of the slot table: the LDS-class fronts, then the HBM fronts, level by level"""
    fronts = [dict(keys=[int(k) for k in keys], nfk=nfk, nf=f["nf"], n=f["n"], cls=f["cls"], level=f["level"], rsd=np.asarray(rsd, dtype=np.float64))
              for f, (keys, nfk, rsd, *_) in zip(infos, cliques)]
    assert all(f["rsd"].shape == (f["nf"], f["n"]) for f in fronts)
    return sorted((f for f in fronts if f["cls"] == 0), key=lambda f: f["level"]) + sorted((f for f in fronts if f["cls"] == 1), key=lambda f: f["level"])


def _columns(f, off, dims):
    return np.concatenate([np.arange(off[k], off[k] + dims[k]) for k in f["keys"]])


def _slot_table(fronts, off, dims, ntot, defect):
    """bt_build_gather: (first slot of every front, per scalar the list of slots), LDS fronts n - 1 slots, HBM fronts (n - 1) per chunk of
    64 rows of which chunk c lists the columns j >= 64 c"""
    first, slots, o = [], [[] for _ in range(ntot)], 0
    dropped = False
    for f in fronts:
        first.append(o)
        cols, w = _columns(f, off, dims), f["n"] - 1
        for c in range(1 if f["cls"] == 0 else (f["nf"] + 63) // 64):
            for j in range(64 * c, w):
                if defect == DEFECTS[5] and not dropped and j == w - 1 and w > f["nf"]:
                    dropped = True
                    continue
                slots[cols[j]].append(o + c * w + j)
        o += w * (1 if f["cls"] == 0 else (f["nf"] + 63) // 64)
    return first, slots, o


def restated_products(fronts, off, dims, ntot, x, alpha, defect=None):
    """the five loops in float64 numpy, one defect of DEFECTS planted or none: (squared norm, gradient)"""
    tot, skipped = 0.0, False
    for f in fronts:  # bt_lds_forward_kernel / bt_hbm_forward_kernel: row i, frontal columns j >= i, then the separator
        cols, nf, n, rsd = _columns(f, off, dims), f["nf"], f["n"], f["rsd"]
        xs = x[cols]
        for i in range(nf):
            row = rsd[i]
            terms = row[i:nf] * xs[i:nf]
            if defect == DEFECTS[0] and not skipped and i + 64 < nf and terms[64] != 0:  # (the first such row whose entry is no structural zero)
                terms[64] = 0.0
                skipped = True
            sep = row[nf:n - 1] * xs[nf:]
            if defect == DEFECTS[1]:
                sep = sep[:64]
            e = terms.sum() + sep.sum() - (1.0 if defect == DEFECTS[2] and alpha == 0 else alpha) * row[n - 1]
            tot += e * e
    first, slots, total = _slot_table(fronts, off, dims, ntot, defect)
    if defect == DEFECTS[6]:  # the data lands where the present order puts it; the table still lists the order before (two fronts swapped)
        slots = _slot_table([fronts[1], fronts[0]] + fronts[2:], off, dims, ntot, None)[1]
    part = np.zeros(total + max(f["n"] for f in fronts) * 16)
    for f, o in zip(fronts, first):  # bt_lds_transpose_kernel / bt_hbm_transpose_kernel
        nf, w, rsd = f["nf"], f["n"] - 1, f["rsd"]
        d = rsd[:, -1]
        if f["cls"] == 0:
            part[o:o + w] = -(rsd[:, :w].T @ d)
            continue
        for c in range((nf + 63) // 64):
            v = -(rsd[64 * c:64 * c + 64, :w].T @ d[64 * c:64 * c + 64])
            if defect == DEFECTS[3] and c == 1:
                v[64:128] = 0.0
            if defect == DEFECTS[4]:
                v[256 * ((w - 1) // 256):] = 0.0
            part[o + c * w:o + (c + 1) * w] = v
    g = np.array([sum(part[s] for s in sl) for sl in slots])  # bt_gather_kernel
    return tot, g


# ---------------------------------------------------------------------------------------------------------------- one Dogleg iteration, restated
STEEPEST, BLEND, NEWTON = 0, 1, 2  # csrc/dogleg_step.hpp
BRANCH_NAME = ("steepest", "blend", "newton")
RHO_NAME = ("grow", "keep", "halve", "retry")  # rho >= 0.75, >= 0.25, >= 0, < 0
RHO_THRESHOLDS = (0.75, 0.25, 0.0)
MARGIN_RATIO, MARGIN_RHO, MARGIN_F = 4.0, 0.05, 1e-6


def trial_point_ld(delta, uu, nn, un):
    """dogleg_trial_point in np.longdouble (delta^2 as the library squares it: in float64)"""
    dsq = LD(np.float64(delta) * np.float64(delta))
    if dsq < uu:
        return STEEPEST, np.sqrt(dsq / uu)
    if dsq < nn:
        a, b, c = uu - 2 * un + nn, 2 * (un - uu), uu - dsq
        sq = np.sqrt(b * b - 4 * a * c)
        tau1, tau2 = (-b + sq) / (2 * a), (-b - sq) / (2 * a)
        return BLEND, (tau1 if -EPS <= tau1 <= 1 + EPS else tau2)
    return NEWTON, LD(1)


def radius_update_ld(rho, delta, norm):
    """dogleg_radius_update: (new delta, stay, moved, index into RHO_NAME)"""
    if rho >= 0.75:
        return max(delta, float(3 * norm)), False, True, 0
    if rho >= 0.25:
        return delta, False, True, 1
    if rho >= 0.0:
        return (delta * 0.5 if delta > 1e-5 else delta), False, True, 2
    if delta > 1e-5:
        return delta * 0.5, True, True, 3
    return delta, False, False, 3


def values_of(c, by_key):
    out = Values()
    for k in c["initial"].keys():
        out.insert(k, c["initial"].type(k), by_key[k])
    return out


def by_key_of(c, packed):
    off, dims, _ = slot_offsets(c)
    return {k: np.asarray(packed[off[k]:off[k] + dims[k]], dtype=np.float64) for k in off}


def packed_of(c, by_key):
    off, dims, n = slot_offsets(c)
    out = np.zeros(n)
    for k in off:
        out[off[k]:off[k] + dims[k]] = by_key[k]
    return out


def restated_iteration(c, values, f_error, delta):
    """one DoglegOptimizer::iterate from `values` (a Values) with radius delta, the linear algebra in np.longdouble: gradient, Newton step
    and both quadratic models from the reference of the oracle's Jacobians at `values`; retract and nonlinear error are the oracle's.
    Returns dict(delta, error, step (packed float64), values, trials = [dict(branch, scalar, rho, rho_branch, new_f, delta)], ratio =
    |x_N| / |x_u|, moved)"""
    import oracle_harness as oh
    cv = dict(c, initial=values)
    orc = oh.OracleProblem(c["graph"], values, c["ordering"])
    orc.linearize()
    ref = ProductsReference(cv, [orc.jacobian(g) for g in range(c["graph"].size())])
    x_n = ref.newton()
    g = ref.gradient()
    x_u = (-(g @ g) / ref.sq_norm(g, 0)) * g
    m0 = ref.sq_norm(np.zeros(ref.n, dtype=LD), 1) / 2
    uu, nn, un = x_u @ x_u, x_n @ x_n, x_u @ x_n
    trials, stay, moved, new_f, step, new_values = [], True, True, f_error, None, values
    while stay:
        branch, scalar = trial_point_ld(delta, uu, nn, un)
        x_d = scalar * x_u if branch == STEEPEST else (1 - scalar) * x_u + scalar * x_n if branch == BLEND else x_n
        step = x_d.astype(np.float64)
        trial = oh.OracleProblem(c["graph"], values, c["ordering"])
        trial.retract(by_key_of(c, step))
        new_f = trial.error()
        new_m = ref.sq_norm(x_d, 1) / 2
        rho = 0.5 if abs(f_error - new_f) < 1e-15 or abs(m0 - new_m) < 1e-15 else float((LD(f_error) - LD(new_f)) / (m0 - new_m))
        radius = delta
        delta, stay, moved, rho_branch = radius_update_ld(rho, delta, np.sqrt(x_d @ x_d))
        trials.append(dict(branch=branch, scalar=float(scalar), rho=rho, rho_branch=rho_branch, new_f=new_f, radius=radius, delta=delta))
        new_values = values_of(c, trial.values())
    if not moved:
        new_f, step, new_values = f_error, np.zeros(ref.n), values
    return dict(delta=delta, error=new_f, step=step, values=new_values, trials=trials, moved=moved, f_error=f_error,
                ratio=float(np.sqrt(nn / uu)), norms=(float(np.sqrt(uu)), float(np.sqrt(nn))))


def margins_hold(it):
    """the margins under which a float64 implementation takes the branches of the restatement: see test_bt_products_reference"""
    rho_ok = all(abs(t["rho"] - th) >= MARGIN_RHO for t in it["trials"] for th in RHO_THRESHOLDS)
    f_ok = all(abs(it["f_error"] - t["new_f"]) >= MARGIN_F * it["f_error"] for t in it["trials"])
    return it["ratio"] >= MARGIN_RATIO and rho_ok and f_ok


def start_norms(c):
    """(|x_u|, |x_N|) at the case's initial values, from the reference"""
    import oracle_harness as oh
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    it = restated_iteration(c, c["initial"], orc.error(), 1.0)
    return it["norms"]


# the Dogleg runs: (case, start, radius rule).  start None = the case's own initial values, else (scale, seed) of `perturbed`; radius
# "cut" / "blend" / "newton" = |x_u| / 4, sqrt(|x_u| |x_N|), 4 |x_N| of the start (start_norms), or a number = deltaInitial.  EXPECTED
# gives, per iteration, one word per trial point: the branch of the blend (S steepest-descent cut, B blend, N Newton step) and of the gain
# ratio (g rho >= 0.75: grow, k >= 0.25: keep, h >= 0: halve, r < 0: halve and try again).  A run has as many iterations as EXPECTED lists:
# the next one would fail a margin (MARGIN_*; rho is rounding noise once f no longer moves).
RUNS = {
    "children[5]-cut": ("children[5]", None, "cut", ("Sg", "Sg", "Bg", "Bg")),
    "children[5]-blend": ("children[5]", None, "blend", ("Bg", "Ng", "Ng")),
    "children[5]-newton": ("children[5]", None, "newton", ("Ng", "Ng", "Ng")),
    "bin[65,73]-cut": ("bin[65,73]", None, "cut", ("Sg", "Sg", "Bg", "Ng")),
    "bin[65,73]-blend": ("bin[65,73]", None, "blend", ("Bg", "Ng", "Ng")),
    "bin[65,73]-newton": ("bin[65,73]", None, "newton", ("Ng", "Ng")),
    "deep_chain-cut": ("deep_chain", None, "cut", ("Sg", "Sg", "Bg", "Ng")),
    "deep_chain-blend": ("deep_chain", None, "blend", ("Bg", "Ng", "Ng")),
    "deep_chain-newton": ("deep_chain", None, "newton", ("Ng", "Ng")),
    "one_panel[65]-cut": ("one_panel[65]", None, "cut", ("Sg", "Sg", "Bg", "Bg")),
    "one_panel[65]-blend": ("one_panel[65]", None, "blend", ("Bg", "Ng", "Ng")),
    "one_panel[65]-newton": ("one_panel[65]", None, "newton", ("Ng", "Ng", "Ng")),
    # far starts: the radius goes x 1/32 within the first iteration
    "bin[65,73]~1000": ("bin[65,73]", (3.0, 1), 1000.0, ("Nr Nr Nr Nr Nr Bk",)),
    "bin[65,73]~8": ("bin[65,73]", (3.0, 1), 8.0, ("Bg", "Bh")),
    "one_panel[65]~1000": ("one_panel[65]", (3.0, 1), 1000.0, ("Nr Nr Nr Nr Nr Bk", "Bk", "Bk", "Bk")),
}
MAX_ITERATIONS = 4


def words(it):
    return " ".join("SBN"[t["branch"]] + "gkhr"[t["rho_branch"]] for t in it["trials"])


@functools.lru_cache(maxsize=None)
def run_start(name):
    """(case with the run's start values, deltaInitial)"""
    cname, start, radius, _ = RUNS[name]
    c = case(cname) if start is None else perturbed(case(cname), *start)
    if isinstance(radius, str):
        xu, xn = start_norms(c)
        radius = dict(cut=xu / 4, blend=float(np.sqrt(xu * xn)), newton=4 * xn)[radius]
    return c, float(radius)


@functools.lru_cache(maxsize=None)
def restated_run(name):
    """([(restated iteration, what the float64 oracle's dl_iterate deviates from it: dict(delta, error, step: relative; trials: the
    oracle's count))], the iteration after the last one or None): the run stops where EXPECTED stops"""
    import oracle_harness as oh
    c, radius = run_start(name)
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    orc.dl_init(radius)
    values, f, delta, out, inner = c["initial"], orc.error(), radius, [], 0
    for _ in range(len(RUNS[name][3])):
        it = restated_iteration(c, values, f, delta)
        assert orc.dl_iterate() == 0
        so = orc.lm_state()
        out.append((it, dict(delta=abs(so["lambda_"] - it["delta"]) / it["delta"], error=abs(so["error"] - it["error"]) / it["error"],
                             step=step_deviation(orc.get_delta(), it["step"]), trials=so["inner"] - inner)))
        inner = so["inner"]
        values, f, delta = it["values"], it["error"], it["delta"]
    return out, (restated_iteration(c, values, f, delta) if len(out) < MAX_ITERATIONS else None)


def step_deviation(got, want):
    return float(np.linalg.norm(np.asarray(got) - want) / np.linalg.norm(want))
