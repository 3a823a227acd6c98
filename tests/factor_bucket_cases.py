"""TEST INFRASTRUCTURE: the numpy-only half of the factor-bucket tests (csrc/kernels_factors.hpp: whiten_block, robust_reweight,
gnc_reweight, the SFM tile store, linear_error_kernel, hessian_diag_kernel, reduce_stage1 / 2, retract_kernel).

It reads tests/golden/factor_bucket_edges.npz -- 37 benign cases per factor type (values, measurement, the 50-digit UNWHITENED
[H1 H2 (H3) | b] rounded to FP64) and 37 retract cases per variable type, written by tests/tools/make_factor_bucket_edges.py -- and
builds from them
  * a seeded noise model per factor (noise_for): every factor of a bucket has a noise row of its own,
  * the reference chain in np.longdouble: whitening, Robust, the GNC sqrt(w), per-factor error, Hessian diagonal, the two linear
    errors for a given delta (reference_blocks, hessian_diagonal, linear_errors; sums by math.fsum).  The chain is written over a small
    "number backend" so that tests/test_factor_bucket_reference.py can run the SAME code on mpmath numbers at 50 digits,
  * the case table (CASES / build): graphs, values and orderings,
  * the restatement of which path every wave of linear_error_kernel takes (linear_error_waves).

37 is prime: a bucket that tiles the cases (factor f uses case f mod 37) never repeats at a stride of 64, 128 or 256, so a lane, wave
or block slip lands on a different expected row.  The cases are chained so that variables can be shared: Pose2 case i joins pose
P2[i] to P2[(i + 1) mod 37] (the same for Pose3 and the 9-vectors), the priors of case i sit on P2[i] / P3[i] / V9[i] / point PT[i],
the bearing-range case i looks from P2[i], every GeneralSFMFactor2 case looks from P3[0] through the one calibration K0.

The weight and loss tables are restated from gtsam/linear/LossFunctions.cpp, not imported from the package."""
from __future__ import annotations

import math
import os

import numpy as np

from gtsam_personal_amd.graph import (CAL3_S2, CAM_BUNDLER, F_BEARING_RANGE_2D, F_BETWEEN_POSE2, F_BETWEEN_POSE3, F_CHORDAL_BETWEEN,
                                      F_PRIOR_CAL3_S2, F_PRIOR_CAM, F_PRIOR_POINT3, F_PRIOR_POSE2, F_PRIOR_POSE3, F_PRIOR_VEC9, F_SFM,
                                      F_SFM2, FACTOR_MEAS, FACTOR_ROWS, FACTOR_VARS, N_DIAG, N_GAUSS, N_UNIT, POINT2, POINT3, POSE2, POSE3,
                                      VAR_DIM, VAR_STORE, VEC9, NonlinearFactorGraph, Ordering, Values, _MEstimator, noiseModel)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_bucket_edges.npz")
NCASE = 37
FACTOR_TYPES = tuple(range(14))
VAR_TYPES = tuple(range(7))
KIND_NAME = {N_UNIT: "unit", N_DIAG: "diag", N_GAUSS: "gauss"}
LAMBDA = 1e-3           # the damping of every solve
MIN_REDUCTION = 0.1     # (e0 - e1) / e0 of every linear_error case at the delta used
WHITEN_SIZES = (1, 127, 128, 129)     # the 128-lane generic / three-variable kernels: one lane, block - 1, block, block + 1
SFM_SIZES = (255, 256, 257, 513)      # the 256-lane SFM kernels and their 256 x 26 tile
REDUCE_SIZES = (1, 255, 256, 257, 65536, 65537)
RETRACT_SIZES = (255, 256, 257)
HDIAG_NTOT = (255, 256, 257)
ROBUST_TYPES = (F_SFM, F_BETWEEN_POSE3, F_PRIOR_CAM)
ROBUST_N = 129
CHAIN_BETWEEN = {POSE2: F_BETWEEN_POSE2, POSE3: F_BETWEEN_POSE3, VEC9: F_CHORDAL_BETWEEN}
CHAIN_PRIOR = {POSE2: F_PRIOR_POSE2, POSE3: F_PRIOR_POSE3, VEC9: F_PRIOR_VEC9}


def load():
    return dict(np.load(FIXTURE, allow_pickle=False))


def factor_dims(ft):
    return tuple(VAR_DIM[t] for t in FACTOR_VARS[ft])


def factor_cols(ft):
    return sum(factor_dims(ft))


def factor_size(ft):
    """doubles of the factor's [A b]"""
    return FACTOR_ROWS[ft] * (factor_cols(ft) + 1)


def split_vals(ft, flat):
    out, o = [], 0
    for t in FACTOR_VARS[ft]:
        out.append(flat[o:o + VAR_STORE[t]])
        o += VAR_STORE[t]
    return out


# ---------------------------------------------------------------- number backends
class LongDouble:
    """np.longdouble (64-bit significand on x86): 2^-11 of an FP64 ulp per operation"""
    name = "longdouble"
    sqrt, exp, expm1, log1p = staticmethod(np.sqrt), staticmethod(np.exp), staticmethod(np.expm1), staticmethod(np.log1p)

    @staticmethod
    def array(a):
        return np.asarray(a, dtype=np.longdouble)

    @staticmethod
    def scalar(x):
        return np.longdouble(x)


LD = LongDouble


# ---------------------------------------------------------------- noise
def noise_for(ftype, f, kind, robust=None):
    """the seeded noise model of factor number f of a bucket: Unit, Diagonal with sigmas spread over [0.05, 20] (log-uniform), or
    Gaussian given as a full upper-triangular SqrtInformation whose off-diagonals are of the size of their row's diagonal entry.
    smart=False: none collapses to a simpler kind.  robust = (m-estimator id, k) wraps it in noiseModel.Robust"""
    m = FACTOR_ROWS[ftype]
    if kind == N_UNIT:
        model = noiseModel.Unit.Create(m)
    else:
        rng = np.random.default_rng([int(ftype), int(f), int(kind), 20261018])
        d = 0.05 * 400.0 ** rng.random(m)
        if kind == N_DIAG:
            model = noiseModel.Diagonal.Sigmas(d, smart=False)
        else:
            R = np.diag(d)
            for r in range(m):
                for c in range(r + 1, m):
                    R[r, c] = d[r] * rng.uniform(0.5, 1.5) * (1.0 if rng.random() < 0.5 else -1.0)
            model = noiseModel.Gaussian.SqrtInformation(R, smart=False)
    if robust is not None:
        model = noiseModel.Robust.Create(_MEstimator(int(robust[0]), float(robust[1])), model)
    assert model.kind == kind
    return model


# ---------------------------------------------------------------- the reference chain
def robust_weight(num, kind, k, d):
    """LossFunctions.cpp: Fair :146, Huber :179, Cauchy :217, Tukey :250, Welsch :289, GemanMcClure :320, DCS :354, L2WithDeadZone :400"""
    one, zero = num.scalar(1), num.scalar(0)
    if kind == 1:
        return one / (one + d / k)
    if kind == 2:
        return one if d <= k else k / d
    if kind == 3:
        return k * k / (k * k + d * d)
    if kind == 4:
        return (one - d * d / (k * k)) ** 2 if d <= k else zero
    if kind == 5:
        return num.exp(-(d * d) / (k * k))
    if kind == 6:
        return (k * k / (k * k + d * d)) ** 2
    if kind == 7:
        return (2 * k / (k + d * d)) ** 2 if d * d > k else one
    if kind == 8:
        return zero if d <= k else (d - k) / d
    raise ValueError(kind)


def robust_loss(num, kind, k, d):
    zero = num.scalar(0)
    if kind == 1:
        return k * k * (d / k - num.log1p(d / k))
    if kind == 2:
        return d * d / 2 if d <= k else k * (d - k / 2)
    if kind == 3:
        return k * k * num.log1p(d * d / (k * k)) / 2
    if kind == 4:
        return k * k * (1 - (1 - d * d / (k * k)) ** 3) / 6 if d <= k else k * k / 6
    if kind == 5:
        return -(k * k) * num.expm1(-(d * d) / (k * k)) / 2
    if kind == 6:
        return k * k * d * d / (k * k + d * d) / 2
    if kind == 7:
        e2 = d * d
        return (k * k * e2 + k * e2 * e2) / ((e2 + k) * (e2 + k))
    if kind == 8:
        return zero if d < k else (k - d) * (k - d) / 2
    raise ValueError(kind)


def whiten(num, J, model):
    """the Gaussian part: Unit leaves J, Diagonal multiplies row r by the stored FP64 number 1 / sigma_r (NoiseModel.cpp keeps
    invsigmas; the host hands them to the device), Gaussian multiplies by R"""
    if model.kind == N_UNIT:
        return J
    if model.kind == N_DIAG:
        return num.array(1.0 / model.data)[:, None] * J
    assert model.kind == N_GAUSS
    return num.array(model.data).dot(J)


def reference_factor(num, Ju, model, gw=None, robust_from_unwhitened=False):
    """(whitened, reweighted (rows, cols + 1) [A b], error, whitened |b|) of one factor from its unwhitened FP64 block Ju.
    robust_from_unwhitened is a planted defect of the CPU test."""
    Ju = num.array(Ju)
    Ab = whiten(num, Ju, model)
    b = (Ju if robust_from_unwhitened else Ab)[:, -1]
    bw = Ab[:, -1]
    d = num.sqrt((b * b).sum())
    if model.robust_kind:
        k = num.scalar(model.robust_k)
        Ab = Ab * num.sqrt(robust_weight(num, model.robust_kind, k, d))
        err = robust_loss(num, model.robust_kind, k, num.sqrt((bw * bw).sum()))
    else:
        err = (bw * bw).sum() / 2
    if gw is not None:
        Ab = Ab * num.sqrt(num.scalar(gw))
        err = err * num.scalar(gw)
    return Ab, err, d


# ---------------------------------------------------------------- a case: graph, values, ordering, and what the reference needs
class Case:
    def __init__(self, cls, name, fx):
        self.cls, self.name, self.fx = cls, name, fx
        self.graph, self.values, self.factors, self.ordering = NonlinearFactorGraph(), Values(), [], None
        self.weights = None      # GNC weights by graph index (interleaved_gnc)
        self.delta = None        # retract: {key: tangent vector}; expected = {key: (vtype, retracted value)}
        self.expected = None
        self._next = 0

    # -- building
    def var(self, vtype, value):
        key = self._next
        self._next += 1
        self.values.insert(key, vtype, value)
        return key

    def own(self, ft, case):
        """new variables holding the values of `case` of type ft"""
        return [self.var(t, v) for t, v in zip(FACTOR_VARS[ft], split_vals(ft, self.fx["f%d_vals" % ft][case]))]

    def add(self, ft, keys, case, model):
        for key, t, v in zip(keys, FACTOR_VARS[ft], split_vals(ft, self.fx["f%d_vals" % ft][case])):
            assert self.values.type(key) == t and np.array_equal(self.values.at(key), v), (self.name, ft, case, key)
        self.graph._add(ft, [keys], self.fx["f%d_meas" % ft][case], model)
        self.factors.append(dict(ft=ft, case=case, keys=[int(k) for k in keys], model=model))

    def tile(self, ft, n, kind, robust=None):
        """n factors of type ft on variables of their own, factor f = case f mod 37 under noise_for(ft, f, kind)"""
        for f in range(n):
            self.add(ft, self.own(ft, f % NCASE), f % NCASE, noise_for(ft, f, kind, robust))

    def finish(self, ordering=None):
        self.ordering = Ordering.Natural(self.graph) if ordering is None else Ordering(ordering)
        return self

    # -- the reference
    def unwhitened(self, g):
        f = self.factors[g]
        return self.fx["f%d_J" % f["ft"]][f["case"]].reshape(FACTOR_ROWS[f["ft"]], -1)

    def reference_blocks(self, num=LD, weights=None):
        """[(Ab, error, whitened |b| before the reweighting)] in graph order"""
        w = self.weights if weights is None else weights
        return [reference_factor(num, self.unwhitened(g), f["model"], None if w is None else w[g]) for g, f in enumerate(self.factors)]

    def hessian_diagonal(self, blocks, num=LD, third_at_d0=False):
        """{key: sum over the factors of the squared column norms}; third_at_d0 is a planted defect of the CPU test"""
        out = {k: num.array(np.zeros(VAR_DIM[self.values.type(k)])) for k in self.values.keys()}
        for f, (Ab, _, _) in zip(self.factors, blocks):
            dims, o = factor_dims(f["ft"]), 0
            for pos, (k, d) in enumerate(zip(f["keys"], dims)):
                c0 = dims[0] if (third_at_d0 and pos == 2) else o
                out[k] = out[k] + (Ab[:, c0:c0 + d] * Ab[:, c0:c0 + d]).sum(axis=0)
                o += d
        return out

    def linear_error_terms(self, blocks, delta_by_key, num=LD):
        """per factor (0.5 |b|^2, 0.5 |A d - b|^2)"""
        out = []
        for f, (Ab, _, _) in zip(self.factors, blocks):
            d = num.array(np.concatenate([np.asarray(delta_by_key[k], dtype=np.float64) for k in f["keys"]]))
            r = Ab[:, :-1].dot(d) - Ab[:, -1]
            out.append(((Ab[:, -1] * Ab[:, -1]).sum() / 2, (r * r).sum() / 2))
        return out

    def linear_errors(self, blocks, delta_by_key, num=LD):
        t = self.linear_error_terms(blocks, delta_by_key, num)
        return fsum(x[0] for x in t), fsum(x[1] for x in t)

    # -- the layout linear_error_kernel sees
    def descriptors(self):
        """[(sz, joff, cols, arity)] in graph order.  Restated from the host tables: a bucket is (type, device noise kind, robust kind, k)
        in order of first appearance; its factors lie back to back in graph order; every bucket starts at a multiple of 16 doubles."""
        order, members = [], {}
        for g, f in enumerate(self.factors):
            m = f["model"]
            key = (f["ft"], N_UNIT if m.kind == N_UNIT else (N_GAUSS if m.kind == N_GAUSS else N_DIAG), m.robust_kind, m.robust_k)
            if key not in members:
                members[key] = []
                order.append(key)
            members[key].append(g)
        joff, off = {}, 0
        for key in order:
            sz = factor_size(key[0])
            for i, g in enumerate(members[key]):
                joff[g] = off + i * sz
            off = (off + len(members[key]) * sz + 15) & ~15
        return [(factor_size(f["ft"]), joff[g], factor_cols(f["ft"]), len(f["keys"])) for g, f in enumerate(self.factors)]

    def bucket_positions(self):
        """position of every factor inside its bucket, in graph order"""
        seen, out = {}, []
        for f in self.factors:
            m = f["model"]
            key = (f["ft"], m.kind, m.robust_kind, m.robust_k)
            out.append(seen.get(key, 0))
            seen[key] = out[-1] + 1
        return out


def fsum(it):
    return math.fsum(float(x) for x in it)


LINERR_MAX_SZ, LINERR_STRIDE = 32, 512


def linear_error_waves(desc):
    """one dict per 64-lane wave of the launch (256-lane blocks over len(desc) factors), restated from linear_error_kernel:
    cnt      valid lanes (<= 0: the wave has none, it skips the copy and every lane returns)
    path     'empty' | 'staged' (one shape <= 32 doubles, back to back) | 'direct_big' (a shape above 32) | 'direct_mixed'
    passes   staged: trips of the 512-stride copy loop; partial: the last trip is not full; padded: pitch sz | 1 differs from sz
    forms    the column forms of its valid lanes: 'small' (<= 12 columns, the unrolled form), 'loop3' (three variables), 'loop18'"""
    n, out = len(desc), []
    for w in range(4 * ((n + 255) // 256)):
        cnt = min(64, n - 64 * w)
        if cnt <= 0:
            out.append(dict(cnt=cnt, path="empty", forms=set()))
            continue
        lanes = desc[64 * w:64 * w + cnt]
        sz0, j0 = lanes[0][0], lanes[0][1]
        forms = {"small" if d[2] <= 12 else ("loop3" if d[3] == 3 else "loop18") for d in lanes}
        if all(d[0] == sz0 and d[1] == j0 + i * sz0 for i, d in enumerate(lanes)) and sz0 <= LINERR_MAX_SZ:
            total = cnt * sz0
            out.append(dict(cnt=cnt, path="staged", forms=forms, sz=sz0, passes=-(-total // LINERR_STRIDE), partial=total % LINERR_STRIDE != 0,
                            padded=(sz0 | 1) != sz0))
        else:
            out.append(dict(cnt=cnt, path="direct_big" if max(d[0] for d in lanes) > LINERR_MAX_SZ else "direct_mixed", forms=forms,
                            same_shape=all(d[0] == sz0 for d in lanes)))
    return out


# ---------------------------------------------------------------- the case table
def _whiten(fx, ft, kind, n):
    c = Case("whiten", "whiten_t%d_%s_n%d" % (ft, KIND_NAME[kind], n), fx)
    c.tile(ft, n, kind)
    return c.finish()


def _sfm_blocks(fx, kind, n):
    c = Case("sfm_blocks", "sfm_%s_n%d" % (KIND_NAME[kind], n), fx)
    c.tile(F_SFM, n, kind)
    return c.finish()


def robust_constant(fx, ft, kind, rk):
    """the m-estimator constant of a robust case, from the reference alone: the geometric middle of the widest relative gap between
    two consecutive whitened |b| in the central third of the 129 sorted values, to three significant digits (squared for DCS, whose
    switch is at d^2 = k).  Between a third and two thirds of the factors lie on each side, and none lies so close to the switch that
    1 - d^2 / k^2 (Tukey) or (d - k) / d (dead zone) loses more than a digit or two."""
    d = [reference_factor(LD, fx["f%d_J" % ft][f % NCASE].reshape(FACTOR_ROWS[ft], -1), noise_for(ft, f, kind))[2] for f in range(ROBUST_N)]
    d = np.sort(np.array(d, dtype=np.float64))
    lo, hi = ROBUST_N // 3, 2 * ROBUST_N // 3
    i = lo + int(np.argmax(d[lo + 1:hi + 1] / d[lo:hi]))
    k = float("%.3g" % np.sqrt(d[i] * d[i + 1]))
    assert d[i] * 1.02 < k < d[i + 1] / 1.02, (ft, kind, d[i], k, d[i + 1])
    return float("%.6g" % (k * k)) if rk == 7 else k


def _robust(fx, ft, kind, rk):
    c = Case("robust", "robust_t%d_%s_m%d" % (ft, KIND_NAME[kind], rk), fx)
    c.tile(ft, ROBUST_N, kind, (rk, robust_constant(fx, ft, kind, rk)))
    return c.finish()


class _Chain:
    """variables of one chained type, created when first used; variable j holds chain value j mod 37"""

    def __init__(self, case, vt):
        self.case, self.vt, self._keys = case, vt, {}

    def key(self, j):
        if j not in self._keys:
            self._keys[j] = self.case.var(self.vt, self.case.fx["f%d_vals" % CHAIN_PRIOR[self.vt]][j % NCASE])
        return self._keys[j]

    def between(self, j, kind):
        """a between factor from variable j to j + 1"""
        ft = CHAIN_BETWEEN[self.vt]
        self.case.add(ft, [self.key(j), self.key(j + 1)], j % NCASE, noise_for(ft, len(self.case.factors), kind))

    def prior(self, j, kind):
        ft = CHAIN_PRIOR[self.vt]
        self.case.add(ft, [self.key(j)], j % NCASE, noise_for(ft, len(self.case.factors), kind))


def _interleaved(fx, gnc=False):
    """257 factors cycling one at a time through between Pose2 under Unit, Diagonal and Gaussian noise, bearing-range, prior Pose2,
    between Pose3, prior Pose3 and GeneralSFMFactor2: graph order differs from bucket order everywhere"""
    c = Case("interleaved", "interleaved_gnc" if gnc else "interleaved", fx)
    p2, p3 = _Chain(c, POSE2), _Chain(c, POSE3)
    K = c.var(CAL3_S2, split_vals(F_SFM2, fx["f%d_vals" % F_SFM2][0])[2])
    pts = {}
    for g in range(257):
        s, t = g % 8, g // 8
        j = t % NCASE
        if s < 3:
            p2.between((3 * t + s) % NCASE, (N_UNIT, N_DIAG, N_GAUSS)[s])
        elif s == 3:
            lm = c.var(POINT2, split_vals(F_BEARING_RANGE_2D, fx["f%d_vals" % F_BEARING_RANGE_2D][j])[1])
            c.add(F_BEARING_RANGE_2D, [p2.key(j), lm], j, noise_for(F_BEARING_RANGE_2D, g, N_DIAG))
        elif s == 4:
            p2.prior(t % (NCASE + 1), N_GAUSS)
        elif s == 5:
            p3.between(j, N_DIAG)
        elif s == 6:
            p3.prior(t % (NCASE + 1), N_GAUSS)
        else:
            if j not in pts:
                pts[j] = c.var(POINT3, split_vals(F_SFM2, fx["f%d_vals" % F_SFM2][j])[1])
            c.add(F_SFM2, [p3.key(0), pts[j], K], j, noise_for(F_SFM2, g, N_DIAG))
    if gnc:
        w = np.random.default_rng(257).random(257)
        w[::9], w[4::11] = 0.0, 1.0
        c.weights = w
    return c.finish()


def _chain_graph(c, vt, nfac, priors_first, kb, kp):
    """nfac factors on a chain of ceil(nfac / 3) variables: a prior on every variable and nfac - nv between factors that walk the chain
    (again from its start when they run out of links), all betweens then all priors or the other way round"""
    nv = max(1, (nfac + 2) // 3)
    ch = _Chain(c, vt)
    nb = nfac - nv
    assert nb == 0 or nv >= 2

    def betweens():
        for i in range(nb):
            ch.between(i % (nv - 1), kb)

    def priors():
        for j in range(nv):
            ch.prior(j, kp)
    (priors if priors_first else betweens)()
    (betweens if priors_first else priors)()
    return ch


def _linerr_a(fx, nfac, priors_first):
    c = Case("linear_error", "linerr_a_n%d_%s" % (nfac, "pb" if priors_first else "bp"), fx)
    _chain_graph(c, POSE2, nfac, priors_first, N_DIAG, N_GAUSS)
    return c.finish()


def _linerr_b(fx):
    """sz 12: 70 bearing-range factors (a full staged wave is 768 doubles: two trips of the copy loop, the second partial), 70 Point3
    priors on points of their own, then the priors of the poses"""
    c = Case("linear_error", "linerr_b_sz12", fx)
    p2 = _Chain(c, POSE2)
    for f in range(70):
        j = f % NCASE
        lm = c.var(POINT2, split_vals(F_BEARING_RANGE_2D, fx["f%d_vals" % F_BEARING_RANGE_2D][j])[1])
        c.add(F_BEARING_RANGE_2D, [p2.key(j), lm], j, noise_for(F_BEARING_RANGE_2D, f, N_GAUSS))
    c.tile(F_PRIOR_POINT3, 70, N_DIAG)
    for j in range(NCASE + 1):
        p2.prior(j, N_DIAG)
    return c.finish()


def _linerr_c(fx):
    """sz 30: 70 GeneralSFMFactor2 (staged, then the fac_xoff column loop) on one pose, 37 points and one calibration, then their priors"""
    c = Case("linear_error", "linerr_c_sfm2", fx)
    vals = fx["f%d_vals" % F_SFM2]
    pose, K = c.var(POSE3, split_vals(F_SFM2, vals[0])[0]), c.var(CAL3_S2, split_vals(F_SFM2, vals[0])[2])
    pts = [c.var(POINT3, split_vals(F_SFM2, vals[j])[1]) for j in range(NCASE)]
    for f in range(70):
        c.add(F_SFM2, [pose, pts[f % NCASE], K], f % NCASE, noise_for(F_SFM2, f, N_GAUSS))
    for j in range(NCASE):
        c.add(F_PRIOR_POINT3, [pts[j]], j, noise_for(F_PRIOR_POINT3, j, N_DIAG))
    c.add(F_PRIOR_POSE3, [pose], 0, noise_for(F_PRIOR_POSE3, 0, N_GAUSS))
    c.add(F_PRIOR_CAL3_S2, [K], 0, noise_for(F_PRIOR_CAL3_S2, 0, N_DIAG))
    return c.finish()


def _linerr_d(fx):
    """sz 78 and 90: the direct path with 12 and 9 columns"""
    c = Case("linear_error", "linerr_d_big", fx)
    _chain_graph(c, POSE3, 130, False, N_GAUSS, N_DIAG)
    c.tile(F_PRIOR_CAM, 66, N_GAUSS)
    return c.finish()


def _linerr_e(fx):
    """18 columns: the direct path with the column loop and d2 = 0"""
    c = Case("linear_error", "linerr_e_chordal", fx)
    _chain_graph(c, VEC9, 100, False, N_DIAG, N_UNIT)
    return c.finish()


def _linerr_f(fx):
    """63 between-Pose2 factors and one bearing-range factor in the same wave: one lane breaks the staged path"""
    c = Case("linear_error", "linerr_f_one_lane", fx)
    p2 = _Chain(c, POSE2)
    for i in range(63):
        p2.between(i % NCASE, N_DIAG)
    lm = c.var(POINT2, split_vals(F_BEARING_RANGE_2D, fx["f%d_vals" % F_BEARING_RANGE_2D][5])[1])
    c.add(F_BEARING_RANGE_2D, [p2.key(5), lm], 5, noise_for(F_BEARING_RANGE_2D, 63, N_DIAG))
    for j in range(NCASE + 1):
        p2.prior(j, N_GAUSS)
    return c.finish()


def _linerr_g(fx):
    """two between-Pose2 buckets, 16 Diagonal then 56 Gaussian factors: 16 x 21 doubles is a multiple of 16, so the second bucket
    follows the first without padding and the first wave stages across the bucket boundary"""
    c = Case("linear_error", "linerr_g_two_buckets", fx)
    p2 = _Chain(c, POSE2)
    for i in range(72):
        p2.between(i % NCASE, N_DIAG if i < 16 else N_GAUSS)
    for j in range(NCASE + 1):
        p2.prior(j, N_UNIT)
    return c.finish()


def _hessian_diag(fx, ntot):
    """a hub Pose3 in all three column positions of 300 factors (first and second variable of between factors, the pose of
    GeneralSFMFactor2), the shared Cal3_S2 in the third position, and single-factor variables filling the total dimension to ntot"""
    c = Case("hessian_diag", "hdiag_ntot%d" % ntot, fx)
    p3 = fx["f%d_vals" % F_PRIOR_POSE3]
    hub, nxt, prv = c.var(POSE3, p3[0]), c.var(POSE3, p3[1]), c.var(POSE3, p3[NCASE - 1])
    K = c.var(CAL3_S2, split_vals(F_SFM2, fx["f%d_vals" % F_SFM2][0])[2])
    pts = [c.var(POINT3, split_vals(F_SFM2, fx["f%d_vals" % F_SFM2][j])[1]) for j in range(NCASE)]
    for t in range(100):
        c.add(F_BETWEEN_POSE3, [hub, nxt], 0, noise_for(F_BETWEEN_POSE3, 3 * t, N_GAUSS))
        c.add(F_SFM2, [hub, pts[t % NCASE], K], t % NCASE, noise_for(F_SFM2, 3 * t + 1, N_GAUSS))
        c.add(F_BETWEEN_POSE3, [prv, hub], NCASE - 1, noise_for(F_BETWEEN_POSE3, 3 * t + 2, N_DIAG))
    rest = ntot - c.values.dim()
    n5 = {0: 0, 1: 2, 2: 1}[rest % 3]   # bearing-range pairs (3 + 2 scalars), the rest Point3 priors (3 scalars)
    for i in range(n5):
        c.add(F_BEARING_RANGE_2D, c.own(F_BEARING_RANGE_2D, i), i, noise_for(F_BEARING_RANGE_2D, i, N_GAUSS))
    for i in range((rest - 5 * n5) // 3):
        c.add(F_PRIOR_POINT3, c.own(F_PRIOR_POINT3, (i + 1) % NCASE), (i + 1) % NCASE, noise_for(F_PRIOR_POINT3, i, N_DIAG))
    assert c.values.dim() == ntot
    return c.finish()


def reduce_problem(n):
    """(graph, values, exact per-factor errors): n Point3 priors under Unit noise on variables of their own, added in bulk.
    x - m = (1 + i 2^-17, 1/2, -1/4): every difference, square and sum is exact in FP64, the terms are distinct and lie in
    [0.65, 2.2], i.e. each is more than a quarter of the mean"""
    i = np.arange(n, dtype=np.float64)
    x = np.stack([2.0 + i * 2.0 ** -17, np.full(n, 1.5), np.full(n, 0.75)], axis=1)
    graph, values = NonlinearFactorGraph(), Values()
    for k in range(n):
        values.insert(k, POINT3, x[k])
    graph._add(F_PRIOR_POINT3, np.arange(n).reshape(-1, 1), np.ones((n, 3)), noiseModel.Unit.Create(3))
    d = x - 1.0
    return graph, values, 0.5 * (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def reduce_chain_bound(n):
    """additions of the longest chain of reduce_stage1 / reduce_stage2 over n elements: the grid-stride loop of a thread, the 8-level
    tree of its block, then the same over the g partial sums"""
    g = min(256, -(-n // 256))
    return -(-n // (256 * g)) + 8 + -(-g // 256) + 8


RETRACT_PRIOR = {POSE2: F_PRIOR_POSE2, POSE3: F_PRIOR_POSE3, POINT3: F_PRIOR_POINT3, CAM_BUNDLER: F_PRIOR_CAM, CAL3_S2: F_PRIOR_CAL3_S2,
                 VEC9: F_PRIOR_VEC9}


def _retract(fx, n):
    """n variables of every type tiling the 37 retract cases (whose values are the chain values, so the prior case j mod 37 fits
    variable j; a Point2 hangs on Pose2 variable j by bearing-range case j mod 37), in a seeded shuffled ordering: xoff is not
    monotone inside a type array.  delta is given by key; the test packs it in the ordering."""
    c = Case("retract", "retract_n%d" % n, fx)
    c.delta, c.expected, by_type = {}, {}, {}
    for j in range(n):          # types interleaved variable by variable
        for vt in VAR_TYPES:
            k = c.var(vt, fx["r%d_val" % vt][j % NCASE])
            by_type.setdefault(vt, []).append(k)
            c.delta[k], c.expected[k] = fx["r%d_delta" % vt][j % NCASE], (vt, fx["r%d_exp" % vt][j % NCASE])
    for j in range(n):
        for vt in VAR_TYPES:
            if vt == POINT2:
                c.add(F_BEARING_RANGE_2D, [by_type[POSE2][j], by_type[POINT2][j]], j % NCASE, noiseModel.Unit.Create(2))
            else:
                c.add(RETRACT_PRIOR[vt], [by_type[vt][j]], j % NCASE, noiseModel.Unit.Create(VAR_DIM[vt]))
    order = np.array(c.values.keys())
    np.random.default_rng(n).shuffle(order)
    return c.finish([int(k) for k in order])


def _table():
    T = {}
    for ft in FACTOR_TYPES:
        for kind in (N_DIAG, N_GAUSS):
            for n in WHITEN_SIZES:
                T["whiten_t%d_%s_n%d" % (ft, KIND_NAME[kind], n)] = ("whiten", lambda fx, a=ft, b=kind, c=n: _whiten(fx, a, b, c))
    for kind in (N_UNIT, N_DIAG, N_GAUSS):
        for n in SFM_SIZES:
            T["sfm_%s_n%d" % (KIND_NAME[kind], n)] = ("sfm_blocks", lambda fx, b=kind, c=n: _sfm_blocks(fx, b, c))
    for ft in ROBUST_TYPES:
        for kind in (N_DIAG, N_GAUSS):
            for rk in range(1, 9):
                T["robust_t%d_%s_m%d" % (ft, KIND_NAME[kind], rk)] = ("robust", lambda fx, a=ft, b=kind, c=rk: _robust(fx, a, b, c))
    T["interleaved"] = ("interleaved", lambda fx: _interleaved(fx))
    T["interleaved_gnc"] = ("interleaved", lambda fx: _interleaved(fx, True))
    for nfac in (1, 63, 64, 65, 255, 256, 257):
        for pf in (False, True):
            T["linerr_a_n%d_%s" % (nfac, "pb" if pf else "bp")] = ("linear_error", lambda fx, a=nfac, b=pf: _linerr_a(fx, a, b))
    for nm, fn in (("linerr_b_sz12", _linerr_b), ("linerr_c_sfm2", _linerr_c), ("linerr_d_big", _linerr_d), ("linerr_e_chordal", _linerr_e),
                   ("linerr_f_one_lane", _linerr_f), ("linerr_g_two_buckets", _linerr_g)):
        T[nm] = ("linear_error", fn)
    for ntot in HDIAG_NTOT:
        T["hdiag_ntot%d" % ntot] = ("hessian_diag", lambda fx, a=ntot: _hessian_diag(fx, a))
    for n in RETRACT_SIZES:
        T["retract_n%d" % n] = ("retract", lambda fx, a=n: _retract(fx, a))
    return T


CASES = _table()


def names(cls):
    return [k for k, v in CASES.items() if v[0] == cls]


def build(fx, name):
    c = CASES[name][1](fx)
    assert c.name == name and c.cls == CASES[name][0], (name, c.name)
    return c


# ---------------------------------------------------------------- deviations and floors
def dev(got, exp):
    """max-abs difference relative to max(1, |expected|) of that case and quantity"""
    got, exp = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(exp, dtype=np.float64).reshape(-1)
    if got.shape != exp.shape or not np.all(np.isfinite(got)):
        return np.inf
    return float(np.abs(got - exp).max() / max(1.0, np.abs(exp).max()))


def floor_index(f):
    """index of a factor (an entry of Case.factors) into the fixture's floor_J / floor_err: [factor type][0 unit, 1 diagonal,
    2 gaussian][m-estimator id, 0 without Robust]"""
    return f["ft"], {N_UNIT: 0, N_DIAG: 1, N_GAUSS: 2}[f["model"].kind], int(f["model"].robust_kind)


def to_f64(a):
    return np.asarray(a, dtype=np.float64)
