"""numpy restatement of the reference's translation averaging: the checker of the device's TranslationRecovery (include/lmgpu.h, the
lmgpu_translation_recovery_* group).  Dense and sequential.
  TranslationFactor::evaluateError           gtsam/sfm/TranslationFactor.h:68-78 with normalize, gtsam/geometry/Point3.cpp:52-62
  BetweenFactor<Point3>, PriorFactor<Point3> gtsam/slam/BetweenFactor.h:111-124, gtsam/nonlinear/PriorFactor.h:98-102
  TranslationRecovery::run                   gtsam/sfm/TranslationRecovery.cpp:49-228 (zero-direction sets, buildGraph, addPrior,
                                             initializeRandomly, the empty-initial branch, addSameTranslationNodes)
  the optimizer                              smart_restatement.LM (LevenbergMarquardtOptimizer.cpp:121-308, defaultOptimize) on this
                                             module's Graph, which records the loop's decisions in `ctl`
Stated deviations, the same as the library's: a set's representative is its smallest key; the generator is a 32-bit Mersenne Twister
owned by the caller (seed 42 by default), a coordinate is 2 ((x1 + x2 2^32) / 2^64) - 1 from two consecutive draws.
A value is a 3-vector; values are a dict key -> vector.  An edge is (key1, key2, z, Noise | None)."""
import numpy as np

import smart_restatement as sr


# ---------------------------------------------------------------- the generator
class MT19937:
    """the 32-bit Mersenne Twister of std::mt19937 (Matsumoto & Nishimura 1998; init_genrand with 1812433253)"""

    def __init__(self, seed=42):
        self.seed(seed)

    def seed(self, s):
        mt = [0] * 624
        mt[0] = int(s) & 0xFFFFFFFF
        for i in range(1, 624):
            mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.mt, self.i = mt, 624

    def __call__(self):
        if self.i >= 624:
            mt = self.mt
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7FFFFFFF)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.i = 0
        y = self.mt[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def uniform(gen):
    """one coordinate in [-1, 1): the two draws in double arithmetic, as the library writes it out"""
    x1 = float(gen())
    x2 = float(gen())
    return 2.0 * ((x1 + x2 * 4294967296.0) / 18446744073709551616.0) - 1.0


# ---------------------------------------------------------------- noise
class Noise:
    """a Gaussian model as its square-root information R (whitened e = R e), optionally under noiseModel::Robust with Huber(k)"""

    def __init__(self, R, huber_k=None):
        self.R = np.asarray(R, dtype=float).reshape(3, 3)
        self.huber_k = huber_k

    @staticmethod
    def isotropic(sigma, huber_k=None):
        return Noise(np.eye(3) / sigma, huber_k)

    @staticmethod
    def diagonal(sigmas, huber_k=None):
        return Noise(np.diag(1.0 / np.asarray(sigmas, dtype=float)), huber_k)


UNIT = Noise(np.eye(3))


def _huber_weight(k, d):
    return 1.0 if d <= k else k / d  # LossFunctions.cpp:179-182


def _huber_loss(k, d):
    return d * d / 2 if d <= k else k * (d - k / 2)  # :184-191


# ---------------------------------------------------------------- factors
def normalize_jac(p):
    """H of Point3.cpp:52-62"""
    x, y, z = p
    x2, y2, z2, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
    H = np.array([[y2 + z2, -xy, -xz], [-xy, x2 + z2, -yz], [-xz, -yz, x2 + y2]])
    return H / (x2 + y2 + z2) ** 1.5


class Factor:
    """keys, unwhitened error e(values) and Jacobians [H_k]; whitening, Robust and the Hessian form are shared"""

    def __init__(self, keys, z, noise):
        self.keys, self.z, self.noise = [int(k) for k in keys], np.asarray(z, dtype=float).reshape(3), noise or UNIT

    def whitened(self, values):
        """-> ([A_k], b) of NoiseModelFactor::linearize (NonlinearFactor.cpp:152-184): A = R H, b = -R e, times sqrt(weight) under Robust"""
        e, Hs = self.evaluate(values)
        A, b = [self.noise.R @ H for H in Hs], -(self.noise.R @ e)
        if self.noise.huber_k is not None:
            w = np.sqrt(_huber_weight(self.noise.huber_k, np.sqrt(b @ b)))
            A, b = [w * a for a in A], w * b
        return A, b

    def jacobian(self, values):
        """[A1 (A2) b], rows x (3 arity + 1): what lmgpu_get_jacobian returns"""
        A, b = self.whitened(values)
        return np.hstack(A + [b.reshape(3, 1)])

    def error(self, values):
        e, _ = self.evaluate(values)
        we = self.noise.R @ e
        if self.noise.huber_k is not None:
            return _huber_loss(self.noise.huber_k, np.sqrt(we @ we))
        return 0.5 * (we @ we)

    def hessian(self, values):
        J = self.jacobian(values)
        return J.T @ J


class TranslationFactor(Factor):
    def evaluate(self, values):
        d = values[self.keys[1]] - values[self.keys[0]]
        H = normalize_jac(d)
        return d / np.sqrt(d @ d) - self.z, [-H, H]


class BetweenPoint3(Factor):
    def evaluate(self, values):
        return (values[self.keys[1]] - values[self.keys[0]]) - self.z, [-np.eye(3), np.eye(3)]


class PriorPoint3(Factor):
    def evaluate(self, values):
        return values[self.keys[0]] - self.z, [np.eye(3)]


class Graph:
    """the interface smart_restatement.LM drives: error, linearize -> (H, g, c), retract"""

    def __init__(self, factors, order):
        self.factors, self.order = list(factors), [int(k) for k in order]
        self.col = {k: 3 * i for i, k in enumerate(self.order)}

    def error(self, values):
        return float(sum(f.error(values) for f in self.factors))

    def linearize(self, values):
        n = 3 * len(self.order)
        H, g, c = np.zeros((n, n)), np.zeros(n), 0.0
        for f in self.factors:
            A = f.hessian(values)
            idx = np.concatenate([np.arange(self.col[k], self.col[k] + 3) for k in f.keys])
            H[np.ix_(idx, idx)] += A[:-1, :-1]
            g[idx] += A[:-1, -1]
            c += A[-1, -1]
        return H, g, c

    def retract(self, values, delta):
        return {k: values[k] + delta[self.col[k]:self.col[k] + 3] for k in values}


# ---------------------------------------------------------------- TranslationRecovery::run
def merge_sets(relative):
    """getSameTranslationDSFMap (:49-60) -> {key: representative} over the keys of `relative`, the smallest key of a set representing it"""
    parent = {}

    def find(k):
        parent.setdefault(k, k)
        while parent[k] != k:
            k = parent[k]
        return k

    for k1, k2, z, _ in relative:
        a, b = find(int(k1)), find(int(k2))
        if a != b and np.abs(np.asarray(z, dtype=float)).max() <= 1e-9:  # Unit3::equals' default tolerance
            parent[max(a, b)] = min(a, b)
    return {k: find(k) for k in list(parent)}


def build(relative, scale=1.0, betweens=(), initial_values=None, gen=None, prior_sigma=0.01):
    """everything of run() before the optimizer: -> dict(factors, initial, keys, rep, n_dir).  `gen` is advanced by the random draws."""
    gen = gen if gen is not None else MT19937(42)
    rep = merge_sets(relative)
    keys = list(rep)
    for k1, k2, _, _ in betweens:
        for k in (int(k1), int(k2)):
            if k not in rep:
                rep[k] = k
                keys.append(k)

    def reduce(edges):
        out = []
        for k1, k2, z, m in edges:
            a, b = rep[int(k1)], rep[int(k2)]
            if a != b:
                out.append((a, b, np.asarray(z, dtype=float), m))
        return out

    D, B = reduce(relative), reduce(betweens)
    factors = [TranslationFactor((a, b), z, m) for a, b, z, m in D]
    if D:  # addPrior (:119-143)
        a, b, z, m = D[0]
        factors.append(PriorPoint3((a,), np.zeros(3), Noise.isotropic(prior_sigma)))
        if not B:
            factors.append(PriorPoint3((b,), scale * z, m))
        else:
            factors += [BetweenPoint3((a2, b2), z2, m2) for a2, b2, z2, m2 in B]
    initial = {}
    for a, b, _, _ in D + B:
        for k in (a, b):
            if k in initial:
                continue
            if initial_values is not None and k in initial_values:
                initial[k] = np.asarray(initial_values[k], dtype=float).copy()
            else:
                initial[k] = np.array([uniform(gen), uniform(gen), uniform(gen)])
    if not initial and relative:  # :218-223
        for k in keys:
            if rep[k] == k:
                initial[k] = np.zeros(3)
    return dict(factors=factors, initial=initial, keys=keys, rep=rep, n_dir=len(D))


def run(relative, scale=1.0, betweens=(), initial_values=None, gen=None, prior_sigma=0.01, params=None, order=None):
    """-> (result {key: Point3} over every key of the input, the LM object | None for an empty graph, its (error, lambda) history)"""
    P = build(relative, scale, betweens, initial_values, gen, prior_sigma)
    values, lm, hist = dict(P["initial"]), None, []
    if P["factors"]:
        order = [k for k in (order if order is not None else P["initial"]) if k in P["initial"]]
        lm = sr.LM(Graph(P["factors"], order), P["initial"], params)
        hist = lm.optimize()
        values = lm.values
    return {k: values[P["rep"][k]].copy() for k in P["keys"]}, lm, hist


def simulate(positions, edges, sigma=0.01):
    """SimulateMeasurements (:230-243) on {key: position}: Unit3(Tb - Ta), the zero vector for coincident positions"""
    out = []
    for a, b in edges:
        d = np.asarray(positions[b], dtype=float) - np.asarray(positions[a], dtype=float)
        n = np.sqrt(d @ d)
        out.append((a, b, d / n if n > 0 else d, Noise.isotropic(sigma)))
    return out
