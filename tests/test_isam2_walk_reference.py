"""The ISAM2 walk cases (isam2_walk_cases.py) and the longdouble restatement of the walk kernels (isam2_walk_reference.py) held against the
CPU oracle, with the cases' own ordering (no oracle/_ref needed): every edge of EDGES is reached by a clique the oracle really builds,
the restatement on the oracle's tree reproduces the oracle's getDelta(), marginalCovariance() and dog-leg step within the float64 floor of
the same operation, and every margin the GPU suite relies on holds -- threshold factor 10, radius factor 1.5, the rho bands, the 1e-9 cap
on 16 x floor.  test_gpu_isam2_walk_edges.py runs the same checks with the device in the oracle's place; a failure there and none here
points at a kernel."""
import functools

import numpy as np
import pytest

import isam2_walk_cases as wc
import isam2_walk_reference as wr
import oracle_harness as oh


def make(threshold):
    return oh.OracleISAM2(0.0, 0, False, threshold, ccolamd=wc.natural_order)


def make_dogleg(radius):
    orc = make(0.0)
    orc.set_dogleg(radius, 0.0, 2)
    return orc


@functools.lru_cache(maxsize=None)
def tables(name):
    """the clique tables (nf, ns, children, root) of the oracle's tree after each update"""
    c, orc = wc.case(name), make(0.0)
    return [wc.clique_table(wr.Tree(orc.cliques(), wc.dims_of(c))) for _ in wc.replay(c, orc, upto=2)]


def test_every_edge_is_covered():
    missing = [e for e, pred in wc.EDGES.items() if not any(pred(t) for n in wc.NAMES for t in tables(n))]
    assert not missing, missing


def test_the_memory_boundary_lies_where_the_cases_say():
    """n - 1 = 139 is (64, 75), n - 1 = 140 is (65, 75)"""
    assert (64, 75) in [t[:2] for t in tables("pair[64,75]")[0]] and (65, 75) in [t[:2] for t in tables("pair[65,75]")[0]]
    assert wc.LDS_MAX_COLS == 139


@pytest.mark.parametrize("name", wc.NAMES)
def test_wildfire_reproduces_the_oracle(name):
    c = wc.case(name)
    _, stats = wc.check_walk(c, make, c["threshold"])
    if name in wc.THRESHOLD_NAMES:  # the threshold cuts the walk: some clique is visited and left, some never visited
        assert stats[1]["kept"] < stats[1]["visited"] < len(c["expect"])


@pytest.mark.parametrize("name", wc.NAMES)
def test_full_solve_and_marginals_reproduce_the_oracle(name):
    c = wc.case(name)
    orc, _ = wc.check_walk(c, make, 0.0)
    tree = wr.Tree(orc.cliques(), wc.dims_of(c))
    assert wr.deviation(tree.vec(orc.getDelta(), np.float64), wr.full_solve(tree)) <= wr.tolerance(wr.deviation(wr.full_solve(tree, np.float64), wr.full_solve(tree)), tree.widest())
    wc.check_marginals(c, orc, dense=True)


@pytest.mark.parametrize("name", wc.DOGLEG_NAMES)
def test_dogleg_reproduces_the_oracle(name):
    c = wc.case(name)
    # the stored radii are the three the issue names, from the restatement on the oracle's tree
    orc = make(0.0)
    g, v, _ = c["updates"][0]
    orc.update(g, v)
    d = wr.dogleg_point(wr.Tree(orc.cliques(), wc.dims_of(c)), 1.0)
    want = (0.5 * d["nu"], float(np.sqrt(d["nu"] * d["nn"])), 2.0 * d["nn"])
    assert np.allclose(c["radii"], want, rtol=1e-4), (name, want)
    assert d["nn"] >= 1.5 ** 2 * d["nu"], "no room for a blend radius a factor 1.5 from both norms"
    stats = wc.check_dogleg(c, make_dogleg)
    assert all(s["rho"] >= 0.825 for s in stats)  # (all cases start near their solution: the model is good)


def test_threshold_gaps():
    """the thresholds of the section-5 cases lie in the widest gap of the changes"""
    for name in wc.THRESHOLD_NAMES:
        c = wc.case(name)
        _, stats = wc.check_walk(c, make, 1e-300)  # (every clique visited and kept: all changes)
        ch = np.array([x for x in stats[1]["changes"] if x > 0])
        gaps = ch[1:] / ch[:-1]
        i = int(np.argmax(gaps))
        assert ch[i] * 10 <= c["threshold"] <= ch[i + 1] / 10, (name, ch[i], ch[i + 1])


def test_epoch_case():
    """262 updates, each with a reader: the threshold margins at EVERY update, the walk cut at the anchor"""
    c = wc.epoch_case(35)
    assert len(c["updates"]) >= 260
    _, stats = wc.check_walk(c, make, c["threshold"])
    assert all(s["kept"] < s["visited"] < len(c["expect"]) for s in stats[1:])
    orc, _ = wc.check_walk(c, make_dogleg_wide, 0.0, exact=False)


def make_dogleg_wide(_threshold):
    return make_dogleg(1e3)  # a radius no Newton step reaches: the dog-leg point is the Newton point, the walk's result


class _OneKeyLeftOut:
    """a solver whose walk never reaches `key` after the first update: its delta keeps the value it had"""

    def __init__(self, inner, key):
        self.inner, self.key, self.last = inner, key, None

    def update(self, g, v):
        return self.inner.update(g, v)

    def cliques(self):
        return self.inner.cliques()

    def getDelta(self):
        d = self.inner.getDelta()
        if self.last is not None:
            d[self.key] = self.last[self.key]
        self.last = d
        return d


@pytest.mark.parametrize("key", [1, 256, 257])
def test_a_child_left_out_of_the_walk_is_seen(key):
    """planted defect: one of the 257 children of one root is never queued (a children loop of one pass of 256)"""
    c = wc.case("children[257]")
    with pytest.raises(AssertionError):
        wc.check_walk(c, lambda thr: _OneKeyLeftOut(make(thr), key), c["threshold"])


def test_restatement_against_mpmath():
    """the longdouble restatement itself, on a small tree, against 50 digits"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    c, orc = wc.case("forest[1]"), make(0.0)
    for _ in wc.replay(c, orc):
        pass
    tree = wr.Tree(orc.cliques(), wc.dims_of(c))
    R, pos = wr.global_R(tree, np.float64)
    d = np.zeros(tree.n)
    for cl in tree.cliques:
        d[pos[cl["fx"]]] = cl["rsd"][:, -1]
    Rm = mp.matrix(R.tolist())
    x = mp.lu_solve(Rm, mp.matrix(d.tolist()))
    ref = np.array([float(x[int(pos[i])]) for i in range(tree.n)])
    assert wr.deviation(wr.full_solve(tree), ref) <= 4 * wr.EPS
    cov = (Rm.T * Rm) ** -1
    k = c["marginals"][0]
    idx = [int(pos[tree.off[k] + i]) for i in range(tree.dims[k])]
    refc = np.array([[float(cov[a, b]) for b in idx] for a in idx])
    assert wr.deviation(wr.marginal_covariance(tree, k), refc) <= 4 * wr.EPS
