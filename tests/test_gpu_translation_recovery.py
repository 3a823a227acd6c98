"""TranslationRecovery on the device against the numpy restatement (tests/translation_recovery_restatement.py) on identical inputs:
the two internal factor kinds' Jacobians to 1e-12 relative, the reference's known answers at its own tolerances, a noisy scene's
Levenberg-Marquardt trajectory at the project's parity bound of 1e-6 relative, merged nodes, between-translations, initial values and
seeds, and a complete graph whose elimination is one dense front of POINT3 columns."""
import ctypes as ct

import numpy as np
import pytest

import smart_restatement as sr
import translation_recovery_cases as c
import translation_recovery_restatement as trr
from gtsam_personal_amd import LevenbergMarquardtParams, TranslationRecovery, Values, _lib
from gtsam_personal_amd.translation_recovery import TranslationRecoverySession
from test_translation_recovery_reference import to_measurements

pytestmark = pytest.mark.gpu


def session(rel, scale=1.0, betweens=(), initial=None, ordering=None, seed=None):
    s = TranslationRecoverySession(device=0)
    if seed is not None:
        s.seed(seed)
    s.add_directions(to_measurements(rel))
    s.add_betweens(to_measurements(betweens))
    iv = None
    if initial is not None:
        iv = Values()
        for k, v in initial.items():
            iv.insert_point3(k, v)
    s.finalize(scale, iv, ordering)
    return s


def jacobians(s):
    """every whitened [A1 (A2) b] of the inner handle's linearization at its current values, by graph index, as (rows, cols) arrays"""
    lib, h, nf = s.lib, s.handle(), s.num_factors()
    assert lib.lmgpu_linearize(h) == _lib.LMGPU_OK
    n = ct.c_int32()
    gi, rows, cols, offs = np.zeros(nf, np.int32), np.zeros(nf, np.int32), np.zeros(nf, np.int32), np.zeros(nf + 1, np.int64)
    ip, lp = (lambda a: a.ctypes.data_as(_lib._I)), (lambda a: a.ctypes.data_as(ct.POINTER(ct.c_int64)))
    assert lib.lmgpu_get_jacobians(h, ct.byref(n), ip(gi), ip(rows), ip(cols), lp(offs), None) == _lib.LMGPU_OK and n.value == nf
    out = np.zeros(int(offs[nf]))
    assert lib.lmgpu_get_jacobians(h, ct.byref(n), ip(gi), ip(rows), ip(cols), lp(offs), out.ctypes.data_as(_lib._D)) == _lib.LMGPU_OK
    return {int(gi[i]): out[offs[i]:offs[i + 1]].reshape(cols[i], rows[i]).T for i in range(nf)}


# ---------------------------------------------------------------- (a) Jacobians
def _jacobian_scene(n):
    """n + 1 nodes on a path whose hops grow from 1e-3 to 1e3; every hop carries four direction edges and four betweens, one per noise group
    (unit, diagonal, full Gaussian, Huber over diagonal): eight buckets of n factors each.  Measured directions are unrelated unit vectors,
    so whitened errors lie on both sides of the Huber constant."""
    rng = np.random.RandomState(100 + n)
    hops = np.logspace(-3, 3, n) if n > 1 else np.array([1e-3])
    pos = {0: rng.uniform(-1, 1, 3)}
    for i in range(n):
        d = rng.normal(size=3)
        pos[i + 1] = pos[i] + hops[i] * d / np.linalg.norm(d)
    G = rng.uniform(-1, 1, (3, 3)) + 2 * np.eye(3)
    groups = [None, trr.Noise.diagonal([0.5, 1.5, 0.8]), trr.Noise(G), trr.Noise.diagonal([0.7, 0.9, 1.1], huber_k=1.345)]
    rel, bt = [], []
    for g in groups:
        for i in range(n):
            z = rng.normal(size=3)
            rel.append((i, i + 1, z / np.linalg.norm(z), g))
            bt.append((i, i + 1, (pos[i + 1] - pos[i]) * (1 + rng.uniform(-0.5, 0.5, 3)) + 0.3 * rng.uniform(-1, 1, 3), g))
    return rel, bt, pos


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_jacobians_of_both_internal_types(n):
    rel, bt, pos = _jacobian_scene(n)
    s = session(rel, 1.0, bt, pos)
    P = trr.build(rel, 1.0, bt, pos)
    assert s.num_factors() == len(P["factors"]) == 8 * n + 1
    got = jacobians(s)
    worst, above, below = 0.0, 0, 0
    for gi, f in enumerate(P["factors"]):
        want = f.jacobian(P["initial"])
        assert got[gi].shape == want.shape
        err = np.abs(got[gi] - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err <= 1e-12, (n, gi, type(f).__name__, err)
        if f.noise.huber_k is not None:
            d = np.linalg.norm(f.noise.R @ f.evaluate(P["initial"])[0])
            above, below = above + (d > f.noise.huber_k), below + (d <= f.noise.huber_k)
    print("n", n, "worst relative Jacobian error", worst, "Huber above / below k", above, below)
    assert n == 1 or (above > 0 and below > 0)
    e = ct.c_double()
    assert s.lib.lmgpu_error(s.handle(), ct.byref(e)) == _lib.LMGPU_OK
    want_e = trr.Graph(P["factors"], list(P["initial"])).error(P["initial"])
    assert abs(e.value - want_e) <= 1e-12 * want_e
    s.close()


# ---------------------------------------------------------------- (b) known answers
@pytest.mark.parametrize("name", list(c.known_answers()))
def test_known_answers(name):
    sc = c.known_answers()[name]
    res = TranslationRecovery().run(to_measurements(sc["rel"]), sc["scale"], to_measurements(sc["betweens"]))
    assert res.keys() == sorted(sc["expected"])
    for k, (want, tol) in sc["expected"].items():
        print(name, k, np.abs(res.at(k) - want).max(), tol)
        assert np.abs(res.at(k) - want).max() <= tol, (name, k)


# ---------------------------------------------------------------- (c) noisy scene
def test_noisy_scene_trajectory():
    """error and lambda after every iteration to 1e-6 relative, the positions after the last of them to 1e-6 of the scene's extent.  The run
    is deliberately truncated at NOISY_MAX_ITERATIONS, the iterations whose decisions keep their margin (see
    test_noisy_scene_decisions_have_margin); the run to convergence is test_complete_graph_dense_root, whose decisions, convergence tests
    included, have theirs (test_complete_graph_decisions_have_margin)."""
    rel, init, pos = c.noisy_scene()
    P = trr.build(rel, 1.0, [], init)
    p = sr.LMParams()
    p.maxIterations = c.NOISY_MAX_ITERATIONS
    lm = sr.LM(trr.Graph(P["factors"], list(P["initial"])), P["initial"], p)
    e0 = lm.error
    hist = lm.optimize()
    s = session(rel, 1.0, [], init)
    lib, h = s.lib, s.handle()
    dp = LevenbergMarquardtParams()
    dp.maxIterations = c.NOISY_MAX_ITERATIONS
    cp, st = dp._c(), _lib.lmgpu_lm_state()
    assert lib.lmgpu_lm_init(h, ct.byref(cp), ct.byref(st)) == _lib.LMGPU_OK
    assert abs(st.error - e0) <= 1e-9 * e0
    for it, (err, lam) in enumerate(hist):
        assert lib.lmgpu_iterate(h, ct.byref(cp), ct.byref(st)) == _lib.LMGPU_OK
        print(it, st.error, err, st.lambda_, lam)
        assert abs(st.error - err) <= 1e-6 * err, it
        assert abs(st.lambda_ - lam) <= 1e-6 * lam, it
    assert st.iterations == lm.iterations
    # the same through run(), which starts again from the initial values
    state = s.run(dp)
    assert state.iterations == lm.iterations and abs(state.error - hist[-1][0]) <= 1e-6 * hist[-1][0]
    got = s.get()
    extent = np.ptp(np.array(list(pos.values())), axis=0).max()
    worst = max(np.abs(got.at(k) - lm.values[k]).max() for k in lm.values)
    print("worst position difference", worst, "extent", extent)
    assert worst <= 1e-6 * extent
    s.close()


# ---------------------------------------------------------------- (d) merged nodes
def test_merged_nodes_equal_their_representative_bitwise():
    sc = c.known_answers()["FourPosesIncludingZeroTranslation"]
    # one more node, 7, at node 3's place: two sets, {1, 2} and {3, 7}
    rel = sc["rel"] + [(3, 7, np.zeros(3), trr.Noise.isotropic(0.01))]
    s = session(rel, sc["scale"])
    keys, rep = s.keys()
    assert dict(zip(keys, rep)) == {0: 0, 1: 1, 2: 1, 3: 3, 7: 3}
    s.run()
    got = s.get()
    assert np.array_equal(got.at(2), got.at(1)) and np.array_equal(got.at(7), got.at(3))
    want, _, _ = trr.run(rel, sc["scale"], gen=trr.MT19937(42))
    for k in keys:
        assert np.abs(got.at(k) - want[k]).max() <= 1e-8, k
    s.close()


# ---------------------------------------------------------------- (e) between-translations
def test_between_translations():
    """a node reached only by a between (the reference's NodeWithBetweenFactorAndNoMeasurements); and between-translations alone, for which
    the reference's addPrior adds nothing (TranslationRecovery.cpp:125-126): an empty graph, the result is the initial values"""
    sc = c.known_answers()["NodeWithBetweenFactorAndNoMeasurements"]
    s = session(sc["rel"], sc["scale"], sc["betweens"])
    assert s.num_factors() == 3 + 1 + 2 and s.slots() == [0, 1, 3, 4]
    s.run()
    got = s.get()
    want, _, _ = trr.run(sc["rel"], sc["scale"], sc["betweens"], gen=trr.MT19937(42))
    for k in (0, 1, 3, 4):
        assert np.abs(got.at(k) - want[k]).max() <= 1e-6 * 3, k
        assert np.abs(got.at(k) - sc["expected"][k][0]).max() <= 1e-4, k
    s.close()
    bt = [(0, 1, np.array([1.0, 0, 0]), None), (1, 5, np.array([0.0, 2, 0]), trr.Noise.isotropic(0.1))]
    s = session([], 1.0, bt)
    st = s.run()
    assert st.iterations == 0 and s.handle() is None
    want, lm, _ = trr.run([], 1.0, bt, gen=trr.MT19937(42))
    assert lm is None and all(np.array_equal(s.get().at(k), want[k]) for k in (0, 1, 5))
    s.close()


# ---------------------------------------------------------------- (f) initial values and seed
def test_initial_values_and_seed():
    sc = c.known_answers()["ThreePoseTest"]
    rel = to_measurements(sc["rel"])
    # explicit initial values are honoured: with maxIterations = 0 the result IS the initial values
    p0 = LevenbergMarquardtParams()
    p0.maxIterations = 0
    iv = Values()
    for k, v in {0: [0.1, 0.2, 0.3], 1: [2.5, 0.1, -0.1], 3: [1.0, -2.0, 0.5]}.items():
        iv.insert_point3(k, v)
    r0 = TranslationRecovery(p0).run(rel, 3.0, initialValues=iv)
    assert all(np.array_equal(r0.at(k), iv.at(k)) for k in (0, 1, 3))
    a, b = TranslationRecovery(), TranslationRecovery()
    ra, rb = a.run(rel, 3.0), b.run(rel, 3.0)
    assert all(np.array_equal(ra.at(k), rb.at(k)) for k in (0, 1, 3))  # the same seed: bitwise
    t7 = TranslationRecovery()
    t7.seed(7)
    r7 = t7.run(rel, 3.0)
    assert any(not np.array_equal(ra.at(k), r7.at(k)) for k in (0, 1, 3))  # another start, another rounding of the same optimum
    for k, (want, tol) in sc["expected"].items():
        assert np.abs(r7.at(k) - want).max() <= tol
    i42 = TranslationRecovery(p0).run(rel, 3.0)
    t = TranslationRecovery(p0)
    t.seed(7)
    i7 = t.run(rel, 3.0)
    w42, w7 = trr.build(sc["rel"], gen=trr.MT19937(42))["initial"], trr.build(sc["rel"], gen=trr.MT19937(7))["initial"]
    assert all(np.array_equal(i42.at(k), w42[k]) and np.array_equal(i7.at(k), w7[k]) for k in (0, 1, 3))


# ---------------------------------------------------------------- (g) dense root
def test_complete_graph_dense_root():
    """60 nodes, every pair: one front of 180 columns, above the LDS front limit, so the dense-front kernels eliminate POINT3 columns only"""
    rel, init, pos = c.complete_graph()
    s = session(rel, 1.0, [], init)
    lib, h = s.lib, s.handle()
    info = (ct.c_int32 * 8)()
    nf = lib.lmgpu_num_fronts(h)
    assert lib.lmgpu_front_info(h, nf - 1, info) == _lib.LMGPU_OK
    assert info[2] == 180 and info[3] == 181 and info[5] == 1, list(info)
    st = s.run()
    want, lm, hist = trr.run(rel, 1.0, [], init)
    assert st.iterations == lm.iterations
    got = s.get()
    extent = np.ptp(np.array(list(pos.values())), axis=0).max()
    worst = max(np.abs(got.at(k) - want[k]).max() for k in want)
    print("iterations", st.iterations, "worst position difference", worst, "extent", extent)
    assert worst <= 1e-6 * extent
    s.close()
