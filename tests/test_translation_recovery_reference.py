"""CPU tests of TranslationRecovery: the numpy restatement (tests/translation_recovery_restatement.py) against the known answers of the
reference's tests/testTranslationRecovery.cpp at that file's tolerances, its generator and Jacobians, the margins of every
Levenberg-Marquardt decision the GPU tests' noisy scene takes, the session's host logic on a device-less session (merged sets, priors, initial
values, ordering, refusals), and the C ABI's surface.  No GPU."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import smart_restatement as sr
import translation_recovery_cases as c
import translation_recovery_restatement as trr
from gtsam_personal_amd import BinaryMeasurement, LevenbergMarquardtParams, PCGSolverParameters, TranslationRecovery, Values, _lib, graph as G, noiseModel
from gtsam_personal_amd.translation_recovery import CONSTRAINED_MESSAGE, Constrained, TranslationRecoverySession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_U64 = ct.POINTER(ct.c_uint64)


def to_model(noise):
    """a restatement Noise as the package's noise model (isotropic / diagonal / full Gaussian, Huber on top)"""
    if noise is None:
        return None
    d = np.diag(noise.R)
    if np.count_nonzero(noise.R - np.diag(d)):
        m = noiseModel.Gaussian.SqrtInformation(noise.R)
    elif (d == d[0]).all():
        m = noiseModel.Isotropic.Sigma(3, 1.0 / d[0])
    else:
        m = noiseModel.Diagonal.Sigmas(1.0 / d)
    return m if noise.huber_k is None else noiseModel.Robust.Create(noiseModel.mEstimator.Huber.Create(noise.huber_k), m)


def to_measurements(edges):
    return [BinaryMeasurement(a, b, z, to_model(n)) for a, b, z, n in edges]


# ---------------------------------------------------------------- the generator
def test_mt19937_is_numpys():
    """the first draws of the seed-42 generator against numpy's legacy RandomState(42), whose 32-bit output over the full range is the raw
    stream of init_genrand(42)"""
    g = trr.MT19937(42)
    mine = np.array([g() for _ in range(2000)], dtype=np.uint64)
    ref = np.random.RandomState(42).randint(0, 2 ** 32, size=2000, dtype=np.uint64)
    assert mine[0] == 1608637542 and np.array_equal(mine, ref)
    g.seed(7)
    assert g() == int(np.random.RandomState(7).randint(0, 2 ** 32, dtype=np.uint64))


def test_uniform_is_the_written_out_formula():
    raw = np.random.RandomState(42).randint(0, 2 ** 32, size=6, dtype=np.uint64)
    g = trr.MT19937(42)
    for i in range(3):
        x1, x2 = int(raw[2 * i]), int(raw[2 * i + 1])
        exact = 2 * ((x1 + x2 * 2 ** 32) / 2 ** 64) - 1  # Python rounds the integer ratio once
        u = trr.uniform(g)
        assert -1 <= u < 1 and abs(u - exact) <= 2 ** -52


# ---------------------------------------------------------------- factors
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_jacobians_by_central_differences(scale):
    rng = np.random.RandomState(11)
    noise = trr.Noise(rng.uniform(-1, 1, (3, 3)) + 3 * np.eye(3))
    for cls in (trr.TranslationFactor, trr.BetweenPoint3):
        f = cls((0, 1), rng.uniform(-1, 1, 3), noise)
        v = {0: rng.uniform(-1, 1, 3), 1: rng.uniform(-1, 1, 3)}
        v[1] = v[0] + scale * (v[1] - v[0]) / np.linalg.norm(v[1] - v[0])
        J = f.jacobian(v)
        h = 1e-6 * scale
        for k in (0, 1):
            for j in range(3):
                vp, vm = {a: b.copy() for a, b in v.items()}, {a: b.copy() for a, b in v.items()}
                vp[k][j] += h
                vm[k][j] -= h
                num = (noise.R @ f.evaluate(vp)[0] - noise.R @ f.evaluate(vm)[0]) / (2 * h)
                assert np.abs(num - J[:, 3 * k + j]).max() <= 1e-6 * max(1.0, np.abs(J).max()), (cls.__name__, k, j)
        assert np.allclose(J[:, 6], -(noise.R @ f.evaluate(v)[0]), rtol=0, atol=0)


def test_translation_jacobian_is_the_references_expression():
    """H2 = H, H1 = -H with H of Point3.cpp:52-62; the rows of H annihilate the direction itself"""
    v = {0: np.array([0.3, -0.2, 0.9]), 1: np.array([1.1, 0.4, -0.5])}
    e, (H1, H2) = trr.TranslationFactor((0, 1), [0, 0, 1], None).evaluate(v)
    d = v[1] - v[0]
    assert np.array_equal(H1, -H2) and np.abs(H2 @ d).max() < 1e-15
    assert np.allclose(H2, (np.eye(3) - np.outer(d, d) / (d @ d)) / np.linalg.norm(d), rtol=1e-14)
    assert np.allclose(e, d / np.linalg.norm(d) - [0, 0, 1])


# ---------------------------------------------------------------- known answers
BUILD_GRAPH_SIZE = {"BAL": 3, "TwoPoseTest": 1, "ThreePoseTest": 3}  # EXPECT_LONGS_EQUAL(n, graph.size()) where the reference has one


@pytest.mark.parametrize("name", list(c.known_answers()))
def test_known_answers(name):
    """tests/testTranslationRecovery.cpp, each from a fresh seed-42 generator, at that test's tolerance per key"""
    s = c.known_answers()[name]
    res, lm, _ = trr.run(s["rel"], s["scale"], s["betweens"], gen=trr.MT19937(42))
    assert sorted(res) == sorted(s["expected"])
    for k, (want, tol) in s["expected"].items():
        print(name, k, np.abs(res[k] - want).max(), tol)
        assert np.abs(res[k] - want).max() <= tol, (name, k)
    if name in BUILD_GRAPH_SIZE:
        assert trr.build(s["rel"], s["scale"], s["betweens"])["n_dir"] == BUILD_GRAPH_SIZE[name]


def test_zero_direction_sets():
    s = c.known_answers()["FourPosesIncludingZeroTranslation"]
    P = trr.build(s["rel"], s["scale"])
    assert P["rep"] == {0: 0, 1: 1, 2: 1, 3: 3} and P["n_dir"] == 3 and list(P["initial"]) == [0, 1, 3]
    assert len(P["factors"]) == 5  # three directions, the origin prior, the scale prior
    z = c.known_answers()["ThreePosesWithZeroTranslation"]
    P = trr.build(z["rel"], z["scale"])
    assert P["rep"] == {0: 0, 1: 0, 2: 0} and not P["factors"] and list(P["initial"]) == [0] and not P["initial"][0].any()


@pytest.mark.parametrize("name", ["ThreePosesWithOneHardConstraint", "NodeWithBetweenFactorAndNoMeasurements"])
def test_constrained_models_are_refused(name):
    """the two cases of the reference's test file whose between-translations carry noiseModel::Constrained::All(3, 1e2)"""
    rel = to_measurements(trr.simulate(c.P3, [(0, 1), (0, 3), (1, 3)]))
    bt = [BinaryMeasurement(0, 1, [2, 0, 0], Constrained.All(3, 1e2))]
    if name.startswith("Node"):
        bt.append(BinaryMeasurement(0, 4, [1, 2, 1]))
    with pytest.raises(NotImplementedError) as ei:
        TranslationRecovery(device=-1).run(rel, 0.0, bt)
    assert str(ei.value) == CONSTRAINED_MESSAGE
    with pytest.raises(NotImplementedError) as ei2:
        noiseModel.Diagonal.Sigmas([0.0, 1.0, 1.0])
    assert str(ei2.value) == CONSTRAINED_MESSAGE  # the wording of graph.py


def test_other_refusals_each_with_one_message():
    with pytest.raises(NotImplementedError, match="1-D variable type"):
        TranslationRecovery(use_bilinear_translation_factor=True)
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        TranslationRecovery(world_size=2)
    p = LevenbergMarquardtParams()
    p.linearSolverType, p.iterativeParams = "ITERATIVE", PCGSolverParameters()
    with pytest.raises(NotImplementedError, match="direct solver"):
        TranslationRecovery(p)
    lib = _lib.load()
    tr = ct.c_void_p()
    cfg = _lib.lmgpu_config(-1, 0, 2, 0)
    assert lib.lmgpu_translation_recovery_create(ct.byref(cfg), ct.byref(tr)) == _lib.LMGPU_INVALID


# ---------------------------------------------------------------- noisy scene
def test_noisy_scene_decisions_have_margin():
    """the GPU file compares error and lambda after every iteration of this run: every decision the loop takes lies at least 1e-3 (relative
    to its scale) from its bound.  The trajectory is DELIBERATELY TRUNCATED at NOISY_MAX_ITERATIONS: on a problem whose optimum keeps a
    residual, the linearized cost change l0 - l1 shrinks against the linear error l0 as the iterates converge (1.7e-3, 3.5e-5, 7e-7 ... of
    l0 from the fourth iteration on in the zero-rejection variants of this scene), so in the scale these decisions are recorded in no
    converging run of such a problem keeps 1e-3; the loop therefore ends on maxIterations with the convergence test far from met.  The
    run to convergence whose every decision, the convergence test included, has margin is the complete graph's, below."""
    rel, init, _ = c.noisy_scene()
    assert len(init) == 40 and len(rel) == 120
    P = trr.build(rel, 1.0, [], init)
    p = sr.LMParams()
    p.maxIterations = c.NOISY_MAX_ITERATIONS
    lm = sr.LM(trr.Graph(P["factors"], list(P["initial"])), P["initial"], p)
    hist = lm.optimize()
    assert lm.iterations == c.NOISY_MAX_ITERATIONS == len(hist) and lm.inner > lm.iterations  # some trial steps are rejected
    worst = min(abs(d[1] - d[2]) / d[3] for d in lm.ctl)
    print("smallest decision margin", worst, "errors", [h[0] for h in hist])
    for d in lm.ctl:
        assert abs(d[1] - d[2]) >= 1e-3 * d[3], d
    assert 1.0 < hist[-1][0] < 100.0  # an optimum of order one to ten, not a zero-residual problem
    for a, b in zip([None] + [h[0] for h in hist][:-1], [h[0] for h in hist]):
        if a is not None:
            assert (a - b) / a > 1e-3 and a - b > 1e-3  # checkConvergence (1e-5 / 1e-5) is clear as well


def test_complete_graph_decisions_have_margin():
    """the GPU file runs this scene to convergence: every decision of the loop AND both convergence tests of every iteration
    (relative and absolute error decrease against 1e-5, NonlinearOptimizer.cpp:182-231) lie at least 1e-3 of their scale from their bound"""
    rel, init, _ = c.complete_graph()
    P = trr.build(rel, 1.0, [], init)
    lm = sr.LM(trr.Graph(P["factors"], list(P["initial"])), P["initial"])
    errs = [lm.error] + [h[0] for h in lm.optimize()]
    assert 3 < lm.iterations < 100 and errs[-1] < 1e-15  # converged, not stopped by maxIterations; exact directions: no residual
    for d in lm.ctl:
        assert abs(d[1] - d[2]) >= 1e-3 * d[3], d
    p = sr.LMParams()
    for it, (a, b) in enumerate(zip(errs[:-1], errs[1:])):
        for value, bound in (((a - b) / a, p.relativeErrorTol), (a - b, p.absoluteErrorTol)):
            assert abs(value - bound) >= 1e-3 * max(abs(value), bound), (it, value, bound)
        assert b > p.errorTol  # errorTol = 0 never ends the loop
        assert sr.check_convergence(p, a, b) == (it == len(errs) - 2)


# ---------------------------------------------------------------- the session's host logic (no device)
def _session(rel, scale=1.0, betweens=(), initial=None, ordering=None, seed=None):
    s = TranslationRecoverySession(device=-1)
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


@pytest.mark.parametrize("name", list(c.known_answers()))
def test_session_host_logic_matches_restatement(name):
    """keys, representatives, factor count and the seed-42 initial values, bitwise"""
    sc = c.known_answers()[name]
    P = trr.build(sc["rel"], sc["scale"], sc["betweens"], gen=trr.MT19937(42))
    s = _session(sc["rel"], sc["scale"], sc["betweens"])
    keys, rep = s.keys()
    assert keys == P["keys"] and rep == [P["rep"][k] for k in keys]
    assert s.slots() == list(P["initial"]) and s.num_factors() == len(P["factors"])
    got = s.initial()
    for k, v in P["initial"].items():
        assert np.array_equal(got[k], v), (name, k)
    assert (s.handle() is None) == (not P["factors"])
    st = _lib.lmgpu_lm_state()
    cp = LevenbergMarquardtParams()._c()
    assert s.lib.lmgpu_translation_recovery_run(s._tr, ct.byref(cp), ct.byref(st)) == _lib.LMGPU_HIP_ERROR  # no device
    s.close()


def test_session_seed_initial_values_and_ordering():
    rel = c.known_answers()["FourPosesIncludingZeroTranslation"]["rel"]
    a, b, s7 = _session(rel), _session(rel), _session(rel, seed=7)
    assert all(np.array_equal(a.initial()[k], b.initial()[k]) for k in a.slots())
    assert any(not np.array_equal(a.initial()[k], s7.initial()[k]) for k in a.slots())
    want7 = trr.build(rel, gen=trr.MT19937(7))["initial"]
    assert all(np.array_equal(s7.initial()[k], want7[k]) for k in want7)
    # given values are taken, the others drawn in order: node 1 given -> nodes 0 and 3 get the first six coordinates of the stream
    g = _session(rel, initial={1: [9.0, 8.0, 7.0], 2: [1.0, 1.0, 1.0]})
    w = trr.build(rel, initial_values={1: [9.0, 8.0, 7.0]}, gen=trr.MT19937(42))["initial"]
    assert np.array_equal(g.initial()[1], [9, 8, 7]) and all(np.array_equal(g.initial()[k], w[k]) for k in w)
    # the ordering ranges over the original keys; the merged-away node 2 is ignored
    o = _session(rel, ordering=[3, 2, 1, 0])
    assert o.slots() == [3, 1, 0] and all(np.array_equal(o.initial()[k], a.initial()[k]) for k in a.slots())
    lib = a.lib
    for bad, msg in (([3, 1], "not in the ordering"), ([3, 1, 0, 3], "duplicate key")):
        arr = np.array(bad, dtype=np.uint64)
        assert lib.lmgpu_translation_recovery_finalize(a._tr, 1.0, 0, None, None, len(arr), arr.ctypes.data_as(_U64)) == _lib.LMGPU_INVALID
        assert msg in lib.lmgpu_translation_recovery_last_error(a._tr).decode()
        assert a.slots() == [0, 1, 3]  # a refusal changes nothing
    for s in (a, b, s7, g, o):
        s.close()


def test_between_only_and_dangling_merged_set():
    """without a direction edge addPrior returns before it adds anything (TranslationRecovery.cpp:125-126): the graph is empty and the
    betweens only name the nodes that get initial values; a merged set whose every edge was dropped is refused (the reference throws)"""
    bt = [(0, 1, np.array([1.0, 0, 0]), None), (1, 5, np.array([0.0, 2, 0]), trr.Noise.isotropic(0.1))]
    s = _session([], betweens=bt)
    P = trr.build([], betweens=bt, gen=trr.MT19937(42))
    assert s.num_factors() == 0 == len(P["factors"]) and s.handle() is None and s.slots() == [0, 1, 5] == list(P["initial"])
    assert all(np.array_equal(s.initial()[k], P["initial"][k]) for k in P["initial"])
    s.close()
    rel = [(0, 1, np.array([1.0, 0, 0]), None), (4, 5, np.zeros(3), None)]
    t = TranslationRecoverySession(device=-1)
    t.add_directions(to_measurements(rel))
    with pytest.raises(_lib.LmgpuError, match="no other edge left"):
        t.finalize()
    t.close()


def test_near_zero_directions_merge_within_unit3_tolerance():
    """measured().equals(Unit3(0, 0, 0)) has Unit3::equals' default tolerance of 1e-9 per component"""
    for z, merged in (([5e-10, -1e-9, 0.0], True), ([2e-9, 0.0, 0.0], False)):
        rel = [(0, 1, np.array([1.0, 0, 0]), None), (1, 2, np.array(z), None), (2, 3, np.array([0.0, 1, 0]), None)]
        s = _session(rel)
        keys, rep = s.keys()
        assert dict(zip(keys, rep))[2] == (1 if merged else 2)
        assert trr.build(rel)["rep"][2] == (1 if merged else 2)
        s.close()


def test_key_only_in_dropped_betweens_has_its_own_message():
    rel = [(0, 1, np.array([1.0, 0, 0]), None)]
    t = TranslationRecoverySession(device=-1)
    t.add_directions(to_measurements(rel))
    t.add_betweens(to_measurements([(9, 9, np.array([0.0, 0, 0]), None)]))
    with pytest.raises(_lib.LmgpuError, match="two ends are the same node"):
        t.finalize()
    t.close()


def test_generator_moves_only_on_a_successful_finalize():
    rel = c.known_answers()["ThreePoseTest"]["rel"]
    s = _session(rel)
    first = s.initial()
    bad = np.array([3, 1], dtype=np.uint64)
    assert s.lib.lmgpu_translation_recovery_finalize(s._tr, 1.0, 0, None, None, 2, bad.ctypes.data_as(_U64)) == _lib.LMGPU_INVALID
    s.finalize()  # the second successful finalize goes on in the stream: nine draws further
    g = trr.MT19937(42)
    a, b = trr.build(rel, gen=g)["initial"], trr.build(rel, gen=g)["initial"]
    assert all(np.array_equal(first[k], a[k]) and np.array_equal(s.initial()[k], b[k]) for k in a)
    s.close()


# ---------------------------------------------------------------- ABI surface
TR_SYMBOLS = ("create", "destroy", "last_error", "seed", "set_prior_sigma", "add_directions", "add_betweens", "finalize", "num_keys", "num_factors",
              "get_keys", "get_slots", "get_initial", "handle", "run", "get")
MFAS_SYMBOLS = ("lmgpu_mfas_outlier_weights", "lmgpu_mfas_lds_node_capacity", "lmgpu_mfas_last_error")


def test_symbols_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ct.CDLL(_lib.LIB_PATH)
    names = ["lmgpu_translation_recovery_" + n for n in TR_SYMBOLS] + list(MFAS_SYMBOLS)
    assert sorted(n for n in _lib.SYMBOLS if "translation_recovery" in n or "mfas" in n) == sorted(names)
    for name in names:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in integ, name
    for phrase in ("OUTSIDE THE CONTRACT", "TIE RULE", "LOWEST KEY", "given twice"):
        assert phrase in header, phrase


def test_public_enums_are_unchanged_and_the_boundary_refuses_the_internal_rows():
    header = open(os.path.join(ROOT, "include", "lmgpu.h")).read()
    val = lambda name: int(re.search(r"\b%s = (\d+)" % name, header).group(1))  # noqa: E731
    assert val("LMGPU_NUM_FACTOR_TYPES") == 14 == len(G.FACTOR_ROWS) and val("LMGPU_NUM_VAR_TYPES") == 7 == len(G.VAR_DIM)
    lib = _lib.load()
    h = ct.c_void_p()
    cfg = _lib.lmgpu_config(-1, 0, 1, 0)
    assert lib.lmgpu_create(ct.byref(cfg), ct.byref(h)) == _lib.LMGPU_OK
    keys = np.array([0, 1], dtype=np.uint64)
    types = np.array([G.POINT3, G.POINT3], dtype=np.int32)
    assert lib.lmgpu_set_variables(h, 2, keys.ctypes.data_as(_U64), types.ctypes.data_as(_lib._I)) == _lib.LMGPU_OK
    gi, slots, meas = np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([1.0, 0, 0])
    for t in (14, 15, 16, 17):
        assert lib.lmgpu_add_factor_bucket(h, t, 1, gi.ctypes.data_as(_lib._I), slots.ctypes.data_as(_lib._I), meas.ctypes.data_as(_lib._D), 0,
                                           None) == _lib.LMGPU_INVALID
        assert lib.lmgpu_last_error(h).decode() == ("lmgpu_add_factor_bucket_robust: refused (h->finalized || type < 0 || type >= "
                                                    "LMGPU_NUM_FACTOR_TYPES || n < 0 || h->plan.n_vars == 0)")
        rec = (ct.c_int32 * 6)()
        assert lib.lmgpu_selftest_factor_type(t, rec) == _lib.LMGPU_INVALID
    lib.lmgpu_destroy(h)
    ip = ct.c_void_p()
    cfg0 = _lib.lmgpu_config(0, 0, 1, 0)
    assert lib.lmgpu_init_pose3_create(ct.byref(cfg0), ct.byref(ip)) == _lib.LMGPU_OK  # creating the object touches no device
    for t in (15, 16):
        assert lib.lmgpu_init_pose3_add_factors(ip, t, 0, None, None, None, 0, None) == _lib.LMGPU_INVALID
    lib.lmgpu_init_pose3_destroy(ip)
