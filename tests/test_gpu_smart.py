"""Smart projection factors on the device against the numpy restatement (tests/smart_restatement.py) on identical inputs and in the
reference's order of calls.  Bound: the project's parity bound, 1e-6 relative -- errors and linear errors relative to the initial error of
the problem (the magnitude of the terms the sums are made of), steps / points / values relative to their norm, Hessian taps relative to
their largest entry.  Statuses, lambda sequences, iteration counts and retriangulation counts must be equal.  Each test prints the margin
it reached."""
import numpy as np
import pytest

import smart_cases as sc
import smart_restatement as sr
import triangulation_restatement as tr

pytestmark = pytest.mark.gpu

REL = 1e-6


def close(what, got, want, scale=None):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    s = float(scale if scale is not None else max(np.max(np.abs(want)), 1e-300))
    err = float(np.max(np.abs(got - want))) / s
    print(f"  {what}: relative error {err:.3g} (bound {REL:g})")
    assert err <= REL, (what, err)


def device(scene, gn=False, params=None):
    import gtsam_personal_amd as gpa
    g, v, order, objs = sc.package(scene)
    cls = gpa.GaussNewtonOptimizer if gn else gpa.LevenbergMarquardtOptimizer
    return cls(g, v, order, params), objs


def packed(opt, dct):
    return np.concatenate([dct[k] for k in opt.ordering])


def values_of(opt):
    v = opt.values()
    return {k: v.at(k).copy() for k in opt.ordering}


# ---------------------------------------------------------------- the scenes compared with the restatement, with the calls made on them
CACHE_THR = 1e-3
EDGE_COUNTS = (1, 3, 4, 5, 63, 64, 65)
EDGE_DEGREES = (2, 3, 9, 10, 16, 17)


def edge_scene(n):
    return sc.ring_scene([EDGE_DEGREES[i % len(EDGE_DEGREES)] for i in range(n)], seed=100 + n)


def wide_scene():
    return sc.ring_scene([22, 23, 2], seed=7)  # point fronts of 6 * 22 + 3 + 1 = 136 and 142 columns: either side of the LDS limit 139


def bins_scene():
    """one parameter group, 100 factors given with their observation counts interleaved (a real permutation in the launch order): the bin of
    2 observations holds 34 lanes, the bin of 3 .. 4 holds 66 = two workgroups of 64 with a tail of two lanes"""
    return sc.ring_scene([2, 3, 4] * 32 + [2, 4, 2, 3], seed=9)


def lm_scene(perturbed=True):
    return sc.three_poses_scene(perturbed, params=sc.every_change())


def lm_params(**kw):
    """-> (the restatement's LMParams, the package's LevenbergMarquardtParams) with the same fields set"""
    import gtsam_personal_amd as gpa
    a, b = sr.LMParams(), gpa.LevenbergMarquardtParams()
    for k, v in kw.items():
        assert hasattr(a, k) and hasattr(b, k), k
        setattr(a, k, v)
        setattr(b, k, v)
    return a, b


# Levenberg-Marquardt runs with rejected trials, a fixed number of iterate() calls each:
#   "rejected": threshold 0, lambdaInitial 1e3 -- from the third iteration on every iteration evaluates a trial, rejects it, and accepts the next
#   "frozen":   threshold 2 (ten times above the largest pose change of the run, 0.102: the point of the first triangulation is used
#               throughout), minModelFidelity 0.9 -- mostly rejected trials, one accepted
LM_RUNS = {"rejected": (dict(lambdaInitial=1e3), 0.0, 6), "frozen": (dict(minModelFidelity=0.9), 2.0, 6)}


def lm_run_scene(name):
    return sc.three_poses_scene(params=sc.zero_on_degeneracy(retriangulationThreshold=LM_RUNS[name][1]))


def _steps_lm_run(name):
    def steps(g, v):
        lm = sr.LM(g, v, lm_params(**LM_RUNS[name][0])[0])
        for _ in range(LM_RUNS[name][2]):
            lm.iterate()
        return lm
    return steps


def cache_scene():
    return sc.three_poses_scene(params=sc.zero_on_degeneracy(retriangulationThreshold=CACHE_THR))


def moved(values, key, by):
    out = {k: p.copy() for k, p in values.items()}
    out[key][9] += by
    return out


def _steps_lm(g, v):
    lm = sr.LM(g, v)
    lm.optimize()
    return lm


def _steps_gn(g, v):
    g.error(v)
    sr.gn_step(g, v)


def _steps_cache(g, v):
    g.error(v)
    g.linearize(v)
    g.error(moved(v, sc.X3, 1e-4))
    g.error(moved(v, sc.X3, 1e-2))


def _steps_lm_once(g, v):
    lm = sr.LM(g, v)
    lm.iterate()
    return lm


def parity_scenes():
    out = [("factors", sc.factors_scene(), _steps_gn), ("three_poses", lm_scene(), _steps_lm),
           ("five_status", sc.five_status_scene(), _steps_lm_once), ("cache", cache_scene(), _steps_cache),
           ("wide", wide_scene(), _steps_gn), ("bins", bins_scene(), _steps_gn)]
    out += [(name, lm_run_scene(name), _steps_lm_run(name)) for name in LM_RUNS]
    out += [(f"edge{n}", edge_scene(n), _steps_gn) for n in EDGE_COUNTS]
    return out


# ---------------------------------------------------------------- 1
def test_factors_scene():
    scene = sc.factors_scene()
    g, v = sc.restatement(scene)
    e_ref = g.error(v)
    opt, objs = device(scene)
    close("error", opt.error(), e_ref, 1.0)
    opt.linearize()
    A_ref = g.smart()[0].hessian(v)
    pts, st = opt.smart_points()
    assert st.tolist() == [tr.VALID]
    close("point", pts[0], [0, 0, 10.0])
    close("point vs restatement", pts[0], g.smart()[0].point)
    A = opt.smart_hessian(0)
    close("tap vs restatement", A, A_ref, np.max(np.abs(A_ref)))
    close("tap vs A1 / A2", A, sc.factors_expected_information(), np.max(np.abs(A_ref)))
    assert objs[0].isValid() and np.allclose(objs[0].point().get(), [0, 0, 10.0], atol=1e-9)
    opt.close()


def same_smart_state(opt, g, lm, what):
    """after an iterate() on both sides: the last evaluation that counts re-triangulated the same factors and left the same statuses; and
    the accepted (or last evaluated) trial's cache is the one in force -- a linearization at the current values, which changes nothing
    on either side, finds every factor's poses in the cache"""
    st = opt.smart_stats()
    want = sum(f.retriangulated for f in g.smart())
    print(f"  {what}: retriangulations {st['retriangulations']} (restatement {want}), statuses {st['n_status']}")
    assert st["retriangulations"] == want, what
    assert st["n_status"] == [sum(f.status == k for f in g.smart()) for k in range(6)], what
    opt.linearize()
    g.linearize(lm.values)
    assert opt.smart_stats()["retriangulations"] == 0 == sum(f.retriangulated for f in g.smart()), what


# ---------------------------------------------------------------- 2
def test_three_poses_iteration_by_iteration():
    scene = lm_scene()
    g, v = sc.restatement(scene)
    lm = sr.LM(g, v)
    e0 = lm.error
    hist = lm.optimize()
    g0, v0 = sc.restatement(lm_scene(False))
    opt0, _ = device(lm_scene(False))
    close("error at the ground truth", opt0.error(), g0.error(v0), 1.0)
    assert abs(opt0.error()) <= 1e-9
    opt0.close()

    opt, objs = device(scene)
    close("initial error", opt.error(), e0)
    for i, (err, lam) in enumerate(hist):
        opt.iterate()
        close(f"iteration {i + 1} error", opt.error(), err, e0)
        assert opt.lambda_() == lam, (i, opt.lambda_(), lam)
    assert opt.iterations() == lm.iterations and opt.getInnerIterations() == lm.inner
    same_smart_state(opt, g, lm, "after the last iteration")
    got = values_of(opt)
    close("x3 vs pose_above (1e-6 absolute, :332)", got[sc.X3], sc.POSE_ABOVE, 1.0)
    close("values vs restatement", packed(opt, got), packed(opt, lm.values), 1.0)
    opt.close()

    opt, objs = device(scene)
    opt.optimize()
    assert opt.iterations() == lm.iterations
    close("optimize(): values", packed(opt, values_of(opt)), packed(opt, lm.values), 1.0)
    pts, st = opt.smart_points()
    assert st.tolist() == [f.status for f in g.smart()] == [tr.VALID] * 3
    for i, f in enumerate(g.smart()):
        close(f"point {i}", pts[i], f.point)
        assert objs[i].isValid()
        close(f"factor object {i} point()", objs[i].point().get(), f.point)
    opt.close()


@pytest.mark.parametrize("name", sorted(LM_RUNS))
def test_lm_with_rejected_trials(name):
    """the cache through tryLambda's speculative error evaluation: the counts and statuses after every iterate(), the errors and the
    lambda sequence over runs in which trials are evaluated and rejected"""
    kw, _, n_it = LM_RUNS[name]
    scene = lm_run_scene(name)
    g, v = sc.restatement(scene)
    pr, pd = lm_params(**kw)
    lm = sr.LM(g, v, pr)
    opt, _ = device(scene, params=pd)
    e0 = lm.error
    close("initial error", opt.error(), e0)
    assert opt.smart_stats()["retriangulations"] == 3
    rejected = 0
    for i in range(n_it):
        n0 = len(lm.trace)
        lm.iterate()
        opt.iterate()
        rejected += sum(1 for t in lm.trace[n0:] if t[3] is not None and not t[4])
        close(f"iterate {i + 1}: error", opt.error(), lm.error, e0)
        assert opt.lambda_() == lm.lam and opt.iterations() == lm.iterations and opt.getInnerIterations() == lm.inner, i
        same_smart_state(opt, g, lm, f"iterate {i + 1}")
    assert rejected >= 4 and lm.iterations >= 1  # both happen: trials evaluated and rejected, trials accepted
    close("values", packed(opt, values_of(opt)), packed(opt, lm.values), 1.0)
    pts, st = opt.smart_points()
    for i, f in enumerate(g.smart()):
        close(f"point {i}", pts[i], f.point)
    opt.close()


# ---------------------------------------------------------------- 3
def test_all_statuses_in_one_graph():
    scene = sc.five_status_scene()
    g, v = sc.restatement(scene)
    lm = sr.LM(g, v)
    opt, objs = device(scene)
    close("error", opt.error(), lm.error)
    valid_alone = g.smart()[0].error(v) + sum(f.error(v) for f in g.factors if isinstance(f, sr.Prior))
    close("error = the VALID factor's + priors", opt.error(), valid_alone)
    opt.linearize()
    H, gg, c = g.linearize(v)
    pts, st = opt.smart_points()
    assert tuple(st.tolist()) == sc.FIVE_STATUS == tuple(f.status for f in g.smart())
    assert np.isnan(pts[1:]).all()
    close("valid point", pts[0], g.smart()[0].point)
    for i in range(1, 6):
        assert not opt.smart_hessian(i).any(), i  # exactly zero
    A_ref = g.smart()[0].hessian_at_cache(v)
    close("tap of the valid factor", opt.smart_hessian(0), A_ref, np.max(np.abs(A_ref)))
    lam = 1e-5
    _, d, l0, l1 = opt.solve(lam)  # raises on LMGPU_INDETERMINATE
    x = sr.solve(H, gg, lam)
    close("LM step", d, x, np.max(np.abs(x)))
    close("lin_err0", l0, 0.5 * c, lm.error)
    close("lin_err1", l1, sr.lin_error(H, gg, c, x), lm.error)
    opt.close()
    opt, _ = device(scene)
    lm.iterate()
    opt.iterate()
    close("error after one LM iteration", opt.error(), lm.error, valid_alone)
    assert opt.lambda_() == lm.lam and opt.getInnerIterations() == lm.inner
    same_smart_state(opt, g, lm, "after one LM iteration")
    opt.close()


# ---------------------------------------------------------------- 4
def _set(opt, dct):
    import gtsam_personal_amd as gpa
    from gtsam_personal_amd import graph as G
    v = gpa.Values()
    for k, p in dct.items():
        v.insert(k, G.POSE3, p)
    opt.set_values(v)


def test_cache():
    scene = cache_scene()
    g, v = sc.restatement(scene)
    opt, _ = device(scene)
    g.error(v)
    assert opt.smart_stats()["retriangulations"] == 3  # the constructor's error evaluation
    opt.linearize()
    g.linearize(v)
    assert opt.smart_stats()["retriangulations"] == 0
    p0, s0 = opt.smart_points()
    # within the threshold: nothing moves
    near = moved(v, sc.X3, 1e-4)
    _set(opt, near)
    e = opt.graph_error()
    close("error within the threshold", e, g.error(near))
    p1, s1 = opt.smart_points()
    assert opt.smart_stats()["retriangulations"] == 0 and [f.retriangulated for f in g.smart()] == [False] * 3
    assert p1.tobytes() == p0.tobytes() and s1.tolist() == s0.tolist()
    # beyond it: re-triangulated
    far = moved(v, sc.X3, 1e-2)
    _set(opt, far)
    e = opt.graph_error()
    close("error beyond the threshold", e, g.error(far))
    p2, _ = opt.smart_points()
    assert opt.smart_stats()["retriangulations"] == 3 and [f.retriangulated for f in g.smart()] == [True] * 3
    assert p2.tobytes() != p0.tobytes()
    for i, f in enumerate(g.smart()):
        close(f"re-triangulated point {i}", p2[i], f.point)
    # unchanged poses: the cache holds; after smart_reset it is empty
    opt.graph_error()
    assert opt.smart_stats()["retriangulations"] == 0
    opt.smart_reset()
    opt.graph_error()
    assert opt.smart_stats()["retriangulations"] == 3
    p3, _ = opt.smart_points()
    assert p3.tobytes() == p2.tobytes()
    # save / restore move the values, not the cache
    opt.save_values()
    _set(opt, moved(far, sc.X3, 1e-4))
    opt.graph_error()
    assert opt.smart_stats()["retriangulations"] == 0
    opt.restore_values()
    opt.graph_error()
    assert opt.smart_stats()["retriangulations"] == 0
    assert opt.smart_points()[0].tobytes() == p2.tobytes()
    _set(opt, v)
    opt.graph_error()
    assert opt.smart_stats()["retriangulations"] == 3
    opt.restore_values()  # back at `far`, the cache is the one of `v`
    opt.graph_error()
    assert opt.smart_stats()["retriangulations"] == 3
    close("points after the restore", opt.smart_points()[0], p2)
    opt.close()


# ---------------------------------------------------------------- 5
def _gn_step_case(scene):
    g, v = sc.restatement(scene)
    e0 = g.error(v)
    x, l0, l1 = sr.gn_step(g, v)
    opt, objs = device(scene, gn=True)
    close("error", opt.error(), e0)
    # one parameter object = one lmgpu_add_smart_factors call: the constructor's error evaluation triangulated every factor in launches
    # of one group, a bin per degree class
    assert len({id(o.params) for o in objs}) == 1
    assert opt.smart_stats()["retriangulations"] == sum(len(f.keys) >= 2 for f in g.smart()) == len(g.smart())
    opt.linearize()
    _, d, d0, d1 = opt.solve(0.0)
    pts, st = opt.smart_points()
    assert st.tolist() == [f.status for f in g.smart()]
    for i, f in enumerate(g.smart()):
        if f.status == tr.VALID:
            close(f"point {i}", pts[i], f.point, np.linalg.norm(f.point))
    close("GN step", d, x, np.max(np.abs(x)))
    close("lin_err0", d0, l0, e0)
    close("lin_err1", d1, l1, e0)
    st = opt.smart_stats()
    assert st["n_factors"] == len(g.smart()) and st["retriangulations"] == 0
    opt.close()


@pytest.mark.parametrize("n", EDGE_COUNTS)
def test_factor_and_observation_counts(n):
    _gn_step_case(edge_scene(n))


def test_bins_of_more_than_one_workgroup():
    _gn_step_case(bins_scene())


def test_point_fronts_either_side_of_the_lds_limit():
    scene = wide_scene()
    _gn_step_case(scene)
    opt, _ = device(scene, gn=True)
    ns = sorted(opt.front_info(i)["n"] for i in range(opt.num_fronts()) if opt.front_info(i)["nf"] == 3)
    assert ns == [16, 136, 142], ns
    opt.close()


# ---------------------------------------------------------------- 6
def mixed_scene():
    epi = sc.zero_on_degeneracy(enableEPI=True)
    a = sc.ring_scene([2, 3, 4, 6, 9, 3, 5], seed=21, perturb=2e-3)
    b = sc.ring_scene([3, 5, 7], seed=21, perturb=2e-3, params=epi)  # the same cameras (same seed), other landmarks
    fs = [f for f in a["factors"] if f[0] == "smart"] + [f for f in b["factors"] if f[0] == "smart"][1:]
    keys = a["order"]
    truth = {f[1]: f[2] for f in a["factors"] if f[0] == "prior"}
    fs += [("between", keys[i], keys[(i + 1) % len(keys)], sr.between(truth[keys[i]], truth[keys[(i + 1) % len(keys)]]), 0.02) for i in range(len(keys))]
    fs += [("prior", keys[0], truth[keys[0]], 0.01), ("prior", keys[7], truth[keys[7]], 0.01)]
    return dict(values=a["values"], order=keys, factors=fs)


def test_mixed_graph_against_the_explicit_landmark_graph():
    import gtsam_personal_amd as gpa
    scene = mixed_scene()
    opt, objs = device(scene, gn=True)
    assert opt.num_smart_factors() == 9
    e_smart = opt.error()
    opt.linearize()
    dk, d, l0, l1 = opt.solve(0.0)
    pts, st = opt.smart_points()
    assert (st == tr.VALID).all()
    g2, v2, o2, _ = sc.package(scene, explicit_points=list(pts))
    ex = gpa.GaussNewtonOptimizer(g2, v2, o2)
    close("error of the explicit-landmark graph at the triangulated points", e_smart, ex.error())
    ex.linearize()
    dk2, _, m0, m1 = ex.solve(0.0)
    want = np.concatenate([dk2[k] for k in opt.ordering])
    close("GN step vs the pose part of the explicit graph's", d, want, np.max(np.abs(want)))
    close("lin_err1 (the point's optimum is the Schur complement)", l1, m1, e_smart)
    assert l0 < m0  # the Hessian factors' constant terms leave out what the point absorbs
    ex.close()
    opt.iterate()
    assert opt.error() < e_smart
    opt.close()
    lm, _ = device(scene)
    lm.iterate()
    assert lm.error() < e_smart and lm.iterations() == 1
    lm.optimize()
    assert lm.error() < 0.5 * e_smart
    lm.close()


# ---------------------------------------------------------------- 7
def test_python_surface():
    import gtsam_personal_amd as gpa
    from gtsam_personal_amd import graph as G
    from gtsam_personal_amd import smart as S
    scene = lm_scene()
    g, v, order, objs = sc.package(scene)
    assert all(o.isDegenerate() for o in objs)  # nothing evaluated yet
    opt = gpa.LevenbergMarquardtOptimizer(g, v, order)
    opt.optimize()
    for o, lm in zip(objs, (sc.LANDMARK1, sc.LANDMARK2, sc.LANDMARK3)):
        assert o.isValid() and not (o.isDegenerate() or o.isOutlier() or o.isFarPoint() or o.isPointBehindCamera())
        close("point() after optimize()", o.point().get(), lm, np.linalg.norm(lm) * 1e1)  # the optimum reproduces the landmarks to 1e-5
    st = opt.smart_stats()
    assert st["n_factors"] == 3 and st["n_status"][tr.VALID] == 3 and st["triangulate_ms"] >= 0.0
    opt.close()
    f = gpa.SmartProjectionPoseFactor(G.noiseModel.Isotropic.Sigma(2, 0.1), sc.K2, gpa.SmartProjectionParams())
    f.add([np.zeros(2), np.zeros(2)], [sc.X1, sc.X2])
    gd = gpa.NonlinearFactorGraph()
    gd.add_SmartProjectionPoseFactor(f)
    with pytest.raises(ValueError, match="IGNORE_DEGENERACY"):
        gpa.LevenbergMarquardtOptimizer(gd, v, gpa.Ordering([sc.X1, sc.X2, sc.X3]))
    assert S.ZERO_ON_DEGENERACY == 1
    # the incremental path refuses a graph that holds a smart factor, with a message, before anything reaches the device
    isam = gpa.ISAM2(ccolamd=lambda *a: 1, device=0)
    with pytest.raises(ValueError, match="newAffectedKeys"):
        isam.update(g, v)
    isam.close()


def _plain_results():
    """two small graphs without smart factors through the LM loop: the arrays a caller receives"""
    import gtsam_personal_amd as gpa
    from gtsam_personal_amd.synthetic import make_bal
    out = []
    graph, initial, _, ordering = make_bal(n_cam=6, n_pt=40, obs_per_point=3, seed=3)
    opt = gpa.LevenbergMarquardtOptimizer(graph, initial, ordering)
    assert opt.num_smart_factors() == 0 and opt.smart_stats()["n_factors"] == 0 and opt.smart_points()[0].shape == (0, 3)
    opt.smart_reset()
    for _ in range(3):
        opt.iterate()
    out.append(np.concatenate([opt.values().at(k) for k in ordering] + [[opt.error(), opt.lambda_()]]))
    opt.close()
    scene = mixed_scene()
    scene["factors"] = [f for f in scene["factors"] if f[0] != "smart"]
    g, v, order, _ = sc.package(scene)
    opt = gpa.GaussNewtonOptimizer(g, v, order)
    opt.iterate()
    out.append(np.concatenate([opt.values().at(k) for k in order] + [[opt.error()]]))
    opt.close()
    return out


def test_plain_handles_are_deterministic_beside_a_smart_handle():
    """no state leaks from a smart handle into a plain one: the same plain graphs give bitwise the same arrays before and after a smart
    handle has run in the process.  (This is not a comparison with an earlier revision of the library: that needs arrays of that revision,
    which are not kept; the parity suite against the oracle, unchanged, is what pins the plain path.)"""
    before = _plain_results()
    opt, _ = device(lm_scene())
    opt.optimize()
    opt.close()
    after = _plain_results()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
