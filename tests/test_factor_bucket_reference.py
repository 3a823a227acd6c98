"""CPU checks around tests/factor_bucket_cases.py, the reference that tests/test_gpu_factor_bucket_edges.py holds the factor-bucket
kernels to (csrc/kernels_factors.hpp):
  * the long-double reference chain (whitening, Robust, GNC weight, error, Hessian diagonal, linear errors) agrees with the SAME chain
    run on mpmath numbers at 50 digits to one FP64 ulp of max(1, |expected|), on every case of the table;
  * the case table is what the issue asks of it: a noise row of its own per factor, every m-estimator with factors on both sides of
    its switch, every path and tail form of linear_error_kernel reached (restated from sz, joff contiguity and cnt), the two-bucket
    layout of case (g) from joff arithmetic, (e0 - e1) / e0 >= 0.1 on every linear_error case, exact and distinct reduce terms;
  * the CPU oracle against the reference over the whole table -- these deviations are the floors of the fixture -- and
    tests/golden/factor_bucket_edges.npz is what tests/tools/make_factor_bucket_edges.py writes today;
  * every planted defect, restated in FP64, misses the tolerance of the GPU test by at least 100 x (the smallest ratio is printed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

import factor_bucket_cases as fb  # noqa: E402
import geometry_edges as ge  # noqa: E402
import oracle_harness as oh  # noqa: E402
from gtsam_personal_amd.graph import (CAM_BUNDLER, F_BETWEEN_POSE2, F_SFM, F_SFM2, FACTOR_ROWS, N_DIAG, N_GAUSS, N_UNIT, POSE2, POSE3,  # noqa: E402
                                      VAR_DIM)

mp = pytest.importorskip("mpmath")
import make_factor_bucket_edges as mk  # noqa: E402  (needs mpmath)

ULP = 2.0 ** -52
MIN_DEFECT_RATIO = 100.0


class MP:
    """the number backend of factor_bucket_cases on mpmath numbers: object arrays of mpf, 50 digits"""
    name = "mpmath"
    sqrt, exp, expm1, log1p = staticmethod(mp.sqrt), staticmethod(mp.exp), staticmethod(mp.expm1), staticmethod(mp.log1p)

    @staticmethod
    def array(a):
        a = np.asarray(a)
        if a.dtype == object:
            return a
        out = np.empty(a.shape, dtype=object)
        flat = out.reshape(-1)
        for i, x in enumerate(a.reshape(-1)):
            flat[i] = mp.mpf(float(x))
        return out

    @staticmethod
    def scalar(x):
        return mp.mpf(float(x))


class F64:
    """the same chain in FP64: what a correct kernel computes, up to rounding; the planted defects are applied to it"""
    name = "float64"
    sqrt, exp, expm1, log1p = staticmethod(np.sqrt), staticmethod(np.exp), staticmethod(np.expm1), staticmethod(np.log1p)

    @staticmethod
    def array(a):
        return np.asarray(a, dtype=np.float64)

    @staticmethod
    def scalar(x):
        return np.float64(x)


@pytest.fixture(scope="module")
def fx():
    return fb.load()


@pytest.fixture(scope="module")
def generated():
    with mp.workdps(50):
        e = mk.expected()
    return e, mk.oracle_deviations(e)


def _mpdev(got, exp):
    """deviation of long-double numbers from mpf numbers, relative to max(1, |expected|), in FP64 ulps"""
    got, exp = np.asarray(got).reshape(-1), np.asarray(exp, dtype=object).reshape(-1)
    scale = max(1, max(abs(x) for x in exp))
    return float(max(abs(mp.mpf(float(g)) + mp.mpf(float(g - np.longdouble(float(g)))) - e) for g, e in zip(got, exp)) / scale) / ULP


# ---------------------------------------------------------------- the reference chain
def _heads(names):
    """of the cases that differ only in the number of factors (a smaller bucket is a prefix of the larger one) the largest"""
    best = {}
    for n in names:
        stem, _, size = n.rpartition("_n")
        if stem and size.isdigit():
            if stem not in best or int(size) > best[stem][0]:
                best[stem] = (int(size), n)
        else:
            best[n] = (0, n)
    return [v[1] for v in best.values()]


@pytest.mark.parametrize("cls", ("whiten", "sfm_blocks", "robust", "interleaved", "linear_error", "hessian_diag"))
def test_long_double_chain_against_mpmath(fx, cls):
    """every case (of size-nested cases the largest): about forty factors spread over the graph and its last one, their [A b], error
    and whitened |b|; for the three-variable, the two-bucket and the weighted case also the whole Hessian diagonal and both linear
    errors at a seeded delta"""
    mp.mp.dps = 50
    worst = 0.0
    for name in _heads(fb.names(cls)):
        c = fb.build(fx, name)
        n = len(c.factors)
        full = name in ("linerr_c_sfm2", "linerr_g_two_buckets", "interleaved_gnc", "hdiag_ntot256")
        pick = range(n) if full else sorted(set(range(0, n, max(1, n // 40))) | {n - 1})
        ld, ex = [], []
        for g in pick:
            f, w = c.factors[g], None if c.weights is None else c.weights[g]
            ld.append(fb.reference_factor(fb.LD, c.unwhitened(g), f["model"], w))
            ex.append(fb.reference_factor(MP, c.unwhitened(g), f["model"], w))
            for a, b in zip(ld[-1], ex[-1]):
                d = _mpdev(a, b)
                worst = max(worst, d)
                assert d <= 1.0, (name, g, d)
        if full:
            h1, h2 = c.hessian_diagonal(ld), c.hessian_diagonal(ex, MP)
            rng = np.random.default_rng(5)
            delta = {k: rng.uniform(-1, 1, VAR_DIM[c.values.type(k)]) for k in c.values.keys()}
            t1, t2 = c.linear_error_terms(ld, delta), c.linear_error_terms(ex, delta, MP)
            for k in h1:
                assert _mpdev(h1[k], h2[k]) <= 1.0, (name, k)
            for q in (0, 1):
                s1, s2 = fb.fsum(t[q] for t in t1), sum(t[q] for t in t2)
                assert abs(mp.mpf(s1) - s2) <= ULP * max(1, s2), (name, q)
    print("%s: largest deviation of the long-double chain from 50 digits %.3g ulp" % (cls, worst))


# ---------------------------------------------------------------- the case table
def test_every_factor_has_a_noise_row_of_its_own(fx):
    for ft in fb.FACTOR_TYPES:
        for kind in (N_DIAG, N_GAUSS):
            rows = [fb.noise_for(ft, f, kind) for f in range(129)]
            assert all(m.kind == kind for m in rows)
            assert len({m.data.tobytes() for m in rows}) == 129
            if kind == N_DIAG:
                assert all(0.05 <= m.data.min() and m.data.max() <= 20.0 and len(set(m.data.tolist())) == len(m.data) for m in rows)
            else:
                m = FACTOR_ROWS[ft]
                for r in rows:
                    R = r.data.reshape(m, m)
                    ratio = np.abs(R) / np.diag(R)[:, None]
                    assert np.all(np.tril(R, -1) == 0) and np.all((ratio[np.triu_indices(m, 1)] >= 0.5) & (ratio[np.triu_indices(m, 1)] <= 1.5))
    c = fb.build(fx, "interleaved")
    models = [f["model"] for f in c.factors if f["model"].kind != N_UNIT]
    assert len({(m.kind, m.data.tobytes()) for m in models}) == len(models)
    # graph order differs from bucket order everywhere: no two consecutive factors share a bucket
    keys = [(f["ft"], f["model"].kind) for f in c.factors]
    assert len(keys) == 257 and all(a != b for a, b in zip(keys, keys[1:]))
    assert c.bucket_positions() != list(range(257))
    w = fb.build(fx, "interleaved_gnc").weights
    assert (w == 0).sum() >= 20 and (w == 1).sum() >= 20 and ((w > 0) & (w < 1)).sum() >= 150


def test_every_estimator_sees_both_sides_of_its_switch(fx):
    for name in fb.names("robust"):
        c = fb.build(fx, name)
        rk, k = c.factors[0]["model"].robust_kind, c.factors[0]["model"].robust_k
        assert all(f["model"].robust_kind == rk and f["model"].robust_k == k for f in c.factors)
        d = np.array([float(b[2]) for b in c.reference_blocks()])
        q = d * d if rk == 7 else d
        below, above = int((q < k).sum()), int((q > k).sum())
        assert below >= fb.ROBUST_N // 3 and above >= fb.ROBUST_N // 3 - 1 and below + above == fb.ROBUST_N, (name, below, above)
        assert np.abs(q / k - 1).min() >= 0.02, name


def test_linear_error_paths_are_reached(fx):
    seen, per_case = set(), {}
    for name in fb.names("linear_error") + fb.names("interleaved"):
        c = fb.build(fx, name)
        waves = fb.linear_error_waves(c.descriptors())
        per_case[name] = waves
        for w in waves:
            seen.add(w["path"])
            if w["path"] == "staged":
                seen.add("staged_%s" % ("full" if w["cnt"] == 64 else "ragged"))
                seen.add("staged_sz%d" % w["sz"])
                seen.add("staged_padded" if w["padded"] else "staged_odd")
                if w["passes"] == 2 and w["partial"]:
                    seen.add("staged_two_trips_second_partial")
                seen.update("staged_" + f for f in w["forms"])
            elif w["path"] != "empty":
                seen.add("%s_%s" % (w["path"], "full" if w["cnt"] == 64 else "ragged"))
                seen.update("%s_%s" % (w["path"], f) for f in w["forms"])
                if w["path"] == "direct_mixed" and w["same_shape"]:
                    seen.add("direct_same_shape_not_back_to_back")
    want = {"empty", "staged", "direct_big", "direct_mixed", "staged_full", "staged_ragged", "staged_sz21", "staged_sz12", "staged_sz30",
            "staged_padded", "staged_odd", "staged_two_trips_second_partial", "staged_small", "staged_loop3", "direct_big_small",
            "direct_big_loop18", "direct_big_full", "direct_big_ragged", "direct_mixed_full", "direct_mixed_ragged",
            "direct_same_shape_not_back_to_back"}
    assert want <= seen, sorted(want - seen)
    # the named cases reach what they are named for
    a = per_case["linerr_a_n255_pb"]
    assert [w["path"] for w in a] == ["staged", "direct_mixed", "staged", "staged"] and a[3]["cnt"] == 63 and a[3]["sz"] == 21
    a = per_case["linerr_a_n257_pb"]
    assert [w["cnt"] for w in a] == [64, 64, 64, 64, 1, -63, -127, -191] and a[4]["path"] == "staged" and a[5]["path"] == "empty"
    assert [w["cnt"] for w in per_case["linerr_a_n1_bp"]] == [1, -63, -127, -191]
    b = per_case["linerr_b_sz12"]
    assert b[0]["path"] == "staged" and b[0]["sz"] == 12 and b[0]["passes"] == 2 and b[0]["partial"] and b[1]["same_shape"]
    assert per_case["linerr_c_sfm2"][0]["path"] == "staged" and per_case["linerr_c_sfm2"][0]["forms"] == {"loop3"}
    assert {w["path"] for w in per_case["linerr_d_big"]} == {"direct_big"}
    assert all(w["forms"] == {"loop18"} for w in per_case["linerr_e_chordal"][:1])
    f = per_case["linerr_f_one_lane"][0]
    assert f["cnt"] == 64 and f["path"] == "direct_mixed" and not f["same_shape"]
    # (g): 16 factors of 21 doubles fill 336 = 21 x 16 doubles, a multiple of the 16-double bucket alignment: the Gaussian bucket
    # starts where the Diagonal one ends and the first wave is staged across the boundary
    g = fb.build(fx, "linerr_g_two_buckets")
    d = g.descriptors()
    assert [f["model"].kind for f in g.factors[:17]] == [N_DIAG] * 16 + [N_GAUSS] and (16 * 21) % 16 == 0
    assert d[16][1] == d[15][1] + 21 == 16 * 21 and per_case["linerr_g_two_buckets"][0]["path"] == "staged"
    # every wave of the interleaved graph that holds more than one factor is mixed
    assert {w["path"] for w in per_case["interleaved"] if w["cnt"] > 1} <= {"direct_mixed", "direct_big"}


def test_hessian_diag_cases(fx):
    for ntot in fb.HDIAG_NTOT:
        c = fb.build(fx, "hdiag_ntot%d" % ntot)
        assert c.values.dim() == ntot
        hub, pos = 0, {}
        for f in c.factors:
            if hub in f["keys"]:
                pos[f["keys"].index(hub), f["ft"]] = pos.get((f["keys"].index(hub), f["ft"]), 0) + 1
        assert sum(pos.values()) == 300 and sorted(pos) == [(0, 2), (0, F_SFM2), (1, 2)] and min(pos.values()) == 100
        assert sum(1 for f in c.factors if f["ft"] == F_SFM2 and f["keys"][2] == 3) == 100     # the shared calibration, third position
        count = {}
        for f in c.factors:
            for k in f["keys"]:
                count[k] = count.get(k, 0) + 1
        assert sum(1 for v in count.values() if v == 1) >= 37


def test_reduce_terms_are_exact_and_distinct():
    from fractions import Fraction
    assert [fb.reduce_chain_bound(n) for n in fb.REDUCE_SIZES] == [18, 18, 18, 18, 18, 19]
    for n in fb.REDUCE_SIZES:
        graph, values, terms = fb.reduce_problem(n)
        assert graph.size() == n and len(graph.buckets()) == 1 and len(set(terms.tolist())) == n
        for i in sorted({0, n // 2, n - 1}):
            x, m = values.at(i), graph.buckets()[0][4][i]
            exact = sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(x, m)) / 2
            assert Fraction(float(terms[i])) == exact and all(float(a) - float(b) == Fraction(float(a)) - Fraction(float(b)) for a, b in zip(x, m))
        assert terms.min() >= fb.fsum(terms) / (4 * n)


def test_retract_cases(fx):
    """the retract graphs: a shuffled ordering (xoff not monotone inside a type array), and the CPU oracle within the one-ulp floor's
    tolerance of the 50-digit values, so the tolerance is one a correct FP64 implementation meets"""
    from gtsam_personal_amd.graph import Ordering
    c = fb.build(fx, "retract_n257")
    slot = {k: i for i, k in enumerate(c.ordering)}
    for vt in fb.VAR_TYPES:
        s = [slot[k] for k in c.values.keys() if c.values.type(k) == vt]
        assert len(s) == 257 and any(a > b for a, b in zip(s, s[1:]))
    orc = oh.OracleProblem(c.graph, c.values, Ordering.Natural(c.graph))
    orc.retract(c.delta)
    got, tol, worst = orc.values(), ge.tolerance(ge.EPS), 0.0
    for k, (vt, exp) in c.expected.items():
        d, ortho = retract_deviation(vt, got[k], exp)
        worst = max(worst, d)
        assert d <= tol and ortho <= ge.ORTHO_TOL, (k, vt, d, ortho)
    print("oracle retract: largest deviation %.3g (tolerance %.3g)" % (worst, tol))


def retract_deviation(vt, got, exp):
    if vt in (POSE2, POSE3, CAM_BUNDLER):
        return ge.retract_deviation(vt, got, exp)
    return fb.dev(got, exp), 0.0


# ---------------------------------------------------------------- the oracle and the fixture
def test_oracle_against_reference(generated):
    _, (floors, per_case, solved) = generated
    limit = ge.PROJECT_TOL / ge.GPU_MARGIN
    bad = ["%s: %s" % kv for kv in per_case.items() if max(kv[1]) > limit]
    assert not bad, "\n".join(bad)
    assert sorted(solved) == sorted(fb.names("linear_error") + ["interleaved"])
    low = {k: v for k, v in solved.items() if k in fb.names("linear_error") and not v[2] >= fb.MIN_REDUCTION}
    assert not low, low
    print("smallest (e0 - e1) / e0 over the linear_error cases: %.3f" % min(v[2] for k, v in solved.items()))
    for k in mk.FLOOR_KEYS:
        print(k, "max %.3g" % floors[k].max())


def test_fixture_is_current(generated):
    e, (floors, _, _) = generated
    committed = fb.load()
    assert sorted(committed) == sorted(list(e) + list(floors))
    for k, v in e.items():
        assert committed[k].dtype == v.dtype and np.array_equal(committed[k], v), k
    # the floors are FP64 measurements of the oracle as built here: the same up to a libm's last bits
    for k, v in floors.items():
        assert committed[k].shape == v.shape, k
        assert np.all(v <= 2 * np.maximum(committed[k], ge.EPS)) and np.all(committed[k] <= 2 * np.maximum(v, ge.EPS)), (k, v, committed[k])
    assert os.path.getsize(fb.FIXTURE) <= 4 * os.path.getsize(ge.FIXTURE) and os.path.getsize(fb.FIXTURE) < 1 << 20
    for k in mk.FLOOR_KEYS:
        for x in committed[k].reshape(-1):
            ge.tolerance(x)
    for ft in fb.FACTOR_TYPES:
        assert committed["f%d_J" % ft].shape == (fb.NCASE, fb.factor_size(ft))


# ---------------------------------------------------------------- planted defects
def _tolJ(fx, f):
    return ge.tolerance(fx["floor_J"][fb.floor_index(f)])


def _lin_terms_f64(c, blocks, delta):
    return c.linear_error_terms(blocks, delta, F64)


def _solve_delta(c):
    orc = oh.OracleProblem(c.graph, c.values, c.ordering)
    orc.linearize()
    rc, delta, _, _ = orc.solve(fb.LAMBDA)
    assert rc == 0
    return delta


def _staged_wrong_pitch(c, blocks, delta):
    """e0, e1 of linear_error_kernel when a staged wave reads lane l at l * sz instead of l * (sz | 1); FP64"""
    desc = c.descriptors()
    t = [list(x) for x in _lin_terms_f64(c, blocks, delta)]
    hit = 0
    for w, wave in enumerate(fb.linear_error_waves(desc)):
        if wave["path"] != "staged" or not wave["padded"]:
            continue
        sz, pitch, lanes = wave["sz"], wave["sz"] | 1, range(64 * w, 64 * w + wave["cnt"])
        stage = np.zeros(64 * fb.LINERR_MAX_SZ + 64)
        for q, g in enumerate(lanes):
            stage[q * pitch:q * pitch + sz] = np.asarray(blocks[g][0], dtype=np.float64).T.reshape(-1)   # column-major
        for q, g in enumerate(lanes):
            f = c.factors[g]
            m = FACTOR_ROWS[f["ft"]]
            Ab = stage[q * sz:q * sz + sz].reshape(-1, m).T
            d = np.concatenate([delta[k] for k in f["keys"]])
            r = Ab[:, :-1] @ d - Ab[:, -1]
            t[g] = [0.5 * float(Ab[:, -1] @ Ab[:, -1]), 0.5 * float(r @ r)]
            hit += q > 0
    assert hit > 0
    return fb.fsum(x[0] for x in t), fb.fsum(x[1] for x in t)


def test_planted_defects_miss_the_tolerance(fx):
    """each defect is applied to the chain restated in FP64; ratio = largest deviation over the cases meant for it / the tolerance the
    GPU test allows that quantity there"""
    ratios = {}

    def blocks64(c, weights=None, **kw):
        w = c.weights if weights is None else weights
        return [fb.reference_factor(F64, c.unwhitened(g), f["model"], None if w is None else w[g], **kw) for g, f in enumerate(c.factors)]

    # the undamaged FP64 chain passes everywhere it is used below (else a ratio would say nothing)
    def clean(c, ref):
        for f, a, b in zip(c.factors, blocks64(c), ref):
            assert fb.dev(a[0], fb.to_f64(b[0])) <= _tolJ(fx, f), c.name

    # 1. whitening with R transposed; 2. the noise row taken at stride M where M * M is meant
    r1 = r2 = np.inf
    for ft in fb.FACTOR_TYPES:
        c = fb.build(fx, "whiten_t%d_gauss_n129" % ft)
        ref, m = c.reference_blocks(), FACTOR_ROWS[ft]
        clean(c, ref)
        flat = np.concatenate([f["model"].data.reshape(-1) for f in c.factors] + [np.zeros(m * m)])
        a = b = 0.0
        for g, (f, (Ab, _, _)) in enumerate(zip(c.factors, ref)):
            J = c.unwhitened(g)
            a = max(a, fb.dev(f["model"].data.reshape(m, m).T @ J, fb.to_f64(Ab)) / _tolJ(fx, f))
            b = max(b, fb.dev(flat[g * m:g * m + m * m].reshape(m, m) @ J, fb.to_f64(Ab)) / _tolJ(fx, f))
        r1, r2 = min(r1, a), min(r2, b)
    ratios["R transposed"], ratios["noise stride M"] = r1, r2
    # 3. the Robust weight from the unwhitened b
    r3 = np.inf
    for name in fb.names("robust"):
        c = fb.build(fx, name)
        ref = c.reference_blocks()
        clean(c, ref)
        r3 = min(r3, max(fb.dev(a[0], fb.to_f64(b[0])) / _tolJ(fx, f) for f, a, b in zip(c.factors, blocks64(c, robust_from_unwhitened=True), ref)))
    ratios["robust weight from unwhitened b"] = r3
    # 4. the GNC weight indexed by bucket position instead of graph position
    c = fb.build(fx, "interleaved_gnc")
    ref = c.reference_blocks()
    clean(c, ref)
    wrong = c.weights[np.array(c.bucket_positions())]
    ratios["gnc weight by bucket position"] = max(fb.dev(a[0], fb.to_f64(b[0])) / _tolJ(fx, f) for f, a, b in zip(c.factors, blocks64(c, wrong), ref))
    # 5. a staged wave read at pitch sz; 6. a wave that drops its last valid lane
    tol_lin = [ge.tolerance(x) for x in fx["floor_lin"]]
    r5 = r6 = np.inf
    for name in fb.names("linear_error"):
        c = fb.build(fx, name)
        ref, delta = c.reference_blocks(), _solve_delta(c)
        want = c.linear_errors(ref, delta)
        b64 = blocks64(c)
        t = _lin_terms_f64(c, b64, delta)
        got = (fb.fsum(x[0] for x in t), fb.fsum(x[1] for x in t))
        assert all(fb.dev(got[q], want[q]) <= tol_lin[q] for q in (0, 1)), name
        waves = fb.linear_error_waves(c.descriptors())
        if any(w["path"] == "staged" and w["padded"] and w["cnt"] > 1 for w in waves):
            bad = _staged_wrong_pitch(c, b64, delta)
            r5 = min(r5, min(fb.dev(bad[q], want[q]) / tol_lin[q] for q in (0, 1)))
        for w, wave in enumerate(waves):
            if 0 < wave["cnt"] < 64:
                last = 64 * w + wave["cnt"] - 1
                bad = [fb.fsum(x[q] for i, x in enumerate(t) if i != last) for q in (0, 1)]
                r6 = min(r6, min(fb.dev(bad[q], want[q]) / tol_lin[q] for q in (0, 1)))
    ratios["staged pitch sz"], ratios["last valid lane dropped"] = r5, r6
    # 7. the Hessian diagonal of a third variable taken at d0 + c
    r7 = np.inf
    for ntot in fb.HDIAG_NTOT:
        c = fb.build(fx, "hdiag_ntot%d" % ntot)
        ref = c.reference_blocks()
        want, ok, bad = c.hessian_diagonal(ref), c.hessian_diagonal(blocks64(c), F64), c.hessian_diagonal(blocks64(c), F64, third_at_d0=True)
        tol = ge.tolerance(fx["floor_hdiag"][0])
        assert all(fb.dev(ok[k], fb.to_f64(want[k])) <= tol for k in want)
        r7 = min(r7, max(fb.dev(bad[k], fb.to_f64(want[k])) for k in want) / tol)
    ratios["third variable at d0 + c"] = r7
    # 8. a reduction that drops element n - 1
    r8 = np.inf
    for n in fb.REDUCE_SIZES:
        _, _, terms = fb.reduce_problem(n)
        total = fb.fsum(terms)
        r8 = min(r8, abs(fb.fsum(terms[:-1]) - total) / reduce_tolerance(n, total))
    ratios["reduction drops the last element"] = r8
    # 9. the SFM tile store shifted by one row at a block edge: the factors of block 1 get the row before theirs
    r9 = np.inf
    for name in fb.names("sfm_blocks"):
        c = fb.build(fx, name)
        if len(c.factors) <= 256:
            continue
        ref = c.reference_blocks()
        b64 = blocks64(c)
        r9 = min(r9, min(fb.dev(b64[g - 1][0], fb.to_f64(ref[g][0])) / _tolJ(fx, c.factors[g]) for g in range(256, len(c.factors))))
    ratios["sfm tile shifted at a block edge"] = r9
    for k, v in ratios.items():
        print("planted defect %-36s misses by %.3g x" % (k, v))
    print("smallest planted-defect ratio: %.3g" % min(ratios.values()))
    assert min(ratios.values()) >= MIN_DEFECT_RATIO, ratios


def reduce_tolerance(n, total):
    """absolute tolerance of a device sum of n exact terms: the one-ulp floor's tolerance plus the rounding of the longest add chain,
    ceil(n / (256 g)) + 8 + ceil(g / 256) + 8 additions with g = min(256, ceil(n / 256)), each at most 2^-53 of the sum"""
    g = min(256, -(-n // 256))
    chain = -(-n // (256 * g)) + 8 + -(-g // 256) + 8
    assert chain == fb.reduce_chain_bound(n)
    return (ge.tolerance(ge.EPS) + chain * 2.0 ** -53) * max(1.0, total)
