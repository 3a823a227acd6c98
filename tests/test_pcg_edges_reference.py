"""The PCG edge cases (tests/pcg_cases.py) and their long-double reference (tests/pcg_reference.py), without a GPU, on the CPU oracle's
Jacobians.  This is the half of the pin that needs no device: it fixes the cases, the reference, the tolerance of every comparison and
the proof that the comparison sees what it is for.  The device half (the same comparisons on the Jacobians read back from the device)
is not in the suite yet -- DESIGN section 11 says why.

The cases:
  * every predicate of pcg_cases.EDGES is true for some case.
The reference on its own:
  * its batched Cholesky, triangular solves and scatter-adds against numpy's in float64;
  * its float64 mode and tests/pcg_restatement.py agree with its long-double run within the case's tolerance;
  * the long-double run's TRUE preconditioned residual |L^-1 (b - A x_k)|^2 equals the gamma_k its recurrence carries;
  * the seeded permutations change the last bits and nothing else.
What a device test of these cases relies on:
  * the tolerance of every comparison: floor = largest distance of three permuted float64 runs from the long-double run, tolerance =
    16 x floor, at least 64 ulps, and 16 x floor <= 1e-9 asserted here (a condition on the case);
  * the stop decisions: eps_abs = sqrt(gamma_(k*-1) gamma_k*) lies a factor 16 from both and below every earlier gamma;
  * every planted defect (pcg_reference.trajectory(defect=)) misses the tolerance of the cases built for it by at least 100 x.

Measured (CPU oracle's Jacobians, lambda 1e-3).  Per case the LARGEST over the four modes (BlockJacobi / Dummy x identity / diagonal
damping) and over the compared k; `at` names the mode of the largest x floor; time = one long-double run of the case:
    case                      k      floor x   floor gamma   tolerance x   tolerance gamma   at               time
    single                    <=1    3.4e-16   5.3e-16       1.4e-14       1.4e-14           bj-identity      0.00 s
    block[ntot255,nfac255]    <=4    3.4e-16   1.6e-15       1.4e-14       2.6e-14           bj-identity      0.00 s
    block[ntot256,nfac256]    <=4    4.0e-16   1.6e-15       1.4e-14       2.6e-14           dummy-identity   0.00 s
    block[ntot257,nfac257]    <=4    3.8e-16   1.0e-15       1.4e-14       1.6e-14           bj-diag          0.00 s
    block[nvars255]           <=4    3.4e-16   9.2e-16       1.4e-14       1.5e-14           bj-identity      0.00 s
    block[nvars256]           <=4    3.2e-16   1.6e-15       1.4e-14       2.5e-14           bj-diag          0.00 s
    block[nvars257]           <=4    3.7e-16   1.2e-15       1.4e-14       2.0e-14           bj-identity      0.00 s
    mixed                     <=4    4.7e-11   3.0e-13       7.5e-10       4.8e-12           bj-identity      0.01 s
    hub                       <=4    2.9e-11   7.0e-14       4.6e-10       1.1e-12           bj-identity      0.01 s
    stride                    <=4    3.4e-16   8.3e-16       1.4e-14       1.4e-14           dummy-identity   0.01 s
    partials[65536]           4      3.2e-16   2.3e-15       1.4e-14       3.7e-14           bj-identity      1.08 s
    partials[65537]           4      3.1e-16   1.8e-15       1.4e-14       2.9e-14           bj-identity      0.85 s
    weak_chain reset 501      <=33   1.2e-14   9.4e-14       2.0e-13       1.5e-12           bj-identity      0.01 s
    weak_chain reset 1        <=33   1.2e-15   3.5e-14       1.8e-14       5.6e-13           bj-identity      0.01 s
    weak_chain reset 2        <=33   2.1e-15   6.5e-14       3.3e-14       1.0e-12           bj-identity      0.00 s
    weak_chain reset 16       <=33   6.0e-15   7.9e-14       9.5e-14       1.3e-12           bj-identity      0.00 s
    weak_chain reset 17       <=33   1.0e-14   7.2e-14       1.7e-13       1.2e-12           bj-identity      0.00 s
    weak_chain reset 33       <=33   1.2e-14   1.5e-13       1.9e-13       2.4e-12           bj-identity      0.00 s
Stops (stop[K]): eps_abs = sqrt(gamma_(K-1) gamma_K); its distance from either, smallest over the four modes, and the largest tolerance of x_K:
    stop[3]    eps_abs 8.6e-16 .. 1.1e-14   gamma_(K-1) / eps = eps / gamma_K >= 8.8e+13   tolerance x_K <= 1.6e-14
    stop[16]   eps_abs 7.0e-16 .. 8.2e-14   gamma_(K-1) / eps = eps / gamma_K >= 4.8e+11   tolerance x_K <= 3.4e-13
    stop[17]   eps_abs 4.2e-16 .. 1.1e-13   gamma_(K-1) / eps = eps / gamma_K >= 1.6e+11   tolerance x_K <= 2.9e-13
Planted defects: the smallest miss / tolerance over the cases and modes run (asserted >= 100), and where:
    stride_tail            5.6e+11   (stride, dummy-diag; 6 runs)
    pq_beyond_256          3.0e+16   (partials[65536], dummy-diag; 4 runs)
    last_rr_partial        5.9e+08   (partials[65537], dummy-diag; 4 runs)
    key2_at_d0             4.3e+12   (mixed, dummy-diag; 4 runs)
    no_damping             6.1e+07   (mixed, bj-identity; 6 runs)
    stale                  3.3e+13   (block[nvars256], bj-identity; 4 runs)
    reset_stale_partials   2.8e+16   (weak_chain, dummy-diag; 8 runs)
gamma_(k-1) for the fresh gamma at a reset is NOT such a defect (exact arithmetic makes them the same number): its runs lie 0.03 to 0.14
tolerances from the reference, asserted <= 1 (test_previous_gamma_at_a_reset_is_the_same_number).
The partials cases are the slowest tests here: 3 to 7 s each (the oracle linearizes 131 073 factors one call at a time, 2.5 s, once per
case and process; one long-double run of four iterations is 0.9 to 1.1 s, a permuted float64 run 0.4 s).
"""
import numpy as np
import pytest

import pcg_cases as pc
import pcg_reference as ref
import pcg_restatement as pr

SMALL = pc.SHAPES + ["weak_chain", "stop[3]"]


@pytest.mark.parametrize("d", (1, 2, 3, 5, 6, 9))
def test_batched_cholesky_and_solves(d):
    rng = np.random.default_rng(d)
    M = rng.normal(size=(17, d + 3, d))
    H = np.einsum("nri,nrj->nij", M, M) + 1e-3 * np.eye(d)
    y = rng.normal(size=(17, d))
    L = ref._chol(H)
    for i in range(17):
        Li = np.linalg.cholesky(H[i])
        assert np.allclose(L[i], Li, rtol=1e-12, atol=1e-14)
        assert np.allclose(ref._lsolve(L, y)[i], np.linalg.solve(Li, y[i]), rtol=1e-10)
        assert np.allclose(ref._ltsolve(L, y)[i], np.linalg.solve(Li.T, y[i]), rtol=1e-10)
    Lq = ref._chol(H.astype(ref.LD))
    assert Lq.dtype == ref.LD and np.abs(np.einsum("nij,nkj->nik", Lq, Lq) - H).max() <= 1e-17 * np.abs(H).max()


def test_scatter_add_is_bincount_in_float64_and_exact_in_long_double():
    rng = np.random.default_rng(0)
    t = rng.integers(0, 50, 4000)
    w = rng.normal(size=4000)
    for seed_rng in (None, np.random.default_rng(1)):
        order, starts, uq = ref._scatter_plan(t, seed_rng)
        out = np.zeros(50)
        out[uq] = np.add.reduceat(w[order], starts)
        assert np.allclose(out, np.bincount(t, w, minlength=50), rtol=1e-12, atol=1e-13)
    # 1 + 2^-60 + ... : float64 loses the small terms, long double keeps them
    w2 = np.array([1.0] + [2.0 ** -60] * 8, dtype=ref.LD)
    order, starts, uq = ref._scatter_plan(np.zeros(9, dtype=np.int64), None)
    assert np.add.reduceat(w2[order], starts)[0] == ref.LD(1) + ref.LD(2.0 ** -57)


def _restated(arr, damp):
    facs, dims = [], {s: int(d) for s, d in enumerate(arr.dims)}
    for i, g in enumerate(arr.gi):
        Ab = arr.data[arr.off[i]:arr.off[i + 1]].reshape(arr.cols[i], arr.rows[i]).T
        sl = [int(s) for s in arr.slots[g] if s >= 0]
        o = np.concatenate([[0], np.cumsum([dims[s] for s in sl])])
        facs.append((sl, [Ab[:, o[j]:o[j + 1]] for j in range(len(sl))], Ab[:, -1]))
    xoff = np.concatenate([[0], np.cumsum(arr.dims)])
    return pr.System(facs, dims, damping={s: damp[xoff[s]:xoff[s + 1]] for s in dims})


@pytest.mark.parametrize("pre,diag", ref.MODES, ids=ref.MODE_IDS)
@pytest.mark.parametrize("name", SMALL)
def test_float64_and_restatement_agree_with_long_double(name, pre, diag):
    KS = pc.shape_ks(name)
    arr, damp, r, tol, _ = ref.cpu_compared(name, pre, diag, 4)
    ref.check_cap(tol, KS)
    plain = ref.trajectory(ref.System(arr, damp, np.float64), ref.params(pre, maxIterations=4))
    sysr = _restated(arr, damp)
    assert ref.rel(sysr.getb(), ref.System(arr, damp).rhs) <= 1e-13
    for k in KS:
        x, iters, gammas, thr = pr.pcg(sysr, pr.PCGParams(1, k, 501, 0.0, 0.0, pre))
        assert iters == k and thr == 0.0
        for what, xx, gg in (("float64", plain.x[k], plain.gammas[k]), ("restatement", x, gammas[k])):
            mx, mg = ref.x_miss(tol[k], xx, r.x[k]), ref.gamma_miss(tol[k], gg, r.gammas[k])
            assert mx <= 1 and mg <= 1, (name, what, k, mx, mg, tol[k])


@pytest.mark.parametrize("pre,diag", ref.MODES, ids=ref.MODE_IDS)
@pytest.mark.parametrize("name", pc.SHAPES + ["weak_chain", "stride"])
def test_long_double_residual_is_consistent_with_gamma(name, pre, diag):
    kmax = 33 if name == "weak_chain" else max(pc.shape_ks(name))
    arr, damp, r, _, _ = ref.cpu_compared(name, pre, diag, kmax)
    S = ref.System(arr, damp)
    P = ref._Precond(S, pre)
    for k in range(kmax + 1):
        t = P.solve(S.rhs - S.multiply(r.x[k]))
        true = (t * t).sum()
        assert abs(true - r.gammas[k]) <= 1e-13 * r.gammas[k] + 1e-30 * r.gammas[0], (name, k, float(true), float(r.gammas[k]))
    assert float(S.residual_norm(r.x[kmax])) < float(S.residual_norm(r.x[0]))


def test_permuted_runs_differ_in_their_last_bits_only():
    arr, damp, r, tol, _ = ref.cpu_compared("stride", ref.BLOCK_JACOBI, False, 4)
    runs = [ref.trajectory(ref.System(arr, damp, np.float64, s), ref.params(ref.BLOCK_JACOBI, maxIterations=4)) for s in (1, 2, 3)]
    assert not np.array_equal(runs[0].x[4], runs[1].x[4]) and not np.array_equal(runs[1].x[4], runs[2].x[4])
    assert all(ref.rel(t.x[4], r.x[4]) <= 64 * ref.EPS64 for t in runs)
    again = ref.trajectory(ref.System(arr, damp, np.float64, 1), ref.params(ref.BLOCK_JACOBI, maxIterations=4))
    assert np.array_equal(again.x[4], runs[0].x[4])


# ---------------------------------------------------------------- the cases
def test_every_edge_is_reached():
    st = [pc.stats(pc.case(n)) for n in pc.NAMES]
    missing = [e for e, pred in pc.EDGES.items() if not any(pred(s) for s in st)]
    assert not missing, missing


# ---------------------------------------------------------------- the tolerance of every comparison of the GPU test
def _row(name, extra, tol, ks, t):
    fx, fg = max(tol[k]["floor_x"] for k in ks), max(tol[k]["floor_g"] for k in ks)
    tx, tg = max(tol[k]["tol_x"] for k in ks), max(tol[k]["tol_g"] for k in ks)
    print("TABLE %-24s %-30s k<=%-3d floor x %.1e gamma %.1e  tolerance x %.1e gamma %.1e  reference %.2f s" % (name, extra, max(ks), fx, fg, tx, tg, t))


@pytest.mark.parametrize("pre,diag", ref.MODES, ids=ref.MODE_IDS)
@pytest.mark.parametrize("name", pc.SHAPES + ["stride"])
def test_tolerance_of_the_shape_cases(name, pre, diag):
    _, _, _, tol, t = ref.cpu_compared(name, pre, diag, 4)
    _row(name, ref.mode_id(pre, diag), tol, pc.shape_ks(name), t)
    ref.check_cap(tol, pc.shape_ks(name))


@pytest.mark.parametrize("pre,diag", ref.MODES, ids=ref.MODE_IDS)
@pytest.mark.parametrize("n", (65536, 65537))
def test_tolerance_of_the_partials_cases(n, pre, diag):
    name = "partials[%d]" % n
    _, _, _, tol, t = ref.cpu_compared(name, pre, diag, 4)
    _row(name, ref.mode_id(pre, diag), tol, (4,), t)
    ref.check_cap(tol, (4,))


def reset_ks(reset, kmax=33):
    """the iterations a reset run is compared at: the last one and one just after a reset"""
    return sorted({kmax, min(kmax, reset + 1)})


@pytest.mark.parametrize("pre,diag", ref.MODES, ids=ref.MODE_IDS)
def test_tolerance_of_the_chunk_and_reset_runs(pre, diag):
    for reset in (501,) + pc.RESETS + (33,):
        _, _, r, tol, t = ref.cpu_compared("weak_chain", pre, diag, 33, reset)
        ks = pc.CHUNK_MAX if reset == 501 else reset_ks(reset)
        _row("weak_chain", "%s reset %d" % (ref.mode_id(pre, diag), reset), tol, ks, t)
        ref.check_cap(tol, ks)
        assert min(float(g) for g in r.gammas) > 1e-12 * float(r.gammas[0])  # 33 iterations are natural, nothing near underflow


@pytest.mark.parametrize("pre,diag", ref.MODES, ids=ref.MODE_IDS)
@pytest.mark.parametrize("K", pc.STOP_K)
def test_stop_decisions_are_clear(K, pre, diag):
    """stop[K]: the loop ends after exactly K iterations for eps_abs between gamma_(K-1) and gamma_K, by a factor 16 on either side, in
    long double and in every permuted float64 run"""
    name = "stop[%d]" % K
    arr = ref.cpu_arrays(name)
    damp = ref.damping_vector(arr, pc.LAMBDA, diag)
    r = ref.trajectory(ref.System(arr, damp), ref.params(pre, maxIterations=K + 3))
    eps = ref.stop_epsilon(r, K)
    runs = [r] + [ref.trajectory(ref.System(arr, damp, np.float64, s), ref.params(pre, maxIterations=K + 3)) for s in (1, 2, 3)]
    for t in runs:
        g = [float(x) for x in t.gammas]
        assert all(x >= 16 * eps for x in g[:K]) and g[K] * 16 <= eps, (name, eps, g)
        assert all(np.isfinite(g)) and all(np.isfinite(np.asarray(t.x[K + 3], dtype=np.float64)))  # iterating on after the end stays finite
    stopped = ref.trajectory(ref.System(arr, damp), ref.params(pre, maxIterations=500, epsilon_abs=eps))
    assert stopped.iterations == K
    _, tol = ref.tolerances(arr, damp, ref.params(pre, maxIterations=K), (K,))
    print("TABLE %-24s %-30s eps_abs %.2e: gamma_(K-1) / eps %.1e, eps / gamma_K %.1e, tolerance x_K %.1e" % (
        name, ref.mode_id(pre, diag), eps, float(r.gammas[K - 1]) / eps, eps / float(r.gammas[K]), tol[K]["tol_x"]))
    ref.check_cap(tol, (K,))


# ---------------------------------------------------------------- planted defects
def _miss(arr, damp, p, ks, defect):
    """the largest miss over the compared k, in tolerances, of the unpermuted float64 run with the defect (the same run without it passes)"""
    r, tol = ref.tolerances(arr, damp, p, ks)
    ref.check_cap(tol, ks)
    key2 = defect == "key2_at_d0"
    good = ref.trajectory(ref.System(arr, damp, np.float64), p)
    bad = ref.trajectory(ref.System(arr, damp, np.float64, key2_at_d0=key2), p, None if key2 else defect)
    for k in ks:
        assert ref.x_miss(tol[k], good.x[k], r.x[k]) <= 1 and ref.gamma_miss(tol[k], good.gammas[k], r.gammas[k]) <= 1
    return max(max(ref.x_miss(tol[k], bad.x[k], r.x[k]), ref.gamma_miss(tol[k], bad.gammas[k], r.gammas[k])) for k in ks)


def _defect_cases():
    out = [(("stride_tail", cap), "stride", dict(maxIterations=4), (2, 4)) for cap in pc.STRIDE_CAPS[1:]]
    out += [("pq_beyond_256", "partials[%d]" % n, dict(maxIterations=2), (1, 2)) for n in (65536, 65537)]
    out += [("last_rr_partial", nm, dict(maxIterations=2), (1, 2)) for nm in ("partials[65537]", "block[nvars257]")]
    out += [("key2_at_d0", nm, dict(maxIterations=2), (1, 2)) for nm in ("mixed", "hub")]
    out += [("no_damping", nm, dict(maxIterations=2), (1, 2)) for nm in ("mixed", "block[ntot256,nfac256]", "stride")]
    out += [("stale", nm, dict(maxIterations=2), (1, 2)) for nm in ("block[nvars256]", "weak_chain")]
    out += [("reset_stale_partials", "weak_chain", dict(maxIterations=33, reset=rs), tuple(reset_ks(rs))) for rs in pc.RESETS]
    return out


DEFECTS = _defect_cases()
DEFECT_IDS = ["%s-%s-%s" % ("%s%d" % d if isinstance(d, tuple) else d, n, "-".join("%s%d" % kv for kv in sorted(kw.items()))) for d, n, kw, _ in DEFECTS]


@pytest.mark.parametrize("defect,name,kw,ks", DEFECTS, ids=DEFECT_IDS)
@pytest.mark.parametrize("pre,diag", [ref.MODES[0], ref.MODES[3]], ids=[ref.MODE_IDS[0], ref.MODE_IDS[3]])
def test_planted_defect_is_seen(defect, name, kw, ks, pre, diag):
    arr = ref.cpu_arrays(name)
    damp = ref.damping_vector(arr, pc.LAMBDA, diag)
    d = ("stale", ref.System(ref.cpu_arrays(name, True), damp, np.float64)) if defect == "stale" else defect
    miss = _miss(arr, damp, ref.params(pre, **kw), ks, d)
    print("DEFECT %-18s %-24s %-16s %-36s miss / tolerance %.1e" % ("%s %d" % defect if isinstance(defect, tuple) else defect, name,
                                                                     ref.mode_id(pre, diag), kw, miss))
    assert miss >= 100.0, (defect, name, miss)


@pytest.mark.parametrize("reset", pc.RESETS)
@pytest.mark.parametrize("pre,diag", [ref.MODES[0], ref.MODES[3]], ids=[ref.MODE_IDS[0], ref.MODE_IDS[3]])
def test_previous_gamma_at_a_reset_is_the_same_number(reset, pre, diag):
    """A reset iteration that divided by gamma_(k-1) instead of the gamma of the recomputed residual is NOT a defect a comparison can
    see: b - A x_k is the residual the recurrence carries, the two gammas differ by the recurrence's rounding drift, and that drift is
    what the floor measures.  Measured: the float64 run with it lies 0.03 to 0.14 tolerances from the long-double run (1 / 16 is the
    floor itself).  So the device may use either; what a reset can get wrong visibly is WHICH partials it sums (reset_stale_partials)."""
    arr = ref.cpu_arrays("weak_chain")
    damp = ref.damping_vector(arr, pc.LAMBDA, diag)
    miss = _miss(arr, damp, ref.params(pre, maxIterations=33, reset=reset), reset_ks(reset), "reset_prev_gamma")
    print("DEFECT %-18s %-24s %-16s reset %-2d miss / tolerance %.1e" % ("reset_prev_gamma", "weak_chain", ref.mode_id(pre, diag), reset, miss))
    assert miss <= 1.0
