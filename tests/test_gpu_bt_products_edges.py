"""The Dogleg half of the solver at its front and radius edges: the five kernels of csrc/kernels_bayes.hpp (bt_lds_forward_kernel,
bt_lds_transpose_kernel, bt_gather_kernel, bt_hbm_forward_kernel, bt_hbm_transpose_kernel) with the slot table of bt_build_gather, read
through lmgpu_bt_products, and dl_iterate itself, on the cases and runs of tests/bt_products_cases.py.

Products, per case: the fronts are the ones the case was chosen for (front_info); linearize, solve with lambda = 0; the gradient and
the squared norm for alpha in {0, 1, -0.5} with a standard-normal x and with x = 0 against the extended-precision reference built from
the DEVICE's own Jacobians (-A^T b; ||A x - alpha b||^2 - alpha^2 (||b||^2 - ||d||^2)); every call is repeated once and is bitwise
equal; then the Newton step is retracted -- from h->delta, which the tap must have left alone: the values are compared with the oracle's
retract of the solve's step -- and everything is done again on the second linearization, over the slot table and the row buffer of the
first.  Tolerance: max(16 x the oracle-cliques floor of the case, 64 n 2.2e-16), n = the widest front (bt_products_cases; 16 x floor
above 1e-9 fails the case); the squared norm of x = 0, alpha = 0 has to be an exact zero.  test_bt_products_reference.py shows on the
CPU that each of seven planted defects misses this tolerance by more than 100 x.

Dogleg, per run of bt_products_cases.RUNS (three radii chosen from |x_u| and |x_N| of the start on four cases, three far starts whose
radius collapses within the iteration): DoglegOptimizer::iterate against the long-double restatement, iteration by iteration -- the
number of trial points (getInnerIterations), error and radius within max(16 x what the float64 oracle deviates from the restatement,
64 n 2.2e-16), the values against the oracle's retract of the restatement's step within that bound for the step.  The branches are the
ones bt_products_cases.RUNS writes down (asserted from the restatement on the CPU); a device that took another would show another
count, radius or step.

Measured on an MI355X (gradient: max|g - g_ref| / max|g_ref|; norm: relative; worst over the six probes and the two linearizations;
every repeated call was bitwise equal, x = 0 with alpha = 0 gave an exact zero in every case).  The device deviates by at most 9.4e-15 /
1.9e-15, the float64 oracle by 9.9e-15 / 1.7e-15:
                          oracle floor          device                tolerance
    case                  gradient  norm        gradient  norm        gradient / norm
    staging[31]           9.1e-15   7.2e-16     1.6e-15   9.2e-16     1.4e-13 / 9.9e-14
    children[3]           2.1e-15   4.2e-16     1.3e-15   6.7e-16     3.1e-13 / 3.1e-13
    children[4]           1.4e-15   4.1e-16     7.5e-16   4.1e-16     3.1e-13 / 3.1e-13
    children[5]           1.1e-15   3.3e-16     2.4e-15   3.3e-16     3.1e-13 / 3.1e-13
    bin[24]               2.0e-15   4.3e-16     3.0e-15   2.8e-16     3.4e-13 / 3.4e-13
    bin[64,74]            3.3e-15   3.8e-16     2.8e-15   3.5e-16     2.0e-12 / 2.0e-12
    bin[65,73]            3.1e-15   2.0e-16     3.2e-15   3.6e-16     2.0e-12 / 2.0e-12
    bin[3,135]            2.7e-15   3.3e-16     2.7e-15   8.9e-16     2.0e-12 / 2.0e-12
    bin[135,3]            4.4e-15   3.0e-16     1.7e-15   7.2e-16     2.0e-12 / 2.0e-12
    backsub[128,8]        3.8e-15   5.2e-16     3.8e-15   6.2e-16     1.9e-12 / 1.9e-12
    backsub[129,6]        2.8e-15   3.2e-16     4.1e-15   5.2e-16     1.9e-12 / 1.9e-12
    pivots[48]            9.4e-16   2.7e-16     7.1e-16   7.6e-16     9.0e-13 / 9.0e-13
    pivots[49]            6.1e-15   5.2e-16     2.7e-15   6.1e-16     9.3e-13 / 9.3e-13
    children_wide         2.5e-15   3.2e-16     2.7e-15   5.1e-16     2.0e-12 / 2.0e-12
    deep_chain            9.2e-16   2.0e-16     5.8e-16   1.1e-16     1.8e-13 / 1.8e-13
    tiny_sfm              1.9e-16   2.1e-16     2.1e-16   3.1e-16     2.1e-13 / 2.1e-13
    pair[48,16]           1.4e-15   1.9e-16     1.6e-15   5.9e-16     9.2e-13 / 9.2e-13
    fused_level           4.2e-15   4.1e-16     1.0e-15   3.6e-16     3.7e-12 / 3.7e-12
    dims_2_3              2.6e-15   1.7e-15     1.9e-15   1.9e-15     2.0e-12 / 2.0e-12
    leaf_degrees          4.3e-16   3.0e-16     4.8e-16   1.6e-16     2.2e-12 / 2.2e-12
    medium_batch          6.3e-15   2.1e-16     5.2e-15   1.9e-16     3.6e-12 / 3.6e-12
    tail[257]             2.6e-15   3.5e-16     6.1e-15   2.0e-16     3.6e-12 / 3.6e-12
    tail[321]             9.9e-15   5.8e-16     4.8e-15   2.6e-16     4.5e-12 / 4.5e-12
    chain[576]            2.2e-15   5.0e-16     7.6e-16   2.0e-16     8.1e-12 / 8.1e-12
    separator[300,138]    8.0e-16   2.5e-16     1.0e-15   3.7e-16     6.2e-12 / 6.2e-12
    separator[96,600]     2.1e-15   3.7e-16     9.4e-15   6.0e-16     9.8e-12 / 9.8e-12
The Dogleg runs (relative deviation from the restatement; one tolerance for radius and error since both floors are below 64 n eps; the
words are the branches of every trial point: S cut / B blend / N Newton, g grow / k keep / h halve / r halve and try again).  Every trial
count was the restatement's and every value within the bound of its step:
    run                    iteration  trials               radius   error      tolerance   oracle: radius  error    step
    children[5]-cut        0          Sg                   0.0e+00  1.6e-15    3.1e-13     0.0e+00         0.0e+00  2.3e-16
    children[5]-cut        1          Sg                   0.0e+00  2.0e-15    3.1e-13     0.0e+00         0.0e+00  8.5e-17
    children[5]-cut        2          Bg                   2.3e-16  3.6e-15    3.1e-13     2.3e-16         8.3e-16  3.2e-15
    children[5]-cut        3          Bg                   3.0e-16  5.0e-15    3.1e-13     6.1e-16         1.5e-15  3.0e-15
    children[5]-blend      0          Bg                   1.6e-16  4.8e-15    3.1e-13     0.0e+00         2.4e-16  3.0e-15
    children[5]-blend      1          Ng                   5.2e-15  4.0e-15    3.1e-13     4.4e-15         3.8e-16  1.1e-14
    children[5]-blend      2          Ng                   5.2e-15  2.3e-15    3.1e-13     4.4e-15         8.8e-16  1.9e-12
    children[5]-newton     0          Ng                   0.0e+00  2.9e-15    3.1e-13     0.0e+00         1.3e-16  3.2e-15
    children[5]-newton     1          Ng                   0.0e+00  1.3e-15    3.1e-13     0.0e+00         1.4e-15  6.0e-14
    children[5]-newton     2          Ng                   0.0e+00  1.0e-15    3.1e-13     0.0e+00         1.5e-15  1.8e-11
    bin[65,73]-cut         0          Sg                   2.2e-16  2.0e-15    2.0e-12     2.2e-16         0.0e+00  2.3e-16
    bin[65,73]-cut         1          Sg                   4.4e-16  3.1e-15    2.0e-12     4.4e-16         0.0e+00  4.7e-16
    bin[65,73]-cut         2          Bg                   5.9e-16  1.3e-15    2.0e-12     0.0e+00         1.2e-16  5.9e-15
    bin[65,73]-cut         3          Ng                   1.8e-15  9.4e-16    2.0e-12     1.9e-16         8.2e-16  9.7e-15
    bin[65,73]-blend       0          Bg                   1.7e-16  6.1e-16    2.0e-12     0.0e+00         1.4e-15  7.0e-15
    bin[65,73]-blend       1          Ng                   5.0e-15  2.3e-16    2.0e-12     2.2e-15         9.4e-16  2.0e-14
    bin[65,73]-blend       2          Ng                   5.0e-15  1.2e-16    2.0e-12     2.2e-15         7.0e-16  1.0e-12
    bin[65,73]-newton      0          Ng                   0.0e+00  2.3e-16    2.0e-12     0.0e+00         1.9e-15  7.9e-15
    bin[65,73]-newton      1          Ng                   0.0e+00  1.9e-15    2.0e-12     0.0e+00         5.8e-16  1.6e-13
    deep_chain-cut         0          Sg                   0.0e+00  4.5e-16    1.8e-13     0.0e+00         0.0e+00  2.2e-16
    deep_chain-cut         1          Sg                   4.0e-16  1.2e-15    1.8e-13     4.0e-16         0.0e+00  3.4e-16
    deep_chain-cut         2          Bg                   5.4e-16  0.0e+00    1.8e-13     5.4e-16         2.9e-16  1.0e-15
    deep_chain-cut         3          Ng                   8.2e-15  1.6e-15    1.8e-13     2.6e-16         3.5e-16  5.5e-15
    deep_chain-blend       0          Bg                   1.7e-16  8.6e-15    1.8e-13     1.7e-16         2.2e-16  1.7e-15
    deep_chain-blend       1          Ng                   5.9e-15  2.9e-15    1.8e-13     1.2e-16         0.0e+00  1.5e-15
    deep_chain-blend       2          Ng                   5.9e-15  3.7e-15    1.8e-13     1.2e-16         5.8e-16  2.9e-13
    deep_chain-newton      0          Ng                   0.0e+00  3.0e-15    1.8e-13     0.0e+00         1.1e-15  2.0e-15
    deep_chain-newton      1          Ng                   0.0e+00  3.5e-16    1.8e-13     0.0e+00         1.2e-15  6.7e-14
    one_panel[65]-cut      0          Sg                   1.1e-16  1.6e-15    2.0e-12     1.1e-16         0.0e+00  2.6e-16
    one_panel[65]-cut      1          Sg                   3.0e-16  3.5e-15    2.0e-12     0.0e+00         0.0e+00  2.7e-16
    one_panel[65]-cut      2          Bg                   4.0e-16  2.4e-14    2.0e-12     2.0e-16         3.5e-16  8.1e-15
    one_panel[65]-cut      3          Bg                   1.3e-16  5.4e-15    2.0e-12     6.7e-16         9.3e-16  7.5e-15
    one_panel[65]-blend    0          Bg                   1.2e-16  2.0e-15    2.0e-12     2.4e-16         7.6e-16  6.4e-15
    one_panel[65]-blend    1          Ng                   1.7e-16  4.2e-16    2.0e-12     5.0e-16         2.1e-16  1.5e-14
    one_panel[65]-blend    2          Ng                   1.7e-16  2.1e-16    2.0e-12     5.0e-16         6.3e-16  5.1e-13
    one_panel[65]-newton   0          Ng                   0.0e+00  2.1e-16    2.0e-12     0.0e+00         2.1e-16  6.6e-15
    one_panel[65]-newton   1          Ng                   0.0e+00  1.5e-15    2.0e-12     0.0e+00         0.0e+00  1.2e-13
    one_panel[65]-newton   2          Ng                   0.0e+00  1.7e-15    2.0e-12     0.0e+00         1.5e-15  2.0e-11
    bin[65,73]~1000        0          Nr Nr Nr Nr Nr Bk    0.0e+00  4.7e-16    2.0e-12     0.0e+00         1.6e-16  7.0e-15
    bin[65,73]~8           0          Bg                   0.0e+00  1.8e-16    2.0e-12     3.0e-16         1.8e-16  6.7e-15
    bin[65,73]~8           1          Bh                   0.0e+00  1.9e-16    2.0e-12     3.0e-16         1.9e-16  3.8e-15
    one_panel[65]~1000     0          Nr Nr Nr Nr Nr Bk    0.0e+00  0.0e+00    2.0e-12     0.0e+00         1.5e-16  7.9e-15
    one_panel[65]~1000     1          Bk                   0.0e+00  0.0e+00    2.0e-12     0.0e+00         0.0e+00  5.4e-15
    one_panel[65]~1000     2          Bk                   0.0e+00  1.5e-16    2.0e-12     0.0e+00         4.6e-16  2.7e-15
    one_panel[65]~1000     3          Bk                   0.0e+00  7.5e-16    2.0e-12     0.0e+00         7.5e-16  3.0e-15
The whole module (41 tests) takes 11 s, no test more than a few seconds (the largest reference, medium_batch with n = 1348, is 2 s per
linearization).
"""
import numpy as np
import pytest

import bt_products_cases as bc
import oracle_harness as oh
from gtsam_personal_amd import DoglegOptimizer, DoglegParams, LevenbergMarquardtOptimizer
from gtsam_personal_amd.graph import POSE2

pytestmark = pytest.mark.gpu

# the fronts of the cases that carry no table of their own (schur_cases): (LDS fronts, [(nf, n) of the HBM fronts])
SCHUR_FRONTS = {"dims_2_3": (14, [(141, 142)]), "leaf_degrees": (15, [(3, 148), (3, 148), (153, 154)])}


def _assert_fronts(name, c, infos):
    if name in SCHUR_FRONTS:
        lds, hbm = SCHUR_FRONTS[name]
        assert sum(f["cls"] == 0 for f in infos) == lds and [(f["nf"], f["n"]) for f in infos if f["cls"] == 1] == hbm, infos
        return
    fields = [k for k in ("nf", "n", "parent", "cls", "level") if k in c["fronts"][0]]
    assert [{k: f[k] for k in fields} for f in infos] == [{k: f[k] for k in fields} for f in c["fronts"]], infos


def _values_close(c, got, want, bound):
    for k in c["initial"].keys():
        a, b = np.asarray(got.at(k), dtype=float), np.asarray(want.at(k), dtype=float)
        if c["initial"].type(k) == POSE2:  # theta = +pi and -pi are the same rotation
            a, b = np.array([a[0], a[1], np.cos(a[2]), np.sin(a[2])]), np.array([b[0], b[1], np.cos(b[2]), np.sin(b[2])])
        assert np.abs(a - b).max() <= bound + 8 * bc.EPS * max(1.0, np.abs(b).max()), (k, a, b, bound)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_products_against_reference(request, monkeypatch, name):
    switch = bc.switch_of(name)
    if switch:
        request.getfixturevalue("dev_switches")
        monkeypatch.setenv(*switch)
    c, fl = bc.case(name), bc.oracle_floor(name)
    assert bc.FACTOR * fl["gradient"] <= bc.CAP and bc.FACTOR * fl["norm"] <= bc.CAP, fl
    opt = LevenbergMarquardtOptimizer(c["graph"], c["initial"], c["ordering"], device=0)
    infos = [opt.front_info(i) for i in range(opt.num_fronts())]
    _assert_fronts(name, c, infos)
    widest = max(f["n"] for f in infos)
    tol_g, tol_n = bc.tolerance(fl["gradient"], widest), bc.tolerance(fl["norm"], widest)
    with pytest.raises(Exception, match="lmgpu_bt_products"):  # no factor in the pool yet
        opt.bt_products(np.zeros(opt._ntot), 1.0)
    orc = oh.OracleProblem(c["graph"], c["initial"], c["ordering"])
    worst = [0.0, 0.0]
    for p in range(2):
        opt.linearize()
        ref = bc.ProductsReference(c, [opt.jacobian(g) for g in range(c["graph"].size())])
        g_ref = ref.gradient()
        dk, packed, _, _ = opt.solve(0.0, False)
        state = (opt.error(), opt.lambda_(), opt.iterations(), opt.getInnerIterations())
        for x, alpha in bc.probes(ref.n, p):
            s, g = opt.bt_products(x, alpha)
            dg, dn = bc.gradient_deviation(g, g_ref), bc.norm_deviation(s, ref.sq_norm(x, alpha))
            print(f"{name} pass {p} alpha {alpha:4.1f} {'x = 0' if not x.any() else 'x ~ N'}: gradient {dg:.2e} (tolerance {tol_g:.2e})  norm {dn:.2e} (tolerance {tol_n:.2e})")
            worst = [max(worst[0], dg), max(worst[1], dn)]
            assert dg <= tol_g and dn <= tol_n, (name, p, alpha, dg, dn)
            s2, g2 = opt.bt_products(x, alpha)
            assert s2 == s and np.array_equal(g2, g)
        assert opt.bt_products()[0] is None and np.array_equal(opt.bt_products()[1], g)  # the gradient alone
        assert state == (opt.error(), opt.lambda_(), opt.iterations(), opt.getInnerIterations())
        if p == 0:
            opt.retract()  # h->delta: still the Newton step of the solve
            orc.retract(dk)
            _values_close(c, opt.values(), bc.values_of(c, orc.values()), 1e-9 * max(1.0, float(np.linalg.norm(packed))))
    opt.close()
    print(f"ROW {name:20s} {fl['gradient']:.1e}  {fl['norm']:.1e}   {worst[0]:.1e}  {worst[1]:.1e}   {tol_g:.1e} / {tol_n:.1e}")


@pytest.mark.parametrize("name", list(bc.RUNS))
def test_dogleg_against_restatement(name):
    c, radius = bc.run_start(name)
    its, _ = bc.restated_run(name)
    params = DoglegParams()
    params.deltaInitial = radius
    opt = DoglegOptimizer(c["graph"], c["initial"], c["ordering"], params, device=0)
    widest = max(opt.front_info(i)["n"] for i in range(opt.num_fronts()))
    assert abs(opt.error() - its[0][0]["f_error"]) <= 64 * widest * bc.EPS * its[0][0]["f_error"]
    inner = 0
    for k, (it, dev) in enumerate(its):
        opt.iterate()
        tol = {q: bc.tolerance(dev[q], widest) for q in ("delta", "error", "step")}
        got = dict(trials=opt.getInnerIterations() - inner, delta=abs(opt.getDelta() - it["delta"]) / it["delta"], error=abs(opt.error() - it["error"]) / it["error"])
        inner = opt.getInnerIterations()
        print(f"DROW {name:22s} {k}  {bc.words(it):18s} trials {got['trials']}  radius {got['delta']:.1e} ({tol['delta']:.1e})  error {got['error']:.1e} ({tol['error']:.1e})"
              f"  oracle {dev['delta']:.1e} {dev['error']:.1e} {dev['step']:.1e}")
        assert got["trials"] == len(it["trials"]), (name, k, got, bc.words(it))
        assert got["delta"] <= tol["delta"] and got["error"] <= tol["error"], (name, k, got, tol)
        assert opt.iterations() == k + 1
        _values_close(c, opt.values(), it["values"], tol["step"] * float(np.linalg.norm(it["step"])))
        # the next iteration starts from the restatement's own state on the restatement's side, from the device's on the device's: they
        # differ by the deviations just bounded
    opt.close()
