"""ISAM2's tree-walk kernels (csrc/isam2.hpp) at clique, list and epoch edges, against the longdouble restatement
(isam2_walk_reference.py) computed on the DEVICE's own tree, ISAM2.cliques(): elimination, which has suites of its own, is not part of the
comparison, and oracle/_ref is not read (the ordering is the cases' natural_order).  The cases and what each reaches:
isam2_walk_cases.py; the same checks with the CPU oracle in the device's place: test_isam2_walk_reference.py.

  isam2_wildfire_kernel        every case, two updates: a batch one (all replaced: by default the by-value top; the wide cliques and all of
                               it under LMGPU_ISAM2_NO_BYVALUE through the done flags) and one that re-eliminates the roots alone (the
                               others dirty by their separator: solve, compare with the threshold, keep).  Threshold > 0, threshold 0 and
                               the forced full solve of calculateBestEstimate().  Untouched cliques BITWISE equal to the delta before.
  isam2_mark_kernel, isam2_tree_patch_kernel   through the same runs: a wrong replaced flag or child list changes which cliques are solved
  isam2_marginal_kernel        the cases' marginal keys (dimensions 2, 3, 6; paths of 1 .. 33 cliques, through LDS and wide cliques)
  gradient / gather / rg / dot / gradient_search / blend / tree_error   the first update under ISAM2DoglegParams at three radii, one per
                               branch of ComputeDoglegPoint; the radius afterwards from rho (model part: the tree's error at 0 and at the point)
  the 8-bit epoch              262 updates, each read: the wrap after walk 255, every walk checked, bitwise where untouched

Tolerance: max(16 x floor, 64 n eps) relative to the largest entry, n the widest clique; floor = the same operation on the same cliques in
float64 numpy against longdouble.  Measured on an MI355X (largest over a case's updates; floor / device deviation):

  case                 walk                NO_BYVALUE          NO_MIRROR           marginals           dog leg             tolerance (walk)
  lone                 5.9e-17 / 9.3e-17   5.9e-17 / 9.3e-17   5.9e-17 / 9.3e-17   5.8e-17 / 5.8e-17   1.2e-16 / 9.3e-17   4.2e-14
  pair[32,8]           5.9e-16 / 4.5e-16   5.9e-16 / 4.5e-16   5.9e-16 / 4.5e-16   1.6e-16 / 2.3e-16   6.4e-16 / 4.6e-16   5.6e-13
  pair[33,8]           3.6e-16 / 4.8e-16   3.6e-16 / 4.8e-16   3.6e-16 / 4.8e-16   2.9e-16 / 2.3e-16   3.9e-16 / 4.8e-16   5.8e-13
  pair[63,3]           7.3e-16 / 8.5e-16   7.3e-16 / 8.5e-16   7.3e-16 / 8.5e-16   2.1e-16 / 2.1e-16   7.3e-16 / 8.5e-16   9.3e-13
  pair[64,75]          2.1e-15 / 1.3e-15   2.1e-15 / 1.3e-15   2.1e-15 / 1.3e-15   3.8e-16 / 2.5e-16   2.1e-15 / 1.3e-15   2.0e-12
  pair[65,73]          5.7e-16 / 1.4e-15   5.7e-16 / 1.4e-15   5.7e-16 / 1.4e-15   3.0e-16 / 3.2e-16   5.7e-16 / 1.4e-15   1.9e-12
  pair[128,8]          6.0e-16 / 1.3e-15   6.0e-16 / 1.3e-15   6.0e-16 / 1.3e-15   2.6e-16 / 1.6e-16   7.2e-16 / 1.3e-15   1.9e-12
  pair[129,6]          1.1e-15 / 6.2e-16   1.1e-15 / 6.2e-16   1.1e-15 / 6.2e-16   1.9e-16 / 1.9e-16   1.1e-15 / 6.4e-16   1.9e-12
  pair[3,135]          4.3e-16 / 5.6e-16   4.3e-16 / 5.6e-16   4.3e-16 / 5.6e-16   2.7e-16 / 2.9e-16   2.2e-16 / 5.6e-16   1.9e-12
  pair[65,75]          4.9e-16 / 1.1e-15   4.9e-16 / 1.1e-15   4.9e-16 / 1.1e-15   4.0e-16 / 1.5e-16   5.0e-16 / 1.1e-15   2.0e-12
  pair[64,78]          8.1e-16 / 7.4e-16   8.1e-16 / 7.4e-16   8.1e-16 / 7.4e-16   1.6e-16 / 2.4e-16   8.1e-16 / 7.4e-16   2.0e-12
  pair[128,12]         6.8e-16 / 1.8e-15   6.8e-16 / 1.8e-15   6.8e-16 / 1.8e-15   2.7e-16 / 1.6e-16   6.8e-16 / 1.8e-15   2.0e-12
  pair[129,12]         1.1e-15 / 1.5e-15   1.1e-15 / 1.5e-15   1.1e-15 / 1.5e-15   1.4e-16 / 3.7e-16   1.1e-15 / 1.5e-15   2.0e-12
  wide_tree            8.3e-16 / 7.0e-16   8.3e-16 / 7.0e-16   8.3e-16 / 7.0e-16   4.7e-16 / 1.1e-15   3.5e-16 / 7.0e-16   4.5e-12
  children[1]          1.5e-16 / 1.8e-16   1.5e-16 / 1.8e-16   1.5e-16 / 1.8e-16   2.2e-16 / 2.2e-16   2.1e-16 / 1.8e-16   8.4e-14
  children[256]        2.2e-16 / 2.3e-16   2.2e-16 / 2.3e-16   2.2e-16 / 2.3e-16   9.0e-17 / 1.2e-16   1.9e-16 / 1.9e-16   8.4e-14
  children[257]        2.0e-16 / 2.4e-16   2.0e-16 / 2.4e-16   2.0e-16 / 2.4e-16   1.3e-16 / 2.8e-16   1.4e-16 / 2.4e-16   8.4e-14
  forest[1]            4.3e-16 / 2.5e-16   4.3e-16 / 2.5e-16   4.3e-16 / 2.5e-16   7.7e-17 / 7.7e-17   4.3e-16 / 2.5e-16   8.4e-14
  forest[64]           2.6e-16 / 6.2e-16   2.6e-16 / 6.2e-16   2.6e-16 / 6.2e-16   1.7e-16 / 1.7e-16   3.6e-16 / 6.2e-16   8.4e-14
  forest[65]           4.7e-16 / 6.1e-16   4.7e-16 / 6.1e-16   4.7e-16 / 6.1e-16   1.6e-16 / 1.6e-16   5.0e-16 / 6.1e-16   8.4e-14
  chain[350]           1.5e-15 / 1.2e-15   1.5e-15 / 1.2e-15   1.5e-15 / 1.2e-15   4.2e-16 / 8.2e-16   1.5e-15 / 1.1e-15   8.4e-14
  pose3                2.0e-16 / 7.7e-16   2.0e-16 / 7.7e-16   2.0e-16 / 7.7e-16   9.4e-17 / 1.6e-16   2.0e-16 / 7.7e-16   1.7e-13
  decay[40]            3.9e-16 / 5.2e-16   3.9e-16 / 5.2e-16   3.9e-16 / 5.2e-16   3.0e-16 / 1.0e-16   -                   8.4e-14
  decay[two anchors]   2.8e-16 / 2.5e-16   2.8e-16 / 2.5e-16   2.8e-16 / 2.5e-16   1.2e-16 / 2.3e-16   -                   8.4e-14
  epoch wrap (262 updates): default 4.8e-16 / 6.5e-16; NO_BYVALUE 4.8e-16 / 6.5e-16; NO_MIRROR 4.8e-16 / 6.5e-16; dogleg 4.1e-16 / 5.1e-16

Planted defects (a scratch build each, these tests in the default form): the three clears at the epoch wrap dropped -- test_epoch_wrap fails
at update 255 (walk 256) on the bitwise assertion, nothing else; the wide branch skipping its partial last block of 64 rows --
test_walk and test_dogleg fail on pair[65,75], pair[129,12] and wide_tree with deviations of 0.16 .. 10.  A children loop of a
single pass was not run on a GPU (it spins to the bound on purpose); test_isam2_walk_reference.py plants its numerical effect instead.
"""
import numpy as np
import pytest

from gtsam_personal_amd import ISAM2, ISAM2DoglegParams, ISAM2GaussNewtonParams, ISAM2Params

import isam2_walk_cases as wc
import isam2_walk_reference as wr

pytestmark = pytest.mark.gpu

FORMS = ["LMGPU_ISAM2_NO_BYVALUE", "LMGPU_ISAM2_NO_MIRROR"]


def make(threshold):
    return ISAM2(ISAM2Params(ISAM2GaussNewtonParams(threshold), 0.0, 0, False), ccolamd=wc.natural_order, device=0)


def make_dogleg(radius):
    return ISAM2(ISAM2Params(ISAM2DoglegParams(radius, 0.0, ISAM2DoglegParams.ONE_STEP_PER_ITERATION), 0.0, 0, False), ccolamd=wc.natural_order, device=0)


def record(test, name, stats):
    print(f"measured {test} {name}: floor {stats['floor']:.1e} dev {stats['dev']:.1e} tol {stats['tol']:.1e}")


def forced_full_solve(c, isam):
    """calculateBestEstimate() walks with the threshold forced to 0 and leaves its result in delta"""
    isam.calculateBestEstimate()
    tree = wr.Tree(isam.cliques(), wc.dims_of(c))
    ref = wr.full_solve(tree)
    floor = wr.deviation(wr.full_solve(tree, np.float64), ref)
    dev, tol = wr.deviation(tree.vec(isam.getDelta(), np.float64), ref), wr.tolerance(floor, tree.widest())
    assert wr.FACTOR * floor <= wr.CAP and dev <= tol, (dev, tol)
    return dict(floor=floor, dev=dev, tol=tol)


def walk_forms(c):
    """threshold > 0 (then the forced full solve on top of it) and threshold 0"""
    isam, stats = wc.check_walk(c, make, c["threshold"])
    stats.append(forced_full_solve(c, isam))
    isam.close()
    isam, stats0 = wc.check_walk(c, make, 0.0)
    isam.close()
    return wc.merge(stats + stats0)


@pytest.mark.parametrize("name", wc.NAMES)
def test_walk(name):
    c = wc.case(name)
    record("walk", name, walk_forms(c))


@pytest.mark.parametrize("switch", FORMS)
@pytest.mark.parametrize("name", wc.NAMES)
def test_walk_scheduling_forms(monkeypatch, dev_switches, name, switch):
    """the by-value top and the host mirror each switched off: the done-flag hand-off everywhere, delta copied instead of mirrored"""
    monkeypatch.setenv(switch, "1")
    record(switch, name, walk_forms(wc.case(name)))


@pytest.mark.parametrize("name", wc.NAMES)
def test_marginals(name):
    c = wc.case(name)
    isam = make(0.0)
    for _ in wc.replay(c, isam):
        pass
    record("marginals", name, wc.check_marginals(c, isam))
    isam.close()


@pytest.mark.parametrize("name", wc.DOGLEG_NAMES)
def test_dogleg(name):
    made = []

    def factory(radius):
        made.append(make_dogleg(radius))
        return made[-1]

    stats = wc.check_dogleg(wc.case(name), factory)
    for isam in made:
        isam.close()
    record("dogleg", name, wc.merge(stats))


def epoch_run():
    c = wc.epoch_case(35)
    assert len(c["updates"]) >= 260  # one walk per update: ++epoch == 0 after the 255th
    isam, stats = wc.check_walk(c, make, c["threshold"])  # EVERY update: the margins, bitwise where untouched, the tolerance where kept
    assert all(s["kept"] < s["visited"] < len(c["expect"]) for s in stats[1:])  # the walk is cut: cliques left alone, cliques never visited
    marg = wc.check_marginals(c, isam)
    full = forced_full_solve(c, isam)
    isam.close()
    return wc.merge(stats + [marg, full])


def test_epoch_wrap():
    record("epoch", "default", epoch_run())


@pytest.mark.parametrize("switch", FORMS)
def test_epoch_wrap_scheduling_forms(monkeypatch, dev_switches, switch):
    monkeypatch.setenv(switch, "1")
    record("epoch", switch, epoch_run())


def test_epoch_wrap_dogleg():
    """the dog leg walks once per update into delta_newton; at a radius no Newton step reaches, delta is that walk's result"""
    isam, stats = wc.check_walk(wc.epoch_case(35), lambda _thr: make_dogleg(1e3), 0.0, exact=False)
    isam.close()
    record("epoch", "dogleg", wc.merge(stats))
