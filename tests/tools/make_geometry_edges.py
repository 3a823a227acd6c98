"""Writes tests/golden/geometry_edges.npz: the edge cases of tests/geometry_reference.py (inputs as stored FP64 numbers), their
expected [H1 H2 (H3) b], factor errors and retracted values evaluated in 50 digits and rounded to FP64, and the floors: the CPU
oracle's own largest deviation from those values per factor type / variable type and quantity (e -- also per comparison mode, since
on the tie axis the two valid permutations differ by d^2 --, H, error, retracted value), measured with tests/geometry_edges.py.  The GPU test allows 16 x the floor.

    python tests/tools/make_geometry_edges.py          (after __graft_entry__.build(): the floors need oracle/liblm_oracle.so)

tests/test_geometry_reference.py regenerates all of it in memory and compares it with the committed file."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import geometry_edges as ge  # noqa: E402
import geometry_reference as gr  # noqa: E402
from gtsam_personal_amd.graph import FACTOR_ROWS  # noqa: E402


def expected():
    """every array of the fixture that comes from the 50-digit reference alone"""
    fx = {}
    for ft, rows in gr.factor_cases().items():
        J, err, aux = [], [], []
        for r in rows:
            e, H, _ = gr.evaluate_factor(ft, r["vals"], r["meas"])
            J.append([float(x) for i in range(FACTOR_ROWS[ft]) for x in sum((h[i] for h in H), []) + [-e[i]]])
            err.append(float(sum(x * x for x in e) / 2))
            aux.append(gr.flat3(gr.se3_exp(gr.sc(-r["sgn"], e[:6]))) if r["mode"] == gr.MODE_EXP3 else [0.0] * 12)
        fx["f%d_vals" % ft] = np.array([np.concatenate(r["vals"]) for r in rows])
        fx["f%d_meas" % ft] = np.array([r["meas"] for r in rows])
        fx["f%d_J" % ft] = np.array(J)
        fx["f%d_err" % ft] = np.array(err)
        fx["f%d_aux" % ft] = np.array(aux)
        fx["f%d_mode" % ft] = np.array([r["mode"] for r in rows], dtype=np.int32)
        fx["f%d_sgn" % ft] = np.array([r["sgn"] for r in rows], dtype=np.float64)
        fx["f%d_name" % ft] = np.array([r["name"] for r in rows])
    for vt, rows in gr.retract_cases().items():
        fx["r%d_name" % vt] = np.array([r[0] for r in rows])
        fx["r%d_val" % vt] = np.array([r[1] for r in rows])
        fx["r%d_delta" % vt] = np.array([r[2] for r in rows])
        fx["r%d_exp" % vt] = np.array([[float(x) for x in gr.retract_value(vt, r[1], r[2])] for r in rows])
    rb = gr.robust_cases()
    fx["b_kind"] = np.array([r[0] for r in rb], dtype=np.int32)
    fx["b_k"] = np.array([r[1] for r in rb])
    fx["b_d"] = np.array([r[2] for r in rb])
    fx["b_w"] = np.array([float(gr.robust_weight(*r)) for r in rb])
    fx["b_loss"] = np.array([float(gr.robust_loss(*r)) for r in rb])
    fx["b_J"] = np.array([[float(gr.mp.sqrt(gr.robust_weight(*r)) * x) for x in (1, 0, 0, -gr.M(r[2]), 0, 1, 0, 0, 0, 0, 1, 0)] for r in rb])
    return fx


def oracle_deviations(fx):
    """the CPU oracle over the whole table: one graph with every factor case on variables of its own, one per m-estimator, one per
    retracted variable type.  Returns (floors as fixture arrays, per-case deviations for messages, graph errors (oracle, expected))"""
    import oracle_harness as oh
    from gtsam_personal_amd.graph import Ordering
    fl = dict(floor_e=np.zeros((14, 3)), floor_H=np.zeros(14), floor_err=np.zeros(14), floor_x=np.zeros(7), floor_rb=np.zeros(2))
    per_case, sums = {}, []
    fts = ge.factor_types(fx)
    graph, values, order = ge.build_factor_graph(fx, fts, gr.ROWS_PER_TYPE)
    orc = oh.OracleProblem(graph, values, Ordering.Natural(graph))
    orc.linearize()
    for g, (ft, i) in enumerate(order):
        de, dH, derr = ge.factor_deviation(fx, ft, i, orc.jacobian(g))
        per_case[(ft, str(fx["f%d_name" % ft][i]))] = (de, dH, derr)
        mode = int(fx["f%d_mode" % ft][i])
        fl["floor_e"][ft, mode] = max(fl["floor_e"][ft, mode], de)
        fl["floor_H"][ft], fl["floor_err"][ft] = max(fl["floor_H"][ft], dH), max(fl["floor_err"][ft], derr)
    sums.append((orc.error(), float(sum(fx["f%d_err" % ft].sum() for ft in fts))))
    for kind in sorted(set(fx["b_kind"].tolist())):
        graph, values, rows = ge.build_robust_graph(fx, kind)
        orc = oh.OracleProblem(graph, values, Ordering.Natural(graph))
        orc.linearize()
        for g, i in enumerate(rows):
            d = ge._dev(orc.jacobian(g), fx["b_J"][i].reshape(3, 4))
            per_case[("robust", "kind%d_d%.17g" % (kind, fx["b_d"][i]))] = (d,)
            fl["floor_rb"][0] = max(fl["floor_rb"][0], d)
        fl["floor_rb"][1] = max(fl["floor_rb"][1], ge._dev(orc.error(), fx["b_loss"][rows].sum()))
        sums.append((orc.error(), float(fx["b_loss"][rows].sum())))
    for vt in sorted(int(k[1:-4]) for k in fx if k.startswith("r") and k.endswith("_val")):
        graph, values, delta = ge.build_retract_graph(fx, vt)
        orc = oh.OracleProblem(graph, values, Ordering.Natural(graph))
        orc.retract(delta)
        got = orc.values()
        for k, exp in enumerate(fx["r%d_exp" % vt]):
            d, ortho = ge.retract_deviation(vt, got[k], exp)
            per_case[("retract%d" % vt, str(fx["r%d_name" % vt][k]))] = (d, ortho)
            fl["floor_x"][vt] = max(fl["floor_x"][vt], d)
    return fl, per_case, sums


def generate():
    fx = expected()
    fx.update(oracle_deviations(fx)[0])
    return fx


if __name__ == "__main__":
    out = generate()
    np.savez_compressed(ge.FIXTURE, **out)
    print("wrote %s: %d arrays, %d bytes" % (ge.FIXTURE, len(out), os.path.getsize(ge.FIXTURE)))
    for k in ("floor_e", "floor_H", "floor_err", "floor_x", "floor_rb"):
        print(k, out[k])
