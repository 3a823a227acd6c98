"""CPU tests of the launch schedule of a dense front (csrc/dense_schedule.hpp: dense_front_schedule), read through
lmgpu_selftest_dense_schedule -- the list do_eliminate runs record by record.  No handle, no device: host arithmetic only.

A record is (kind, i, nsteps, chunk).  Every expectation below is written from the rules themselves (rows of a panel, column counts,
the limits of the kernels), never by asking the planner a second time."""
import ctypes as ct

import pytest

import dense_front_cases as dfc
from gtsam_personal_amd import _lib

PANEL_DATAFLOW, PANEL_TWO_LAUNCH, CHAIN, STEP_FUSED, UPDATE_QUADRANTS, UPDATE_MFMA, TAIL, ADD_CHUNK, WAIT_CHUNK = range(9)
SINGLE, SPLIT_HOST, SPLIT_EVENTS = range(3)
FORM_BIT = dict(two_launch=1, no_fuse=2, no_chain=4, no_tail=8)
PDF_MAX_COLTILES, PDF_MAX_CHAIN_T = 992, 114  # kernels_potrf.hpp
CAP = 4096

# the eight front shapes of test_chained_launch_ticket_order_is_a_topological_order
CHAIN_SHAPES = [(9001, 9000), (5401, 5400), (2000, 1500), (1081, 1080), (30000, 29000), (10000, 4000), (777, 770), (4097, 4096)]
SPLIT_SHAPES = [(9001, 9000), (5401, 5400), (2000, 1500), (1081, 1080)]


def schedule(n, nf, mode=SINGLE, forms=0):
    buf = (ct.c_int32 * (4 * CAP))()
    count = _lib.load().lmgpu_selftest_dense_schedule(n, nf, mode, forms, CAP, buf)
    assert count > 0, (n, nf, mode, forms, count)
    return [tuple(buf[4 * k:4 * k + 4]) for k in range(count)]


def rows(nf, i):
    return min(nf, 256 * (i + 1)) - 256 * i


def cols_behind(n, nf, i):
    return n - 256 * i - rows(nf, i)


def case_fronts():
    """(nf, n) of every dense front of dense_front_cases on the per-front path, and of the separator cases' roots"""
    out = [(nf, nf + 1) if nf + 1 > dfc.LDS_MAX_N else (nf, nf + dfc.SMALL_NS + 1) for nf in dfc.MEDIUM_SIZES]
    out += [(nf, nf + 1) for nf in dfc.TAIL_SIZES + dfc.CHAIN_SIZES + (1290,)]
    for nf, ns in dfc.SEPARATOR_SIZES:
        out += [(nf, nf + ns + 1), (ns + 3, ns + 4)]
    return out


@pytest.mark.parametrize("switch", [None] + sorted(dfc.SWITCH_ARGUMENT.values()))
def test_records_give_the_launch_counters_of_the_restatement(switch):
    """panel events, syrk launches and chain launches of the record list = dense_front_cases.front_launches, which the GPU test holds
    against kernel_times()"""
    kw = {switch: True} if switch else {}
    for nf, n in case_fronts():
        got = dict(panel=0, syrk=0, chain=0)
        for kind, _, _, _ in schedule(n, nf, SINGLE, FORM_BIT[switch] if switch else 0):
            assert kind not in (ADD_CHUNK, WAIT_CHUNK)  # one rank: no chunk protocol
            got["panel" if kind in (PANEL_DATAFLOW, PANEL_TWO_LAUNCH, TAIL) else "chain" if kind == CHAIN else "syrk"] += 1
        want = dfc.front_launches(nf, n, **kw)
        assert got == {k: want[k] for k in got}, (nf, n, switch)


def _panel_forms(n, nf, recs):
    """per outer panel: how the schedule factors it -- 'dataflow' / 'two_launch' (a panel record), 'in_step' (inside a fused step or a
    chained launch, which run the dataflow form) or 'tail'; every panel exactly once"""
    form = {}

    def put(i, what):
        assert i not in form, (n, nf, i)
        form[i] = what
    for kind, i, nsteps, _ in recs:
        if kind in (PANEL_DATAFLOW, PANEL_TWO_LAUNCH):
            put(i, "dataflow" if kind == PANEL_DATAFLOW else "two_launch")
        elif kind == STEP_FUSED:
            put(i + 1, "in_step")
        elif kind == CHAIN:
            for q in range(i, i + nsteps):
                put(q + 1, "in_step")
        elif kind == TAIL:
            put(i + 1, "tail")
    assert sorted(form) == list(range(-(-nf // 256))), (n, nf)
    return form


@pytest.mark.parametrize("two_launch", [False, True])
def test_dataflow_panel_exactly_when_rows_and_width_allow(two_launch):
    """what the launch counters cannot see: a panel runs as panel_dataflow_kernel (alone or inside a step) exactly when its rows are a
    multiple of 64, LMGPU_PANEL_2L is off and its row of 64-column tiles fits the flag buffer.  70 000 columns: the first 26 panels
    are too wide."""
    shapes = [(nf + 1, nf) for nf in (63, 64, 65, 193, 255, 256, 319, 320, 321)] + [(70000, 69952)]
    for n, nf in shapes:
        form = _panel_forms(n, nf, schedule(n, nf, SINGLE, FORM_BIT["two_launch"] if two_launch else 0))
        for i, what in form.items():
            ok = rows(nf, i) % 64 == 0 and not two_launch and (n - 256 * i + 63) // 64 <= PDF_MAX_COLTILES
            if what == "tail":
                assert not ok and rows(nf, i) < 64
            else:
                assert (what in ("dataflow", "in_step")) == ok, (n, nf, i, what)
    if not two_launch:
        form = _panel_forms(70000, 69952, schedule(70000, 69952))
        assert [i for i in sorted(form) if form[i] == "two_launch"] == list(range(26))


def test_tail_is_taken_up_to_48_columns():
    for nf, taken in ((257, True), (303, True), (304, False)):
        n = nf + 1
        assert cols_behind(n, nf, 0) == {257: 2, 303: 48, 304: 49}[nf]
        kinds = [r[0] for r in schedule(n, nf)]
        assert (TAIL in kinds) == taken, nf
        if taken:
            assert kinds == [PANEL_DATAFLOW, TAIL]
        assert TAIL not in [r[0] for r in schedule(n, nf, SINGLE, FORM_BIT["no_tail"])]


def test_quadrant_update_up_to_1024_columns():
    seen = set()
    for n, nf in ((1291, 1290), (1280, 300), (1281, 300)):
        for kind, i, _, _ in schedule(n, nf, SINGLE, FORM_BIT["no_fuse"]):
            assert kind not in (STEP_FUSED, CHAIN)
            if kind in (UPDATE_QUADRANTS, UPDATE_MFMA):
                m = cols_behind(n, nf, i)
                seen.add(m)
                assert (kind == UPDATE_QUADRANTS) == (m <= 1024), (n, nf, i, m)
    assert {1035, 1024, 1025} <= seen


@pytest.mark.parametrize("n,nf", [(141, 140), (300, 256), (300, 257), (1290, 540), (1600, 513)])
def test_plainest_form_is_the_wide_clique_sequence_of_isam2(n, nf):
    """two_launch | no_fuse | no_chain | no_tail, one rank: the form ISAM2 runs its wide cliques in.  Panel 0, then per panel the
    update with it (quadrants up to 1024 columns behind it, 128-tiles above) and the next panel; every panel in the two-launch form;
    the update of the last panel only when separator or right-hand-side columns follow it.  1, 2 and 3 panels; (1290, 540) crosses
    the 1024-column threshold between its first and its second update."""
    forms = FORM_BIT["two_launch"] | FORM_BIT["no_fuse"] | FORM_BIT["no_chain"] | FORM_BIT["no_tail"]
    want = []
    for i in range(-(-nf // 256)):
        want.append((PANEL_TWO_LAUNCH, i, 0, -1))
        m = cols_behind(n, nf, i)
        if m > 0:
            want.append((UPDATE_QUADRANTS if m <= 1024 else UPDATE_MFMA, i, 0, -1))
    assert schedule(n, nf, SINGLE, forms) == want
    assert want[-1][0] != PANEL_TWO_LAUNCH  # (n > nf in every shape: the right-hand side column at least)
    kinds = [r[0] for r in want]
    if (n, nf) == (1290, 540):  # 1034, 778 and 750 columns behind its three panels
        assert kinds == [PANEL_TWO_LAUNCH, UPDATE_MFMA, PANEL_TWO_LAUNCH, UPDATE_QUADRANTS, PANEL_TWO_LAUNCH, UPDATE_QUADRANTS]
    if (n, nf) == (1600, 513):  # 1344, 1088 and (behind a panel of one row) 1087 columns
        assert kinds == [PANEL_TWO_LAUNCH, UPDATE_MFMA] * 3


def test_chain_starts_where_its_tile_flags_fit():
    """(30000, 29000): fused steps until the trailing matrix has at most PDF_MAX_CHAIN_T tile rows, then ONE chained launch up to the
    last step whose next panel is full"""
    n, nf = 30000, 29000
    first = next(i for i in range(200) if (n - 256 * (i + 1) + 127) // 128 <= PDF_MAX_CHAIN_T)
    last = max(i for i in range(-(-nf // 256) - 1) if rows(nf, i + 1) % 64 == 0)
    assert (first, last) == (60, 111)
    recs = schedule(n, nf)
    assert recs[:first + 1] == [(PANEL_DATAFLOW, 0, 0, -1)] + [(STEP_FUSED, i, 0, -1) for i in range(first)]
    assert recs[first + 1] == (CHAIN, first, last - first + 1, -1)
    assert [r[0] for r in recs[first + 2:]] == [UPDATE_MFMA, PANEL_TWO_LAUNCH, UPDATE_QUADRANTS]  # 1072 columns, 72 rows, 1000 columns
    assert (n - 256 * first + 127) // 128 > PDF_MAX_CHAIN_T  # the step before does not fit


@pytest.mark.parametrize("mode", [SINGLE, SPLIT_EVENTS])
def test_every_chain_record_has_a_valid_ticket_order(mode):
    lib = _lib.load()
    checked = 0
    for n, nf in CHAIN_SHAPES:
        for kind, i0, nsteps, _ in schedule(n, nf, mode):
            if kind == CHAIN:
                assert lib.lmgpu_selftest_chain_schedule(n, nf, i0, nsteps, 100) == 0, (n, nf, i0, nsteps)
                checked += 1
    assert checked >= (8 if mode == SINGLE else 20)


def _chain_runs(n, nf):
    """maximal runs (first step, length >= 2) of steps that can share a launch: full panel, full-or-64-multiple next panel, columns behind"""
    np_ = -(-nf // 256)
    ok = [i + 1 < np_ and rows(nf, i) == 256 and rows(nf, i + 1) % 64 == 0 and (n - 256 * (i + 1) + 127) // 128 <= PDF_MAX_CHAIN_T for i in range(np_)]
    runs, i = [], 0
    while i < np_:
        j = i
        while j < np_ and ok[j]:
            j += 1
        if j - i >= 2:
            runs.append((i, j - i))
        i = max(j, i + 1)
    return runs


@pytest.mark.parametrize("n,nf", SPLIT_SHAPES)
def test_event_mode_chains_in_growing_segments_behind_their_chunk(n, nf):
    recs = schedule(n, nf, SPLIT_EVENTS)
    chains = [(k, r) for k, r in enumerate(recs) if r[0] == CHAIN]
    runs = _chain_runs(n, nf)
    assert runs and runs == _chain_runs_of(chains)
    for first, length in runs:
        sizes = [r[2] for _, r in chains if first <= r[1] < first + length]
        grow = [1, 1] + [2 ** k for k in range(1, 30)]
        assert sum(sizes) == length
        assert sizes[:-1] == grow[:len(sizes) - 1]  # 1, 1, 2, 4, 8, ...
        assert 1 <= sizes[-1] <= grow[len(sizes) - 1] + 1  # the last one takes what is left, at most one step more than its turn
        assert sizes[-1] != 1 or len(sizes) == 1  # no one-step remainder
    for k, (_, i0, nsteps, _) in chains:
        assert recs[k - 1] == (WAIT_CHUNK, -1, 0, i0 + nsteps)  # the last row chunk the segment folds in


def _chain_runs_of(chains):
    runs = []
    for _, (_, i0, nsteps, _) in chains:
        if runs and runs[-1][0] + runs[-1][1] == i0:
            runs[-1] = (runs[-1][0], runs[-1][1] + nsteps)
        else:
            runs.append((i0, nsteps))
    return runs


@pytest.mark.parametrize("n,nf", SPLIT_SHAPES)
def test_host_summed_mode_has_no_chained_launch(n, nf):
    recs = schedule(n, nf, SPLIT_HOST)
    assert CHAIN not in [r[0] for r in recs] and TAIL not in [r[0] for r in recs]
    for k, (kind, i, _, _) in enumerate(recs):
        if kind == STEP_FUSED:  # its head tiles fold the chunk of the next panel in: summed just before, not added by a kernel
            assert recs[k - 1] == (WAIT_CHUNK, -1, 0, i + 1)


@pytest.mark.parametrize("mode", [SPLIT_HOST, SPLIT_EVENTS])
@pytest.mark.parametrize("n,nf", SPLIT_SHAPES)
def test_every_row_chunk_arrives_once_and_before_it_is_needed(n, nf, mode):
    """Chunk c (rows 256 c ...) has to be in the working matrix (ADD_CHUNK) or summed for the launch that folds it in (WAIT_CHUNK)
    before panel 0 (c = 0) / before the step that updates with panel c - 1 and factors panel c.  One record per chunk; only the
    segments of event mode wait once for all their chunks: the events of one communication stream complete in order, so the wait
    for chunk i0 + nsteps stands for i0 + 1 .. i0 + nsteps."""
    nchunks = -(-n // 256)
    arrived = []

    def need(c, where):
        assert c >= nchunks or c in arrived, (n, nf, mode, c, where)
    for kind, i, nsteps, chunk in schedule(n, nf, mode):
        if kind in (ADD_CHUNK, WAIT_CHUNK):
            assert 0 <= chunk < nchunks and chunk not in arrived
            arrived.append(chunk)
        elif kind == CHAIN:
            assert mode == SPLIT_EVENTS and arrived[-1] == i + nsteps
            inside = list(range(i + 1, i + nsteps))
            assert not set(inside) & set(arrived)
            arrived += inside
        elif kind in (PANEL_DATAFLOW, PANEL_TWO_LAUNCH):
            need(i, "panel")
        else:  # a step in any form: update with panel i
            need(i + 1, "step")
    assert sorted(arrived) == list(range(nchunks))


def test_schedule_is_repeatable_and_refuses_nonsense():
    for n, nf in CHAIN_SHAPES:
        for mode in (SINGLE, SPLIT_HOST, SPLIT_EVENTS):
            assert schedule(n, nf, mode) == schedule(n, nf, mode)
    lib, buf = _lib.load(), (ct.c_int32 * 64)()
    for n, nf in ((100, 200), (0, 0), (-5, -6), (0, 5)):
        assert lib.lmgpu_selftest_dense_schedule(n, nf, SINGLE, 0, 16, buf) < 0
    assert lib.lmgpu_selftest_dense_schedule(1291, 1290, 3, 0, 16, buf) < 0  # unknown mode
    assert lib.lmgpu_selftest_dense_schedule(9001, 9000, SPLIT_HOST, 0, 16, buf) < 0  # more records than the buffer holds
    assert lib.lmgpu_selftest_dense_schedule(1291, 1290, SINGLE, 0, 16, buf) == 3  # panel 0, run of 4, tail
