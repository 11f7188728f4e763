"""The joint Levenberg-Marquardt driver, once for the kernels (csrc/dcx_lm_dev.h) and once for the host definitions
(deepcharuco_amd/_lm.py), walked through the branches real scenes rarely reach: rejected steps, the damping's two clamps, a step
forced at lg > 16, the iteration cap, the stop test at its boundary, and what each ends in.

The device automaton is plain C++: tests/lm_host_main.cpp is compiled here with the host compiler (no HIP, no GPU) at NG = 6 and
NG = 9 and both STOP_FORCED policies, and fed scripts of (cost, |dp|^2, |p|^2, bad) attempts.  The expected states below are
written out from the rules (damping 1 + 10^lg from lg = -3; a cost that is not <= the cost before: lg + 1 and retry, up to 16; at
17 the step is forced; an accepted or forced step: lg - 1 down to -16; at most 30 accepted steps; stop at |dp| < DBL_EPSILON |p|),
not from either implementation.  The same scripts then drive _lm.refine through toy callables."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from deepcharuco_amd import _lm

HERE = os.path.dirname(os.path.abspath(__file__))
EVALUATE, SCHUR, FINISHED = 0, 1, 2           # the state word: what the host launches next
OK, NO_UNITS, DEGENERATE, NONFINITE = range(4)
EPS = 2.0 ** -52                               # DBL_EPSILON
INF, NAN = math.inf, math.nan
UNITS, POINTS, INIT_COST = 3.0, 36.0, 10.0


@pytest.fixture(scope="module")
def lm_host(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("lm") / "lm_host")
    # (#pragma unroll is the device compilers'; the host compiler may not know it)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                    os.path.join(HERE, "lm_host_main.cpp"), "-o", exe], check=True)
    return exe


def _num(v):
    return "inf" if v == INF else "nan" if v != v else repr(float(v))


def _run(exe, ng, stop_forced, attempts, init=(INIT_COST, UNITS, POINTS)):
    """-> per decision (the init first) a dict of what the program printed."""
    text = " ".join(_num(v) for v in init) + "\n"
    text += "".join(f"{_num(c)} {_num(dn)} {_num(pn)} {int(bad)}\n" for c, dn, pn, bad in attempts)
    out = subprocess.run([exe, str(ng), str(int(stop_forced))], input=text, capture_output=True, text=True, check=True).stdout
    keys = ("code", "lg", "iters", "attempts", "verdict", "status", "prev_cost", "rms", "result_iters", "result_attempts")
    return [dict(zip(keys, (float(v) if k in ("prev_cost", "rms") else int(v) for k, v in zip(keys, line.split()))))
            for line in out.splitlines()]


def _state(row):
    return tuple(row[k] for k in ("code", "lg", "iters", "attempts", "verdict", "status"))


# ------------------------------------------------------------------------------------------------ the scripts
# name -> (attempts [(cost, dn, pn, bad)], expected (code, lg, iters, attempts, verdict, status) after each attempt).  Every script
# starts from an init cost of 10, which must answer (SCHUR, -3, 0, 0, 0, OK).

REJECT19 = [(11.0, 1.0, 1.0, False)] * 19      # lg -3 -> 16: nineteen retries
REJECT19_STATES = [(SCHUR, -3 + k, 0, k, 0, OK) for k in range(1, 20)]

SCRIPTS = {
    "accept and go on": ([(9.0, 1.0, 1.0, False)], [(EVALUATE, -4, 1, 1, 1, OK)]),
    "three rejections then accept": (
        [(12.0, 1.0, 1.0, False), (INF, 1.0, 1.0, False), (11.0, 1.0, 1.0, False), (10.0, 1.0, 1.0, False)],   # equal is accepted
        [(SCHUR, -2, 0, 1, 0, OK), (SCHUR, -1, 0, 2, 0, OK), (SCHUR, 0, 0, 3, 0, OK), (EVALUATE, -1, 1, 4, 1, OK)]),
    "stop test": ([(9.0, 0.0, 1.0, False)], [(FINISHED, -4, 1, 1, 2, OK)]),
    "stop test boundary": ([(9.0, EPS * EPS, 1.0, False)], [(EVALUATE, -4, 1, 1, 1, OK)]),      # sqrt(dn) == eps sqrt(pn): not <
    "max iterations": (
        [(10.0 - 0.25 * k, 1.0, 1.0, False) for k in range(1, 31)],
        [(EVALUATE, max(-3 - k, -16), k, k, 1, OK) for k in range(1, 30)] + [(FINISHED, -16, 30, 30, 2, OK)]),
    "forced finite": (REJECT19 + [(11.0, 1.0, 1.0, False)], REJECT19_STATES + [(EVALUATE, 16, 1, 20, 1, OK)]),
}


@pytest.mark.parametrize("stop_forced", [False, True])
@pytest.mark.parametrize("ng", [6, 9])
@pytest.mark.parametrize("name", list(SCRIPTS))
def test_device_automaton(lm_host, name, ng, stop_forced):
    attempts, states = SCRIPTS[name]
    rows = _run(lm_host, ng, stop_forced, attempts)
    assert _state(rows[0]) == (SCHUR, -3, 0, 0, 0, OK) and rows[0]["prev_cost"] == INIT_COST
    assert [_state(r) for r in rows[1:]] == states
    last = rows[-1]
    if name == "stop test":
        assert last["rms"] == math.sqrt(9.0 / POINTS) and (last["result_iters"], last["result_attempts"]) == (1, 1)
    if name == "max iterations":
        assert [r["lg"] for r in rows[1:14]] == list(range(-4, -17, -1)) and rows[13]["lg"] == -16       # -16 after 13 accepts
        assert last["rms"] == math.sqrt(2.5 / POINTS) and (last["result_iters"], last["result_attempts"]) == (30, 30)
    if name == "forced finite":
        assert last["prev_cost"] == 11.0       # the forced step's cost is what the next one is measured against
    if name == "three rejections then accept":
        assert last["prev_cost"] == 10.0


@pytest.mark.parametrize("ng", [6, 9])
def test_device_automaton_forced_non_finite(lm_host, ng):
    # as "forced finite", the twentieth cost inf: the policies part
    rows = _run(lm_host, ng, True, REJECT19 + [(INF, 1.0, 1.0, False)])
    assert [_state(r) for r in rows[1:]] == REJECT19_STATES + [(FINISHED, 16, 1, 20, 1, DEGENERATE)]
    assert (rows[-1]["result_iters"], rows[-1]["result_attempts"], rows[-1]["rms"]) == (1, 20, 0.0)
    rows = _run(lm_host, ng, False, REJECT19 + [(INF, 1.0, 1.0, False)])
    assert [_state(r) for r in rows[1:]] == REJECT19_STATES + [(EVALUATE, 16, 1, 20, 1, OK)]
    assert rows[-1]["prev_cost"] == INF
    # a trial pose that is not finite, or a NaN cost: NONFINITE
    for last in ((INF, 1.0, 1.0, True), (NAN, 1.0, 1.0, False)):
        rows = _run(lm_host, ng, True, REJECT19 + [last])
        assert _state(rows[-1]) == (FINISHED, 16, 1, 20, 1, NONFINITE)
    # forced with cost inf while the stop test fires: DEGENERATE under both policies
    for stop_forced in (False, True):
        rows = _run(lm_host, ng, stop_forced, REJECT19 + [(INF, 0.0, 1.0, False)])
        assert _state(rows[-1]) == (FINISHED, 16, 1, 20, 1, DEGENERATE)
        assert (rows[-1]["result_iters"], rows[-1]["result_attempts"], rows[-1]["rms"]) == (1, 20, 0.0)


@pytest.mark.parametrize("stop_forced", [False, True])
@pytest.mark.parametrize("ng", [6, 9])
def test_device_automaton_init(lm_host, ng, stop_forced):
    rows = _run(lm_host, ng, stop_forced, [], init=(INF, UNITS, POINTS))
    assert len(rows) == 1 and _state(rows[0]) == (FINISHED, -3, 0, 0, 0, DEGENERATE)
    rows = _run(lm_host, ng, stop_forced, [], init=(0.0, 0.0, 0.0))
    assert len(rows) == 1 and _state(rows[0]) == (FINISHED, -3, 0, 0, 0, NO_UNITS)
    rows = _run(lm_host, ng, stop_forced, [(9.0, 1.0, 1.0, False)], init=(INF, UNITS, POINTS))
    assert len(rows) == 1                       # nothing is decided once the state word says finished


# ------------------------------------------------------------------------------------------------ the host driver

def _drive(ng, stop_forced, attempts, monkeypatch, init_cost=INIT_COST):
    """_lm.refine on one unit whose pose starts at (1, 0, 0, 0, 0, 0) (|p|^2 = 1, the globals are zero).  Attempt k's scripted
    step moves the pose's second coordinate by sqrt(dn) (or makes it inf for `bad`), which leaves |p|^2 of the committed point at
    1 or 2 and gives |dp|^2 = dn exactly for dn in {0, 1, eps^2}; the toy callables answer the scripted costs.  -> (refine's result,
    the lg every Schur step was given)."""
    lgs, at, sign = [], [0], [1.0]
    state = {"cost": init_cost}

    def schur_step(U, W, V, ga, gb, lg):
        lgs.append(lg)
        c, dn, pn, bad = attempts[at[0]]
        dp = np.zeros((1, 6))
        dp[0, 1] = INF if bad else sign[0] * math.sqrt(dn)
        return np.zeros(ng), dp

    def trial_costs(g, P):
        c = attempts[at[0]][0]
        at[0] += 1
        if c <= state["prev"]:
            sign[0] = -sign[0]                  # an accepted step: the next one goes back
        state["cost"] = c
        return None if c == INF else np.array([c])

    def normal_blocks(g, P):
        c = state["cost"]
        state["prev"] = c
        if c == INF:
            return None
        return np.zeros((1, 6, 6)), np.zeros((1, ng, 6)), np.zeros((ng, ng)), np.zeros(ng), np.zeros((1, 6)), np.array([c])

    monkeypatch.setattr(_lm, "schur_step", schur_step)
    P0 = np.array([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    out = _lm.refine(np.zeros(ng), P0, normal_blocks, trial_costs, lambda c: float(np.sum(c)), stop_forced, 30, EPS)
    return out, lgs


STOP = (8.0, 0.0, 1.0, False)                  # appended where a script leaves the solve running: the stop test ends it OK


@pytest.mark.parametrize("stop_forced", [False, True])
@pytest.mark.parametrize("ng", [6, 9])
@pytest.mark.parametrize("name", list(SCRIPTS))
def test_host_driver_walks_the_same_scripts(lm_host, monkeypatch, name, ng, stop_forced):
    """Status, accepted steps, attempts and the lg of every Schur step: the program's and refine's are the same, and are what
    the table says."""
    attempts, states = SCRIPTS[name]
    if states[-1][0] != FINISHED:
        attempts = attempts + [STOP]
        code, lg, iters, att, _, _ = states[-1]
        states = states + [(FINISHED, max(lg - 1, -16), iters + 1, att + 1, 2, OK)]
    rows = _run(lm_host, ng, stop_forced, attempts)
    assert [_state(r) for r in rows[1:]] == states
    (status, g, P, vc, iters, att), lgs = _drive(ng, stop_forced, attempts, monkeypatch)
    assert (status, iters, att) == (states[-1][5], states[-1][2], states[-1][3])
    assert lgs == [-3] + [s[1] for s in states[:-1]]
    assert vc is not None and float(vc[0]) == attempts[-1][0]


@pytest.mark.parametrize("ng", [6, 9])
def test_host_driver_forced_non_finite(monkeypatch, ng):
    """Only stop_forced = True: without it the driver has no handling for normal equations that cannot be formed."""
    lg_all = [-3] + [s[1] for s in REJECT19_STATES]
    (status, _, _, vc, iters, att), lgs = _drive(ng, True, REJECT19 + [(INF, 1.0, 1.0, False)], monkeypatch)
    assert (status, iters, att, vc) == (DEGENERATE, 1, 20, None) and lgs == lg_all
    (status, _, _, vc, iters, att), lgs = _drive(ng, True, REJECT19 + [(INF, 1.0, 1.0, True)], monkeypatch)
    assert (status, iters, att, vc) == (NONFINITE, 1, 20, None) and lgs == lg_all
    (status, _, _, vc, iters, att), lgs = _drive(ng, True, REJECT19 + [(INF, 0.0, 1.0, False)], monkeypatch)
    assert (status, iters, att, vc) == (DEGENERATE, 1, 20, None) and lgs == lg_all


@pytest.mark.parametrize("stop_forced", [False, True])
def test_host_driver_init(monkeypatch, stop_forced):
    (status, _, _, vc, iters, att), lgs = _drive(6, stop_forced, [], monkeypatch, init_cost=INF)
    assert (status, iters, att, vc, lgs) == (DEGENERATE, 0, 0, None, [])


# ------------------------------------------------------------------------------------------------ the single-pose loop

EPS32 = 2.0 ** -23                             # FLT_EPSILON, the stop test of the pose solvers
BELOW = math.nextafter(EPS32, 0.0)             # sqrt(fl(s s)) == s for every double s (no over- or underflow): |dp| is the step itself


def _drive_pose(monkeypatch, trials, max_iter, init_cost=INIT_COST, jacobian=None):
    """_lm.refine_pose from p = (1, 0, 0, 0, 0, 0) (|p| = 1) through a toy ``project`` of three points whose J is the identity, so
    the damped matrix is diag(1 + 10^lg).  Trial k = (cost, step, bad): the solve of that trial (as _drive's Schur step) moves
    the pose's second coordinate by ``step`` from the committed point (to NaN for ``bad``), and the toy answers the scripted cost.
    With ``jacobian`` the toy's J is that and _lm's own Cholesky solve runs.  -> (status, accepted steps, trial evaluations,
    evaluations with the Jacobian, the damping of every solve, the final pose, the final cost)."""
    count = {"trial": 0, "jac": 0}
    damp = []

    def solve(A, b):
        damp.append(float(A[0, 0]))
        assert np.array_equal(A, np.diag(np.diag(A))) and np.ptp(np.diag(A)) == 0.0          # every diagonal entry, equally
        _, step, bad = trials[count["trial"]]
        x = np.zeros(6)
        x[1] = NAN if bad else step
        return x

    def project(p, jac):
        if jac:
            count["jac"] += 1
            cost = init_cost if count["trial"] == 0 else trials[count["trial"] - 1][0]
            return np.zeros((3, 2)), cost, np.eye(6) if jacobian is None else jacobian
        count["trial"] += 1
        return None, trials[count["trial"] - 1][0], None

    if jacobian is None:
        monkeypatch.setattr(_lm, "_cholesky_solve", solve)
    status, p, cost, iters = _lm.refine_pose(project, np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0]), max_iter, EPS32)
    return status, iters, count["trial"], count["jac"], damp, p, cost


def _damping(lgs):
    return [1.0 + 10.0 ** lg for lg in lgs]


def test_refine_pose_walks_the_rules(monkeypatch):
    """Expected (status, accepted steps, trials) and the damping of every solve, from the rules in _lm's docstring: lg starts at -3;
    a cost that is not <= the cost before takes lg + 1 and the same point is tried again while lg <= 16; the trial that takes lg
    to 17 is committed whatever it costs; a committed step takes lg - 1, not below -16; ``max_iter`` committed steps at the most;
    stop when |dp| < eps |p| at the point the step left; a damped matrix that is not positive definite, a start whose cost is not
    finite and a final cost of inf are DEGENERATE; a final pose or cost that is NaN is NONFINITE."""
    drive = lambda *a, **kw: _drive_pose(monkeypatch, *a, **kw)
    acc, rej = (9.0, 1.0, False), (11.0, 1.0, False)
    # _lm's own Cholesky solve on J = 0 (a zero pivot): DEGENERATE before anything is tried
    assert drive([], 20, jacobian=np.zeros((6, 6)))[:4] == (DEGENERATE, 0, 0, 1)
    # rejected three times (a higher cost, inf, higher), accepted on an EQUAL cost at lg 0, then the stop test
    st, iters, n, njac, damp, p, cost = drive([(12.0, 1.0, False), (INF, 1.0, False), rej, (10.0, 1.0, False), (9.0, 0.0, False)], 20)
    assert (st, iters, n) == (OK, 2, 5) and damp == _damping([-3, -2, -1, 0, -1]) and njac == 2 and cost == 9.0
    assert p.tolist() == [1.0, -1.0, 0.0, 0.0, 0.0, 0.0]                  # the rejected trials left nothing behind
    # lg -3 .. 16 is twenty trials; the twentieth rejection takes lg to 17 and that trial is the step; then lg 16
    st, iters, n, _, damp, _, cost = drive([rej] * 20 + [(8.0, 0.0, False)], 20)
    assert (st, iters, n) == (OK, 2, 21) and damp == _damping(list(range(-3, 17)) + [16]) and cost == 8.0
    # four rejections and a step accepted at lg 1 leave lg at 0: sixteen rejections (lg 0 .. 15) reach 16, the trial there is
    # rejected too, lg is 17 and it is the step
    st, iters, n, _, damp, _, _ = drive([rej] * 4 + [acc] + [rej] * 17 + [(8.0, 0.0, False)], 20)
    assert (st, iters, n) == (OK, 3, 23) and damp == _damping([-3, -2, -1, 0, 1] + list(range(0, 17)) + [16])
    # the lower clamp: the 14th accepted step is solved at lg -16, and so is the trial after it (from -17 the forced trial would
    # be the 34th, not the 33rd); then five accepted steps reach the cap of 20
    st, iters, n, njac, damp, _, _ = drive([acc] * 14 + [rej] * 33 + [acc] * 5 + [rej], 20)
    assert (st, iters, n, njac) == (OK, 20, 52, 20)
    assert damp == _damping(list(range(-3, -17, -1)) + list(range(-16, 17)) + [16, 15, 14, 13, 12])
    assert damp[12] != damp[13] == 1.0                                    # 1 + 1e-15 is not 1; 1 + 1e-16 is
    # the iteration cap alone, at two sizes; the trial after it is never asked for
    assert drive([acc] * 21, 20)[:3] == (OK, 20, 20) and drive([acc] * 4, 3)[:3] == (OK, 3, 3)
    # the stop test, |p| = 1 at the start: a step of exactly eps is not < eps |p| and the solve goes on; the next double below stops it
    assert drive([(9.0, EPS32, False), (8.0, 1.0, False), (7.0, 0.0, False)], 20)[:3] == (OK, 3, 3)
    assert drive([(9.0, BELOW, False), (8.0, 1.0, False)], 20)[:3] == (OK, 1, 1)
    assert drive([(9.0, 0.0, False)], 20)[:3] == (OK, 1, 1)
    # the endings: a NaN pose, a forced step whose cost is NaN, one whose cost is inf (with the cap and with the stop test ending
    # the solve), a start whose cost is not finite
    st, iters, n, _, _, p, _ = drive([(9.0, 1.0, True)], 1)
    assert (st, iters, n) == (NONFINITE, 1, 1) and np.isnan(p[1])
    assert drive([rej] * 19 + [(NAN, 1.0, False)], 1)[:3] == (NONFINITE, 1, 20)
    assert drive([rej] * 19 + [(INF, 1.0, False)], 1)[:3] == (DEGENERATE, 1, 20)
    assert drive([rej] * 19 + [(INF, 0.0, False)], 20)[:3] == (DEGENERATE, 1, 20)
    for c in (INF, NAN):
        assert drive([], 20, init_cost=c)[:5] == (DEGENERATE, 0, 0, 1, [])
