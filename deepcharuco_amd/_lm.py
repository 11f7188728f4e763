"""The joint Levenberg-Marquardt driver of the two calibration definitions (``calib.py`` over 9 intrinsics, ``stereo.py`` over the 6
rig parameters), one copy: g holds the global parameters, P [N, 6] one pose per unit (a view, a pair) that couples only to g.
csrc/dcx_lm_dev.h is the same driver for the kernels; tests/test_lm_host.py walks both through the same scripts.  ``refine_pose`` is
the same loop over one pose alone (``pnp._solve``, ``fisheye._solve``, ``rig.rig_pose_host_full``), and the small Cholesky solve
both loops use is here too: this module imports no solver.

The CvLevMarq rules: damping diag * (1 + 10^lg), lg from -3; a step whose cost is not <= the cost before is rejected: lg + 1 and
the same point is tried again, up to lg = 16; at 17 the step is taken whatever it costs (forced); an accepted or forced step takes
lg - 1, down to -16; at most ``max_iter`` accepted steps; stop at |dp| < eps |p| over all parameters.
"""
from __future__ import annotations

import math

import numpy as np

# the overall status: calib's CALIB_* and stereo's STEREO_* are these numbers (include/deepcharuco_amd.h)
LM_OK, LM_NO_UNITS, LM_DEGENERATE, LM_NONFINITE = range(4)


def _cholesky_solve(A: np.ndarray, b: np.ndarray):
    """A x = b by the Cholesky factor of A, in the kernels' order of operations -> x, or None if A is not positive definite."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for i in range(n):
        for j in range(i + 1):
            s = A[i, j] - float(L[i, :j] @ L[j, :j])
            if i == j:
                if not s > 0:
                    return None
                L[i, i] = math.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - float(L[i, :i] @ y[:i])) / L[i, i]
    x = np.zeros(n)
    for i in reversed(range(n)):
        x[i] = (y[i] - float(L[i + 1:, i] @ x[i + 1:])) / L[i, i]
    return x


def schur_step(U, W, V, ga, gb, lg: int):
    """Solve [V* W; W^T U*] [dg; dP] = [ga; gb] with the diagonals of V and of every U_i scaled by 1 + 10^lg (Marquardt), by
    eliminating the pose blocks: S = V* - sum W_i U_i*^-1 W_i^T, dg = S^-1 (ga - sum W_i U_i*^-1 gb_i),
    dP_i = U_i*^-1 (gb_i - W_i^T dg).  U [N, 6, 6], W [N, n, 6], V [n, n] for any n.  -> (dg [n], dP [N, 6]), or None if a block is
    not positive definite."""
    s = 1.0 + 10.0 ** lg
    Us = U.copy()
    d6 = np.arange(6)
    Us[:, d6, d6] *= s
    try:
        np.linalg.cholesky(Us)
    except np.linalg.LinAlgError:
        return None
    Y = np.linalg.solve(Us, W.transpose(0, 2, 1))                  # U_i*^-1 W_i^T  [N, 6, n]
    z = np.linalg.solve(Us, gb[:, :, None])[:, :, 0]              # U_i*^-1 gb_i   [N, 6]
    S = V.copy()
    S[np.diag_indices(V.shape[0])] *= s
    S -= np.einsum("nij,njk->ik", W, Y)
    rhs = ga - np.einsum("nij,nj->i", W, z)
    dg = _cholesky_solve(S, rhs)
    if dg is None:
        return None
    return dg, z - np.einsum("nij,j->ni", Y, dg)


def _spd_inverse(A):
    """The inverse of symmetric positive definite matrices [..., n, n] through their Cholesky factors (L^-T L^-1: symmetric to the
    bit), or None if one of them is not positive definite or not finite."""
    if not np.isfinite(A).all():
        return None
    try:
        Li = np.linalg.inv(np.linalg.cholesky(A))
    except np.linalg.LinAlgError:
        return None
    inv = np.swapaxes(Li, -1, -2) @ Li
    return inv if np.isfinite(inv).all() else None


def schur_covariance(U, W, V, costs):
    """The covariance blocks of a solved joint problem from its UNDAMPED normal blocks (``schur_step``'s U [N, 6, 6], W [N, n, 6],
    V [n, n]; ``costs`` the units' costs), by the elimination ``schur_step`` solves with: S = V - sum W_i U_i^-1 W_i^T,
    Y_i = U_i^-1 W_i^T; the inverse of the full normal matrix has S^-1 as its global corner and U_i^-1 + Y_i S^-1 Y_i^T as unit i's
    6x6 diagonal block.  -> (S^-1 [n, n], the units' blocks [N, 6, 6]), both without the factor sigma^2 (the caller's: its degrees
    of freedom are its own), or None if a U_i or S is not positive definite or something is not finite.  csrc/dcx_calib_cov.hip
    runs the same steps per camera model; the stereo and rig solvers have the same block structure."""
    if not np.isfinite(np.asarray(costs, np.float64)).all() or not np.isfinite(W).all():
        return None
    Ui = _spd_inverse(U)
    if Ui is None:
        return None
    Y = Ui @ W.transpose(0, 2, 1)                                  # U_i^-1 W_i^T  [N, 6, n]
    Si = _spd_inverse(V - np.einsum("nij,njk->ik", W, Y))
    if Si is None:
        return None
    P = Ui + Y @ Si @ Y.transpose(0, 2, 1)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    if not np.isfinite(P).all():
        return None
    return Si, P


def refine(g, P, normal_blocks, trial_costs, total, stop_forced: bool, max_iter: int, eps: float, constrain=None):
    """-> (status LM_*, g, P, the units' costs at the solution or None, accepted steps, attempts).

    ``normal_blocks(g, P)`` -> (U, W, V, ga, gb, costs) as ``schur_step`` takes them, or None if a point is behind a camera;
    ``trial_costs(g, P)`` -> the units' costs, or None for the same reason (the cost is then inf); ``total(costs)`` adds them up
    in the caller's order.  ``stop_forced``: a step forced at lg > 16 that leaves a point behind a camera ends the solve
    (DEGENERATE, NONFINITE if a parameter is not finite): there are no normal equations to go on from.  Without it that case is
    not handled here (``normal_blocks`` must not answer None after an accepted step).  ``constrain(g)`` -> the trial g with the
    caller's ties between global parameters restored (calibration's fx = a fy); None: the trial g is taken as it is."""
    blocks = normal_blocks(g, P)
    if blocks is None or not math.isfinite(total(blocks[5])):
        return LM_DEGENERATE, g, P, None, 0, 0
    vc = blocks[5]
    prev_cost, lg, iters, attempts = total(vc), -3, 0, 0
    while True:
        U, W, V, ga, gb, _ = blocks
        prev_g, prev_p = g, P
        while True:
            step = schur_step(U, W, V, ga, gb, lg)
            if step is None:
                return LM_DEGENERATE, g, P, None, iters, attempts
            g, P = prev_g - step[0], prev_p - step[1]
            if constrain is not None:
                g = constrain(g)
            vc = trial_costs(g, P)
            cost = total(vc) if vc is not None else math.inf
            attempts += 1
            if not cost <= prev_cost:              # (a point behind a camera: cost = inf, rejected like an increase)
                lg += 1
                if lg <= 16:
                    continue
            break
        lg = max(lg - 1, -16)
        iters += 1
        d = np.r_[g - prev_g, (P - prev_p).ravel()]
        pv = np.r_[prev_g, prev_p.ravel()]
        if iters >= max_iter or math.sqrt(float(d @ d)) < eps * math.sqrt(float(pv @ pv)):
            break
        prev_cost = cost
        blocks = normal_blocks(g, P)
        if blocks is None and stop_forced:         # forced at lg > 16 with a point behind a camera: nothing to go on from
            bad = not (np.isfinite(g).all() and np.isfinite(P).all())
            return (LM_NONFINITE if bad else LM_DEGENERATE), g, P, None, iters, attempts
    if not (np.isfinite(g).all() and np.isfinite(P).all()) or math.isnan(cost):
        return LM_NONFINITE, g, P, None, iters, attempts
    if not math.isfinite(cost):
        return LM_DEGENERATE, g, P, None, iters, attempts
    return LM_OK, g, P, vc, iters, attempts


def refine_pose(project, p, max_iter: int, eps: float):
    """The rules above over one pose p (6) alone -> (status LM_*, p, cost, accepted steps).  ``project(p, jac)`` -> (residuals,
    cost, J [2N, 6] with ``jac``); a cost of inf (a point behind its camera) rejects a trial like an increase.  A start whose cost
    is not finite and a damped matrix that is not positive definite are DEGENERATE."""
    res, cost, J = project(p, True)
    if not math.isfinite(cost):
        return LM_DEGENERATE, p, cost, 0
    prev_cost, lg, iters = cost, -3, 0
    while True:
        JtJ, Jtr = J.T @ J, J.T @ res.ravel()
        prev = p
        while True:
            A = JtJ.copy()
            A[np.diag_indices(6)] *= 1.0 + 10.0 ** lg
            x = _cholesky_solve(A, Jtr)
            if x is None:
                return LM_DEGENERATE, p, cost, iters
            p = prev - x
            _, cost, _ = project(p, False)
            if not cost <= prev_cost:
                lg += 1
                if lg <= 16:
                    continue
            break
        lg = max(lg - 1, -16)
        iters += 1
        if iters >= max_iter or math.sqrt(float((p - prev) @ (p - prev))) < eps * math.sqrt(float(prev @ prev)):
            break
        prev_cost = cost
        res, cost, J = project(p, True)
    if not np.isfinite(p).all() or math.isnan(cost):
        return LM_NONFINITE, p, cost, iters
    if not math.isfinite(cost):
        return LM_DEGENERATE, p, cost, iters
    return LM_OK, p, cost, iters
