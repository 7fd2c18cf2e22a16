"""The feedback rule between two steps of a closed-loop (receding-horizon) run, on the host.

This is the documented mirror of what ``dg_closed_loop_kernel`` (csrc/dgsqp_closed_loop.h) does between two solves of one chain and
of what ``DGSQP.step()`` does for a single scenario (reference DGSQP.py:283-297):

* the plant is the game's own discrete model: the next state is stage 1 of the prediction, plus an optional disturbance (one fp64 add);
* the next warm start is the solution shifted by one stage per agent with the last row repeated --
  ``np.vstack((u_pred[1:], u_pred[-1]))`` -- unless the solve ended 'diverged' or 'qp_fail': then the warm start it started from is kept.

Everything here is exact data movement apart from that one add, so device and host agree bit for bit."""
from __future__ import annotations

import numpy as np

DIVERGED, QP_FAIL = 3, 4        # include/dgsqp.h: the exit codes after which step() does not shift the warm start
NUA = 2                         # every vehicle model has two inputs (DGSQP_NUA)


def shift_warm_start(u_am: np.ndarray, N: int, num_ua_d) -> np.ndarray:
    """``u_am`` [..., n] agent-major (agent a: N rows of ``num_ua_d[a]`` inputs) -> the same layout with every agent's rows moved up
    by one stage and its last row repeated."""
    u_am = np.asarray(u_am, dtype=np.float64)
    if u_am.shape[-1] != N * int(sum(num_ua_d)):
        raise ValueError(f'u_am has {u_am.shape[-1]} entries per scenario, expected {N * int(sum(num_ua_d))}')
    parts, si = [], 0
    for nu in num_ua_d:
        blk = u_am[..., si:si + N * nu].reshape(*u_am.shape[:-1], N, nu)
        parts.append(np.concatenate((blk[..., 1:, :], blk[..., -1:, :]), axis=-2).reshape(*u_am.shape[:-1], N * nu))
        si += N * nu
    return np.concatenate(parts, axis=-1)


def feedback(x_pred: np.ndarray, u_am: np.ndarray, status, u_ws_prev: np.ndarray, w=None, num_ua_d=None):
    """One feedback step for a batch (or a single scenario: no leading axis).

    ``x_pred`` [..., N+1, n_q] prediction of the solve, ``u_am`` [..., n] its solution (agent-major), ``status`` [...] its exit code,
    ``u_ws_prev`` [..., n] the warm start it started from, ``w`` [..., n_q] disturbance or None.  ``num_ua_d``: inputs per agent
    (default: two each).  Returns ``(q_next [..., n_q], u_ws_next [..., n], finite [...])``; a chain whose ``finite`` is False ends."""
    x_pred = np.asarray(x_pred, dtype=np.float64)
    u_am = np.asarray(u_am, dtype=np.float64)
    u_ws_prev = np.asarray(u_ws_prev, dtype=np.float64)
    status = np.asarray(status)
    N = x_pred.shape[-2] - 1
    if num_ua_d is None:
        num_ua_d = [NUA] * (u_am.shape[-1] // (N * NUA))
    q_next = x_pred[..., 1, :].copy()
    if w is not None:
        q_next = q_next + np.asarray(w, dtype=np.float64)
    keep = (status == DIVERGED) | (status == QP_FAIL)
    u_ws_next = np.where(keep[..., None], u_ws_prev, shift_warm_start(u_am, N, num_ua_d))
    return q_next, u_ws_next, np.isfinite(q_next).all(axis=-1)
