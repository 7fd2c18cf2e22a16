"""Closed-loop batches (DGSQP.step_batch / dgsqp_closed_loop_batch), the parts that need no GPU: the symbol is declared, exported by both
builds and bound with the header's argument count; the host mirror of the feedback rule (dgsqp_amd/closed_loop.py) is the rule of
DGSQP.step() (DGSQP.py:283-297)."""
import ctypes
import pathlib
import re
import types

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _declaration():
    text = (ROOT / 'include' / 'dgsqp.h').read_text()
    m = re.search(r'int\s+dgsqp_closed_loop_batch\s*\((.*?)\)\s*;', text, re.S)
    assert m, 'dgsqp_closed_loop_batch is not declared in include/dgsqp.h'
    return text, re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)


def test_symbol_is_declared_exported_by_both_builds_and_bound():
    from dgsqp_amd import _ffi
    from dgsqp_amd.csrc import build
    text, args = _declaration()
    assert re.search(r'#define\s+DGSQP_NOT_RUN\s+\(-1\)', text) and _ffi.NOT_RUN == -1
    n_args = len([a for a in args.split(',') if a.strip()])
    assert n_args == 18
    assert 'dgsqp_closed_loop_batch' in _ffi.EXPORTED_SYMBOLS
    assert (build.HERE / 'dgsqp_closed_loop.h') in build.DEPS             # a change of the kernel rebuilds the libraries
    build.build()
    for wg in (1, 2):
        lib = ctypes.CDLL(str(_ffi.library_path(wg)))                     # loads without a GPU
        assert lib.dgsqp_closed_loop_batch is not None
        bound = _ffi.load_library(wg).dgsqp_closed_loop_batch
        assert len(bound.argtypes) == n_args and bound.restype is ctypes.c_int


def _agent_major(u_tm, M, N):
    """DGSQP._to_agent_major (what step() feeds set_warm_start through) without a device handle."""
    from dgsqp_amd.solver import DGSQP
    return DGSQP._to_agent_major(types.SimpleNamespace(N=N, num_ua_d=[2] * M), u_tm)


@pytest.mark.parametrize('M', [1, 2, 3])
@pytest.mark.parametrize('N', [2, 5])
def test_shift_warm_start_is_the_vstack_of_step(M, N):
    from dgsqp_amd import closed_loop
    nua = [2] * M
    rng = np.random.default_rng(100 * M + N)
    u_tm = rng.standard_normal((N, 2 * M))
    want = _agent_major(np.vstack((u_tm[1:], u_tm[-1])), M, N)           # solver.py: step()
    got = closed_loop.shift_warm_start(_agent_major(u_tm, M, N), N, nua)
    assert got.shape == want.shape == (2 * M * N,) and np.array_equal(got, want)
    # ... and batched, with leading axes
    U = rng.standard_normal((3, 2, N, 2 * M))
    wantB = _agent_major(np.concatenate((U[..., 1:, :], U[..., -1:, :]), axis=-2), M, N)
    assert np.array_equal(closed_loop.shift_warm_start(_agent_major(U, M, N), N, nua), wantB)
    with pytest.raises(ValueError):
        closed_loop.shift_warm_start(np.zeros(2 * M * N + 1), N, nua)


def test_feedback_on_hand_made_arrays():
    from dgsqp_amd import closed_loop
    N, M, nq = 3, 2, 4
    B = 6
    status = np.array([0, 1, 2, 3, 4, 5], np.int32)
    x = np.arange(B * (N + 1) * nq, dtype=float).reshape(B, N + 1, nq)
    u = 100.0 + np.arange(B * 2 * M * N, dtype=float).reshape(B, 2 * M * N)
    prev = -1.0 - np.arange(B * 2 * M * N, dtype=float).reshape(B, 2 * M * N)
    q, ws, ok = closed_loop.feedback(x, u, status, prev)
    assert np.array_equal(q, x[:, 1]) and ok.all()
    # agent-major, N = 3 rows of 2 per agent: rows (0, 1, 2) -> (1, 2, 2)
    idx = np.array([2, 3, 4, 5, 4, 5, 8, 9, 10, 11, 10, 11])
    for b in (0, 1, 2, 5):                                                # every status but 'diverged' and 'qp_fail' shifts
        assert np.array_equal(ws[b], u[b, idx]), b
    for b in (3, 4):                                                      # those two keep the warm start the solve started from
        assert np.array_equal(ws[b], prev[b]), b
    # the disturbance is one fp64 add
    w = 1e-3 * np.random.default_rng(0).standard_normal((B, nq))
    q2, ws2, ok2 = closed_loop.feedback(x, u, status, prev, w=w)
    assert np.array_equal(q2, x[:, 1] + w) and np.array_equal(ws2, ws) and ok2.all()
    # a non-finite next state is reported, from the plant or from the disturbance, per scenario
    w[1, 2] = np.nan
    x[4, 1, 0] = np.inf
    _, _, ok3 = closed_loop.feedback(x, u, status, prev, w=w)
    assert ok3.tolist() == [True, False, True, True, False, True]
    # a single scenario, without a batch axis
    q1, ws1, ok1 = closed_loop.feedback(x[0], u[0], status[0], prev[0])
    assert np.array_equal(q1, x[0, 1]) and np.array_equal(ws1, u[0, idx]) and bool(ok1) is True
