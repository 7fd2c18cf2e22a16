"""The launch streams of the C-ABI host layer (csrc/dgsqp_api.hip, DgLaunchStreams): dg_solve_kernel launches run on a small pool of
streams per device, taken round robin in launch order, so that launches in flight sit on different hardware queues whichever handles
lead them.  Scheduling only: every output equals the same solve made alone, bit for bit."""
import ctypes as C
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ('u', 'l', 'x', 'status', 'num_iters', 'qp_solves', 'cond', 'cost')


def pool_streams():
    """K of the library: min(GPU_MAX_HW_QUEUES of the process, 8); 4 queues when unset or unparsable."""
    try:
        q = int(os.environ.get('GPU_MAX_HW_QUEUES', ''))
    except ValueError:
        q = 0
    return min(q if q >= 1 else 4, 8)


def make(g, count):
    from dgsqp_amd.solver import DGSQP
    return [DGSQP(*g.solver_args(), print_method=None) for _ in range(count)]


def stage(s, x0, u_ws):
    from dgsqp_amd import _ffi
    x0, u_am = s._inputs(x0, u_ws)
    assert s._lib.dgsqp_stage_inputs(s._h, x0.shape[0], _ffi.dptr(x0), _ffi.dptr(u_am)) == 0, s._lib.dgsqp_last_error(s._h)
    return x0.shape[0]


def launch(s):
    assert s._lib.dgsqp_launch_staged(s._h) == 0, s._lib.dgsqp_last_error(s._h)


def wait(s):
    from dgsqp_amd import _ffi
    tm = _ffi.TimingT()
    assert s._lib.dgsqp_wait(s._h, C.byref(tm)) == 0, s._lib.dgsqp_last_error(s._h)
    return tm.kernel_ms


def fetch(s, B):
    from dgsqp_amd.solver import _record_ptrs
    out = s._records((B,))
    assert s._lib.dgsqp_fetch_results(s._h, *_record_ptrs(out)) == 0, s._lib.dgsqp_last_error(s._h)
    return out


def solve_alone(s, x0, u_ws):
    """stage, launch, wait, fetch with nothing else in flight: (results, kernel_ms)"""
    B = stage(s, x0, u_ws)
    launch(s)
    ms = wait(s)
    return fetch(s, B), ms


def assert_same(res, ref, what):
    for k in KEYS:
        assert np.array_equal(res[k], ref[k], equal_nan=True), (what, k)


def test_a_short_launch_overtakes_the_tail_of_a_long_one(games):
    """Launch A (1,024 scenarios of configs[1], no cooperative helpers: its workgroups exit when the queue is empty) ends behind its
    slowest scenario; launch B (64 copies of A's shortest converged scenario), started once A has handed out its last scenario, must
    finish while A is still running -- whichever of four later handles stages it."""
    from dgsqp_amd.montecarlo import sample_scenarios
    g = games['dyn_curve_N25'][0]
    S = make(g, 5)
    lib, A = S[0]._lib, S[0]
    A.set_cooperative(0)
    xa, ua = sample_scenarios(g, 1024, seed=1, solver=A)
    ref_a, t_a = solve_alone(A, xa, ua)
    conv = np.nonzero((ref_a['status'] >= 0) & (ref_a['status'] <= 1))[0]
    short = conv[np.argmin(ref_a['num_iters'][conv])]
    xb, ub = np.repeat(xa[short:short + 1], 64, axis=0), np.repeat(ua[short:short + 1], 64, axis=0)
    ref_b, t_b = solve_alone(S[1], xb, ub)
    print(f'T_A {t_a:.1f} ms, T_B {t_b:.1f} ms (scenario {short}: {ref_a["num_iters"][short]} iterations)')
    assert t_a >= 5.0 * t_b, (t_a, t_b)           # precondition of the set-up
    stage(A, xa, ua)
    for k in range(1, 5):
        stage(S[k], xb, ub)
        launch(A)
        deadline = time.perf_counter() + 5.0
        while not lib.dgsqp_draining(A._h) and time.perf_counter() < deadline:
            time.sleep(0.0002)
        assert lib.dgsqp_draining(A._h)
        launch(S[k])
        deadline = time.perf_counter() + 30.0
        while True:
            b_done = lib.dgsqp_finished(S[k]._h)         # (B first: "B done, and then A still running")
            a_done = lib.dgsqp_finished(A._h)
            if a_done or b_done or time.perf_counter() > deadline:
                break
            time.sleep(0.0002)
        ms_b, ms_a = wait(S[k]), wait(A)
        print(f'handle {k}: B finished {bool(b_done)}, A finished {bool(a_done)}; kernel ms A {ms_a:.1f} B {ms_b:.1f}')
        assert b_done and not a_done, (k, b_done, a_done)
        assert_same(fetch(A, 1024), ref_a, ('A', k))
        assert_same(fetch(S[k], 64), ref_b, ('B', k))


def test_more_launches_in_flight_than_launch_streams(games):
    """2K + 1 launches back to back without a wait, collected in reverse order: launches j and j - K share a stream."""
    from dgsqp_amd.montecarlo import sample_scenarios
    g = games['kb_chicane_N15'][0]
    n = 2 * pool_streams() + 1
    S = make(g, n)
    data = [sample_scenarios(g, 64, seed=70 + j) for j in range(n)]
    refs = [solve_alone(s, *d)[0] for s, d in zip(S, data)]
    for s, d in zip(S, data):
        stage(s, *d)
    t0 = time.perf_counter()
    for s in S:
        launch(s)
    ms = [wait(s) for s in reversed(S)][::-1]
    wall_ms = (time.perf_counter() - t0) * 1e3
    print(f'{n} launches in {wall_ms:.1f} ms, kernel ms', [round(m, 2) for m in ms])
    assert all(0.0 < m <= wall_ms for m in ms), (ms, wall_ms)
    for j, (s, ref) in enumerate(zip(S, refs)):
        assert_same(fetch(s, 64), ref, j)


def test_three_grouped_launches_in_flight(games):
    """Three groups of two handles, launched back to back: every member waits for, and reports, its own group's kernel."""
    from dgsqp_amd import _ffi
    from dgsqp_amd.montecarlo import sample_scenarios
    g = games['kb_chicane_N15'][0]
    S = make(g, 6)
    lib = S[0]._lib
    sizes = [64, 64, 150, 150, 96, 96]              # (a group's batches have one size)
    data = [sample_scenarios(g, b, seed=80 + j) for j, b in enumerate(sizes)]
    refs = [solve_alone(s, *d)[0] for s, d in zip(S, data)]
    for s, d in zip(S, data):
        stage(s, *d)
    for i in (0, 2, 4):
        arr = (C.c_void_p * 2)(S[i]._h, S[i + 1]._h)
        assert lib.dgsqp_launch_staged_group(arr, 2) == 0, lib.dgsqp_last_error(S[i]._h)
    ev_ms = []
    for i in (4, 0, 2):                               # members first, out of launch order
        m_ms = wait(S[i + 1])
        assert lib.dgsqp_finished(S[i]._h) == 1 and lib.dgsqp_finished(S[i + 1]._h) == 1
        l_ms = wait(S[i])
        assert m_ms > 0.0 and m_ms == l_ms, (i, m_ms, l_ms)          # the same pair of events
        ev_ms.append(l_ms)
    print('grouped launches, kernel ms', ev_ms)
    tm = _ffi.TimingT()
    for j, (s, ref) in enumerate(zip(S, refs)):
        assert lib.dgsqp_wait(s._h, C.byref(tm)) == 0 and tm.grid > 0
        assert_same(fetch(s, sizes[j]), ref, j)


def test_synchronous_calls_while_a_launch_is_in_flight(games):
    """solve_batch (fp64 and fp32 boundary), a device-sampled staged batch and step_batch on one handle while another handle's
    asynchronous launch is in flight: the same results as with nothing in flight."""
    from dgsqp_amd import _ffi
    from dgsqp_amd.montecarlo import sample_scenarios
    g = games['kb_chicane_N15'][0]
    A, Bh = make(g, 2)
    xa, ua = sample_scenarios(g, 1024, seed=90)
    ref_a = solve_alone(A, xa, ua)[0]
    x, u = sample_scenarios(g, 64, seed=91)
    tm = _ffi.TimingT()

    def sampled():
        Bh.sample_batch(g, 64, seed=17, stage=True, fetch=False)
        assert Bh._lib.dgsqp_solve_staged(Bh._h, C.byref(tm)) == 0, Bh._lib.dgsqp_last_error(Bh._h)
        return fetch(Bh, 64)
    calls = [('fp64', lambda: Bh.solve_batch(x, u)), ('fp32', lambda: Bh.solve_batch(x, u, dtype=np.float32)), ('sampled', sampled),
             ('step_batch', lambda: Bh.step_batch(x[:8], u[:8], 2, keep_predictions=True))]
    refs = [f() for _, f in calls]
    stage(A, xa, ua)
    for (name, f), ref in zip(calls, refs):
        launch(A)
        res = f()
        in_flight = not A._lib.dgsqp_finished(A._h)
        wait(A)
        print(name, 'launch A still in flight after the call:', in_flight)
        for k in KEYS + (('q', 'u_ws', 'steps_done') if name == 'step_batch' else ()):
            assert np.array_equal(res[k], ref[k], equal_nan=True), (name, k)
        assert_same(fetch(A, 1024), ref_a, ('A', name))


def test_destroy_with_launches_in_flight(games):
    """dgsqp_destroy of a handle whose launch is in flight, next to another handle's launch in flight, waits for its own launch and
    leaves the launch streams to the others: the survivor's results and a new handle's are what they are alone."""
    from dgsqp_amd.montecarlo import sample_scenarios
    g = games['kb_chicane_N15'][0]
    A, Bh = make(g, 2)
    xa, ua = sample_scenarios(g, 512, seed=95)
    xb, ub = sample_scenarios(g, 512, seed=96)
    ref_a, ref_b = solve_alone(A, xa, ua)[0], solve_alone(Bh, xb, ub)[0]
    stage(A, xa, ua)
    stage(Bh, xb, ub)
    launch(A)
    launch(Bh)
    A.__del__()                                       # dgsqp_destroy(A) with both in flight
    Cn = make(g, 1)[0]
    assert_same(solve_alone(Cn, xa, ua)[0], ref_a, 'new handle')
    assert wait(Bh) > 0.0
    assert_same(fetch(Bh, 512), ref_b, 'survivor')
    Bh.__del__()                                      # ... and with the last-but-one handle gone, the pool still serves the one left
    assert_same(Cn.solve_batch(xa, ua), ref_a, 'new handle, again')
