"""The host layer of the C-ABI (csrc/dgsqp_api.hip below its kernels, solver.py): what one handle keeps between calls -- record
buffers that grow and are reused, the two logs, the closed-loop buffers, group membership -- must never show in a result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RECORDS = ('u', 'l', 'x', 'cond', 'cost', 'status', 'num_iters', 'qp_solves')
CLOSED_LOOP = RECORDS + ('q', 'u_ws', 'steps_done', 'u_pred', 'u_applied', 'converged')


def raw_trace(s, B, cap):
    """Per scenario (event count, the recorded (code, value) pairs), read through the C-ABI: DGSQP.fetch_trace refuses a log that holds
    more events than its capacity, and 64 pairs are fewer than most solves produce; the pairs past the count are never written."""
    from dgsqp_amd import _ffi
    raw = np.zeros((B, 1 + 2 * cap))
    assert s._lib.dgsqp_fetch_trace(s._h, _ffi.dptr(raw), raw.size) == 0, s._lib.dgsqp_last_error(s._h)
    return [(int(raw[b, 0]), raw[b, 1:1 + 2 * min(int(raw[b, 0]), cap)].copy()) for b in range(B)]


def test_one_handle_through_every_entry_point(games):
    """One long-lived DGSQP object goes through every entry point of the host layer in turn; each call must return exactly what the same
    call returns on a handle created for that call alone (np.array_equal on every array of the result and on the logs)."""
    from dgsqp_amd.montecarlo import sample_scenarios
    from dgsqp_amd.solver import DGSQP, solve_batches
    g = games['kb_chicane_N15'][0]
    make = lambda: DGSQP(*g.solver_args(), print_method=None)
    old = make()
    scen = lambda B, seed: sample_scenarios(g, B, seed=seed)

    def same_records(got, ref, keys, tag, equal_nan=False):
        for k in keys:
            if k in ref or k in got:
                assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (tag, k)
                assert np.array_equal(got[k], ref[k], equal_nan=equal_nan and got[k].dtype.kind == 'f'), (tag, k)
        assert got['msg'] == ref['msg'], tag

    def solve(B, seed, tag, **kw):
        x0, u_ws = scen(B, seed)
        got, ref = old.solve_batch(x0, u_ws, **kw), make().solve_batch(x0, u_ws, **kw)
        assert got['u'].shape == (B, old.n)
        same_records(got, ref, RECORDS + ('u_pred', 'converged'), tag)

    solve(3, 101, 'B=3')
    solve(9, 102, 'B=9 (growth)')
    solve(2, 103, 'B=2 (larger buffers reused)')

    def with_iterate_log(s):
        s.set_iterate_log(4)
        res = s.solve_batch(*scen(5, 104))
        log = s.fetch_iterate_log(5)
        s.set_iterate_log(0)
        return res, log
    (got, glog), (ref, rlog) = with_iterate_log(old), with_iterate_log(make())
    same_records(got, ref, RECORDS, 'iterate log')
    assert len(glog) == len(rlog) == 5
    for (gu, gl), (ru, rl) in zip(glog, rlog):
        assert np.array_equal(gu, ru) and np.array_equal(gl, rl)

    def with_trace(s):
        s.set_trace(64)
        res = s.solve_batch(*scen(7, 105))
        log = raw_trace(s, 7, 64)
        s.set_trace(0)
        return res, log
    (got, glog), (ref, rlog) = with_trace(old), with_trace(make())
    same_records(got, ref, RECORDS, 'trace')
    assert len(glog) == len(rlog) == 7
    for (gn, gp), (rn, rp) in zip(glog, rlog):
        assert gn == rn and gn > 0 and np.array_equal(gp, rp)

    solve(4, 106, 'float32', dtype=np.float32)

    def steps(B, T, seed, tag, **kw):
        x0, u_ws = scen(B, seed)
        got, ref = old.step_batch(x0, u_ws, T, **kw), make().step_batch(x0, u_ws, T, **kw)
        assert sorted(got) == sorted(ref), tag
        same_records(got, ref, CLOSED_LOOP, tag, equal_nan=True)
    steps(3, 2, 107, 'step_batch B=3 T=2')
    w = 1e-3 * np.random.default_rng(108).standard_normal((5, 3, old.n_q))
    steps(5, 3, 109, 'step_batch B=5 T=3 (closed-loop growth)', keep_predictions=True, disturbance=w)

    batches = [scen(4, 110), scen(4, 111)]
    got2, ref2 = solve_batches([old, make()], batches), solve_batches([make(), make()], batches)
    for i, (got, ref) in enumerate(zip(got2, ref2)):
        same_records(got, ref, RECORDS + ('u_pred', 'converged'), f'solve_batches[{i}]')

    x0, u_ws = scen(2, 112)
    u_am = old._to_agent_major(u_ws)
    got, ref = old.evaluate_batch(x0, u_am), make().evaluate_batch(x0, u_am)
    assert sorted(got) == sorted(ref) == ['G', 'Q', 'g', 'l0', 'q', 'x']
    for k in ref:
        assert np.array_equal(got[k], ref[k]), ('evaluate_batch', k)
    l0 = ref['l0']
    got, ref = old.qp_batch(x0, u_am, l0), make().qp_batch(x0, u_am, l0)
    assert sorted(got) == sorted(ref) == ['Qpd', 'du', 'flag', 'info', 'lhat']
    for k in ref:
        assert np.array_equal(got[k], ref[k]), ('qp_batch', k)

    solve(9, 113, 'B=9 (last)')


def test_one_handle_through_every_closed_loop_setting(games):
    """One long-lived DGSQP object runs step_batch launches whose shapes go up and down and whose settings change from launch to launch;
    every key of every result must equal, bit for bit, the same launch on a handle created for it alone.  After the smaller launches the
    fetchers are called through the C-ABI with exactly that launch's size: a side buffer that only grows must not make them ask for more,
    and they return that launch's data."""
    from closed_loop_checks import DELAYS, configs_of, same
    from dgsqp_amd import _ffi
    from dgsqp_amd.closed_loop import Drivers, PlantModel, perturbed_configs
    from dgsqp_amd.montecarlo import sample_scenarios
    from dgsqp_amd.solver import DGSQP
    g = games['kb_curve_N10'][0]
    make = lambda: DGSQP(*g.solver_args(), print_method=None)
    old = make()
    kw = dict(method='rk4', M=2, sim_steps=2)
    plain = PlantModel(delay_steps=DELAYS, **kw)
    rng = np.random.default_rng(7)

    def per_chain(B):
        return PlantModel(per_chain_configs=perturbed_configs(configs_of(g), dict(mass=0.2), B, seed=B), per_chain_delay_steps=rng.integers(0, 4, size=(B, 2, 2)), **kw)

    def noise(B, T):
        return 1e-2 * rng.standard_normal((B, T, old.n_q))

    def replay(B, T):
        rep = np.zeros((B, T, old.n_u))
        rep[:, :, 2:4] = [0.3, 0.02]
        return Drivers(kinds=['game', 'replay'], u_replay=rep)

    def everything(B, T):
        return dict(plant=per_chain(B), estimate_noise=noise(B, T), monitor='stop', drivers=Drivers(kinds=['pid', 'replay'], u_replay=replay(B, T).u_replay))

    def fetched(name, shape):
        """What dgsqp_fetch_<name> returns into a buffer of exactly the last launch's size, scenario-major."""
        buf = np.empty(shape)
        assert getattr(old._lib, 'dgsqp_fetch_' + name)(old._h, _ffi.dptr(buf), buf.size) == 0, (name, old._lib.dgsqp_last_error(old._h))
        return buf.swapaxes(0, 1)

    launches = [((5, 3), 'everything at once', everything),
                ((2, 2), 'plain plant with delays', lambda B, T: dict(plant=plain)),
                ((7, 1), 'vehicles and delays per chain', lambda B, T: dict(plant=per_chain(B))),
                ((5, 3), 'estimates', lambda B, T: dict(plant=plain, estimate_noise=noise(B, T))),
                ((2, 2), 'estimates and monitor', lambda B, T: dict(plant=plain, estimate_noise=noise(B, T), monitor=True)),
                ((7, 1), "monitor 'stop'", lambda B, T: dict(plant=per_chain(B), monitor='stop')),
                ((5, 3), 'PID driver on one car', lambda B, T: dict(plant=plain, drivers=Drivers(kinds=['game', 'pid']))),
                ((2, 2), 'replay', lambda B, T: dict(plant=plain, drivers=replay(B, T))),
                ((7, 1), 'no setting', lambda B, T: {}),
                ((5, 3), 'everything at once, again', everything)]
    for i, ((B, T), tag, settings) in enumerate(launches):
        x0, u_ws = sample_scenarios(g, B, seed=120 + i)
        args = settings(B, T)
        got, ref = old.step_batch(x0, u_ws, T, keep_predictions=True, **args), make().step_batch(x0, u_ws, T, keep_predictions=True, **args)
        assert sorted(got) == sorted(ref), tag
        for k in ref:
            if k not in ('time', 'kernel_ms'):
                assert same(got[k], ref[k]) if isinstance(ref[k], np.ndarray) else got[k] == ref[k], (tag, k)
        added = dict(u_plant='plant', q_est='estimate_noise', clearance='monitor', box_excess='monitor', hit_step='monitor', u_cmd='drivers')
        assert all((k in got) == (arg in args) for k, arg in added.items()), tag
        if (B, T) == (2, 2):              # smaller than an earlier launch with the same records
            assert same(fetched('u_plant', (T, B, 2, old.n_u)), got['u_plant']), tag
            if 'estimate_noise' in args:
                assert same(fetched('q_est', (T, B, old.n_q)), got['q_est']), tag
            if 'drivers' in args:
                assert same(fetched('u_cmd', (T, B, old.n_u)), got['u_cmd']), tag
