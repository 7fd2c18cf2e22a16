#!/usr/bin/env python3
"""B closed-loop runs of T steps: the host loop a user had to write before step_batch against step_batch itself.

(a) host loop: T rounds of ``solve_batch`` (default cooperative mode), numpy ``closed_loop.feedback``, re-upload -- T launches, each
    ending with its slowest scenario, and 2 T copies;
(b) ``step_batch``: one launch that ends with its longest chain, no intermediate copies (and no line-search helpers, no deferral);
(c) with ``--plant``: ``step_batch`` with a plant of its own (``closed_loop.PlantModel``: the game's vehicle, rk4 with 10 sub-steps, 2
    simulation steps per control step, car 1's steering delayed by one simulation step), timed next to (a) and (b).  Its chains differ
    from (b)'s -- another state is fed back --, so its time is reported, not compared.

Game and size: BASELINE configs[1] (dyn_curve_N25), B = 1,024, T = 10, no disturbance, inputs from the device sampler.  The two are
alternated ``--repeats`` times in one process after one warm-up each; times are host clocks around synchronous calls.  The script also
asserts that both produce identical status, num_iters and q.

    python tools/closed_loop_bench.py [--out profiles/closed_loop_dyn_curve_N25.txt]
    python tools/closed_loop_bench.py --plant --out profiles/closed_loop_plant_dyn_curve_N25.txt

``--ensemble`` times the launch kinds of a robustness study instead, each ``--repeats`` times, alternated, after one warm-up each:
``plain`` (no plant), ``plant`` ((c)'s plant), ``ensemble`` (that plant with a vehicle per chain: mass, drag and tyre D +-10 %, and a
delay per chain), ``estimates`` (that plant, solves from q + 1e-3 N(0, 1)), and the last two with the monitor recording
(``ensemble+monitor``, ``estimates+monitor``); and two launches with drivers (``closed_loop.Drivers``) on that plant: ``pid`` (car 2 on the
PID lane follower with its default gains, references from x0) and ``replay`` (car 2 replays the commands the game gave it in the ``plant``
launch: the same chains as ``plant``, bit for bit, with car 2's command read from u_replay).  ``--carry-u-prev`` adds ``carry-u-prev``: ``plain`` with the command of step t carried into solve t + 1 as the input
before its stage 0 (``step_batch(..., u_prev=True)``) -- other solves, so other chains: its time stands next to the others, not against them.
``--kinds ...,hold`` adds ``hold`` (named in ``--kinds`` only): the ``plant`` launch with a held plan (``closed_loop.PlanHold``, on_fail 'reference'), once per value of
``--replan-every`` (default 1).  R = 1 is the ``plant`` launch's own chains with the hold named (asserted), so its time stands against ``plant``'s; R > 1 follows each
accepted plan for R control steps -- other chains -- and the report counts the solves actually run and the held steps.
``--kinds ...,cross`` with ``--model kinematic`` adds ``cross`` (named in ``--kinds`` only): the kinematic curve game (N = 25) on DYNAMIC-bicycle plants of their own state
(``PlantModel(own_class=True)``: the Pacejka vehicle of configs[1], the ``plant`` launch's integrator, simulation steps and delay; GAME drivers) -- other chains than ``plant``'s,
so its time stands next to it.
``--kinds`` restricts the list (a library without the newer entry points can still time
``plain,plant``), ``--label`` names the build in the output, ``--append`` adds to ``--out`` instead of replacing it.

    python tools/closed_loop_bench.py --ensemble --repeats 5 --out profiles/closed_loop_ensemble_dyn_curve_N25.txt
"""
import argparse
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def host_loop(s, x0, u_am, T):
    """What a user writes without step_batch.  Chains whose next state is not finite drop out, as in the kernel."""
    from dgsqp_amd import closed_loop
    B = len(x0)
    q = np.full((B, T + 1, s.n_q), np.nan)
    status = np.full((B, T), -1, np.int32)
    iters = np.zeros((B, T), np.int32)
    q[:, 0] = x0
    ws = u_am.copy()
    live = np.arange(B)
    kernel_ms = 0.0
    for t in range(T):
        if not len(live):
            break
        r = s.solve_batch(q[live, t], ws[live])
        kernel_ms += r['kernel_ms']
        status[live, t], iters[live, t] = r['status'], r['num_iters']
        q_next, ws_next, ok = closed_loop.feedback(r['x'], r['u'], r['status'], ws[live], num_ua_d=s.num_ua_d)
        q[live, t + 1] = q_next
        ws[live[ok]] = ws_next[ok]
        live = live[ok]
    return dict(q=q, status=status, num_iters=iters, kernel_ms=kernel_ms)


KINDS = ('plain', 'plant', 'ensemble', 'ensemble+monitor', 'estimates', 'estimates+monitor', 'pid', 'replay')
CARRY = 'carry-u-prev'          # added by --carry-u-prev (or named in --kinds): 'plain' with step_batch(..., u_prev=True)
HOLD = 'hold'                   # named in --kinds: 'plant' with step_batch(..., hold=PlanHold(replan_every=R)) for every R of --replan-every
CROSS = 'cross'                 # named in --kinds with --model kinematic: the kinematic game on dynamic plants, step_batch(..., plant=PlantModel(own_class=True))


def ensemble_bench(args, g, s, x0, u_am):
    """The launch kinds of ``--ensemble``; returns the report's lines."""
    import copy
    from dgsqp_amd import closed_loop
    B, T = args.batch, args.steps
    kinds = [k for k in args.kinds.split(',') if k]
    if args.carry_u_prev and CARRY not in kinds:
        kinds.append(CARRY)
    unknown = [k for k in kinds if k not in KINDS + (CARRY, HOLD, CROSS)]
    if unknown:
        raise SystemExit(f'unknown kinds {unknown}; choose from {KINDS + (CARRY, HOLD, CROSS)}')
    if CROSS in kinds and args.model != 'kinematic':
        raise SystemExit(f'the kind {CROSS} puts dynamic plants under a kinematic game: --model kinematic')
    base = dict(method='rk4', M=10, sim_steps=2)
    calls = {'plain': lambda: s.step_batch(x0, u_am, T)}
    if CARRY in kinds:
        calls[CARRY] = lambda: s.step_batch(x0, u_am, T, u_prev=True)
    plant = closed_loop.PlantModel(delay_steps=[[0, 1], [0, 0]], **base)
    calls['plant'] = lambda: s.step_batch(x0, u_am, T, plant=plant)
    if 'pid' in kinds:
        pid = closed_loop.Drivers(kinds=['game', 'pid'])
        calls['pid'] = lambda: s.step_batch(x0, u_am, T, plant=plant, drivers=pid)
    if 'replay' in kinds:
        own = calls['plant']()
        replay = closed_loop.Drivers(kinds=['game', 'replay'], u_replay=own['u_applied'])
        calls['replay'] = lambda: s.step_batch(x0, u_am, T, plant=plant, drivers=replay)
        again = calls['replay']()
        for key in ('status', 'num_iters', 'q', 'u_plant'):
            assert np.array_equal(again[key], own[key], equal_nan=True), f'{key}: the replay of the plant launch\'s own commands differs from it'
    if CROSS in kinds:
        from dgsqp_amd.montecarlo import dynamic_racing_game
        dyn = [copy.deepcopy(m.model_config) for m in dynamic_racing_game(N=5).joint_model.dynamics_models]
        cross = closed_loop.PlantModel(dynamics_configs=dyn, own_class=True, delay_steps=[[0, 1], [0, 0]], **base)
        calls[CROSS] = lambda: s.step_batch(x0, u_am, T, plant=cross)
    if HOLD in kinds:
        at = kinds.index(HOLD)
        kinds[at:at + 1] = [f'{HOLD} R={R}' for R in args.replan_every]
        for R in args.replan_every:
            calls[f'{HOLD} R={R}'] = lambda R=R: s.step_batch(x0, u_am, T, plant=plant, hold=closed_loop.PlanHold(replan_every=R))
        if 1 in args.replan_every:
            own, held = calls['plant'](), calls[f'{HOLD} R=1']()
            for key in ('status', 'num_iters', 'q', 'u_plant'):
                assert np.array_equal(held[key], own[key], equal_nan=True), f'{key}: the held-plan launch with R = 1 differs from the plant launch'
    if any(k not in ('plain', 'plant', 'pid', 'replay', CARRY, CROSS) and not k.startswith(HOLD) for k in kinds):
        cfgs = [copy.deepcopy(m.model_config) for m in g.joint_model.dynamics_models]
        spread = dict(mass=0.1, drag_coefficient=0.1, pacejka_d_front=0.1, pacejka_d_rear=0.1)
        delays = np.random.default_rng(args.seed).integers(0, 3, size=(B, len(cfgs), 2))
        ens = closed_loop.PlantModel(per_chain_configs=closed_loop.perturbed_configs(cfgs, spread, B, args.seed), per_chain_delay_steps=delays, **base)
        v = 1e-3 * np.random.default_rng(args.seed + 1).standard_normal((B, T, s.n_q))
        calls['ensemble'] = lambda: s.step_batch(x0, u_am, T, plant=ens)
        calls['ensemble+monitor'] = lambda: s.step_batch(x0, u_am, T, plant=ens, monitor=True)
        calls['estimates'] = lambda: s.step_batch(x0, u_am, T, plant=plant, estimate_noise=v)
        calls['estimates+monitor'] = lambda: s.step_batch(x0, u_am, T, plant=plant, estimate_noise=v, monitor=True)
    wall, kern, last = {k: [] for k in kinds}, {k: [] for k in kinds}, {}
    for k in kinds:
        calls[k]()                                                 # warm-up of each (code objects, buffers)
    for _ in range(args.repeats):
        for k in kinds:
            t0 = time.perf_counter()
            r = calls[k]()
            wall[k].append(time.perf_counter() - t0)
            kern[k].append(r['kernel_ms'] / 1e3)
            last[k] = r
    ms = lambda v: f'median {np.median(v) * 1e3:8.1f} ms (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}; spread {(max(v) - min(v)) / np.median(v) * 100:.1f} %)'
    lines = [f'[{args.label}] closed loop, {args.game_name}, B = {B} chains x T = {T} steps, device-sampled inputs (seed {args.seed}); '
             f'{args.repeats} alternated repeats of every kind after one warm-up each; plant: rk4, 10 sub-steps, 2 simulation steps per control step']
    for k in kinds:
        r = last[k]
        note = f'steps run {int((r["status"] >= 0).sum())} of {B * T}, iterations per chain: mean {r["num_iters"].sum(axis=1).mean():.1f}'
        if 'plan_stage' in r:
            note = f'solves run {int((r["status"] >= 0).sum())} and held steps {int((r["status"] == -2).sum())} of {B * T}' + note[note.index(','):]
        if 'hit_step' in r:
            note += f'; chains with a contact {int((r["hit_step"] >= 0).sum())}, mean box_excess {np.nanmean(r["box_excess"]):.4f}'
        lines.append(f'[{args.label}] {k:18s} kernel {ms(kern[k])}; wall {ms(wall[k])}; kernel times {", ".join(f"{v * 1e3:.1f}" for v in kern[k])} ms; {note}')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--plant', action='store_true', help='also time step_batch with a plant of its own (c)')
    ap.add_argument('--ensemble', action='store_true', help='time the launch kinds of a robustness study instead (see the module docstring)')
    ap.add_argument('--kinds', default=','.join(KINDS), help='with --ensemble: comma-separated subset of ' + ', '.join(KINDS + (CARRY, HOLD)))
    ap.add_argument('--carry-u-prev', action='store_true', help='with --ensemble: also time the plain launch with the command carried into the next solve (kind ' + CARRY + ')')
    ap.add_argument('--replan-every', type=int, nargs='+', default=[1], help='with --ensemble and the kind ' + HOLD + ': one launch kind per value R')
    ap.add_argument('--label', default='this build', help='with --ensemble: names the build in the report')
    ap.add_argument('--append', action='store_true', help='with --ensemble: add to --out instead of replacing it')
    ap.add_argument('--model', choices=('dynamic', 'point-mass', 'kinematic'), default='dynamic',
                    help="the game: BASELINE configs[1] (dynamic bicycles, N = 25), the race demo's point-mass game on its circuit (N = 20), or the kinematic "
                         "curve game (N = 25; for the kind " + CROSS + ')')
    ap.add_argument('--out', default=None, help='default: profiles/closed_loop_<game>.txt')
    args = ap.parse_args()
    from dgsqp_amd.montecarlo import dynamic_racing_game, kinematic_racing_game, point_mass_racing_game
    from dgsqp_amd.solver import DGSQP
    if args.model == 'point-mass':
        g, game_name = point_mass_racing_game('barc', N=20), 'pm_barc_N20 (scripts/race/game_setup_unicycle.py)'
    elif args.model == 'kinematic':
        g, game_name = kinematic_racing_game('curve', N=25), 'kb_curve_N25 (kinematic curve game)'
    else:
        g, game_name = dynamic_racing_game(N=25, rk4_substeps=10), 'dyn_curve_N25 (BASELINE configs[1])'
    args.game_name = game_name
    if args.out is None:
        args.out = str(ROOT / 'profiles' / f'closed_loop_{game_name.split()[0]}.txt')
    s = DGSQP(*g.solver_args(), print_method=None, qp_method='active_set')
    B, T = args.batch, args.steps
    smp = s.sample_batch(g, B, seed=args.seed)
    x0, u_am = smp['x0'], s._to_agent_major(smp['u_ws'])
    if args.ensemble:
        text = '\n'.join(ensemble_bench(args, g, s, x0, u_am))
        print(text)
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, 'a' if args.append else 'w') as f:
            f.write(text + '\n')
        return

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    run_a = lambda: host_loop(s, x0, u_am, T)
    run_b = lambda: s.step_batch(x0, u_am, T)
    if args.plant:
        from dgsqp_amd.closed_loop import PlantModel
        plant = PlantModel(method='rk4', M=10, sim_steps=2, delay_steps=[[0, 1], [0, 0]])
        run_c = lambda: s.step_batch(x0, u_am, T, plant=plant)
    _, a = timed(run_a)                                          # warm-up of each (code objects, buffers)
    _, b = timed(run_b)
    if args.plant:
        timed(run_c)
    for key in ('status', 'num_iters', 'q'):
        assert np.array_equal(a[key], b[key], equal_nan=(key == 'q')), f'{key}: host loop and step_batch differ'
    ta, tb, tc, ka, kb, kc = [], [], [], [], [], []
    for _ in range(args.repeats):
        dt, a = timed(run_a); ta.append(dt); ka.append(a['kernel_ms'] / 1e3)
        dt, b = timed(run_b); tb.append(dt); kb.append(b['kernel_ms'] / 1e3)
        if args.plant:
            dt, c = timed(run_c); tc.append(dt); kc.append(c['kernel_ms'] / 1e3)
    st = b['status']
    fmt = lambda v: f'median {np.median(v) * 1e3:.1f} ms (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})'
    lines = [f'closed loop, {game_name}, B = {B} chains x T = {T} steps, no disturbance, device-sampled inputs (seed {args.seed}); {args.repeats} alternated repeats after one warm-up each',
             f'(a) host loop: {T} x solve_batch (cooperative line search + deferral) + numpy feedback + re-upload: wall {fmt(ta)}; kernels alone {fmt(ka)}',
             f'(b) step_batch: one launch of dg_closed_loop_kernel:                                               wall {fmt(tb)}; kernel alone {fmt(kb)}',
             f'(b) / (a), medians of the wall times: {np.median(tb) / np.median(ta):.3f}   ((a) / (b) = {np.median(ta) / np.median(tb):.3f})',
             f'identical status, num_iters and q in (a) and (b): yes (asserted); steps run {int((st >= 0).sum())} of {B * T}, converged {np.mean((st >= 0) & (st <= 1)):.3f}, '
             f'iterations per step: mean {b["num_iters"].mean():.2f}, max {int(b["num_iters"].max())}; per chain: mean {b["num_iters"].sum(axis=1).mean():.1f}, max {int(b["num_iters"].sum(axis=1).max())}']
    if args.plant:
        sc = c['status']
        lines.append(f'(c) step_batch with a plant (rk4, 10 sub-steps, 2 simulation steps per control step, one delayed channel):  wall {fmt(tc)}; kernel alone {fmt(kc)}; '
                     f'steps run {int((sc >= 0).sum())} of {B * T}, converged {np.mean((sc >= 0) & (sc <= 1)):.3f}, iterations per chain: mean {c["num_iters"].sum(axis=1).mean():.1f}, '
                     f'max {int(c["num_iters"].sum(axis=1).max())}; every wall time of (b): {", ".join(f"{v * 1e3:.1f}" for v in tb)} ms')
    text = '\n'.join(lines)
    print(text)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(text + '\n')


if __name__ == '__main__':
    main()
