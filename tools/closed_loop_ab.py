#!/usr/bin/env python3
"""A/B of step_batch between two checkouts, byte for byte: every result key of a fixed list of closed-loop launches.

    python tools/closed_loop_ab.py --parent /path/to/parent/checkout [--out profiles/closed_loop_one_pack_ab.txt]

Each side runs in fresh processes of its own (``--dump``): the checkout's package is imported and ``DGSQP_HIP_LIB`` names the checkout's own
library, the product build for one process and libdgsqp_hip_b256.so for another.  Every key of every result goes to an ``.npz``; the
parent process then compares the arrays' bytes (NaN payloads and the sign of zero count) and the key sets.  Both checkouts must be built.

The launches: kb_curve_N10, B = 7, T = 3 through the settings of test_one_handle_through_every_closed_loop_setting (no plant; a plant
with delays; vehicles and delays per chain; estimates + monitor 'stop'; PID + replay drivers; hold R = 2, on_fail 'hold'; everything at
once), on ONE solver object in that order; everything at once with B = 600, more chains than workgroups; the kinematic game on dynamic
plants with one TRACK agent (B = 3, T = 3).  The b256 process runs the plant with delays and everything at once.
``--models`` runs the one-lane consumers of the vehicle models instead, on the product build: one control step (B = 3) under a plant of each
integrator (euler, rk2, rk3, rk4 with 2 sub-steps; sim_steps = 2) on kb_curve_N10, dyn_curve_N15, merge_N8, the point-mass curve game
(N = 10) and the F1 game (N = 12, kinematic); ``pid_warm_start_batch(..., want_trajectories=True)`` (B = 8) on kb_chicane_N15, dyn_curve_N15,
the point-mass game and the F1 game, kinematic and dynamic; ``mpc_batch`` with the smallest cases of tests/test_ltv_mpc.py (kinematic N = 3,
dynamic N = 4, point mass N = 3, kinematic on the spline track N = 3; scenario, weights and bounds are that module's own).
A child that fails ends the run: nothing more is started on the device."""
import argparse
import os
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
DELAYS = [[2, 1], [0, 3]]


def launches(build):
    """(tag, game, B, T, settings) -- settings(B, T, solver, game) -> keyword arguments of step_batch."""
    from dgsqp_amd import closed_loop as cl
    from dgsqp_amd.dynamics import DynamicBicycleConfig
    import copy
    kw = dict(method='rk4', M=2, sim_steps=2)
    plain = cl.PlantModel(delay_steps=DELAYS, **kw)
    rng = np.random.default_rng(7)

    def per_chain(B, g):
        cfgs = [copy.deepcopy(m.model_config) for m in g.joint_model.dynamics_models]
        return cl.PlantModel(per_chain_configs=cl.perturbed_configs(cfgs, dict(mass=0.2), B, seed=B), per_chain_delay_steps=rng.integers(0, 4, size=(B, 2, 2)), **kw)

    def noise(B, T, s):
        return 1e-2 * rng.standard_normal((B, T, s.n_q))

    def replay(B, T, s):
        rep = np.zeros((B, T, s.n_u))
        rep[:, :, 2:4] = [0.3, 0.02]
        return cl.Drivers(kinds=['pid', 'replay'], u_replay=rep)

    hold = cl.PlanHold(replan_every=2, on_fail='hold')

    def everything(B, T, s, g):
        return dict(plant=per_chain(B, g), estimate_noise=noise(B, T, s), monitor='stop', drivers=replay(B, T, s), hold=hold, u_prev=True)

    def cross(B, T, s, g):
        dyn = [DynamicBicycleConfig(dt=0.1, model_name='dynamic_bicycle', noise=False, discretization_method='rk4', simple_slip=False,
                                    tire_model='pacejka', mass=2.2187, yaw_inertia=0.02723, wheel_friction=0.9, pacejka_b_front=5.0,
                                    pacejka_b_rear=5.0, pacejka_c_front=2.28, pacejka_c_rear=2.28, M=4) for _ in range(2)]
        return dict(plant=cl.PlantModel(dynamics_configs=dyn, own_class=True, method='rk4', M=3, sim_steps=2, delay_steps=DELAYS),
                    drivers=cl.Drivers(kinds=['game', 'track']))

    some = [('plant with delays', 7, 3, lambda B, T, s, g: dict(plant=plain)),
            ('everything at once', 7, 3, everything)]
    if build == '256':
        return some
    return [('no plant', 7, 3, lambda B, T, s, g: {}),
            some[0],
            ('vehicles and delays per chain', 7, 3, lambda B, T, s, g: dict(plant=per_chain(B, g))),
            ("estimates + monitor 'stop'", 7, 3, lambda B, T, s, g: dict(plant=plain, estimate_noise=noise(B, T, s), monitor='stop')),
            ('PID + replay drivers', 7, 3, lambda B, T, s, g: dict(plant=plain, drivers=replay(B, T, s))),
            ("hold R = 2, on_fail 'hold'", 7, 3, lambda B, T, s, g: dict(plant=plain, hold=hold)),
            some[1],
            ('everything at once, B = 600 > the grid', 600, 3, everything),
            ('cross: kinematic game on dynamic plants, one TRACK agent', 3, 3, cross)]


def dump(root, build, out):
    sys.path.insert(0, str(root))
    import dgsqp_amd
    from dgsqp_amd import _ffi
    from dgsqp_amd.montecarlo import kinematic_racing_game, sample_scenarios
    from dgsqp_amd.solver import DGSQP
    assert pathlib.Path(dgsqp_amd.__file__).resolve().parent.parent == pathlib.Path(root).resolve(), dgsqp_amd.__file__
    g = kinematic_racing_game('curve', N=10)
    s = DGSQP(*g.solver_args(), print_method=None)
    arrays = {}
    for i, (tag, B, T, settings) in enumerate(launches(build)):
        x0, u_ws = sample_scenarios(g, B, seed=120 + i)
        res = s.step_batch(x0, u_ws, T, keep_predictions=True, **settings(B, T, s, g))
        for key, val in res.items():
            if key in ('kernel_ms', 'total_ms', 'time'):      # clocks, not results
                continue
            arrays[f'{tag}|{key}'] = np.asarray(val)
        print(f'{tag}: steps_done {np.bincount(res["steps_done"], minlength=T + 1).tolist()}, keys {len(res)}', flush=True)
    np.savez(out, library=np.array(pathlib.Path(_ffi.library_path(1)).name), **arrays)


def dump_models(root, out):
    sys.path[:0] = [str(root), str(ROOT / 'tests')]
    import dgsqp_amd
    from dgsqp_amd import _ffi, closed_loop as cl, montecarlo as mc
    from dgsqp_amd.solver import DGSQP
    import test_ltv_mpc as tm                      # scenario, weights, wide_bounds: plain functions of this tree's test module
    assert pathlib.Path(dgsqp_amd.__file__).resolve().parent.parent == pathlib.Path(root).resolve(), dgsqp_amd.__file__
    games = dict(kb_curve_N10=lambda: mc.kinematic_racing_game('curve', N=10), kb_chicane_N15=lambda: mc.kinematic_racing_game('chicane', N=15),
                 dyn_curve_N15=lambda: mc.dynamic_racing_game(N=15, rk4_substeps=4, game_def='curve'), merge_N8=lambda: mc.merge_game(N=8),
                 pm_curve_N10=lambda: mc.point_mass_racing_game('curve', N=10), pm_curve_N5=lambda: mc.point_mass_racing_game(N=5),
                 f1_kin_N12=lambda: mc.f1_racing_game(N=12, model='kinematic', rk4_substeps=3),
                 f1_dyn_N12=lambda: mc.f1_racing_game(N=12, model='dynamic', rk4_substeps=3), f1_kin_N6=lambda: mc.f1_racing_game(N=6))
    plants = ('kb_curve_N10', 'dyn_curve_N15', 'merge_N8', 'pm_curve_N10', 'f1_kin_N12')
    pids = ('kb_chicane_N15', 'dyn_curve_N15', 'pm_curve_N10', 'f1_kin_N12', 'f1_dyn_N12')
    mpcs = dict(kb_curve_N10=('kin', 3, 4, 5, {}), dyn_curve_N15=('dyn', 4, 4, 5, {}), pm_curve_N5=('kin', 3, 3, 29, dict(u=(0.6, 0.2), du=(3.0, 1.0))),
                f1_kin_N6=('kin', 3, 3, 23, dict(u=(0.6, 0.2), du=(3.0, 1.0))))
    arrays = {}

    def keep(tag, res):
        for key, val in res.items():
            if key not in ('kernel_ms', 'total_ms', 'time', 'timing', 'dims'):      # clocks and the launch's sizes, not results
                arrays[f'{tag}|{key}'] = np.asarray(val)
        print(f'{tag}: keys {len(res)}', flush=True)

    for name, make in games.items():
        g = make()
        s = DGSQP(*g.solver_args(), print_method=None)
        if name in plants:
            x0, u_ws = mc.sample_scenarios(g, 3, seed=31)
            for method in ('euler', 'rk2', 'rk3', 'rk4'):
                keep(f'{name}, {method} plant', s.step_batch(x0, u_ws, 1, keep_predictions=True, plant=cl.PlantModel(method=method, M=2, sim_steps=2)))
        if name in pids:
            keep(f'{name}, pid_warm_start_batch', s.pid_warm_start_batch(mc.sample_scenarios(g, 8, seed=37)[0], want_trajectories=True))
        if name in mpcs:
            kind, N, B, seed, bkw = mpcs[name]
            q0, u_ws, du_ws, q_ref, idx = tm.scenario(kind, B, N, seed=seed)
            if name == 'f1_kin_N6':
                q0[:, idx[1]] += np.array([0.0, 7.3, 21.9])
                q_ref[:, :, idx[1]] += np.array([0.0, 7.3, 21.9])[:, None]
            mdl = s.joint_dynamics.dynamics_models[0]
            keep(f'{name}, mpc_batch {kind} N = {N}', s.mpc_batch(0, tm.weights(kind, idx), tm.wide_bounds(mdl, idx, **bkw), q0, u_ws, du_ws, q_ref, None, log=True, N=N))
    np.savez(out, library=np.array(pathlib.Path(_ffi.library_path(1)).name), **arrays)


def compare(a, b):
    """Lines of the report, and whether everything is equal."""
    A, B = np.load(a), np.load(b)
    lines, ok = [f'  libraries: {A["library"]} | {B["library"]}'], set(A.files) == set(B.files)
    if not ok:
        lines.append(f'  KEY SETS DIFFER: only parent {sorted(set(A.files) - set(B.files))}, only tree {sorted(set(B.files) - set(A.files))}')
    tags = []
    for name in A.files:
        if '|' in name and name.split('|')[0] not in tags:
            tags.append(name.split('|')[0])
    for tag in tags:
        keys = [n.split('|')[1] for n in A.files if n.startswith(tag + '|') and n in B.files]
        bad = [k for k in keys if A[f'{tag}|{k}'].dtype != B[f'{tag}|{k}'].dtype or A[f'{tag}|{k}'].shape != B[f'{tag}|{k}'].shape
               or A[f'{tag}|{k}'].tobytes() != B[f'{tag}|{k}'].tobytes()]
        ok = ok and not bad
        lines.append(f'  {tag}: {len(keys)} keys ({", ".join(keys)}): ' + ('all bytes equal' if not bad else f'DIFFERENT: {bad}'))
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help='the other checkout (built)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'closed_loop_one_pack_ab.txt'))
    ap.add_argument('--dump', help='(child) write the results of --root / --build here')
    ap.add_argument('--root', default=str(ROOT))
    ap.add_argument('--build', choices=('512', '256'), default='512')
    ap.add_argument('--models', action='store_true', help='the one-lane consumers of the vehicle models (plants of every integrator, PID warm starts, the tracker) instead')
    args = ap.parse_args()
    if args.dump:
        return dump_models(args.root, args.dump) if args.models else dump(args.root, args.build, args.dump)
    if not args.parent:
        ap.error('--parent is needed')
    what = 'plants of every integrator, PID warm starts and the tracker' if args.models else 'step_batch'
    text, all_ok = [f'{what}, parent checkout against this tree, every result key byte for byte (tools/closed_loop_ab.py{" --models" * args.models})'], True
    with tempfile.TemporaryDirectory() as td:
        for build in ('512',) if args.models else ('512', '256'):
            files = []
            for side, root in (('parent', pathlib.Path(args.parent).resolve()), ('tree', ROOT)):
                lib = root / 'dgsqp_amd' / 'csrc' / ('libdgsqp_hip.so' if build == '512' else 'libdgsqp_hip_b256.so')
                files.append(f'{td}/{side}_{build}.npz')
                env = dict(os.environ, DGSQP_HIP_LIB=str(lib))
                subprocess.run([sys.executable, __file__, '--dump', files[-1], '--root', str(root), '--build', build] + ['--models'] * args.models,
                               env=env, check=True, timeout=240, cwd=str(root))
            lines, ok = compare(*files)
            text += [f'build {build}:'] + lines
            all_ok = all_ok and ok
    text.append('RESULT: ' + ('every key of every launch is equal, byte for byte' if all_ok else 'DIFFERENCES (see above)'))
    print('\n'.join(text))
    pathlib.Path(args.out).write_text('\n'.join(text) + '\n')
    return 0 if all_ok else 1


if __name__ == '__main__':
    sys.exit(main())
