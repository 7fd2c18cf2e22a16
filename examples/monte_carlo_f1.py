#!/usr/bin/env python3
"""The F1 study (scripts/comparison_study_f1) on the MI355X library: the head-to-head race on ``f1_austin_tenth_scale`` with its front end on
the device.  ``--front-end raceline``: cars drawn around the TUM raceline (monte_carlo_sampler.py: car 2 ahead of car 1) and warm-started
by the LTV-MPC tracker following it (warm_start.py); ``--front-end circuit``: the placement of DGSQP_comp_monte_carlo.py with PID warm
starts, BASELINE configs[3]'s.  Sampling, warm starts and the solve stay on the device (``stage=True`` -> ``dgsqp_solve_staged``).  One
``sample_<i>.pkl`` = ``dict(solver_result=<solve() info>, initial_condition=<joint VehicleStates>)`` per sample, as the study's scripts write.

    python examples/monte_carlo_f1.py --num-mc 1024 --out /tmp/f1
    python examples/monte_carlo_f1.py --front-end raceline --model dynamic --N 25 --s-range 60 80
"""
import argparse
import ctypes
import pathlib
import time

import numpy as np

from _driver import ROOT, dump
from dgsqp_amd import _ffi
from dgsqp_amd.montecarlo import f1_racing_game, sample_scenarios
from dgsqp_amd.results import solve_infos
from dgsqp_amd.solver import DGSQP

FIXTURE = ROOT / 'tests' / 'golden' / 'f1_traj_race_cl.csv.gz'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-mc', type=int, default=100, help='samples')
    ap.add_argument('--N', type=int, default=None, help='horizon (default: 50 for the kinematic game, 25 for the dynamic one)')
    ap.add_argument('--model', choices=('kinematic', 'dynamic'), default=None, help="default: 'kinematic' (circuit), 'dynamic' (raceline)")
    ap.add_argument('--front-end', choices=('circuit', 'raceline'), default='circuit',
                    help="'circuit': DGSQP_comp_monte_carlo.py's sampler with PID warm starts; 'raceline': the F1 study's sampler and tracker warm starts")
    ap.add_argument('--raceline', default=str(FIXTURE), help="the study's traj_race_cl.csv (TUM format, full scale)")
    ap.add_argument('--s-range', type=float, nargs=2, default=None, metavar=('S_LO', 'S_HI'),
                    help="raceline front end: car 1's arclength window (the study's track segment: 60 80); default [0, L - 10]")
    ap.add_argument('--edges', choices=('constant', 'track'), default='constant',
                    help="'track': the game's e_y box becomes the track's edge rows; the raceline front end clips with 0.9 x the width functions and its tracker gets the edge rows")
    ap.add_argument('--time-scale', type=float, default=1.0, help='raceline front end: the line is driven time_scale times slower')
    ap.add_argument('--seed', type=int, default=0, help='seed of the counter-based sampler (the script seeds its generator with 0)')
    ap.add_argument('--rk4-substeps', type=int, default=10)
    ap.add_argument('--host-sampler', action='store_true',
                    help="sequential np.random.default_rng(seed) draws on the host (montecarlo.sample_scenarios) instead of the counter-based device sampler")
    ap.add_argument('--out', default=None, help='directory of the sample_<i>.pkl files')
    args = ap.parse_args(argv)
    raceline = args.front_end == 'raceline'
    model = args.model or ('dynamic' if raceline else 'kinematic')
    N = args.N or (25 if model == 'dynamic' else 50)
    game = f1_racing_game(N=N, model=model, rk4_substeps=args.rk4_substeps, sampler=args.front_end, raceline=args.raceline if raceline else None,
                          time_scale=args.time_scale, s_range=args.s_range if raceline else None,
                          edges=args.edges)
    solver = DGSQP(*game.solver_args(), print_method=None)
    B = args.num_mc
    t0 = time.time()
    if args.host_sampler:
        x0, u_ws = sample_scenarios(game, B, seed=args.seed, solver=solver if raceline else None)      # (the tracker's warm starts still run on the device)
        x0, u_am = np.ascontiguousarray(x0), np.ascontiguousarray(solver._to_agent_major(u_ws))
        if solver._lib.dgsqp_stage_inputs(solver._h, B, _ffi.dptr(x0), _ffi.dptr(u_am)) != 0:
            raise RuntimeError(solver._lib.dgsqp_last_error(solver._h).decode())
        smp = dict(x0=x0, u_ws=u_ws, candidates=float('nan'))
    else:
        smp = (solver.sample_raceline_batch if raceline else solver.sample_batch)(game, B, seed=args.seed, stage=True)
    t1 = time.time()
    tm = _ffi.TimingT()
    if solver._lib.dgsqp_solve_staged(solver._h, ctypes.byref(tm)) != 0:
        raise RuntimeError(solver._lib.dgsqp_last_error(solver._h).decode())
    res = solver._records((B,))
    if solver._lib.dgsqp_fetch_results(solver._h, _ffi.dptr(res['u']), _ffi.dptr(res['l']), _ffi.dptr(res['x']), _ffi.iptr(res['status']),
                                       _ffi.iptr(res['num_iters']), _ffi.iptr(res['qp_solves']), _ffi.dptr(res['cond']), _ffi.dptr(res['cost'])) != 0:
        raise RuntimeError(solver._lib.dgsqp_last_error(solver._h).decode())
    wall = time.time() - t1
    res['msg'] = [_ffi.STATUS_NAMES[int(s)] for s in res['status']]
    infos = solve_infos(res, wall)
    samples = [dict(solver_result=si, initial_condition=game.joint_model.qu2state(None, smp['x0'][b], np.zeros(game.joint_model.n_u)))
               for b, si in enumerate(infos)]
    conv = res['status'] <= 1
    print(f'{game.name} [{args.front_end} front end]: {B} samples; front end {t1 - t0:.2f} s ({smp["candidates"]} candidates, '
          f'{smp["candidates"] / B:.2f} per accepted), solve {wall:.2f} s ({B / max(wall, 1e-9):.0f} scenarios/s); converged {conv.mean():.3f}, '
          f'mean iterations (converged) {res["num_iters"][conv].mean() if conv.any() else float("nan"):.1f}, qp_fail {np.mean(res["status"] == 4):.3f}')
    if args.out:
        for i, s in enumerate(samples):
            dump(pathlib.Path(args.out) / f'sample_{i + 1}.pkl', s)
    return samples


if __name__ == '__main__':
    main()
