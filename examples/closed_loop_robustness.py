#!/usr/bin/env python3
"""A robustness study in one launch per parameter spread: B closed-loop runs on the curve game, every chain against a vehicle of its own
(mass, drag and slip coefficient drawn within +-spread of the nominal by ``closed_loop.perturbed_configs``), planned from a noisy state
estimate, watched by the safety monitor between control steps.  Prints, against the spread, the share of chains with a contact and the
mean box excess (how far the worst state entry is from its bound, negative: inside).

``--opponent pid`` runs the same ensemble a second time with car 2 on the PID lane follower (``closed_loop.Drivers``) instead of its part of
the game's solution -- an opponent that does not play the equilibrium the ego assumes -- and prints clearance and hit statistics next to the
self-play ones.

    python examples/closed_loop_robustness.py --batch 1024 --steps 20 --spreads 0 0.05 0.1 0.2
    python examples/closed_loop_robustness.py --opponent pid
"""
import argparse
import copy
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from dgsqp_amd.closed_loop import Drivers, PlantModel, perturbed_configs          # noqa: E402
from dgsqp_amd.montecarlo import kinematic_racing_game                            # noqa: E402
from dgsqp_amd.solver import DGSQP                                                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024, help='chains per launch')
    ap.add_argument('--steps', type=int, default=20, help='control steps per chain')
    ap.add_argument('--N', type=int, default=15, help='horizon')
    ap.add_argument('--spreads', type=float, nargs='+', default=[0.0, 0.05, 0.1, 0.2], help='relative half-widths of the vehicle parameters')
    ap.add_argument('--noise', type=float, default=1e-2, help='standard deviation of the state-estimate noise')
    ap.add_argument('--sim-steps', type=int, default=4, help='simulation steps of the plant per control step')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--opponent', choices=('game', 'pid'), default='game', help="who drives car 2: its part of the game's solution, or the PID lane follower")
    args = ap.parse_args()

    game = kinematic_racing_game('curve', N=args.N)
    s = DGSQP(*game.solver_args(), print_method=None)
    B, T = args.batch, args.steps
    smp = s.sample_batch(game, B, seed=args.seed)
    nominal = [copy.deepcopy(m.model_config) for m in game.joint_model.dynamics_models]
    noise = args.noise * np.random.default_rng(args.seed).standard_normal((B, T, s.n_q))
    print(f'{B} chains x {T} steps, estimate noise {args.noise:g}, plant: rk4, {args.sim_steps} simulation steps per control step')
    opponents = [('self-play', None)] + ([('pid', Drivers(kinds=['game', 'pid']))] if args.opponent == 'pid' else [])
    print('spread   car 2       chains with a contact   min clearance   mean clearance   mean box_excess   mean steps run   kernel [ms]')
    for spread in args.spreads:
        ens = perturbed_configs(nominal, dict(mass=spread, drag_coefficient=spread, slip_coefficient=spread), B, args.seed)
        plant = PlantModel(per_chain_configs=ens, method='rk4', M=2, sim_steps=args.sim_steps)
        for name, drivers in opponents:
            r = s.step_batch(smp['x0'], smp['u_ws'], T, plant=plant, estimate_noise=noise, monitor='stop', drivers=drivers)
            print(f'{spread:6.3f}   {name:9s}   {np.mean(r["hit_step"] >= 0):21.4f}   {np.nanmin(r["clearance"]):13.4f}   {np.nanmean(r["clearance"]):14.4f}   '
                  f'{np.nanmean(r["box_excess"]):15.4f}   {r["steps_done"].mean():14.2f}   {r["kernel_ms"]:11.1f}')


if __name__ == '__main__':
    main()
