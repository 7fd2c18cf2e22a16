#!/usr/bin/env python3
"""A robustness study in one launch per parameter spread: B closed-loop runs on the curve game, every chain against a vehicle of its own
(mass, drag and slip coefficient drawn within +-spread of the nominal by ``closed_loop.perturbed_configs``), planned from a noisy state
estimate, watched by the safety monitor between control steps.  Prints, against the spread, the share of chains with a contact and the
mean box excess (how far the worst state entry is from its bound, negative: inside).

``--opponent pid`` runs the same ensemble a second time with car 2 on the PID lane follower (``closed_loop.Drivers``) instead of its part of
the game's solution -- an opponent that does not play the equilibrium the ego assumes -- and prints clearance and hit statistics next to the
self-play ones.

The last columns are the actuator's view: per input channel (u_a, u_steer) the largest jump of the command that entered a plant between two
control steps, |cmd[t] - cmd[t-1]| / (dt rate_ub) with cmd[-1] = 0, over every agent and chain, and the share of control steps with a jump
beyond the game's own rate limit.  Without ``--carry-u-prev`` every solve measures its stage-0 rate rows against zero, so the limit holds
inside a prediction and not between two of them; with it the command of step t is the next solve's input before stage 0
(``step_batch(..., u_prev=True)``) and the limit holds along the chain wherever the solve converged.

``--replan-every R`` plans at every R-th control step only and follows the last accepted plan in between, ``--on-fail hold`` applies the next
stage of that plan after a failed solve ('diverged', 'qp_fail') instead of stage 0 of the failed iterate (``closed_loop.PlanHold``,
``step_batch(..., hold=...)``).  Two more columns then report the share of the steps that ran which were held (no solve) and which fell back
on the held plan or, with ``--on-fail reference``, applied a failed iterate.

    python examples/closed_loop_robustness.py --batch 1024 --steps 20 --spreads 0 0.05 0.1 0.2
    python examples/closed_loop_robustness.py --opponent pid
    python examples/closed_loop_robustness.py --carry-u-prev
    python examples/closed_loop_robustness.py --replan-every 3 --on-fail hold
    python examples/closed_loop_robustness.py --model point-mass
    python examples/closed_loop_robustness.py --model point-mass --plant-class dynamic --track

``--plant-class dynamic`` runs the chains on dynamic bicycles with Pacejka tyres -- a plant of ANOTHER model class than the game's, with a
state of its own (``PlantModel(own_class=True)``; mass, drag and yaw inertia perturbed).  The kinematic game's commands mean the same on
that plant; the point-mass game's (Fx, wz) do not, so there ``--track`` is needed: every car follows its part of the game's plan with the
lane follower (``Drivers('track')``) -- the race demo's set-up, with the PID law in place of its tracking MPC.
"""
import argparse
import copy
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from dgsqp_amd.closed_loop import Drivers, PlanHold, PlantModel, perturbed_configs          # noqa: E402
from dgsqp_amd.montecarlo import dynamic_racing_game, kinematic_racing_game, point_mass_racing_game    # noqa: E402
from dgsqp_amd.solver import DGSQP                                                # noqa: E402


def command_jumps(r, lim):
    """(largest jump per channel [2], share of steps that ran with a jump over the limit) of the commands the plants received: u_cmd with
    drivers, else stage 0 of the solution; in units of ``lim`` [n_u] = dt rate_ub.  NaN for a game without rate rows (``lim`` None): there is
    no limit to measure against."""
    if lim is None:
        return np.full(2, np.nan), np.nan
    cmd = r['u_cmd'] if 'u_cmd' in r else r['u_applied']
    prev = np.concatenate([np.zeros_like(cmd[:, :1]), cmd[:, :-1]], axis=1)
    jump = np.abs(cmd - prev) / lim                                 # NaN where a step never ran
    ran = np.isfinite(jump).all(axis=-1)
    worst = np.nanmax(jump.reshape(-1, lim.size // 2, 2), axis=(0, 1)) if ran.any() else np.full(2, np.nan)
    return worst, float((jump[ran].max(axis=-1) > 1.0 + 1e-9).mean()) if ran.any() else np.nan


def held_and_fallback(r, hold) -> str:
    """The two columns of a launch with a held plan: of the steps that ran, the share that was held (no solve) and the share whose solve
    failed -- the chain then applied the next stage of its plan ('hold') or stage 0 of the failed iterate ('reference')."""
    if hold is None:
        return ''
    st = r['status']
    ran = st != -1
    failed = (st >= 0) & (((hold.mask >> np.clip(st, 0, 5)) & 1) == 1)
    return f'   {(st == -2).sum() / max(1, ran.sum()):10.4f}   {failed.sum() / max(1, ran.sum()):14.4f}'


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
    ap.add_argument('--carry-u-prev', action='store_true', help="carry each step's command into the next solve as the input before its stage 0")
    ap.add_argument('--replan-every', type=int, default=1, help='solve at every R-th control step and follow the accepted plan in between')
    ap.add_argument('--on-fail', choices=('reference', 'hold'), default='reference',
                    help="after a failed solve: stage 0 of the failed iterate (the reference's step()), or the next stage of the plan the chain holds")
    ap.add_argument('--model', choices=('kinematic', 'point-mass'), default='kinematic',
                    help="the vehicles: kinematic bicycles, or the race demo's Frenet point masses (mass and damping perturbed; that game has no rate rows)")
    ap.add_argument('--plant-class', choices=('game', 'dynamic'), default='game',
                    help="the plants: the game's model class, or dynamic bicycles with Pacejka tyres (a state of their own)")
    ap.add_argument('--track', action='store_true', help="every car follows its part of the game's plan with the lane follower (needs --plant-class dynamic)")
    args = ap.parse_args()
    if args.track and args.plant_class != 'dynamic':
        ap.error('--track needs --plant-class dynamic')
    if args.plant_class == 'dynamic' and args.model == 'point-mass' and not args.track:
        ap.error("the point-mass game's inputs (Fx, wz) cannot command a bicycle: add --track")
    if args.track and args.opponent == 'pid':
        ap.error('--track drives every car; leave --opponent at game')

    game = point_mass_racing_game('curve', N=args.N) if args.model == 'point-mass' else kinematic_racing_game('curve', N=args.N)
    s = DGSQP(*game.solver_args(), print_method=None)
    B, T = args.batch, args.steps
    smp = s.sample_batch(game, B, seed=args.seed)
    cross = args.plant_class == 'dynamic'
    nominal = [copy.deepcopy(m.model_config) for m in (dynamic_racing_game(N=5) if cross else game).joint_model.dynamics_models]
    noise = args.noise * np.random.default_rng(args.seed).standard_normal((B, T, s.n_q))
    P = s._problem
    has_rate = all(P.agents[a].has_rate for a in range(s.M))          # (a game without rate rows stores rate_ub = 0)
    lim = np.array([P.dt * P.agents[a].rate_ub[j] for a in range(s.M) for j in range(2)]) if has_rate else None
    print(f'{B} chains x {T} steps, estimate noise {args.noise:g}, plant: rk4, {args.sim_steps} simulation steps per control step, '
          f'u_prev {"carried" if args.carry_u_prev else "zero in every solve"}')
    hold = PlanHold(replan_every=args.replan_every, on_fail=args.on_fail) if (args.replan_every, args.on_fail) != (1, 'reference') else None
    if hold is not None:
        print(f'a plan every {args.replan_every} control step(s), after a failed solve: {args.on_fail}')
    opponents = [('self-play', None)] + ([('pid', Drivers(kinds=['game', 'pid']))] if args.opponent == 'pid' else [])
    if args.track:
        opponents = [('tracked', Drivers(kinds=['track'] * s.M))]
    print('spread   car 2       chains with a contact   min clearance   mean clearance   mean box_excess   mean steps run   kernel [ms]   max jump / (dt rate_ub): u_a, u_steer   steps over the limit'
          + ('   held steps   fallback steps' if hold is not None else ''))
    for spread in args.spreads:
        fields = (('mass', 'drag_coefficient', 'yaw_inertia') if cross else ('mass', 'damping_coefficient') if args.model == 'point-mass'
                  else ('mass', 'drag_coefficient', 'slip_coefficient'))
        ens = perturbed_configs(nominal, {f: spread for f in fields}, B, args.seed)
        plant = PlantModel(dynamics_configs=nominal if cross else None, per_chain_configs=ens, method='rk4', M=2, sim_steps=args.sim_steps, own_class=cross)
        for name, drivers in opponents:
            r = s.step_batch(smp['x0'], smp['u_ws'], T, plant=plant, estimate_noise=noise, monitor='stop', drivers=drivers,
                             u_prev=True if args.carry_u_prev else None, hold=hold)
            worst, share = command_jumps(r, lim)
            print(f'{spread:6.3f}   {name:9s}   {np.mean(r["hit_step"] >= 0):21.4f}   {np.nanmin(r["clearance"]):13.4f}   {np.nanmean(r["clearance"]):14.4f}   '
                  f'{np.nanmean(r["box_excess"]):15.4f}   {r["steps_done"].mean():14.2f}   {r["kernel_ms"]:11.1f}   {worst[0]:27.3f}, {worst[1]:7.3f}   {share:20.4f}' + held_and_fallback(r, hold))


if __name__ == '__main__':
    main()
