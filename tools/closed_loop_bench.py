#!/usr/bin/env python3
"""B closed-loop runs of T steps: the host loop a user had to write before step_batch against step_batch itself.

(a) host loop: T rounds of ``solve_batch`` (default cooperative mode), numpy ``closed_loop.feedback``, re-upload -- T launches, each
    ending with its slowest scenario, and 2 T copies;
(b) ``step_batch``: one launch that ends with its longest chain, no intermediate copies (and no line-search helpers, no deferral).

Game and size: BASELINE configs[1] (dyn_curve_N25), B = 1,024, T = 10, no disturbance, inputs from the device sampler.  The two are
alternated ``--repeats`` times in one process after one warm-up each; times are host clocks around synchronous calls.  The script also
asserts that both produce identical status, num_iters and q.

    python tools/closed_loop_bench.py [--out profiles/closed_loop_dyn_curve_N25.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'closed_loop_dyn_curve_N25.txt'))
    args = ap.parse_args()
    from dgsqp_amd.montecarlo import dynamic_racing_game
    from dgsqp_amd.solver import DGSQP
    g = dynamic_racing_game(N=25, rk4_substeps=10)               # BASELINE configs[1]
    s = DGSQP(*g.solver_args(), print_method=None, qp_method='active_set')
    B, T = args.batch, args.steps
    smp = s.sample_batch(g, B, seed=args.seed)
    x0, u_am = smp['x0'], s._to_agent_major(smp['u_ws'])

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    run_a = lambda: host_loop(s, x0, u_am, T)
    run_b = lambda: s.step_batch(x0, u_am, T)
    _, a = timed(run_a)                                          # warm-up of each (code objects, buffers)
    _, b = timed(run_b)
    for key in ('status', 'num_iters', 'q'):
        assert np.array_equal(a[key], b[key], equal_nan=(key == 'q')), f'{key}: host loop and step_batch differ'
    ta, tb, ka, kb = [], [], [], []
    for _ in range(args.repeats):
        dt, a = timed(run_a); ta.append(dt); ka.append(a['kernel_ms'] / 1e3)
        dt, b = timed(run_b); tb.append(dt); kb.append(b['kernel_ms'] / 1e3)
    st = b['status']
    fmt = lambda v: f'median {np.median(v) * 1e3:.1f} ms (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})'
    lines = [f'closed loop, dyn_curve_N25 (BASELINE configs[1]), B = {B} chains x T = {T} steps, no disturbance, device-sampled inputs (seed {args.seed}); {args.repeats} alternated repeats after one warm-up each',
             f'(a) host loop: {T} x solve_batch (cooperative line search + deferral) + numpy feedback + re-upload: wall {fmt(ta)}; kernels alone {fmt(ka)}',
             f'(b) step_batch: one launch of dg_closed_loop_kernel:                                               wall {fmt(tb)}; kernel alone {fmt(kb)}',
             f'(b) / (a), medians of the wall times: {np.median(tb) / np.median(ta):.3f}   ((a) / (b) = {np.median(ta) / np.median(tb):.3f})',
             f'identical status, num_iters and q in (a) and (b): yes (asserted); steps run {int((st >= 0).sum())} of {B * T}, converged {np.mean((st >= 0) & (st <= 1)):.3f}, '
             f'iterations per step: mean {b["num_iters"].mean():.2f}, max {int(b["num_iters"].max())}; per chain: mean {b["num_iters"].sum(axis=1).mean():.1f}, max {int(b["num_iters"].sum(axis=1).max())}']
    text = '\n'.join(lines)
    print(text)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(text + '\n')


if __name__ == '__main__':
    main()
