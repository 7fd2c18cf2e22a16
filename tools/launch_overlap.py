#!/usr/bin/env python3
"""How the dg_solve_kernel launches of a pipelined run overlap, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py
    python3 tools/launch_overlap.py DIR            (or the *_kernel_trace.csv itself)

For every dg_solve_kernel dispatch: queue id, stream id, start and end (ms from the first timed dispatch), its length, how long it
ran concurrently with its predecessor, and the gap between the predecessor's end and its start (negative: they overlapped).
Then, over the timed region -- from the start of the first timed dispatch to the end of the last one --: the time during which
no dg_solve_kernel was running, the summed kernel time over the region's length (R: 1 = one after the other), and how many
consecutive launches shared a queue.

The timed region is the dispatches after the first `--warmup` ones (bench.py's warm-up steps are single launches before the
region; default 1) and, with `--launches N`, the N dispatches from there on (default: bench.py's 10; 0 = all that remain: the
legs bench.py --full runs after the timed region would otherwise be counted)."""
import argparse
import csv
import pathlib
import sys


def read_dispatches(path, kernel):
    p = pathlib.Path(path)
    files = [p] if p.is_file() else sorted(p.rglob('*kernel_trace.csv'))
    if not files:
        sys.exit(f'launch_overlap: no *kernel_trace.csv under {p}')
    rows = []
    for f in files:
        with open(f, newline='') as fh:
            for r in csv.DictReader(fh):
                if kernel in r['Kernel_Name']:
                    rows.append(dict(queue=r['Queue_Id'], stream=r.get('Stream_Id', '?'), start=int(r['Start_Timestamp']), end=int(r['End_Timestamp']),
                                     grid=int(r['Grid_Size_X']) // max(1, int(r['Workgroup_Size_X']))))
    rows.sort(key=lambda r: r['start'])
    return rows


def idle_time(rows, t0, t1):
    """ns of [t0, t1] covered by no dispatch"""
    idle, reach = 0, t0
    for r in rows:
        if r['start'] > reach:
            idle += r['start'] - reach
        reach = max(reach, r['end'])
    return idle + max(0, t1 - reach)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('trace', help='the kernel-trace CSV of rocprofv3, or a directory that holds it')
    ap.add_argument('--kernel', default='dg_solve_kernel')
    ap.add_argument('--warmup', type=int, default=1, help='leading dispatches that are not part of the timed region')
    ap.add_argument('--launches', type=int, default=10, help='dispatches of the timed region (0: all that remain)')
    a = ap.parse_args()
    rows = read_dispatches(a.trace, a.kernel)
    timed = rows[a.warmup:a.warmup + a.launches] if a.launches > 0 else rows[a.warmup:]
    if not timed:
        sys.exit(f'launch_overlap: {len(rows)} {a.kernel} dispatches, none left after --warmup {a.warmup}')
    t0, t1 = timed[0]['start'], max(r['end'] for r in timed)
    ms = lambda ns: ns / 1e6
    print(f'{a.kernel}: {len(rows)} dispatches in the trace, {len(timed)} in the timed region (after {a.warmup} warm-up)')
    print(f'{"#":>3} {"queue":>5} {"stream":>6} {"wgs":>5} {"start ms":>10} {"end ms":>10} {"length ms":>10} {"with prev ms":>12} {"gap to prev ms":>14}')
    same_queue = 0
    for j, r in enumerate(timed):
        if j == 0:
            both, gap = '', ''
        else:
            p = timed[j - 1]
            both = f'{ms(max(0, min(r["end"], p["end"]) - max(r["start"], p["start"]))):.1f}'
            gap = f'{ms(r["start"] - p["end"]):.1f}'
            same_queue += r['queue'] == p['queue']
        print(f'{j:>3} {r["queue"]:>5} {r["stream"]:>6} {r["grid"]:>5} {ms(r["start"] - t0):>10.1f} {ms(r["end"] - t0):>10.1f} {ms(r["end"] - r["start"]):>10.1f} {both:>12} {gap:>14}')
    busy = sum(r['end'] - r['start'] for r in timed)
    idle = idle_time(timed, t0, t1)
    print(f'timed region {ms(t1 - t0):.1f} ms; no {a.kernel} running for {ms(idle):.1f} ms ({100.0 * idle / (t1 - t0):.1f} %)')
    print(f'summed kernel time {ms(busy):.1f} ms = {busy / (t1 - t0):.2f} x the region (R; 1.00 = one launch after the other)')
    print(f'queues used: {len({r["queue"] for r in timed})}; consecutive launches on the same queue: {same_queue} of {len(timed) - 1}')


if __name__ == '__main__':
    main()
