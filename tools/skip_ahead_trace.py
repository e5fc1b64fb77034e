"""Summarise a `rocprofv3 --kernel-trace --output-format csv` run of eager hr steps (bench.py --eager) for the skip-ahead
branch: the LAST step of the trace, the nested lr net's chain in it and what ran beside it.

    python tools/skip_ahead_trace.py <kernel_trace.csv> [--step-csv OUT.csv]

A step starts at its timestep_embedding kernel.  The lr chain is taken from the first to the last kernel that only the
dense net launches (gn_fused_rows*, attention_mfma*), on the queue of the first of them; "beside" = kernels on another
hardware queue whose interval intersects the chain's.  Times are the kernels' own start / end stamps: an eager step under the tracer is host-bound, so
the chain's wall span is longer than in a replayed hipGraph -- the kernels' summed durations are the comparable figure.
"""
import argparse
import csv
import re


def short(name):
    name = re.sub(r'^void\s+', '', name)
    return re.split(r'[<(]', name)[0].split('::')[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('csv')
    ap.add_argument('--step-csv', default=None, help='write the last step\'s rows (name, queue, start us, duration us) here')
    a = ap.parse_args()
    rows = [r for r in csv.DictReader(open(a.csv)) if r['Kind'] == 'KERNEL_DISPATCH']
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    names = [short(r['Kernel_Name']) for r in rows]
    starts = [i for i, n in enumerate(names) if n.startswith('timestep_embedding')]
    assert len(starts) >= 2, 'no whole step in the trace'
    step = list(zip(names, rows))[starts[-1]:]
    t0 = int(step[0][1]['Start_Timestamp'])
    ev = [(n, r['Queue_Id'], (int(r['Start_Timestamp']) - t0) / 1e3, (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
          for n, r in step]
    lr_only = [e for e in ev if e[0].startswith('gn_fused_rows') or e[0].startswith('attention_mfma')]
    chain_q = lr_only[0][1]            # (a replayed hipGraph puts its branches on queues of the runtime's choosing)
    c0, c1 = lr_only[0][2], max(e[2] + e[3] for e in lr_only)
    chain = [e for e in ev if e[1] == chain_q and c0 <= e[2] and e[2] + e[3] <= c1]
    side = [e for e in ev if e[1] != chain_q and e[2] < c1 and e[2] + e[3] > c0]
    overlap = sum(max(0.0, min(c1, e[2] + e[3]) - max(c0, e[2])) for e in side)
    print('last step: %d kernels on queues %s' % (len(ev), sorted(set(e[1] for e in ev))))
    print('lr chain (queue %s): %d kernels at %.1f .. %.1f us of the step, wall span %.1f us, summed kernel time %.1f us'
          % (chain_q, len(chain), c0, c1, c1 - c0, sum(e[3] for e in chain)))
    print('kernels of other queues that intersect the chain: %d, summed %.1f us, of which %.1f us inside the chain'
          % (len(side), sum(e[3] for e in side), overlap))
    for n in sorted(set(e[0] for e in side)):
        sel = [e for e in side if e[0] == n]
        print('  %-28s x %2d  %8.1f us  (first at %.1f us)' % (n, len(sel), sum(e[3] for e in sel), sel[0][2]))
    if a.step_csv:
        with open(a.step_csv, 'w') as f:
            f.write('kernel,queue,start_us,duration_us\n')
            for e in ev:
                f.write('%s,%s,%.2f,%.2f\n' % e)


if __name__ == '__main__':
    main()
