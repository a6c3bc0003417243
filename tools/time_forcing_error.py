"""What forcing uncertainty costs at BASELINE C3's size (100 000 members x 10 957 days, sigma_P = 0.3, daily groups).

Three device-resident timings with torch events, one warm-up and three repeats each:
  1. the run with ``forcing_error`` (the generator, then the run on the generated table);
  2. the same run handed the kept table explicitly as E forcing sets: (1) - (2) is the generator;
  3. the shared-forcing run of today: (2) - (3) is what per-member forcing reads cost the main kernel.
Prints one JSON line; ``--md FILE`` also writes the figures as a table.  ``--members`` / ``--days`` shrink the problem.
``--rho`` makes the errors of P autocorrelated (the AR(1) generator kernel instead of the independent one), ``--groups`` picks
``'day'`` | ``'month'`` | ``'year'`` groups.
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--members', type=int, default=100000)
    ap.add_argument('--days', type=int, default=0, help='0 = all 10 957')
    ap.add_argument('--sigma', type=float, default=0.3)
    ap.add_argument('--rho', type=float, default=0.0, help='lag-one correlation of the P errors; > 0: the AR(1) generator')
    ap.add_argument('--groups', default='day', choices=['day', 'month', 'year'])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()

    import torch
    from simplyp_amd import engine, forcing, synthetic
    E = args.members
    pr = synthetic.c3_problem(E, solver=dict(out_slot_order=1))
    if args.days:
        pr['forcing'], pr['doy'], pr['met'] = pr['forcing'][:, :, :args.days].copy(), pr['doy'][:args.days].copy(), pr['met'].iloc[:args.days]
    D = pr['forcing'].shape[2]
    eng = engine.get_engine(0)
    fe = forcing.resolve({'P': {'sigma': args.sigma, 'rho': args.rho, 'groups': args.groups}}, pr['met'].index, E, False, seed=1)
    dev = {k: eng.to_device(pr[k]) for k in ('forcing', 'doy', 'member_params', 'reach_params')}
    out = torch.empty((5, D, 1, E), dtype=torch.float64, device=eng.tdev)
    mos = torch.empty((E,), dtype=torch.int32, device=eng.tdev)
    ident = torch.arange(E, dtype=torch.int32, device=eng.tdev)

    def one(f, **kw):
        return eng.run(f, dev['doy'], dev['member_params'], dev['reach_params'], pr['up_ptr'], pr['up_idx'], pr['opts'], out=out,
                       member_of_slot=mos, **kw)[2]

    def timed(fn):
        fn()                                                    # warm-up
        ms, stats = [], None
        for _ in range(args.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            stats = fn()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms, stats

    torch.cuda.synchronize(eng.tdev)
    stream = torch.cuda.Stream(eng.tdev)
    with torch.cuda.stream(stream):
        ms1, st1 = timed(lambda: one(dev['forcing'], forcing_error=fe))
        table = one(dev['forcing'], forcing_error=fe, keep_forcing_table=True)['forcing_table']
        ms2, st2 = timed(lambda: one(table, forcing_of_member=ident))
        del table
        ms3, st3 = timed(lambda: one(dev['forcing']))
    table_bytes = E * 2 * D * 8
    gen_ms = float(np.median(ms1) - np.median(ms2))
    res = dict(members=E, days=D, sigma_P=args.sigma, rho_P=args.rho, groups=args.groups, table_bytes=table_bytes,
               with_forcing_error_ms=ms1, explicit_table_ms=ms2, shared_forcing_ms=ms3,
               kernel_ms=[st1['kernel_ms'], st2['kernel_ms'], st3['kernel_ms']], pilot_ms=[st1['pilot_ms'], st2['pilot_ms'], st3['pilot_ms']],
               rhs_per_member_day=[st['rhs_evals'] / float(E * D) for st in (st1, st2, st3)],
               simt_efficiency=[st['simt_efficiency'] for st in (st1, st2, st3)],
               generator_ms=gen_ms, generator_write_gbs=table_bytes / gen_ms / 1e6 if gen_ms > 0 else None,
               per_member_reads_ms=float(np.median(ms2) - np.median(ms3)))
    print(json.dumps(res))
    if args.md:
        med = lambda x: float(np.median(x))
        with open(args.md, 'w') as fh:
            fh.write("| run (%d members x %d days, sigma_P = %g, rho_P = %g, %s groups) | median ms | repeats ms | main launch ms | pilot ms |\n|---|---|---|---|---|\n"
                     % (E, D, args.sigma, args.rho, args.groups))
            for name, ms, k in (('1. forcing_error', ms1, 0), ('2. kept table given explicitly', ms2, 1), ('3. shared forcing', ms3, 2)):
                fh.write("| %s | %.1f | %s | %.1f | %.1f |\n" % (name, med(ms), ', '.join('%.1f' % x for x in ms), res['kernel_ms'][k], res['pilot_ms'][k]))
            fh.write("\nRight-hand sides per member-day: %s; SIMT efficiency: %s.\n"
                     % (', '.join('%.2f' % x for x in res['rhs_per_member_day']), ', '.join('%.3f' % x for x in res['simt_efficiency'])))
            fh.write("\nTable: %.2f GB.  Generator (1 - 2): %.1f ms = %s GB/s of table writes.  Per-member forcing reads in the main kernel (2 - 3): %.1f ms.\n"
                     % (table_bytes / 1e9, gen_ms, 'n/a' if gen_ms <= 0 else '%.0f' % res['generator_write_gbs'], res['per_member_reads_ms']))


if __name__ == '__main__':
    main()
