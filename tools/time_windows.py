"""What cutting a run into time windows costs, on one MI355X.
`python tools/time_windows.py [--members N] [--end-dt YYYY-MM-DD] [--repeats R] [--leg c3|strong] [--out DIR]`; one JSON line.

  c3      BASELINE config C3 (100 000 members x 1981-2010, REACH-5, table left on the device): ONE call against the same run as
          annual windows (run_simply_p_ensemble_windows, the state threaded through on the device): wall of each, and per window
          wall, kernel_ms and pilot_ms.  The two alternate inside one process; the first pair is a warm-up.  The windows' summed
          rhs_evals must equal the one call's (the same integration, step for step) -- asserted.
  strong  the strong_1m shape (--members 1000000) as daily REACH-5 windows of one year each (~15 GB per window), left on the
          device and reduced there to quantiles=[0.025, 0.5, 0.975]: the daily band of an ensemble whose whole table (440 GB)
          fits nowhere; time per window and in all.  There is no one-call counterpart.

Wall clock around calls that end synchronised; the problem is built the way bench.py builds C3."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import simplyp_amd as sp
from simplyp_amd import synthetic

Q = [0.025, 0.5, 0.975]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=['c3', 'strong'], default='c3')
    ap.add_argument('--members', type=int, default=None)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--out', default=None, help='directory that receives time_windows_<leg>.json')
    args = ap.parse_args()
    import torch
    E = args.members or (100000 if args.leg == 'c3' else 1000000)
    inputs = synthetic.tarland_inputs('1981-01-01', args.end_dt)
    seed = synthetic.C3_SEED + (100 if args.leg == 'strong' else 0)
    over = synthetic.monte_carlo_overrides(inputs[5], inputs[3], E, seed)
    solver = dict(out_slot_order=1) if args.leg == 'c3' else None

    def fresh():
        return [x.copy() for x in inputs]

    def one_call():
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            r = sp.run_simply_p_ensemble(*fresh(), overrides=over, solver=solver, to_host=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r['stats']

    def windows(**kw):
        per, t_all = [], time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            gen = sp.run_simply_p_ensemble_windows(*fresh(), window='annual', overrides=over, solver=solver, to_host=False, **kw)
            t0 = time.perf_counter()
            for w in gen:
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                d = dict(year=int(w['window'][0].year), wall_ms=(t1 - t0) * 1e3, kernel_ms=w['stats']['kernel_ms'],
                         pilot_ms=w['stats']['pilot_ms'], run_wall_ms=w['stats']['wall_ms'], rhs_evals=int(w['stats']['rhs_evals']),
                         flagged=int((w['status'] != 0).sum().item()))
                if 'quantiles' in w:
                    d['quantiles_ms'] = w['quantiles']['info']['kernel_ms']
                    d['median_qr_mean'] = float(np.nanmean(w['quantiles']['data'][1, 1]))
                per.append(d)
                del w
                t0 = time.perf_counter()
        return (time.perf_counter() - t_all) * 1e3, per

    res = dict(leg=args.leg, members=E, end_dt=args.end_dt, repeats=args.repeats)
    if args.leg == 'c3':
        ones, wins = [], []
        for k in range(args.repeats + 1):
            t1, st = one_call()
            tw, per = windows()
            assert sum(p['rhs_evals'] for p in per) == st['rhs_evals'], "the windows did not take the one call's steps"
            if k:
                ones.append(dict(wall_ms=t1, kernel_ms=st['kernel_ms'], pilot_ms=st['pilot_ms'], run_wall_ms=st['wall_ms']))
                wins.append(dict(wall_ms=tw, kernel_ms=sum(p['kernel_ms'] for p in per), pilot_ms=sum(p['pilot_ms'] for p in per),
                                 run_wall_ms=sum(p['run_wall_ms'] for p in per), per_window=per))
        res.update(one_call=ones, windows=wins, n_windows=len(wins[0]['per_window']),
                   windows_over_one_call_wall=min(w['wall_ms'] for w in wins) / min(o['wall_ms'] for o in ones),
                   windows_over_one_call_kernel=min(w['kernel_ms'] for w in wins) / min(o['kernel_ms'] for o in ones))
    else:
        tw, per = windows(quantiles=Q, keep_daily=False)
        res.update(q=Q, total_wall_ms=tw, per_window=per, window_table_gb=5 * 8 * 365.25 * E / 1e9)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_windows_%s.json' % args.leg), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
