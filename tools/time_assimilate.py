"""What a window of the particle filter costs on the 30-year Tarland record, step by step.
`python tools/time_assimilate.py [--particles E] [--window DAYS] [--end-dt YYYY-MM-DD] [--threshold X] [--out DIR]`; one JSON line.

sp.assimilate over the shipped discharge observations with fc, T_g, a_Q and m_Q filtered inside +-30 % of the workbook's values
(m_Q in [0.01, 1)), E particles (default 100 000), windows of DAYS days (default 30).  One warm-up call over the first two
windows, then the timed call over the whole record.  Per window the kernel times of run, loglik, weights, resample, gather and
jitter (device events) and the run's pilot_ms; reported as medians over the windows, with the filter's overhead (everything but
the run) against the run, and the call's wall time."""
import argparse
import json
import os
import sys
import time

ROOT = os.environ.get('SIMPLYP_TREE') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # env: time another checkout
sys.path.insert(0, ROOT)
import numpy as np
import simplyp_amd as sp
from simplyp_amd import synthetic

STEPS = ['run', 'loglik', 'weights', 'resample', 'gather', 'jitter']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=100000)
    ap.add_argument('--window', type=int, default=30)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--threshold', type=float, default=1.0)
    ap.add_argument('--out', default=None, help='directory that receives time_assimilate.json')
    args = ap.parse_args()
    fresh = lambda: synthetic.tarland_inputs(end_dt=args.end_dt)
    obs_dict = synthetic.tarland_observations(end_dt=args.end_dt)
    p = fresh()[5]
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    kw = dict(priors=priors, variables=['Q'], n_particles=args.particles, window=args.window, seed=2016,
              resample_threshold=args.threshold)
    a = fresh()
    first = a[0].index.get_loc(obs_dict[1]['Q'].first_valid_index())                      # warm-up over two windows that hold observations:
    sp.assimilate(a[0].iloc[first:first + 2 * args.window], *a[1:], obs_dict, **kw)       # workspaces, torch's allocator
    t0 = time.perf_counter()
    r = sp.assimilate(*fresh(), obs_dict, **kw)
    wall = time.perf_counter() - t0
    ms = {k: np.asarray(r['kernel_ms'][k]) for k in STEPS}
    full = np.array([hi - lo == args.window for _, _, lo, hi in r['windows']])
    did = r['resampled'] & full
    overhead = sum(ms[k] for k in STEPS[1:])
    res = dict(particles=args.particles, window=args.window, days=len(fresh()[0]), n_windows=len(r['windows']),
               n_resampled=int(r['resampled'].sum()), wall_s=wall, wall_ms_per_window_median=float(np.median(r['wall_ms'])),
               median_ms={k: float(np.median(ms[k][did])) for k in STEPS}, max_ms={k: float(ms[k][did].max()) for k in STEPS},
               pilot_ms_median=float(np.median(np.asarray(r['pilot_ms'])[full])),
               overhead_ms_median=float(np.median(overhead[did])), overhead_over_run_median=float(np.median(overhead[did] / ms['run'][did])),
               sum_ms={k: float(ms[k].sum()) for k in STEPS}, ess_median=float(np.median(r['ess'])),
               n_unique_median=float(np.median(r['n_unique'])), n_outside_median=float(np.median(r['n_outside'])),
               log_evidence_total=r['log_evidence_total'])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_assimilate.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
