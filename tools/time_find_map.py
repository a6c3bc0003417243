"""What an iteration of find_map costs on the 30-year Tarland run, against the call a host-driven optimiser would make.
`python tools/time_find_map.py [--mode map|loop] [--starts S] [--iters N] [--end-dt YYYY-MM-DD] [--out DIR]`; one JSON line.

  map    sp.find_map with S simplexes (default 2 048: runs of 8 192 members) over fc, T_g, a_Q within +-30 % of the workbook's
         values and m_Q in [0.01, 1): a first call of 2 iterations warms up, a second call with max_iter = N + 1 is timed.
         Reports the mean wall time of a run in which the simplexes step (every run after the initial simplex is evaluated) and
         its split into the run's kernel_ms, the goodness-of-fit reduction and the optimiser's kernels (propose, log_prob,
         update; device events).  The mirror replays the recorded values (and must arrive at the same simplexes); the run points
         of the last run in which every simplex stepped are written to DIR/time_find_map_points.npy.
  loop   run_simply_p_ensemble(overrides = those run points, obs_dict, keep_daily=False): what an optimiser on the host pays per
         iteration -- frames read, arrays marshalled, uploaded and allocated every time.  One warm-up call, then N calls; wall
         time and the run's kernel_ms.  Uses nothing that find_map added, so it runs unchanged on the commit before it
         (SIMPLYP_TREE names that checkout).  `--points FILE`: the array `map` wrote.
"""
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

NAMES = ['fc', 'T_g', 'a_Q']


def summary(xs):
    return dict(mean=float(np.mean(xs)), median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['map', 'loop'], default='map')
    ap.add_argument('--starts', type=int, default=2048)
    ap.add_argument('--iters', type=int, default=8)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--points', default=None, help='loop: an array [>= 3, 4 S] of run points')
    ap.add_argument('--out', default=None, help='directory that receives time_find_map_<mode>.json')
    args = ap.parse_args()
    S = args.starts
    inputs = synthetic.tarland_inputs(end_dt=args.end_dt)
    obs_dict = synthetic.tarland_observations(end_dt=args.end_dt)
    p = inputs[5]
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in NAMES}
    priors['m_Q'] = (0.01, 1.0)
    lo = np.array([v[0] for v in priors.values()]); hi = np.array([v[1] for v in priors.values()])
    res = dict(mode=args.mode, starts=S, members_per_run=4 * S, days=len(inputs[0]), iters=args.iters)
    if args.mode == 'map':
        from simplyp_amd import neldermead as nm
        fresh = lambda: synthetic.tarland_inputs(end_dt=args.end_dt)
        kw = dict(priors=priors, variables=['Q'], n_starts=S, seed=2016, record_evaluations=True)
        t0 = time.perf_counter()
        sp.find_map(*fresh(), obs_dict, max_iter=3, **kw)
        t1 = time.perf_counter()
        r = sp.find_map(*fresh(), obs_dict, max_iter=args.iters + 1, **kw)
        t2 = time.perf_counter()
        st = r['stats']
        first = -(-(len(priors) + 1) // 4)                       # the runs that evaluate the initial simplex
        pick = lambda k: st[k][first:]
        wall = summary(pick('wall_ms'))
        opt = summary(pick('optimiser_ms'))
        # the mirror's replay of the recorded values: the same simplexes, and the run points of every run
        runs, points = iter(range(len(r['evaluations']))), []

        def recorded(pts):
            points.append(pts)
            return -r['evaluation_log_prob'][next(runs)]

        rep = nm.run(recorded, None, lo, hi, max_iter=args.iters + 1, state=r['start'])
        same = bool(np.array_equal(rep['sim'], r['final_simplex'][0]) and np.array_equal(rep['fsim'], r['final_simplex'][1]))
        stepping = [k for k in range(first, len(points)) if st['n_shrinking'][k] == 0 and st['n_active'][k] == S]
        last = stepping[-1] if stepping else len(points) - 1
        res.update(step_run_wall_ms=wall, run_kernel_ms=summary(pick('run_kernel_ms')), gof_ms=summary(pick('gof_ms')),
                   optimiser_kernels_ms=opt, optimiser_share_of_wall=opt['mean'] / wall['mean'],
                   host_share_of_wall=1.0 - (np.mean(pick('run_kernel_ms')) + np.mean(pick('gof_ms')) + opt['mean']) / wall['mean'],
                   points_run=dict(index=last, wall_ms=st['wall_ms'][last], run_kernel_ms=st['run_kernel_ms'][last]),
                   n_runs=len(st['wall_ms']), n_shrinking=st['n_shrinking'], replay_equal=same,
                   call_wall_s=dict(warmup_call=t1 - t0, timed_call=t2 - t1),
                   moves={k: int(v.sum()) for k, v in r['moves'].items()}, best_fun=float(r['fun'].min()),
                   fun_median_first_last=[float(np.median(r['history'][0])), float(np.median(r['fun']))])
    else:
        pts = np.load(args.points)
        over = {nm_: pts[d].copy() for d, nm_ in enumerate(NAMES)}
        walls, kernels = [], []
        for k in range(1 + args.iters):
            a = [x.copy() for x in inputs]                 # the call edits p_LU / p_SC in place
            t0 = time.perf_counter()
            e = sp.run_simply_p_ensemble(*a, overrides=over, obs_dict=obs_dict, keep_daily=False)
            dt = 1e3 * (time.perf_counter() - t0)
            if k >= 1:
                walls.append(dt); kernels.append(e['stats']['kernel_ms'])
        res.update(members=int(pts.shape[1]), call_wall_ms=summary(walls), run_kernel_ms=summary(kernels),
                   gof_ms=float(e['gof']['info']['kernel_ms']))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        if args.mode == 'map':
            np.save(os.path.join(args.out, 'time_find_map_points.npy'), points[last])
        with open(os.path.join(args.out, 'time_find_map_%s.json' % args.mode), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
