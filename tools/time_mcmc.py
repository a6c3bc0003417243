"""What a half-step of sample_posterior costs on the 30-year Tarland run, against the call a user's own sampler loop would make.
`python tools/time_mcmc.py [--mode mcmc|loop] [--walkers W] [--steps N] [--warmup K] [--end-dt YYYY-MM-DD] [--out DIR]`; one JSON line.

  mcmc   sp.sample_posterior with W walkers (default 16 384: half-steps of 8 192 members), fc, T_g, a_Q within +-30 % of the
         workbook's values and m_Q in [0.01, 1), started from uniform draws in the central half of that box: K warm-up steps,
         then N steps continued through state=.  Reports the wall time of a half-step (median, min, max) and its split into the
         run's kernel_ms, the goodness-of-fit reduction and the three sampler kernels (device events).  The run's time depends on
         where the walkers are (the most expensive member sets it), so for a like-for-like figure the final positions are
         evaluated once more as the start of a chain of 0 steps (`same_members`: a half-step's run and reduction on exactly the
         members `loop --positions` runs) and written to DIR/time_mcmc_positions.npy.
  loop   run_simply_p_ensemble(overrides = the first W / 2 of the same start positions, obs_dict, keep_daily=False): what a
         sampler on the host calls once per half-step -- frames read, arrays marshalled, uploaded and allocated every time.
         K warm-up calls, then 2 N calls; wall time and the run's kernel_ms.  Uses nothing that sample_posterior added, so
         it runs unchanged on the commit before it.  `--positions FILE`: the first W / 2 columns of that array instead.
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
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['mcmc', 'loop'], default='mcmc')
    ap.add_argument('--walkers', type=int, default=16384)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--positions', default=None, help='loop: an array [>= 3, W] whose first W / 2 columns are the members')
    ap.add_argument('--out', default=None, help='directory that receives time_mcmc_<mode>.json')
    args = ap.parse_args()
    W = args.walkers
    inputs = synthetic.tarland_inputs(end_dt=args.end_dt)
    obs_dict = synthetic.tarland_observations(end_dt=args.end_dt)
    p = inputs[5]
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in NAMES}
    priors['m_Q'] = (0.01, 1.0)
    lo = np.array([v[0] for v in priors.values()]); hi = np.array([v[1] for v in priors.values()])
    u = np.random.default_rng(2016).uniform(0.25, 0.75, (len(priors), W))
    start = lo[:, None] + (hi - lo)[:, None] * u
    res = dict(mode=args.mode, walkers=W, members_per_half_step=W // 2, days=len(inputs[0]), steps=args.steps, warmup=args.warmup)
    if args.mode == 'mcmc':
        fresh = lambda: synthetic.tarland_inputs(end_dt=args.end_dt)
        kw = dict(priors=priors, variables=['Q'], n_walkers=W, seed=2016)
        t0 = time.perf_counter()
        warm = sp.sample_posterior(*fresh(), obs_dict, start=start, n_steps=args.warmup, **kw)
        t1 = time.perf_counter()
        r = sp.sample_posterior(*fresh(), obs_dict, state=warm['state'], n_steps=args.steps, **kw)
        t2 = time.perf_counter()
        again = sp.sample_posterior(*fresh(), obs_dict, start=r['state']['theta'], n_steps=0, **kw)['stats']
        st = r['stats']
        wall = summary(st['wall_ms'])
        res.update(half_step_wall_ms=wall, run_kernel_ms=summary(st['run_kernel_ms']), gof_ms=summary(st['gof_ms']),
                   sampler_kernels_ms=summary(st['sampler_ms']),
                   sampler_share_of_wall=float(np.median(st['sampler_ms'])) / wall['median'],
                   host_share_of_wall=1.0 - (float(np.median(st['run_kernel_ms'])) + float(np.median(st['gof_ms']))
                                             + float(np.median(st['sampler_ms']))) / wall['median'],
                   same_members=dict(wall_ms=again['start_wall_ms'], run_kernel_ms=again['start_run_kernel_ms']),
                   call_wall_s=dict(warmup_call=t1 - t0, timed_call=t2 - t1),
                   acceptance_fraction=float(r['acceptance_fraction'].mean()),
                   mean_inside=float(np.mean(st['n_inside'])) / (W // 2), log_prob_median=float(np.median(r['state']['lp'])))
    else:
        pos = start if args.positions is None else np.load(args.positions)
        over = {nm: pos[d, :W // 2].copy() for d, nm in enumerate(NAMES)}
        walls, kernels = [], []
        for k in range(args.warmup + 2 * args.steps):
            a = [x.copy() for x in inputs]                 # the call edits p_LU / p_SC in place
            t0 = time.perf_counter()
            e = sp.run_simply_p_ensemble(*a, overrides=over, obs_dict=obs_dict, keep_daily=False)
            dt = 1e3 * (time.perf_counter() - t0)
            if k >= args.warmup:
                walls.append(dt); kernels.append(e['stats']['kernel_ms'])
        res.update(call_wall_ms=summary(walls), run_kernel_ms=summary(kernels), gof_ms=float(e['gof']['info']['kernel_ms']),
                   columns=e['columns'])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        if args.mode == 'mcmc':
            np.save(os.path.join(args.out, 'time_mcmc_positions.npy'), r['state']['theta'])
        with open(os.path.join(args.out, 'time_mcmc_%s.json' % args.mode), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
