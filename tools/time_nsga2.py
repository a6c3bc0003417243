"""What a generation of find_pareto costs on the 30-year Tarland run.
`python tools/time_nsga2.py [--pop N] [--gens G] [--end-dt YYYY-MM-DD] [--out DIR]`; one JSON line.

sp.find_pareto over fc, T_g and E_M within +-30 % of the workbook's values on NSE(Q), NSE(TP) and |Bias (%)|(Q): a first call of one
generation warms up, a second call of G generations is timed.  Reports, per generation after the initial population's, the wall
time and its split into the model run, the goodness-of-fit reduction, the Pareto ranks (whose front peeling makes one host round
trip per front of the 2 N set), crowding, selection and offspring kernels (device events), the number of fronts of every
generation, and the share of the wall time no kernel accounts for."""
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

NAMES = ['fc', 'T_g', 'E_M']
OBJECTIVES = [('NSE', 'Q'), ('NSE', 'TP'), ('Bias (%)', 'Q')]
KERNELS = ['run_kernel_ms', 'gof_ms', 'pareto_ms', 'crowding_ms', 'select_ms', 'offspring_ms']


def summary(xs):
    return dict(mean=float(np.mean(xs)), median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pop', type=int, default=4096)
    ap.add_argument('--gens', type=int, default=8)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--out', default=None, help='directory that receives time_nsga2_<pop>.json')
    args = ap.parse_args()
    fresh = lambda: synthetic.tarland_inputs(end_dt=args.end_dt)
    obs_dict = synthetic.tarland_observations(end_dt=args.end_dt)
    p = fresh()[5]
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in NAMES}
    kw = dict(priors=priors, objectives=OBJECTIVES, n_pop=args.pop, seed=2016)
    t0 = time.perf_counter()
    sp.find_pareto(*fresh(), obs_dict, n_gen=1, **kw)
    t1 = time.perf_counter()
    r = sp.find_pareto(*fresh(), obs_dict, n_gen=args.gens, **kw)
    t2 = time.perf_counter()
    st, h = r['stats'], r['history']
    pick = lambda k: st[k][1:]                               # the generations that breed: offspring, run, ranks of 2 N members
    wall = summary(pick('wall_ms'))
    kernels = sum(float(np.mean(pick(k))) for k in KERNELS)
    res = dict(pop=args.pop, days=len(fresh()[0]), gens=args.gens, generation_wall_ms=wall,
               host_share_of_wall=1.0 - kernels / wall['mean'], initial_generation_wall_ms=st['wall_ms'][0],
               n_fronts=h['n_fronts'], n_front0=h['n_front0'], n_invalid=h['n_invalid'], best_first_last=[h['best'][0].tolist(), h['best'][-1].tolist()],
               labels=r['labels'], call_wall_s=dict(warmup_call=t1 - t0, timed_call=t2 - t1))
    for k in KERNELS:
        res[k] = summary(pick(k))
        res[k]['share_of_wall'] = res[k]['mean'] / wall['mean']
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_nsga2_%d.json' % args.pop), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
