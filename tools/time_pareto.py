"""What Pareto counts and ranks cost on the goodness-of-fit table of BASELINE config C3 (100 000 members, REACH-5, against the
shipped Tarland observations), on one MI355X.
`python tools/time_pareto.py [--members N] [--end-dt YYYY-MM-DD] [--repeats R] [--warmup W] [--host-members H] [--out DIR]`; one
JSON line.

Objective rows come from a real simplyp_gof table: the first 2, 3 and 6 of a fixed preference list whose rows are finite for
most members (which variables qualify depends on the observation record).  One M = 3 case of i.i.d. normals stands beside them.
Per case, minimum of R calls after W warm-ups, device events (the info's kernel_ms):
  full      Engine.pareto with counts and ranks
  counts    rank=False: prepare + the all-pairs pass           ->  peel    = full - counts
  prepare   the same call with an all-zero include mask: the flag, scan, compact and fill launches and the read-back of n with
            nobody taking part (the compaction then writes no key)   ->  count = counts - prepare
  counts_scalar   as counts with SIMPLYP_PARETO_JLOAD=scalar: the j keys read from memory with wave-uniform addresses instead of
            LDS tiles
and the yardsticks a user without the entry has for the same rows:
  torch     both counts by a blocked broadcast comparison in torch on the same device (rows of 1024 members against all),
            device events, minimum of R -- counts only, to be set beside `count`
  host      simplyp_amd.pareto.ranks (blocked NumPy, counts and ranks) on the first H members, wall clock, once, and that time
            scaled by (n / H)^2 -- an extrapolation, stated as one."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import helpers
from simplyp_amd import abi, engine, marshal, pareto, synthetic, visualise_results as vr

PREFERENCE = [('NSE', 'Q'), ('NSE', 'TP'), ('Bias (%)', 'Q'), ('NSE', 'SS'), ('NSE', 'PP'), ('NSE', 'TDP'), ('log NSE', 'Q'),
              ('nRMSD (%)', 'Q'), ('NSE', 'SRP'), ('Bias (%)', 'TP'), ('Bias (%)', 'SS'), ('r2', 'Q')]


def torch_counts(y, block=1024):
    """Both counts of y [M, n] (larger is better, no NaN) by broadcast comparison, a block of rows at a time."""
    n = y.shape[1]
    by = torch.empty(n, dtype=torch.int32, device=y.device)
    of = torch.empty(n, dtype=torch.int32, device=y.device)
    for lo in range(0, n, block):
        mine = y[:, lo:lo + block, None]
        ge = (y[:, None, :] >= mine).all(dim=0)
        le = (y[:, None, :] <= mine).all(dim=0)
        by[lo:lo + block] = (ge & ~le).sum(dim=1)
        of[lo:lo + block] = (le & ~ge).sum(dim=1)
    return by, of


def best(fn, warmup, repeats):
    ms, last = [], None
    for k in range(warmup + repeats):
        last = fn()
        if k >= warmup:
            ms.append(last['kernel_ms'])
    return float(min(ms)), last


def case(eng, obj, sense, args):
    E = int(obj.shape[1])
    full_ms, full = best(lambda: eng.pareto(obj, sense), args.warmup, args.repeats)
    counts_ms, counts = best(lambda: eng.pareto(obj, sense, rank=False), args.warmup, args.repeats)
    prep_ms, _ = best(lambda: eng.pareto(obj, sense, rank=False, include=np.zeros(E, dtype=bool)), args.warmup, args.repeats)
    os.environ['SIMPLYP_PARETO_JLOAD'] = 'scalar'
    try:
        scalar_ms, scalar = best(lambda: eng.pareto(obj, sense, rank=False), args.warmup, args.repeats)
    finally:
        del os.environ['SIMPLYP_PARETO_JLOAD']
    assert bool((scalar['dominated_by'] == counts['dominated_by']).all()) and bool((scalar['dominates'] == counts['dominates']).all())
    assert bool((full['dominated_by'] == counts['dominated_by']).all())
    # the torch yardstick on the participants, larger is better
    keep = ~torch.isnan(obj).any(dim=0)
    y = (obj * torch.tensor(sense, dtype=torch.float64, device=obj.device)[:, None])[:, keep].contiguous()
    t_ms = []
    for k in range(args.warmup + args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        by, of = torch_counts(y)
        b.record()
        torch.cuda.synchronize()
        if k >= args.warmup:
            t_ms.append(a.elapsed_time(b))
    assert bool((by == counts['dominated_by'][keep]).all()) and bool((of == counts['dominates'][keep]).all())
    n = int(full['n_used'])
    count_ms = counts_ms - prep_ms
    return dict(M=int(obj.shape[0]), n_used=n, n_fronts=int(full['n_fronts']), n_front0=int(full['n_front0']),
                pair_tests=int(full['pair_tests']), full_ms=full_ms, counts_ms=counts_ms, prepare_ms=prep_ms, count_ms=count_ms,
                peel_ms=full_ms - counts_ms, counts_scalar_ms=scalar_ms, count_scalar_ms=scalar_ms - prep_ms,
                pair_tests_per_s_count=float(n) * n / (count_ms * 1e-3) if count_ms > 0 else None,
                pair_tests_per_s_full=full['pair_tests'] / (full_ms * 1e-3),
                torch_counts_ms=float(min(t_ms)), torch_over_count=float(min(t_ms)) / count_ms if count_ms > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=100000)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--host-members', type=int, default=20000)
    ap.add_argument('--out', default=None, help='directory that receives time_pareto.json')
    args = ap.parse_args()
    E = args.members
    eng = engine.get_engine(0)
    pr = synthetic.c3_problem(E, end_dt=args.end_dt, solver=dict(out_slot_order=1))
    rp = eng.to_device(pr['reach_params'])
    out, status, stats = eng.run(pr['forcing'], pr['doy'], pr['member_params'], rp, pr['up_ptr'], pr['up_idx'], pr['opts'])
    obs = vr.observation_array(helpers.observations('1981-01-01', args.end_dt), [1], pr['met'].index)
    gof, ginfo = eng.gof(out, marshal.MASK_REACH5, obs, 0.7, rp, member_of_slot=stats['member_of_slot'])
    del out
    resolved = [r for r in pareto.resolve_objectives(PREFERENCE[:8]) + pareto.resolve_objectives(PREFERENCE[8:])]
    rows = pareto.objective_rows(gof, None, resolved)
    good = [k for k in range(len(resolved)) if int(torch.isfinite(rows[k]).sum()) > E // 2]
    res = dict(members=E, days=int(len(pr['met'])), run_kernel_ms=stats['kernel_ms'], gof_kernel_ms=ginfo['kernel_ms'],
               repeats=args.repeats, warmup=args.warmup, jtile=abi.PARETO_JTILE, jsplit=abi.PARETO_JSPLIT, cases={})
    for M in (2, 3, 6):
        if len(good) < M:
            continue
        pick = good[:M]
        obj = rows[pick].contiguous()
        sense = [resolved[k]['sense'] for k in pick]
        res['cases']['gof_M%d' % M] = dict(case(eng, obj, sense, args), objectives=[resolved[k]['label'] for k in pick])
        if M == 3:                                   # the host yardstick, on the first H members
            H = min(args.host_members, E)
            sub = obj[:, :H].cpu().numpy()
            t0 = time.perf_counter()
            got = pareto.ranks(sub, sense)
            dt = time.perf_counter() - t0
            n = res['cases']['gof_M3']['n_used']
            res['host'] = dict(members=H, n_used=got['n_used'], n_fronts=got['n_fronts'], seconds=dt,
                               scaled_to_n_seconds=dt * (float(n) / max(1, got['n_used'])) ** 2,
                               over_full=dt * (float(n) / max(1, got['n_used'])) ** 2 * 1e3 / res['cases']['gof_M3']['full_ms'])
    normals = torch.from_numpy(np.random.default_rng(2016).standard_normal((3, E))).to(eng.tdev)
    res['cases']['normals_M3'] = dict(case(eng, normals, [1, 1, 1], args), objectives=['i.i.d. normal'] * 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_pareto.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
