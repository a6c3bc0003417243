"""What scoring a forecast costs on BASELINE config C3 (100 000 members x 10 957 days, REACH-5) against Tarland's discharge
observations 1981-2010 (data/Coull_DailyMeanQ.xlsx), on one MI355X.
`python tools/time_scores.py [--members N] [--end-dt YYYY-MM-DD] [--repeats R] [--warmup W] [--out DIR]`; one JSON line.

  (a) simplyp_predictive_scores of 'Q_cumecs', err_m NULL: the parameter-only forecast              (kernel_ms, gen_ms, sort_ms)
  (b) the same with err_m = 0.1: the overall forecast, the error model drawn for the observed rows   (kernel_ms, gen_ms, sort_ms)
  (c) (a) under integer weights (a made-up likelihood weighting, a third of the members at 0)
  (d) simplyp_predictive_bands_weighted of the same series under the same weights, q = [0.025, 0.5, 0.975], err_m NULL: every
      day of the run, a radix select of three ranks per row -- the neighbour a reader can place the scores beside
Device events throughout (the infos' kernel_ms / gen_ms / sort_ms); medians after the warm-ups, with minimum and maximum.  Only
the observed days are generated and sorted by (a) to (c); (d) generates and selects all of them.  The problem is built the way
bench.py builds C3 (synthetic.c3_problem, slot-order output)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pandas as pd
from simplyp_amd import abi, engine, synthetic, xlsx

Q = [0.025, 0.5, 0.975]


def summary(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), all=[float(x) for x in xs])


def discharge_observations(index):
    """[1, D, 1]: the observed daily mean discharge on the run's days, NaN where there is none."""
    df = xlsx.read_excel(xlsx.Workbook(os.path.join(ROOT, 'data', 'Coull_DailyMeanQ.xlsx')), '1', index_col=0)
    df.index = pd.to_datetime(df.index)
    df = df[~df.index.duplicated(keep='first')].sort_index().reindex(index)
    return np.ascontiguousarray(df['Q'].to_numpy(dtype=float).reshape(1, -1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=100000)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None, help='directory that receives time_scores.json')
    args = ap.parse_args()
    E = args.members
    eng = engine.get_engine(0)
    pr = synthetic.c3_problem(E, end_dt=args.end_dt, solver=dict(out_slot_order=1))
    rp = eng.to_device(pr['reach_params'])
    out, status, stats = eng.run(pr['forcing'], pr['doy'], pr['member_params'], rp, pr['up_ptr'], pr['up_idx'], pr['opts'])
    mos = stats['member_of_slot']
    mask = pr['opts'].out_mask
    D = int(out.shape[1])
    obs = discharge_observations(pr['met'].index)
    inc = (status & abi.STATUS_NONFINITE) == 0
    series = [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index('Q_cumecs')]
    rng = np.random.default_rng(2016)
    weights = rng.integers(1, (1 << 40) + 1, E).astype(np.int64)
    weights[rng.random(E) < 1.0 / 3.0] = 0
    res = dict(members=E, days=D, n_obs=int((~np.isnan(obs)).sum()), series='Q_cumecs', tile=abi.SCORE_TILE, run_kernel_ms=stats['kernel_ms'],
               repeats=args.repeats, warmup=args.warmup)
    n = args.warmup + args.repeats
    kw = dict(seed=2016, include=inc, f_tdp=0.7, reach_params=rp, member_of_slot=mos)

    for leg, m, w in (('a_param_only', None, None), ('b_overall', 0.1, None), ('c_param_only_weighted', None, weights)):
        ms = dict(kernel_ms=[], gen_ms=[], sort_ms=[])
        info = sums = None
        for k in range(n):
            sums, counts, info = eng.predictive_scores(out, mask, series, obs, err_m=m, weights=w, **kw)
            if k >= args.warmup:
                for key in ms:
                    ms[key].append(info[key])
        crps = (sums[0] - sums[1]).cpu().numpy()
        res[leg] = dict({key: summary(v) for key, v in ms.items()}, n_chunks=info['n_chunks'], n_rows_scored=info['n_rows_scored'],
                        n_used=info['n_used'], bytes_read=info['bytes_read'], bytes_workspace=info['bytes_workspace'],
                        mean_crps=float(np.nanmean(crps)))
        del sums, counts
    d_ms, d_info = [], None
    for k in range(n):
        values, d_info = eng.predictive_bands(out, mask, Q, series, weights=weights, **kw)
        if k >= args.warmup:
            d_ms.append(d_info['kernel_ms'])
    res['d_predictive_bands_weighted'] = dict(kernel_ms=summary(d_ms), n_passes=d_info['n_passes'], n_used=d_info['n_used'], rows=D)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_scores.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
