"""What the predictive band costs on BASELINE config C3 (100 000 members x 10 957 days, REACH-5), one series, on one MI355X.
`python tools/time_predictive.py [--members N] [--end-dt YYYY-MM-DD] [--repeats R] [--warmup W] [--out DIR]`; one JSON line.

  (a) simplyp_predictive_bands of 'Q_cumecs', q = [0.025, 0.5, 0.975], err_m NULL: the series generated, no draws  (gen_ms, kernel_ms)
  (b) the same with err_m = 0.1: Philox4x32-10, log, sqrt and cospi per member and day                            (gen_ms, kernel_ms)
  (c) simplyp_quantiles on the plain column Qr of the same table: the same rows selected where they lie, nothing generated
  (d) simplyp_waterbody over the table: the project's yardstick for one coalesced pass
Device events throughout (info.kernel_ms / info.gen_ms); medians after the warm-ups, with minimum and maximum.  The
generation pass reads one column and writes one series: its HBM floor is 16 B per member and day over the copy bandwidth --
the 2.65 TB/s section 5 records for (d), and what (d) gives in this session.  The problem is built the way bench.py builds C3
(synthetic.c3_problem, slot-order output)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from simplyp_amd import abi, engine, marshal, synthetic

Q = [0.025, 0.5, 0.975]
COPY_TBS_SECTION5 = 2.65          # simplyp_waterbody over C3's table, DESIGN.md section 5


def summary(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), all=[float(x) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=100000)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='directory that receives time_predictive.json')
    args = ap.parse_args()
    E = args.members
    eng = engine.get_engine(0)
    pr = synthetic.c3_problem(E, end_dt=args.end_dt, solver=dict(out_slot_order=1))
    rp = eng.to_device(pr['reach_params'])
    out, status, stats = eng.run(pr['forcing'], pr['doy'], pr['member_params'], rp, pr['up_ptr'], pr['up_idx'], pr['opts'])
    mos = stats['member_of_slot']
    mask = pr['opts'].out_mask
    D = int(out.shape[1])
    inc = (status & abi.STATUS_NONFINITE) == 0
    series = [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index('Q_cumecs')]
    res = dict(members=E, days=D, q=Q, series='Q_cumecs', run_kernel_ms=stats['kernel_ms'], repeats=args.repeats, warmup=args.warmup)
    n = args.warmup + args.repeats

    for leg, m in (('a_param_only', None), ('b_overall', 0.1)):
        gen, ker, info = [], [], None
        for k in range(n):
            lo, up, info = eng.predictive_bands(out, mask, Q, series, err_m=m, seed=2016, include=inc, f_tdp=0.7, reach_params=rp,
                                                member_of_slot=mos)
            if k >= args.warmup:
                gen.append(info['gen_ms']); ker.append(info['kernel_ms'])
        res[leg] = dict(gen_ms=summary(gen), kernel_ms=summary(ker), n_chunks=info['n_chunks'], n_passes=info['n_passes'],
                        n_used=info['n_used'], bytes_read=info['bytes_read'], bytes_workspace=info['bytes_workspace'],
                        band_median_mean=float(lo[1].mean()))
        del lo, up
    col = out[marshal.columns_of_mask(mask).index('Qr')]
    c_ms, c_info = [], None
    for k in range(n):
        lo, up, c_info = eng.quantiles(col, Q, include=inc, member_of_slot=mos)
        if k >= args.warmup:
            c_ms.append(c_info['kernel_ms'])
    res['c_quantiles_plain_column'] = dict(kernel_ms=summary(c_ms), n_passes=c_info['n_passes'], bytes_table=c_info['bytes_table'])
    d_ms, d_info = [], None
    for k in range(n):
        wb, d_info = eng.waterbody(out, mask, [0], 0.7, rp, member_of_slot=mos, columns=['Q_cumecs'])
        if k >= args.warmup:
            d_ms.append(d_info['kernel_ms'])
    d_tbs = d_info['bytes_moved'] / (float(np.median(d_ms)) * 1e-3) / 1e12
    res['d_waterbody'] = dict(kernel_ms=summary(d_ms), bytes_moved=int(d_info['bytes_moved']), tbs=d_tbs)

    moved = 16 * E * D                                   # the generation pass: one column read, one series written
    ga, gb = res['a_param_only']['gen_ms']['median'], res['b_overall']['gen_ms']['median']
    ka, kb = res['a_param_only']['kernel_ms']['median'], res['b_overall']['kernel_ms']['median']
    kc = res['c_quantiles_plain_column']['kernel_ms']['median']
    res.update(gen_bytes_moved=moved,
               gen_floor_ms_section5=moved / (COPY_TBS_SECTION5 * 1e12) * 1e3, gen_floor_ms_this_session=moved / (d_tbs * 1e12) * 1e3,
               gen_tbs_param_only=moved / (ga * 1e-3) / 1e12, gen_tbs_overall=moved / (gb * 1e-3) / 1e12,
               draws_per_s=E * D / (gb * 1e-3), draw_cost_ms=gb - ga,
               param_only_over_plain_quantiles=ka / kc, overall_over_plain_quantiles=kb / kc)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_predictive.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
