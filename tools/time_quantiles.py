"""What the percentile band costs on BASELINE config C3 (100 000 members x 10 957 days, REACH-5), on one MI355X.
`python tools/time_quantiles.py [--members N] [--end-dt YYYY-MM-DD] [--repeats R] [--warmup W] [--out DIR]`; one JSON line.

  (a) simplyp_quantiles on the device-resident table for q = [0.025, 0.5, 0.975]              (device events, info.kernel_ms)
  (b) simplyp_waterbody over the same table: the project's yardstick for one coalesced pass over it
  (c) the whole call run_simply_p_ensemble(..., quantiles=q, keep_daily=False): the band, the table never leaving the device
  (d) the same call with quantiles=None, to_host=True: today's way of merely delivering the rows (before any host percentiles)
(c) and (d) alternate inside one process; wall clock around calls that end synchronised.  The problem is built the way
bench.py builds C3 (synthetic.tarland_inputs + monte_carlo_overrides, slot-order output).  Under
`rocprofv3 --pmc FETCH_SIZE -- python tools/time_quantiles.py --only-a` only leg (a) runs (counters in a run of their own)."""
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
from simplyp_amd import abi, engine, marshal, synthetic

Q = [0.025, 0.5, 0.975]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=100000)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--only-a', action='store_true', help='leg (a) only, once warmed up: for a counters-only profiler run')
    ap.add_argument('--out', default=None, help='directory that receives time_quantiles.json')
    args = ap.parse_args()
    import torch
    E = args.members
    eng = engine.get_engine(0)
    solver = dict(out_slot_order=1)

    # ---- (a), (b): the table resident, one run
    pr = synthetic.c3_problem(E, end_dt=args.end_dt, solver=solver)
    rp = eng.to_device(pr['reach_params'])
    out, status, stats = eng.run(pr['forcing'], pr['doy'], pr['member_params'], rp, pr['up_ptr'], pr['up_idx'], pr['opts'])
    mos = stats['member_of_slot']
    D = out.shape[1]
    res = dict(members=E, days=D, columns=int(out.shape[0]), q=Q, table_bytes=int(out.numel()) * 8,
               run_kernel_ms=stats['kernel_ms'], run_wall_ms=stats['wall_ms'], repeats=args.repeats, warmup=args.warmup)
    inc = (status & abi.STATUS_NONFINITE) == 0
    a_ms, a_info = [], None
    for k in range(args.warmup + args.repeats):
        lo, hi, a_info = eng.quantiles(out, Q, include=inc, member_of_slot=mos)
        if k >= args.warmup:
            a_ms.append(a_info['kernel_ms'])
    res.update(a_quantiles_ms=min(a_ms), a_quantiles_ms_all=a_ms, n_passes=a_info['n_passes'], n_used=a_info['n_used'],
               a_table_gbs=a_info['bytes_table'] / (min(a_ms) * 1e-3) / 1e9)
    if args.only_a:
        print(json.dumps(res))
        return
    b_ms, b_info = [], None
    for k in range(args.warmup + args.repeats):
        wb, b_info = eng.waterbody(out, pr['opts'].out_mask, [0], 0.7, rp, member_of_slot=mos, columns=['Q_cumecs'])
        if k >= args.warmup:
            b_ms.append(b_info['kernel_ms'])
    del wb
    # the yardstick reads 4 of the table's columns (32 B per member and day) and writes one series: per byte of table read
    b_read = 32 * E * D
    res.update(b_waterbody_ms=min(b_ms), b_waterbody_ms_all=b_ms, b_bytes_moved=int(b_info['bytes_moved']),
               b_moved_gbs=b_info['bytes_moved'] / (min(b_ms) * 1e-3) / 1e9,
               a_over_b=min(a_ms) / min(b_ms),
               a_over_b_per_table_byte=(min(a_ms) / a_info['bytes_table']) / (min(b_ms) / b_read))
    del out, lo, hi
    torch.cuda.empty_cache()

    # ---- (c), (d): the public call, alternating
    inputs = synthetic.tarland_inputs('1981-01-01', args.end_dt)
    over = synthetic.monte_carlo_overrides(inputs[5], inputs[3], E, synthetic.C3_SEED)

    def call(**kw):
        met_df, p_struc, p_SU, p_LU, p_SC, p, dyn = (x.copy() for x in inputs)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            r = sp.run_simply_p_ensemble(met_df, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=over, solver=solver, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    c_ms, d_ms, c_run, d_run, c_q, pinned = [], [], [], [], [], None
    for k in range(args.warmup + args.repeats):
        t, r = call(quantiles=Q, keep_daily=False)
        assert r['data'] is None and r['stats']['streamed_chunks'] == 0
        if k >= args.warmup:
            c_ms.append(t); c_run.append(r['stats']['wall_ms']); c_q.append(r['quantiles']['info']['kernel_ms'])
        band = r['quantiles']['data']
        del r
        t, r = call(to_host=True)
        if k >= args.warmup:
            d_ms.append(t); d_run.append(r['stats']['wall_ms'])
        del r
    res.update(c_band_call_ms=min(c_ms), c_band_call_ms_all=c_ms, c_run_wall_ms=min(c_run), c_quantiles_ms=min(c_q),
               d_rows_to_host_call_ms=min(d_ms), d_rows_to_host_call_ms_all=d_ms, d_run_wall_ms=min(d_run),
               c_shorter_than_d=bool(min(c_ms) < min(d_ms)), c_shorter_than_d_run_alone=bool(min(c_ms) < min(d_run)),
               band_bytes=int(band.nbytes), band_median_qr_mean=float(np.nanmean(band[1, 1])))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_quantiles.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
