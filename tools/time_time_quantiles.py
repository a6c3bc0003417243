"""What the per-member quantiles over time cost on BASELINE config C3 (100 000 members x 10 957 days, REACH-5, slot order,
table resident), on one MI355X.
`python tools/time_time_quantiles.py [--members N] [--end-dt YYYY-MM-DD] [--repeats R] [--warmup W] [--out DIR]`; one JSON line.

  (a) simplyp_time_quantiles, 'Q_cumecs' over the whole run, q = [0.05, 0.5, 0.95]            (device events, info.kernel_ms)
  (b) simplyp_time_quantiles, 'SRP_mgl' per calendar year, the same q
  (c) simplyp_waterbody over the same table: the project's yardstick for one coalesced pass over it
  (d) what a user with the device table can do today: torch.sort(out[Qr], dim=0) of the same [D, E] slice, then indexing
      the two ranks of each q (device events; the largest member count that fits beside the table, scaled to E if smaller)
Medians over the repeats after the warm-ups.  bytes_read counts every sweep's loads, so bytes_read / kernel_ms is the rate the
sweeps ran at and (bytes_read / one sweep's bytes) the mean number of sweeps; n_sweeps is the most any wave needed.  The
problem is built the way bench.py builds C3 (synthetic.c3_problem, slot-order output)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from simplyp_amd import abi, engine, marshal, synthetic

Q = [0.05, 0.5, 0.95]


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=100000)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sort-members', type=int, default=0, help='members of the slice leg (d) sorts (default: all, halved until it fits)')
    ap.add_argument('--out', default=None, help='directory that receives time_time_quantiles.json')
    args = ap.parse_args()
    import torch
    E = args.members
    eng = engine.get_engine(0)
    pr = synthetic.c3_problem(E, end_dt=args.end_dt, solver=dict(out_slot_order=1))
    rp = eng.to_device(pr['reach_params'])
    out, status, stats = eng.run(pr['forcing'], pr['doy'], pr['member_params'], rp, pr['up_ptr'], pr['up_idx'], pr['opts'])
    mos = stats['member_of_slot']
    mask = pr['opts'].out_mask
    D = int(out.shape[1])
    years = np.asarray(pr['met'].index.year)
    assert len(years) == D
    f_tdp = np.random.default_rng(synthetic.C3_SEED).uniform(0.5, 0.9, E)
    res = dict(members=E, days=D, columns=int(out.shape[0]), q=Q, table_bytes=int(out.numel()) * 8,
               run_kernel_ms=stats['kernel_ms'], repeats=args.repeats, warmup=args.warmup)
    n_runs = args.warmup + args.repeats

    def leg(series, pod):
        ms, info = [], None
        for k in range(n_runs):
            lo, hi, info = eng.time_quantiles(out, mask, Q, series=[abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index(series)],
                                              period_of_day=pod, f_tdp=f_tdp, reach_params=rp, member_of_slot=mos)
            if k >= args.warmup:
                ms.append(info['kernel_ms'])
        return ms, info, lo, hi

    a_ms, a_info, a_lo, a_hi = leg('Q_cumecs', None)
    one_sweep = 8 * E * D
    res.update(a_q_cumecs_whole_run_ms=median(a_ms), a_ms_all=a_ms, a_n_sweeps=a_info['n_sweeps'], a_bytes_read=int(a_info['bytes_read']),
               a_mean_sweeps=a_info['bytes_read'] / one_sweep, a_read_gbs=a_info['bytes_read'] / (median(a_ms) * 1e-3) / 1e9)
    b_ms, b_info, _, _ = leg('SRP_mgl', years - years[0])
    res.update(b_srp_annual_ms=median(b_ms), b_ms_all=b_ms, b_n_sweeps=b_info['n_sweeps'], b_bytes_read=int(b_info['bytes_read']),
               b_mean_sweeps=b_info['bytes_read'] / (2 * one_sweep), b_read_gbs=b_info['bytes_read'] / (median(b_ms) * 1e-3) / 1e9,
               b_periods=int(b_info['n_periods']))
    c_ms, c_info = [], None
    for k in range(n_runs):
        wb, c_info = eng.waterbody(out, mask, [0], 0.7, rp, member_of_slot=mos, columns=['Q_cumecs'])
        if k >= args.warmup:
            c_ms.append(c_info['kernel_ms'])
    del wb
    c_gbs = c_info['bytes_moved'] / (median(c_ms) * 1e-3) / 1e9
    res.update(c_waterbody_ms=median(c_ms), c_ms_all=c_ms, c_bytes_moved=int(c_info['bytes_moved']), c_moved_gbs=c_gbs,
               a_rate_over_c=res['a_read_gbs'] / c_gbs, b_rate_over_c=res['b_read_gbs'] / c_gbs)

    # ---- (d) torch.sort of the Qr slice along the day axis, then the ranks
    h = np.asarray(Q) * np.float64(D - 1)
    k_lo = np.floor(h).astype(np.int64)
    k_hi = np.minimum(k_lo + 1, D - 1)
    idx = torch.from_numpy(np.concatenate([k_lo, k_hi])).to(out.device)
    col = out[marshal.columns_of_mask(mask).index('Qr'), :, 0, :]               # [D, E], the slice leg (a) reads
    Es = args.sort_members or E
    d_ms = None
    while Es >= 1024:
        try:
            d_ms = []
            for k in range(n_runs):
                sl = col[:, :Es]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                picked = torch.sort(sl, dim=0).values[idx]
                t1.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    d_ms.append(t0.elapsed_time(t1))
            break
        except RuntimeError:                                                   # out of device memory: half the members
            d_ms = None
            torch.cuda.empty_cache()
            Es //= 2
    if d_ms is not None:
        # the sorted Qr, scaled like Q_cumecs, is leg (a)'s answer (a positive factor keeps the order): a check of both
        A = rp[marshal.PR_NAMES.index('A_catch'), 0][mos.long()[:Es]]
        want = picked * A * 1000 / 86400
        got = torch.cat([a_lo[:, 0, 0, 0, :Es], a_hi[:, 0, 0, 0, :Es]])
        res.update(d_torch_sort_ms=median(d_ms) * E / Es, d_ms_all=d_ms, d_sorted_members=Es,
                   d_agrees_with_a=bool(torch.equal(want, got)),
                   a_not_slower_than_d=bool(median(a_ms) <= median(d_ms) * E / Es))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_time_quantiles.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
