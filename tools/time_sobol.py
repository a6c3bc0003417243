"""What Sobol' indices with bootstrap intervals cost on the 30-year Tarland run, on the device and done on the host.
`python tools/time_sobol.py [--mode device|host] [--base N] [--boot B] [--host-boot K] [--end-dt YYYY-MM-DD] [--out DIR]`; one JSON line.

  device  sp.sobol_indices over ten member parameters within +-20 % of the workbook's values, N base samples (default 8 192:
          98 304 members), annual sums of Qr and PP_kg/day, B bootstrap resamples (default 1 000).  One warm-up call with 64 base
          samples, then the timed call: its wall time and split (the run's kernel, the design, validity + counts, the contraction,
          the quantile selection; device events), and the contraction's rate against its own count of useful fp64 operations,
          2 (1 + B) n_rows N (2 d + 2), at the 78.6 TFLOP/s vector peak.  The design is written to DIR/time_sobol_x.npy.
  host    the same analysis without anything this feature added, so it runs unchanged on the commit before it (SIMPLYP_TREE names
          that checkout): after a warm-up call of 768 members, run_simply_p_ensemble(overrides = that design, outputs,
          reduce='annual'), the table on the host, then
          the bootstrap with fancy indexing (a[idx], b[idx], ab[:, idx] per resample and row, scipy's saltelli_2010 formulas).
          K resamples are timed (default 50) and the cost of B stated as K's scaled up, which is marked as such.
          `--points FILE`: the array `device` wrote.
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

NAMES = ['fc', 'T_g', 'a_Q', 'b_Q', 'beta', 'alpha', 'f_quick', 'E_M', 'k_M', 'T_s_A']
COLUMNS = ['Qr', 'PP_kg/day']
PEAK_FP64_VECTOR = 78.6e12


def workbook_value(p, p_LU, name):
    from simplyp_amd import marshal
    return float(marshal.member_params(p, p_LU, 1)[marshal.PM_NAMES.index(name), 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['device', 'host'], default='device')
    ap.add_argument('--base', type=int, default=8192)
    ap.add_argument('--boot', type=int, default=1000)
    ap.add_argument('--host-boot', type=int, default=50)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--points', default=None, help='host: the design [10, E] the device mode wrote')
    ap.add_argument('--out', default=None, help='directory that receives time_sobol_<mode>.json')
    args = ap.parse_args()
    fresh = lambda: synthetic.tarland_inputs(end_dt=args.end_dt)
    inputs = fresh()
    d = len(NAMES)
    res = dict(mode=args.mode, base=args.base, dims=d, boot=args.boot, days=len(inputs[0]), columns=COLUMNS)
    if args.mode == 'device':
        a = fresh()
        from simplyp_amd import marshal
        marshal.prologue(a[2], a[3], a[4], a[5])
        priors = {nm: tuple(sorted((0.8 * workbook_value(a[5], a[3], nm), 1.2 * workbook_value(a[5], a[3], nm)))) for nm in NAMES}
        kw = dict(priors=priors, columns=COLUMNS, reduce='annual', n_boot=args.boot, seed=2016)
        t0 = time.perf_counter()
        sp.sobol_indices(*fresh(), n_base=64, **kw)
        t1 = time.perf_counter()
        r = sp.sobol_indices(*fresh(), n_base=args.base, **kw)
        t2 = time.perf_counter()
        st = r['stats']
        n_rows = int(np.prod(r['S1'].shape[1:]))
        flops = 2.0 * (1 + args.boot) * n_rows * args.base * (2 * d + 2)
        res.update(members=int(r['x'].shape[1]), n_rows=n_rows, n_valid=int(r['n_valid']), stats=st,
                   call_wall_s=dict(warmup_call=t1 - t0, timed_call=t2 - t1),
                   contraction=dict(flops=flops, tflops=flops / (st['contract_ms'] * 1e-3) / 1e12 if st['contract_ms'] > 0 else None,
                                    share_of_vector_peak=flops / (st['contract_ms'] * 1e-3) / PEAK_FP64_VECTOR if st['contract_ms'] > 0 else None),
                   analysis_ms=st['design_ms'] + st['counts_ms'] + st['contract_ms'] + st['quantile_ms'],
                   ST_Qr_last_year={nm: [float(r['ST'][k, 0, -1, 0]), float(r['ST_conf'][0, k, 0, -1, 0]), float(r['ST_conf'][1, k, 0, -1, 0])]
                                    for k, nm in enumerate(NAMES)})
        x = r['x']
    else:
        x = np.load(args.points)
        N = x.shape[1] // (d + 2)
        over = {nm: x[k].copy() for k, nm in enumerate(NAMES)}
        sp.run_simply_p_ensemble(*fresh(), overrides={nm: v[:768].copy() for nm, v in over.items()}, outputs=COLUMNS, reduce='annual')   # warm-up
        t0 = time.perf_counter()
        e = sp.run_simply_p_ensemble(*fresh(), overrides=over, outputs=COLUMNS, reduce='annual')
        t1 = time.perf_counter()
        rows = np.asarray(e['data']).reshape(-1, x.shape[1])
        fa, fb, fab = rows[:, :N], rows[:, N:2 * N], rows[:, 2 * N:].reshape(len(rows), d, N)
        mean = np.mean(np.concatenate([fa, fb], axis=1), axis=1)
        fa, fb, fab = fa - mean[:, None], fb - mean[:, None], fab - mean[:, None, None]
        rng = np.random.default_rng(2016)
        K = args.host_boot
        s1, st_ = np.empty((K, len(rows), d)), np.empty((K, len(rows), d))
        t2 = time.perf_counter()
        for k in range(K):
            idx = rng.integers(0, N, N)
            ra, rb, rab = fa[:, idx], fb[:, idx], fab[:, :, idx]
            var = np.var(np.concatenate([ra, rb], axis=1), axis=1)
            s1[k] = np.mean(rb[:, None, :] * (rab - ra[:, None, :]), axis=-1) / var[:, None]
            st_[k] = 0.5 * np.mean((ra[:, None, :] - rab) ** 2, axis=-1) / var[:, None]
        t3 = time.perf_counter()
        res.update(members=int(x.shape[1]), n_rows=int(len(rows)), run_call_wall_ms=1e3 * (t1 - t0), run_kernel_ms=e['stats']['kernel_ms'],
                   host_boot_resamples=K, host_boot_wall_ms=1e3 * (t3 - t2),
                   host_boot_wall_ms_scaled_to_boot=1e3 * (t3 - t2) * args.boot / max(K, 1),
                   total_wall_ms_scaled=1e3 * (t1 - t0) + 1e3 * (t3 - t2) * args.boot / max(K, 1))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        if args.mode == 'device':
            np.save(os.path.join(args.out, 'time_sobol_x.npy'), x)
        with open(os.path.join(args.out, 'time_sobol_%s.json' % args.mode), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
