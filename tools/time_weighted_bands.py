"""What a weighted band costs beside the unweighted one on BASELINE config C3's table (100 000 members x 10 957 days, one
column: Qr), on one MI355X.  `python tools/time_weighted_bands.py [--members N] [--end-dt YYYY-MM-DD] [--repeats R] [--warmup W]
[--out DIR]`; one JSON line.

  (w) simplyp_weighted_quantiles on the device-resident table for q = [0.025, 0.5, 0.975], weights from a simplyp_pf_weights
      call on log weights that fall off with the distance of a member's mean flow from the ensemble's median (a Gaussian
      likelihood of one summary statistic)
  (u) simplyp_quantiles on the same table in the same session: the same select under its unweighted policy, the yardstick
  (e) (w) again with all weights equal: what the weights' spread itself costs
and the sweeps per row of each, the quotient (w) / (u), the table bytes per second each sweep reaches, and the HBM floor of one
sweep: 8 B per member and row at the MI355X's nominal 8 TB/s (the weight vector, 8 B per member, stays in cache).  Device events
(info.kernel_ms), the minimum over the repeats.  With SIMPLYP_HIP_LIB naming a library built with -DSIMPLYP_WQ_NO_MERGE the same
run times the weighted select without its wave merge (the macro sets WQSelect::MERGE_ROUNDS in simplyp_quantile.hip.h to 0)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simplyp_amd import engine, marshal, synthetic

Q = [0.025, 0.5, 0.975]
HBM_GBS = 8000.0            # the MI355X's nominal HBM3E bandwidth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=100000)
    ap.add_argument('--end-dt', default='2010-12-31')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='directory that receives time_weighted_bands.json')
    args = ap.parse_args()
    import torch
    E = args.members
    eng = engine.get_engine(0)
    pr = synthetic.c3_problem(E, end_dt=args.end_dt, out_mask=marshal.mask_of_columns(['Qr']))
    out, status, stats = eng.run(pr['forcing'], pr['doy'], pr['member_params'], eng.to_device(pr['reach_params']), pr['up_ptr'],
                                 pr['up_idx'], pr['opts'])
    D = int(out.shape[1])
    mean = out[0, :, 0, :].mean(dim=0)
    centre = mean[torch.isfinite(mean)].median()
    lw = -0.5 * ((mean - centre) / (0.25 * centre)) ** 2
    w_d, q_d, pinfo = eng.pf_weights(lw.contiguous())
    res = dict(members=E, days=D, q=Q, table_bytes=int(out.numel()) * 8, run_kernel_ms=stats['kernel_ms'], repeats=args.repeats,
               warmup=args.warmup, weights_alive=pinfo['n_alive'], weights_ess=pinfo['sum_w'] ** 2 / pinfo['sum_w2'])

    def timed(call):
        ms, info = [], None
        for k in range(args.warmup + args.repeats):
            info = call()
            if k >= args.warmup:
                ms.append(info['kernel_ms'])
        return min(ms), ms, info

    w_ms, w_all, w_info = timed(lambda: eng.weighted_quantiles(out, Q, q_d)[1])
    u_ms, u_all, u_info = timed(lambda: eng.quantiles(out, Q)[2])
    e_ms, e_all, e_info = timed(lambda: eng.weighted_quantiles(out, Q, torch.full_like(q_d, 1 << 40))[1])
    floor_ms = 8.0 * E * D / (HBM_GBS * 1e9) * 1e3
    res.update(weighted_ms=w_ms, weighted_ms_all=w_all, weighted_passes=w_info['n_passes'], weighted_n_used=w_info['n_used'],
               weight_total=int(w_info['T']), unweighted_ms=u_ms, unweighted_ms_all=u_all, unweighted_passes=u_info['n_passes'],
               equal_weights_ms=e_ms, equal_weights_ms_all=e_all, equal_weights_passes=e_info['n_passes'], weighted_over_unweighted=w_ms / u_ms,
               hbm_floor_ms_per_sweep=floor_ms, weighted_ms_per_sweep=w_ms / max(w_info['n_passes'], 1),
               unweighted_ms_per_sweep=u_ms / max(u_info['n_passes'], 1),
               weighted_table_gbs_per_sweep=8.0 * E * D * w_info['n_passes'] / (w_ms * 1e-3) / 1e9,
               unweighted_table_gbs_per_sweep=8.0 * E * D * u_info['n_passes'] / (u_ms * 1e-3) / 1e9)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'time_weighted_bands.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
