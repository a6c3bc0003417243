"""How the members of tests/golden/dry_network.npz and tests/golden/branch_network.npz were chosen: the CPU oracle's default solver
against Cash-Karp alone at rtol 1e-11 / atol 1e-13, every member of a `members`-member draw of C4's distribution, over the fixture's
period, compared over ALL reaches and the 9 reach columns.
  --network dry (default): config C4's chain (upper `reaches` reaches) on the dry climate (precipitation x DRY_PSCALE, PET / DRY_PSCALE);
      prints per member the worst error and the reach it is at, then the members with the largest errors and those whose headwater
      comes nearest to drying (smallest minimum daily Qr of reach 1).
  --network branch: the branching network of simplyp_amd.synthetic.branch_inputs on Tarland's own climate (`reaches` is the network's
      22 and may be left out); prints per member the worst error, the reach it is at and the mean outlet Qr, then the members with the
      largest errors and those with the largest mean outlet Qr.
Usage: python tools/sweep_dry_network.py [--network dry|branch] [members reaches st_dt end_dt threads]"""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import time
import numpy as np
from simplyp_amd import marshal, synthetic
from oracle import oracle
import helpers

ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
ap.add_argument('--network', choices=('dry', 'branch'), default='dry')
ap.add_argument('rest', nargs='*', help='members reaches st_dt end_dt threads')
args = ap.parse_args()
argv = args.rest
BRANCH = args.network == 'branch'
E = int(argv[0]) if len(argv) > 0 else (64 if BRANCH else 256)
S = int(argv[1]) if len(argv) > 1 else (len(synthetic.BRANCH_UPSTREAM) if BRANCH else 32)
ST, EN = (argv[2], argv[3]) if len(argv) > 3 else ('1981-01-01', '1982-12-31')
THREADS = int(argv[4]) if len(argv) > 4 else 8
if BRANCH and S != len(synthetic.BRANCH_UPSTREAM):
    sys.exit('--network branch has %d reaches' % len(synthetic.BRANCH_UPSTREAM))

mask = sum(1 << marshal.OUT_COLUMNS.index(c) for c in helpers.REACH_COLS)     # (OUT_COLUMNS order: Vr, Qr_EndOfDay, Qr, ...)
QR = [c for c in marshal.OUT_COLUMNS if c in helpers.REACH_COLS].index('Qr')


def run(solver):
    if BRANCH:
        pr = helpers.branch_network_inputs(E, ST, EN, solver=solver, out_mask=mask)
    else:
        pr = helpers.dry_network_inputs(E, S, ST, EN, solver=solver, out_mask=mask)
    t0 = time.time()
    out, status, stats = oracle.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'], pr['up_ptr'], pr['up_idx'],
                                    pr['opts'], n_threads=THREADS)
    assert status.max() == 0
    print('%s: %.1f s, %.1f rhs per catchment-day' % (solver, time.time() - t0, stats['rhs_evals'] / (E * S * out.shape[1])), flush=True)
    return out


truth = run(dict(rtol=1e-11, atol=1e-13, stiff_pair=-1))
got = run(None)
rel = np.abs(got - truth) / np.maximum(np.abs(truth), 1e-300)
rel = np.where(got == truth, 0.0, rel)
per_reach = rel.max(axis=(0, 1))                       # [S, E]
worst = per_reach.max(axis=0)
worst_reach = per_reach.argmax(axis=0) + 1
if BRANCH:
    qr_out = truth[QR, :, S - 1, :].mean(axis=0)
    for e in range(E):
        print('member %3d  worst %.2e at reach %2d  mean outlet Qr %.3f' % (e, worst[e], worst_reach[e], qr_out[e]))
else:
    qr_head = truth[QR, :, 0, :].min(axis=0)
    for e in range(E):
        print('member %3d  worst %.2e at reach %2d  headwater min Qr %.3e' % (e, worst[e], worst_reach[e], qr_head[e]))
print('worst %.2e (member %d, reach %d), median %.2e' % (worst.max(), worst.argmax(), worst_reach[worst.argmax()], np.median(worst)))
print('largest errors:', [(int(e), '%.2e' % worst[e], int(worst_reach[e])) for e in np.argsort(-worst)[:8]])
if BRANCH:
    print('largest mean outlet Qr:', [(int(e), '%.3f' % qr_out[e], '%.2e' % worst[e], int(worst_reach[e])) for e in np.argsort(-qr_out)[:8]])
else:
    print('driest headwaters:', [(int(e), '%.3e' % qr_head[e], '%.2e' % worst[e], int(worst_reach[e])) for e in np.argsort(qr_head)[:8]])
