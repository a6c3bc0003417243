"""What the lag-one sums cost beside the goodness-of-fit reduction on the same daily table (C3: 100 000 members x 30 years,
REACH-5 columns in slot order) against the shipped Tarland observations: both entries' kernel times in one run, interleaved,
their algorithmic bytes and what those make of the HBM roofline.  The lag pass reads the rows simplyp_gof reads plus one row
(four for a chemistry day) per slice of a day list, so its time is to be read against simplyp_gof's.
Usage: python tools/time_residual_lag.py [members] [reps]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import helpers
from simplyp_amd import abi, engine, marshal, synthetic, visualise_results as vr

E = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
eng = engine.get_engine(0)
pr = synthetic.c3_problem(E, solver=dict(out_slot_order=1, rtol=1e-6, atol=1e-8))     # the table's content does not matter here
rp = eng.to_device(pr['reach_params'])
out, status, st = eng.run(pr['forcing'], pr['doy'], pr['member_params'], rp, pr['up_ptr'], pr['up_idx'], pr['opts'])
obs = vr.observation_array(helpers.observations('1981-01-01', '2010-12-31'), [1], pr['met'].index)
kw = dict(member_of_slot=st['member_of_slot'])
ms = dict(gof=[], lag=[])
for _ in range(reps):                                # interleaved: both see the same clocks and the same cache state
    gof, ginfo = eng.gof(out, marshal.MASK_REACH5, obs, 0.7, rp, **kw)
    ms['gof'].append(ginfo['kernel_ms'])
    lag, linfo = eng.gof_lag(out, marshal.MASK_REACH5, obs, 0.7, rp, **kw)
    ms['lag'].append(linfo['kernel_ms'])
for name, info in (('gof', ginfo), ('lag', linfo)):
    t = float(np.median(ms[name][1:])) if reps > 1 else ms[name][0]
    print('%s E=%d: %d discharge days + %d chemistry days, %d/%d slices; %.1f MB algorithmic; kernels %.3f ms (median of %d; min %.3f, max %.3f) '
          '-> %.0f GB/s = %.1f %% of 8 TB/s' % (name, E, info['n_q_days'], info['n_chem_days'], info['n_chunks_q'], info['n_chunks_chem'],
                                                 info['bytes_read'] / 1e6, t, max(1, reps - 1), min(ms[name][1:] or ms[name]),
                                                 max(ms[name][1:] or ms[name]), info['bytes_read'] / t / 1e6, info['bytes_read'] / t / 1e6 / 80.0),
          flush=True)
print('re-read rows: %.3f MB (%.4f %% of the lag pass)' % ((linfo['bytes_read'] - ginfo['bytes_read']) / 1e6,
                                                           100.0 * (linfo['bytes_read'] - ginfo['bytes_read']) / linfo['bytes_read']))
lg = lag.cpu().numpy()
q = abi.GOF_VARS.index('Q')
with np.errstate(all='ignore'):
    phi = lg[3, q, 0] / lg[2, q, 0]
print('Q: n_link %d of %d observations; phi_hat median %.3f (5 %% %.3f, 95 %% %.3f) over %d finite members'
      % (int(np.nanmax(lg[0, q, 0])), int(gof.cpu().numpy()[0, q, 0, 0]), np.nanmedian(phi), np.nanpercentile(phi, 5),
         np.nanpercentile(phi, 95), int(np.isfinite(phi).sum())))
