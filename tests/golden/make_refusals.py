"""The refusal census of the C ABI's analysis entries: every entry called through ``engine.lib()`` with one scalar argument its
own checks reject (E = 0, K above the maximum, half = 2, ...), and what it answers -- the return code, the text of
``simplyp_last_error`` and the bytes of the info struct it was handed.  Every case is refused on the host before any device work:
the device pointers all name one small scratch tensor that nothing touches, the host arrays are real.

``python tests/golden/make_refusals.py [out.json]`` (needs the built library and a GPU for the context) writes the census of
the tree it runs in; tests/golden/refusals.json was written that way at the commit BEFORE the entries were moved onto one entry
frame, and tests/test_gpu_refusals.py replays the cases against it byte for byte.  A case added later is recorded at the commit
that adds it.
"""

import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'refusals.json')
SENTINEL = 0xA5                 # every byte of an info before the call: a refused call leaves it so, or its case records what it wrote


def cases(h, dev):
    """[(entry, case label, arguments without the info, info class or None)].  h: a context handle; dev: the address of a device
    buffer of at least 32 KiB."""
    from simplyp_amd import abi, marshal
    dbl, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    keep = []                                           # the host arrays live as long as the list that is returned

    def hd(*v):
        a = np.ascontiguousarray(v, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(dbl)

    def hi(*v):
        a = np.ascontiguousarray(v, dtype=np.int32)
        keep.append(a)
        return a.ctypes.data_as(i32)

    def dims(E=4, S=1, D=3):
        d = abi.Dims(E, S, D, 1)
        keep.append(d)
        return C.byref(d)

    def head(mask=marshal.MASK_ALL, **kw):                     # what every entry over a daily table starts with
        return (h, dims(**kw), mask, None, 0, dev, None)

    seed = C.c_uint64(7)
    obs = hd(*([1.0] * 18))                                     # [1][6][3]
    q, lo, up, tg = hd(0.5), hd(0.0), hd(1.0), hi(-2)
    series, pv, pr = hi(0), hi(0), hi(0)
    m_dim, m_const = hi(*([-1] * 6)), hd(*([0.1] * 6))
    out = []

    def add(entry, label, args, info_class):
        out.append((entry, label, tuple(args), info_class))

    def gof(entry, label, **kw):
        add(entry, label, head(**kw) + (dev, dev, obs, dev), abi.GofInfo)
    gof('simplyp_gof', 'E = 0', E=0)
    gof('simplyp_gof', 'out_mask = 0', mask=0)
    gof('simplyp_gof_spearman', 'D = 0', D=0)
    gof('simplyp_gof_spearman', 'S = 0', S=0)
    add('simplyp_gof_waterbody', 'E = 0', (h, dims(E=0), abi.WB_MASK_ALL, dev, None, dev, obs, dev), abi.GofInfo)
    add('simplyp_gof_waterbody', 'wb_mask = 0', (h, dims(), 0, dev, None, dev, obs, dev), abi.GofInfo)

    def waterbody(label, n_sum=1, wb_mask=1, **kw):
        add('simplyp_waterbody', label, head(**kw) + (dev, dev, hi(0), n_sum, wb_mask, dev), abi.WbInfo)
    waterbody('n_sum = 0', n_sum=0)
    waterbody('n_sum = 17', n_sum=17)
    waterbody('wb_mask = 0', wb_mask=0)
    waterbody('E = 0', E=0)

    def quantiles(label, E=4, n_rows=2, K=1):
        add('simplyp_quantiles', label, (h, E, n_rows, dev, None, None, q, K, dev), abi.QuantileInfo)
    quantiles('E = 0', E=0)
    quantiles('n_rows = -1', n_rows=-1)
    quantiles('K = 0', K=0)
    quantiles('K = 17', K=17)

    def weighted(label, E=4, n_rows=2, K=1):
        add('simplyp_weighted_quantiles', label, (h, E, n_rows, dev, None, None, dev, q, K, dev), abi.WqInfo)
    weighted('E = 0', E=0)
    weighted('n_rows = -1', n_rows=-1)
    weighted('K = 17', K=17)

    def time_quantiles(label, n_series=1, n_periods=0, K=1, **kw):
        add('simplyp_time_quantiles', label, head(**kw) + (None, None, series, n_series, None, n_periods, q, K, dev, None), abi.TqInfo)
    time_quantiles('E = 0', E=0)
    time_quantiles('K = 0', K=0)
    time_quantiles('n_series = 0', n_series=0)
    time_quantiles('n_periods = -1', n_periods=-1)

    def pred_tail(day0=0, n_series=1):
        return (None, None, series, n_series, None, seed, day0)
    add('simplyp_predictive_series', 'which = 2', head() + pred_tail() + (2, dev), None)
    add('simplyp_predictive_series', 'day0 = -1', head() + pred_tail(day0=-1) + (0, dev), None)
    add('simplyp_predictive_series', 'E = 0', head(E=0) + pred_tail() + (0, dev), None)

    def bands(label, K=1, day0=0, **kw):
        add('simplyp_predictive_bands', label, head(**kw) + (None,) + pred_tail(day0=day0) + (q, K, dev), abi.PredInfo)
        add('simplyp_predictive_bands_weighted', label, head(**kw) + (None,) + pred_tail(day0=day0) + (q, K, dev, dev), abi.WqInfo)
    bands('K = 0', K=0)
    bands('K = 17', K=17)
    bands('day0 = -1', day0=-1)
    bands('S = 0', S=0)

    def scores(label, E=4, n_rows=2):
        add('simplyp_scores', label, (h, E, n_rows, dev, None, None, None, hd(1.0, 2.0), dev, dev), abi.ScoreInfo)
    scores('E = 0', E=0)
    scores('n_rows = -1', n_rows=-1)
    add('simplyp_predictive_scores', 'day0 = -1', head() + (None,) + pred_tail(day0=-1) + (None, obs, dev, dev), abi.ScoreInfo)
    add('simplyp_predictive_scores', 'n_series = 0', head() + (None,) + pred_tail(n_series=0) + (None, obs, dev, dev), abi.ScoreInfo)
    add('simplyp_predictive_scores', 'E = 0', head(E=0) + (None,) + pred_tail() + (None, obs, dev, dev), abi.ScoreInfo)

    def pareto(label, E=4, M=2, max_fronts=0):
        add('simplyp_pareto', label, (h, E, M, dev, hi(*([1] * 9)), None, None, max_fronts, dev, dev, dev), abi.ParetoInfo)
    pareto('E = 0', E=0)
    pareto('M = 0', M=0)
    pareto('M = 9', M=9)
    pareto('max_fronts = -1', max_fronts=-1)

    def move(W=4, n_dim=1, half=0, a=2.0):
        return (h, W, n_dim, half, a, seed, C.c_uint32(1))

    def propose(label, **kw):
        add('simplyp_mcmc_propose', label, move(**kw) + (lo, up, tg, dev, dev, dev, None, None), abi.McmcInfo)

    def accept(label, **kw):
        add('simplyp_mcmc_accept', label, move(**kw) + (dev, dev, dev, dev, dev, dev, None), abi.McmcInfo)
    for f in (propose, accept):
        f('n_dim = 0', n_dim=0)
        f('n_dim = 17', n_dim=17)
        f('W = 3', W=3)
        f('half = 2', half=2)
        f('a = 1', a=1.0)

    def log_prob(label, W=4, n_dim=1, R=1, n_pairs=1):
        add('simplyp_mcmc_log_prob', label, (h, W, n_dim, R, dev, None, None, pv, pr, n_pairs, m_dim, m_const, dev, dev), abi.McmcInfo)
    log_prob('n_dim = 0', n_dim=0)
    log_prob('n_out_reaches = 0', R=0)
    log_prob('n_pairs = 0', n_pairs=0)
    log_prob('n_pairs = 33', n_pairs=33)

    def nm_propose(label, S=2, n_dim=1):
        add('simplyp_nm_propose', label, (h, S, n_dim, lo, up, tg, dev, dev, dev, dev, None, None), abi.NmInfo)
    nm_propose('S = 0', S=0)
    nm_propose('n_dim = 0', n_dim=0)

    def nm_update(label, S=2, n_dim=1, max_iter=10, xatol=1e-4, fatol=1e-4, history_rows=0):
        add('simplyp_nm_update', label, (h, S, n_dim, max_iter, xatol, fatol, dev, dev, dev, dev, dev, dev, None, history_rows), abi.NmInfo)
    nm_update('S = 0', S=0)
    nm_update('max_iter = 0', max_iter=0)
    nm_update('xatol = -1', xatol=-1.0)
    nm_update('history_rows = -1', history_rows=-1)

    def design(label, N=4, n_dim=1):
        add('simplyp_sobol_design', label, (h, N, n_dim, seed, lo, up, tg, None, dev, None, None), abi.SobolInfo)
    design('N = 1', N=1)
    design('N = 32769', N=32769)
    design('n_dim = 0', n_dim=0)

    def indices(label, N=4, n_dim=1, n_rows=2, n_boot=0):
        add('simplyp_sobol_indices', label, (h, N, n_dim, n_rows, dev, None, n_boot, seed, None, None, dev), abi.SobolInfo)
    indices('N = 1', N=1)
    indices('n_dim = 17', n_dim=17)
    indices('n_rows = -1', n_rows=-1)
    indices('n_boot = -1', n_boot=-1)
    # the one refusal that comes after the entry has written its info: cleared, n_resamples = 1 + n_boot
    indices('n_rows (1 + n_boot) = 2^32 - 2', n_rows=2 ** 31 - 1, n_boot=1)

    def loglik(label, n_pairs=1, **kw):
        add('simplyp_pf_loglik', label, head(**kw) + (dev, dev, obs, pv, pr, n_pairs, dev, None, dev, None, 1), abi.PfInfo)
    loglik('E = 0', E=0)
    loglik('n_pairs = 0', n_pairs=0)
    loglik('n_pairs = 33', n_pairs=33)
    big = 2 ** abi.PF_MAX_LOG2_E + 1
    for E, label in ((0, 'E = 0'), (big, 'E = 2^22 + 1')):
        add('simplyp_pf_weights', label, (h, E, dev, dev, dev), abi.PfInfo)
        add('simplyp_pf_resample', label, (h, E, dev, seed, C.c_uint32(1), dev, None), abi.PfInfo)
        add('simplyp_gather_members', label, (h, E, 1, dev, dev, dev + 16384), abi.PfInfo)
        add('simplyp_pf_jitter', label, (h, E, 1, seed, C.c_uint32(1), 0.5, hd(0.5), hd(0.1), lo, up, tg, dev, None, None), abi.PfInfo)
    add('simplyp_gather_members', 'n_rows = -1', (h, 4, -1, dev, dev, dev + 16384), abi.PfInfo)
    for n_dim in (0, 17):
        add('simplyp_pf_jitter', 'n_dim = %d' % n_dim, (h, 4, n_dim, seed, C.c_uint32(1), 0.5, hd(0.5), hd(0.1), lo, up, tg, dev, None, None), abi.PfInfo)
    add('simplyp_pf_jitter', 'a = inf', (h, 4, 1, seed, C.c_uint32(1), float('inf'), hd(0.5), hd(0.1), lo, up, tg, dev, None, None), abi.PfInfo)
    add('simplyp_eval_units', 'which = 8', (h, 8, 1, dev, dev), None)
    add('simplyp_eval_units', 'n = -1', (h, 0, -1, dev, dev), None)

    def order(label, E=4, cost=dev, where=0, perm=dev, keys=None):
        add('simplyp_order_members', label, (h, E, cost, where, perm, None, keys), None)
    order('E = 0', E=0)
    order('cost = NULL', cost=None)
    order('perm = NULL', perm=None)
    order('where = 2', where=2)
    order('where = 0, E = 196609', E=196609)
    order('where = 1 with keys', where=1, keys=dev)
    out.append(keep)
    return out


def replay(L, h, dev):
    """Every case called once: [{entry, case, rc, error, info}] -- info: the hex bytes of the struct after the call, or None."""
    todo = cases(h, dev)
    todo.pop()                                          # (the host arrays, alive until this function returns)
    got = []
    for entry, label, args, info_class in todo:
        info = None
        if info_class is not None:
            info = info_class()
            C.memset(C.byref(info), SENTINEL, C.sizeof(info))
            args = args + (C.byref(info),)
        rc = getattr(L, entry)(*args)
        got.append(dict(entry=entry, case=label, rc=int(rc), error=L.simplyp_last_error(h).decode(),
                        info=None if info is None else bytes(info).hex()))
    return got


def main(path=OUT):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from simplyp_amd import engine
    eng = engine.get_engine(0)
    scratch = torch.zeros(4096, dtype=torch.float64, device=eng.tdev)
    torch.cuda.synchronize()
    got = replay(engine.lib(), eng._h, scratch.data_ptr())
    assert all(g['rc'] != 0 for g in got), [g for g in got if g['rc'] == 0]
    with open(path, 'w') as fh:
        json.dump(got, fh, indent=1)
        fh.write('\n')
    print('%d cases over %d entries -> %s' % (len(got), len({g['entry'] for g in got}), path))


if __name__ == '__main__':
    main(*sys.argv[1:2])
