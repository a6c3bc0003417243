"""Global sensitivity analysis on the device: which parameters matter for which output.

``sobol_indices`` answers the question the reference's paper asks of parameter-rich catchment models with variance-based
(Sobol') indices: Saltelli's design of ``n_base (n_dim + 2)`` parameter sets is one ensemble run, and the first-order and
total-order indices of every reduced output, with bootstrap percentile intervals, are one contraction on the device
(``simplyp_amd.sobol`` is the NumPy statement of the estimator).  The names, the box and the host checks are the calibration
calls' (``simplyp_amd.priors``)."""

import time

import numpy as np

from . import abi, engine, marshal, priors as _priors, request, sobol, visualise_results as vr
from .model import _DeviceEnsemble, _engine_opts


def _plan(priors, n_base, columns, reduce, obs_dict, n_boot, conf, seed, unit_samples, index):
    """Everything the call can check without the device; raises ValueError."""
    if not isinstance(priors, dict) or not priors:
        raise ValueError("priors must be a dict name -> (lo, hi) with at least one entry")
    names = list(priors)
    target = [_priors.target_of(nm) for nm in names]
    unknown = [nm for nm, t in zip(names, target) if t is None]
    if unknown:
        raise ValueError("unknown parameter %r: the names are %s and 'f_TDP'" % (unknown[0], marshal.PM_NAMES))
    if 'f_TDP' in names and not obs_dict:
        raise ValueError("'f_TDP' without obs_dict: no selected output depends on it")
    lo, hi = _priors.box(priors, names)
    try:
        sobol.check_shape(int(n_base), len(names))
    except ValueError as exc:
        raise ValueError("sobol_indices: %s" % exc)
    N = int(n_base)
    if not 0.0 < float(conf) < 1.0:
        raise ValueError("conf must lie in (0, 1) (got %r)" % (conf,))
    n_boot, seed = int(n_boot), int(seed)
    if not 0 <= n_boot <= 1 << 20 or not 0 <= seed < 1 << 64:
        raise ValueError("n_boot must be in [0, 2^20] and seed in [0, 2^64)")
    unit = None if unit_samples is None else sobol.check_unit(unit_samples, N, len(names))
    columns = [columns] if isinstance(columns, str) else list(columns)
    bad = [c for c in columns if c not in marshal.OUT_COLUMNS]
    if bad or not columns or len(set(columns)) != len(columns):
        raise ValueError("columns must be distinct names among the reference's columns (got %s)" % columns)
    period = request.reduce_periods(reduce, index, total=True)[1]
    return names, np.array(target, dtype=np.int32), lo, hi, N, n_boot, seed, unit, columns, period


def _intervals(eng, ind_d, n_boot, conf):
    """The percentile interval over the bootstrap axis, selected on the device: ``[2] + ind.shape[:-1]`` (NaN without resamples)."""
    shape = tuple(int(v) for v in ind_d.shape[:-1])
    if n_boot < 1:
        return np.full((2,) + shape, np.nan), 0.0
    q = [(1.0 - conf) / 2.0, (1.0 + conf) / 2.0]
    lower, upper, info = eng.quantiles(ind_d[..., 1:].contiguous(), q)
    return engine.interpolate_quantiles(lower.cpu().numpy(), upper.cpu().numpy(), q, info['n_used']), info['kernel_ms']


def _result(eng, ind_d, sums_d, n_used_d, n_boot, conf):
    """The host's view of one ``Engine.sobol_indices`` call: S1, ST, their intervals and the variance, ``[n_dim] + rows``."""
    ind = ind_d.cpu().numpy()
    conf_int, q_ms = _intervals(eng, ind_d, n_boot, conf)
    s0, n0 = sums_d[0].cpu().numpy(), np.float64(int(n_used_d[0]))
    with np.errstate(all='ignore'):
        m1, m2 = s0[..., 0] / (2.0 * n0), s0[..., 1] / (2.0 * n0)
        var = m2 - m1 * m1
    return dict(S1=np.ascontiguousarray(ind[0, ..., 0]), ST=np.ascontiguousarray(ind[1, ..., 0]),
                S1_conf=np.ascontiguousarray(conf_int[:, 0]), ST_conf=np.ascontiguousarray(conf_int[:, 1]), var=var), q_ms


def sobol_indices(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, priors, n_base, columns=('Qr',), reduce='annual',
                  obs_dict=None, n_boot=1000, conf=0.95, seed=0, unit_samples=None, out_reaches=None, step_len=1., solver=None,
                  device=0, keep_table=False):
    """First-order and total-order Sobol' indices of reduced model outputs with respect to model parameters, with bootstrap
    percentile intervals (Saltelli et al. 2010, as ``scipy.stats.sobol_indices`` and its ``bootstrap``).

    ``priors``: dict name -> (lo, hi), the box the parameters are uniform in; names are member parameters
    (``marshal.PM_NAMES``) and ``'f_TDP'`` (which only the goodness of fit depends on: it needs ``obs_dict``); at most 16.
    ``n_base``: base samples N in [2, 32768]; the ensemble has ``N (n_dim + 2)`` members.  ``columns``: the reference's output
    columns; ``reduce``: ``'annual'`` = the sum of every calendar year, ``'total'`` = the sum of the whole run, or an int array
    of period indices per day -- the outputs are the period sums ``[n_cols, P, R]``.  ``obs_dict``: with observations, the
    goodness-of-fit statistics of a daily run of the same design are a second set of outputs (``'gof'``).  ``n_boot`` bootstrap
    resamples give the ``conf`` percentile interval; ``seed`` keys the counter-based streams of the design and the bootstrap
    (``simplyp_amd.sobol``); ``unit_samples``: the caller's ``[2, n_dim, n_base]`` unit points in [0, 1) -- a scrambled
    ``scipy.stats.qmc.Sobol``, say -- instead of the design's own stream.

    The inputs are marshalled and uploaded once: ``Engine.sobol_design`` writes the design into the run's arrays,
    ``Engine.run`` reduces to period sums, ``Engine.sobol_indices`` computes the indices of every (column, period, reach) and
    ``Engine.quantiles`` selects the interval on the bootstrap axis.  A sample with a member whose run went non-finite takes
    part in nothing.  A constant output has NaN indices (scipy reports 0).

    Returns dict(names, columns, reaches, S1, ST ``[n_dim, n_cols, P, R]``, S1_conf, ST_conf ``[2, n_dim, n_cols, P, R]``,
    var ``[n_cols, P, R]``, n_valid, x ``[n_dim, E]`` -- the design --, status ``[E]``, table ``[n_cols, P, R, E]`` -- the period sums
    the indices were taken of, with ``keep_table`` --, gof -- with ``obs_dict``: dict(stats,
    variables, S1, ST ``[n_dim, n_stats, 6, R]``, S1_conf, ST_conf, var, n_valid) --, stats = dict(run_kernel_ms, design_ms,
    counts_ms, contract_ms, quantile_ms, wall_ms)).  ``ValueError`` before any device call for an unknown name, ``lo >= hi``,
    ``n_base`` out of range, ``conf`` outside (0, 1), a ``unit_samples`` of the wrong shape or outside [0, 1), ``'f_TDP'``
    without ``obs_dict``.  The caller's ``p_LU`` / ``p_SC`` are edited in place exactly as by ``run_simply_p``."""
    names, target, lo, hi, N, n_boot, seed, unit, columns, period = _plan(priors, n_base, columns, reduce, obs_dict, n_boot, conf,
                                                                            seed, unit_samples, met_df.index)
    n_dim = len(names)
    E = N * (n_dim + 2)
    with marshal.reference_edits(p_SU, p_LU, p_SC, p):
        scs, up_ptr, up_idx, reaches, oreach = marshal.catchment(p_struc, p, out_reaches)
        _priors.check_corners(names, lo, hi, p, p_LU, p_SC, scs)
        snow = _priors.snow_rule(names, met_df)
        obs = vr.observation_array(obs_dict, reaches, met_df.index) if obs_dict else None

        # ---- the device: everything is marshalled and uploaded once
        w0 = time.perf_counter()
        dev = _DeviceEnsemble("sobol_indices keeps members in design order", met_df, p_SU, p_LU, p_SC, p, dynamic_options, step_len,
                              solver, device, E, columns, snow, n_periods=int(period.max()) + 1)
        eng = dev.eng
        run = lambda opts, **kw: eng.run(dev.f_d, dev.doy_d, dev.mp_d, dev.rp_d, up_ptr, up_idx, opts, out_reaches=oreach, **kw)
        x_d, dinfo = eng.sobol_design(N, lo, hi, target, dev.mp_d, dev.ft_d, seed=seed, unit=unit)
        out_d, status_d, rstats = run(dev.opts, period_of_day=period)
        ind_d, sums_d, n_used_d, sinfo = eng.sobol_indices(out_d, N, n_dim, status=status_d, n_boot=n_boot, seed=seed)
        res, q_ms = _result(eng, ind_d, sums_d, n_used_d, n_boot, conf)
        order = [marshal.columns_of_mask(dev.mask).index(c) for c in columns]      # the table's columns are in mask order
        for k in ('S1', 'ST'):
            res[k] = np.ascontiguousarray(res[k][:, order])
        for k in ('S1_conf', 'ST_conf'):
            res[k] = np.ascontiguousarray(res[k][:, :, order])
        res['var'] = np.ascontiguousarray(res['var'][order])
        stats = dict(run_kernel_ms=rstats['kernel_ms'], design_ms=dinfo['kernel_ms'], counts_ms=sinfo['counts_ms'],
                     contract_ms=sinfo['contract_ms'], quantile_ms=q_ms)
        res.update(names=names, columns=columns, reaches=reaches, n_valid=sinfo['n_valid'], x=x_d.cpu().numpy(),
                   status=status_d.cpu().numpy())
        if keep_table:
            res['table'] = np.ascontiguousarray(out_d.cpu().numpy()[order])
        if obs is not None:
            del out_d
            gmask = marshal.mask_of_columns(marshal.FLUX_COLUMNS)                  # what simplyp_gof reads
            daily_d, gstatus_d, gstats = run(_engine_opts(p_SU, p, dynamic_options, step_len, solver, gmask, snow=snow))
            gof_d, _ = eng.gof(daily_d, gmask, obs, dev.ft_d, dev.rp_d, out_reaches=oreach)
            del daily_d
            gi_d, gs_d, gn_d, ginfo = eng.sobol_indices(gof_d, N, n_dim, status=gstatus_d, n_boot=n_boot, seed=seed)
            gres, gq_ms = _result(eng, gi_d, gs_d, gn_d, n_boot, conf)
            gres.update(stats=list(abi.GOF_STATS), variables=list(abi.GOF_VARS), n_valid=ginfo['n_valid'])
            res['gof'] = gres
            stats['run_kernel_ms'] += gstats['kernel_ms']
            stats['counts_ms'] += ginfo['counts_ms']
            stats['contract_ms'] += ginfo['contract_ms']
            stats['quantile_ms'] += gq_ms
    stats['wall_ms'] = 1e3 * (time.perf_counter() - w0)
    res['stats'] = stats
    return res
