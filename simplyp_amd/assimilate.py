"""Assimilating observations as they arrive: a particle filter (sequential importance resampling) over the joint (state,
parameter) space, every step of it on the device.

``find_map``, ``sample_posterior`` and ``sobol_indices`` answer questions about a closed calibration period.  A catchment model
in operation faces the other one: new discharge and chemistry samples arrive every few weeks, and the parameter distribution,
the model state and a forecast band are wanted each time without running thirty years again.  ``assimilate`` walks the record
window by window; ``simplyp_amd.particle`` states its steps in NumPy and Python integers."""

import time

import numpy as np
import pandas as pd

from . import abi, marshal, particle
from .calibrate import _plan, _host_setup, _check_inside, _shaped_for_the_ensemble

FLUX = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']            # what the likelihood and the df_R series read
STEPS = ('run', 'loglik', 'weights', 'resample', 'gather', 'jitter')


def _rejuvenation(rejuvenate, delta, names, lo, hi):
    """('liu_west', a) | ('fixed', scale [n_dim]) | None; raises ValueError."""
    if rejuvenate is None:
        return None
    if isinstance(rejuvenate, str):
        if rejuvenate != 'liu_west':
            raise ValueError("rejuvenate must be 'liu_west', a fraction of the box width, a dict name -> fraction, or None")
        if not 1.0 / 3.0 < float(delta) <= 1.0:
            raise ValueError("delta must lie in (1/3, 1] (Liu & West recommend 0.95 to 0.99; got %r)" % (delta,))
        return 'liu_west', (3.0 * float(delta) - 1.0) / (2.0 * float(delta))
    if isinstance(rejuvenate, dict):
        unknown = [nm for nm in rejuvenate if nm not in names]
        if unknown:
            raise ValueError("rejuvenate names parameters that priors does not: %s" % unknown)
        frac = np.array([float(rejuvenate.get(nm, 0.0)) for nm in names])
    else:
        try:
            frac = np.full(len(names), float(rejuvenate))
        except (TypeError, ValueError):
            raise ValueError("rejuvenate must be 'liu_west', a fraction of the box width, a dict name -> fraction, or None")
    if not (np.isfinite(frac).all() and (frac >= 0).all()):
        raise ValueError("a jitter fraction must be finite and >= 0")
    return 'fixed', frac * (hi - lo)


def assimilate(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, obs_dict, priors, variables=('Q',), error_m=None,
               n_particles=None, window=30, start=None, initial_state=None, seed=0, resample_threshold=1.0, rejuvenate='liu_west',
               delta=0.98, quantiles=None, forecast_series=None, record=False, state=None, step_len=1., solver=None, device=0,
               out_reaches=None, forecast_weighted=False, score=False):
    """Update the parameter distribution and the model state of ``n_particles`` particles window by window as the observations
    of ``obs_dict`` arrive (sequential importance resampling), every step on the device.

    ``priors``, ``variables``, ``error_m``, ``out_reaches`` and their checks are ``sample_posterior``'s: names are member
    parameters, ``'f_TDP'`` and ``'m_<VAR>'`` -- which makes the error model's ``m`` a filtered dimension --, the box is
    ``lo <= x < hi``, and a selected variable needs more than 10 observations over the whole period at some output reach (a
    single window needs none).  ``window``: as ``ensemble.window_bounds`` takes it (days per window, ``'annual'``, or start dates).
    ``start``: None = uniform in the box (``particle.uniform_start``), or an array [n_dim, n_particles] inside it, for example
    ``sample_posterior(...)['state']['theta']``: the hand-over from calibration to operation.  ``initial_state``: as in
    ``run_simply_p_ensemble`` (None: the cold initial conditions).  ``seed``: the key of the counter-based random streams.

    One window ``t``: ``Engine.run`` over its days from the particles' state, parameters and ``f_tdp`` on the device, state in
    and state out -> ``pf_loglik`` adds the window's log-likelihood to the log weights -> ``pf_weights`` gives the effective
    sample size and the evidence increment (the log of the mean weight after the window minus the one before it, which is 0
    right after a resampling) -> if ``ESS < resample_threshold * n_particles``: ``pf_resample``, ``gather_members`` for the state,
    ``member_params``, ``reach_params``, ``f_tdp`` and the positions, the log weights back to 0, and the rejuvenation move
    ``pf_jitter``.  ``rejuvenate='liu_west'``: shrink towards the mean by ``a = (3 delta - 1) / (2 delta)`` and add
    ``sqrt(1 - a^2)`` standard deviations of noise per dimension (Liu & West 2001: mean and variance are kept; mean and standard
    deviation of the resampled positions are taken with torch on the device); a float or a dict name -> float: plain jitter of
    that fraction of the box width; None: no move -- degenerate for this deterministic model, whose duplicates then stay
    identical for ever.  ``delta`` is a user's knob inside Liu & West's recommended 0.95 to 0.99, not a tolerance.

    ``quantiles``: per-window forecast bands of ``forecast_series`` (``df_R`` names or columns among %s; default: the series of
    ``variables``) through ``Engine.predictive_bands``, taken BEFORE the window's weighting: the parameter-only band, and the
    overall band of the series whose ``m`` the filter knows.  The bands are unweighted, so they are right only when the
    particles entering every window are equally weighted: ``quantiles`` with ``resample_threshold < 1`` is a ``ValueError``
    unless ``forecast_weighted=True``.  Then a window's bands are weighted by the particles' integer weights as they ENTER the
    window -- the ``q`` of the previous ``pf_weights`` call, all equal at the start and right after a resampling --, selected by
    ``Engine.predictive_bands(weights=)`` under numpy's ``method='inverted_cdf'`` rule (``simplyp_amd.weighted``; not the
    ``'linear'`` rule of the unweighted bands); any ``resample_threshold`` is allowed and ``forecast['rule']`` is
    ``'inverted_cdf'``.
    ``devices=[...]`` is not offered: resampling spans the whole ensemble.

    ``score=True``: every window's observations are scored against the forecast BEFORE that window's weighting, where the forecast
    bands are taken (``Engine.predictive_scores``; ``simplyp_amd.score`` states the rule): CRPS in its two terms and the PIT
    counts of every observed (series, day, reach), for each ``df_R`` series that has an observation at some output reach.  They
    are always taken under the integer weights with which the particles ENTER the window -- all equal at the start and right
    after a resampling --, so any ``resample_threshold`` is allowed; ``overall`` draws the error model with the ``m`` the filter
    knows (0 for the other series; None when it knows the ``m`` of no scored series, as the ensemble call without
    ``predictive_m``).  ``['scores']`` has the shape of ``run_simply_p_ensemble(score=True)``'s over all days of the
    call, with ``weight_total`` and ``n_members`` one entry per window, and ``kernel_ms`` gains ``'score'``.

    ``state``: the ``'state'`` of an earlier result; ``met_df`` then covers the dates that follow, and the filter continues bit
    for bit (``start``, ``initial_state`` and ``seed`` are ignored).

    Returns dict(names, windows -- (first day, last day, lo, hi) each --, ess, log_evidence, resampled, n_unique, n_outside
    (one entry per window), log_evidence_total, kernel_ms -- dict step -> per-window list for %s --, pilot_ms, wall_ms,
    theta [n_dim, E], log_weights [E], overrides, error_m -- shaped for ``run_simply_p_ensemble`` as ``sample_posterior``'s --,
    state -- the model state dict ``run_simply_p_ensemble(initial_state=)`` takes, plus theta, lw, t, seed, day: the filter's
    continuation --, forecast -- dict(q, series, param_only [K, n_series, D, R], overall_series, overall, day0) with
    ``quantiles`` --, and with ``record`` the per-window lists inc, q, ancestors, theta_before, theta_after, state_in,
    state_out).  ``ValueError`` before any device call for bad arguments; ``RuntimeError`` naming the window when every particle is
    dead there.  The caller's ``p_LU`` / ``p_SC`` are edited in place exactly as by ``run_simply_p``."""
    from . import ensemble, engine
    from .model import _engine_opts, _state_blocks

    if not obs_dict:
        raise ValueError("assimilate needs obs_dict: the observations that arrive")
    E = int(np.asarray(state['theta']).shape[1]) if state is not None else n_particles

    def check_shape(n_dim):
        if E is None:
            raise ValueError("n_particles must be given")
        try:
            particle.check_shape(int(E), n_dim)
        except ValueError as exc:
            raise ValueError("assimilate: %s" % exc)

    names, variables, lo, hi, target, m_dim, m_const = _plan(priors, variables, error_m, check_shape)
    n_dim, E = len(names), int(E)
    seed = int(state['seed']) if state is not None else int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in [0, 2^64)")
    if not float(resample_threshold) >= 0.0:
        raise ValueError("resample_threshold must be >= 0 (got %r)" % (resample_threshold,))
    move = _rejuvenation(rejuvenate, delta, names, lo, hi)
    known_m = [abi.TQ_DERIVED_SERIES[abi.GOF_VARS.index(v)] for v in variables]
    fc_names = fc_ids = None
    if quantiles is not None:
        if float(resample_threshold) < 1.0 and not forecast_weighted:
            raise ValueError("quantiles needs resample_threshold >= 1: the forecast bands are unweighted, which is right only for "
                             "equally weighted particles (or pass forecast_weighted=True for bands under the particles' weights)")
        quantiles = [float(x) for x in np.atleast_1d(quantiles)]
        if not 1 <= len(quantiles) <= 16 or not all(0.0 <= x <= 1.0 for x in quantiles):
            raise ValueError("quantiles must be 1 to 16 probabilities in [0, 1]")
        fc_names = list(known_m) if forecast_series is None else ([forecast_series] if isinstance(forecast_series, str) else list(forecast_series))
        unknown = [c for c in fc_names if c not in abi.TQ_DERIVED_SERIES and c not in FLUX]
        if unknown or not 1 <= len(fc_names) <= 32:
            raise ValueError("forecast_series must be 1 to 32 names among %s and %s (unknown: %s)" % (abi.TQ_DERIVED_SERIES, FLUX, unknown))
        fc_ids = [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index(c) if c in abi.TQ_DERIVED_SERIES else marshal.ALL_COLUMNS.index(c)
                  for c in fc_names]
    elif forecast_series is not None:
        raise ValueError("forecast_series needs quantiles: the probabilities of the bands")
    bounds = ensemble.window_bounds(met_df.index, window)

    hs = _host_setup(met_df, p_struc, p_SU, p_LU, p_SC, p, obs_dict, names, variables, lo, hi, out_reaches)
    try:
        scs, S = hs['scs'], len(hs['scs'])
        sc_names = sc_ids = sc_obs = None
        if score:                                                      # the df_R series with an observation, on any date, at some output reach
            seen = {var for SC in hs['reaches'] if SC in obs_dict for var in abi.GOF_VARS
                    if var in obs_dict[SC].columns and obs_dict[SC][var].notna().any()}
            sc_names = [c for c, var in zip(abi.TQ_DERIVED_SERIES, abi.GOF_VARS) if var in seen]
            sc_ids = [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index(c) for c in sc_names]
            sc_obs = np.ascontiguousarray(np.stack([hs['obs'][:, abi.TQ_DERIVED_SERIES.index(c), :].T for c in sc_names])) \
                if sc_names else None
        if state is not None:
            theta0, lw0 = np.array(state['theta'], dtype=np.float64), np.array(state['lw'], dtype=np.float64)
            t0, day0 = int(state['t']), int(state['day'])
            if theta0.shape != (n_dim, E) or lw0.shape != (E,) or t0 < 0 or day0 < 0:
                raise ValueError("state does not match this call: theta %s for %d names" % (theta0.shape, n_dim))
            st_in = _state_blocks({k: state[k] for k in ('rows', 'reaches', 'data', 'end') if k in state}, scs, E, met_df.index, [(0, E)])[0]
        else:
            t0, day0, lw0 = 0, 0, np.zeros(E)
            theta0 = particle.uniform_start(seed, n_dim, E, lo, hi) if start is None else np.array(start, dtype=np.float64)
            if theta0.shape != (n_dim, E):
                raise ValueError("start must have shape [n_dim, n_particles] = %s, got %s" % ((n_dim, E), theta0.shape))
            st_in = None if initial_state is None else _state_blocks(initial_state, scs, E, met_df.index, [(0, E)])[0]
        _check_inside(theta0, lo, hi, names)
        if t0 + len(bounds) >= 1 << 32 or day0 + len(met_df) >= 1 << 31:
            raise ValueError("the absolute window index must stay below 2^32 and the absolute day below 2^31")
        mask = marshal.mask_of_columns(FLUX)
        opts = _engine_opts(p_SU, p, dynamic_options, step_len, solver, mask, snow=hs['snow'])
        if opts.out_slot_order:
            raise ValueError("assimilate keeps members in particle order: solver['out_slot_order'] must stay 0")
    except ValueError:
        marshal.epilogue_mutations(p_SU, p_LU, p_SC, p)
        raise

    # ---- the device: everything is marshalled and uploaded once; from here on only info structs come back per window
    eng = engine.get_engine(device)
    torch = eng.torch
    f64 = dict(dtype=torch.float64, device=eng.tdev)
    forcing, doy = marshal.forcing_arrays(met_df, snow=hs['snow'])
    f_d, doy_d = eng.to_device(forcing, torch.float64), eng.to_device(doy, torch.int32)
    mp_d = eng.to_device(marshal.member_params(p, p_LU, E), torch.float64)
    rp_d = eng.to_device(marshal.reach_params(p_SC, p, E), torch.float64)
    ft_d = torch.full((E,), float(p['f_TDP']), **f64)
    theta_d, lw_d, inc_d = eng.to_device(theta0, torch.float64), eng.to_device(lw0, torch.float64), torch.empty((E,), **f64)
    for d in range(n_dim):                                             # the positions into the run's arrays
        if target[d] >= 0:
            mp_d[int(target[d])].copy_(theta_d[d])
        elif target[d] == abi.MCMC_TARGET_F_TDP:
            ft_d.copy_(theta_d[d])
    state_d = None if st_in is None else eng.to_device(st_in, torch.float64).clone()
    pairs = hs['pairs']

    def m_rows(series_vars):
        """The error model's m [n, E] of the variables ``series_vars`` (indices of abi.GOF_VARS), from the positions."""
        return torch.stack([theta_d[m_dim[v]] if m_dim[v] >= 0 else torch.full((E,), m_const[v], **f64) for v in series_vars]).contiguous()

    out = dict(ess=[], log_evidence=[], resampled=[], n_unique=[], n_outside=[])
    kms = {k: [] for k in STEPS + (('score',) if score else ())}
    sc_parts = []
    pilot_ms, wall_ms = [], []
    rec = {k: [] for k in ('inc', 'q', 'ancestors', 'theta_before', 'theta_after', 'state_in', 'state_out')}
    bands_po, bands_ov = [], []
    ov_at = [i for i, c in enumerate(fc_names or []) if c in known_m]
    host = lambda x: None if x is None else x.cpu().numpy()
    w_d, q_d, info = eng.pf_weights(lw_d)
    lm_prev = particle.log_mean(info['lw_max'], info['sum_w'], E)
    try:
        for n, (d_lo, d_hi) in enumerate(bounds):
            t = t0 + n
            torch.cuda.synchronize(eng.tdev)
            w0 = time.perf_counter()
            if record:
                rec['theta_before'].append(host(theta_d))
                rec['state_in'].append(host(state_d))
            table_d, status_d, rstats = eng.run(f_d[:, :, d_lo:d_hi].contiguous(), doy_d[d_lo:d_hi].contiguous(), mp_d, rp_d, hs['up_ptr'],
                                                hs['up_idx'], opts, out_reaches=hs['oreach'], state_in=state_d, state_out=True)
            state_d = rstats['state']
            kms['run'].append(rstats['kernel_ms'])
            pilot_ms.append(rstats['pilot_ms'])
            tkw = dict(f_tdp=ft_d, reach_params=rp_d, out_reaches=hs['oreach'])
            if quantiles is not None:                                  # before the weighting
                pkw = dict(seed=seed, day0=day0 + d_lo, **tkw)

                def forecast_band(ids, **kw):
                    if forecast_weighted:                              # under the weights the particles enter the window with
                        return host(eng.predictive_bands(table_d, mask, quantiles, ids, weights=q_d, **dict(pkw, **kw))[0])
                    lo_b, up_b, binfo = eng.predictive_bands(table_d, mask, quantiles, ids, **dict(pkw, **kw))
                    return engine.interpolate_quantiles(host(lo_b), host(up_b), quantiles, binfo['n_used'])
                bands_po.append(forecast_band(fc_ids))
                if ov_at:
                    em = m_rows([abi.GOF_VARS.index(variables[known_m.index(fc_names[i])]) for i in ov_at])
                    bands_ov.append(forecast_band([fc_ids[i] for i in ov_at], err_m=em))
            if sc_names:                                               # before the weighting, under the weights of entry
                skw = dict(seed=seed, day0=day0 + d_lo, weights=q_d, include=(status_d & abi.STATUS_NONFINITE) == 0, **tkw)
                sobs = np.ascontiguousarray(sc_obs[:, d_lo:d_hi])
                po_w, ov_w = eng.predictive_scores(table_d, mask, sc_ids, sobs, **skw), None
                if any(c in known_m for c in sc_names):                # the m the filter knows; 0 for the other series
                    zero = torch.zeros((E,), **f64)
                    em_all = torch.stack([m_rows([abi.GOF_VARS.index(variables[known_m.index(c)])])[0] if c in known_m else zero
                                          for c in sc_names])
                    ov_w = eng.predictive_scores(table_d, mask, sc_ids, sobs, err_m=em_all.contiguous(), **skw)
                sc_parts.append((po_w, ov_w))
                kms['score'].append(po_w[2]['kernel_ms'] + (0.0 if ov_w is None else ov_w[2]['kernel_ms']))
            elif score:
                kms['score'].append(0.0)
            linfo = eng.pf_loglik(table_d, mask, hs['obs'][:, :, d_lo:d_hi], pairs, m_rows([v for v, _ in pairs]), lw_d, status=status_d,
                                  inc=inc_d, accumulate=True, **tkw)
            w_d, q_d, winfo = eng.pf_weights(lw_d, w_d, q_d)
            kms['loglik'].append(linfo['kernel_ms'])
            kms['weights'].append(winfo['kernel_ms'])
            if record:
                rec['inc'].append(host(inc_d))
                rec['q'].append(host(q_d).astype(np.uint64))
                rec['state_out'].append(host(state_d))
            if winfo['T'] == 0:
                raise RuntimeError("assimilate: every particle is dead in window %d (%s to %s): no log weight is finite -- the error "
                                   "model's m or the prior box leaves no particle that explains the observations"
                                   % (t, met_df.index[d_lo].date(), met_df.index[d_hi - 1].date()))
            ess = particle.ess(winfo['sum_w'], winfo['sum_w2'])
            lm = particle.log_mean(winfo['lw_max'], winfo['sum_w'], E)
            out['ess'].append(ess)
            out['log_evidence'].append(lm - lm_prev)
            lm_prev = lm
            do = ess < float(resample_threshold) * E
            ms = dict(resample=0.0, gather=0.0, jitter=0.0)
            n_unique, n_outside, anc_h = E, 0, None
            if do:
                anc_d, _, rinfo = eng.pf_resample(q_d, seed, t, offspring=False)
                ms['resample'], n_unique = rinfo['kernel_ms'], rinfo['n_unique']
                moved = []
                for src in (state_d, mp_d, rp_d, ft_d, theta_d):       # everything a particle owns travels with it
                    dst, ginfo = eng.gather_members(src, anc_d)
                    ms['gather'] += ginfo['kernel_ms']
                    moved.append(dst)
                state_d, mp_d, rp_d, ft_d, theta_d = moved
                lw_d.zero_()
                lm_prev = 0.0
                if forecast_weighted or score:                         # the next window's particles enter it equally weighted
                    w_d, q_d, _ = eng.pf_weights(lw_d, w_d, q_d)
                if move is not None:
                    if move[0] == 'liu_west':
                        a = move[1]
                        centre = host(theta_d.mean(dim=1))
                        scale = np.sqrt(1.0 - a * a) * host(theta_d.std(dim=1, unbiased=False))
                    else:
                        a, centre, scale = 1.0, np.zeros(n_dim), move[1]
                    jinfo = eng.pf_jitter(theta_d, t, a, centre, scale, lo, hi, target, mp_d, ft_d, seed=seed)
                    ms['jitter'], n_outside = jinfo['kernel_ms'], jinfo['n_outside']
                anc_h = host(anc_d)
            for k in ('resample', 'gather', 'jitter'):
                kms[k].append(ms[k])
            out['resampled'].append(bool(do))
            out['n_unique'].append(int(n_unique))
            out['n_outside'].append(int(n_outside))
            if record:
                rec['ancestors'].append(np.arange(E, dtype=np.int32) if anc_h is None else anc_h)
                rec['theta_after'].append(host(theta_d))
            torch.cuda.synchronize(eng.tdev)
            wall_ms.append(1e3 * (time.perf_counter() - w0))
    finally:
        marshal.epilogue_mutations(p_SU, p_LU, p_SC, p)

    theta, lw = host(theta_d), host(lw_d)
    overrides, err_m = _shaped_for_the_ensemble(names, target, variables, m_dim, m_const, theta)
    res = {k: np.array(v) for k, v in out.items()}
    res.update(names=names, windows=[(met_df.index[a_], met_df.index[b_ - 1], int(a_), int(b_)) for a_, b_ in bounds],
               log_evidence_total=float(np.sum(res['log_evidence'])), kernel_ms=kms, pilot_ms=pilot_ms, wall_ms=wall_ms,
               theta=theta, log_weights=lw, overrides=overrides, error_m=err_m,
               state=dict(rows=list(abi.STATE_ROWS), reaches=list(scs), data=host(state_d), end=pd.Timestamp(met_df.index[-1]),
                          theta=theta.copy(), lw=lw.copy(), t=t0 + len(bounds), seed=seed, day=day0 + len(met_df)))
    if quantiles is not None:
        res['forecast'] = dict(q=list(quantiles), series=list(fc_names), param_only=np.concatenate(bands_po, axis=2),
                               overall_series=[fc_names[i] for i in ov_at],
                               overall=np.concatenate(bands_ov, axis=2) if ov_at else None, day0=day0)
        if forecast_weighted:
            res['forecast']['rule'] = 'inverted_cdf'
    if score:
        res['scores'] = _joined_scores(sc_names, hs['reaches'], sc_obs, sc_parts, seed, day0)
    if record:
        res.update(rec)
    return res


def _joined_scores(series, reaches, obs, parts, seed, day0):
    """The windows' scores laid end to end along the day axis, in the shape of ``run_simply_p_ensemble(score=True)['scores']``;
    ``weight_total``, ``n_members`` and ``info`` are one entry per window (a window's pit is taken with its own total)."""
    from .model import _scores_result, _mean_crps
    if not series or not parts:
        return _scores_result([], reaches, None, 0 if obs is None else obs.shape[1], None, seed, day0)
    at, wins = 0, []
    for po, ov in parts:
        n = int(po[0].shape[2])
        wins.append(_scores_result(series, reaches, obs[:, at:at + n], n, (po, ov), seed, day0))
        at += n

    def join(key):
        d = {k: np.concatenate([w[key][k] for w in wins], axis=1) for k in ('crps', 'abs_err', 'spread', 'below', 'at_or_below', 'pit')}
        d['n_obs'], d['mean_crps'] = _mean_crps(d['crps'])
        return d
    return dict(series=list(series), reaches=list(reaches), param_only=join('param_only'),
                overall=None if parts[0][1] is None else join('overall'),
                weight_total=[w['weight_total'] for w in wins], n_members=[w['n_members'] for w in wins], seed=seed, day0=day0,
                info=dict(param_only=[w['info']['param_only'] for w in wins], overall=[w['info']['overall'] for w in wins]))


assimilate.__doc__ = assimilate.__doc__ % (FLUX, list(STEPS))
