"""Assimilating observations as they arrive: a particle filter (sequential importance resampling) over the joint (state,
parameter) space, every step of it on the device.

``find_map``, ``sample_posterior`` and ``sobol_indices`` answer questions about a closed calibration period.  A catchment model
in operation faces the other one: new discharge and chemistry samples arrive every few weeks, and the parameter distribution,
the model state and a forecast band are wanted each time without running thirty years again.  ``assimilate`` walks the record
window by window; ``simplyp_amd.particle`` states its steps in NumPy and Python integers."""

import time
from types import SimpleNamespace

import numpy as np
import pandas as pd

from . import abi, engine, ensemble, marshal, particle, request
from . import forcing as forcing_rules
from .calibrate import _plan, _host_setup, _check_inside, _shaped_for_the_ensemble
from .model import _DeviceEnsemble, _state_blocks, _scores_result, _mean_crps

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


def _host(x):
    return None if x is None else x.cpu().numpy()


def _m_rows(dev, s, c, series_vars):
    """The error model's m [n, E] of the variables ``series_vars`` (indices of abi.GOF_VARS; None: a series without one, m = 0)."""
    fixed = lambda v: dev.torch.full((s.theta.shape[1],), 0.0 if v is None else c.m_const[v], **dev.f64)
    return dev.torch.stack([s.theta[c.m_dim[v]] if v is not None and c.m_dim[v] >= 0 else fixed(v) for v in series_vars]).contiguous()


def _window(dev, hs, s, c, t, d_lo, d_hi):
    """Window ``t`` = days [d_lo, d_hi): run, forecast, log-likelihood, weights, and the resampling when the ESS asks for it.
    What it changes: the filter's state ``s`` (theta, lw, inc, state, w, q on the device, lm_prev) and, on resampling, the
    particles' arrays ``dev.mp_d`` / ``rp_d`` / ``ft_d``.  ``c``: the call's settings, read only.  Returns the window's record."""
    eng, torch, mask, E = dev.eng, dev.torch, dev.mask, s.theta.shape[1]
    torch.cuda.synchronize(eng.tdev)
    w0 = time.perf_counter()
    rec = dict(theta_before=_host(s.theta), state_in=_host(s.state)) if c.record else {}
    if c.record and c.noisy:
        rec['forcing_noise_in'] = _host(s.noise)
    table_d, status_d, rstats = eng.run(dev.f_d[:, :, d_lo:d_hi].contiguous(), dev.doy_d[d_lo:d_hi].contiguous(), dev.mp_d, dev.rp_d,
                                        hs['up_ptr'], hs['up_idx'], dev.opts, out_reaches=hs['oreach'], state_in=s.state, state_out=True,
                                        forcing_error=forcing_rules.day_window(c.forcing, d_lo, d_hi),
                                        keep_forcing_table=c.record and c.forcing is not None,
                                        forcing_noise_in=s.noise, forcing_noise_out=True if c.noisy else None)
    s.state, s.noise = rstats['state'], rstats.get('forcing_noise')
    if c.record and c.noisy:
        rec['forcing_noise_out'] = _host(s.noise)
    if 'forcing_table' in rstats:
        rec['forcing_table'] = _host(rstats['forcing_table'])
    ms = dict(dict.fromkeys(STEPS + ('score',), 0.0), run=rstats['kernel_ms'])
    win = dict(ms=ms, pilot_ms=rstats['pilot_ms'], rec=rec, n_unique=E, n_outside=0)
    tkw = dict(f_tdp=dev.ft_d, reach_params=dev.rp_d, out_reaches=hs['oreach'])
    pkw = dict(tkw, seed=c.seed, day0=c.day0 + d_lo)
    if c.quantiles is not None:                                    # before the weighting
        def band(ids, **kw):
            if c.forecast_weighted:                                # under the weights the particles enter the window with
                return _host(eng.predictive_bands(table_d, mask, c.quantiles, ids, weights=s.q, **dict(pkw, **kw))[0])
            lo_b, up_b, binfo = eng.predictive_bands(table_d, mask, c.quantiles, ids, **dict(pkw, **kw))
            return engine.interpolate_quantiles(_host(lo_b), _host(up_b), c.quantiles, binfo['n_used'])
        win['band_po'] = band(c.fc_ids)
        if c.ov_ids:
            win['band_ov'] = band(c.ov_ids, err_m=_m_rows(dev, s, c, c.ov_vars))
    if c.sc_ids:                                                   # before the weighting, under the weights of entry
        skw = dict(pkw, weights=s.q, include=(status_d & abi.STATUS_NONFINITE) == 0)
        sobs = np.ascontiguousarray(c.sc_obs[:, d_lo:d_hi])
        po_w, ov_w = eng.predictive_scores(table_d, mask, c.sc_ids, sobs, **skw), None
        if any(v is not None for v in c.sc_vars):                  # the m the filter knows; 0 for the other series
            ov_w = eng.predictive_scores(table_d, mask, c.sc_ids, sobs, err_m=_m_rows(dev, s, c, c.sc_vars), **skw)
        win['scores'] = (po_w, ov_w)
        ms['score'] = po_w[2]['kernel_ms'] + (0.0 if ov_w is None else ov_w[2]['kernel_ms'])
    linfo = eng.pf_loglik(table_d, mask, hs['obs'][:, :, d_lo:d_hi], hs['pairs'], _m_rows(dev, s, c, [v for v, _ in hs['pairs']]), s.lw,
                          status=status_d, inc=s.inc, accumulate=True, **tkw)
    s.w, s.q, winfo = eng.pf_weights(s.lw, s.w, s.q)
    ms['loglik'], ms['weights'] = linfo['kernel_ms'], winfo['kernel_ms']
    if c.record:
        rec.update(inc=_host(s.inc), q=_host(s.q).astype(np.uint64), state_out=_host(s.state), ancestors=np.arange(E, dtype=np.int32))
    if winfo['T'] == 0:
        raise RuntimeError("assimilate: every particle is dead in window %d (%s to %s): no log weight is finite -- the error "
                           "model's m or the prior box leaves no particle that explains the observations"
                           % (t, c.index[d_lo].date(), c.index[d_hi - 1].date()))
    lm = particle.log_mean(winfo['lw_max'], winfo['sum_w'], E)
    win.update(ess=particle.ess(winfo['sum_w'], winfo['sum_w2']), log_evidence=lm - s.lm_prev)
    s.lm_prev = lm
    win['resampled'] = bool(win['ess'] < float(c.resample_threshold) * E)
    if win['resampled']:
        anc_d, _, rinfo = eng.pf_resample(s.q, c.seed, t, offspring=False)
        ms['resample'], win['n_unique'] = rinfo['kernel_ms'], int(rinfo['n_unique'])
        for owner, key in ((s, 'state'), (dev, 'mp_d'), (dev, 'rp_d'), (dev, 'ft_d'), (s, 'theta')) + (((s, 'noise'),) if c.noisy else ()):
            # all a particle owns travels with it, the noise state of its forcing errors included
            dst, ginfo = eng.gather_members(getattr(owner, key), anc_d)
            setattr(owner, key, dst)
            ms['gather'] += ginfo['kernel_ms']
        s.lw.zero_()
        s.lm_prev = 0.0
        if c.forecast_weighted or c.score:                         # the next window's particles enter it equally weighted
            s.w, s.q, _ = eng.pf_weights(s.lw, s.w, s.q)
        if c.move is not None:
            if c.move[0] == 'liu_west':
                a = c.move[1]
                centre = _host(s.theta.mean(dim=1))
                scale = np.sqrt(1.0 - a * a) * _host(s.theta.std(dim=1, unbiased=False))
            else:
                a, centre, scale = 1.0, np.zeros(len(c.target)), c.move[1]
            jinfo = eng.pf_jitter(s.theta, t, a, centre, scale, c.lo, c.hi, c.target, dev.mp_d, dev.ft_d, seed=c.seed)
            ms['jitter'], win['n_outside'] = jinfo['kernel_ms'], int(jinfo['n_outside'])
        rec.update(ancestors=_host(anc_d))
    if c.record:
        rec['theta_after'] = _host(s.theta)
    torch.cuda.synchronize(eng.tdev)
    win['wall_ms'] = 1e3 * (time.perf_counter() - w0)
    return win


def assimilate(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, obs_dict, priors, variables=('Q',), error_m=None,
               n_particles=None, window=30, start=None, initial_state=None, seed=0, resample_threshold=1.0, rejuvenate='liu_west',
               delta=0.98, quantiles=None, forecast_series=None, record=False, state=None, step_len=1., solver=None, device=0,
               out_reaches=None, forecast_weighted=False, score=False, forcing_error=None, error_phi=None):
    """Update the parameter distribution and the model state of ``n_particles`` particles window by window as the observations
    of ``obs_dict`` arrive (sequential importance resampling), every step on the device.

    ``priors``, ``variables``, ``error_m``, ``out_reaches`` and their checks are ``sample_posterior``'s: names are member
    parameters, ``'f_TDP'`` and ``'m_<VAR>'`` -- which makes the error model's ``m`` a filtered dimension --, the box is
    ``lo <= x < hi``, and a selected variable needs more than 10 observations over the whole period at some output reach (a
    single window needs none).  The errors are independent from day to day: ``'phi_<VAR>'`` names and ``error_phi`` -- the AR(1)
    error model of ``sample_posterior`` -- are a ``ValueError`` here, because a window's likelihood would need each particle's last
    residual of the window before, carried through resampling.  ``window``: as ``ensemble.window_bounds`` takes it (days per window, ``'annual'``, or start dates).
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

    ``forcing_error``: input noise, as ``run_simply_p_ensemble`` takes it (``simplyp_amd.forcing``): every window's run draws each
    particle's own rainfall, PET and air temperature on the device, keyed on (``seed``, the particle's index, the calendar group
    id, the forcing row).  Siblings of one ancestor therefore diverge after a resampling through their forcing as well as through
    the rejuvenation move, and because the group ids are absolute a continuation from ``state`` draws what the one call would.
    With ``record`` the per-window list ``forcing_table`` [E, 2 or 3, days] is kept.  With a ``rho`` (autocorrelated errors) the
    noise state [6, n_particles] (``abi.FORCING_NOISE_ROWS``) is something a particle owns: it starts stationary or comes from
    ``state``, goes into and out of every window's run, is gathered with the ancestors on resampling and returned as
    ``['state']['forcing_noise']``; ``record`` keeps ``forcing_noise_in`` (None for a stationary start) and ``forcing_noise_out``
    (after the window's run, before its resampling) per window.  After a resampling two offspring of one ancestor share
    ``z_prev`` and then draw their own ``eps``, because the member id of a draw is the particle's slot.

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

    if error_phi or (isinstance(priors, dict) and any(str(nm).startswith('phi_') for nm in priors)):
        raise ValueError("assimilate takes no lag-one coefficient ('phi_<VAR>' names, error_phi): the window likelihood has "
                         "independent errors")
    names, variables, lo, hi, target, m_dim, m_const, _ = _plan(priors, variables, error_m, check_shape)
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
        quantiles = request.probabilities('quantiles', quantiles)
        fc_names, fc_ids, _ = request.series_ids('forecast_series', known_m if forecast_series is None else forecast_series,
                                              "%s and %s" % (abi.TQ_DERIVED_SERIES, marshal.FLUX_COLUMNS), marshal.FLUX_COLUMNS)
    elif forecast_series is not None:
        raise ValueError("forecast_series needs quantiles: the probabilities of the bands")
    bounds = ensemble.window_bounds(met_df.index, window)
    forcing_rules.refuse_pet_model(forcing_error, 'assimilate')

    with marshal.reference_edits(p_SU, p_LU, p_SC, p):
        hs = _host_setup(met_df, p_struc, p_SU, p_LU, p_SC, p, obs_dict, names, variables, lo, hi, out_reaches)
        scs = hs['scs']
        fe = forcing_rules.resolve(forcing_error, met_df.index, E, hs['snow'], seed)
        sc_names, sc_ids, sc_obs = request.observed_series(obs_dict, hs['reaches'], hs['obs']) if score else (None, None, None)
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
        noisy = forcing_rules.any_rho(fe)
        nz_in = None
        if noisy and state is not None and state.get('forcing_noise') is not None:
            nz_in = forcing_rules.check_noise(_host(state['forcing_noise']) if hasattr(state['forcing_noise'], 'cpu') else state['forcing_noise'], E)
        _check_inside(theta0, lo, hi, names)
        if t0 + len(bounds) >= 1 << 32 or day0 + len(met_df) >= 1 << 31:
            raise ValueError("the absolute window index must stay below 2^32 and the absolute day below 2^31")

        # ---- the device: everything is marshalled and uploaded once; from here on only info structs come back per window
        dev = _DeviceEnsemble("assimilate keeps members in particle order", met_df, p_SU, p_LU, p_SC, p, dynamic_options, step_len,
                              solver, device, E, marshal.FLUX_COLUMNS, hs['snow'])
        eng, torch = dev.eng, dev.torch
        s = SimpleNamespace(theta=eng.to_device(theta0, torch.float64), lw=eng.to_device(lw0, torch.float64),
                            inc=torch.empty((E,), **dev.f64), state=None if st_in is None else eng.to_device(st_in, torch.float64).clone(),
                            noise=None if nz_in is None else eng.to_device(nz_in, torch.float64).clone())
        dev.write_positions(s.theta, target)
        s.w, s.q, info = eng.pf_weights(s.lw)
        s.lm_prev = particle.log_mean(info['lw_max'], info['sum_w'], E)
        var_of = lambda c_: abi.GOF_VARS.index(variables[known_m.index(c_)]) if c_ in known_m else None
        ov_at = [i for i, c_ in enumerate(fc_names or []) if c_ in known_m]
        c = SimpleNamespace(index=met_df.index, seed=seed, day0=day0, target=target, lo=lo, hi=hi, m_dim=m_dim, m_const=m_const,
                            resample_threshold=resample_threshold, move=move, record=record, score=score, quantiles=quantiles,
                            forecast_weighted=forecast_weighted, fc_ids=fc_ids, ov_ids=[fc_ids[i] for i in ov_at],
                            ov_vars=[var_of(fc_names[i]) for i in ov_at], sc_ids=sc_ids, sc_obs=sc_obs,
                            sc_vars=[var_of(c_) for c_ in sc_names or []], forcing=fe, noisy=noisy)
        wins = [_window(dev, hs, s, c, t0 + n, d_lo, d_hi) for n, (d_lo, d_hi) in enumerate(bounds)]

    theta, lw = _host(s.theta), _host(s.lw)
    overrides, err_m = _shaped_for_the_ensemble(names, target, variables, m_dim, m_const, theta)
    res = {k: np.array([w[k] for w in wins]) for k in ('ess', 'log_evidence', 'resampled', 'n_unique', 'n_outside')}
    res.update(names=names, windows=[(met_df.index[a_], met_df.index[b_ - 1], int(a_), int(b_)) for a_, b_ in bounds],
               log_evidence_total=float(np.sum(res['log_evidence'])),
               kernel_ms={k: [w['ms'][k] for w in wins] for k in STEPS + (('score',) if score else ())},
               pilot_ms=[w['pilot_ms'] for w in wins], wall_ms=[w['wall_ms'] for w in wins],
               theta=theta, log_weights=lw, overrides=overrides, error_m=err_m,
               state=dict(rows=list(abi.STATE_ROWS), reaches=list(scs), data=_host(s.state), end=pd.Timestamp(met_df.index[-1]),
                          theta=theta.copy(), lw=lw.copy(), t=t0 + len(bounds), seed=seed, day=day0 + len(met_df)))
    if noisy:
        res['state']['forcing_noise'] = _host(s.noise)
    if quantiles is not None:
        res['forecast'] = dict(q=list(quantiles), series=list(fc_names), param_only=np.concatenate([w['band_po'] for w in wins], axis=2),
                               overall_series=[fc_names[i] for i in ov_at],
                               overall=np.concatenate([w['band_ov'] for w in wins], axis=2) if ov_at else None, day0=day0)
        if forecast_weighted:
            res['forecast']['rule'] = 'inverted_cdf'
    if score:
        res['scores'] = _joined_scores(sc_names, hs['reaches'], sc_obs, [w['scores'] for w in wins if 'scores' in w], seed, day0)
    if record:
        res.update({k: [w['rec'][k] for w in wins] for k in ('inc', 'q', 'ancestors', 'theta_before', 'theta_after', 'state_in', 'state_out')
                    + (('forcing_table',) if fe is not None else ()) + (('forcing_noise_in', 'forcing_noise_out') if noisy else ())})
    return res


def _joined_scores(series, reaches, obs, parts, seed, day0):
    """The windows' scores laid end to end along the day axis, in the shape of ``run_simply_p_ensemble(score=True)['scores']``;
    ``weight_total``, ``n_members`` and ``info`` are one entry per window (a window's pit is taken with its own total)."""
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


assimilate.__doc__ = assimilate.__doc__ % (marshal.FLUX_COLUMNS, list(STEPS))
