"""Sampling the posterior on the device: the middle of the reference's calibration notebook (Development/2016/MCMC.ipynb, cell 10),
``emcee.EnsembleSampler(n_walk, n_dim, log_posterior).run_mcmc(start, n_steps)``, with the walkers, the model runs, the
likelihood and the decisions all on the GPU.  ``simplyp_amd.mcmc`` is the NumPy statement of the move."""

import time

import numpy as np

from . import abi, marshal, mcmc, predictive

START_SERIES = 0x53544152        # "STAR": the counter's fourth word of the start ball's normals


def _plan(priors, variables, error_m, n_walkers):
    """Names, box, targets and error-model wiring of a call; host only, raises ValueError."""
    if not isinstance(priors, dict) or not priors:
        raise ValueError("priors must be a dict name -> (lo, hi) with at least one entry")
    names = list(priors)
    variables = [variables] if isinstance(variables, str) else list(variables)
    unknown = [v for v in variables if v not in abi.GOF_VARS]
    if unknown or not variables or len(set(variables)) != len(variables):
        raise ValueError("variables must be distinct names among %s (got %s)" % (abi.GOF_VARS, variables))
    error_m = dict(error_m or {})
    unknown = [v for v in error_m if v not in variables]
    if unknown:
        raise ValueError("error_m names variables that are not selected: %s" % unknown)
    target, m_dim, m_const = [], [-1] * len(abi.GOF_VARS), [float('nan')] * len(abi.GOF_VARS)
    for d, nm in enumerate(names):
        if nm in marshal.PM_NAMES:
            target.append(marshal.PM_NAMES.index(nm))
        elif nm == 'f_TDP':
            target.append(abi.MCMC_TARGET_F_TDP)
        elif nm.startswith('m_') and nm[2:] in variables:
            if nm[2:] in error_m:
                raise ValueError("%s is sampled and fixed through error_m at once" % nm)
            target.append(abi.MCMC_TARGET_NONE)
            m_dim[abi.GOF_VARS.index(nm[2:])] = d
        else:
            raise ValueError("unknown parameter %r: sampled names are %s, 'f_TDP' and 'm_<VAR>' for the selected variables %s"
                             % (nm, marshal.PM_NAMES, variables))
    for v in variables:
        vi = abi.GOF_VARS.index(v)
        if m_dim[vi] < 0:
            if v not in error_m:
                raise ValueError("variable %r needs its error model: sample 'm_%s' or fix it through error_m={'%s': ...}" % (v, v, v))
            m_const[vi] = float(error_m[v])
    n_dim = len(names)
    if n_walkers is None:
        raise ValueError("n_walkers must be given")
    try:
        mcmc.check_shape(int(n_walkers), n_dim)
    except ValueError as exc:
        raise ValueError("sample_posterior: %s" % exc)
    try:
        box = np.array([[float(priors[nm][0]), float(priors[nm][1])] for nm in names], dtype=np.float64)
    except (TypeError, ValueError, IndexError):
        raise ValueError("priors must map each name to a pair (lo, hi)")
    if not (box[:, 0] < box[:, 1]).all():
        bad = names[int(np.argmin(box[:, 0] < box[:, 1]))]
        raise ValueError("prior of %r needs lo < hi (got %s)" % (bad, tuple(priors[bad])))
    return names, variables, box[:, 0].copy(), box[:, 1].copy(), np.array(target, dtype=np.int32), m_dim, m_const


def sample_posterior(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, obs_dict, priors, variables=('Q',), error_m=None,
                     n_walkers=None, n_steps=0, start=None, seed=0, a=2.0, thin=1, state=None, record_proposals=False,
                     step_len=1., solver=None, device=0, out_reaches=None):
    """Sample the posterior of model parameters with the affine-invariant stretch move (Goodman & Weare 2010; the reference's
    ``run_mcmc``), every half-step one ensemble run of ``n_walkers / 2`` members on the device.

    ``priors``: dict name -> (lo, hi), the flat prior box ``lo <= x < hi`` (the reference's ``log_prior``); names are member
    parameters (``marshal.PM_NAMES``), ``'f_TDP'``, and ``'m_<VAR>'`` -- the ``m`` of the error model ``sigma = m * sim`` --
    for ``VAR`` in ``variables`` (names of ``abi.GOF_VARS``: the observed series the likelihood is taken over, at every
    output reach that has more than 10 observations of it).  A variable whose ``m`` is not sampled gets it through
    ``error_m={'Q': 0.1}``.  ``n_walkers`` even and >= twice the number of names (at most 16); ``n_steps`` steps;
    ``a`` the stretch scale; ``seed`` the key of the counter-based random stream (``simplyp_amd.mcmc``); every ``thin``-th
    step is kept.  ``start``: None = the notebook's ball -- the workbook's values (box centres for the ``m``) plus
    ``1e-4 (hi - lo) z`` with ``z = predictive.standard_normal(seed, walker, dimension, 0, START_SERIES)`` -- or an array
    [n_dim, n_walkers] inside the box; a start whose log posterior is not finite raises ``ValueError``.  ``state``: the
    ``'state'`` of an earlier result: the chain continues from it bit for bit (``start`` is ignored).

    The inputs are marshalled and uploaded once; one half-step is ``mcmc_propose`` -> ``Engine.run`` -> ``Engine.gof`` ->
    ``mcmc_log_prob`` -> ``mcmc_accept`` on device buffers of ``n_walkers / 2`` members, and the chain comes to the host at the
    end.  Returns dict(names, chain[n_kept, n_dim, W], log_prob[n_kept, W], acceptance_fraction[W], n_steps, seed, overrides,
    error_m -- the last positions shaped for ``run_simply_p_ensemble(overrides=, predictive_series=list(error_m),
    predictive_m=error_m)``, ``error_m`` keyed by the ``df_R`` series name --, state = dict(theta, lp, n_accept, t),
    start = dict(theta, lp, t): where this call began,
    proposals[n_steps, n_dim, W] and proposal_log_prob[n_steps, W] with ``record_proposals``, stats = per-half-step lists of
    wall_ms, run_kernel_ms, gof_ms, sampler_ms, n_inside, n_accepted, and start_wall_ms, start_run_kernel_ms of the start's two
    evaluations).  ``ValueError`` before any device call for an odd or
    too small ``n_walkers``, an unknown name, ``lo >= hi``, a start outside the box, a selected variable with 10 or fewer
    observations at every output reach, a missing ``obs_dict``, a box whose corners ``marshal.validate_ensemble`` rejects.
    The caller's ``p_LU`` / ``p_SC`` are edited in place exactly as by ``run_simply_p``."""
    from . import visualise_results as vr
    from .model import _engine_opts

    if not obs_dict:
        raise ValueError("sample_posterior needs obs_dict: the observations the likelihood is taken over")
    names, variables, lo, hi, target, m_dim, m_const = _plan(priors, variables, error_m, n_walkers)
    n_dim, W = len(names), int(n_walkers)
    h = W // 2
    if not float(a) > 1.0:
        raise ValueError("the stretch scale a must be > 1 (got %r)" % (a,))
    seed, thin, n_steps = int(seed), int(thin), int(n_steps)
    if not 0 <= seed < 1 << 64 or thin < 1 or n_steps < 0:
        raise ValueError("seed must be in [0, 2^64), thin >= 1 and n_steps >= 0")

    marshal.prologue(p_SU, p_LU, p_SC, p)
    scs = marshal.sc_list(p)
    up_ptr, up_idx, _ = marshal.topology(p_struc, p)
    reaches = scs if out_reaches is None else list(out_reaches)
    oreach = None if out_reaches is None else [scs.index(int(r)) for r in out_reaches]
    obs = vr.observation_array(obs_dict, reaches, met_df.index)
    n_obs = (~np.isnan(obs)).sum(axis=-1)                                 # [R, 6]
    pairs = []
    for v in variables:
        vi = abi.GOF_VARS.index(v)
        at = [(vi, r) for r in range(len(reaches)) if n_obs[r, vi] > 10]
        if not at:
            raise ValueError("variable %r has 10 or fewer observations at every output reach: its statistics are NaN "
                             "(visualise_results.py:430)" % v)
        pairs += at
    if len(pairs) > 32:
        raise ValueError("at most 32 (variable, output reach) pairs enter the likelihood (got %d): name fewer out_reaches" % len(pairs))
    # the reference's input checks at the box's two extreme corners (the checks are per parameter)
    pm = [(d, nm) for d, nm in enumerate(names) if nm in marshal.PM_NAMES]
    if pm:
        corners = marshal.member_params(p, p_LU, 2, {nm: np.array([lo[d], hi[d]]) for d, nm in pm})
        try:
            marshal.validate_ensemble(corners, marshal.reach_params(p_SC, p, 2), scs)
        except AssertionError as exc:
            raise ValueError("the prior box holds points the model rejects: %s" % exc)
    snow = 'f_DDSM' in names or 'D_snow_0' in names
    if snow and not {'Precipitation', 'T_air'} <= set(met_df.columns):
        raise ValueError("sampling f_DDSM / D_snow_0 runs the snow module in the kernel: met_df needs 'Precipitation' and 'T_air'")

    base = marshal.member_params(p, p_LU, 1)[:, 0]
    if state is not None:
        theta0 = np.array(state['theta'], dtype=np.float64)
        lp0 = np.array(state['lp'], dtype=np.float64)
        nacc0 = np.array(state['n_accept'], dtype=np.int32)
        t0 = int(state['t'])
        if theta0.shape != (n_dim, W) or lp0.shape != (W,) or nacc0.shape != (W,) or t0 < 0:
            raise ValueError("state does not match this call: theta %s for %d names and %d walkers" % (theta0.shape, n_dim, W))
    else:
        t0, lp0, nacc0 = 0, None, np.zeros(W, dtype=np.int32)
        if start is None:
            centre = np.array([base[marshal.PM_NAMES.index(nm)] if nm in marshal.PM_NAMES else
                               (float(p['f_TDP']) if nm == 'f_TDP' else 0.5 * (lo[d] + hi[d])) for d, nm in enumerate(names)])
            z = predictive.standard_normal(seed, np.arange(W)[None, :], np.arange(n_dim)[:, None], 0, START_SERIES)
            theta0 = centre[:, None] + (1e-4 * (hi - lo))[:, None] * z
        else:
            theta0 = np.array(start, dtype=np.float64)
            if theta0.shape != (n_dim, W):
                raise ValueError("start must have shape [n_dim, n_walkers] = %s, got %s" % ((n_dim, W), theta0.shape))
    if not ((theta0 >= lo[:, None]) & (theta0 < hi[:, None])).all():
        d = int(np.argmin(((theta0 >= lo[:, None]) & (theta0 < hi[:, None])).all(axis=1)))
        raise ValueError("the start lies outside the prior box in %r" % names[d])
    if t0 + n_steps >= 1 << 32:
        raise ValueError("the absolute step index must stay below 2^32")

    # ---- the device: everything is marshalled and uploaded once, for an ensemble of h members
    from . import engine
    eng = engine.get_engine(device)
    torch = eng.torch
    cols = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']              # what simplyp_gof reads
    mask = marshal.mask_of_columns(cols)
    opts = _engine_opts(p_SU, p, dynamic_options, step_len, solver, mask, snow=snow)
    if opts.out_slot_order:
        raise ValueError("sample_posterior keeps members in walker order: solver['out_slot_order'] must stay 0")
    forcing, doy = marshal.forcing_arrays(met_df, snow=snow)
    f_d, doy_d = eng.to_device(forcing, torch.float64), eng.to_device(doy, torch.int32)
    mp_d = eng.to_device(marshal.member_params(p, p_LU, h), torch.float64)
    rp_d = eng.to_device(marshal.reach_params(p_SC, p, h), torch.float64)
    f64 = dict(dtype=torch.float64, device=eng.tdev)
    ft_d = torch.full((h,), float(p['f_TDP']), **f64)
    D, R = len(met_df), len(reaches)
    out_d = torch.empty((len(cols), D, R, h), **f64)
    gof_d = torch.empty((len(abi.GOF_STATS), len(abi.GOF_VARS), R, h), **f64)
    prop_d, lpp_d = torch.empty((n_dim, h), **f64), torch.empty((h,), **f64)
    inside_d = torch.ones((h,), dtype=torch.int32, device=eng.tdev)
    theta_d = eng.to_device(theta0, torch.float64)
    nacc_d = eng.to_device(nacc0, torch.int32)
    kept = [t for t in range(t0, t0 + n_steps) if (t + 1) % thin == 0]
    chain_d = torch.empty((len(kept), n_dim + 1, W), **f64)
    if record_proposals:
        props_d, plp_d = torch.empty((n_steps, n_dim, W), **f64), torch.empty((n_steps, W), **f64)
    stats = dict(wall_ms=[], run_kernel_ms=[], gof_ms=[], sampler_ms=[], n_inside=[], n_accepted=[],
                 start_wall_ms=[], start_run_kernel_ms=[])

    def evaluate():
        """The model and the likelihood at the run points mp_d / ft_d hold, for the proposals in prop_d: lpp_d."""
        _, status_d, rstats = eng.run(f_d, doy_d, mp_d, rp_d, up_ptr, up_idx, opts, out_reaches=oreach, out=out_d)
        _, ginfo = eng.gof(out_d, mask, obs, ft_d, rp_d, out_reaches=oreach, gof=gof_d)
        linfo = eng.mcmc_log_prob(gof_d, pairs, m_dim, m_const, prop_d, lpp_d, status=status_d, inside=inside_d)
        return rstats['kernel_ms'], ginfo['kernel_ms'], linfo['kernel_ms']

    if lp0 is None:                               # the start's log posterior: one evaluation per half, through the same kernels
        lp_d = torch.empty((W,), **f64)
        for k in (0, 1):
            sl = slice(k * h, (k + 1) * h)
            torch.cuda.synchronize(eng.tdev)
            w0 = time.perf_counter()
            prop_d.copy_(theta_d[:, sl])
            for d in range(n_dim):
                if target[d] >= 0:
                    mp_d[int(target[d])].copy_(theta_d[d, sl])
                elif target[d] == abi.MCMC_TARGET_F_TDP:
                    ft_d.copy_(theta_d[d, sl])
            run_ms = evaluate()[0]
            lp_d[sl].copy_(lpp_d)
            torch.cuda.synchronize(eng.tdev)
            stats['start_wall_ms'].append(1e3 * (time.perf_counter() - w0))
            stats['start_run_kernel_ms'].append(run_ms)
        lp_host = lp_d.cpu().numpy()
        if not np.isfinite(lp_host).all():
            marshal.epilogue_mutations(p_SU, p_LU, p_SC, p)
            raise ValueError("the start has a non-finite log posterior at walker %d (%r): the model or the likelihood fails there"
                             % (int(np.argmin(np.isfinite(lp_host))), float(lp_host[int(np.argmin(np.isfinite(lp_host)))])))
    else:
        lp_d = eng.to_device(lp0, torch.float64)

    lp_start = lp_d.cpu().numpy()
    for n, t in enumerate(range(t0, t0 + n_steps)):
        row = chain_d[kept.index(t)] if (t + 1) % thin == 0 else None
        for k in (0, 1):
            torch.cuda.synchronize(eng.tdev)
            w0 = time.perf_counter()
            pinfo = eng.mcmc_propose(theta_d, k, t, lo, hi, target, prop_d, inside_d, mp_d, ft_d, a=a, seed=seed)
            run_ms, gof_ms, lp_ms = evaluate()
            ainfo = eng.mcmc_accept(theta_d, lp_d, nacc_d, k, t, prop_d, inside_d, lpp_d, chain_row=row, a=a, seed=seed)
            stats['wall_ms'].append(1e3 * (time.perf_counter() - w0))
            stats['run_kernel_ms'].append(run_ms)
            stats['gof_ms'].append(gof_ms)
            stats['sampler_ms'].append(pinfo['kernel_ms'] + lp_ms + ainfo['kernel_ms'])
            stats['n_inside'].append(pinfo['n_inside'])
            stats['n_accepted'].append(ainfo['n_accepted'])
            if record_proposals:
                props_d[n, :, k * h:(k + 1) * h].copy_(prop_d)
                plp_d[n, k * h:(k + 1) * h].copy_(lpp_d)
    marshal.epilogue_mutations(p_SU, p_LU, p_SC, p)

    chain = chain_d.cpu().numpy()
    theta, lp, n_accept = theta_d.cpu().numpy(), lp_d.cpu().numpy(), nacc_d.cpu().numpy()
    t_end = t0 + n_steps
    res = dict(names=names, chain=np.ascontiguousarray(chain[:, :n_dim]), log_prob=np.ascontiguousarray(chain[:, n_dim]),
               acceptance_fraction=n_accept / float(t_end) if t_end else np.zeros(W), n_steps=n_steps, seed=seed,
               overrides={nm: theta[d].copy() for d, nm in enumerate(names) if target[d] != abi.MCMC_TARGET_NONE},
               error_m={abi.TQ_DERIVED_SERIES[abi.GOF_VARS.index(v)]:
                        (theta[m_dim[abi.GOF_VARS.index(v)]].copy() if m_dim[abi.GOF_VARS.index(v)] >= 0
                         else np.full(W, m_const[abi.GOF_VARS.index(v)])) for v in variables},
               state=dict(theta=theta, lp=lp, n_accept=n_accept, t=t_end), start=dict(theta=theta0, lp=lp_start, t=t0), stats=stats)
    if record_proposals:
        res['proposals'], res['proposal_log_prob'] = props_d.cpu().numpy(), plp_d.cpu().numpy()
    return res
