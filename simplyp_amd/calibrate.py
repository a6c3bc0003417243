"""Calibration on the device: the middle of the reference's calibration notebooks (Development/2016/MCMC.ipynb, MAP.ipynb).

``find_map`` is the notebooks' ``find_map`` -- ``scipy.optimize.fmin`` on the negative log posterior -- as a multi-start
Nelder-Mead search (``simplyp_amd.neldermead`` is its NumPy statement); ``sample_posterior`` is their
``emcee.EnsembleSampler(n_walk, n_dim, log_posterior).run_mcmc(start, n_steps)`` (``simplyp_amd.mcmc`` states the move); and
``start_ball`` hands the one's result to the other.  The points, the model runs, the likelihood and the decisions are all on the
GPU; both calls share the names, the checks, the marshalling and the evaluation (``_host_setup``, ``_Evaluator``).
``find_pareto`` is the multi-objective calibration the notebooks stop short of: NSGA-II over several goodness-of-fit criteria at
once (``simplyp_amd.nsga2`` states the rule), on the same set-up without a likelihood."""

import time

import numpy as np

from . import abi, marshal, mcmc, neldermead, nsga2, pareto, predictive, priors as _priors, visualise_results as vr
from .model import _DeviceEnsemble
from .priors import box as _box

START_SERIES = 0x53544152        # "STAR": the counter's fourth word of the start ball's normals


def _plan(priors, variables, error_m, check_shape, error_phi=None):
    """Names, box, targets and error-model wiring of a call; host only, raises ValueError.  ``check_shape(n_dim)`` is the
    caller's own rule for how many points it moves.  The last item is None when no variable has a lag-one coefficient -- neither
    a sampled ``'phi_<VAR>'`` nor one fixed through ``error_phi`` -- and (phi_dim, phi_const, the variables that have one)
    otherwise, wired like (m_dim, m_const) with ``phi_const = 0`` (independent errors) for the variables that have none."""
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
    error_phi = dict(error_phi or {})
    unknown = [v for v in error_phi if v not in variables]
    if unknown:
        raise ValueError("error_phi names variables that are not selected: %s" % unknown)
    for v, x in error_phi.items():
        if not -1.0 < float(x) < 1.0:
            raise ValueError("error_phi[%r] = %r is not inside (-1, 1)" % (v, x))
    target, m_dim, m_const = [], [-1] * len(abi.GOF_VARS), [float('nan')] * len(abi.GOF_VARS)
    phi_dim, phi_const = [-1] * len(abi.GOF_VARS), [0.0] * len(abi.GOF_VARS)
    for d, nm in enumerate(names):
        if _priors.target_of(nm) is not None:
            target.append(_priors.target_of(nm))
        elif nm.startswith('m_') and nm[2:] in variables:
            if nm[2:] in error_m:
                raise ValueError("%s is sampled and fixed through error_m at once" % nm)
            target.append(abi.MCMC_TARGET_NONE)
            m_dim[abi.GOF_VARS.index(nm[2:])] = d
        elif nm.startswith('phi_') and nm[4:] in abi.GOF_VARS:
            if nm[4:] not in variables:
                raise ValueError("%s: variable %r is not selected (variables = %s)" % (nm, nm[4:], variables))
            if nm[4:] in error_phi:
                raise ValueError("%s is sampled and fixed through error_phi at once" % nm)
            try:
                plo, phi_hi = (float(x) for x in priors[nm])
            except (TypeError, ValueError):
                raise ValueError("priors[%r] must be (lo, hi)" % nm)
            if not (-1.0 < plo and phi_hi < 1.0):
                raise ValueError("the box of %s must lie inside (-1, 1): the AR(1) model is stationary for |phi| < 1 only (got %r)"
                                 % (nm, (plo, phi_hi)))
            target.append(abi.MCMC_TARGET_NONE)
            phi_dim[abi.GOF_VARS.index(nm[4:])] = d
        else:
            raise ValueError("unknown parameter %r: sampled names are %s, 'f_TDP', and 'm_<VAR>' and 'phi_<VAR>' for the selected "
                             "variables %s" % (nm, marshal.PM_NAMES, variables))
    for v in variables:
        vi = abi.GOF_VARS.index(v)
        if m_dim[vi] < 0:
            if v not in error_m:
                raise ValueError("variable %r needs its error model: sample 'm_%s' or fix it through error_m={'%s': ...}" % (v, v, v))
            m_const[vi] = float(error_m[v])
        if v in error_phi:
            phi_const[vi] = float(error_phi[v])
    check_shape(len(names))
    lo, hi = _box(priors, names)
    with_phi = [v for v in variables if v in error_phi or phi_dim[abi.GOF_VARS.index(v)] >= 0]
    phi = (phi_dim, phi_const, with_phi) if with_phi else None
    return names, variables, lo, hi, np.array(target, dtype=np.int32), m_dim, m_const, phi


def _host_setup(met_df, p_struc, p_SU, p_LU, p_SC, p, obs_dict, names, variables, lo, hi, out_reaches):
    """What a calibration call works out on the host, after the prologue and before it touches the device: the topology, the
    observations and the (variable, output reach) pairs of the likelihood, the input checks at the box's corners, the snow rule,
    the workbook's member parameters.  Raises ValueError."""
    scs, up_ptr, up_idx, reaches, oreach = marshal.catchment(p_struc, p, out_reaches)
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
    _priors.check_corners(names, lo, hi, p, p_LU, p_SC, scs)
    snow = _priors.snow_rule(names, met_df)
    base = marshal.member_params(p, p_LU, 1)[:, 0]
    centre = np.array([base[marshal.PM_NAMES.index(nm)] if nm in marshal.PM_NAMES else
                       (float(p['f_TDP']) if nm == 'f_TDP' else 0.5 * (lo[d] + hi[d])) for d, nm in enumerate(names)])
    return dict(scs=scs, up_ptr=up_ptr, up_idx=up_idx, reaches=reaches, oreach=oreach, obs=obs, pairs=pairs, snow=snow, centre=centre)


class _Evaluator:
    """The device side both calls share: an ensemble of ``n_members`` uploaded once (``dev``) and the buffers of one evaluation;
    ``evaluate()`` is the model and the likelihood at the run points ``dev.mp_d`` / ``dev.ft_d`` hold: the log posterior in ``lpp_d``."""

    def __init__(self, order, hs, met_df, p_SU, p_LU, p_SC, p, dynamic_options, step_len, solver, device, n_members, n_dim,
                 m_dim, m_const, phi=None):
        self.dev = dev = _DeviceEnsemble(order, met_df, p_SU, p_LU, p_SC, p, dynamic_options, step_len, solver, device, n_members,
                                         marshal.FLUX_COLUMNS, hs['snow'])        # the columns simplyp_gof reads
        torch, f64 = dev.torch, dev.f64
        D, R = len(met_df), len(hs['reaches'])
        self.out_d = torch.empty((len(marshal.FLUX_COLUMNS), D, R, n_members), **f64)
        self.gof_d = torch.empty((len(abi.GOF_STATS), len(abi.GOF_VARS), R, n_members), **f64)
        self.prop_d, self.lpp_d = torch.empty((n_dim, n_members), **f64), torch.empty((n_members,), **f64)
        self.inside_d = torch.ones((n_members,), dtype=torch.int32, device=dev.eng.tdev)
        self.hs, self.m_dim, self.m_const, self.phi = hs, m_dim, m_const, phi
        self.lag_ms = None                            # the last evaluation's lag-one pass; stays None without a phi
        if phi is not None:
            self.lag_d = torch.empty((len(abi.LAG_STATS), len(abi.GOF_VARS), R, n_members), **f64)

    def run_gof(self):
        """The model at the run points and the goodness-of-fit table ``gof_d`` of its output: (the members' status on the device,
        the run's stats, the table's info)."""
        hs, dev, eng = self.hs, self.dev, self.dev.eng
        _, status_d, rstats = eng.run(dev.f_d, dev.doy_d, dev.mp_d, dev.rp_d, hs['up_ptr'], hs['up_idx'], dev.opts,
                                      out_reaches=hs['oreach'], out=self.out_d)
        _, ginfo = eng.gof(self.out_d, dev.mask, hs['obs'], dev.ft_d, dev.rp_d, out_reaches=hs['oreach'], gof=self.gof_d)
        return status_d, rstats, ginfo

    def evaluate(self):
        """Returns the kernel times of the run, the goodness of fit and the log posterior, in ms.  With a lag-one coefficient
        (``phi``) the lag-one sums are taken between the last two and the AR(1) log posterior replaces the independent one."""
        hs, dev, eng = self.hs, self.dev, self.dev.eng
        status_d, rstats, ginfo = self.run_gof()
        if self.phi is None:
            linfo = eng.mcmc_log_prob(self.gof_d, hs['pairs'], self.m_dim, self.m_const, self.prop_d, self.lpp_d, status=status_d,
                                      inside=self.inside_d)
        else:
            _, ainfo = eng.gof_lag(self.out_d, dev.mask, hs['obs'], dev.ft_d, dev.rp_d, out_reaches=hs['oreach'], lag=self.lag_d)
            self.lag_ms = ainfo['kernel_ms']
            linfo = eng.mcmc_log_prob_ar1(self.gof_d, self.lag_d, hs['pairs'], self.m_dim, self.m_const, self.phi[0], self.phi[1],
                                          self.prop_d, self.lpp_d, status=status_d, inside=self.inside_d)
        return rstats['kernel_ms'], ginfo['kernel_ms'], linfo['kernel_ms']


def _shaped_for_the_ensemble(names, target, variables, m_dim, m_const, theta):
    """Positions ``theta[n_dim, M]`` as ``run_simply_p_ensemble(overrides=, predictive_series=list(error_m), predictive_m=error_m)``
    takes them: (overrides, error_m), ``error_m`` keyed by the ``df_R`` series name."""
    M = theta.shape[1]
    overrides = {nm: theta[d].copy() for d, nm in enumerate(names) if target[d] != abi.MCMC_TARGET_NONE}
    error_m = {abi.TQ_DERIVED_SERIES[abi.GOF_VARS.index(v)]:
               (theta[m_dim[abi.GOF_VARS.index(v)]].copy() if m_dim[abi.GOF_VARS.index(v)] >= 0
                else np.full(M, m_const[abi.GOF_VARS.index(v)])) for v in variables}
    return overrides, error_m


def _shaped_phi(phi, theta):
    """The lag-one coefficients at positions ``theta[n_dim, M]``, keyed like ``error_m``: one array [M] per variable that has a
    ``phi``, sampled or fixed; {} without any."""
    if phi is None:
        return {}
    phi_dim, phi_const, with_phi = phi
    M = theta.shape[1]
    at = lambda v: abi.GOF_VARS.index(v)
    return {abi.TQ_DERIVED_SERIES[at(v)]: (theta[phi_dim[at(v)]].copy() if phi_dim[at(v)] >= 0 else np.full(M, phi_const[at(v)]))
            for v in with_phi}


def start_ball(centre, priors, n_walkers, seed=0):
    """The notebook's start of a chain around a point estimate, ``param_est + 1e-4 randn``: ``centre + 1e-4 (hi - lo) z`` with
    ``z = predictive.standard_normal(seed, walker, dimension, 0, START_SERIES)``, as ``[n_dim, n_walkers]``.  ``centre``: one value
    per name of ``priors``, in its order -- ``find_map(...)['x'][:, best]``.  This is ``sample_posterior``'s own start for
    ``start=None``, around the workbook's values.  ``ValueError`` where a walker leaves the prior box."""
    if not isinstance(priors, dict) or not priors:
        raise ValueError("priors must be a dict name -> (lo, hi) with at least one entry")
    names = list(priors)
    lo, hi = _box(priors, names)
    centre = np.asarray(centre, dtype=np.float64)
    n_dim, W = len(names), int(n_walkers)
    if centre.shape != (n_dim,):
        raise ValueError("centre needs one value per name of priors: %d, got shape %s" % (n_dim, centre.shape))
    z = predictive.standard_normal(int(seed), np.arange(W)[None, :], np.arange(n_dim)[:, None], 0, START_SERIES)
    theta0 = centre[:, None] + (1e-4 * (hi - lo))[:, None] * z
    _check_inside(theta0, lo, hi, names)
    return theta0


def _check_inside(theta0, lo, hi, names):
    if not ((theta0 >= lo[:, None]) & (theta0 < hi[:, None])).all():
        d = int(np.argmin(((theta0 >= lo[:, None]) & (theta0 < hi[:, None])).all(axis=1)))
        raise ValueError("the start lies outside the prior box in %r" % names[d])


def sample_posterior(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, obs_dict, priors, variables=('Q',), error_m=None,
                     n_walkers=None, n_steps=0, start=None, seed=0, a=2.0, thin=1, state=None, record_proposals=False,
                     step_len=1., solver=None, device=0, out_reaches=None, error_phi=None):
    """Sample the posterior of model parameters with the affine-invariant stretch move (Goodman & Weare 2010; the reference's
    ``run_mcmc``), every half-step one ensemble run of ``n_walkers / 2`` members on the device.

    ``priors``: dict name -> (lo, hi), the flat prior box ``lo <= x < hi`` (the reference's ``log_prior``); names are member
    parameters (``marshal.PM_NAMES``), ``'f_TDP'``, and ``'m_<VAR>'`` -- the ``m`` of the error model ``sigma = m * sim`` --
    for ``VAR`` in ``variables`` (names of ``abi.GOF_VARS``: the observed series the likelihood is taken over, at every
    output reach that has more than 10 observations of it).  A variable whose ``m`` is not sampled gets it through
    ``error_m={'Q': 0.1}``.  ``'phi_<VAR>'`` samples the lag-one coefficient of an AR(1) error model for ``VAR``
    (``simplyp_amd.residuals``: the standardised residuals are autocorrelated along runs of consecutive observation days and
    independent across gaps; the box must lie inside (-1, 1) and the start is its centre), ``error_phi={'Q': 0.6}`` fixes it, and
    a variable with neither has independent errors.  With any ``phi`` an evaluation is ``Engine.gof`` -> ``Engine.gof_lag`` ->
    ``mcmc_log_prob_ar1``, ``stats`` gains ``lag_ms`` and the result's ``error_phi`` holds the last positions' coefficients,
    keyed like ``error_m``; with none the call does exactly what it did without the option.  Per-day predictive bands do not
    depend on ``phi`` (the per-day marginal of the standardised residual stays N(0, 1)), so ``predictive_series=`` takes no
    ``phi``.  ``n_walkers`` even and >= twice the number of names (at most 16); ``n_steps`` steps;
    ``a`` the stretch scale; ``seed`` the key of the counter-based random stream (``simplyp_amd.mcmc``); every ``thin``-th
    step is kept.  ``start``: None = the notebook's ball -- the workbook's values (box centres for the ``m``) plus
    ``1e-4 (hi - lo) z`` with ``z = predictive.standard_normal(seed, walker, dimension, 0, START_SERIES)``: ``start_ball`` -- or an array
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
    if not obs_dict:
        raise ValueError("sample_posterior needs obs_dict: the observations the likelihood is taken over")

    def check_shape(n_dim):
        if n_walkers is None:
            raise ValueError("n_walkers must be given")
        try:
            mcmc.check_shape(int(n_walkers), n_dim)
        except ValueError as exc:
            raise ValueError("sample_posterior: %s" % exc)

    names, variables, lo, hi, target, m_dim, m_const, phi = _plan(priors, variables, error_m, check_shape, error_phi)
    n_dim, W = len(names), int(n_walkers)
    h = W // 2
    if not float(a) > 1.0:
        raise ValueError("the stretch scale a must be > 1 (got %r)" % (a,))
    seed, thin, n_steps = int(seed), int(thin), int(n_steps)
    if not 0 <= seed < 1 << 64 or thin < 1 or n_steps < 0:
        raise ValueError("seed must be in [0, 2^64), thin >= 1 and n_steps >= 0")

    with marshal.reference_edits(p_SU, p_LU, p_SC, p):
        hs = _host_setup(met_df, p_struc, p_SU, p_LU, p_SC, p, obs_dict, names, variables, lo, hi, out_reaches)
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
                theta0 = start_ball(hs['centre'], priors, W, seed)
            else:
                theta0 = np.array(start, dtype=np.float64)
                if theta0.shape != (n_dim, W):
                    raise ValueError("start must have shape [n_dim, n_walkers] = %s, got %s" % ((n_dim, W), theta0.shape))
        _check_inside(theta0, lo, hi, names)
        if t0 + n_steps >= 1 << 32:
            raise ValueError("the absolute step index must stay below 2^32")

        # ---- the device: everything is marshalled and uploaded once, for an ensemble of h members
        ev = _Evaluator("sample_posterior keeps members in walker order", hs, met_df, p_SU, p_LU, p_SC, p, dynamic_options, step_len,
                        solver, device, h, n_dim, m_dim, m_const, phi)
        dev, prop_d, lpp_d, inside_d, evaluate = ev.dev, ev.prop_d, ev.lpp_d, ev.inside_d, ev.evaluate
        eng, torch, f64, mp_d, ft_d = dev.eng, dev.torch, dev.f64, dev.mp_d, dev.ft_d
        theta_d = eng.to_device(theta0, torch.float64)
        nacc_d = eng.to_device(nacc0, torch.int32)
        kept = [t for t in range(t0, t0 + n_steps) if (t + 1) % thin == 0]
        chain_d = torch.empty((len(kept), n_dim + 1, W), **f64)
        if record_proposals:
            props_d, plp_d = torch.empty((n_steps, n_dim, W), **f64), torch.empty((n_steps, W), **f64)
        stats = dict(wall_ms=[], run_kernel_ms=[], gof_ms=[], sampler_ms=[], n_inside=[], n_accepted=[],
                     start_wall_ms=[], start_run_kernel_ms=[])
        if phi is not None:
            stats['lag_ms'] = []

        if lp0 is None:                               # the start's log posterior: one evaluation per half, through the same kernels
            lp_d = torch.empty((W,), **f64)
            for k in (0, 1):
                sl = slice(k * h, (k + 1) * h)
                torch.cuda.synchronize(eng.tdev)
                w0 = time.perf_counter()
                prop_d.copy_(theta_d[:, sl])
                dev.write_positions(theta_d[:, sl], target)
                run_ms = evaluate()[0]
                lp_d[sl].copy_(lpp_d)
                torch.cuda.synchronize(eng.tdev)
                stats['start_wall_ms'].append(1e3 * (time.perf_counter() - w0))
                stats['start_run_kernel_ms'].append(run_ms)
            lp_host = lp_d.cpu().numpy()
            if not np.isfinite(lp_host).all():
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
                if phi is not None:
                    stats['lag_ms'].append(ev.lag_ms)
                stats['sampler_ms'].append(pinfo['kernel_ms'] + lp_ms + ainfo['kernel_ms'])
                stats['n_inside'].append(pinfo['n_inside'])
                stats['n_accepted'].append(ainfo['n_accepted'])
                if record_proposals:
                    props_d[n, :, k * h:(k + 1) * h].copy_(prop_d)
                    plp_d[n, k * h:(k + 1) * h].copy_(lpp_d)

    chain = chain_d.cpu().numpy()
    theta, lp, n_accept = theta_d.cpu().numpy(), lp_d.cpu().numpy(), nacc_d.cpu().numpy()
    t_end = t0 + n_steps
    overrides, err_m = _shaped_for_the_ensemble(names, target, variables, m_dim, m_const, theta)
    res = dict(names=names, chain=np.ascontiguousarray(chain[:, :n_dim]), log_prob=np.ascontiguousarray(chain[:, n_dim]),
               acceptance_fraction=n_accept / float(t_end) if t_end else np.zeros(W), n_steps=n_steps, seed=seed,
               overrides=overrides, error_m=err_m, error_phi=_shaped_phi(phi, theta),
               state=dict(theta=theta, lp=lp, n_accept=n_accept, t=t_end), start=dict(theta=theta0, lp=lp_start, t=t0), stats=stats)
    if record_proposals:
        res['proposals'], res['proposal_log_prob'] = props_d.cpu().numpy(), plp_d.cpu().numpy()
    return res


def find_map(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, obs_dict, priors, variables=('Q',), error_m=None,
             init_guess=None, n_starts=64, max_iter=None, xatol=1e-4, fatol=1e-4, seed=0, state=None, record_evaluations=False,
             step_len=1., solver=None, device=0, out_reaches=None, error_phi=None):
    """Find the mode of the posterior (the reference's ``find_map``: ``scipy.optimize.fmin`` on the negative log posterior) with
    ``n_starts`` Nelder-Mead simplexes at once, every run one ensemble of ``4 n_starts`` members on the device.

    ``priors``, ``variables``, ``error_m``, ``error_phi``, ``out_reaches`` and the checks are ``sample_posterior``'s: the names are
    member parameters, ``'f_TDP'``, ``'m_<VAR>'`` and ``'phi_<VAR>'``; the box is ``lo <= x < hi``, outside of which the target is +inf and the model is
    never run.  The algorithm is scipy's, its coefficients, decisions and termination (``xatol``, ``fatol``; ``max_iter`` counts
    like scipy's ``maxiter`` and defaults to its ``200 n_dim``), with an iteration's four candidates evaluated together
    (``simplyp_amd.neldermead``).  ``init_guess``: an array [n_dim, n_starts] inside the box, or None: simplex 0 starts at the
    workbook's values (box centres for the ``m``) and simplex ``s >= 1`` at ``lo + (hi - lo) u`` with ``u`` the uniform of Philox
    counter ``(s, dimension, 0, neldermead.START_STREAM)`` under key ``seed`` (``neldermead.uniform_starts``).  Every initial
    simplex is scipy's (``neldermead.initial_simplex``: a vertex that would leave the box steps inwards instead).  ``4 n_starts``
    must be at least the number of names.  ``state``: the ``'state'`` of an earlier result, typically with a higher ``max_iter``:
    the search continues from it bit for bit (``init_guess`` is ignored).

    The inputs are marshalled and uploaded once; one run is ``nm_propose`` -> ``Engine.run`` -> ``Engine.gof`` ->
    ``mcmc_log_prob`` -> ``nm_update`` on device buffers, until no simplex is active.  Returns dict(names, x[n_dim, S] -- the best
    vertex of every simplex --, fun[S] = -log posterior there, best -- the index of the lowest ``fun`` --, map -- name -> value
    at ``best`` --, overrides, error_m -- the best point shaped for ``run_simply_p_ensemble(overrides=,
    predictive_series=list(error_m), predictive_m=error_m)``: arrays of one member --, n_iter[S] and status[S] as scipy reports
    them (0 converged, 2 at the limit), history[max_iter, S] -- the best value after every iteration, row 0 the initial simplex,
    NaN where a simplex had stopped --, final_simplex = (sim[n_dim + 1, n_dim, S], fsim[n_dim + 1, S]), moves -- dict kind ->
    [S] counts --, state, start -- the state this call began from --, evaluations[n_runs, n_dim, 4 S] and evaluation_log_prob[n_runs, 4 S] with ``record_evaluations``,
    stats = per-run lists of wall_ms, run_kernel_ms, gof_ms, optimiser_ms, n_active, n_shrinking -- the simplexes that
    were moving and re-evaluating a shrunk simplex in that run --).  ``ValueError`` for what
    ``sample_posterior`` rejects, an ``init_guess`` outside the box or of the wrong shape, and a start whose log posterior is not
    finite (it names the simplex).  The caller's ``p_LU`` / ``p_SC`` are edited in place exactly as by ``run_simply_p``."""
    if not obs_dict:
        raise ValueError("find_map needs obs_dict: the observations the likelihood is taken over")
    S = int(n_starts) if state is None else int(np.asarray(state['sim']).shape[-1])

    def check_shape(n_dim):
        if not 1 <= n_dim <= neldermead.MAX_DIM:
            raise ValueError("find_map: n_dim must be in [1, %d] (got %d)" % (neldermead.MAX_DIM, n_dim))
        if S < 1 or 4 * S < n_dim:
            raise ValueError("find_map: n_starts must be >= 1 and 4 n_starts >= n_dim (got %d starts, n_dim = %d)" % (S, n_dim))

    names, variables, lo, hi, target, m_dim, m_const, phi = _plan(priors, variables, error_m, check_shape, error_phi)
    n_dim = len(names)
    seed = int(seed)
    max_iter = 200 * n_dim if max_iter is None else int(max_iter)
    if not 0 <= seed < 1 << 64 or max_iter < 1 or not float(xatol) >= 0.0 or not float(fatol) >= 0.0:
        raise ValueError("seed must be in [0, 2^64), max_iter >= 1, xatol and fatol >= 0")

    with marshal.reference_edits(p_SU, p_LU, p_SC, p):
        hs = _host_setup(met_df, p_struc, p_SU, p_LU, p_SC, p, obs_dict, names, variables, lo, hi, out_reaches)
        if state is not None:
            st = neldermead.copy_state({k: state[k] for k in ('sim', 'fsim', 'phase', 'cursor', 'n_iter', 'status', 'counts')})
            if st['sim'].shape != (n_dim + 1, n_dim, S) or st['fsim'].shape != (n_dim + 1, S):
                raise ValueError("state does not match this call: sim %s for %d names" % (st['sim'].shape, n_dim))
            neldermead.resume(st, max_iter, xatol, fatol)
            hist0 = np.asarray(state['history'], dtype=np.float64)
        else:
            if init_guess is None:
                x0 = neldermead.uniform_starts(seed, n_dim, S, lo, hi)
                x0[:, 0] = hs['centre']
            else:
                x0 = np.array(init_guess, dtype=np.float64)
                if x0.shape != (n_dim, S):
                    raise ValueError("init_guess must have shape [n_dim, n_starts] = %s, got %s" % ((n_dim, S), x0.shape))
            st = neldermead.new_state(neldermead.initial_simplex(x0, lo, hi))
            hist0 = np.empty((0, S))
        hist = np.full((max_iter, S), np.nan)
        hist[:min(len(hist0), max_iter)] = hist0[:max_iter]
        begin = dict(neldermead.copy_state(st), history=hist.copy())

        # ---- the device: everything is marshalled and uploaded once, for an ensemble of 4 S members
        ev = _Evaluator("find_map keeps members in slot order", hs, met_df, p_SU, p_LU, p_SC, p, dynamic_options, step_len, solver,
                        device, neldermead.SLOTS * S, n_dim, m_dim, m_const, phi)
        eng, torch = ev.dev.eng, ev.dev.torch
        sim_d, fsim_d = eng.to_device(st['sim'], torch.float64), eng.to_device(st['fsim'], torch.float64)
        ist_d = eng.to_device(neldermead.pack_istate(st), torch.int32)
        hist_d = eng.to_device(hist, torch.float64)
        stats = dict(wall_ms=[], run_kernel_ms=[], gof_ms=[], optimiser_ms=[], n_active=[], n_shrinking=[])
        if phi is not None:
            stats['lag_ms'] = []
        evals, evals_lp = [], []
        n_active = int((st['phase'] != neldermead.DONE).sum())
        while n_active:
            torch.cuda.synchronize(eng.tdev)
            w0 = time.perf_counter()
            pinfo = eng.nm_propose(sim_d, ist_d, lo, hi, target, ev.prop_d, ev.inside_d, ev.dev.mp_d, ev.dev.ft_d)
            run_ms, gof_ms, lp_ms = ev.evaluate()
            uinfo = eng.nm_update(sim_d, fsim_d, ist_d, ev.prop_d, ev.inside_d, ev.lpp_d, max_iter, xatol, fatol, history=hist_d)
            stats['wall_ms'].append(1e3 * (time.perf_counter() - w0))
            stats['run_kernel_ms'].append(run_ms)
            stats['gof_ms'].append(gof_ms)
            if phi is not None:
                stats['lag_ms'].append(ev.lag_ms)
            stats['optimiser_ms'].append(pinfo['kernel_ms'] + lp_ms + uinfo['kernel_ms'])
            stats['n_active'].append(pinfo['n_active'])
            stats['n_shrinking'].append(pinfo['n_shrinking'])
            if record_evaluations:
                evals.append(ev.prop_d.clone())
                evals_lp.append(ev.lpp_d.clone())
            if uinfo['n_nonfinite_start']:
                bad = int(np.argmax(ist_d[abi.NM_ISTATE.index('status')].cpu().numpy() == neldermead.NONFINITE_START))
                raise ValueError("the start of simplex %d has a vertex with a non-finite log posterior: the model or the likelihood "
                                 "fails there" % bad)
            n_active = uinfo['n_active']

    st['sim'], st['fsim'] = sim_d.cpu().numpy(), fsim_d.cpu().numpy()
    neldermead.unpack_istate(ist_d.cpu().numpy(), st)
    hist = hist_d.cpu().numpy()
    x, fun = st['sim'][0].copy(), st['fsim'][0].copy()
    best = int(np.argmin(fun))
    overrides, err_m = _shaped_for_the_ensemble(names, target, variables, m_dim, m_const, x[:, best:best + 1])
    res = dict(names=names, x=x, fun=fun, best=best, map={nm: float(x[d, best]) for d, nm in enumerate(names)},
               overrides=overrides, error_m=err_m, error_phi=_shaped_phi(phi, x[:, best:best + 1]), n_iter=st['n_iter'].copy(), status=st['status'].copy(), history=hist,
               final_simplex=(st['sim'], st['fsim']), moves={m: st['counts'][i].copy() for i, m in enumerate(neldermead.MOVES)},
               state=dict(st, history=hist), start=begin, stats=stats)
    if record_evaluations:
        res['evaluations'] = torch.stack(evals).cpu().numpy() if evals else np.empty((0, n_dim, neldermead.SLOTS * S))
        res['evaluation_log_prob'] = torch.stack(evals_lp).cpu().numpy() if evals_lp else np.empty((0, neldermead.SLOTS * S))
    return res


def _pareto_plan(priors, objectives, n_pop, n_gen, seed, eta_c, eta_m, p_cross, p_mut, n_reaches=1 << 30):
    """Names, box, targets, objectives and operator settings of ``find_pareto``; host only, raises ValueError."""
    if not isinstance(priors, dict) or not priors:
        raise ValueError("priors must be a dict name -> (lo, hi) with at least one entry")
    names = list(priors)
    target = []
    for nm in names:
        if nm.startswith('m_') or nm.startswith('phi_'):
            raise ValueError("find_pareto takes no error-model parameter (%r): no likelihood is involved" % nm)
        if _priors.target_of(nm) is None:
            raise ValueError("unknown parameter %r: searched names are %s and 'f_TDP'" % (nm, marshal.PM_NAMES))
        target.append(_priors.target_of(nm))
    if n_pop is None:
        raise ValueError("n_pop must be given")
    try:
        objectives = [tuple(o) for o in objectives]
    except TypeError:
        raise ValueError("objectives must be a list of (stat, variable[, reach_index[, sense]])")
    if any(len(o) and o[0] == 'spearman' for o in objectives):
        raise ValueError("find_pareto takes no 'spearman' objective in this version")
    resolved = pareto.resolve_objectives(objectives, n_reaches=n_reaches)
    try:
        nsga2.check_shape(int(n_pop), len(names), len(resolved))
    except ValueError as exc:
        raise ValueError("find_pareto: %s" % exc)
    k_c, k_m = nsga2.k_of_eta(eta_c, 'eta_c'), nsga2.k_of_eta(eta_m, 'eta_m')
    p_cross = nsga2.check_probability(p_cross, 'p_cross')
    p_mut = nsga2.check_probability(1.0 / len(names) if p_mut is None else p_mut, 'p_mut')
    if not 0 <= int(seed) < 1 << 64 or int(n_gen) < 0:
        raise ValueError("seed must be in [0, 2^64) and n_gen >= 0")
    lo, hi = _box(priors, names)
    return names, lo, hi, np.array(target, dtype=np.int32), resolved, k_c, k_m, p_cross, p_mut


def find_pareto(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, obs_dict, priors, objectives, n_pop=None, n_gen=0,
                start=None, seed=0, eta_c=15, eta_m=15, p_cross=0.9, p_mut=None, state=None, record_children=False,
                step_len=1., solver=None, device=0, out_reaches=None):
    """Move a population towards the Pareto front of several goodness-of-fit criteria with NSGA-II (Deb et al. 2002), every
    generation one ensemble run of ``n_pop`` members on the device.

    ``priors``: dict name -> (lo, hi), the closed box ``lo <= x <= hi`` of member parameters (``marshal.PM_NAMES``) and
    ``'f_TDP'``, at most 16; ``'m_<VAR>'`` / ``'phi_<VAR>'`` are refused: no likelihood is involved.  ``objectives``: as for
    ``pareto_ranks`` (``pareto.resolve_objectives``: NSE, log NSE and r2 are maximised, nRMSD (%) is minimised, Bias (%) is
    minimised in absolute value, a fourth element gives the sense), 1 to 8 of them, each at an output reach with more than 10
    observations of its variable; ``'spearman'`` is refused in this version.  ``n_pop`` even, in [4, 65536]; ``n_gen``
    generations after the initial population's; ``eta_c`` / ``eta_m``: the distribution indices of the crossover and the
    mutation, one of 1, 3, 7, 15, 31; ``p_cross``; ``p_mut`` (None: ``1 / n_dim``); ``seed`` the key of the counter-based
    stream.  ``start``: None = ``lo + (hi - lo) u`` drawn on the device, or an array [n_dim, n_pop] inside the box.
    ``state``: the ``'state'`` of an earlier result: the search continues at its generation count, bit for bit (``start`` is
    ignored).  ``simplyp_amd.nsga2`` states the whole rule.

    The inputs are marshalled and uploaded once; a generation is ``nsga2_offspring`` -> ``Engine.run`` -> ``Engine.gof`` -> the
    objective rows -> ``Engine.pareto`` on the 2 ``n_pop`` parents and children, a member with a non-finite objective or a
    non-finite run left out -> ``nsga2_crowding`` -> ``nsga2_select``, all on device buffers.  Returns dict(names, x[n_dim, n_pop]
    sorted best first, objectives[M, n_pop] -- the statistics as the goodness-of-fit table has them: a bias keeps its sign --,
    labels, sense, absolute -- which objectives are ranked by their absolute value --, rank[n_pop], crowding[n_pop], front -- the
    indices of rank 0 --, overrides -- ``x`` shaped for ``run_simply_p_ensemble(overrides=)`` --, history = dict(n_front0,
    n_fronts, n_invalid: one entry per evaluated generation, counted in the set that was ranked; best[n, M]: the best value of
    every objective as it is ranked among the survivors), with ``record_children`` children[n, n_dim, n_pop],
    children_objectives[n, M, n_pop], children_valid[n, n_pop] and survivors[n, n_pop], ranks[n, n_pop], crowdings[n, n_pop]
    after every evaluated generation (the initial population is the first "children" of a search that starts here),
    state = dict(theta, objectives, rank, crowd, t), seed, stats = per-generation lists of wall_ms, run_kernel_ms, gof_ms,
    pareto_ms, crowding_ms, select_ms, offspring_ms).  Every ``ValueError`` comes before any device call.  The caller's
    ``p_LU`` / ``p_SC`` are edited in place exactly as by ``run_simply_p``."""
    if not obs_dict:
        raise ValueError("find_pareto needs obs_dict: the observations the criteria are taken over")
    names, lo, hi, target, resolved, k_c, k_m, p_cross, p_mut = _pareto_plan(priors, objectives, n_pop, n_gen, seed, eta_c, eta_m,
                                                                             p_cross, p_mut)
    n_dim, N, M, n_gen, seed = len(names), int(n_pop), len(resolved), int(n_gen), int(seed)
    variables = list(dict.fromkeys(r['variable'] for r in resolved))

    with marshal.reference_edits(p_SU, p_LU, p_SC, p):
        hs = _host_setup(met_df, p_struc, p_SU, p_LU, p_SC, p, obs_dict, names, variables, lo, hi, out_reaches)
        resolved = pareto.resolve_objectives(objectives, n_reaches=len(hs['reaches']))
        n_obs = (~np.isnan(hs['obs'])).sum(axis=-1)
        for r in resolved:
            if n_obs[r['reach'], r['var_index']] <= 10:
                raise ValueError("objective %s: 10 or fewer observations of %r at that output reach: its statistics are NaN"
                                 % (r['label'], r['variable']))
        sense = [r['sense'] for r in resolved]
        absolute = np.array([r['absolute'] for r in resolved], dtype=bool)
        raw = [dict(r, absolute=False) for r in resolved]
        inside = lambda x: bool(((x >= lo[:, None]) & (x <= hi[:, None])).all())
        if state is not None:
            st0 = dict(theta=np.array(state['theta'], dtype=np.float64), objectives=np.array(state['objectives'], dtype=np.float64),
                       rank=np.array(state['rank'], dtype=np.int32), crowd=np.array(state['crowd'], dtype=np.float64))
            t0 = int(state['t'])
            if st0['theta'].shape != (n_dim, N) or st0['objectives'].shape != (M, N) or st0['rank'].shape != (N,) \
                    or st0['crowd'].shape != (N,) or t0 < 0:
                raise ValueError("state does not match this call: theta %s for %d names and %d members" % (st0['theta'].shape, n_dim, N))
            if not inside(st0['theta']):
                raise ValueError("the state lies outside the box")
        else:
            t0 = 0
            if start is not None:
                start = np.array(start, dtype=np.float64)
                if start.shape != (n_dim, N):
                    raise ValueError("start must have shape [n_dim, n_pop] = %s, got %s" % ((n_dim, N), start.shape))
                if not inside(start):
                    d = int(np.argmin(((start >= lo[:, None]) & (start <= hi[:, None])).all(axis=1)))
                    raise ValueError("the start lies outside the box in %r" % names[d])
        if t0 + n_gen >= 1 << 32:
            raise ValueError("the absolute generation count must stay below 2^32")

        # ---- the device: everything is marshalled and uploaded once, for an ensemble of n_pop members
        ev = _Evaluator("find_pareto keeps members in population order", hs, met_df, p_SU, p_LU, p_SC, p, dynamic_options, step_len,
                        solver, device, N, n_dim, None, None)
        dev = ev.dev
        eng, torch, f64 = dev.eng, dev.torch, dev.f64
        child_d = ev.prop_d                                              # [n_dim, N]
        par_d = torch.empty((2, N), dtype=torch.int32, device=eng.tdev) if record_children else None
        abs_d = torch.from_numpy(absolute).to(eng.tdev)
        sense_d = torch.tensor([float(s) for s in sense], **f64)[:, None]
        stats = {k: [] for k in ('wall_ms', 'run_kernel_ms', 'gof_ms', 'pareto_ms', 'crowding_ms', 'select_ms', 'offspring_ms')}
        hist = dict(n_front0=[], n_fronts=[], n_invalid=[])
        best, rec = [], {k: [] for k in ('children', 'children_objectives', 'children_valid', 'survivors', 'ranks', 'crowdings')}

        def ranked(rows):
            return torch.where(abs_d[:, None], rows.abs(), rows)

        def generation(theta_d, obj_d, rank_d, off_ms):
            """The children in ``child_d`` (their run points are in place) evaluated and the set of parents (None: generation 0)
            and children reduced to N survivors: (theta, objectives, rank, crowd) on the device, sorted best first."""
            status_d, rstats, ginfo = ev.run_gof()
            cobj = pareto.objective_rows(ev.gof_d, None, raw)
            valid = torch.isfinite(cobj).all(dim=0) & ((status_d & abi.STATUS_NONFINITE) == 0)
            if theta_d is None:
                pool, include = torch.cat([child_d, cobj]), valid
            else:
                pool = torch.cat([torch.cat([theta_d, child_d], dim=1), torch.cat([obj_d, cobj], dim=1)])
                include = torch.cat([rank_d >= 0, valid])
            robj = ranked(pool[n_dim:]).contiguous()
            pr = eng.pareto(robj, sense, include=include, counts=False)
            crowd_all, cinfo = eng.nsga2_crowding(robj, sense, pr['rank'])
            sel = eng.nsga2_select(N, pr['rank'], crowd_all, rows=pool.contiguous())
            new_theta, new_obj = sel['rows'][:n_dim].contiguous(), sel['rows'][n_dim:].contiguous()
            hist['n_front0'].append(int(pr['n_front0']))
            hist['n_fronts'].append(int(pr['n_fronts']))
            hist['n_invalid'].append(int(pool.shape[1]) - int(pr['n_used']))
            y = torch.where((sel['rank'] >= 0)[None, :], ranked(new_obj) * sense_d, torch.full_like(new_obj, -float('inf')))
            best.append(y.max(dim=1).values * sense_d[:, 0])
            if record_children:
                for k, v in (('children', child_d), ('children_objectives', cobj), ('children_valid', valid),
                             ('survivors', sel['survivor']), ('ranks', sel['rank']), ('crowdings', sel['crowd'])):
                    rec[k].append(v.clone())
            for k, v in (('run_kernel_ms', rstats['kernel_ms']), ('gof_ms', ginfo['kernel_ms']), ('pareto_ms', pr['kernel_ms']),
                         ('crowding_ms', cinfo['kernel_ms']), ('select_ms', sel['kernel_ms']), ('offspring_ms', off_ms)):
                stats[k].append(v)
            return new_theta, new_obj, sel['rank'], sel['crowd']

        if state is None:
            torch.cuda.synchronize(eng.tdev)
            w0 = time.perf_counter()
            if start is None:
                off_ms = eng.nsga2_init(child_d, lo, hi, target, dev.mp_d, dev.ft_d, seed=seed)['kernel_ms']
            else:
                child_d.copy_(eng.to_device(start, torch.float64))
                dev.write_positions(child_d, target)
                off_ms = 0.0
            theta_d, obj_d, rank_d, crowd_d = generation(None, None, None, off_ms)
            torch.cuda.synchronize(eng.tdev)
            stats['wall_ms'].append(1e3 * (time.perf_counter() - w0))
        else:
            theta_d, obj_d = eng.to_device(st0['theta'], torch.float64), eng.to_device(st0['objectives'], torch.float64)
            rank_d, crowd_d = eng.to_device(st0['rank'], torch.int32), eng.to_device(st0['crowd'], torch.float64)
        for t in range(t0 + 1, t0 + n_gen + 1):
            torch.cuda.synchronize(eng.tdev)
            w0 = time.perf_counter()
            oinfo = eng.nsga2_offspring(theta_d, rank_d, crowd_d, t, lo, hi, target, child_d, parents=par_d, member_params=dev.mp_d,
                                        f_tdp=dev.ft_d, k_c=k_c, k_m=k_m, p_cross=p_cross, p_mut=p_mut, seed=seed)
            theta_d, obj_d, rank_d, crowd_d = generation(theta_d, obj_d, rank_d, oinfo['kernel_ms'])
            torch.cuda.synchronize(eng.tdev)
            stats['wall_ms'].append(1e3 * (time.perf_counter() - w0))

    x, obj = theta_d.cpu().numpy(), obj_d.cpu().numpy()
    rank, crowd = rank_d.cpu().numpy(), crowd_d.cpu().numpy()
    hist['best'] = torch.stack(best).cpu().numpy() if best else np.empty((0, M))
    res = dict(names=names, x=x, objectives=obj, labels=[r['label'] for r in resolved], sense=sense, absolute=absolute, rank=rank,
               crowding=crowd, front=np.flatnonzero(rank == 0), overrides={nm: x[d].copy() for d, nm in enumerate(names)},
               history=hist, seed=seed, state=dict(theta=x.copy(), objectives=obj.copy(), rank=rank.copy(), crowd=crowd.copy(), t=t0 + n_gen),
               stats=stats)
    if record_children:
        shapes = dict(children=(0, n_dim, N), children_objectives=(0, M, N), children_valid=(0, N), survivors=(0, N), ranks=(0, N),
                      crowdings=(0, N))
        for k, v in rec.items():
            res[k] = torch.stack(v).cpu().numpy() if v else np.empty(shapes[k])
    return res
