"""What the calls that move points inside a prior box share on the host (``calibrate.sample_posterior``, ``calibrate.find_map``,
``sensitivity.sobol_indices``): the box of a ``priors`` dict, where a name goes in the run's arrays, the reference's input checks
at the box's corners, and the snow rule.  Host only; everything raises ``ValueError``."""

import numpy as np

from . import abi, marshal


def box(priors, names):
    """The prior box of ``names`` as (lo, hi); raises ValueError."""
    try:
        b = np.array([[float(priors[nm][0]), float(priors[nm][1])] for nm in names], dtype=np.float64)
    except (TypeError, ValueError, IndexError):
        raise ValueError("priors must map each name to a pair (lo, hi)")
    if not (b[:, 0] < b[:, 1]).all():
        bad = names[int(np.argmin(b[:, 0] < b[:, 1]))]
        raise ValueError("prior of %r needs lo < hi (got %s)" % (bad, tuple(priors[bad])))
    return b[:, 0].copy(), b[:, 1].copy()


def target_of(name):
    """Where a dimension called ``name`` goes: a row of ``member_params``, ``abi.MCMC_TARGET_F_TDP``, or None for a name that
    is neither a member parameter nor ``'f_TDP'``."""
    if name in marshal.PM_NAMES:
        return marshal.PM_NAMES.index(name)
    if name == 'f_TDP':
        return abi.MCMC_TARGET_F_TDP
    return None


def check_corners(names, lo, hi, p, p_LU, p_SC, scs):
    """The reference's input checks at the box's two extreme corners (the checks are per parameter)."""
    pm = [(d, nm) for d, nm in enumerate(names) if nm in marshal.PM_NAMES]
    if pm:
        corners = marshal.member_params(p, p_LU, 2, {nm: np.array([lo[d], hi[d]]) for d, nm in pm})
        try:
            marshal.validate_ensemble(corners, marshal.reach_params(p_SC, p, 2), scs)
        except AssertionError as exc:
            raise ValueError("the prior box holds points the model rejects: %s" % exc)


def snow_rule(names, met_df):
    """True when a name makes the snow module run in the kernel, which needs the raw forcing columns."""
    snow = 'f_DDSM' in names or 'D_snow_0' in names
    if snow and not {'Precipitation', 'T_air'} <= set(met_df.columns):
        raise ValueError("sampling f_DDSM / D_snow_0 runs the snow module in the kernel: met_df needs 'Precipitation' and 'T_air'")
    return snow
