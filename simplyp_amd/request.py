"""The host-only rules the public calls share, each stated once.  Nothing here touches the device (neither torch nor ``engine``
is imported); every function raises ``ValueError``, worded for the argument ``what``."""

import numpy as np

from . import abi, marshal


def probabilities(what, values):
    """``values`` (a scalar or a sequence) as a list of 1 to 16 floats in [0, 1]."""
    q = [float(x) for x in np.atleast_1d(np.asarray(values, dtype=np.float64))]
    if not 1 <= len(q) <= 16 or not all(0.0 <= x <= 1.0 for x in q):
        raise ValueError("%s must be 1 to 16 probabilities in [0, 1]" % what)
    return q


def series_ids(what, names, among=None, columns=marshal.ALL_COLUMNS):
    """(names, ids, needs) of 1 to 32 series (a bare string is one): a ``df_R`` name gets ``abi.TQ_DERIVED`` + its index, a table
    column of ``columns`` its own (``among`` words another choice); ``needs``: the outputs they add, fluxes first, then the named columns."""
    names = [names] if isinstance(names, str) else list(names)
    unknown = [c for c in names if c not in columns and c not in abi.TQ_DERIVED_SERIES]
    if unknown or not 1 <= len(names) <= 32:
        among = among or "the reference's columns and %s" % (abi.TQ_DERIVED_SERIES,)
        raise ValueError("%s must be 1 to 32 names among %s (unknown: %s)" % (what, among, unknown))
    ids = [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index(c) if c in abi.TQ_DERIVED_SERIES else marshal.ALL_COLUMNS.index(c) for c in names]
    flux = marshal.FLUX_COLUMNS if any(i >= abi.TQ_DERIVED for i in ids) else []
    return names, ids, flux + [c for c in names if c in marshal.ALL_COLUMNS and c not in flux]


def annual_periods(index):
    """(years, period_of_day int32 [D]): one period per calendar year of the dates ``index``."""
    years, pod = np.unique(np.asarray(index.year), return_inverse=True)
    return years, np.ascontiguousarray(pod, dtype=np.int32)


def reduce_periods(reduce, index, total=False):
    """(periods, period_of_day int32 [D]) of ``reduce``: ``'annual'``, ``'total'`` where allowed, or a period index >= 0 per day."""
    if isinstance(reduce, str):
        if reduce == 'annual':
            return annual_periods(index)
        if total and reduce == 'total':
            return np.arange(1), np.zeros(len(index), dtype=np.int32)
        raise ValueError("reduce must be %s or an array of period indices" % ("'annual', 'total'" if total else "None, 'annual'"))
    pod = np.asarray(reduce)
    if pod.shape != (len(index),) or pod.min() < 0:
        raise ValueError("reduce array needs one non-negative period index per day")
    return np.arange(int(pod.max()) + 1), np.ascontiguousarray(pod, dtype=np.int32)


def skipping_periods(what, spec):
    """(labels, period_of_day int32) of an int array whose -1 marks a day outside every period and whose other entries do not
    decrease; (None, None) for None and ``'annual'``, which ``annual_periods`` resolves once the dates are known."""
    wrong = "%s must be None, 'annual' or an int array [D] of period indices >= -1" % what
    if spec is None or isinstance(spec, str):
        if spec not in (None, 'annual'):
            raise ValueError(wrong)
        return None, None
    pod = np.asarray(spec)
    if pod.ndim != 1 or pod.dtype.kind not in 'iu' or (pod < -1).any():
        raise ValueError(wrong)
    named = pod[pod >= 0]
    if (np.diff(named) < 0).any():
        raise ValueError("%s must not decrease (apart from -1 = no period)" % what)
    return np.arange(int(named.max()) + 1 if len(named) else 1), np.ascontiguousarray(pod, dtype=np.int32)


def observed_series(obs_dict, reaches, obs, among=None):
    """(names, ids, obs[n_series, D, n_reaches]) of the scored series: the ``df_R`` names (of ``among``, when given) with an
    observation, on any date, at some reach of ``reaches``; cut from ``obs[n_reaches, 6, D]``.  Nothing observed: ([], None, None)."""
    seen = {var for SC in reaches if SC in obs_dict for var in abi.GOF_VARS
            if var in obs_dict[SC].columns and obs_dict[SC][var].notna().any()}
    at = [i for i, (c, var) in enumerate(zip(abi.TQ_DERIVED_SERIES, abi.GOF_VARS)) if var in seen and (among is None or c in among)]
    if not at:
        return [], None, None
    return [abi.TQ_DERIVED_SERIES[i] for i in at], [abi.TQ_DERIVED + i for i in at], \
        np.ascontiguousarray(np.stack([obs[:, i, :].T for i in at]))


def error_model_rows(predictive_m, names, E):
    """``predictive_m`` -- a float, an array [E], or a dict name -> either (a name it lacks gets 0) -- as [n_series, E]."""
    per = predictive_m if isinstance(predictive_m, dict) else {c: predictive_m for c in names}
    try:
        rows = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(per.get(c, 0.0), dtype=np.float64), (E,)) for c in names]))
    except (TypeError, ValueError):
        raise ValueError("predictive_m must be a float, an array [E], or a dict name -> float or array [E]")
    if not (np.isfinite(rows).all() and (rows >= 0).all()):
        raise ValueError("predictive_m must be finite and >= 0")
    return rows
