"""Forcing uncertainty: the error model of the members' own rainfall, PET and air temperature, stated once.  NumPy, CPU only
(neither torch nor ``engine`` is imported); csrc/simplyp_forcing.hip.h is the device's copy of it.

For member ``e``, forcing row ``r`` (``abi.FORCING_ROWS``: 0 = P, or Precipitation with the in-kernel snow module; 1 = PET;
2 = T_air, present only with that module) and day ``d`` whose group id is ``g = groups[r][d]``::

    z      = predictive.standard_normal(seed, member0 + e, g, r, abi.FORCING_STREAM)
    P'     = (P   * scale_P[e])   * exp(sigma_P   * z - 0.5 * sigma_P   * sigma_P)        mean-one lognormal multiplier
    PET'   = (PET * scale_PET[e]) * exp(sigma_PET * z - 0.5 * sigma_PET * sigma_PET)
    T_air' = (T_air + offset_T[e]) + sigma_T * z

in this order of operations, no fused multiply-add.  ``sigma == 0`` for a row: no draw, the row is ``base * scale`` (``base +
offset``) only; with no scale or offset given either, the base value passes through bit for bit.  A dry day stays exactly 0.  A
draw depends on (seed, member id, group id, row) and on nothing else -- not on the launch shape, the lane slot, the balancing,
the time chunks, the window or the device block.  The days of one group share one draw per member and row; group ids are
absolute integers in [0, 2^31), made from the calendar so that a window of a run sees the ids the whole run sees.  No noise state
is carried from run to run, so autocorrelated errors are not offered.

The public calls take ``forcing_error`` as a dict of dicts (``resolve``); ``Engine.run`` takes what ``resolve`` returns.
"""

import numpy as np

from . import abi, predictive

SIGMA_MAX = 2.0
_ROW_KEYS = [('sigma', 'groups', 'scale'), ('sigma', 'groups', 'scale'), ('sigma', 'groups', 'offset')]
_ORDINAL_1970 = 719163                       # date(1970, 1, 1).toordinal()


def calendar_groups(index, kind):
    """Absolute group ids int64 [D] of the dates ``index``: ``'day'`` = the date's proleptic Gregorian ordinal, ``'month'`` =
    year * 12 + month - 1, ``'year'`` = the year."""
    if kind == 'day':
        return np.asarray(index.values.astype('datetime64[D]').astype(np.int64) + _ORDINAL_1970, dtype=np.int64)
    if kind == 'month':
        return np.asarray(index.year, dtype=np.int64) * 12 + np.asarray(index.month, dtype=np.int64) - 1
    if kind == 'year':
        return np.asarray(index.year, dtype=np.int64)
    raise ValueError("forcing_error groups must be 'day', 'month', 'year' or an int array with one group id per day (got %r)" % (kind,))


def _groups(what, spec, index):
    if isinstance(spec, str):
        g = calendar_groups(index, spec)
    else:
        g = np.asarray(spec)
        if g.dtype.kind not in 'iu' or g.shape != (len(index),):
            raise ValueError("%s must be 'day', 'month', 'year' or an int array with one group id per day [%d] (got %s %s)"
                             % (what, len(index), g.dtype, g.shape))
    if len(g) and (int(g.min()) < 0 or int(g.max()) >= 1 << 31):
        raise ValueError("%s: group ids must lie in [0, 2^31)" % what)
    return np.ascontiguousarray(g, dtype=np.int32)


def resolve(forcing_error, index, E, snow, seed=0, member0=0):
    """The public ``forcing_error`` -- ``{'P': {'sigma':, 'groups':, 'scale':}, 'PET': {...}, 'T_air': {'sigma':, 'groups':,
    'offset':}}``, every key optional, ``groups`` = ``'day'`` (default) | ``'month'`` | ``'year'`` | int array [D], ``scale`` /
    ``offset`` a float or an array [E] -- as what ``Engine.run`` and ``table`` take: dict(sigma float64 [3], groups [3 x (int32
    [D] or None)], shift (float64 [2 or 3, E]: P scale, PET scale(, T_air offset); None when none is given), seed, member0).
    None for None.  ``ValueError`` for an unknown key, a sigma that is not finite or outside [0, 2], an array of the wrong length,
    group ids outside [0, 2^31), ``'T_air'`` without the in-kernel snow module, a seed outside [0, 2^64)."""
    if forcing_error is None:
        return None
    if not isinstance(forcing_error, dict):
        raise ValueError("forcing_error must be a dict with keys among %s" % (abi.FORCING_ROWS,))
    unknown = [k for k in forcing_error if k not in abi.FORCING_ROWS]
    if unknown:
        raise ValueError("forcing_error: unknown keys %s (known: %s)" % (unknown, abi.FORCING_ROWS))
    if 'T_air' in forcing_error and not snow:
        raise ValueError("forcing_error['T_air'] needs the in-kernel snow module (snow_in_kernel=True): without it T_air is no "
                         "forcing row of the run")
    seed, member0, E, D = int(seed), int(member0), int(E), len(index)
    if not 0 <= seed < 1 << 64:
        raise ValueError("forcing_seed must be in [0, 2^64)")
    if not 0 <= member0 or member0 + E > 1 << 32:
        raise ValueError("forcing member ids must stay below 2^32")
    sigma, groups, shift = np.zeros(3), [None] * 3, [None] * 3
    for r, name in enumerate(abi.FORCING_ROWS):
        row = forcing_error.get(name)
        if row is None:
            continue
        what = "forcing_error[%r]" % name
        if not isinstance(row, dict) or [k for k in row if k not in _ROW_KEYS[r]]:
            raise ValueError("%s must be a dict with keys among %s" % (what, _ROW_KEYS[r]))
        try:
            sigma[r] = float(row.get('sigma', 0.0))
        except (TypeError, ValueError):
            raise ValueError("%s['sigma'] must be a number" % what)
        if not (np.isfinite(sigma[r]) and 0.0 <= sigma[r] <= SIGMA_MAX):
            raise ValueError("%s['sigma'] must be finite and in [0, %g] (got %r)" % (what, SIGMA_MAX, row.get('sigma')))
        g = _groups("%s['groups']" % what, row.get('groups', 'day'), index)
        groups[r] = g if sigma[r] > 0.0 else None
        key = _ROW_KEYS[r][2]
        if row.get(key) is not None:
            try:
                shift[r] = np.ascontiguousarray(np.broadcast_to(np.asarray(row[key], dtype=np.float64), (E,)))
            except (TypeError, ValueError):
                raise ValueError("%s[%r] must be a float or an array with one entry per member [%d]" % (what, key, E))
            if not np.isfinite(shift[r]).all():
                raise ValueError("%s[%r] must be finite" % (what, key))
    sh = None
    if any(s is not None for s in shift):
        neutral = [np.ones(E), np.ones(E), np.zeros(E)]
        sh = np.ascontiguousarray(np.stack([neutral[r] if shift[r] is None else shift[r] for r in range(3 if shift[2] is not None else 2)]))
    return dict(sigma=sigma, groups=groups, shift=sh, seed=seed, member0=member0)


def check_resolved(fe, E, D, rows):
    """A resolved ``forcing_error`` against the run it is handed to (``Engine.run``): ``ValueError``."""
    sigma = np.asarray(fe['sigma'], dtype=np.float64)
    if sigma.shape != (3,) or len(fe['groups']) != 3:
        raise ValueError("forcing_error: sigma and groups need one entry per forcing row %s" % (abi.FORCING_ROWS,))
    for r in range(3):
        g = fe['groups'][r]
        if g is not None and tuple(np.shape(g)) != (D,):
            raise ValueError("forcing_error: groups of %s need one id per day [%d], got %s" % (abi.FORCING_ROWS[r], D, np.shape(g)))
    sh = fe.get('shift')
    if sh is not None and (np.ndim(sh) != 2 or np.shape(sh)[0] not in (2, 3) or np.shape(sh)[1] != E):
        raise ValueError("forcing_error: shift must have shape [2 or 3, E = %d], got %s" % (E, np.shape(sh)))


def cut_group_arrays(forcing_error, D, lo, hi):
    """The public ``forcing_error`` of a run of ``D`` days as the window of days [lo, hi) takes it: group id arrays cut with the
    days (names stay: calendar ids are absolute).  ``ValueError`` for an array that does not cover the run."""
    if not isinstance(forcing_error, dict):
        return forcing_error                                     # resolve words the refusal
    cut = {}
    for name, row in forcing_error.items():
        if isinstance(row, dict) and row.get('groups') is not None and not isinstance(row['groups'], str):
            g = np.asarray(row['groups'])
            if g.shape != (D,):
                raise ValueError("forcing_error[%r]['groups'] must have one group id per day of the whole run [%d], got %s"
                                 % (name, D, g.shape))
            row = dict(row, groups=g[lo:hi])
        cut[name] = row
    return cut


def member_block(fe, lo, hi):
    """The resolved ``forcing_error`` of members [lo, hi) of the ensemble ``fe`` describes: the block draws what the whole would."""
    if fe is None:
        return None
    return dict(fe, shift=None if fe['shift'] is None else np.ascontiguousarray(fe['shift'][:, lo:hi]), member0=fe['member0'] + lo)


def day_window(fe, lo, hi):
    """... of days [lo, hi): the group ids are absolute, so the window draws what the whole run would."""
    if fe is None:
        return None
    return dict(fe, groups=[None if g is None else np.ascontiguousarray(g[lo:hi]) for g in fe['groups']])


def multiplier(sigma, z):
    """The mean-one lognormal multiplier exp(sigma z - 0.5 sigma sigma) in the device's order of operations."""
    sigma = float(sigma)
    return np.exp(sigma * np.asarray(z, dtype=np.float64) - 0.5 * sigma * sigma)


def normals(fe, r, E):
    """z [E, D] of row ``r``: one draw per (member, group)."""
    g = np.asarray(fe['groups'][r], dtype=np.int64)
    members = fe['member0'] + np.arange(E, dtype=np.int64)
    return predictive.standard_normal(fe['seed'], members[:, None], g[None, :], r, abi.FORCING_STREAM)


def table(base, fe, forcing_of_member=None, E=None):
    """The members' forcing sets [E, rows, D] from the base sets ``base`` [n_sets, rows, D] (rows = 2, or 3 with T_air) and the
    resolved ``fe``: what the device writes into ``simplyp_opts.forcing_table``.  ``forcing_of_member`` [E] picks each member's
    base set (None: set 0, and ``E`` must be given or follow from ``fe['shift']``)."""
    base = np.asarray(base, dtype=np.float64)
    n_sets, rows, D = base.shape
    if forcing_of_member is not None:
        fom = np.asarray(forcing_of_member, dtype=np.int64)
        E = len(fom)
    else:
        E = int(fe['shift'].shape[1]) if E is None else int(E)
        fom = np.zeros(E, dtype=np.int64)
    check_resolved(fe, E, D, rows)
    sh = fe.get('shift')
    if fe['sigma'][2] > 0.0 and rows < 3 or (sh is not None and sh.shape[0] == 3 and rows < 3):
        raise ValueError("forcing_error perturbs T_air, which the base sets do not hold")
    out = base[fom].copy()                                       # [E, rows, D]
    for r in range(rows):
        v = out[:, r, :]
        if sh is not None and r < sh.shape[0]:
            v = v * sh[r][:, None] if r < 2 else v + sh[r][:, None]
        sg = float(fe['sigma'][r])
        if sg > 0.0:
            z = normals(fe, r, E)
            v = v * multiplier(sg, z) if r < 2 else v + sg * z
        out[:, r, :] = v
    return out
