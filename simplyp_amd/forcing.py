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
absolute integers in [0, 2^31), made from the calendar so that a window of a run sees the ids the whole run sees.

Autocorrelated errors: ``rho`` of a row is the lag-one correlation of ``z`` between *consecutive groups* along the day axis.  Walk
the days of the call in order; day ``d`` starts a step when its group id differs from the previous day's (for ``d = 0``: from the
incoming noise state's last group id, "none" without a state).  At a step with group id ``g``::

    eps = predictive.standard_normal(seed, member0 + e, g, r, abi.FORCING_STREAM)     the very draw of the independent model
    z   = eps                           when there is no previous z (no state: a stationary start)
    z   = (rho * z_prev) + (c * eps)    otherwise, c = sqrt(1.0 - rho * rho) computed once in fp64

two products and a sum, each rounded (no fused multiply-add); the other days reuse ``z``, which then goes through the formulas
above unchanged.  ``rho = 0`` is the independent row, bit for bit.  A group id that comes back after other ids is simply a new
step that happens to reuse its ``eps``.  The noise state is a float64 table ``[6, E]`` in member order
(``abi.FORCING_NOISE_ROWS``): rows 0-2 hold ``z`` of P, PET and T_air, rows 3-5 that row's last group id as an exact integer,
``-1.0`` = none; a row without ``rho`` is written as ``0.0`` / ``-1.0`` and ignored on input.  It travels from run to run as the
model state does: a run over ``D1 + D2`` days equals a run over ``D1`` days followed by one over ``D2`` days handed the first
one's noise state, bit for bit, also when the cut falls inside a group.  AR orders above one, cross-correlation between rows and
a ``rho`` per member are not offered.

Seasonal change factors: ``scale`` (``offset``) may be ``[G, E]`` or ``[G]`` together with ``scale_groups`` (``offset_groups``) --
``'month_of_year'`` (ids month - 1, G = 12) or an int array [D] with ids in [0, G) --: day ``d`` takes the entry of its shift
group.  The rows share one shift-group array; ``G`` lies in [1, 4096].

The public calls take ``forcing_error`` as a dict of dicts (``resolve``); ``Engine.run`` takes what ``resolve`` returns.
"""

import numpy as np

from . import abi, predictive

SIGMA_MAX = 2.0
RHO_MAX, SHIFT_GROUPS_MAX = abi.FORCING_RHO_MAX, abi.FORCING_SHIFT_GROUPS_MAX
_ROW_KEYS = [('sigma', 'groups', 'scale', 'rho', 'scale_groups'), ('sigma', 'groups', 'scale', 'rho', 'scale_groups'),
             ('sigma', 'groups', 'offset', 'rho', 'offset_groups')]
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


def _shift_groups(what, spec, index):
    """(shift-group ids int64 [D], G where the name fixes it else None) of a ``scale_groups`` / ``offset_groups``."""
    if isinstance(spec, str):
        if spec != 'month_of_year':
            raise ValueError("%s must be 'month_of_year' or an int array with one shift group id per day [%d] (got %r)" % (what, len(index), spec))
        return np.asarray(index.month, dtype=np.int64) - 1, 12
    g = np.asarray(spec)
    if g.dtype.kind not in 'iu' or g.shape != (len(index),):
        raise ValueError("%s must be 'month_of_year' or an int array with one shift group id per day [%d] (got %s %s)"
                         % (what, len(index), g.dtype, g.shape))
    return g.astype(np.int64), None


def _grouped_shift(what, key, value, ids, G, E):
    """``scale`` / ``offset`` given with shift groups as [G, E]: from [G, E], [G] (broadcast over members) or a float."""
    try:
        val = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s[%r] must be a float or an array [G] or [G, E = %d] with %r" % (what, key, E, key + '_groups'))
    if val.ndim == 0:
        val = np.full((G if G is not None else int(ids.max()) + 1 if len(ids) else 1, E), float(val))
    elif val.ndim == 1:
        val = np.broadcast_to(val[:, None], (val.shape[0], E))
    elif val.ndim != 2 or val.shape[1] != E:
        raise ValueError("%s[%r] with %r must have shape [G] or [G, E = %d], got %s" % (what, key, key + '_groups', E, val.shape))
    n = val.shape[0]
    if not 1 <= n <= SHIFT_GROUPS_MAX:
        raise ValueError("%s[%r]: the number of shift groups G must lie in [1, %d] (got %d)" % (what, key, SHIFT_GROUPS_MAX, n))
    if G is not None and n != G:
        raise ValueError("%s[%r] needs one entry per shift group: G = %d with 'month_of_year' (got %d)" % (what, key, G, n))
    if len(ids) and (int(ids.min()) < 0 or int(ids.max()) >= n):
        raise ValueError("%s[%r]: shift group ids must lie in [0, G = %d)" % (what, key + '_groups', n))
    if not np.isfinite(val).all():
        raise ValueError("%s[%r] must be finite" % (what, key))
    return np.ascontiguousarray(val)


def resolve(forcing_error, index, E, snow, seed=0, member0=0):
    """The public ``forcing_error`` -- ``{'P': {'sigma':, 'groups':, 'rho':, 'scale':, 'scale_groups':}, 'PET': {...}, 'T_air':
    {'sigma':, 'groups':, 'rho':, 'offset':, 'offset_groups':}}``, every key optional, ``groups`` = ``'day'`` (default) |
    ``'month'`` | ``'year'`` | int array [D], ``rho`` the lag-one correlation between consecutive groups in [0, 0.999] (needs
    ``sigma > 0``), ``scale`` / ``offset`` a float or an array [E] -- or, with ``scale_groups`` / ``offset_groups`` =
    ``'month_of_year'`` | int array [D] of ids in [0, G), an array [G, E] or [G] -- as what ``Engine.run`` and ``table`` take:
    dict(sigma float64 [3], rho float64 [3], groups [3 x (int32 [D] or None)], shift (float64 [2 or 3, E]: P scale, PET scale(,
    T_air offset); [2 or 3, G, E] with shift groups, a per-member row broadcast over G; None when none is given), shift_groups
    (int32 [D] or None: the one array the rows share), seed, member0).  None for None.  ``ValueError`` for an unknown key, a
    sigma that is not finite or outside [0, 2], a rho that is not finite or outside [0, 0.999] or comes without sigma, an array of
    the wrong shape, group ids outside [0, 2^31), shift group ids outside [0, G), G outside [1, 4096], rows with different shift
    groups, ``'T_air'`` without the in-kernel snow module, a seed outside [0, 2^64)."""
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
    sigma, rho, groups, shift, sg, n_groups = np.zeros(3), np.zeros(3), [None] * 3, [None] * 3, None, 0
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
        try:
            rho[r] = float(row.get('rho', 0.0))
        except (TypeError, ValueError):
            raise ValueError("%s['rho'] must be a number" % what)
        if not (np.isfinite(rho[r]) and 0.0 <= rho[r] <= RHO_MAX):
            raise ValueError("%s['rho'] must be finite and in [0, %g] (got %r)" % (what, RHO_MAX, row.get('rho')))
        if rho[r] > 0.0 and not sigma[r] > 0.0:
            raise ValueError("%s['rho'] > 0 needs 'sigma' > 0: there is no error to correlate" % what)
        g = _groups("%s['groups']" % what, row.get('groups', 'day'), index)
        groups[r] = g if sigma[r] > 0.0 else None
        key = _ROW_KEYS[r][2]
        if row.get(key + '_groups') is not None:
            if row.get(key) is None:
                raise ValueError("%s[%r] needs %s[%r]: one entry per shift group" % (what, key + '_groups', what, key))
            ids, G = _shift_groups("%s[%r]" % (what, key + '_groups'), row[key + '_groups'], index)
            shift[r] = _grouped_shift(what, key, row[key], ids, G, E)
            if sg is not None and not (np.array_equal(sg, ids) and n_groups == shift[r].shape[0]):
                raise ValueError("forcing_error: the rows share one array of shift groups, %s gives different ones (ids or G)" % what)
            sg, n_groups = ids, shift[r].shape[0]
        elif row.get(key) is not None:
            if np.ndim(row[key]) > 1:
                raise ValueError("%s[%r] with more than one dimension needs %r: the shift group of every day" % (what, key, key + '_groups'))
            try:
                shift[r] = np.ascontiguousarray(np.broadcast_to(np.asarray(row[key], dtype=np.float64), (E,)))
            except (TypeError, ValueError):
                raise ValueError("%s[%r] must be a float or an array with one entry per member [%d]" % (what, key, E))
            if not np.isfinite(shift[r]).all():
                raise ValueError("%s[%r] must be finite" % (what, key))
    sh = None
    if any(s is not None for s in shift):
        neutral = [np.ones(E), np.ones(E), np.zeros(E)]
        rows = [neutral[r] if shift[r] is None else shift[r] for r in range(3 if shift[2] is not None else 2)]
        if sg is not None:                                       # a per-member row next to a grouped one: the same for every group
            rows = [np.broadcast_to(x, (n_groups, E)) for x in rows]
        sh = np.ascontiguousarray(np.stack(rows))
    return dict(sigma=sigma, rho=rho, groups=groups, shift=sh, shift_groups=None if sg is None else np.ascontiguousarray(sg, dtype=np.int32),
                seed=seed, member0=member0)


def any_rho(fe):
    """Whether the resolved ``fe`` has an autocorrelated row, so a noise state."""
    return fe is not None and fe.get('rho') is not None and bool((np.asarray(fe['rho'], dtype=np.float64) > 0.0).any())


def check_resolved(fe, E, D, rows):
    """A resolved ``forcing_error`` against the run it is handed to (``Engine.run``): ``ValueError``."""
    sigma = np.asarray(fe['sigma'], dtype=np.float64)
    if sigma.shape != (3,) or len(fe['groups']) != 3:
        raise ValueError("forcing_error: sigma and groups need one entry per forcing row %s" % (abi.FORCING_ROWS,))
    for r in range(3):
        g = fe['groups'][r]
        if g is not None and tuple(np.shape(g)) != (D,):
            raise ValueError("forcing_error: groups of %s need one id per day [%d], got %s" % (abi.FORCING_ROWS[r], D, np.shape(g)))
    if fe.get('rho') is not None:
        rho = np.asarray(fe['rho'], dtype=np.float64)
        if rho.shape != (3,) or not (np.isfinite(rho).all() and (rho >= 0.0).all() and (rho <= RHO_MAX).all()):
            raise ValueError("forcing_error: rho needs one finite entry in [0, %g] per forcing row %s" % (RHO_MAX, abi.FORCING_ROWS))
        if ((rho > 0.0) & ~(sigma > 0.0)).any() or any(rho[r] > 0.0 and fe['groups'][r] is None for r in range(3)):
            raise ValueError("forcing_error: rho > 0 needs sigma > 0 and the group ids of that row")
    sh, sg = fe.get('shift'), fe.get('shift_groups')
    if sg is None:
        if sh is not None and (np.ndim(sh) != 2 or np.shape(sh)[0] not in (2, 3) or np.shape(sh)[1] != E):
            raise ValueError("forcing_error: shift must have shape [2 or 3, E = %d], got %s" % (E, np.shape(sh)))
    else:
        if sh is None or np.ndim(sh) != 3 or np.shape(sh)[0] not in (2, 3) or np.shape(sh)[2] != E \
                or not 1 <= np.shape(sh)[1] <= SHIFT_GROUPS_MAX:
            raise ValueError("forcing_error: shift with shift_groups must have shape [2 or 3, G in [1, %d], E = %d], got %s"
                             % (SHIFT_GROUPS_MAX, E, np.shape(sh)))
        sg = np.asarray(sg)
        if sg.shape != (D,) or sg.dtype.kind not in 'iu' or (D and (int(sg.min()) < 0 or int(sg.max()) >= np.shape(sh)[1])):
            raise ValueError("forcing_error: shift_groups needs one id in [0, G = %d) per day [%d]" % (np.shape(sh)[1], D))


def cut_group_arrays(forcing_error, D, lo, hi):
    """The public ``forcing_error`` of a run of ``D`` days as the window of days [lo, hi) takes it: group id arrays and shift
    group arrays cut with the days (names stay: calendar ids are absolute).  ``ValueError`` for an array that does not cover the
    run."""
    if not isinstance(forcing_error, dict):
        return forcing_error                                     # resolve words the refusal
    cut = {}
    for name, row in forcing_error.items():
        for key in ('groups', 'scale_groups', 'offset_groups'):
            if isinstance(row, dict) and row.get(key) is not None and not isinstance(row[key], str):
                g = np.asarray(row[key])
                if g.shape != (D,):
                    raise ValueError("forcing_error[%r][%r] must have one group id per day of the whole run [%d], got %s"
                                     % (name, key, D, g.shape))
                val = row.get(key[:-7]) if key != 'groups' else None
                if val is not None and np.ndim(val) >= 1 and g.dtype.kind in 'iu' and D and \
                        (int(g.min()) < 0 or int(g.max()) >= np.shape(val)[0]):      # a window would see only its own days' ids
                    raise ValueError("forcing_error[%r][%r]: shift group ids must lie in [0, G = %d)" % (name, key, np.shape(val)[0]))
                row = dict(row, **{key: g[lo:hi]})
        cut[name] = row
    return cut


def member_block(fe, lo, hi):
    """The resolved ``forcing_error`` of members [lo, hi) of the ensemble ``fe`` describes: the block draws what the whole would
    (and continues the columns [lo, hi) of the whole's noise state)."""
    if fe is None:
        return None
    return dict(fe, shift=None if fe['shift'] is None else np.ascontiguousarray(fe['shift'][..., lo:hi]), member0=fe['member0'] + lo)


def day_window(fe, lo, hi):
    """... of days [lo, hi): the group ids are absolute, so the window draws what the whole run would (an autocorrelated row:
    when handed the noise state of the days before)."""
    if fe is None:
        return None
    sg = fe.get('shift_groups')
    return dict(fe, groups=[None if g is None else np.ascontiguousarray(g[lo:hi]) for g in fe['groups']],
                shift_groups=None if sg is None else np.ascontiguousarray(sg[lo:hi]))


def multiplier(sigma, z):
    """The mean-one lognormal multiplier exp(sigma z - 0.5 sigma sigma) in the device's order of operations."""
    sigma = float(sigma)
    return np.exp(sigma * np.asarray(z, dtype=np.float64) - 0.5 * sigma * sigma)


def normals(fe, r, E):
    """The draws [E, D] of row ``r``: one per (member, group) -- z of a row without rho, eps of an autocorrelated one."""
    g = np.asarray(fe['groups'][r], dtype=np.int64)
    members = fe['member0'] + np.arange(E, dtype=np.int64)
    return predictive.standard_normal(fe['seed'], members[:, None], g[None, :], r, abi.FORCING_STREAM)


def check_noise(noise, E):
    """A noise state as float64 [6, E] (``abi.FORCING_NOISE_ROWS``): ``ValueError`` for another shape."""
    noise = np.asarray(noise, dtype=np.float64)
    if noise.shape != (len(abi.FORCING_NOISE_ROWS), E):
        raise ValueError("the forcing noise state must have shape [%d, E = %d], got %s" % (len(abi.FORCING_NOISE_ROWS), E, noise.shape))
    return noise


def ar1_normals(fe, r, E, noise=None):
    """z [E, D] of the autocorrelated row ``r`` walked day by day from the noise state ``noise`` [6, E] (None: a stationary
    start), and the row's state after the last day: (z, z_last [E], last group id)."""
    g = np.asarray(fe['groups'][r], dtype=np.int64)
    rho = float(fe['rho'][r])
    c = float(np.sqrt(1.0 - rho * rho))
    eps = normals(fe, r, E)
    z, prev = (np.zeros(E), np.full(E, -1, dtype=np.int64)) if noise is None else (noise[r].copy(), noise[3 + r].astype(np.int64))
    have = prev >= 0
    out = np.empty((E, len(g)))
    for d in range(len(g)):
        step = prev != g[d]
        z = np.where(step, np.where(have, (rho * z) + (c * eps[:, d]), eps[:, d]), z)
        have = have | step
        prev = np.full(E, g[d], dtype=np.int64)
        out[:, d] = z
    return out, z, int(g[-1])


def table(base, fe, forcing_of_member=None, E=None, noise=None, return_noise=False):
    """The members' forcing sets [E, rows, D] from the base sets ``base`` [n_sets, rows, D] (rows = 2, or 3 with T_air) and the
    resolved ``fe``: what the device writes into ``simplyp_opts.forcing_table``.  ``forcing_of_member`` [E] picks each member's
    base set (None: set 0, and ``E`` must be given or follow from ``fe['shift']``).  ``noise``: the noise state [6, E] the
    autocorrelated rows continue (None: a stationary start); ``return_noise=True``: returns (table, the noise state [6, E]
    after the last day) -- what the device writes into ``simplyp_opts.forcing_noise_out``."""
    base = np.asarray(base, dtype=np.float64)
    n_sets, rows, D = base.shape
    if forcing_of_member is not None:
        fom = np.asarray(forcing_of_member, dtype=np.int64)
        E = len(fom)
    else:
        E = int(fe['shift'].shape[-1]) if E is None else int(E)
        fom = np.zeros(E, dtype=np.int64)
    check_resolved(fe, E, D, rows)
    sh, sg = fe.get('shift'), fe.get('shift_groups')
    if fe['sigma'][2] > 0.0 and rows < 3 or (sh is not None and sh.shape[0] == 3 and rows < 3):
        raise ValueError("forcing_error perturbs T_air, which the base sets do not hold")
    rho = np.zeros(3) if fe.get('rho') is None else np.asarray(fe['rho'], dtype=np.float64)
    noise = None if noise is None else check_noise(noise, E)
    noise_out = np.zeros((6, E))
    noise_out[3:] = -1.0
    out = base[fom].copy()                                       # [E, rows, D]
    for r in range(rows):
        v = out[:, r, :]
        if sh is not None and r < sh.shape[0]:
            s_ = sh[r][:, None] if sg is None else sh[r][np.asarray(sg, dtype=np.int64), :].T        # [E, 1] or [E, D]
            v = v * s_ if r < 2 else v + s_
        sgm = float(fe['sigma'][r])
        if sgm > 0.0:
            if rho[r] > 0.0:
                z, noise_out[r], noise_out[3 + r] = ar1_normals(fe, r, E, noise)
            else:
                z = normals(fe, r, E)
            v = v * multiplier(sgm, z) if r < 2 else v + sgm * z
        out[:, r, :] = v
    return (out, noise_out) if return_noise else out
