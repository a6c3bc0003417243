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

Thornthwaite PET from the member's own air temperature (``'PET': {'model': 'thornthwaite', 'latitude': deg}``, snow module
only): the member's PET row is ``TH * F`` -- ``TH`` = ``thornthwaite_rows`` of the member's FINAL T_air row above, ``F`` = the PET
row the formulas above give for a base PET of 1.0 (the scale and the lognormal multiplier; 1.0 bit for bit with neither).  The
base PET column is not read.  ``thornthwaite_plan`` makes the calendar side once per call on the host; ``thornthwaite_rows``
states the rule (the reference's inputs.py:232-312, :416-508, quirks included) in the device's order of operations.

The public calls take ``forcing_error`` as a dict of dicts (``resolve``); ``Engine.run`` takes what ``resolve`` returns.
"""

import calendar
import math

import numpy as np

from . import abi, predictive

SIGMA_MAX = 2.0
RHO_MAX, SHIFT_GROUPS_MAX = abi.FORCING_RHO_MAX, abi.FORCING_SHIFT_GROUPS_MAX
PET_YEARS_MAX = abi.FORCING_PET_YEARS_MAX
_ROW_KEYS = [('sigma', 'groups', 'scale', 'rho', 'scale_groups'),
             ('sigma', 'groups', 'scale', 'rho', 'scale_groups', 'model', 'latitude'),
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


def daylight_hours(latitude, leap):
    """Mean daylight hours [12] of the months of a (leap) year at ``latitude`` degrees: FAO-56 eq. 24 (solar declination of the
    day of the year), eq. 25 (sunset hour angle, its cosine clipped to [-1, 1]: polar day and night) and eq. 34, the days of a
    month added in order and divided by their number."""
    phi = latitude * (math.pi / 180.0)
    out, doy = [], 1
    for n in (31, 29 if leap else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31):
        total = 0.0
        for _ in range(n):
            dec = 0.409 * math.sin((2.0 * math.pi / 365.0) * doy - 1.39)
            total += (24.0 / math.pi) * math.acos(min(max(-math.tan(phi) * math.tan(dec), -1.0), 1.0))
            doy += 1
        out.append(total / n)
    return out


def thornthwaite_plan(index, latitude, max_years=PET_YEARS_MAX):
    """The calendar side of Thornthwaite PET for the daily dates ``index`` at ``latitude`` degrees, made once per call: dict(D,
    months M = 12 x years, years, latitude; per month m counted from the first January: first (int32 [M], the day index of its
    first day), days (int32 [M], N = daysinmonth), daylight (float64 [M], L); per day d: node (int32 [D], j = the month whose
    16th is the node at or before d, 0 before the first node), k (int32 [D], days since that node; 0 before the first node and
    after the last), n (int32 [D], days from node j to node j + 1)).  L of a year comes from the normal-year table until the
    record's first leap year and from the leap-year table in EVERY year from then on: the reference's loop assigns the leap
    table and never assigns back, and a drop-in reproduces that.  ``ValueError`` for a latitude outside [-90, 90], dates that
    are not consecutive days, a record that does not run from a 1 January to a 31 December, and more than ``max_years``
    years (the device's cap; None on the host: no cap)."""
    try:
        latitude = float(latitude)
    except (TypeError, ValueError):
        raise ValueError("Thornthwaite PET needs a latitude in degrees (got %r)" % (latitude,))
    if not -90.0 <= latitude <= 90.0:
        raise ValueError("Thornthwaite PET: latitude must lie in [-90, 90] degrees (got %r)" % (latitude,))
    D = len(index)
    ordinal = calendar_groups(index, 'day') if D else np.zeros(0, dtype=np.int64)
    if D == 0 or not np.array_equal(ordinal - ordinal[0], np.arange(D)):
        raise ValueError("Thornthwaite PET needs daily met data: one row per consecutive day")
    year, month, dom = (np.asarray(getattr(index, a), dtype=np.int64) for a in ('year', 'month', 'day'))
    for at, ok in ((0, month[0] == 1 and dom[0] == 1), (-1, month[-1] == 12 and dom[-1] == 31)):
        if not ok:
            raise ValueError("PET calc requires input met data for whole calendar years. Year %d does not run from 1 January to "
                             "31 December. Check input met data, or change the start/end dates in the parameter file" % year[at])
    years = int(year[-1] - year[0] + 1)
    if max_years is not None and years > max_years:
        raise ValueError("Thornthwaite PET on the device takes at most %d years per call (got %d)" % (max_years, years))
    M = 12 * years
    m_of_day = (year - year[0]) * 12 + month - 1
    first = np.searchsorted(m_of_day, np.arange(M)).astype(np.int64)
    days = np.diff(np.append(first, D))
    tables, sticky, daylight = (daylight_hours(latitude, False), daylight_hours(latitude, True)), False, []
    for y in range(int(year[0]), int(year[-1]) + 1):
        sticky = sticky or calendar.isleap(y)
        daylight.extend(tables[sticky])
    x_node = first + 15                                          # the 16th of every month
    node = np.clip(np.searchsorted(x_node, np.arange(D), side='right') - 1, 0, M - 1)
    nxt = np.minimum(node + 1, M - 1)
    inside = (np.arange(D) >= x_node[0]) & (nxt > node)
    k = np.where(inside, np.arange(D) - x_node[node], 0)
    n = np.where(nxt > node, x_node[nxt] - x_node[node], 1)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return dict(D=D, months=M, years=years, latitude=latitude, first=i32(first), days=i32(days),
                daylight=np.ascontiguousarray(daylight, dtype=np.float64), node=i32(node), k=i32(k), n=i32(n))


def _pow(x, y):
    """x^y as the device has it: exp(y log x) for x > 0, exactly 0.0 for x == 0, NaN otherwise."""
    with np.errstate(all='ignore'):
        p = np.exp(y * np.log(np.where(x > 0.0, x, 1.0)))
    return np.where(x > 0.0, p, np.where(x == 0.0, 0.0, np.nan))


def thornthwaite_rows(t_air, plan, monthly=False):
    """Thornthwaite's daily PET [E, D] (mm/day) of the air temperature rows ``t_air`` [E, D] under ``plan``
    (``thornthwaite_plan``): the statement the device copies.  Every operation is rounded once, in the order written, no fused
    multiply-add::

        T_m   = (T_air of the month's days added left to right in day order) / N;   T_m = T_m * (T_m >= 0)
        I_y   = the year's twelve (T_m / 5) ** 1.514 added in month order, 0.0 where T_m / 5 is not > 0
        a_y   = (((6.75e-7 * ((I * I) * I)) - (7.71e-5 * (I * I))) + (1.792e-2 * I)) + 0.49239
        PET_m = (((1.6 * (L / 12)) * (N / 30)) * ((10 * T_m) / I_y) ** a_y) * 10             mm per month
        V_m   = PET_m / N                                                                     mm per day, on the 16th
        TH[d] = V_j when k == 0, else V_j + ((V_(j+1) - V_j) / n) * k                         j, k, n of day d from the plan

    with ``x ** y`` = ``exp(y * log(x))`` for ``x > 0``, exactly ``0.0`` for ``x == 0`` and NaN otherwise.  A year whose monthly
    means are all <= 0 has ``I = 0`` and ``PET_m = 0 / 0`` = NaN, as in the reference; every day that interpolates from one of
    its nodes is NaN.  (The reference's pandas step treats such nodes as missing and bridges up to 32 days on either side of
    them from the finite nodes around; a record that mixes such years with others differs there, and is non-finite in both.)
    ``monthly=True``: returns (TH, the clamped T_m [E, M], PET_m [E, M])."""
    t = np.asarray(t_air, dtype=np.float64)
    E, D = t.shape
    if D != plan['D']:
        raise ValueError("thornthwaite_rows: the plan covers %d days, the rows have %d" % (plan['D'], D))
    M, days = plan['months'], plan['days'].astype(np.int64)
    N = days.astype(np.float64)
    at = np.minimum(plan['first'].astype(np.int64)[:, None] + np.arange(31)[None, :], D - 1)       # [M, 31]
    s = np.zeros((E, M))
    for i in range(31):                                          # (+ 0.0 past the month's end leaves the sum as it is)
        s = s + np.where(i < days, t[:, at[:, i]], 0.0)
    with np.errstate(all='ignore'):
        tm = s / N
        tm = tm * (tm >= 0.0)
        x = tm / 5.0
        term = np.where(x > 0.0, _pow(x, 1.514), 0.0)
        I = np.zeros((E, M // 12))
        for j in range(12):
            I = I + term[:, j::12]
        I2 = I * I
        I3 = I2 * I
        a = (((6.75e-07 * I3) - (7.71e-05 * I2)) + (1.792e-02 * I)) + 0.49239
        p = _pow((10.0 * tm) / np.repeat(I, 12, axis=1), np.repeat(a, 12, axis=1))
        pet_m = (((1.6 * (plan['daylight'] / 12.0)) * (N / 30.0)) * p) * 10.0
        v = pet_m / N
        j, k, n = plan['node'].astype(np.int64), plan['k'], plan['n']
        y0, y1 = v[:, j], v[:, np.minimum(j + 1, M - 1)]
        th = np.where(k == 0, y0, y0 + ((y1 - y0) / n.astype(np.float64)) * k.astype(np.float64))
    return (th, tm, pet_m) if monthly else th


def refuse_pet_model(forcing_error, where):
    """``ValueError`` when the public ``forcing_error`` asks for a PET model in a call that runs the days in windows."""
    row = forcing_error.get('PET') if isinstance(forcing_error, dict) else None
    if isinstance(row, dict) and row.get('model') is not None:
        raise ValueError("forcing_error['PET']['model'] is not offered in %s: the daily interpolation between the monthly values "
                         "crosses year boundaries, so windows laid end to end would not be the one call" % where)


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
    groups, ``'T_air'`` without the in-kernel snow module, a seed outside [0, 2^64).  ``'PET'`` also takes ``'model':
    'thornthwaite'`` with ``'latitude'`` in degrees: the result's ``pet`` is then the plan of ``thornthwaite_plan`` with ``model``
    = ``abi.FORCING_PET_MODELS['thornthwaite']`` (None otherwise); ``ValueError`` for another model, a missing latitude or one
    outside [-90, 90], dates that are not whole calendar years of consecutive days (at most ``PET_YEARS_MAX``), no snow module."""
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
    sigma, rho, groups, shift, sg, n_groups, pet = np.zeros(3), np.zeros(3), [None] * 3, [None] * 3, None, 0, None
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
        if row.get('model') is not None:
            if row['model'] not in abi.FORCING_PET_MODELS:
                raise ValueError("%s['model'] must be one of %s (got %r)" % (what, sorted(abi.FORCING_PET_MODELS), row['model']))
            if not snow:
                raise ValueError("%s['model'] needs the in-kernel snow module (snow_in_kernel=True): without it the members have "
                                 "no T_air row to derive PET from" % what)
            if row.get('latitude') is None:
                raise ValueError("%s['model'] needs %s['latitude'] in degrees" % (what, what))
            pet = dict(thornthwaite_plan(index, row['latitude']), model=abi.FORCING_PET_MODELS[row['model']])
        elif row.get('latitude') is not None:
            raise ValueError("%s['latitude'] needs %s['model']" % (what, what))
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
                seed=seed, member0=member0, pet=pet)


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
    pet = fe.get('pet')
    if pet is not None:
        if rows != 3:
            raise ValueError("forcing_error: a PET model needs the T_air row of the in-kernel snow module")
        if pet['D'] != D or pet['months'] != 12 * pet['years'] or not 1 <= pet['years'] <= PET_YEARS_MAX:
            raise ValueError("forcing_error: the PET plan covers %d days in %d months of %d years, the run has %d days (at most %d "
                             "whole years)" % (pet['D'], pet['months'], pet['years'], D, PET_YEARS_MAX))
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
    if fe.get('pet') is not None and (lo, hi) != (0, fe['pet']['D']):
        raise ValueError("forcing_error: a PET model does not run in windows of days (its interpolation crosses year boundaries)")
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
        v = np.ones((E, D)) if r == 1 and fe.get('pet') is not None else out[:, r, :]     # a PET model: F, the row of a base of 1.0
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
    if fe.get('pet') is not None:
        out[:, 1, :] = thornthwaite_rows(out[:, 2, :], fe['pet']) * out[:, 1, :]
    return (out, noise_out) if return_noise else out
