#!/usr/bin/env python3
"""Golden vectors for Thornthwaite PET (reference inputs.py:232-312, :416-508) -> thornthwaite_pet.npz.

Runs only in the build container (needs /root/reference).  The UNMODIFIED reference ``daily_PET`` (loaded the way
make_golden.py loads inputs.py) is applied to the Tarland air temperature at latitude 57.1:

    base      2003-2006, 1461 days: 2003 a normal year, 2004 the first leap year, 2005-2006 under the leap-year
              daylight table the reference's loop never assigns back
    plus3     the same series + 3 degC
    minus20   the same series - 20 degC: years whose monthly means are all <= 0 have I = 0 and a PET of 0/0 = NaN
    full      1981-2010, 10957 days

Recorded per case, data only: the air temperature handed in, the monthly means T_m the reference resamples, the monthly
PET_m (mm/month) its annual_thornthwaite returns, and the daily PET column.

Two shims stand between the reference and the installed pandas, neither touching its arithmetic: the removed constructor
``pd.DatetimeIndex(freq=, start=, end=)`` is answered by ``pd.date_range``, and the resample alias ``'M'`` by ``'ME'``
where pandas no longer takes it.

Usage:  python tests/golden/make_pet_golden.py
"""

import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden        # noqa: E402

LATITUDE = 57.1
MET = os.path.join(REPO, 'data', 'Tarland_MetData_1981-2010.csv')


class _Pandas(object):
    """The module ``pd`` as the reference sees it: everything forwards, ``DatetimeIndex(freq=, start=, end=)`` is a date range."""

    def __getattr__(self, name):
        return getattr(pd, name)

    @staticmethod
    def DatetimeIndex(data=None, freq=None, start=None, end=None, dayfirst=False, **kw):
        if data is None and start is not None:
            return pd.date_range(start=start, end=end, freq=freq)
        return pd.DatetimeIndex(data, freq=freq, dayfirst=dayfirst, **kw)


def _month_end_alias():
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            pd.Series([0.0], index=pd.date_range('2000-01-01', periods=1)).resample('M').mean()
        return None
    except Exception:
        return 'ME'


def run_reference(inputs, t_air, index):
    """(T_m [months], PET_m [months], daily PET [D]) of the reference for the series ``t_air`` on ``index``."""
    seen = {'T_m': [], 'PET_m': []}
    inner = inputs.annual_thornthwaite

    def recording(monthly_t, monthly_mean_dlh, year=None):            # the unmodified function, its arguments and result noted
        pet = inner(monthly_t, monthly_mean_dlh, year=year)
        seen['T_m'].extend(float(t) for t in monthly_t)
        seen['PET_m'].extend(float(v) for v in pet)
        return pet

    inputs.annual_thornthwaite = recording
    alias = _month_end_alias()
    resample = pd.Series.resample
    if alias:
        pd.Series.resample = lambda self, rule, *a, **k: resample(self, alias if rule == 'M' else rule, *a, **k)
    try:
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            df = inputs.daily_PET(LATITUDE, pd.DataFrame({'T_air': t_air}, index=index))
    finally:
        inputs.annual_thornthwaite = inner
        pd.Series.resample = resample
    return np.array(seen['T_m']), np.array(seen['PET_m']), df['PET'].to_numpy(dtype=float)


def main():
    inputs = make_golden.load_reference()['inputs']
    inputs.pd = _Pandas()
    met = pd.read_csv(MET, parse_dates=True, dayfirst=True, index_col=0)
    short = met.truncate(before='2003-01-01', after='2006-12-31')
    assert len(short) == 1461 and len(met) == 10957
    cases = {'base': (short, 0.0), 'plus3': (short, 3.0), 'minus20': (short, -20.0), 'full': (met, 0.0)}
    arrays = {'latitude': np.array(LATITUDE)}
    for name, (df, shift) in cases.items():
        t_air = df['T_air'].to_numpy(dtype=float) + shift
        t_m, pet_m, pet = run_reference(inputs, t_air, df.index)
        assert len(t_m) == len(pet_m) == 12 * (df.index.year[-1] - df.index.year[0] + 1) and len(pet) == len(df)
        arrays[name + '/T_air'] = t_air
        arrays[name + '/first_day'] = np.array(str(df.index[0].date()))
        arrays[name + '/T_m'], arrays[name + '/PET_m'], arrays[name + '/PET'] = t_m, pet_m, pet
        nan_years = sorted(set(int(y) for y in df.index.year[np.isnan(pet)]))
        print(name, len(df), 'days; NaN days %d in years %s' % (np.isnan(pet).sum(), nan_years))
    # minus20: at least one year with I = 0 and a NaN PET, and the other years finite
    years = short.index.year.to_numpy()
    t_m = arrays['minus20/T_m'].reshape(-1, 12)
    dead = (t_m <= 0).all(axis=1)
    assert dead.any(), dead                                           # (at -20 degC every one of the four years is)
    for y, is_dead in zip(range(2003, 2007), dead):
        mid = (years == y) & (short.index.dayofyear.to_numpy() > 20) & (short.index.dayofyear.to_numpy() < 340)
        assert np.isnan(arrays['minus20/PET'][mid]).all() if is_dead else np.isfinite(arrays['minus20/PET'][mid]).all(), y
    for name in ('base', 'plus3', 'full'):
        assert np.isfinite(arrays[name + '/PET']).all()
    np.savez_compressed(os.path.join(HERE, 'thornthwaite_pet.npz'), **arrays)
    print('thornthwaite_pet.npz written')


if __name__ == '__main__':
    main()
