"""Warm start, the host side (no GPU): the SIMPLYP_STATE_* rows of include/simplyp.h against abi.STATE_ROWS, the two new
entry points of the C ABI, the pure-host window splitter, and the refusals of a state that does not fit the run -- raised
before the device layer is touched."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, ensemble

from c_header import c_values, header_text

ROOT = os.path.dirname(engine.HERE)


def test_state_rows_match_the_header():
    txt = re.sub(r'/\*.*?\*/', '', header_text(), flags=re.S)
    body = re.search(r'enum \{\s*SIMPLYP_STATE_VSA = 0(.*?)SIMPLYP_N_STATE', txt, re.S).group(0)
    names = re.findall(r'SIMPLYP_STATE_([A-Z0-9_]+)', body)
    assert names == ['VSA', 'VSS', 'VG', 'VR', 'QR', 'MSUS', 'TDPR', 'PPR', 'PLAB_A', 'TDPS_A', 'PLAB_NC', 'TDPS_NC',
                     'CONC_TDPS_A', 'CONC_TDPS_NC', 'H_NEXT', 'D_SNOW']
    assert abi.STATE_ROWS == ['VsA', 'VsS', 'Vg', 'Vr', 'Qr', 'Msus', 'TDPr', 'PPr', 'Plab_A', 'TDPs_A', 'Plab_NC', 'TDPs_NC',
                              'conc_TDPs_A', 'conc_TDPs_NC', 'h_next', 'D_snow']
    assert [n.lower() for n in names] == [r.lower() for r in abi.STATE_ROWS]
    assert abi.N_STATE == len(names) == 16


def test_n_state_is_16_for_the_c_compiler():
    got = c_values(['SIMPLYP_N_STATE', 'SIMPLYP_STATE_H_NEXT', 'SIMPLYP_ABI_VERSION'])
    assert got == {'SIMPLYP_N_STATE': 16, 'SIMPLYP_STATE_H_NEXT': 14, 'SIMPLYP_ABI_VERSION': abi.ABI_VERSION}


def test_new_symbols_are_declared_listed_and_exported():
    engine.build()
    L = engine.lib()
    declared = set(re.findall(r'\b(simplyp_[a-z0-9_]+)\s*\(', header_text()))
    for name in ('simplyp_state_bytes', 'simplyp_set_state'):
        assert name in declared and name in engine.ABI_SYMBOLS and hasattr(L, name)


def test_state_bytes_and_null_context():
    engine.build()
    L = engine.lib()
    for E, S, D in ((1, 1, 1), (150, 1, 732), (100000, 1, 10957), (10000, 256, 18262), (1000000, 3, 5)):
        dims = abi.Dims(E, S, D, 1)
        assert L.simplyp_state_bytes(C.byref(dims)) == S * 16 * E * 8
    assert L.simplyp_state_bytes(None) < 0
    assert L.simplyp_state_bytes(C.byref(abi.Dims(0, 1, 1, 1))) < 0
    buf = (C.c_double * 16)()
    err_arg = -1                                                   # SIMPLYP_ERR_ARG
    assert L.simplyp_set_state(None, None, None) == err_arg
    assert L.simplyp_set_state(None, C.addressof(buf), C.addressof(buf)) == err_arg


def test_c_example_compiles_and_links_against_the_header(tmp_path):
    engine.build()
    exe = str(tmp_path / 'resume_from_c')
    subprocess.check_call(['gcc', '-O2', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'examples', 'resume_from_c.c'), '-o', exe, '-L' + engine.CSRC, '-lsimplyp_hip',
                           '-Wl,-rpath,' + engine.CSRC, '-lm'])
    p = subprocess.run([exe, '4', '10'], capture_output=True, text=True, timeout=120)
    assert p.returncode in (0, 2), p.stderr            # without a GPU the program stops at simplyp_device_count()
    if p.returncode == 2:
        assert 'no HIP device' in p.stderr


# ---- ensemble.window_bounds ----------------------------------------------------------------------------------------------

def test_annual_windows_of_1981_2010():
    idx = pd.date_range('1981-01-01', '2010-12-31')
    b = ensemble.window_bounds(idx, 'annual')
    assert len(b) == 30 and b[0][0] == 0 and b[-1][1] == len(idx) == 10957
    assert all(hi == lo2 for (_, hi), (lo2, _) in zip(b, b[1:]))
    for (lo, hi), year in zip(b, range(1981, 2011)):
        assert idx[lo] == pd.Timestamp(year, 1, 1) and idx[hi - 1] == pd.Timestamp(year, 12, 31)
        assert hi - lo == (366 if year % 4 == 0 else 365)
    # a series that starts and ends inside a year
    b = ensemble.window_bounds(pd.date_range('2003-11-20', '2005-02-03'), 'annual')
    assert b == [(0, 42), (42, 42 + 366), (42 + 366, 42 + 366 + 34)]


def test_int_window_with_a_short_tail_and_explicit_dates():
    idx = pd.date_range('2004-01-01', '2004-12-31')
    assert ensemble.window_bounds(idx, 100) == [(0, 100), (100, 200), (200, 300), (300, 366)]
    assert ensemble.window_bounds(idx, 366) == [(0, 366)] == ensemble.window_bounds(idx, 1000)
    assert ensemble.window_bounds(idx, ['2004-01-01', '2004-03-01', pd.Timestamp('2004-10-15')]) == [(0, 60), (60, 288), (288, 366)]
    for bad in (['2004-02-01'], ['2004-01-01', '2005-01-01'], ['2004-01-01', '2004-06-01', '2004-03-01'], [], 0, 'monthly'):
        with pytest.raises(ValueError):
            ensemble.window_bounds(idx, bad)


def test_windows_must_fall_on_period_boundaries():
    idx = pd.date_range('1981-01-01', '1983-12-31')
    assert len(ensemble.window_bounds(idx, 'annual', reduce='annual')) == 3
    assert ensemble.window_bounds(idx, ['1981-01-01', '1983-01-01'], reduce='annual') == [(0, 730), (730, 1095)]
    with pytest.raises(ValueError, match='period'):
        ensemble.window_bounds(idx, 100, reduce='annual')
    period = np.arange(len(idx)) // 50
    assert len(ensemble.window_bounds(idx, 100, reduce=period)) == 11
    with pytest.raises(ValueError, match='period'):
        ensemble.window_bounds(idx, 75, reduce=period)


# ---- refusals of initial_state, before the device layer -----------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the call touched the device layer")
    monkeypatch.setattr(engine, 'get_engine', touched)
    monkeypatch.setattr(engine, 'pinned_empty', touched)


def _state_dict(S=1, E=3, end='2003-12-31', reaches=(1,)):
    return dict(rows=list(abi.STATE_ROWS), reaches=list(reaches), data=np.ones((S, 16, E)), end=pd.Timestamp(end))


def test_initial_state_with_a_date_gap_is_refused_before_any_device_is_touched(no_device):
    args = helpers.scenario_inputs('tarland_2004_dynamic')
    assert args[0].index[0] == pd.Timestamp('2004-01-01')
    for end in ('2003-12-30', '2004-01-01', '2004-12-31'):
        with pytest.raises(ValueError, match='must start on'):
            sp.run_simply_p_ensemble(*helpers.scenario_inputs('tarland_2004_dynamic'), n_members=3,
                                     initial_state=_state_dict(end=end))
    with pytest.raises(ValueError, match='must start on'):
        sp.run_simply_p(*helpers.scenario_inputs('tarland_2004_dynamic'), initial_state=_state_dict(E=1, end='2003-06-30'))


def test_initial_state_with_other_reaches_or_shape_is_refused_before_any_device_is_touched(no_device):
    with pytest.raises(ValueError, match='reaches'):
        sp.run_simply_p_ensemble(*helpers.scenario_inputs('tarland_2004_dynamic'), n_members=3,
                                 initial_state=_state_dict(reaches=(2,)))
    with pytest.raises(ValueError, match='reaches'):
        sp.run_simply_p_ensemble(*helpers.scenario_inputs('chain4_val_2004'), n_members=3, initial_state=_state_dict())
    for shape in ((1, 16, 4), (1, 15, 3), (2, 16, 3), (16, 3)):
        with pytest.raises(ValueError, match='shape'):
            sp.run_simply_p_ensemble(*helpers.scenario_inputs('tarland_2004_dynamic'), n_members=3, initial_state=np.ones(shape))
        with pytest.raises(ValueError, match='shape'):
            st = _state_dict()
            st['data'] = np.ones(shape)
            sp.run_simply_p_ensemble(*helpers.scenario_inputs('tarland_2004_dynamic'), n_members=3, initial_state=st)
    # split over devices: the blocks of a list must be the member blocks of the run
    with pytest.raises(ValueError, match='blocks'):
        sp.run_simply_p_ensemble(*helpers.scenario_inputs('tarland_2004_dynamic'), n_members=3, devices=[0, 0],
                                 initial_state=[np.ones((1, 16, 1)), np.ones((1, 16, 2))])


def test_windows_refuse_bad_arguments_when_created(no_device):
    args = helpers.scenario_inputs('tarland_2004_dynamic')
    with pytest.raises(ValueError, match='period'):
        sp.run_simply_p_ensemble_windows(*args, window=100, n_members=3, reduce='annual')
    with pytest.raises(ValueError):
        sp.run_simply_p_ensemble_windows(*args, window='weekly', n_members=3)
