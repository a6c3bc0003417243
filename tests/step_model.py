"""The pieces of the step rule that the one-lane and the four-lane kernel share (simplyp_kernels.hip.h: ck_open_step, ck_propose,
ck_choose_pair, ck_damping, ck_step_factor) in plain Python, from the rules as include/simplyp_controller.h and the oracle's
erk_aug_day state them; the constants are parsed from the header.  Where the device runs its own reciprocal (one Newton step:
sp_rcp1, or the raw seed) the model divides, and tests/test_gpu_step_pieces.py grants that reciprocal's own bar
(tests/elementary.py: SEED_ERR); everything else is the same IEEE operations and compared exactly."""

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'include', 'simplyp_controller.h')) as fh:
    C = {k: float(v) for k, v in re.findall(r'#define SIMPLYP_((?:CTRL|STIFF|DAMP)_[A-Z0-9_]+) \(?(-?[0-9.e+-]+)\)?\s', fh.read())}
with open(os.path.join(ROOT, 'simplyp_amd', 'csrc', 'simplyp_kernels.hip.h')) as fh:
    TAB_STRIDE = int(re.search(r'constexpr int TAB_STRIDE = (\d+);', fh.read()).group(1))

N_IN, N_OUT = 19, 11
# input columns
OPEN, PROPOSE, CHOOSE, DAMP, FACTOR = 0, 3, 6, 11, 17
BENIGN = np.array([0.1, 1.0, 1.0, 0.1, 1.0, 1.1, 0.1, 1.0, 0, 0, 1, 0.5, 1.0, 0.0, 1.0, 1.0, 0.5, 1.0, 0], dtype=np.float64)


def rows_of(first, cases):
    """Rows that carry `cases` [n, k] from column `first` on and benign arguments elsewhere."""
    cases = np.atleast_2d(np.asarray(cases, dtype=np.float64))
    R = np.tile(BENIGN, (len(cases), 1))
    R[:, first:first + cases.shape[1]] = cases
    return R


def open_step(h_carry, T, rate, kink_aware, stiff, real=np.float64):
    """(the opening step with an exact reciprocal, whether the reciprocal entered).  real = float32: integrator 3."""
    T, rate = real(T), real(rate)
    h = real(h_carry)
    if kink_aware:
        h = real(h * real(C['CTRL_DAY_START']))
    if not (h > 0) or h > T:
        h = T
    if stiff:
        h0 = C['STIFF_Z_START'] / float(rate)
        if float(h) > h0:
            return h0, True
    return float(h), False


def propose(h, rem, c11):
    hh = h
    if rem < 2.0 * h:
        hh = 0.5 * rem
    if rem <= c11 * h:
        hh = rem
    return hh


def choose_pair(hh, rate, kneeish, last_chance, alive):
    """(hh after, whether it is the reciprocal's Z_ON / rate, toff, flag)"""
    longstep = hh * rate > C['STIFF_Z_ON']
    second = longstep and not kneeish
    cut = longstep and kneeish and not last_chance and alive
    return (C['STIFF_Z_ON'] / rate if cut else hh), cut, (TAB_STRIDE if second else 0), second


def damping(bQ, Qr, dQr, rate, T, left):
    lam = min(rate - (bQ * dQr) / Qr, rate)
    F = min((lam * T) * (1.0 / C['DAMP_PHI']), lam * left + 1.0)
    return min(max(F, 1.0), C['DAMP_FMAX'])


def step_factor(err, second):
    """(the factor SAFETY err**exponent clamped, t = exponent log2(err)) with the exponent as the fp32 number the device holds."""
    fexp = float(np.float32(C['STIFF_ERR_EXP'] if second else -0.2))
    lo, hi = float(np.float32(C['CTRL_FAC_MIN'])), float(np.float32(C['CTRL_FAC_MAX']))
    if err == 0.0:
        return hi, np.inf
    if np.isinf(err):
        return lo, -np.inf
    t = fexp * np.log2(err)
    return min(max(C['CTRL_SAFETY'] * 2.0 ** t, lo), hi), t
