"""The model's right-hand side as a plain high-precision statement, and the rows the device's and the oracle's statements of it are
held to point by point (tests/test_rhs_host.py, tests/test_gpu_rhs.py).

`statement` evaluates the 12 equations in mpmath at 40 digits, written from the equations as simplyp_amd.model.ode_f states them.
For every component it returns the value AND M, the sum of the absolute values of its additive terms: the scale a rounding error of
a correctly written fp evaluation is proportional to (a component that is a small difference of large terms may be wrong by a
rounding of the large terms, not of the small result).  Where a term carries Qr**b -- evaluated everywhere as exp(b ln Qr), whose
relative error grows with |b ln Qr| (tests/test_gpu_elementary.py::test_pow_as_the_right_hand_side_forms_it) -- its share of M is
multiplied by 1 + |b ln Qr|.

The bound every form is held to:   |got_i - want_i| <= K u M_i + G_i,   K = 64, u = 2^-53 (2^-24 for the fp32 form), and G_i the
gate allowance: the largest change of component i when the clamped argument s of each of the three gates is shifted by one ulp
of 100 (2^-46; 2^-17 in fp32) either way -- s is a difference of two numbers near threshold / d = 100, and one rounding at that
magnitude is inherent in every form.  The counting behind K is in the docstring of tests/test_gpu_rhs.py."""

import functools
import os

import mpmath
import numpy as np

from mpmath import mpf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DPS = 40
K = 64
U64, U32 = 2.0 ** -53, 2.0 ** -24
S_ULP64, S_ULP32 = 2.0 ** -46, 2.0 ** -17          # one ulp of 100 in fp64 / fp32

V = np.load(os.path.join(GOLDEN, 'unit_vectors.npz'), allow_pickle=False)
NAMES = [str(n) for n in V['ode_p_names']]
IX = {n: i for i, n in enumerate(NAMES)}
Y8_OF_Y12 = [0, 1, 2, 3, 4, 6, 8, 10]               # VsA VsS Vg Vr Qr Msus TDPr PPr in the reference's 12 slots

# component names in the order each form returns them
LITERAL = ['dVsA', 'dVsS', 'dVg', 'dVr', 'dQr', 'dMsus', 'dTDPr', 'dPPr', 'Qr', 'oM', 'oT', 'oP']           # rhs: dy[8], q[4]
ORACLE_F = ['dVsA', 'dVsS', 'dVg', 'dVr', 'dQr', 'Qr', 'dMsus', 'oM', 'dTDPr', 'oT', 'dPPr', 'oP']          # ode_f's 12 slots
AUG = ['dVsA', 'dVsS', 'dVg', 'dQr', 'dMsus_i', 'dTDPr_i', 'dPPr_i', 'dEA', 'dES', 'dpb', 'dpk', 'Qr', 'oM_i', 'oT_i', 'oP_i']
AUG_CQ = [n if n != 'dpb' else 'dpbc' for n in AUG]                                 # SysAug::f carries cQ Qr**b_Q
# quad_rhs: lane j's d[3] and qv, as components of the augmented form (lane 3's third slot is empty)
QUAD = [['dVsA', 'dEA', 'dMsus_i', 'oM_i'], ['dVsS', 'dES', 'dTDPr_i', 'oT_i'], ['dVg', 'dpk', 'dPPr_i', 'oP_i'],
        ['dQr', 'dpbc', None, 'Qr']]


def _gate(x, th, shift):
    """f_x(x, th, 0.01) with the clamped argument shifted; threshold 0 is a plain step (1 above 0, else 0)."""
    d = th * mpf('0.01')
    if d == 0:
        return mpf(1) if x > th else mpf(0), None
    s = (x - th) / d
    sc = min(max(s + shift, mpf(0)), mpf(1))
    return 3 * sc ** 2 - 2 * sc ** 3, s


def statement(y8, p43, shifts=(0, 0, 0)):
    """{name: (value, M)} in mpf, and the three gates' unclamped arguments s (None for a plain step).  Names: the literal form's
    dVsA dVsS dVg dVr dQr dMsus dTDPr dPPr Qr oM oT oP with Vr as given; with the suffix _i the reach masses' components with Vr
    on its invariant L_reach / (a_Q 86400) Qr**(1 - b_Q); dEA dES dpb dpk, the derivatives of exp(-mu VsA), exp(-mu VsS),
    Qr**b_Q, Qr**k_M along the solution, and dpbc = cQ dpb."""
    with mpmath.workdps(DPS):
        y = [mpf(float(v)) for v in y8]
        p = {n: mpf(float(p43[i])) for n, i in IX.items()}
        nc = int(p43[IX['NC_type']])
        VsA, VsS, Vg, Vr, Qr, Msus, TDPr, PPr = y
        fc, beta = p['fc'], p['beta']
        gA, sA = _gate(VsA, fc, mpf(shifts[0]))
        gS, sS = _gate(VsS, fc, mpf(shifts[1]))
        QsA = (VsA - fc) * gA / p['T_s_A']
        QsS = (VsS - fc) * gS / p['T_s_S']
        c0, aE = p['P'] * (1 - p['f_quick']), p['alpha'] * p['E']
        EA, ES = mpmath.exp(-p['mu'] * VsA), mpmath.exp(-p['mu'] * VsS)
        out = {}
        out['dVsA'] = (c0 - aE * (1 - EA) - QsA, abs(c0) + abs(aE) + abs(aE * EA) + abs(QsA))
        out['dVsS'] = (c0 - aE * (1 - ES) - QsS, abs(c0) + abs(aE) + abs(aE * ES) + abs(QsS))
        QsNC = QsA if nc == 1 else QsS
        fg, sG = _gate(Vg / p['T_g'], p['Qg_min'], mpf(shifts[2]))
        Qg = (1 - fg) * p['Qg_min'] + fg * (Vg / p['T_g'])
        M_Qg = abs((1 - fg) * p['Qg_min']) + abs(fg * (Vg / p['T_g']))
        Qsum = p['f_A'] * QsA + p['f_S'] * QsS
        M_Qsum = abs(p['f_A'] * QsA) + abs(p['f_S'] * QsS)
        out['dVg'] = (beta * Qsum - Qg, abs(beta) * M_Qsum + M_Qg)
        inflow = p['Qq'] + (1 - beta) * Qsum + Qg + p['Qr_US'] - Qr
        M_in = abs(p['Qq']) + abs(1 - beta) * M_Qsum + M_Qg + abs(p['Qr_US']) + abs(Qr)
        out['dVr'] = (inflow, M_in)
        lnQ = mpmath.log(Qr)
        amp_b, amp_k = 1 + abs(p['b_Q'] * lnQ), 1 + abs(p['k_M'] * lnQ)
        pb, pk = mpmath.exp(p['b_Q'] * lnQ), mpmath.exp(p['k_M'] * lnQ)
        cQ = p['a_Q'] * 86400 / ((1 - p['b_Q']) * p['L_reach'])
        out['dQr'] = (inflow * cQ * pb, M_in * abs(cQ * pb) * amp_b)
        out['Qr'] = (Qr, abs(Qr))
        MA, MS, MIG = p['Esus_A'] * pk, p['Esus_S'] * pk, p['Esus_IG'] * pk
        src_M = p['f_Ar'] * MA + p['f_IG'] * MIG + p['f_S'] * MS
        M_src_M = (abs(p['f_Ar'] * MA) + abs(p['f_IG'] * MIG) + abs(p['f_S'] * MS)) * amp_k
        wA, wNa, wNs = p['f_A'] * (1 - p['f_NC_A']), p['f_A'] * p['f_NC_A'], p['f_S'] * p['f_NC_S']
        cA, cN = p['conc_TDPs_A'], p['conc_TDPs_NC']
        tdp_terms = [(1 - beta) * wA * QsA * cA, (1 - beta) * wNa * QsNC * cN, (1 - beta) * wNs * QsNC * cN,
                     wA * p['Qq'] * cA, wNa * p['Qq'] * cN, wNs * p['Qq'] * cN, p['TDPeff'], p['TDPr_US']]
        tg = p['TDPg'] * p['A_catch']
        src_T = sum(tdp_terms) + Qg * tg
        M_src_T = sum(abs(t) for t in tdp_terms) + M_Qg * abs(tg)
        pA, pN, p0 = (p['Plab_A'] + p['P_inactive']) / p['Msoil'], (p['Plab_NC'] + p['P_inactive']) / p['Msoil'], \
            p['P_inactive'] / p['Msoil']
        pp_terms = [p['f_Ar'] * (1 - p['f_NC_Ar']) * MA * pA, p['f_IG'] * (1 - p['f_NC_IG']) * MIG * pA,
                    p['f_S'] * (1 - p['f_NC_S']) * MS * p0, p['f_Ar'] * p['f_NC_Ar'] * MA * pN,
                    p['f_IG'] * p['f_NC_IG'] * MIG * pN, p['f_S'] * p['f_NC_S'] * MS * pN]
        src_P = p['E_PP'] * sum(pp_terms)
        M_src_P = abs(p['E_PP']) * sum(abs(t) for t in pp_terms) * amp_k
        # the reach's three masses: with Vr as given (the literal form), and with Vr on its invariant (the augmented forms),
        # where Qr / Vr = Qr**b_Q a_Q 86400 / L_reach carries Qr**b_Q
        kap_lit = Qr / Vr
        kap_inv = pb * p['a_Q'] * 86400 / p['L_reach']
        for sfx, kap, amp in (('', kap_lit, mpf(1)), ('_i', kap_inv, amp_b)):
            oM, oT, oP = Msus * kap, TDPr * kap, PPr * kap
            out['oM' + sfx], out['oT' + sfx], out['oP' + sfx] = (oM, abs(oM) * amp), (oT, abs(oT) * amp), (oP, abs(oP) * amp)
            out['dMsus' + sfx] = (src_M + p['Msus_US'] - oM, M_src_M + abs(p['Msus_US']) + abs(oM) * amp)
            out['dTDPr' + sfx] = (src_T - oT, M_src_T + abs(oT) * amp)
            out['dPPr' + sfx] = (src_P + p['PPr_US'] - oP, M_src_P + abs(p['PPr_US']) + abs(oP) * amp)
        # the carried functions' own equations: d exp(-mu Vs) = -mu E dVs;  d Qr**b = b Qr**b dQr / Qr (Qr**b enters twice)
        out['dEA'] = (-p['mu'] * EA * out['dVsA'][0], abs(p['mu'] * EA) * out['dVsA'][1])
        out['dES'] = (-p['mu'] * ES * out['dVsS'][0], abs(p['mu'] * ES) * out['dVsS'][1])
        r, M_r = out['dQr'][0] / Qr, M_in * abs(cQ * pb / Qr)
        out['dpb'] = (p['b_Q'] * pb * r, abs(p['b_Q'] * pb) * M_r * (2 * amp_b - 1))
        out['dpbc'] = (cQ * out['dpb'][0], abs(cQ) * out['dpb'][1])
        out['dpk'] = (p['k_M'] * pk * r, abs(p['k_M'] * pk) * M_r * (amp_b + amp_k - 1))
        return out, (sA, sS, sG)


def invariant_vr(qr, p43):
    """Vr = L_reach / (a_Q 86400) Qr**(1 - b_Q), rounded once."""
    with mpmath.workdps(DPS):
        L, a, b = (mpf(float(p43[IX[n]])) for n in ('L_reach', 'a_Q', 'b_Q'))
        return float(L / (a * 86400) * mpmath.power(mpf(float(qr)), 1 - b))


class Truth(object):
    """The statement on a list of rows: value, M and gate allowance G of every component, as numpy object arrays of mpf."""

    def __init__(self, rows, s_ulp):
        self.names = sorted(statement(rows[0][:8], rows[0][8:])[0])
        n = len(rows)
        self.val = {k: np.empty(n, dtype=object) for k in self.names}
        self.M = {k: np.empty(n, dtype=object) for k in self.names}
        self.G = {k: np.empty(n, dtype=object) for k in self.names}
        self.s = np.full((n, 3), np.nan)
        for i, row in enumerate(rows):
            base, s = statement(row[:8], row[8:])
            g = {k: mpf(0) for k in self.names}
            for gate in range(3):
                if s[gate] is None:
                    continue
                self.s[i, gate] = float(s[gate])
                if not (-2 * s_ulp <= s[gate] <= 1 + 2 * s_ulp):
                    continue                                          # clamped either way: a shift changes nothing
                worst = {k: mpf(0) for k in self.names}
                for sign in (-1, 1):
                    sh = [0, 0, 0]
                    sh[gate] = sign * s_ulp
                    moved = statement(row[:8], row[8:], sh)[0]
                    for k in self.names:
                        worst[k] = max(worst[k], abs(moved[k][0] - base[k][0]))
                for k in self.names:
                    g[k] += worst[k]                                  # the three gates' shifts in their worst combination
            for k in self.names:
                self.val[k][i], self.M[k][i], self.G[k][i] = base[k][0], base[k][1], g[k]

    def ratios(self, got, names, u, rows=None, allowance=True):
        """|got - want| beyond the gate allowance, in units of u M: [rows, components] (nan where a form has no such component).
        A component whose M is 0 must be exact (ratio 0, or inf).  allowance=False: without the gate allowance."""
        got = np.asarray(got, dtype=np.float64)
        idx = range(got.shape[0]) if rows is None else rows
        out = np.full((got.shape[0], len(names)), np.nan)
        with mpmath.workdps(DPS):
            for r, i in enumerate(idx):
                for c, k in enumerate(names):
                    if k is None:
                        continue
                    g = got[r, c]
                    if not np.isfinite(g):
                        out[r, c] = np.inf
                        continue
                    over = abs(mpf(float(g)) - self.val[k][i]) - (self.G[k][i] if allowance else 0)
                    if over <= 0:
                        out[r, c] = 0.0
                    else:
                        out[r, c] = float(over / (u * self.M[k][i])) if self.M[k][i] > 0 else np.inf
        return out


def worst(ratio, names, labels):
    """(largest ratio, its component, its row's label) for a message."""
    r = np.where(np.isnan(ratio), -1.0, ratio)
    i, c = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i, c]), names[c], labels[i]


# ---- the rows ---------------------------------------------------------------------------------------------------------------

RATIOS = [1 - 2.0 ** -30, 1.0, 1 + 2.0 ** -52, 1.005, 1.01, 1.01 * (1 + 2.0 ** -52), 1.2]
UPSTREAM = {'Qr_US': 0.7, 'Msus_US': 1.0e3, 'TDPr_US': 0.05, 'PPr_US': 0.4}


def _variations():
    """[(label, function(y8, p) changing both in place, Vr-on-its-invariant flag)]: the edges, one at a time."""
    out = []

    def put_on_invariant(y, p):
        y[3] = invariant_vr(y[4], p)

    def soil(slot, r):
        def f(y, p):
            y[slot] = p[IX['fc']] * r
            put_on_invariant(y, p)
        return f

    def gw(r):
        def f(y, p):
            if p[IX['Qg_min']] <= 0.0:
                p[IX['Qg_min']] = 0.02
            y[2] = p[IX['T_g']] * p[IX['Qg_min']] * r
            put_on_invariant(y, p)
        return f

    def gw0(vg):
        def f(y, p):
            p[IX['Qg_min']] = 0.0
            y[2] = vg
            put_on_invariant(y, p)
        return f

    def reach(qr, off):
        def f(y, p):
            y[4] = qr
            y[3] = invariant_vr(qr, p) * off
        return f

    def forcing(P, E):
        def f(y, p):
            p[IX['P']], p[IX['E']] = P, E
            p[IX['Qq']] = p[IX['f_quick']] * P
            put_on_invariant(y, p)
        return f

    def upstream(on):
        def f(y, p):
            for k, v in UPSTREAM.items():
                p[IX[k]] = v if on else 0.0
            put_on_invariant(y, p)
        return f

    def nc(t):
        def f(y, p):
            p[IX['NC_type']] = float(t)
            p[IX['f_NC_Ar']], p[IX['f_NC_IG']], p[IX['f_NC_S']] = 0.3, 0.2, 0.4
            p[IX['f_NC_A']] = p[IX['f_Ar']] * 0.3 + 0.2 * p[IX['f_IG']]                  # model.py:319
            if p[IX['conc_TDPs_NC']] == 0.0:
                p[IX['conc_TDPs_NC']] = 0.6 * p[IX['conc_TDPs_A']]
            if p[IX['Plab_NC']] == 0.0:
                p[IX['Plab_NC']] = 0.5 * p[IX['Plab_A']]
            put_on_invariant(y, p)
        return f

    for i, r in enumerate(RATIOS):
        out.append(('VsA/fc#%d' % i, soil(0, r), True))
    for i, r in enumerate(RATIOS):
        out.append(('VsS/fc#%d' % i, soil(1, r), True))
    for i, r in enumerate(RATIOS):
        out.append(('Vg/Tg/Qgmin#%d' % i, gw(r), True))
    for vg in (-1e-3, 0.0, 1e-300, 1e-3):
        out.append(('Qgmin=0,Vg=%g' % vg, gw0(vg), True))
    for qr in (1e-6, 1e-3, 1.0, 50.0):
        out.append(('Qr=%g' % qr, reach(qr, 1.0), True))
    for qr in (1e-6, 50.0):
        for off in (0.9, 1.1):
            out.append(('Qr=%g,Vr x %g' % (qr, off), reach(qr, off), False))
    out.append(('P=PET=0', forcing(0.0, 0.0), True))
    out.append(('P=80', forcing(80.0, 1.5), True))
    out.append(('upstream=0', upstream(False), True))
    out.append(('upstream>0', upstream(True), True))
    for t in (0, 1, 2):
        out.append(('NC_type=%d' % t, nc(t), True))
    return out


def _below_zone(y, p):
    """Everything below its gate, no forcing: QsA = QsS = 0 and Qg = Qg_min exactly."""
    p[IX['P']] = p[IX['E']] = p[IX['Qq']] = 0.0
    if p[IX['Qg_min']] <= 0.0:
        p[IX['Qg_min']] = 0.02
    y[0] = y[1] = p[IX['fc']] * RATIOS[0]
    y[2] = p[IX['T_g']] * p[IX['Qg_min']] * RATIOS[0]
    y[3] = invariant_vr(y[4], p)


@functools.lru_cache(maxsize=None)
def rows():
    """(rows [n, 51], labels, Vr-on-its-invariant flags [n], below-the-zone flags [n]): the 96 fixture rows as recorded; around
    fixture row i five of the 40 edge variations (variation v where (v + i) % 8 == 0, so every variation meets 12 different
    rows); and 12 rows with everything below its gate."""
    fy, fp = V['ode_y'][:, Y8_OF_Y12], V['ode_p']
    R, labels, inv, below = [], [], [], []
    for i in range(len(fy)):
        R.append(np.concatenate([fy[i], fp[i]]))
        labels.append('fixture %d' % i)
        inv.append(False)
        below.append(False)
    var = _variations()
    for i in range(len(fy)):
        for v, (label, f, on) in enumerate(var):
            if (v + i) % 8:
                continue
            y, p = fy[i].copy(), fp[i].copy()
            f(y, p)
            R.append(np.concatenate([y, p]))
            labels.append('fixture %d, %s' % (i, label))
            inv.append(on)
            below.append(False)
    for i in range(0, len(fy), 8):
        y, p = fy[i].copy(), fp[i].copy()
        _below_zone(y, p)
        R.append(np.concatenate([y, p]))
        labels.append('fixture %d, below every gate' % i)
        inv.append(True)
        below.append(True)
    return np.array(R), labels, np.array(inv), np.array(below)


@functools.lru_cache(maxsize=None)
def rows_f32():
    """The same rows with every input rounded to fp32 first: the statement and the fp32 form then see the same numbers."""
    R, labels, inv, below = rows()
    with np.errstate(over='ignore', under='ignore'):
        return R.astype(np.float32).astype(np.float64), labels, inv, below


@functools.lru_cache(maxsize=None)
def truth():
    return Truth(rows()[0], S_ULP64)


@functools.lru_cache(maxsize=None)
def truth_f32():
    return Truth(rows_f32()[0], S_ULP32)


def y12_of(row):
    """The reference's 12-slot state of a row (the four daily integrals, which no right-hand side reads, at 0)."""
    y = np.zeros(12)
    y[Y8_OF_Y12] = row[:8]
    return y
