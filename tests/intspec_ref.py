"""INTSPEC, ROTSPEC and STRSPEC (intspec.F90:107-229, rotspec.F90:69-86, strspec.F90:70-175) restated in numpy, in the reference's
order of operations and in the precision asked for (np.float32 or np.float64): TEST INFRASTRUCTURE, the expected values of
tests/test_nest_host.py and tests/test_gpu_nest.py.  Spectra are [M][K] (the order of the boundary file's records); every scalar is kept
in the working precision, so that the result is what a compiler without contraction computes, up to the transcendental functions
(COS, SIN, ATAN2 feed the rotation weights; LOG10 only feeds INT()).
"""
from __future__ import annotations

import numpy as np

# |restatement - the reference's own INTSPEC| over the 96 cases of tests/golden/intspec_nang12.npz, float64 against its double and float32
# against its single precision build (tests/test_nest_host.py measures and prints them): per bin over the spectrum's peak, the DFIM-weighted
# sum of the differences over the energy, THQ [radians, modulo 2 PI]; EMEAN and FMEAN agree in every bit.  The differences are those of
# COS / SIN / ATAN2 between two mathematical libraries, through the rotation weight.  The gates are three times these figures.
MEASURED = dict(dp=dict(bin=3.54e-15, energy=3.35e-15, thq=1.78e-15), sp=dict(bin=1.91e-6, energy=2.11e-6, thq=9.54e-7))
GATE = {p: {k: 3 * v for k, v in m.items()} for p, m in MEASURED.items()}


def _powi(b, n):
    """b**n with an integer n as compilers lower it: by squaring, the reciprocal last."""
    T = type(b)
    e, r = abs(int(n)), T(1)
    while True:
        if e & 1:
            r = T(r * b)
        e //= 2
        if e == 0:
            break
        b = T(b * b)
    return T(T(1) / r) if n < 0 else r


def rotspec(f1: np.ndarray, rthet) -> np.ndarray:
    T = f1.dtype.type
    ML, KL = f1.shape
    zpi = T(T(8) * np.arctan(T(1)))
    fth = T(np.fmod(T(T(rthet) + zpi), zpi))
    fth = T(T(fth * T(KL)) / zpi)
    inc = int(fth)
    adif = T(fth - T(inc))
    bdif = T(T(1) - adif)
    kc = np.arange(1, KL + 1) - inc
    kc[kc < 1] += KL
    kc1 = kc - 1
    kc1[kc1 < 1] += KL
    return bdif * f1[:, kc - 1] + adif * f1[:, kc1 - 1]


def strspec(fr: np.ndarray, fl: np.ndarray, gamma) -> np.ndarray:
    T = fl.dtype.type
    gamma = T(gamma)
    if gamma == T(1):
        return fl
    ML, KL = fl.shape
    ar1 = np.zeros_like(fl)
    alo = T(np.log10(T(1.1)))
    inc = int(T(T(np.log10(gamma)) / alo))
    z = T(abs(T(_powi(T(1.1), inc) - gamma)))
    ar2 = (fr * gamma).astype(T)
    if z <= T(0.001):
        if gamma > T(1):
            for m in range(1, ML - inc + 1):
                ar1[m - 1] = fl[m + inc - 1]
        else:
            for m in range(1 - inc, ML + 1):
                ar1[m - 1] = fl[m + inc - 1]
    else:
        up = gamma > T(1)
        for m in (range(1, ML - inc) if up else range(2 - inc, ML + 1)):
            ifr = int(T(T(T(np.log10(T(ar2[m - 1] / fr[0]))) / alo) + T(1)))
            mc = m + inc if up else m + inc - 1
            adif = T(T(fr[ifr] - ar2[m - 1]) / T(fr[ifr] - fr[ifr - 1]))
            bdif = T(T(1) - adif)
            ar1[m - 1] = adif * fl[mc - 1] + bdif * fl[mc]
    return ar1


def intspec(fr, del1l, f1, fmean1, emean1, thetm1, f2, fmean2, emean2, thetm2, dtype):
    """(FL [M][K], FMEAN, EMEAN, THETM) of INTSPEC with DEL12 = 1, in `dtype`."""
    T = np.dtype(dtype).type
    fr = np.asarray(fr, dtype=T)
    f1, f2 = np.asarray(f1, dtype=T), np.asarray(f2, dtype=T)
    del12, del1l = T(1), T(del1l)
    fmean1, emean1, thetm1, fmean2, emean2, thetm2 = (T(x) for x in (fmean1, emean1, thetm1, fmean2, emean2, thetm2))
    zpi = T(T(8) * np.arctan(T(1)))
    gw1 = T(T(del12 - del1l) / del12)
    gw2 = T(del1l / del12)
    if emean1 == T(0):
        return gw2 * f2, fmean2, T(gw2 * emean2), thetm2
    if emean2 == T(0):
        return gw1 * f1, fmean1, T(gw1 * emean1), thetm1
    emean = T(T(gw1 * emean1) + T(gw2 * emean2))
    fmean = T(T(gw1 * fmean1) + T(gw2 * fmean2))
    cm = T(T(gw1 * T(np.cos(thetm1))) + T(gw2 * T(np.cos(thetm2))))
    sm = T(T(gw1 * T(np.sin(thetm1))) + T(gw2 * T(np.sin(thetm2))))
    thetm = T(np.arctan2(sm, cm))
    thetm = T(np.fmod(T(thetm + zpi), zpi))
    with np.errstate(all="ignore"):
        f3 = strspec(fr, rotspec(f1, T(thetm - thetm1)), T(fmean1 / fmean)) * T(emean / emean1)
        f4 = strspec(fr, rotspec(f2, T(thetm - thetm2)), T(fmean2 / fmean)) * T(emean / emean2)
    return gw1 * f3 + gw2 * f4, fmean, emean, thetm


def bouinpt_point(fr, bfw, ibcl, ibcr, f1, par1, dtype):
    """One boundary point of bouinpt.F90:385-424: (FL [M][K], (EMEAN, THQ, FMEAN)); f1 [nboinp][M][K], par1 [nboinp][3] = EMEAN, THQ, FMEAN;
    index 0 = the land point.  Where the left spectrum is copied the means are the left point's."""
    T = np.dtype(dtype).type
    zero = np.zeros(f1.shape[1:], dtype=T)

    def side(i):
        return (zero, T(0), T(0), T(0)) if i == 0 else (np.asarray(f1[i - 1], dtype=T), T(par1[i - 1][0]), T(par1[i - 1][1]), T(par1[i - 1][2]))

    fa, ea, ta, ma = side(int(ibcl))
    if not T(bfw) > T(0):
        return fa.copy(), (ea, ta, ma)
    fb, eb, tb, mb = side(int(ibcr))
    fl, fm, em, th = intspec(fr, bfw, fa, ma, ea, ta, fb, mb, eb, tb, dtype)
    return fl, (em, th, fm)


def errors(got, ref, dfim):
    """The two error figures of a point, spectra [M][K]: per bin |got - ref| over the peak of ref (the maximum over the bins), and the
    DFIM-weighted sum of |got - ref| over the energy of ref (its DFIM-weighted sum)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    w = np.asarray(dfim, dtype=np.float64)[:, None]
    return float(d.max() / np.abs(ref).max()), float((d * w).sum() / (ref * w).sum())


# ---- inputs without knife edges (STRSPEC's INT(LOG10(GAMMA)/LOG10(1.1)) is discontinuous where GAMMA nears a power of 1.1): each of the two GAMMAs
# of a case is 1.1**(n+f) with f in [0.1, 0.9] and n in -3 .. 2 (the interpolating branch), 1.1**n (1 +- 3e-4) with the sign away from zero (the
# pure shift), or 1 (both of them then); GW1 GAMMA1 + GW2 GAMMA2 = 1 ties the weight to the pair.  Shared by tools/make_golden_nest.py (the
# fixture's inputs) and tests/test_gpu_nest.py (the 36-direction cases).
INTERP, SHIFT, ONE = 0, 1, 2


def gamma_of(form, n, f, sign):
    if form == INTERP:
        return 1.1 ** (n + f)
    if form == SHIFT:
        return 1.1 ** n * (1 + sign * 3e-4)
    return 1.0


def _pick(rng, above):
    """(form, n, f, sign) of a GAMMA above / below 1"""
    if rng.random() < 0.6:
        return INTERP, int(rng.integers(0, 3) if above else rng.integers(-3, 0)), float(rng.uniform(0.1, 0.9)), 0
    n = int(rng.integers(0, 3) if above else rng.integers(-3, 1))
    return SHIFT, n, 0.0, (1 if above else -1)


def spectrum(rng, fr, th):
    """A peaked spectrum [M][K] with 20 % noise, float32-representable."""
    fr, th = np.asarray(fr, dtype=np.float64), np.asarray(th, dtype=np.float64)
    fp = rng.uniform(0.06, 0.35)
    thp = rng.uniform(0, 2 * np.pi)
    s = rng.uniform(1.0, 4.0)
    e = (fr / fp) ** -5.0 * np.exp(-1.25 * (fr / fp) ** -4.0)
    d = np.maximum(np.cos(th - thp), 0.0) ** (2 * s)
    a = rng.uniform(0.05, 3.0) * e[:, None] * d[None, :] * rng.uniform(0.8, 1.2, (fr.size, th.size))
    return a.astype(np.float32)


def make_cases(rng, ncase, fr, th):
    """(bfw [n], f [n][2][M][K], par [n][2][3] = EMEAN, THQ, FMEAN, form [n][2][4] = the construction), all float32 but form."""
    nfre, nang = len(fr), len(th)
    bfw = np.zeros(ncase, np.float32)
    f = np.zeros((ncase, 2, nfre, nang), np.float32)
    par = np.zeros((ncase, 2, 3), np.float32)
    form = np.zeros((ncase, 2, 4))
    for i in range(ncase):
        if i % 12 == 11:
            g = [(ONE, 0, 0.0, 0), (ONE, 0, 0.0, 0)]
            w2 = float(rng.choice([0.25, 0.5, 0.75]))   # GW1 F + GW2 F = F exactly
        else:
            first_above = bool(rng.integers(0, 2))
            g = [_pick(rng, first_above), _pick(rng, not first_above)]
            g1, g2 = gamma_of(*g[0]), gamma_of(*g[1])
            w2 = (1.0 - g1) / (g2 - g1)
        fm = float(rng.uniform(0.08, 0.3))
        bfw[i] = w2
        for s in range(2):
            f[i, s] = spectrum(rng, fr, th)
            par[i, s] = (rng.uniform(0.05, 4.0), rng.uniform(0, 2 * np.pi), gamma_of(*g[s]) * fm)
            form[i, s] = g[s]
    return bfw, f, par, form
