"""numpy restatement of the output spectrum FL2ND of OUTBLOCK (outblock.F90:159-194): what ecwam_hip_outbs_absolute builds on the chip
before it computes the parameters that read FL2ND.  In the working precision of the tables, vectorised over points, with the loops over M
and K in the reference's order.  Test infrastructure only: the device kernel is checked against it.

  INTPOL, IRA = 1    intpol.F90:98-115 (constants, NFRE_MAX, DFTH), :129-148 (LICE2SEA, FLA = 0), :153-169 (source frequency, wave number,
                     f**-5 factor), :179-198 (FNEF, KNEW, NEWF), :202-244 (OLDFL, the four cases of GWM / GWP), :249-255 (the scatter),
                     :265-271 (MAX(FLA, EPSMIN)); CURRENT_MAX yowcurr.F90:18
  ice reshaping      outblock.F90:175-194

The consumers are not restated here: consumers() applies oracle.outbs (FEMEAN, STHQ, DOMINANT_PERIOD) and columns 0-2 of
sepwisw_ref.sepwisw (MWP1, MWP2, WDIRSPREAD with LLPEAKF = F) to the restated FL2ND.
"""
from __future__ import annotations

import numpy as np

import sepwisw_ref as S
from ecwam_amd.tables import powi

FIELDS = ("swh", "mwd", "mwp", "em", "pp1d", "mp1", "mp2", "wdw")
CURRENT_MAX = 1.5     # yowcurr.F90:18
CASES = ("interior", "below", "top", "outside", "flip")


def nfre_max(t) -> int:
    """NFRE_MAX, intpol.F90:103-105."""
    T = t.dtype
    fmax = t.FR[-1] + (t.ZPI / t.G) * (t.FR[-1] * t.FR[-1]) * T(CURRENT_MAX)
    return int(np.floor(np.log10(fmax / t.FR[0]) * t.FLOGSPRDM1)) + 1


def intpol(t, fl1, wavnum, ucur, vcur, m_last: int | None = None):
    """INTPOL(FLR = fl1 -> FLA, WAVNUM, UCUR, VCUR, IRA = 1).  Returns (FLA [n][NANG][NFRE], info): info["cases"][name] = how many
    (point, K, M) sources with OLDFL > 0 took each of the four NEWM cases, and how many changed direction; info["nfre_max"].
    m_last: the last source frequency of the loop (default NFRE_MAX; NFRE gives the transform without the tail beyond FR(NFRE))."""
    T = t.dtype
    fl1 = np.asarray(fl1, T)
    wavnum = np.asarray(wavnum, T)
    u = np.asarray(ucur, T)
    v = np.asarray(vcur, T)
    n, K, M = fl1.shape
    rows = np.arange(n)
    one = T(1.0)
    FR, FRATIO, EPS = t.FR, t.FRATIO, t.EPSMIN
    fre0 = FRATIO - one
    zpi2gm = (t.ZPI * t.ZPI) / t.G
    coef = one / t.ZPI
    nmax = nfre_max(t)
    cdf = T(0.5) * (FRATIO - one / FRATIO) * t.DELTH
    dfth = (FR * cdf).astype(T)
    fr1ofratio = FR[0] / FRATIO
    lice2sea = ~np.any(fl1 > EPS, axis=(1, 2))
    fla = np.zeros((n, K, M), T)
    cases = dict.fromkeys(CASES, 0)
    for m in range(nmax if m_last is None else m_last):
        if m < M:
            freq, dfreqth, wavn = FR[m], dfth[m], wavnum[:, m]
        else:
            freq = FR[M - 1] * powi(FRATIO, m + 1 - M)
            dfreqth = freq * cdf
            wavn = np.full(n, zpi2gm * (freq * freq), T)
        fr5ofreq5 = t.FR5[M - 1] / powi(freq, 5)
        for k in range(K):
            fnef = freq + coef * wavn * (t.COSTH[k] * v + t.SINTH[k] * u)
            flip = ~(fnef > 0)
            knew = np.where(flip, (k + K // 2) % K, k)
            fnef = np.where(flip, -fnef, fnef).astype(T)
            low = fnef <= fr1ofratio
            with np.errstate(divide="ignore", invalid="ignore"):
                newf = np.floor(np.log10(fnef / FR[0]) * t.FLOGSPRDM1).astype(np.int64) + 1       # 1-based
            newf = np.where(low, -1, newf)
            old = fl1[:, k, m] if m < M else fl1[:, k, M - 1] * fr5ofreq5
            old = np.where(lice2sea, T(0.0), old).astype(T)
            inner = (newf >= 1) & (newf < M)
            below = newf == 0
            top = newf == M
            live = old > 0
            for name, sel in (("interior", inner), ("below", below), ("top", top), ("outside", ~(inner | below | top)), ("flip", flip)):
                cases[name] += int(np.count_nonzero(sel & live))
            i0 = np.clip(newf - 1, 0, M - 2)                     # 0-based NEWM where the interior case holds
            f0, f1 = FR[i0], FR[i0 + 1]
            gwh = dfreqth / (f1 - f0) * old
            gwm = gwh * (f1 - fnef) / dfth[i0]
            gwp = gwh * (fnef - f0) / dfth[i0 + 1]
            r = rows[inner]
            fla[r, knew[inner], i0[inner]] += gwm[inner]
            fla[r, knew[inner], i0[inner] + 1] += gwp[inner]
            gwh = FRATIO * dfreqth / (fre0 * FR[0]) * old
            gwp = gwh * (fnef - fr1ofratio) / dfth[0]
            fla[rows[below], knew[below], 0] += gwp[below]
            gwh = dfreqth / (fre0 * FR[M - 1]) * old
            gwm = gwh * (FRATIO * FR[M - 1] - fnef) / dfth[M - 1]
            fla[rows[top], knew[top], M - 1] += gwm[top]
    return np.maximum(fla, EPS).astype(T), dict(cases=cases, nfre_max=nmax, dfth=dfth)


def ice_reshape(t, fl2nd, cicover, wswave):
    """The noise level under sea ice, outblock.F90:175-194 (LICERUN and not LMASKICE)."""
    T = t.dtype
    f = np.asarray(fl2nd, T)
    zthrs = ((T(1.0) - T(0.9) * np.minimum(np.asarray(cicover, T), T(0.99))) * t.FLMIN).astype(T)
    zrduc = np.exp(T(-10.0) * (t.FR * t.FR)[None, :] / np.sqrt(np.maximum(np.asarray(wswave, T), T(1.0)))[:, None]).astype(T)   # [n][M]
    z = zrduc[:, None, :]
    th = zthrs[:, None, None]
    return np.where(f <= th, np.maximum(z * f, th * (z * z)), f).astype(T)


def fl2nd(t, fl1, wavnum=None, ucur=None, vcur=None, cicover=None, wswave=None, intpol_on=None, ice_on=None):
    """FL2ND as outblock.F90:168-194 builds it (LSECONDORDER = F).  intpol_on / ice_on default to the configuration of the tables:
    IREFRA = 2 / 3, LICERUN and not LMASKICE.  Returns (FL2ND, info of intpol() or None)."""
    c = t.cfg
    intpol_on = int(c.irefra) >= 2 if intpol_on is None else intpol_on
    ice_on = bool(c.licerun and not c.lmaskice) if ice_on is None else ice_on
    info = None
    f = np.asarray(fl1, t.dtype)
    if intpol_on:
        f, info = intpol(t, f, wavnum, ucur, vcur)
    if ice_on:
        f = ice_reshape(t, f, cicover, wswave)
    return f, info


def consumers(t, oracle, f, zmiss: float = -999.0):
    """out [n][8] in the columns FIELDS of the spectrum f: oracle.outbs and the total-spectrum columns of sepwisw_ref.sepwisw."""
    T = t.dtype
    n, K, M = f.shape
    z = np.zeros(n, T)
    sep, _ = S.sepwisw(t, f, np.zeros((n, K, M), T), np.zeros((n, M), T), z, z, zmiss=zmiss)
    return np.concatenate([np.asarray(oracle.outbs(f, zmiss), T), sep[:, :3]], 1)


def deep_wavnum(t, n: int):
    """WAVNUM of deep water, ZPI**2 / G * FR**2: [n][NFRE]."""
    return np.ascontiguousarray(np.broadcast_to(((t.ZPI * t.ZPI) / t.G * (t.FR * t.FR)).astype(t.dtype), (n, len(t.FR))))


def known_answer_inputs(t):
    """Hand-checkable INTPOL cases, one point each (tests/test_outbs_absolute_host.py states the expected values), deep water:
      zero      a JONSWAP spectrum, no current                      empty   an all-zero spectrum under a current (LICE2SEA)
      follow    one bin (K0, M0) and a current of 1 m/s along TH(K0)
      oppose    one bin (K0, NFRE) and a current of -1.5 m/s in both components, K0 the direction nearest to 45 degrees
      tail      FR**-5 in every direction up to NFRE and a current of 1 m/s towards TH(K0): opposing for the far half of the directions
    Returns (names, fl1, wavnum, ucur, vcur, extra) with extra = dict(k0, m0)."""
    from ecwam_amd import synthetic as syn

    T = t.dtype
    K, M = len(t.TH), len(t.FR)
    k0, m0 = 5, M // 2
    kd = int(np.argmin(np.abs(t.TH - np.pi / 4)))
    names, fl, uu, vv = [], [], [], []

    def add(name, f, u, v):
        names.append(name); fl.append(np.asarray(f, T)); uu.append(u); vv.append(v)

    add("zero", syn.jonswap_spectra(t.FR, t.TH, np.array([0.1]), np.array([1.0]), T)[0], 0.0, 0.0)
    add("empty", np.zeros((K, M), T), 0.7, -0.4)
    one = np.zeros((K, M), T); one[k0, m0] = 1.0
    add("follow", one, float(np.sin(t.TH[k0])), float(np.cos(t.TH[k0])))
    opp = np.zeros((K, M), T); opp[kd, M - 1] = 1.0
    add("oppose", opp, -1.5, -1.5)
    add("tail", np.broadcast_to((t.FR / t.FR[0]) ** -5, (K, M)), float(np.sin(t.TH[k0])), float(np.cos(t.TH[k0])))
    n = len(names)
    return (names, np.ascontiguousarray(np.stack(fl), T), deep_wavnum(t, n), np.array(uu, T), np.array(vv, T), dict(k0=k0, m0=m0, kd=kd))
