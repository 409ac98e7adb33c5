"""numpy restatement of the wind-sea / swell separation and the mean-period / spread parameters of OUTBLOCK (outblock.F90:197-382 with
FL2ND = FL1, LLPARTITION = F): what ecwam_hip_outbs_sepwisw computes, in the working precision of the tables, vectorised over points,
with the loops over K and M in the reference's order.  Test infrastructure only: the device kernel is checked against it.

  SEPWISW      sepwisw.F90:146-275 (SEP3TR and the swell trains are not restated)
  FEMEAN       femean.F90:95-120           STHQ     sthq.F90:79-101
  MWP1 / MWP2  mwp1.F90:91-115, mwp2.F90:91-115 (DFIMFR_SIM, DFIMFR2_SIM: initmdl.F90:496-500; WP2TAIL = 0.5, OLDWSFC = 1.2: yowfred.F90)
  WDIRSPREAD   wdirspread.F90:78-119 with PEAKFRI peakfri.F90:64-86 and SCOSFL scosfl.F90:71-92
  DEG          yowpcons.F90:31
"""
from __future__ import annotations

import numpy as np

FIELDS = ("mp1", "mp2", "wdw", "shww", "shts", "mdww", "mdts", "mpww", "mpts",
          "p1sea", "p1swell", "p2sea", "p2swell", "sprdsea", "sprdswell")


def _femean(t, F):
    T = t.dtype
    n, K, M = F.shape
    em = np.zeros(n, T)
    fm = np.zeros(n, T)
    delt25 = t.WETAIL * t.FR[M - 1] * t.DELTH
    delt2 = t.FRTAIL * t.DELTH
    for m in range(M):
        temp2 = np.maximum(F[:, 0, m], t.EPSMIN)
        for k in range(1, K):
            temp2 = temp2 + np.maximum(F[:, k, m], t.EPSMIN)
        em = em + temp2 * t.DFIM[m]
        fm = fm + t.DFIMOFR[m] * temp2
    em = em + delt25 * temp2
    fm = fm + delt2 * temp2
    fm = em / fm
    return em, np.maximum(fm, t.FR[0])


def _sthq(t, F):
    T = t.dtype
    n, K, M = F.shape
    si = np.zeros(n, T)
    ci = np.zeros(n, T)
    for k in range(K):
        temp = np.zeros(n, T)
        for m in range(M):
            temp = temp + F[:, k, m] * t.DFIM[m]
        si = si + t.SINTH[k] * temp
        ci = ci + t.COSTH[k] * temp
    ci = np.where(ci == 0, t.EPSMIN, ci)
    th = np.arctan2(si, ci)
    return np.where(th < 0, th + t.ZPI, th)


def _mwp(t, F, second: bool):
    T = t.dtype
    n, K, M = F.shape
    mo = t.NFRE_ODD
    em = np.zeros(n, T)
    mw = np.zeros(n, T)
    for m in range(mo):
        temp = np.zeros(n, T)
        for k in range(K):
            temp = temp + F[:, k, m]
        w = t.DFIM_SIM[m] * (t.FR[m] * t.FR[m]) if second else t.DFIM_SIM[m] * t.FR[m]
        em = em + t.DFIM_SIM[m] * temp
        mw = mw + w * temp
    fro = t.FR[mo - 1]
    fr1m1 = T(1.0) / t.FR[0]
    delt25 = t.WETAIL * fro * t.DELTH
    coef = T(0.5) * t.DELTH * (fro * fro * fro) if second else t.WP1TAIL * t.DELTH * (fro * fro)
    em = em + delt25 * temp
    mw = mw + coef * temp
    ok = (em > 0) & (mw > t.EPSMIN)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = em / mw
        if second:
            q = np.sqrt(q)
    return np.where(ok, np.minimum(q, fr1m1), T(0.0)).astype(T)


def _scosfl(t, F, mm):
    """SCOSFL at frequency index mm[ij] (0-based)."""
    T = t.dtype
    n, K, M = F.shape
    rows = np.arange(n)
    si = np.zeros(n, T)
    ci = np.zeros(n, T)
    for k in range(K):
        f = F[rows, k, mm]
        si = si + t.SINTH[k] * f
        ci = ci + t.COSTH[k] * f
    md = np.where((ci == 0) & (si == 0), T(0.0), np.arctan2(si, ci)).astype(T)
    mc = np.zeros(n, T)
    for k in range(K):
        mc = mc + np.cos(t.TH[k] - md) * F[rows, k, mm]
    return t.DELTH * mc


def _wdirspread(t, F, emean, peak: bool):
    T = t.dtype
    n, K, M = F.shape
    one = T(1.0)
    if peak:
        epk = np.zeros(n, T)       # PEAKFRI
        ipk = np.full(n, M - 1)
        for m in range(M):
            f1d = np.zeros(n, T)
            for k in range(K):
                f1d = f1d + F[:, k, m] * t.DELTH
            up = epk < f1d
            epk = np.where(up, f1d, epk)
            ipk = np.where(up, m, ipk)
        w = _scosfl(t, F, ipk)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(epk > 0, np.minimum(w / epk, one), one)
    else:
        w = np.zeros(n, T)
        for m in range(M):
            temp = _scosfl(t, F, np.full(n, m))
            w = w + temp * t.DFIM[m]
        w = w / t.DELTH + temp * (t.WETAIL * t.FR[M - 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(emean > t.EPSMIN, np.minimum(w / emean, one), one)
    return np.sqrt(T(2.0) * (one - w)).astype(T)


def coswdif(t, wdwave):
    """COS(TH(K) - WDWAVE), outblock.F90:197-201: [n][NANG]."""
    return np.cos(t.TH[None, :] - np.asarray(wdwave, t.dtype)[:, None]).astype(t.dtype)


def sepwisw(t, fl1, xllws, cinv, ufric, wdwave, small_domain: bool = False, zmiss: float = -999.0):
    """Returns (out [n][15] in the columns FIELDS, info): info["near"] marks the points where some CHECKTA of the masks lies within
    4 ulp of 1 (there a last-bit difference of COSWDIF may flip a bin), info["swm"] the final mask [n][NANG][NFRE]."""
    T = t.dtype
    fl1 = np.asarray(fl1, T)
    xllws = np.asarray(xllws, T)
    cinv = np.asarray(cinv, T)
    ufric = np.asarray(ufric, T)
    wdwave = np.asarray(wdwave, T)
    n, K, M = fl1.shape
    one = T(1.0)
    cw = coswdif(t, wdwave)
    coef = T(1.2) * t.FRIC
    xinv = ufric[:, None] * cinv                                      # XINVWVAGE [n][M]
    dirc = coef * cw                                                  # DIRCOEF [n][K]
    near = np.zeros(n, bool)
    tol = 4 * np.finfo(T).eps

    def _near(ct, live):
        return np.any(live & (np.abs(ct.astype(np.float64) - 1.0) <= tol), axis=(1, 2))

    chk = xinv[:, None, :] * dirc[:, :, None]                         # CHECKTA [n][K][M]
    swm = np.where(xllws != 0, T(0.0), np.where(chk >= one, T(0.0), one)).astype(T)
    near |= _near(chk, xllws == 0)
    if not small_domain:
        f1 = fl1 * swm
        _, fsw = _femean(t, f1)
        f1 = np.maximum(fl1 - f1, T(0.0))
        _, fse = _femean(t, f1)
        r = np.where(fsw > T(0.96) * fse, one, T(0.0)).astype(T)
        dirc2 = r[:, None] * coef * np.copysign(one, T(0.4) + cw)
        chk2 = xinv[:, None, :] * dirc2[:, :, None]
        near |= _near(chk2, r[:, None, None] > 0)
        swm = np.where(chk2 >= one, T(0.0), swm).astype(T)
        for k in range(K):                                            # the walk from NFRE down to 2, per direction
            done = np.zeros(n, bool)                                  # EXIT taken
            for m in range(M - 1, 0, -1):
                s0, s1 = swm[:, k, m] == 1, swm[:, k, m - 1] == 1
                done |= s0 & s1
                drop = ~done & ~s0 & s1 & (fl1[:, k, m] >= fl1[:, k, m - 1])
                swm[drop, k, m - 1] = 0
    f1 = np.maximum(fl1, t.EPSMIN) * swm                              # the swell part
    esw, fsw = _femean(t, f1)
    thsw = _sthq(t, f1)
    p1sw, p2sw = _mwp(t, f1, False), _mwp(t, f1, True)
    spsw = _wdirspread(t, f1, esw, True)
    c4 = (cw * cw) * (cw * cw)
    floor = (cw[:, :, None] > T(0.8)) & (np.arange(M)[None, None, :] + 1 >= M // 2)
    d = fl1 - f1
    d = np.where(floor, d + t.EPSMIN * c4[:, :, None], d)
    f2 = np.maximum(d, T(0.0)).astype(T)                              # the sea part
    ese, fse = _femean(t, f2)
    thse = np.where(ese <= T(1.0e-9), wdwave, _sthq(t, f2))
    p1se, p2se = _mwp(t, f2, False), _mwp(t, f2, True)
    spse = _wdirspread(t, f2, ese, True)
    em, _ = _femean(t, fl1)                                           # the total spectrum
    p1, p2 = _mwp(t, fl1, False), _mwp(t, fl1, True)
    wdw = _wdirspread(t, fl1, em, False)
    deg = T(57.295778667)
    zm = T(zmiss)
    with np.errstate(divide="ignore"):
        cols = [p1, p2, wdw, T(4.0) * np.sqrt(np.maximum(ese, T(0.0))), T(4.0) * np.sqrt(np.maximum(esw, T(0.0))),
                np.fmod(deg * thse + T(180.0), T(360.0)), np.fmod(deg * thsw + T(180.0), T(360.0)),
                np.where(fse > 0, one / fse, zm), np.where(fsw > 0, one / fsw, zm), p1se, p1sw, p2se, p2sw, spse, spsw]
    out = np.stack([np.asarray(c, T) for c in cols], 1)
    return out, dict(near=near, swm=swm)


def synthetic_xllws(t, wdwave, fcut: float):
    """A wind-sea mask where IMPLSCH is not run: the bins within 60 degrees of the wind above the frequency fcut."""
    cw = coswdif(t, wdwave)
    live = (cw[:, :, None] > 0.5) & (t.FR[None, None, :] > fcut)
    return live.astype(t.dtype)


def known_answer_inputs(t):
    """Hand-checkable spectra, one point each (tests/test_outbs_sepwisw_host.py states the expected values):
      allsea   every XLLWS = 1 (all wind sea)            allswell  XLLWS = 0 and UFRIC = 0 (all swell), winds of either sign
      onebin   energy in one bin (K 5, M 9)              iso       an isotropic single frequency (M 12)
      twosys   swell at 0.06 Hz against the wind + wind sea at 0.2 Hz along it, the mask from UFRIC 0.5 m/s
    Returns (names, fl1, xllws, cinv, ufric, wdwave, extra) with extra = the two systems of twosys and their directions."""
    from ecwam_amd import synthetic as syn

    T = t.dtype
    K, M = len(t.TH), len(t.FR)
    G = 9.806
    cinv1 = (t.ZPI * t.FR / T(G)).astype(T)                                 # deep water: 1 / c = 2 pi f / g
    wd_sea = T(0.7)
    swell = syn.jonswap_spectra(t.FR, t.TH, np.array([0.06]), np.array([wd_sea + np.pi]), T, alfa=0.004)[0]
    sea = syn.jonswap_spectra(t.FR, t.TH, np.array([0.2]), np.array([wd_sea]), T)[0]
    base = syn.jonswap_spectra(t.FR, t.TH, np.array([0.1]), np.array([1.0]), T)[0]
    names, fl, xl, uf, wd = [], [], [], [], []

    def add(name, f, x, u, w):
        names.append(name); fl.append(f); xl.append(x); uf.append(u); wd.append(w)

    add("allsea", base, np.ones((K, M), T), 0.3, 1.0)
    for w in (1.0, -1.0, -4.0, 9.0):
        add(f"allswell{w:+.0f}", base, np.zeros((K, M), T), 0.0, w)
    one = np.zeros((K, M), T); one[5, 9] = 1.0
    add("onebin", one, np.zeros((K, M), T), 0.0, 0.0)
    iso = np.zeros((K, M), T); iso[:, 12] = 1.0
    add("iso", iso, np.zeros((K, M), T), 0.0, 0.0)
    add("twosys", (swell + sea).astype(T), np.zeros((K, M), T), 0.5, wd_sea)
    n = len(names)
    fl1 = np.ascontiguousarray(np.stack(fl), T)
    return (names, fl1, np.ascontiguousarray(np.stack(xl), T), np.ascontiguousarray(np.broadcast_to(cinv1, (n, M)), T),
            np.array(uf, T), np.array(wd, T), dict(swell=swell, sea=sea, wd_sea=wd_sea))
