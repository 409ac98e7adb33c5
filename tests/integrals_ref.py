"""numpy restatement of OUTBLOCK's remaining spectral integrals (outblock.F90:266-287, 451-462, 500-523, 597-604) and of OUTSETWMASK: what
ecwam_hip_outbs_integrals and ecwam_hip_outsetwmask compute, in the working precision of the tables, vectorised over points, with the
loops over K and M in the reference's order.  Test infrastructure only: the device kernel is checked against it.

  OUTBETA (CD=)   outbeta.F90:113-133               MEANSQS      meansqs.F90:93-112
  HALPHAP         halphap.F90:68-112                MEANSQS_GC   meansqs_gc.F90:59-82 with OMEGAGC omegagc.F90:51-55, NS_GC ns_gc.F90:47-49
  MEANSQS_LF      meansqs_lf.F90:80-100             FEMEAN       femean.F90:84-121
  CIMSSTRN        cimsstrn.F90:89-121 with AKI_ICE aki_ice.F90:60-112
  WEFLUX          weflux.F90:98-177                 CTCOR        ctcor.F90:68-120
  SEBTMEAN        sebtmean.F90:81-198 (SE10MEAN se10mean.F90:72-74 is the band (10, 1/FR(1)))
  OUTSETWMASK     outsetwmask.F90:57-75             DEG          yowpcons.F90:31

Every data-dependent decision is returned with its margin (`decisions`: name -> (taken [n] bool or int, margin [n])): the margin is the
relative distance of the two compared numbers (for NS_GC: the distance of the truncated argument to the nearest integer, relative to it),
so that a test may leave out a point only where the restatement itself could go either way within a stated number of eps.
NE of MEANSQS_GC and NFRE_MSS of MEANSQS are evaluated in double precision from the working-precision tables, as the library documents.
"""
from __future__ import annotations

import math

import numpy as np

FIELDS = ("cd", "tauw_n", "mss", "strn", "wefmag", "wefdir", "ctcor", "mss_m")
GROUPS = dict(slopes=1, strain=2, flux=4, ctcor=8, bands=16, point=32)
GROUP_COLUMNS = {1: (2, 7), 2: (3,), 4: (4, 5), 8: (6,), 16: None, 32: (0, 1)}   # None: columns 8 ...
# which decisions bear on which column
DECISIONS_OF = {2: ("halp_mean", "halp_max", "ns_gc", "xks_0"), 7: ("halp_mean", "halp_max", "ns_gc", "xks_1"), 3: ("f1lim",), 5: ("wefy",),
                6: ("ctcor_cap",)}


def default_bands(t):
    T = t.dtype
    return [(10.0, float(T(1.0) / t.FR[0])), (10.0, 12.0), (12.0, 14.0), (14.0, 17.0), (17.0, 21.0), (21.0, 25.0), (25.0, 30.0)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


# ---- SEBTMEAN ------------------------------------------------------------------------------------------------------------------------
def band_constants(t, tb, tt):
    """sebtmean.F90:81-102 and the factors of :119-120, :148-149, :165, :172-175, :184, in the working precision.  1-based MCUTB / MCUTT."""
    T = t.dtype
    FR, M = t.FR, len(t.FR)
    tb, tt = T(tb), T(tt)
    c = {}
    fbot = T(1.0) / max(tt, t.EPSMIN)
    fcutb_ft = min(fbot, FR[M - 1])
    fcutb = max(FR[0], fcutb_ft)
    fbot = max(fbot, FR[M - 1])
    mcutb = 1
    while FR[mcutb - 1] < fcutb and mcutb < M:
        mcutb += 1
    ftop = T(1.0) / max(tb, t.EPSMIN)
    fcutt = max(FR[0], min(ftop, FR[M - 1]))
    ftop = max(ftop, FR[M - 1])
    mcutt = M
    while FR[mcutt - 1] > fcutt and mcutt > 1:
        mcutt -= 1
    if fcutb == fcutt:
        mcutt = mcutb - 1
    assert mcutt >= 1, "band wholly below FR(1)"
    frloc = {m: FR[m - 1] for m in range(1, M + 1)}
    if mcutb > 1:
        frloc[mcutb - 1] = fcutb
        c["wlb"] = (FR[mcutb - 1] - fcutb) / (FR[mcutb - 1] - FR[mcutb - 2])
        c["wrb"] = T(1.0) - c["wlb"]
    if mcutt < M:
        frloc[mcutt + 1] = fcutt
        c["wlt"] = (FR[mcutt] - fcutt) / (FR[mcutt] - FR[mcutt - 1])
        c["wrt"] = T(1.0) - c["wlt"]
    c.update(mcutb=mcutb, mcutt=mcutt, m0=max(mcutb - 1, 1), m1=min(mcutt, M - 1))
    c["df"] = {m: T(0.5) * (frloc[m + 1] - frloc[m]) for m in range(c["m0"], c["m1"] + 1)}
    c["front"] = bool(fcutb_ft < fcutb and fcutb == FR[0])
    if c["front"]:
        wl = (FR[0] - fcutb_ft) / FR[0]
        wr = T(1.0) - wl
        c["dft"] = T(0.5) * (FR[0] - fcutb_ft) * (T(1.0) + wr)
    c["tail"] = bool(fbot < ftop)
    if c["tail"]:
        b2, t2 = fbot * fbot, ftop * ftop
        c["zw"] = T(0.25) * t.FR5[M - 1] * (T(1.0) / (b2 * b2) - T(1.0) / (t2 * t2))
    c.update(fcutb=fcutb, fcutt=fcutt, fbot=fbot, ftop=ftop)
    return c


def _f1d_plain(t, F, m):
    s = F[:, 0, m] * t.DELTH
    for k in range(1, F.shape[1]):
        s = s + F[:, k, m] * t.DELTH
    return s


def _f1d_interp(t, F, wl, wr, m):
    """sum over K of (WL F(K,m-1) + WR F(K,m)) DELTH, m 0-based: per K, as sebtmean.F90:124-128"""
    s = (wl * F[:, 0, m - 1] + wr * F[:, 0, m]) * t.DELTH
    for k in range(1, F.shape[1]):
        s = s + (wl * F[:, k, m - 1] + wr * F[:, k, m]) * t.DELTH
    return s


def sebtmean(t, F, tb, tt):
    """EBT [n] of the spectrum F [n][K][M] for the band (tb, tt)."""
    T = t.dtype
    n, K, M = F.shape
    c = band_constants(t, tb, tt)
    f1d = {}
    if c["mcutb"] > 1:
        f1d[c["mcutb"] - 1] = _f1d_interp(t, F, c["wlb"], c["wrb"], c["mcutb"] - 1)
    for m in range(c["mcutb"], c["mcutt"] + 1):
        f1d[m] = _f1d_plain(t, F, m - 1)
    if c["mcutt"] < M:
        f1d[c["mcutt"] + 1] = _f1d_interp(t, F, c["wlt"], c["wrt"], c["mcutt"])
    e = np.full(n, t.EPSMIN, T)
    for m in range(c["m0"], c["m1"] + 1):
        e = e + c["df"][m] * (f1d[m + 1] + f1d[m])
    if c["front"]:
        e = e + c["dft"] * f1d[1]
    if c["tail"]:
        e = e + c["zw"] * _f1d_plain(t, F, M - 1)
    return e


def band_heights(t, F, bands):
    T = t.dtype
    return np.stack([T(4.0) * np.sqrt(np.maximum(sebtmean(t, F, a, b), T(0.0))) for a, b in bands], 1)


# ---- the readers of FL1 ----------------------------------------------------------------------------------------------------------------
def _rowsum(F, m):
    s = np.zeros(F.shape[0], F.dtype)
    for k in range(F.shape[1]):
        s = s + F[:, k, m]
    return s


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


def meansqs_lf(t, nfre_eff, F, wavnum):
    T = t.dtype
    x = np.zeros(F.shape[0], T)
    for m in range(min(nfre_eff, F.shape[2])):
        temp1 = t.DFIM[m] * (wavnum[:, m] * wavnum[:, m])
        x = x + temp1 * _rowsum(F, m)
    return x


def halphap(t, F, wavnum, wdwave):
    """(HALP [n], decisions)"""
    T = t.dtype
    n, K, M = F.shape
    wd = np.stack([T(0.5) + T(0.5) * np.copysign(T(1.0), np.cos(t.TH[k] - wdwave)) for k in range(K)], 1).astype(T)
    flwd = F * wd[:, :, None]
    xmss = meansqs_lf(t, M, flwd, wavnum)
    em, fm = _femean(t, flwd)
    f1d = np.zeros(n, T)
    for k in range(K):
        f1d = f1d + flwd[:, k, M - 1] * t.DELTH
    tail = t.ZPI4GM2 * t.FR5[M - 1] * f1d
    mean_branch = (em > 0) & (fm < t.FR[M - 3])
    with np.errstate(divide="ignore", invalid="ignore"):
        a = xmss / (np.log(t.FR[M - 1]) - np.log(fm))
    over = mean_branch & (a > t.ALPHAPMAX)
    alphap = np.where(mean_branch & ~over, a, tail).astype(T)
    dec = {"halp_mean": (mean_branch, np.minimum(_rel(fm, t.FR[M - 3]), np.where(em > 0, 1.0, 0.0))),
           "halp_max": (over, np.where(mean_branch, _rel(a, t.ALPHAPMAX), 1.0))}
    return T(0.5) * np.minimum(alphap, t.ALPHAPMAX), dec


def ns_gc(t, ustar):
    """NS_GC (1-based) and the margin of its truncation"""
    T = t.dtype
    xks = t.SQRTGOSURFT / (T(1.48) + T(2.05) * ustar)
    arg = np.log(np.maximum(xks * t.XKM_GC[0], T(1.0))) * t.XLOGKRATIOM1_GC
    ns = np.minimum(arg.astype(np.int64) + 1, t.NWAV_GC - 1)
    a64 = arg.astype(np.float64)
    margin = np.abs(a64 - np.rint(a64)) / np.maximum(a64, 1.0)
    return ns, margin


def cutoff_indices(t, xkmss):
    """(FCUT, NFRE_EFF, NE) of a cut-off wavenumber: meansqs.F90:99-101, meansqs_gc.F90:59; the indices in double precision"""
    T = t.dtype
    xkmss = T(xkmss)
    fcut = np.sqrt(t.G * xkmss) / t.ZPI
    mss = int(math.log(float(fcut) / float(t.FR[0])) / math.log(float(t.FRATIO))) + 1
    ne = int(np.rint(math.log(float(xkmss) * float(t.XKM_GC[0])) * float(t.XLOGKRATIOM1_GC)))
    return T(fcut), min(len(t.FR), mss), min(max(ne, 1), t.NWAV_GC)


def default_xkmss(t):
    return t.XK_GC[t.NWAV_GC - 1]


def model_xkmss(t):
    zf = t.ZPI * t.FR[-1]
    return zf * zf / t.G


def meansqs(t, xkmss, F, wavnum, ustar, halp, tag):
    """XMSS [n] with HALP of halphap(); decisions of OMEGAGC and of XKS > XKMSS under the names ns_gc, xks_<tag>"""
    T = t.dtype
    n = F.shape[0]
    xkmss = T(xkmss)
    fcut, nfre_eff, ne = cutoff_indices(t, xkmss)
    ns, ns_margin = ns_gc(t, ustar)
    xks = t.XK_GC[ns - 1]
    frgc = t.OMEGA_GC[ns - 1] / t.ZPI
    above = xks > xkmss
    ns2 = np.where(above, ne, ns)
    x = np.where(above, T(0.0), t.DELKCC_GC_NS[ns - 1] * t.XKM_GC[ns - 1]).astype(T)
    for i in range(int(ns2.min()) + 1, ne + 1):
        x = np.where(i > ns2, x + t.DELKCC_GC[i - 1] * t.XKM_GC[i - 1], x).astype(T)
    coef = t.C2OSQRTVG_GC[ns2 - 1] * halp
    x = x * coef
    x = x + meansqs_lf(t, nfre_eff, F, wavnum)
    xlogfs = np.log(t.FR[nfre_eff - 1])
    x = x + T(2.0) * halp * np.maximum(np.log(np.minimum(frgc, fcut)) - xlogfs, T(0.0))
    dec = {"ns_gc": (ns, ns_margin), f"xks_{tag}": (above, _rel(xks, xkmss))}
    return x.astype(T), dec


def aki_ice(G, xk, depth, rhow, cith):
    """aki_ice.F90:60-112, vectorised: every element iterates until ITS OWN stopping test holds"""
    T = xk.dtype.type
    ymice, rmuice, rhoi, ebs, aki_max = T(5.5e9), T(0.3), T(922.5), T(0.000001), T(20.0)
    ice = cith > 0
    c = np.where(ice, cith, T(1.0)).astype(T)
    ficstf = (ymice * (c * c * c) / (T(12.0) * (T(1.0) - rmuice * rmuice))) / rhow
    rdh = (rhoi / rhow) * c
    om2 = G * xk * np.tanh(xk * depth)
    akiold = np.zeros_like(xk)
    aki = np.minimum(xk, np.power(om2 / np.maximum(ficstf, T(1.0)), T(0.2))).astype(T)
    for _ in range(200):       # (SINH(50)**2 overflows in single precision: DEPTH / inf = 0, as on the device)
        go = ice & (np.abs(aki - akiold) > ebs * akiold) & (aki < aki_max)
        if not go.any():
            break
        akiold = np.where(go, aki, akiold)
        a = np.where(go, aki, T(1.0))
        akid = np.minimum(depth * a, T(50.0))
        a2 = a * a
        a4 = a2 * a2
        fv = ficstf * (a4 * a) + G * a - om2 * (rdh * a + T(1.0) / np.tanh(akid))
        with np.errstate(over="ignore"):
            sh = np.sinh(akid)
            fprime = T(5.0) * ficstf * a4 + G - om2 * (rdh - depth / (sh * sh))
        new = a - fv / fprime
        new = np.where(new <= 0, aki_max, new)
        aki = np.where(go, new, aki).astype(T)
    return np.where(ice, aki, xk).astype(T)


def cimsstrn(t, F, wavnum, depth, cithick):
    T = t.dtype
    n, K, M = F.shape
    f1lim = t.FLMIN / t.DELTH
    strn = np.zeros(n, T)
    margin = np.ones(n)
    every = np.ones(n, bool)
    for m in range(M):
        xki = aki_ice(t.G, wavnum[:, m], depth, t.ROWATER, cithick)
        e = T(0.5) * cithick * (xki * xki * xki) / wavnum[:, m]
        sume = _rowsum(F, m)
        take = sume > f1lim
        strn = np.where(take, strn + e * e * sume * t.DFIM[m], strn).astype(T)
        margin = np.minimum(margin, _rel(sume, f1lim))
        every &= take
    return strn, {"f1lim": (every, margin)}


def weflux(t, F, cgroup):
    """(WEFMAG, direction in degrees, decisions)"""
    T = t.dtype
    n, K, M = F.shape
    mag, wx, wy = np.zeros(n, T), np.zeros(n, T), np.zeros(n, T)
    rog = t.ROWATER * t.G
    delt = t.FRTAIL * t.DELTH * t.G / (T(2.0) * t.ZPI)
    for m in range(M):
        fcg = F[:, 0, m] * cgroup[:, m]
        temp, tx, ty = fcg, fcg * t.SINTH[0], fcg * t.COSTH[0]
        for k in range(1, K):
            fcg = F[:, k, m] * cgroup[:, m]
            temp = temp + fcg
            tx = tx + fcg * t.SINTH[k]
            ty = ty + fcg * t.COSTH[k]
        mag = mag + t.DFIM[m] * temp
        wx = wx + t.DFIM[m] * tx
        wy = wy + t.DFIM[m] * ty
    fcg = F[:, 0, M - 1]
    temp, tx, ty = fcg, fcg * t.SINTH[0], fcg * t.COSTH[0]
    for k in range(1, K):
        fcg = F[:, k, M - 1]
        temp = temp + fcg
        tx = tx + fcg * t.SINTH[k]
        ty = ty + fcg * t.COSTH[k]
    mag = mag + delt * temp
    wx = wx + delt * tx
    wy = wy + delt * ty
    mag = rog * mag
    zero = wy == 0
    wy = np.where(zero, t.EPSMIN, wy).astype(T)
    d = np.arctan2(wx, wy)
    d = np.where(d < 0, d + t.ZPI, d).astype(T)
    deg = np.fmod(T(57.295778667) * d + T(180.0), T(360.0))
    # the guard itself flips only at WEFY = 0; the direction is ill-conditioned where the flux vector is short against its parts
    return mag.astype(T), deg.astype(T), {"wefy": (zero, np.abs(wy.astype(np.float64)) / np.maximum(np.abs(mag.astype(np.float64)) / float(rog), 1e-300))}


def ctcor(t, F, zmiss):
    T = t.dtype
    n, K, M = F.shape
    em, zt1 = np.zeros(n, T), np.zeros(n, T)
    temp = []
    for m in range(M):
        s = _rowsum(F, m)
        temp.append(s)
        em = em + t.DFIM[m] * s
        zt1 = zt1 + t.DFIMFR[m] * s
    fr1m1 = T(1.0) / t.FR[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        per = em / zt1
    capped = (zt1 > 0) & (per > fr1m1)
    per = np.where(zt1 > 0, np.minimum(per, fr1m1), T(0.0)).astype(T)
    rho, lam = np.zeros(n, T), np.zeros(n, T)
    for m in range(M):
        zarg = t.PI * t.FR[m] * per
        zamp = t.DFIM[m] * temp[m]
        rho = rho + zamp * np.cos(zarg)
        lam = lam + zamp * np.sin(zarg)
    with np.errstate(divide="ignore", invalid="ignore"):
        ctr = np.where(em > 0, np.sqrt(rho * rho + lam * lam) / em, T(zmiss))
    return ctr.astype(T), {"ctcor_cap": (capped, np.where(zt1 > 0, _rel(em / np.where(zt1 > 0, zt1, 1), fr1m1), 1.0)), "ctcor_em": (em > 0, np.ones(n))}


def outbeta_cd(t, u10, ustar, chrnck):
    """MIN(CD, 0.01) of outblock.F90:277 and Z0ATM"""
    T = t.dtype
    amax = np.full(u10.shape, t.ALPHAMAX, T) if t.cfg.llgcbz0 else np.minimum(t.ALPHAMAX, T(0.02) + T(0.01) * u10)
    usm = T(1.0) / np.maximum(ustar, t.EPSUS)
    betam = np.maximum(np.minimum(chrnck, amax), t.ALPHAMIN)
    z0atm = t.RNUM * usm + t.GM1 * betam * (ustar * ustar)
    q = t.XKAPPA / np.log(T(1.0) + t.XNLEV / z0atm)
    return np.minimum(q * q, T(0.01)).astype(T), z0atm.astype(T)


def integrals(t, fl1, wv, ff, bands=None, xkmss=None, fl2nd=None, zmiss=-999.0):
    """(out [n][8 + nband], decisions) of ecwam_hip_outbs_integrals with every group selected; wv [n][5][M], ff [n][16] in the device layouts."""
    T = t.dtype
    bands = default_bands(t) if bands is None else bands
    xk0 = default_xkmss(t) if xkmss is None or xkmss <= 0 else T(xkmss)
    wavnum, cgroup = wv[:, 0], wv[:, 1]
    wdwave, u10, ustar, tauw, chrnck, cith, depth = (ff[:, i] for i in (1, 3, 7, 8, 12, 13, 15))
    n = fl1.shape[0]
    out = np.zeros((n, 8 + len(bands)), T)
    dec = {}
    out[:, 0], _ = outbeta_cd(t, u10, ustar, chrnck)
    out[:, 1] = tauw / np.maximum(ustar * ustar, t.EPSUS)
    halp, d = halphap(t, fl1, wavnum, wdwave)
    dec.update(d)
    out[:, 2], d = meansqs(t, xk0, fl1, wavnum, ustar, halp, 0)
    dec.update(d)
    out[:, 7], d = meansqs(t, model_xkmss(t), fl1, wavnum, ustar, halp, 1)
    dec.update(d)
    out[:, 3], d = cimsstrn(t, fl1, wavnum, depth, cith)
    dec.update(d)
    out[:, 4], out[:, 5], d = weflux(t, fl1, cgroup)
    dec.update(d)
    out[:, 6], d = ctcor(t, fl1, zmiss)
    dec.update(d)
    if bands:
        out[:, 8:] = band_heights(t, fl1 if fl2nd is None else fl2nd, bands)
    return out, dec


def outsetwmask(out, colflags, cicover, iodp, licerun, cithrsh, zmiss):
    """OUTSETWMASK on a copy of out [n][ncol]; iodp may be None when no column has bit 1"""
    T = out.dtype.type
    r = out.copy()
    for c, cf in enumerate(colflags):
        if licerun and (cf & 1):
            r[:, c] = np.where(cicover > T(cithrsh), T(zmiss), r[:, c])
        if cf & 2:
            io = iodp.astype(out.dtype)
            r[:, c] = r[:, c] * io + (T(1.0) - io) * T(zmiss)
    return r
