"""numpy restatement of the extreme-wave parameters of OUTBLOCK: KURTOSIS and W_MAXH, what ecwam_hip_outbs_extremes computes, in the
working precision of the tables (t.dtype), vectorised over points, with the loops over K and M in the reference's order.  Test
infrastructure only: the device kernel is checked against it.

  KURTOSIS     kurtosis.F90:241-398        PEAK_ANG    peak_ang.F90:78-174       AKI      aki.F90:249-269
  TRANSF_BFI   transf_bfi.F90:56-91        STAT_NL     stat_nl.F90:185-272       TRANSF_R transf_r.F90:325-346
  H_MAX        h_max.F90:91-125            W_MAXH      w_maxh.F90:106-333        W_MODE_ST w_mode_st.F90:191-211
  WP2TAIL yowfred.F90:54, XKDMIN / BATHYMAX yowshal.F90:22-23, DKMAX yowpcons.F90:34, DFIMFR2 initmdl.F90:447

Integer powers are products (X**2 = X*X, X**4 = (X*X)*(X*X)); EMEAN**1.5 is a power.  AKI's open iteration is bounded at 100 steps,
as on the device.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("c4", "bfi", "qp", "hmax", "tmax", "c3", "eta_m", "r", "xnslc", "cmax_f", "hmax_n", "cmax_st", "hmax_st")
DKMAX, XKDMIN, WP2TAIL = 40.0, 0.75, 0.5
AKI_MAXIT = 100


def zeps(T):
    """ZEPSILON = 10 EPSILON and its square root in precision T (kurtosis.F90:241-242)."""
    z = T(10.0) * np.finfo(T).eps
    return z, np.sqrt(z)


def nint(x):
    """Fortran NINT: the nearest integer, halves away from zero (not numpy's round half to even)."""
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5))


def peak_ang(t, F):
    """PEAK_ANG (peak_ang.F90:78-174): XNU, SIG_TH and the window's MMAX (0-based)."""
    T = t.dtype
    n, K, M = F.shape
    ze, _ = zeps(T)
    nsh = 1 + int(np.log(T(1.5)) / np.log(t.FRATIO))                                  # :80
    s0 = np.full(n, ze, T)
    s1 = np.zeros(n, T)
    s2 = np.zeros(n, T)
    fr2 = t.DFIM * (t.FR * t.FR)
    for m in range(M):                                                                # :88-103
        temp = F[:, 0, m].copy()
        for k in range(1, K):
            temp = temp + F[:, k, m]
        s0 = s0 + temp * t.DFIM[m]
        s1 = s1 + temp * t.DFIMFR[m]
        s2 = s2 + temp * fr2[m]
    frn = t.FR[M - 1]
    s0 = s0 + t.WETAIL * frn * t.DELTH * temp                                         # :106-113
    s1 = s1 + t.WP1TAIL * t.DELTH * (frn * frn) * temp
    s2 = s2 + T(WP2TAIL) * t.DELTH * (frn * frn * frn) * temp
    with np.errstate(invalid="ignore", divide="ignore"):
        xnu = np.where(s0 > ze, np.sqrt(np.maximum(ze, s2 * s0 / (s1 * s1) - T(1))), ze).astype(T)   # :115-121
    xmax = np.zeros(n, T)                                                             # :127-141
    mmax = np.full(n, 1)
    for m in range(1, M - 1):
        for k in range(K):
            up = F[:, k, m] > xmax
            mmax = np.where(up, m, mmax)
            xmax = np.where(up, F[:, k, m], xmax)
    p1 = np.full(n, ze, T)
    p2 = np.zeros(n, T)
    ss = np.zeros(n, T)
    sc = np.full(n, ze, T)
    idx = np.arange(n)
    for j in range(-nsh, nsh + 1):                                                    # :148-165
        m = mmax + j
        live = (m >= 0) & (m <= M - 1)
        mc = np.clip(m, 0, M - 1)
        for k in range(K):
            f = np.where(live, F[idx, k, mc], T(0))
            ss = ss + t.SINTH[k] * f
            sc = sc + t.COSTH[k] * f
        th = np.arctan2(ss, sc)
        dfm = t.DFIM[mc]
        for k in range(K):
            f = F[idx, k, mc]
            p1 = np.where(live, p1 + f * dfm, p1)
            p2 = np.where(live, p2 + np.cos(t.TH[k] - th) * f * dfm, p2)
    with np.errstate(invalid="ignore"):
        sig = np.where(p1 > ze, np.sqrt(T(2) * (T(1) - p2 / p1)), T(0)).astype(T)    # :167-174
    return xnu, sig, mmax


def aki(t, om, beta):
    """AKI (aki.F90:249-269), vectorised: the wave number of OM at depth BETA; also the relative last step |AKP-AO|/AO at the exit and
    BO/DKMAX of the last iteration (for the near-decision test)."""
    T = t.dtype
    om, beta = np.asarray(om, T), np.asarray(beta, T)
    G = t.G
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        akm1 = om * om / (T(4) * G)
        akm2 = om / (T(2) * np.sqrt(G * beta))
        ao = np.maximum(akm1, akm2)
        res = np.zeros_like(ao)
        done = np.zeros(ao.shape, bool)
        step = np.zeros_like(ao)
        bos = np.zeros_like(ao)
        for _ in range(AKI_MAXIT):
            akp = ao
            bo = beta * ao
            bos = np.where(done, bos, bo)
            deep = ~done & (bo > T(DKMAX))
            res = np.where(deep, om * om / G, res)
            done = done | deep
            th = G * ao * np.tanh(bo)
            sth = np.sqrt(th)
            ch = np.cosh(bo)
            new = ao + (om - sth) * sth * T(2) / (th / ao + G * bo / (ch * ch))
            ao = np.where(done, ao, new).astype(T)
            stop = ~done & ~(np.abs(akp - ao) > T(1.0e-4) * ao)
            step = np.where(stop, np.abs(akp - ao) / ao, step)
            res = np.where(stop, ao, res)
            done = done | stop
            if done.all():
                break
        res = np.where(done, res, ao)
    return res.astype(T), step, bos


def _vg(T, c0, x, dk):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = T(0.5) * c0 * (T(1) + T(2) * x / np.sinh(T(2) * x))
    v = np.where(x < T(1.0e-4), c0, v)
    if dk:
        v = np.where(x > T(DKMAX), T(0.5) * c0, v)
    return v.astype(T)


def transf_bfi(t, xk0, d, xnu, sig_th):
    """TRANSF_BFI (transf_bfi.F90:56-91)."""
    T = t.dtype
    G = t.G
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xk = np.maximum(xk0, T(XKDMIN) / d)
        x = xk * d
        t0 = np.tanh(x)
        t0sq = t0 * t0
        om = np.sqrt(G * xk * t0)
        c0 = om / xk
        cssq = G * d
        vg = _vg(T, c0, x, False)
        vgsq = vg * vg
        a = t0 - x * (T(1) - t0sq)
        d2om = a * a + T(4) * (x * x) * t0sq * (T(1) - t0sq)
        xnl1 = (T(9) * (t0sq * t0sq) - T(10) * t0sq + T(9)) / (T(8) * t0sq * t0)
        b = T(2) * vg - T(0.5) * c0
        xnl2 = ((b * b) / (G * d - vgsq) + T(1)) / x
        e = T(2) * c0 + vg * (T(1) - t0sq)
        xnl4 = T(1) / (T(4) * t0) * (e * e) / (cssq - vgsq)
        alp = (T(1) - vgsq / cssq) * (c0 * c0) / vgsq
        zfac = (sig_th * sig_th) / (sig_th * sig_th + alp * (xnu * xnu))
        tnl = xnl1 - xnl2 + zfac * xnl4
        q = vg / c0
        r = np.maximum(np.minimum(T(4), T(4) * (q * q) * tnl * t0 / d2om), T(-4))
    shallow = (d < t.BATHYMAX) & (d > 0)
    return np.where(shallow & ~(xk0 * d > T(DKMAX)), r, T(1)).astype(T)


def transf_r(t, xk0, d):
    """TRANSF_R (transf_r.F90:325-346)."""
    T = t.dtype
    G = t.G
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xk = np.maximum(xk0, T(XKDMIN) / d)
        x = xk * d
        t0 = np.tanh(x)
        t0sq = t0 * t0
        om = np.sqrt(G * xk * t0)
        c0 = om / xk
        vg = _vg(T, c0, x, False)
        a = t0 - x * (T(1) - t0sq)
        d2om = a * a + T(4) * (x * x) * t0sq * (T(1) - t0sq)
        q = vg / c0
        r = T(4) * (q * q * q) * t0sq / d2om
    ok = (d < t.BATHYMAX) & (d > 0) & (xk0 > 0)
    return np.where(ok & ~(xk0 * d > T(DKMAX)), r, T(0.5)).astype(T)


def stat_nl(t, xm0, xk0, bf2, xnu, sig_th, d):
    """STAT_NL (stat_nl.F90:185-272): C3, C4, ETA_M, R."""
    T = t.dtype
    G, PI = t.G, t.PI
    ze, _ = zeps(T)
    sqrt3 = np.sqrt(T(3))
    c4c = T(0.9) * PI / (T(3) * sqrt3)
    zc1 = T(4) * sqrt3 / PI
    zc2 = T(1) / T(3) + T(2) * sqrt3 / PI
    zc3 = T(2) * sqrt3 / PI - T(4) / T(3)
    transf = transf_r(t, xk0, d)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xk = np.maximum(xk0, T(XKDMIN) / d)
        x = xk * d
        t0 = np.tanh(x)
        om = np.sqrt(G * xk * t0)
        t0sq = t0 * t0
        alph = xk / (T(4) * t0sq * t0) * (T(3) - t0sq)
        gam = T(-0.5) * (alph * alph)
        c0 = om / xk
        cssq = G * d
        vg = _vg(T, c0, x, True)
        vgsq = vg * vg
        zfac = T(-0.25) * xk * cssq / (cssq - vgsq)
        d1 = zfac * (T(2) * (T(1) - t0sq) / t0 + T(1) / x)
        zfac1 = T(0.5) * c0 * cssq * vg / t0
        xkap = zfac1 * (T(2) * c0 + vg * (T(1) - t0sq)) / (cssq - vgsq)
        alpha = (T(1) - vgsq / cssq) * (c0 * c0) / vgsq
        zfac2 = (sig_th * sig_th) / (sig_th * sig_th + alpha * (xnu * xnu))
        d2 = T(0.5) * (xk * xk) * xkap / (om * cssq) * zfac2
        delta = d1 + d2
        eta = T(2) * xm0 * delta
        c3 = np.maximum(np.minimum(T(0.25), T(1.12) * T(2) * np.sqrt(xm0) * (alph + T(0.9) * delta)), T(0))
        ad = alph + delta
        c4b = T(0.93) * T(8) * xm0 * (gam + alph * alph + ad * ad)
        q = sig_th / xnu
        r = np.maximum(np.minimum(transf * (q * q), T(16)), T(0))
        xj = np.where(r > 1, -c4c / r * (T(1) - zc1 / np.sqrt(r) + zc2 / r + zc3 / (r * r)),
                      c4c * (T(1) - zc1 * np.sqrt(r) + zc2 * r + zc3 * (r * r)))
        c4 = np.maximum(np.minimum(T(0.25), xj * bf2 + c4b), T(-0.25))
    ok = (xm0 > ze) & (d > 0) & (xk0 > 0)
    z = T(0)
    return tuple(np.where(ok, v, z).astype(T) for v in (c3, c4, eta, r))


def h_max(t, c3, c4, xnslc):
    """H_MAX (h_max.F90:91-125): HMAXN; and DFNORMA (for the near-decision test)."""
    T = t.dtype
    ze, _ = zeps(T)
    gam, eb = T(0.5772), T(10)
    twog1 = T(-2) * gam
    g2 = gam * gam + t.PI * t.PI / T(6)
    ae = T(0.5) * eb * (eb - T(2))
    be = T(0.5) * eb * (eb * eb - T(6) * eb + T(6))
    dfn = c4 * ae + c3 * c3 * be
    ok = (xnslc > 0) & (np.abs(dfn) > ze)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.log(np.maximum(T(1) + dfn, T(0.1)))
        ebf = eb - f
        aa = np.minimum((ebf * ebf - T(2) * eb) / (T(2) * f), T(1000))
        bb = T(2) * (T(1) + aa)
        bbm1 = T(1) / (bb + ze * np.where(bb < 0, T(-1), T(1)))
        e = np.full(c3.shape, T(8), T)
        for _ in range(5):
            z0 = np.log(xnslc * np.sqrt(T(0.5) * e))
            e = (g2 - twog1 * (aa + z0) + (T(2) * aa + z0) * z0) * bbm1
            e = np.minimum(np.maximum(e, T(2)), T(32))
        h = np.sqrt(T(0.5) * e)
    return np.where(ok, h, T(1)).astype(T), dfn


def w_mode_st(t, rn3, rn2, rn1):
    """W_MODE_ST (w_mode_st.F90:191-211): Newton for the mode, at most 20 steps."""
    T = t.dtype

    def F(x):
        return (x * (rn3 * x + rn2) + rn1) * np.exp(T(-0.5) * (x * x)) - T(1)

    def DF(x):
        return (-(x * x) * (rn3 * x + rn2) + (T(2) * rn3 - rn1) * x + rn1 + rn2) * np.exp(T(-0.5) * (x * x))

    with np.errstate(divide="ignore", invalid="ignore"):
        l3 = np.log(rn3)
        z0 = np.sqrt(T(2) * l3 + T(2) * np.log(T(2) * l3 + T(2) * np.log(T(2) * l3)))
        res = np.abs(F(z0))
        for _ in range(20):
            go = T(1.0e-6) < res
            if not go.any():
                break
            fp = DF(z0)
            z0 = np.where(go & (fp != 0), z0 - F(z0) / fp, z0).astype(T)
            res = np.where(go, np.abs(F(z0)), res)
    return z0


def kurtosis(t, fl1, depth):
    """KURTOSIS (kurtosis.F90:241-398): the nine columns 0-8 of FIELDS, the near-decision mask, and intermediates (XKP, SUM0, TRANS)."""
    T = t.dtype
    n, K, M = fl1.shape
    ze, zsq = zeps(T)
    frmax, frmin = t.FR[M - 1], t.FR[0]
    depth = np.asarray(depth, T)
    xnu, sig_th, _ = peak_ang(t, fl1)
    ffm = np.zeros((n, M), T)
    for m in range(M):                                                                # :257-267
        s = fl1[:, 0, m].copy()
        for k in range(1, K):
            s = s + fl1[:, k, m]
        ffm[:, m] = s
    ffmax = ffm[:, 0].copy()
    for m in range(1, M):
        ffmax = np.maximum(ffmax, ffm[:, m])
    s0 = np.full(n, ze, T)
    s1 = np.zeros(n, T)
    s2 = np.zeros(n, T)
    s6 = np.zeros(n, T)
    fr2 = t.DFIM * (t.FR * t.FR)
    for m in range(M):                                                                # :285-292
        s0 = s0 + ffm[:, m] * t.DFIM[m]
        s1 = s1 + ffm[:, m] * t.DFIMFR[m]
        s2 = s2 + ffm[:, m] * fr2[m]
        s6 = s6 + ffm[:, m] * t.DFIMOFR[m]
    fn = ffm[:, M - 1]
    s0 = s0 + t.WETAIL * frmax * t.DELTH * fn                                         # :294-303
    s1 = s1 + t.WP1TAIL * t.DELTH * (frmax * frmax) * fn
    s2 = s2 + T(WP2TAIL) * t.DELTH * (frmax * frmax * frmax) * fn
    s6 = s6 + t.FRTAIL * t.DELTH * fn
    s40 = np.full(n, zsq, T)                                                          # :306-321
    s4 = np.zeros(n, T)
    thr = T(0.4) * ffmax
    for m in range(M):
        fac4 = T(2) * t.DELTH * t.DFIMFR[m]
        sel = ffm[:, m] > thr
        s40 = np.where(sel, s40 + ffm[:, m] * t.DFIM[m], s40)
        s4 = np.where(sel, s4 + ffm[:, m] * ffm[:, m] * fac4, s4)
    ok = (s1 > zsq) & (s0 > ze)                                                       # :325-348
    with np.errstate(divide="ignore", invalid="ignore"):
        f_m = np.where(ok, np.maximum(np.minimum(s1 / s0, frmax), frmin), T(0)).astype(T)
        qp = np.where(ok, np.maximum(np.minimum(s4 / (s40 * s40), T(15)), T(0.5)), T(0)).astype(T)
        sig_om = T(1) / np.sqrt(t.PI) / qp
        cozpi = T(0.89) * t.ZPI
        om_mean = np.where(ok, cozpi * np.maximum(np.minimum(s0 / s6, frmax), frmin), cozpi * frmax).astype(T)
        xkp_n, astep, abo = aki(t, om_mean, depth)
        xkp = np.where(ok, xkp_n, om_mean * om_mean / t.G).astype(T)
        eps = xkp * np.sqrt(s0)
        trans = transf_bfi(t, xkp, depth, xnu, sig_th)
        q = eps / np.maximum(sig_om, ze)
        bf2 = np.where(ok, np.maximum(np.minimum(T(2) * trans * (q * q), T(5)), T(-5)), T(0)).astype(T)
    c3, c4, eta, r = stat_nl(t, s0, xkp, bf2, xnu, sig_th, depth)
    zfac = T(2) * t.ZPI / np.sqrt(t.ZPI)                                              # :367-376
    x = T(1200) * (zfac * xnu * f_m)
    xnslc = np.where(f_m > 0, nint(x), 0).astype(T)
    hmaxn, dfn = h_max(t, c3, c4, xnslc)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = xnu / (np.sqrt(T(2)) * hmaxn)
        z2 = z * z
        tmax = np.where((s1 > ze) & (hmaxn > ze), s0 / s1 * (T(1) + T(0.5) * z2 + T(0.75) * (z2 * z2)), T(0)).astype(T)
    hmax = np.where(s0 > 0, hmaxn * (T(4) * np.sqrt(s0)), T(0)).astype(T)
    # discrete decisions within the noise of the device's summation order and transcendental functions (single precision)
    sp = T == np.float32
    tol = 2e-6 if sp else 1e-13
    frac = np.abs(x - np.floor(x) - 0.5)
    near = (f_m > 0) & (frac < tol * np.abs(x))
    near |= ok & (np.abs(astep - 1e-4) < 1e3 * tol * 1e-4)
    bfx = xkp * depth
    near |= (depth < t.BATHYMAX) & (np.abs(bfx - DKMAX) < 1e2 * tol * DKMAX)
    near |= np.abs(np.abs(dfn) - ze) < 0.5 * ze
    out = np.stack([c4, bf2, qp, hmax, tmax, c3, eta, r, xnslc], 1).astype(T)
    return out, near, dict(xkp=xkp, sum0=s0, trans=trans)


def w_maxh(t, fl1, depth, wavnum):
    """W_MAXH (w_maxh.F90:106-333): CMAX_F, HMAX_N, CMAX_ST, HMAX_ST (columns 9-12 of FIELDS), and the near-decision mask."""
    T = t.dtype
    n, K, M = fl1.shape
    ze, _ = zeps(T)
    G, ZPI = t.G, t.ZPI
    depth = np.asarray(depth, T)
    omega = ZPI * t.FR
    tmin, tmx = T(1) / t.FR[M - 1], T(1) / t.FR[0]
    wvlmin = G / (ZPI * (t.FR[M - 1] * t.FR[M - 1]))
    kth = np.zeros(n, int)                                                            # :135-146
    fmax = np.zeros(n, T)
    for m in range(M):
        for k in range(K):
            up = fl1[:, k, m] > fmax
            fmax = np.where(up, fl1[:, k, m], fmax)
            kth = np.where(up, k, kth)
    ck, sk = t.COSTH[kth], t.SINTH[kth]
    cx = [t.COSTH[k] * ck + t.SINTH[k] * sk for k in range(K)]                       # :152-160
    cy = [t.SINTH[k] * ck - t.COSTH[k] * sk for k in range(K)]
    t1 = np.zeros(n, T)
    t2 = np.zeros(n, T)
    em = np.zeros(n, T)
    rlx = np.zeros(n, T)
    rly = np.zeros(n, T)
    axy = np.zeros(n, T)
    axt = np.zeros(n, T)
    ayt = np.zeros(n, T)
    tdf = np.zeros((n, M), T)
    fr2 = t.DFIM * (t.FR * t.FR)
    for m in range(M):                                                                # :163-197
        tp = np.zeros(n, T)
        tx = np.zeros(n, T)
        ty = np.zeros(n, T)
        tx2 = np.full(n, ze, T)
        ty2 = np.full(n, ze, T)
        txy = np.zeros(n, T)
        for k in range(K):
            f = fl1[:, k, m]
            tp = tp + f
            tx = tx + f * cx[k]
            ty = ty + f * cy[k]
            tx2 = tx2 + f * (cx[k] * cx[k])
            ty2 = ty2 + f * (cy[k] * cy[k])
            txy = txy + f * (cx[k] * cy[k])
        xk = wavnum[:, m]
        t1 = t1 + tp * t.DFIMFR[m]
        t2 = t2 + tp * fr2[m]
        em = em + tp * t.DFIM[m]
        tdf[:, m] = tp * t.DFIM[m]
        xk2d = (xk * xk) * t.DFIM[m]
        rlx = rlx + tx2 * xk2d
        rly = rly + ty2 * xk2d
        axy = axy + txy * xk2d
        xkz = xk * ZPI * t.DFIMFR[m]
        axt = axt + tx * xkz
        ayt = ayt + ty * xkz
    live = em > ze
    out = np.zeros((n, 4), T)
    near = np.zeros(n, bool)
    if not live.any():
        return out, near
    i = np.nonzero(live)[0]
    em_, t1_, t2_, rlx_, rly_ = em[i], t1[i], t2[i], rlx[i], rly[i]
    hs = T(4) * np.sqrt(em_ + t.WETAIL * t.FR[M - 1] * t.DELTH * tp[i])              # :200-208
    axy_ = np.minimum(axy[i] / np.sqrt(rlx_ * rly_), T(1))                            # :210-223
    axt_ = np.minimum(axt[i] / (ZPI * np.sqrt(rlx_ * t2_)), T(1))
    ayt_ = np.minimum(ayt[i] / (ZPI * np.sqrt(rly_ * t2_)), T(1))
    rlx_ = ZPI * np.sqrt(em_ / rlx_)
    rly_ = ZPI * np.sqrt(em_ / rly_)
    rni = np.sqrt(np.maximum(em_ * t2_ / (t1_ * t1_) - T(1), ze))
    zt = ZPI * t1_
    rmu = (zt * zt) * (T(1) - rni + rni * rni) / (G * np.power(em_, T(3) / T(2)))
    t1_ = np.minimum(np.maximum(em_ / t1_, tmin), tmx)
    t2_ = np.minimum(np.maximum(np.sqrt(em_ / t2_), tmin), tmx)
    wmdx, wmdy, wmdur = np.maximum(rlx_, wvlmin), np.maximum(rly_, wvlmin), T(100) * t2_
    # golden-section search (:242-272)
    grrm1 = T(2) / (T(1) + np.sqrt(T(5)))
    td = tdf[i]

    def acfs(tl):
        s = np.zeros(len(i), T)
        for m in range(M):
            s = s + np.cos(omega[m] * tl) * td[:, m]
        return s

    tl1, tl4 = T(0.3) * t2_, T(1.3) * t2_
    tl2, tl3 = tl4 - (tl4 - tl1) * grrm1, tl1 + (tl4 - tl1) * grrm1
    a2, a3 = acfs(tl2), acfs(tl3)
    acf = np.zeros(len(i), T)
    run = np.ones(len(i), bool)
    nr = np.zeros(len(i), bool)
    for _ in range(10):
        lo = a2 < a3
        acf = np.where(run, np.where(lo, a2, a3), acf)
        n4 = np.where(lo, tl3, tl4)
        n1 = np.where(lo, tl1, tl2)
        n2 = np.where(lo, n4 - (n4 - tl1) * grrm1, tl3)
        n3 = np.where(lo, tl2, n1 + (tl4 - n1) * grrm1)
        na2 = np.where(lo, acfs(n2), a3)
        na3 = np.where(lo, a2, acfs(n3))
        tl1, tl2, tl3, tl4 = (np.where(run, a, b) for a, b in ((n1, tl1), (n2, tl2), (n3, tl3), (n4, tl4)))
        a2, a3 = np.where(run, na2, a2), np.where(run, na3, a3)
        crit = np.abs(tl4 - tl1) - T(0.01) * (np.abs(tl2) + np.abs(tl3))
        run = run & ~(crit < 0)
        if not run.any():
            break
    ge = T(0.57721566)                                                                # :276-326
    sqrtem = T(0.25) * hs
    d = depth[i]
    wnum1, astep, _ = aki(t, ZPI / t1_, d)
    nr |= np.abs(astep - 1e-4) < (1e-3 if T == np.float32 else 1e-10) * 1e-4
    steep = ZPI * hs / (G * (t1_ * t1_))
    ursn = hs / ((wnum1 * wnum1) * (d * d * d))
    alfa = T(0.3536) + T(0.2568) * steep + T(0.08) * ursn
    beta = T(2) - T(1.7912) * steep - T(0.5302) * ursn + T(0.284) * (ursn * ursn)
    z0 = np.log(T(1200) / t2_)
    with np.errstate(invalid="ignore", divide="ignore"):
        cmax_f = alfa * np.power(z0, T(1) / beta) * (T(1) + ge / (beta * z0)) * hs
        phist = np.minimum(acf / em_, T(1))
        hmax_n = T(0.5) * np.sqrt(T(1) - phist) * np.sqrt(z0) * (T(1) + T(0.5) * ge / z0) * hs
        axyt = np.sqrt(T(1) + T(2) * axt_ * axy_ * ayt_ - axt_ * axt_ - axy_ * axy_ - ayt_ * ayt_)
        rn3 = ZPI * wmdx * wmdy * wmdur * axyt / (rlx_ * rly_ * t2_)
        rn2 = np.sqrt(ZPI) * (wmdx * wmdur / (rlx_ * t2_) * np.sqrt(T(1) - axt_ * axt_) + wmdx * wmdy / (rlx_ * rly_) * np.sqrt(T(1) - axy_ * axy_)
                              + wmdy * wmdur / (rly_ * t2_) * np.sqrt(T(1) - ayt_ * ayt_))
        rn1 = wmdx / rlx_ + wmdy / rly_ + wmdur / t2_
        z0 = w_mode_st(t, rn3, rn2, rn1)
        xx = T(1) / (z0 - (T(2) * rn3 * z0 + rn2) / (rn3 * (z0 * z0) + rn2 * z0 + rn1))
        cmax_st = ((z0 + T(0.5) * rmu * (z0 * z0)) + ge * ((T(1) + rmu * z0) * xx)) * sqrtem
        hmax_st = (z0 + ge * xx) * np.sqrt(T(2) * (T(1) - phist)) * sqrtem
    out[i] = np.stack([cmax_f, hmax_n, cmax_st, hmax_st], 1).astype(T)
    near[i] = nr
    return out, near


def extremes(t, fl1, depth, wavnum, kurtosis_only: bool = False):
    """Returns (out [n][13] in the columns FIELDS, near): near marks the points where a discrete decision (NINT, an AKI exit, the
    K D = DKMAX switch of TRANSF_BFI, H_MAX's ZEPSILON test) lies within the noise of single precision.  The golden-section
    search's comparisons are not counted: where two of its values are that close, either choice gives the same minimum to that noise.  kurtosis_only: columns 9-12 are 0."""
    fl1 = np.asarray(fl1, t.dtype)
    wavnum = np.asarray(wavnum, t.dtype)
    k, near, _ = kurtosis(t, fl1, depth)
    out = np.zeros((fl1.shape[0], len(FIELDS)), t.dtype)
    out[:, :9] = k
    if not kurtosis_only:
        w, nw = w_maxh(t, fl1, depth, wavnum)
        out[:, 9:] = w
        near = near | nw
    return out, near
