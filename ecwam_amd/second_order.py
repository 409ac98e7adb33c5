"""Tables of the second-order output spectrum (LSECONDORDER): SECONDHH_GEN (secondhh_gen.F90:73-121) and TABLES_2ND
(tables_2nd.F90:107-186) restated in numpy in the working precision, with the coupling functions of second_order_lib.F90, vmin.F90,
vplus.F90 and aki.F90 as array functions (one evaluation covers every depth, angle and frequency pair).

Only the thinning SECONDHH_GEN always selects is served: NFREH = NFRE/2, NANGH = NANG/2, MR = MA = 2.

Arrays are 0-based and C-ordered with the reference's index order: TA[JD][L][M1][M] = TA(JD+1,L+1,M1+1,M+1), IM_P[M1][M] = IM_P(M1+1,M+1)
(the values stay 1-based frequency numbers, 1 .. NMAX).  L counts the direction difference K - K1 wrapped to 1 .. NANGH, so L = NANGH
(index NANGH-1) is "same direction".
"""
from __future__ import annotations

import numpy as np

from .tables import Tables, powi

NDEPTH, DEPTHA, DEPTHD = 74, 1.0, 1.1  # mpuserin.F90:616-618
DKMAX = 40.0                           # yowpcons.F90:34


def nint(x):
    """Fortran NINT: to the nearest integer, halves away from zero."""
    x = np.asarray(x)
    return (np.sign(x) * np.floor(np.abs(x) + x.dtype.type(0.5))).astype(np.int64)


def aki(om, beta, G):
    """AKI (aki.F90:58-79): the wave number of angular frequency OM in depth BETA, Newton's method element by element."""
    om, beta = np.broadcast_arrays(om, beta)
    T = om.dtype.type
    om, beta = om.ravel().copy(), beta.ravel().copy()
    ao = np.maximum(om * om / (T(4.0) * G), om / (T(2.0) * np.sqrt(G * beta)))
    res = np.empty_like(om)
    act = np.arange(om.size)
    while act.size:
        o, b, a = om[act], beta[act], ao[act]
        bo = b * a
        big = bo > T(DKMAX)
        res[act[big]] = o[big] * o[big] / G
        keep = ~big
        act, o, b, a, bo = act[keep], o[keep], b[keep], a[keep], bo[keep]
        th = G * a * np.tanh(bo)
        sth = np.sqrt(th)
        an = a + (o - sth) * sth * T(2.0) / (th / a + G * bo / (np.cosh(bo) * np.cosh(bo)))
        ao[act] = an
        done = ~(np.abs(a - an) > T(0.0001) * an)
        res[act[done]] = an[done]
        act = act[~done]
    return res


class Coupling:
    """The functions of second_order_lib.F90 for depth(s) D (YOWCONST_2ND's DPTH), every argument an array of the working precision."""

    def __init__(self, D, G, PI, dtype):
        self.T = T = np.dtype(dtype).type
        self.D, self.G, self.PI = D, T(G), T(PI)

    def omeg(self, x):
        xk = np.abs(x)
        return np.sqrt(self.G * xk * np.tanh(xk * self.D))

    def vabs(self, xi, xj, thi, thj):
        T = self.T
        arg = xi * xi + xj * xj + T(2.0) * xi * xj * np.cos(thi - thj)
        return np.where(arg <= 0, T(0), np.sqrt(np.maximum(arg, T(0))))

    def vdir(self, xi, xj, thi, thj):
        y = xj * np.sin(thj - thi)
        x = xi + xj * np.cos(thj - thi)
        return np.where(x == 0, self.T(0), np.arctan2(y, x) + thi)

    def _v3(self, xi, xj, xk, thi, thj, thk, s):
        T, G = self.T, self.G
        del1 = T(10.0) ** (-12)
        zconst = T(1.0) / (T(4.0) * np.sqrt(T(2.0)))
        oi, oj, ok = self.omeg(xi) + del1, self.omeg(xj) + del1, self.omeg(xk) + del1
        qi, qj, qk = oi * oi / G, oj * oj / G, ok * ok / G
        rij = xi * xj * np.cos(thj - thi)
        rik = xi * xk * np.cos(thk - thi)
        rjk = xj * xk * np.cos(thk - thj)
        sqijk = np.sqrt(G * ok / (oi * oj))
        sqikj = np.sqrt(G * oj / (oi * ok))
        sqjki = np.sqrt(G * oi / (oj * ok))
        return zconst * ((rij + s * qi * qj) * sqijk + (rik + s * qi * qk) * sqikj + (rjk + qj * qk) * sqjki)

    def vmin(self, xi, xj, xk, thi, thj, thk):
        return self._v3(xi, xj, xk, thi, thj, thk, self.T(-1.0))

    def vplus(self, xi, xj, xk, thi, thj, thk):
        return self._v3(xi, xj, xk, thi, thj, thk, self.T(1.0))

    def a1(self, xi, xj, xk, thi, thj, thk):
        d = self.T(10.0) ** (-8)
        oi, oj, ok = self.omeg(xi) + d, self.omeg(xj) + d, self.omeg(xk) + d
        return -self.vmin(xi, xj, xk, thi, thj, thk) / (oi - oj - ok)

    def a2(self, xi, xj, xk, thi, thj, thk):
        return self.T(-2.0) * self.a1(xk, xj, xi, thk, thj, thi)

    def a3(self, xi, xj, xk, thi, thj, thk):
        d = self.T(10.0) ** (-8)
        oi, oj, ok = self.omeg(xi) + d, self.omeg(xj) + d, self.omeg(xk) + d
        return -self.vplus(xi, xj, xk, thi, thj, thk) / (oi + oj + ok)

    def A(self, xi, xj, thi, thj):
        T, G, PI = self.T, self.G, self.PI
        rk, thk = self.vabs(xi, xj, thi, thj), self.vdir(xi, xj, thi, thj)
        fi, fj, fk = (np.sqrt(self.omeg(r) / (T(2.0) * G)) for r in (xi, xj, rk))
        return fk / (fi * fj) * (self.a1(rk, xi, xj, thk, thi, thj) + self.a3(rk, xi, xj, thk - PI, thi, thj))

    def B(self, xi, xj, thi, thj):
        T, G, PI = self.T, self.G, self.PI
        rk, thk = self.vabs(xj, xi, thj, thi - PI), self.vdir(xj, xi, thj, thi - PI)
        fi, fj, fk = (np.sqrt((self.omeg(r) + T(0.0)) / (T(2.0) * G)) for r in (xi, xj, rk))
        return T(0.5) * fk / (fi * fj) * (self.a2(rk, xi, xj, thk, thi, thj) + self.a2(rk, xj, xi, thk - PI, thj, thi))

    def U(self, xi, xj, xk, xl, thi, thj, thk, thl):
        T, G = self.T, self.G
        oi, oj, ok, ol = self.omeg(xi), self.omeg(xj), self.omeg(xk), self.omeg(xl)
        oik = self.omeg(self.vabs(xi, xk, thi, thk))
        ojk = self.omeg(self.vabs(xj, xk, thj, thk))
        oil = self.omeg(self.vabs(xi, xl, thi, thl))
        ojl = self.omeg(self.vabs(xj, xl, thj, thl))
        qi, qj = oi * oi / G, oj * oj / G
        qik, qjk, qil, qjl = oik * oik / G, ojk * ojk / G, oil * oil / G, ojl * ojl / G
        sq = np.sqrt(ok * ol / (oi * oj))
        return T(1.0) / T(16.0) * sq * (T(2.0) * (xi * xi * qj + xj * xj * qi) - qi * qj * (qik + qjk + qil + qjl))

    def W1(self, xi, xj, xk, xl, thi, thj, thk, thl):
        U, p = self.U, thi - self.PI
        w = (-U(xi, xj, xk, xl, p, thj, thk, thl) - U(xi, xk, xj, xl, p, thk, thj, thl) - U(xi, xl, xj, xk, p, thl, thj, thk)
             + U(xj, xk, xi, xl, thj, thk, p, thl) + U(xj, xl, xi, xk, thj, thl, p, thk) + U(xk, xl, xi, xj, thk, thl, p, thj))
        return w / self.T(3.0)

    def W2(self, xi, xj, xk, xl, thi, thj, thk, thl):
        U, pi, pj = self.U, thi - self.PI, thj - self.PI
        return (U(xi, xj, xk, xl, pi, pj, thk, thl) + U(xk, xl, xi, xj, thk, thl, pi, pj) - U(xk, xj, xi, xl, thk, pj, pi, thl)
                - U(xi, xk, xj, xl, pi, thk, pj, thl) - U(xi, xl, xk, xj, pi, thl, thk, pj) - U(xl, xj, xk, xi, thl, pj, thk, pi))

    def V2(self, xi, xj, xk, xl, thi, thj, thk, thl):
        T, PI = self.T, self.PI
        vabs, vdir, omeg, vmin, vplus = self.vabs, self.vdir, self.omeg, self.vmin, self.vplus
        del1 = T(10.0) ** (-5)
        ri, rj, rk = xi + del1, xj + del1 / T(2.0), xk + del1 / T(3.0)
        rl = xl + del1 * (T(1.0) + T(1.0) / T(2.0) - T(1.0) / T(3.0))
        oi, oj, ok, ol = omeg(ri), omeg(rj), omeg(rk), omeg(rl)
        rij, thij = vabs(ri, rj, thi, thj), vdir(ri, rj, thi, thj)
        rik, thik = vabs(ri, rk, thi, thk - PI), vdir(ri, rk, thi, thk - PI)
        rli, thli = vabs(rl, ri, thl, thi - PI), vdir(xl, xi, thl, thi - PI)
        rjl, thjl = vabs(rj, rl, thj, thl - PI), vdir(rj, rl, thj, thl - PI)
        rjk, thjk = vabs(rj, rk, thj, thk - PI), vdir(rj, rk, thj, thk - PI)
        rkl, thkl = vabs(rk, rl, thk, thl), vdir(rk, rl, thk, thl)
        oij, oik, ojl, ojk, oli, okl = omeg(rij), omeg(rik), omeg(rjl), omeg(rjk), omeg(rli), omeg(rkl)
        xnik, xnjl, xnjk, xnil = ok + oik - oi, oj + ojl - ol, ok + ojk - oj, oi + oli - ol
        ynil, ynjk, ynjl, ynik = ol + oli - oi, oj + ojk - ok, ol + ojl - oj, oi + oik - ok
        znij, znkl, zpij, zpkl = oij - oi - oj, okl - ok - ol, oij + oi + oj, okl + ok + ol
        thlj, thil, thkj, thki, thji, thlk = thjl - PI, thli - PI, thjk - PI, thik - PI, thij - PI, thkl - PI
        one = T(1.0)
        v = (vmin(ri, rk, rik, thi, thk, thik) * vmin(rl, rj, rjl, thl, thj, thlj) * (one / xnik + one / xnjl)
             + vmin(rj, rk, rjk, thj, thk, thjk) * vmin(rl, ri, rli, thl, thi, thli) * (one / xnjk + one / xnil)
             + vmin(ri, rl, rli, thi, thl, thil) * vmin(rk, rj, rjk, thk, thj, thkj) * (one / ynil + one / ynjk)
             + vmin(rj, rl, rjl, thj, thl, thjl) * vmin(rk, ri, rik, thk, thi, thki) * (one / ynjl + one / ynik)
             + vmin(rij, ri, rj, thij, thi, thj) * vmin(rkl, rk, rl, thkl, thk, thl) * (one / znij + one / znkl)
             + vplus(rij, ri, rj, thji, thi, thj) * vplus(rkl, rk, rl, thlk, thk, thl) * (one / zpij + one / zpkl))
        return -v

    def B2(self, ri, rj, rk, rl, thi, thj, thk, thl):
        PI, vabs, vdir, a1, a3 = self.PI, self.vabs, self.vdir, self.a1, self.a3
        rij, thij = vabs(ri, rj, thi, thj), vdir(ri, rj, thi, thj)
        rik, thik = vabs(ri, rk, thi, thk - PI), vdir(ri, rk, thi, thk - PI)
        rki, thki = vabs(rk, ri, thk, thi - PI), vdir(rk, ri, thk, thi - PI)
        ril, thil = vabs(ri, rl, thi, thl - PI), vdir(ri, rl, thi, thl - PI)
        rli, thli = vabs(rl, ri, thl, thi - PI), vdir(rl, ri, thl, thi - PI)
        rjl, thjl = vabs(rj, rl, thj, thl - PI), vdir(rj, rl, thj, thl - PI)
        rlj, thlj = vabs(rl, rj, thl, thj - PI), vdir(rl, rj, thl, thj - PI)
        rjk, thjk = vabs(rj, rk, thj, thk - PI), vdir(rj, rk, thj, thk - PI)
        rkj, thkj = vabs(rk, rj, thk, thj - PI), vdir(rk, rj, thk, thj - PI)
        rkl, thkl = vabs(rk, rl, thk, thl), vdir(rk, rl, thk, thl)
        return (a3(ri, rj, rij, thi, thj, thij - PI) * a3(rk, rl, rkl, thk, thl, thkl - PI)
                + a1(rj, rk, rjk, thj, thk, thjk) * a1(rl, ri, rli, thl, thi, thli)
                + a1(rj, rl, rjl, thj, thl, thjl) * a1(rk, ri, rki, thk, thi, thki)
                - a1(rij, ri, rj, thij, thi, thj) * a1(rkl, rk, rl, thkl, thk, thl)
                - a1(ri, rk, rik, thi, thk, thik) * a1(rl, rj, rlj, thl, thj, thlj)
                - a1(ri, rl, ril, thi, thl, thil) * a1(rk, rj, rkj, thk, thj, thkj))

    def B3(self, ri, rj, rk, rl, thi, thj, thk, thl):
        T, PI = self.T, self.PI
        vabs, vdir, omeg, vmin, vplus, a1, a3 = self.vabs, self.vdir, self.omeg, self.vmin, self.vplus, self.a1, self.a3
        del1 = T(10.0) ** (-5)
        oi, oj, ok, ol = omeg(ri) + del1, omeg(rj) + del1, omeg(rk) + del1, omeg(rl) + del1
        rij, thij = vabs(ri, rj, thi, thj), vdir(ri, rj, thi, thj)
        rji, thji = vabs(rj, ri, thj, thi), vdir(rj, ri, thj, thi)
        rik, thik = vabs(ri, rk, thi, thk), vdir(ri, rk, thi, thk)
        rki, thki = vabs(rk, ri, thk, thi), vdir(rk, ri, thk, thi)
        rlj, thlj = vabs(rl, rj, thl, thj - PI), vdir(rl, rj, thl, thj - PI)
        rjl, thjl = vabs(rj, rl, thj, thl - PI), vdir(rj, rl, thj, thl - PI)
        rjk, thjk = vabs(rj, rk, thj, thk), vdir(rj, rk, thj, thk)
        rli, thli = vabs(rl, ri, thl, thi - PI), vdir(rl, ri, thl, thi - PI)
        ril, thil = vabs(ri, rl, thi, thl - PI), vdir(ri, rl, thi, thl - PI)
        rlk, thlk = vabs(rl, rk, thl, thk - PI), vdir(rl, rk, thl, thk - PI)
        rkl, thkl = vabs(rk, rl, thk, thl - PI), vdir(rk, rl, thk, thl - PI)
        z = oi + oj + ok - ol
        return -T(1.0) / z * (T(2.0) * (
            vmin(rl, ri, rli, thl, thi, thli) * a1(rjk, rj, rk, thjk, thj, thk)
            - vmin(rij, ri, rj, thij, thi, thj) * a1(rl, rk, rlk, thl, thk, thlk)
            - vmin(rik, ri, rk, thik, thi, thk) * a1(rl, rj, rlj, thl, thj, thlj)
            - vplus(rj, ri, rji, thj, thi, thji - PI) * a1(rk, rl, rkl, thk, thl, thkl)
            - vplus(rk, ri, rki, thk, thi, thki - PI) * a1(rj, rl, rjl, thj, thl, thjl)
            + vmin(ri, rl, ril, thi, thl, thil) * a3(rj, rk, rjk, thj, thk, thjk - PI))
            + T(3.0) * self.W1(rl, rk, rj, ri, thl, thk, thj, thi))

    def C_QL(self, xk0, xk1, th0, th1):
        T = self.T
        f1 = np.sqrt(self.omeg(xk1) / (T(2.0) * self.G))
        return T(2.0) / (f1 * f1) * (self.B2(xk0, xk1, xk1, xk0, th0, th1, th1, th0)
                                     + self.B3(xk0, xk0, xk1, xk1, th0 - self.PI, th0, th1, th1))


class SecondOrderTables:
    """SECONDHH_GEN + TABLES_2ND for the spectral grid of ``t`` (a Tables), in its precision."""

    def __init__(self, t: Tables, ndepth: int = NDEPTH, deptha: float = DEPTHA, depthd: float = DEPTHD):
        NANG, NFRE = t.cfg.nang, t.cfg.nfre
        if NANG % 2 or NFRE % 2:
            raise ValueError(f"second-order spectrum: NANG = {NANG} and NFRE = {NFRE} must both be even (SECONDHH_GEN thins with MR = MA = 2)")
        T = self.dtype = t.dtype
        self.t = t
        self.NDEPTH, self.DEPTHA, self.DEPTHD = int(ndepth), T(deptha), T(depthd)
        self.NFREH, self.NANGH = NFRE // 2, NANG // 2
        self.MR = NFRE // self.NFREH
        self.MA = NANG // self.NANGH
        self.XMR = T(1.0) / T(self.MR)
        NH, AH, MR, MA = self.NFREH, self.NANGH, self.MR, self.MA
        self.FRAC = t.FRATIO - T(1.0)
        self.OMSTART = t.ZPI * t.FR[0]
        self.DELTHH = T(MA) * t.DELTH
        self.OMEGA = t.ZPI * t.FR[MR * np.arange(1, NH + 1) - 1]
        k0 = MA * np.arange(1, AH + 1) + 1
        k0 = np.where(k0 > NANG, k0 - NANG, k0)
        self.K0 = k0 - 1                                      # 0-based direction of the full grid behind each thinned one
        self.THH = t.TH[self.K0]
        co1 = T(1.0) / T(2.0) * self.DELTHH / t.ZPI
        d = np.empty(NH, T)
        d[0] = co1 * (self.OMEGA[1] - self.OMEGA[0])
        d[1:-1] = co1 * (self.OMEGA[2:] - self.OMEGA[:-2])
        d[-1] = co1 * (self.OMEGA[-1] - self.OMEGA[-2])
        self.DFDTH = d
        xlf = np.log(T(1.0) + self.FRAC)
        # INTEGER = 1 + REAL: the assignment truncates (22 at NFRE = 36)
        self.NMAX = int(T(1.0) + self.XMR * T(1 + int(nint(np.log(T(2.0) * self.OMEGA[-1] / self.OMSTART) / xlf))))
        self._tables_2nd(xlf)

    def _tables_2nd(self, xlf) -> None:
        t, T, NH, AH, ND = self.t, self.dtype, self.NFREH, self.NANGH, self.NDEPTH
        G = t.G
        OM = self.OMEGA
        dpth = np.array([self.DEPTHA * powi(self.DEPTHD, jd) for jd in range(ND)], T)      # DEPTHA*DEPTHD**(JD-1)
        self.DPTH = dpth
        self.TFAK = aki(OM[:, None], dpth[None, :], G).reshape(NH, ND)      # TFAK(M,JD)
        # axes [JD][L][M1][M]
        D = dpth[:, None, None, None]
        om0, om1 = OM[None, None, None, :], OM[None, None, :, None]
        xk = self.TFAK.T                                                       # [JD][M]
        xk0, xk1 = xk[:, None, None, :], xk[:, None, :, None]
        mp = np.minimum(np.arange(NH) + 1, NH - 1)
        mm = np.maximum(np.arange(NH) - 1, 0)
        xk0p, xk0m = xk[:, mp][:, None, None, :], xk[:, mm][:, None, None, :]
        th0 = self.THH[None, :, None, None]
        th1 = self.THH[AH - 1]
        dfdth1 = self.DFDTH[None, None, :, None]
        c = Coupling(D, G, t.PI, T)
        shape = (ND, AH, NH, NH)
        with np.errstate(all="ignore"):
            minus = np.abs(om1) < om0 / T(2.0)                                 # [1][1][M1][M]
            om2 = np.where(minus, om0 - om1, OM[0])
            xm2 = np.log(om2 / self.OMSTART) / xlf
            self.IM_M = np.where(minus, nint(self.XMR * (xm2 + T(1.0))), 1)[0, 0].astype(np.int32)
            xk2 = aki(np.broadcast_to(om2, (ND, 1, NH, NH)), np.broadcast_to(D, (ND, 1, NH, NH)), G).reshape(ND, 1, NH, NH)
            a = c.A(np.broadcast_to(xk1, shape), np.broadcast_to(xk2, shape), th1, th0)
            self.TA = np.where(minus, dfdth1 * (a * a), T(0)).astype(T)
            om2 = om1 + om0
            xm2 = np.log(om2 / self.OMSTART) / xlf
            self.IM_P = nint(self.XMR * (xm2 + T(1.0)))[0, 0].astype(np.int32)
            xk2 = aki(np.broadcast_to(om2, (ND, 1, NH, NH)), np.broadcast_to(D, (ND, 1, NH, NH)), G).reshape(ND, 1, NH, NH)
            b = c.B(np.broadcast_to(xk1, shape), np.broadcast_to(xk2, shape), th1, th0)
            self.TB = (dfdth1 * (b * b)).astype(T)
            self.TC_QL = (dfdth1 * c.C_QL(np.broadcast_to(xk0, shape), np.broadcast_to(xk1, shape), th0, th1)).astype(T)
            fac = T(2.0) * G / om1 * dfdth1
            x1 = np.broadcast_to(xk1, shape)
            for name, x0 in (("TT_4M", np.broadcast_to(xk0m, shape)), ("TT_4P", np.broadcast_to(xk0p, shape))):
                w = c.W2(x0, x1, x1, x0, th0, th1, th1, th0) + c.V2(x0, x1, x1, x0, th0, th1, th1, th0)
                setattr(self, name, (fac * w).astype(T))

    COEFFICIENTS = ("TA", "TB", "TC_QL", "TT_4M", "TT_4P")
