"""CAL_SECOND_ORDER_SPEC (cal_second_order_spec.F90:91-193, the thinning path MR = MA = 2), FKMEAN (fkmean.F90:100-150) and SECSPOM
(secspom.F90:127-288) restated in numpy in the working precision: every output bin takes its additions in the reference's order (M1
outer, K1 inner, the TA term before the XINCR term), vectorised over the points and the output directions only.  Alongside each sum
comes the sum of the absolute values of what was added, which is what a rounding bound on the sum is stated in.

Indices are 0-based; `so` is an ecwam_amd.second_order.SecondOrderTables.
"""
import numpy as np

from ecwam_amd.second_order import nint
from ecwam_amd.tables import powi

GAM_B_J = 0.6


def fkmean(t, f1, wavnum):
    """(EMEAN, AKMEAN) of FKMEAN, the sums over M one after the other."""
    T = t.dtype
    n, NANG, NFRE = f1.shape
    em = np.full(n, t.EPSMIN, T)
    ak = np.full(n, t.EPSMIN, T)
    delt25 = t.WETAIL * t.FR[-1] * t.DELTH
    coefa = t.FRTAIL * t.DELTH * np.sqrt(t.G) / t.ZPI
    for m in range(NFRE):
        sqrtk = np.sqrt(wavnum[:, m])
        tempa = t.DFIM[m] / sqrtk
        temp2 = f1[:, 0, m].copy()
        for k in range(1, NANG):
            temp2 = temp2 + f1[:, k, m]
        em = em + t.DFIM[m] * temp2
        ak = ak + tempa * temp2
    em = em + delt25 * temp2
    ak = ak + coefa * temp2
    q = em / ak
    return em.astype(T), (q * q).astype(T)


def depth_index(so, akmean, depth):
    """JD, 0-based (secspom.F90:127-135)."""
    T = so.dtype
    xd = np.maximum(T(1.0) / akmean, depth)
    xd = np.log(xd / so.DEPTHA) / np.log(so.DEPTHD) + T(1.0)
    return (np.clip(nint(xd), 1, so.NDEPTH) - 1).astype(np.int64)


def thin(so, f1):
    """PF1 [n][NANGH][NFREH]."""
    m0 = so.MR * np.arange(1, so.NFREH + 1) - 1
    return np.ascontiguousarray(f1[:, so.K0][:, :, m0])


def omega_ext(so):
    """OMEGA_EXT(1 .. NMAX) and OMRT(NFREH+1 .. NMAX) (zero below)."""
    T = so.dtype
    NH = so.NFREH
    ome = np.zeros(so.NMAX, T)
    omrt = np.zeros(so.NMAX, T)
    ome[:NH] = so.OMEGA
    omg5 = powi(so.OMEGA[-1], 5)
    for m in range(NH + 1, so.NMAX + 1):
        ome[m - 1] = so.OMSTART * powi(T(1.0) + so.FRAC, so.MR * m - 1)
        omrt[m - 1] = omg5 / powi(ome[m - 1], 5)
    return ome, omrt


def secspom(so, pf1, jd, tables=None):
    """(F3, S) [n][NANGH][NFREH]: the second-order increment of the thinned spectrum and the sum of |terms| of each bin.
    tables: the five coefficient arrays [JD][L][M1][M] (default: those of `so`)."""
    T = so.dtype
    n, AH, NH = pf1.shape
    NMAX = so.NMAX
    TA, TB, TC, T4M, T4P = tables if tables is not None else [getattr(so, c) for c in so.COEFFICIENTS]
    ome, omrt = omega_ext(so)
    f2 = np.zeros((n, AH, NMAX), T)
    f2[:, :, :NH] = pf1
    for m in range(NH, NMAX):
        f2[:, :, m] = omrt[m] * pf1[:, :, NH - 1]
    f3 = np.zeros((n, AH, NH), T)
    sa = np.zeros((n, AH, NH), np.float64)
    kk = np.arange(AH)
    a64 = lambda x: np.abs(x).astype(np.float64)
    for m in range(NH):
        om0h = T(0.5) * so.OMEGA[m]
        mp, mm = min(m + 1, NMAX - 1), max(m - 1, 0)
        delm1 = T(1.0) / (ome[mp] - so.OMEGA[mm])
        dkp, dkm = f2[:, :, mp] * delm1, f2[:, :, mm] * delm1            # [n][K]
        f0 = f2[:, :, m]
        psum = np.zeros((n, AH), T)
        s = np.zeros((n, AH), np.float64)
        for m1 in range(NH):
            m2m, m2p = so.IM_M[m1, m] - 1, so.IM_P[m1, m] - 1
            r1, rm, rp = f2[:, :, m1], f2[:, :, m2m], f2[:, :, m2p]
            minus = abs(so.OMEGA[m1]) < om0h
            for k1 in range(AH):
                l = (kk - k1 - 1) % AH                                    # L = K - K1 wrapped to 1 .. NANGH, 0-based; [K]
                cf = lambda tab: tab[jd[:, None], l[None, :], m1, m]      # [n][K]
                a, b = r1[:, k1:k1 + 1], rm[:, k1:k1 + 1]
                if minus:
                    ta = cf(TA)
                    p1, p2 = a * rm, r1 * b
                    psum = psum + ta * (p1 + p2)
                    s += a64(ta) * (a64(p1) + a64(p2))
                tb, tc, t4m, t4p = cf(TB), cf(TC), cf(T4M), cf(T4P)
                x1 = T(2.0) * tb * rp
                x2 = tc * f0
                x3, x4 = dkp * t4p, dkm * t4m
                xincr = (x1 + x2) - (x3 - x4)
                psum = psum + a * xincr
                s += a64(a) * (a64(x1) + a64(x2) + a64(x3) + a64(x4))
        f3[:, :, m] = psum
        sa[:, :, m] = s
    return f3, sa


def interpolation_weights(so):
    """Per full-grid M: (M0, MP, D1); per full-grid K: (K0, KP, D3) -- 0-based thinned indices (cal_second_order_spec.F90:156-181)."""
    t, T = so.t, so.dtype
    NANG, NFRE, NH, AH, MR, MA = t.cfg.nang, t.cfg.nfre, so.NFREH, so.NANGH, so.MR, so.MA
    fm, fk = [], []
    for M in range(1, NFRE + 1):
        m0 = M // MR
        if m0 < 1:
            m0, mp, d1 = 1, 2, T(1.0)
        elif m0 < NH:
            mp = m0 + 1
            d1 = (t.FR[M - 1] - t.FR[MR * m0 - 1]) / (t.FR[MR * mp - 1] - t.FR[MR * m0 - 1])
        else:
            m0, mp, d1 = NH, NH, T(0.0)
        fm.append((m0 - 1, mp - 1, T(d1)))
    for K in range(1, NANG + 1):
        k0 = (K - 1) // MA
        d3 = T(K - 1) / T(MA) - T(k0)
        if k0 < 1:
            k0 += AH
        kp = k0 + 1
        if kp > AH:
            kp -= AH
        fk.append((k0 - 1, kp - 1, T(d3)))
    return fm, fk


def cal_second_order_spec(so, f1, wavnum, depth, sig=1.0, tables=None):
    """F1 with the second-order correction added (SIG = +1) or removed (SIG = -1).  Returns (F1 new, info): info["bound"] [n][NANG][NFRE]
    is the sum of |terms| behind each bin (the interpolated sums of SECSPOM and |F1| itself), info["terms"] their number."""
    t, T = so.t, so.dtype
    f1 = np.asarray(f1, T)
    n, NANG, NFRE = f1.shape
    depth = np.asarray(depth, T)
    em, ak = fkmean(t, f1, np.asarray(wavnum, T))
    jd = depth_index(so, ak, depth)
    pf1 = thin(so, f1)
    pf3, s3 = secspom(so, pf1, jd, tables)
    zfac = T(GAM_B_J) * T(GAM_B_J) / T(16.0)
    emaxl = np.where(em <= zfac * (depth * depth), T(1.0), T(0.0)).astype(T)
    fm, fk = interpolation_weights(so)
    out = np.empty_like(f1)
    bound = np.empty(f1.shape, np.float64)
    es = emaxl * T(sig)
    small = T(0.000001)
    for M, (m0, mp, d1) in enumerate(fm):
        d2 = T(1.0) - d1
        for K, (k0, kp, d3) in enumerate(fk):
            d4 = T(1.0) - d3
            c1 = pf3[:, k0, m0] * d4 + pf3[:, kp, m0] * d3
            c2 = pf3[:, kp, mp] * d3 + pf3[:, k0, mp] * d4
            delf = c1 * d2 + c2 * d1
            f = f1[:, K, M]
            out[:, K, M] = np.maximum(np.minimum(small, f), f + es * delf)
            b1 = s3[:, k0, m0] * float(d4) + s3[:, kp, m0] * float(d3)
            b2 = s3[:, kp, mp] * float(d3) + s3[:, k0, mp] * float(d4)
            # (where EMAXL = 0 the product EMAXL SIG DELF is an exact zero: nothing but F1 stands behind the bin)
            bound[:, K, M] = np.abs(f).astype(np.float64) + np.where(emaxl > 0, b1 * float(d2) + b2 * float(d1), 0.0)
    terms = 4 * so.NANGH * so.NFREH + 8
    return out, dict(bound=bound, terms=terms, jd=jd, emaxl=emaxl, emean=em, akmean=ak, pf1=pf1, pf3=pf3)


def device_case(t, so, n: int = 203, seed: int = 5):
    """Inputs of tests/test_gpu_second_order.py: (FL1 [n][NANG][NFRE], WAVNUM [n][NFRE], DEPTH [n]).  Rows 3 .. 66 (the first wavefront of a
    call with kijs = 3) cycle through five depth indices, rows 67 .. 130 are all deep (one depth index: LLSAMEDPTH), the rest are shallow:
    0.5 m and 1 m (JD = 1), 0.05 m (1/AKMEAN exceeds DEPTH), 8 m and 20 m with enough energy for the EMAXL switch."""
    import harness as H
    from ecwam_amd.second_order import aki

    T = t.dtype
    prec = "sp" if T == np.float32 else "dp"
    fl1 = np.ascontiguousarray(H.make_point_case(n, t.cfg, prec, spectra="mixed", seed=seed)["FL1"], T)
    grid = so.DPTH
    depth = np.empty(n, T)
    depth[:3] = 40.0
    depth[3:67] = grid[np.array([10, 30, 50, 60, 73])[np.arange(64) % 5]]
    depth[67:131] = 5000.0
    depth[131:] = np.array([0.5, 1.0, 0.05, 8.0, 20.0], T)[np.arange(n - 131) % 5]
    om = (t.ZPI * t.FR).astype(T)
    wavnum = aki(om[None, :], depth[:, None], t.G).reshape(n, len(t.FR)).astype(T)
    return fl1, wavnum, depth


def near_tie(f, gate):
    """Points whose peak period is not determined within the gate: DOMINANT_PERIOD keeps the bins above 0.1 MAX(F), so a bin within its
    error gate of that threshold may fall on either side.  f, gate: [n][NANG][NFRE]."""
    f = f.astype(np.float64)
    fmax = f.max(axis=(1, 2), keepdims=True)
    gmax = np.take_along_axis(gate.reshape(len(f), -1), f.reshape(len(f), -1).argmax(1)[:, None], 1)[:, :, None]
    return (np.abs(f - 0.1 * fmax) <= gate + 0.1 * gmax).any(axis=(1, 2))
