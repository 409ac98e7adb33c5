"""numpy restatement of SEPWISW with LLPARTITION = T (outblock.F90:214-382 and 436-449 with FL2ND = FL1): the wind-sea / swell split of
sepwisw_ref.py, then SEP3TR with FNDPRT and PARMEAN, which rewrite the swell mask before the swell and wind-sea parameters are taken.
What ecwam_hip_outbs_partition computes, in the working precision of the tables (float32 arrays and float32 operations in sp, so that the
discrete decisions -- the smoothing, the peak comparisons, FL > FL of FNDPRT 2.b, the noise and HSMIN tests -- are the device's), vectorised
over points, with the sums in the reference's order.  Test infrastructure only: the device kernel is checked against it.

  SEPWISW   sepwisw.F90:146-275          SEP3TR   sep3tr.F90 (FRINVMIJ is an INTEGER there: 1/FR(MIJ) truncated)
  FNDPRT    fndprt.F90                   PARMEAN  parmean.F90        SEMEAN  semean.F90
  FLMIN     yowice.F90 (FLLOW)           NPMAX = 20: yowpcons.F90    NTRAIN = 3 (42-50 are 3 trains x 3 fields)

FNDPRT's iteration has two forms: `literal` visits the bins of a sweep one after the other in the reference's loop order; the default
updates a whole sweep at once (2.b, then 2.c).  The two agree because within one sweep neither step depends on the order of the bins:
2.b only turns W2 = 0.5 into 1 and reads W2 = 0.5 of the bin and W2 = 0 of its neighbours, which such a change leaves alone; 2.c only
turns W2 = 0 into 0.5 and reads W2 = 0 of the bin itself and W2 = 1 of its neighbours (tests/test_outbs_partition_host.py checks it).
"""
from __future__ import annotations

import numpy as np

import sepwisw_ref as S

FIELDS = S.FIELDS + ("swh1", "mwd1", "mwp1", "swh2", "mwd2", "mwp2", "swh3", "mwd3", "mwp3")
NPMAX, NTRAIN = 20, 3
DEG = 57.295778667                         # yowpcons.F90:31


def nangh(t) -> int:
    """NINT((75/360) NANG) + 1 in the working precision; NINT rounds half away from zero (2.5 at 12 directions, 7.5 at 36)."""
    T = t.dtype
    x = float((T(75.0) / T(360.0)) * T(len(t.TH)))
    return int(np.floor(x + 0.5)) + 1


def semean(t, F):
    """SEMEAN with LLEPSMIN = F: sum over M of DFIM(M) * sum_K F, the tail on the last frequency."""
    T = t.dtype
    n, K, M = F.shape
    em = np.zeros(n, T)
    for m in range(M):
        temp = F[:, 0, m]
        for k in range(1, K):
            temp = temp + F[:, k, m]
        em = em + t.DFIM[m] * temp
    return em + (t.WETAIL * t.FR[M - 1] * t.DELTH) * temp


def parmean(t, spec):
    """PARMEAN of one partition per point: spec [n][K][M] -> (ENE, DIR, PER), 0 where EM <= EPSMIN."""
    T = t.dtype
    n, K, M = spec.shape
    eps = t.EPSMIN
    em = np.full(n, eps, T)
    fm = np.full(n, eps, T)
    for m in range(M):
        f1d = spec[:, 0, m]
        for k in range(1, K):
            f1d = f1d + spec[:, k, m]
        em = em + f1d * t.DFIM[m]
        fm = fm + f1d * t.DFIMOFR[m]
    si = np.zeros(n, T)
    ci = np.zeros(n, T)
    for k in range(K):
        temp = spec[:, k, 0] * t.DFIM[0]
        for m in range(1, M):
            temp = temp + spec[:, k, m] * t.DFIM[m]
        si = si + t.SINTH[k] * temp
        ci = ci + t.COSTH[k] * temp
        ci = np.where(ci == 0, eps, ci).astype(T)
    thq = np.arctan2(si, ci).astype(T)
    thq = np.where(thq < 0, thq + t.ZPI, thq).astype(T)
    ok = em > eps
    with np.errstate(divide="ignore", invalid="ignore"):
        per = np.where(ok, fm / em, T(0.0)).astype(T)
    return np.where(ok, em, T(0.0)).astype(T), np.where(ok, thq, T(0.0)).astype(T), per


def smooth(t, flsw):
    """SEP3TR's directional smoothing 0.1 (left + right) + 0.8 centre, 0 where FLSW <= 0 (the wind-sea mask imposed again)."""
    T = t.dtype
    sm = T(0.10) * (np.roll(flsw, 1, axis=1) + np.roll(flsw, -1, axis=1)) + T(0.80) * flsw
    return np.where(flsw <= 0, T(0.0), sm).astype(T)


def find_peaks(t, fl, mij, flnoise):
    """The local maxima of SEP3TR over M = 2 .. MIJ-1 (1-based), M-major then K, the first NPMAX kept.  Returns (npeak, kp, mp) with
    kp / mp [n][NPMAX] 0-based, and the count before the cap."""
    n, K, M = fl.shape
    lowest = np.maximum(t.FLMIN, flnoise)[:, None, None]
    up = lambda a: np.concatenate([a[:, :, 1:], np.zeros_like(a[:, :, :1])], 2)      # value at M + 1
    dn = lambda a: np.concatenate([np.zeros_like(a[:, :, :1]), a[:, :, :-1]], 2)     # value at M - 1
    nb = []
    for dk in (-1, 0, 1):
        r = np.roll(fl, -dk, axis=1)                                                    # value at K + dk
        for v in ((dn(r), up(r)) if dk == 0 else (dn(r), r, up(r))):
            nb.append(v)
    pk = fl > lowest
    for v in nb:
        pk &= (v > 0) & (fl >= v)
    m1 = np.arange(M)[None, None, :] + 1
    pk &= (m1 >= 2) & (m1 <= np.asarray(mij)[:, None, None] - 1)
    flat = pk.transpose(0, 2, 1).reshape(n, -1)                                         # M-major, then K
    total = flat.sum(1)
    keep = flat & (np.cumsum(flat, 1) <= NPMAX)
    npeak = np.minimum(total, NPMAX)
    kp = np.zeros((n, NPMAX), np.int64)
    mp = np.zeros((n, NPMAX), np.int64)
    rows, cols = np.nonzero(keep)
    slot = np.cumsum(keep, 1)[rows, cols] - 1
    mp[rows, slot], kp[rows, slot] = cols // K, cols % K
    return npeak, kp, mp, total


def _nbr_any(a, valid_m=True):
    """OR over the 8 neighbours (K +-1 cyclic, M +-1 where it exists) of a boolean [n][K][M]."""
    z = np.zeros_like(a[:, :, :1])
    out = np.zeros_like(a)
    for dk in (-1, 0, 1):
        r = np.roll(a, -dk, axis=1)
        if dk:
            out |= r
        out |= np.concatenate([r[:, :, 1:], z], 2) | np.concatenate([z, r[:, :, :-1]], 2)
    return out


def _sweep_vectorised(fl, w1, w2, w3, sec, mb, mc):
    """One sweep (2.b then 2.c) of every point at once.  w1, w2 in half units.  Returns the per-point change flag."""
    K = fl.shape[1]
    z = np.zeros_like(fl[:, :, :1])
    zb = np.zeros_like(w3[:, :, :1])
    zero2 = w2 == 0
    block = np.zeros_like(w3)
    for dk in (-1, 0, 1):
        f = np.roll(fl, -dk, axis=1)
        q = np.roll(zero2, -dk, axis=1)
        cands = [(np.concatenate([f[:, :, 1:], z], 2), np.concatenate([q[:, :, 1:], zb], 2)),
                 (np.concatenate([z, f[:, :, :-1]], 2), np.concatenate([zb, q[:, :, :-1]], 2))]
        if dk:
            cands.append((f, q))
        for fv, qv in cands:                                      # a missing neighbour has q = False
            block |= qv & (fv > fl)
    addb = w3 & sec & mb & (w2 == 1) & (w1 == 0) & ~block
    w2[addb] = 2
    addc = w3 & (w1 < 2) & sec & mc & (w2 == 0) & _nbr_any(w2 == 2)
    w2[addc] = 1
    return (addb | addc).reshape(len(fl), -1).any(1)


def _sweep_literal(fl, w1, w2, w3, i, kloc, mmin, mmax, mij):
    """One sweep of point i in the reference's order, bin by bin (fndprt.F90 2.b and 2.c).  Returns the change flag."""
    K, M = fl.shape[1:]
    f, a, b, l3 = fl[i], w1[i], w2[i], w3[i]
    change = False
    for m in range(mmin, min(mij - 1, mmax) + 1):
        for k in kloc:
            if l3[k, m] and b[k, m] == 1 and a[k, m] == 0:
                add = True
                for kr in (k - 1, k, k + 1):
                    kl = kr % K
                    for ml in range(max(0, m - 1), min(M - 1, m + 1) + 1):
                        if b[kl, ml] == 0 and f[kl, ml] > f[k, m]:
                            add = False
                            break
                    if not add:
                        break
                if add:
                    b[k, m] = 2
                    change = True
    for m in range(mmin, mmax + 1):
        for k in kloc:
            if l3[k, m] and a[k, m] < 2 and b[k, m] == 0:
                hit = False
                for kr in (k - 1, k, k + 1):
                    kl = kr % K
                    for ml in range(max(0, m - 1), min(M - 1, m + 1) + 1):
                        if b[kl, ml] == 2:
                            hit = True
                            break
                    if hit:
                        break
                if hit:
                    b[k, m] = 1
                    change = True
    return change


def fndprt(t, fl, npeak, kp, mp, mij, llcosdiff, flnoise, literal=False):
    """FNDPRT on the smoothed spectrum fl [n][K][M].  Returns dict(npeak (with the extra partition), ene/dir/per [n][NPMAX + 1] (1-based
    like the reference), fac = MAX(W1, 1) outside COSWDIF < -0.4 and 1 inside, assigned (SUNASGN = 0 there), sweeps [n][NPMAX] (0 where
    no peak), w1 (half units))."""
    T = t.dtype
    n, K, M = fl.shape
    nh = nangh(t)
    w3 = fl > t.FLMIN
    w1 = np.where(w3, 0, 2).astype(np.int8)                       # half units
    anym = w3.any(1)
    mmin = np.where(anym.any(1), np.argmax(anym, 1), M - 1)
    mmax = np.where(anym.any(1), M - 1 - np.argmax(anym[:, ::-1], 1), -1)
    mij = np.asarray(mij, np.int64)
    ene = np.zeros((n, NPMAX + 1), T)
    dir_ = np.zeros((n, NPMAX + 1), T)
    per = np.zeros((n, NPMAX + 1), T)
    sweeps = np.zeros((n, NPMAX), np.int64)
    asg = np.zeros((n, K, M), bool)
    kk = np.arange(K)[None, :]
    mm = np.arange(M)[None, None, :]
    rows = np.arange(n)
    npeak = np.asarray(npeak).copy()
    for ip in range(NPMAX):
        act = npeak > ip
        if not act.any():
            break
        kc, mc = kp[:, ip], mp[:, ip]
        d = (kk - kc[:, None]) % K
        sec = (d <= nh) | (d >= K - nh)                           # KLOC(ITHC-NANGH .. ITHC+NANGH)
        w2 = np.zeros((n, K, M), np.int8)
        for dk in (-1, 0, 1):
            kl = (kc + dk) % K
            for dm in (-1, 0, 1):
                ml = np.clip(mc + dm, 0, M - 1)
                s = act & (w1[rows, kl, ml] <= 1)
                w2[rows[s], kl[s], ml[s]] = 1
        s = act & (w1[rows, kc, mc] == 0)
        w2[rows[s], kc[s], mc[s]] = 2
        # MMAX: the highest M in MMIN .. MMAX with a bin of the sector at W1 < 1
        hasl = ((w1 < 2) & sec[:, :, None]).any(1) & (mm[0] >= mmin[:, None]) & (mm[0] <= mmax[:, None])
        up = hasl.any(1)
        newmax = M - 1 - np.argmax(hasl[:, ::-1], 1)
        mmax = np.where(act & up, newmax, mmax)
        mb = (mm >= mmin[:, None, None]) & (mm <= np.minimum(mij - 1, mmax)[:, None, None])
        mcr = (mm >= mmin[:, None, None]) & (mm <= mmax[:, None, None])
        live = act.copy()
        nitt = 0
        while live.any():
            nitt += 1
            sweeps[live, ip] = nitt
            if literal:
                ch = np.zeros(n, bool)
                for i in np.nonzero(live)[0]:
                    kloc = [(int(kc[i]) + j) % K for j in range(-nh, nh + 1)]
                    ch[i] = _sweep_literal(fl, w1, w2, w3, i, kloc, int(mmin[i]), int(mmax[i]), int(mij[i]))
            else:
                w2l = np.where(live[:, None, None], w2, 0).astype(np.int8)
                ch = _sweep_vectorised(fl, w1, w2l, w3, sec[:, :, None] & live[:, None, None], mb, mcr)
                w2 = np.where(live[:, None, None], w2l, w2)
            live &= ch
            if nitt >= 25:
                break
        w2 = np.where(act[:, None, None], w2, 0).astype(np.int8)
        w1 = (w1 + w2).astype(np.int8)
        spec = (fl * (w2.astype(T) * T(0.5))).astype(T)
        e, th, p = parmean(t, spec)
        ene[act, ip + 1], dir_[act, ip + 1], per[act, ip + 1] = e[act], th[act], p[act]
        asg |= spec > 0
    # the extra partition in the wind sector against the wind
    w2 = np.where((npeak < NPMAX)[:, None, None] & llcosdiff[:, :, None] & (w1 == 0) & (fl > flnoise[:, None, None]), 2, 0).astype(np.int8)
    add = (w2 > 0).reshape(n, -1).any(1)
    w1 = np.where(w2 > 0, 2, w1).astype(np.int8)
    if add.any():
        spec = (fl * (w2.astype(T) * T(0.5))).astype(T)
        e, th, p = parmean(t, spec)
        slot = npeak[add] + 1
        ene[add, slot], dir_[add, slot], per[add, slot] = e[add], th[add], p[add]
        npeak = npeak + add
        asg |= spec > 0
    fac = np.where(llcosdiff[:, :, None], T(1.0), np.maximum(w1.astype(T) * T(0.5), T(1.0))).astype(T)
    return dict(npeak=npeak, ene=ene, dir=dir_, per=per, fac=fac, assigned=asg, sweeps=sweeps, w1=w1)


def sep3tr(t, fl1, mij, wdwave, cw, esw, fsw, thsw, fsea, swm, literal=False):
    """SEP3TR: returns (EMTRAIN, THTRAIN, PMTRAIN [n][3], the new SWM, info)."""
    T = t.dtype
    n, K, M = fl1.shape
    eps = t.EPSMIN
    mij = np.asarray(mij, np.int64)
    frinvmij = np.trunc(T(1.0) / t.FR[mij - 1]).astype(np.int64)            # INTEGER FRINVMIJ
    flsw = (np.maximum(fl1, eps) * swm).astype(T)
    fl = smooth(t, flsw)
    enmax = fl.reshape(n, -1).max(1)
    flnoise = (T(0.005) * enmax).astype(T)
    llcosdiff = cw < T(-0.4)
    npeak, kp, mp, total = find_peaks(t, fl, mij, flnoise)
    fp = fndprt(t, fl, npeak, kp, mp, mij, llcosdiff, flnoise, literal=literal)
    swm = (swm * fp["fac"]).astype(T)
    flsw = (np.maximum(fl1, eps) * swm).astype(T)
    ett = semean(t, flsw)
    npeak = fp["npeak"].copy()
    ene, dir_, per = fp["ene"].copy(), fp["dir"].copy(), fp["per"].copy()
    sumene = np.zeros(n, T)
    for ip in range(1, NPMAX + 1):
        sumene = np.where(ip <= npeak, sumene + ene[:, ip], sumene).astype(T)
    sun = np.where(fp["assigned"], T(0.0), fl).astype(T)
    _, fun = S._femean(t, sun)
    eun = semean(t, sun)
    thun = S._sthq(t, sun)
    # the points where one of SEP3TR's scalar decisions compares two sums within 64 ulp of each other: there the device, which adds in
    # another order, may decide the other way (the tests leave them out, as they leave out CHECKTA near 1)
    tol = 64 * np.finfo(T).eps
    close = lambda a, b: np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol * np.maximum(np.abs(a), np.abs(b))
    tie = close(eun, sumene) & (eun > 0)
    npkna = np.where(eun > sumene, NTRAIN, NTRAIN - 1)
    addu = (npeak < npkna) & (eun > 0)
    rows = np.nonzero(addu)[0]
    slot = npeak[rows] + 1
    ene[rows, slot], dir_[rows, slot] = eun[rows], thun[rows]
    per[rows, slot] = (T(1.0) / fun[rows]).astype(T)
    npeak = npeak + addu
    npk = npeak.copy()
    for ip in range(1, NPMAX + 1):
        hsmin = (T(0.05) + T(-0.0017) * per[:, ip]).astype(T)
        thrs = (T(0.0625) * (hsmin * hsmin)).astype(T)
        live = ip <= npeak
        tie |= live & (close(ene[:, ip], thrs) | close(per[:, ip], frinvmij.astype(T)))
        drop = live & ((ene[:, ip] < thrs) | (per[:, ip] < frinvmij))
        ene[drop, ip] = dir_[drop, ip] = per[drop, ip] = 0
        npk = npk - drop
    tie |= (npk <= 0) & close(fsw, fsea)
    fb = (npk <= 0) & (esw > 0) & (fsw < fsea)
    npeak = np.where(fb, 1, npeak)
    ene[fb, 1], dir_[fb, 1] = esw[fb], thsw[fb]
    per[fb, 1] = (T(1.0) / fsw[fb]).astype(T)
    em = np.zeros((n, NTRAIN), T)
    th = np.zeros((n, NTRAIN), T)
    pm = np.zeros((n, NTRAIN), T)
    ienergy = np.zeros((n, NTRAIN), np.int64)
    for s in range(NTRAIN):                                                    # the first energy sort
        ipnow = np.zeros(n, np.int64)
        emax = np.zeros(n, T)
        for ip in range(1, NPMAX + 1):
            up = ene[:, ip] > emax
            ipnow = np.where(up, ip, ipnow)
            emax = np.where(up, ene[:, ip], emax)
        em[:, s], th[:, s], pm[:, s] = ene[np.arange(n), ipnow], dir_[np.arange(n), ipnow], per[np.arange(n), ipnow]
        ene[np.arange(n), ipnow] = 0
        ienergy[:, s] = np.minimum(ipnow, 1)
    sumet = np.maximum(em[:, 0], eps)
    for s in range(1, NTRAIN):
        sumet = (sumet + em[:, s]).astype(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        enex = np.where(npeak >= npkna, np.maximum(ett - sumet, T(0.0)) / sumet, T(0.0)).astype(T)
    em = (em + enex[:, None] * em).astype(T)
    te, td, tp = em.copy(), th.copy(), pm.copy()
    for s in range(NTRAIN):                                                    # the second sort
        ipnow = np.full(n, -1, np.int64)
        emax = np.zeros(n, T)
        for ip in range(NTRAIN):
            up = te[:, ip] > emax
            ipnow = np.where(up, ip, ipnow)
            emax = np.where(up, te[:, ip], emax)
        ipl = np.maximum(ipnow, 0)
        r = np.arange(n)
        em[:, s], th[:, s], pm[:, s] = te[r, ipl], td[r, ipl], tp[r, ipl]
        te[r, ipl] = 0
    z = ienergy == 0
    em = np.where(z, T(0.0), em).astype(T)
    th = np.where(z, np.asarray(wdwave, T)[:, None], th).astype(T)
    pm = np.where(z, T(0.0), pm).astype(T)
    info = dict(tie=tie, npeak_found=total, npeak_fndprt=fp["npeak"], npeak=npeak, npkna=npkna, ett=ett, sweeps=fp["sweeps"], w1=fp["w1"],
                assigned=fp["assigned"], fl=fl, nz=(em > 0).sum(1))
    return em, th, pm, swm, info


def partition(t, fl1, xllws, mij, cinv, ufric, wdwave, zmiss: float = -999.0, literal=False):
    """Returns (out [n][24] in the columns FIELDS, info).  info["near"]: the points where a CHECKTA of the masks lies within 4 ulp of 1
    (as in sepwisw_ref); info["tie"]: the points where a scalar decision of SEP3TR is a near tie; info["swm"]: the mask after SEP3TR."""
    T = t.dtype
    fl1 = np.asarray(fl1, T)
    xllws = np.asarray(xllws, T)
    cinv = np.asarray(cinv, T)
    ufric = np.asarray(ufric, T)
    wdwave = np.asarray(wdwave, T)
    n, K, M = fl1.shape
    one = T(1.0)
    _, sinfo = S.sepwisw(t, fl1, xllws, cinv, ufric, wdwave, zmiss=zmiss)    # the mask after the walk
    swm = sinfo["swm"]
    cw = S.coswdif(t, wdwave)
    coef = T(1.2) * t.FRIC
    chk = (ufric[:, None] * cinv)[:, None, :] * (coef * cw)[:, :, None]
    swm1 = np.where(xllws != 0, T(0.0), np.where(chk >= one, T(0.0), one)).astype(T)
    f1 = fl1 * swm1
    _, fsea = S._femean(t, np.maximum(fl1 - f1, T(0.0)))                      # FSEA of sepwisw.F90:184
    f1 = (np.maximum(fl1, t.EPSMIN) * swm).astype(T)
    esw, fsw = S._femean(t, f1)
    thsw = S._sthq(t, f1)
    em, th, pm, swm, info = sep3tr(t, fl1, mij, wdwave, cw, esw, fsw, thsw, fsea, swm, literal=literal)
    # SEPWISW 2.2 and 3 on the rewritten swell spectrum
    f1 = (np.maximum(fl1, t.EPSMIN) * swm).astype(T)
    esw, fsw = S._femean(t, f1)
    thsw = S._sthq(t, f1)
    p1sw, p2sw = S._mwp(t, f1, False), S._mwp(t, f1, True)
    spsw = S._wdirspread(t, f1, esw, True)
    c4 = (cw * cw) * (cw * cw)
    floor = (cw[:, :, None] > T(0.8)) & (np.arange(M)[None, None, :] + 1 >= M // 2)
    d = fl1 - f1
    d = np.where(floor, d + t.EPSMIN * c4[:, :, None], d)
    f2 = np.maximum(d, T(0.0)).astype(T)
    ese, fse = S._femean(t, f2)
    thse = np.where(ese <= T(1.0e-9), wdwave, S._sthq(t, f2))
    p1se, p2se = S._mwp(t, f2, False), S._mwp(t, f2, True)
    spse = S._wdirspread(t, f2, ese, True)
    emt, _ = S._femean(t, fl1)
    p1, p2 = S._mwp(t, fl1, False), S._mwp(t, fl1, True)
    wdw = S._wdirspread(t, fl1, emt, False)
    deg = T(DEG)
    zm = T(zmiss)
    with np.errstate(divide="ignore"):
        cols = [p1, p2, wdw, T(4.0) * np.sqrt(np.maximum(ese, T(0.0))), T(4.0) * np.sqrt(np.maximum(esw, T(0.0))),
                np.fmod(deg * thse + T(180.0), T(360.0)), np.fmod(deg * thsw + T(180.0), T(360.0)),
                np.where(fse > 0, one / fse, zm), np.where(fsw > 0, one / fsw, zm), p1se, p1sw, p2se, p2sw, spse, spsw]
    for s in range(NTRAIN):
        cols += [T(4.0) * np.sqrt(np.maximum(em[:, s], T(0.0))), np.fmod(deg * th[:, s] + T(180.0), T(360.0)), pm[:, s]]
    out = np.stack([np.asarray(c, T) for c in cols], 1)
    info.update(near=sinfo["near"], swm=swm, emtrain=em, thtrain=th, pmtrain=pm)
    return out, info
