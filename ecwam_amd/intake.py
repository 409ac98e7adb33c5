"""The host's share of the forcing intake (include/ecwam_hip_intake.h): INITIALINT's once-per-run tables in the working precision and the
per-point table ecwam_hip_set_fldinter takes.  Both restate the reference's statements (initialint.F90:122-174, fldinter.F90:181-186 and
227-247) in its order of operations; tests/test_intake_host.py holds them against the reference's own tables.

Arrays are indexed as the Fortran ones, shifted to 0: a table T(NWX,NWY) is t[i - 1, j - 1], IJBLOCK(0:NC+1,NR) is ijblock[i, j - 1]; the
values of the integer tables and of IJBLOCK, IFROMIJ, JFROMIJ stay 1-based as the reference holds them.
"""
from __future__ import annotations

import numpy as np


def initialint(iu06, nca, nra, ngx, ngy, krgg, klonrgg, xdella, zdello, amowep, amosop, amoeap, amonop, ncad, nrad, rmonop, rmosop, rmowep, rmoeap,
               ilonrgg, iperiodic, nwx, nwy, dtype=np.float64):
    """INITIALINT (initialint.F90:122-174) with its arguments, in the precision `dtype`: (DJ1 [nwy], DII1, DIIP1 [nwx][nwy], JJ [nwy], II, IIP
    [nwx][nwy]).  Entries the routine does not set (I > KLONRGG) are 0.  iu06, nca, nra, ngx, krgg, amoeap and amonop are not used, as in the
    reference."""
    T = np.dtype(dtype).type
    klonrgg, ilonrgg = np.asarray(klonrgg, np.int64), np.asarray(ilonrgg, np.int64)
    zdello = np.asarray(zdello, T)
    xdella, amowep, amosop, rmonop, rmosop, rmowep, rmoeap = (T(v) for v in (xdella, amowep, amosop, rmonop, rmosop, rmowep, rmoeap))
    della = T((rmonop - rmosop) / T(max(1, nrad - 1)))
    if iperiodic == 1:
        rdello = (T(360.0) / np.maximum(1, ilonrgg[:nrad]).astype(T)).astype(T)
    else:
        rdello = (T(rmoeap - rmowep) / np.maximum(1, ilonrgg[:nrad] - 1).astype(T)).astype(T)
    dj1 = np.zeros(nwy, T)
    dii1, diip1 = np.zeros((nwx, nwy), T), np.zeros((nwx, nwy), T)
    jj = np.zeros(nwy, np.int32)
    ii, iip = np.zeros((nwx, nwy), np.int32), np.zeros((nwx, nwy), np.int32)
    for k in range(1, ngy + 1):
        jsn = ngy - k + 1
        xlat = T(amosop + T(T(jsn - 1) * xdella))
        xlat = min(max(xlat, rmosop), rmonop)
        xk = T(rmonop - xlat)
        xk = T(T(xk / della) + T(1.0))
        jj[k - 1] = max(1, int(xk))
        ksn = nrad - jj[k - 1] + 1
        jj1 = min(jj[k - 1] + 1, nrad)
        ksn1 = nrad - jj1 + 1
        dj1[k - 1] = xk - T(jj[k - 1])
        n = int(klonrgg[jsn - 1])
        i = np.arange(n)
        xi = ((amowep + (i.astype(T) * zdello[jsn - 1]).astype(T)).astype(T) - rmowep).astype(T)
        xi = np.fmod((xi + T(720.0)).astype(T), T(360.0)).astype(T)
        for r, itab, dtab in ((rdello[ksn - 1], ii, dii1), (rdello[ksn1 - 1], iip, diip1)):
            x = ((xi / r).astype(T) + T(1.0)).astype(T)
            row = ksn if itab is ii else ksn1
            itab[:n, k - 1] = np.minimum(np.maximum(1 - iperiodic, x.astype(np.int64)), ilonrgg[row - 1])
            dtab[:n, k - 1] = x - itab[:n, k - 1].astype(T)
    return dj1, dii1, diip1, jj, ii, iip


def point_table(ifromij, jfromij, ijblock, ilonrgg, nr, iperiodic, jjm, iim, iipm, dj1m, dii1m, diip1m, interpol=True):
    """(idx int32 [npts][4], w float64 [npts][3]) for ecwam_hip_set_fldinter: per point the 0-based positions IJBLOCK(II,JJ), IJBLOCK(II1,JJ),
    IJBLOCK(IIP,JJ1), IJBLOCK(IIP1,JJ1) - 1 as fldinter.F90:227-247 forms them, and DJ1M(J), DII1M(I,J), DIIP1M(I,J) widened.  Without interpol
    (LLINTERPOL = F, fldinter.F90:181-186): idx[:, 0] = IJBLOCK(I,J) - 1, the other positions repeat it, and w is None."""
    i, j = np.asarray(ifromij, np.int64), np.asarray(jfromij, np.int64)
    ijblock, ilonrgg = np.asarray(ijblock, np.int64), np.asarray(ilonrgg, np.int64)
    if not interpol:
        p = ijblock[i, j - 1] - 1
        return np.ascontiguousarray(np.stack([p, p, p, p], 1), np.int32), None
    jjm, iim, iipm = np.asarray(jjm, np.int64), np.asarray(iim, np.int64), np.asarray(iipm, np.int64)
    jj = jjm[j - 1]
    jsn = nr - jj + 1
    jj1 = np.minimum(jj + 1, nr)
    jsn1 = nr - jj1 + 1
    ii = iim[i - 1, j - 1]
    ii1 = np.minimum(ii + 1, ilonrgg[jsn - 1] + iperiodic)
    iip = iipm[i - 1, j - 1]
    iip1 = np.minimum(iip + 1, ilonrgg[jsn1 - 1] + iperiodic)
    idx = np.stack([ijblock[ii, jj - 1], ijblock[ii1, jj - 1], ijblock[iip, jj1 - 1], ijblock[iip1, jj1 - 1]], 1) - 1
    w = np.stack([np.asarray(dj1m)[j - 1], np.asarray(dii1m)[i - 1, j - 1], np.asarray(diip1m)[i - 1, j - 1]], 1).astype(np.float64)
    return np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(w)
