"""numpy restatement of the first-order propagation scheme (IPROPAGS = 0), statement by statement in the working precision: PROPAGS with its four
sections (propags.F90:230-362, 370-498, 506-753, 761-996), CHECKCFL's inputs as the spherical sections pass them at M = 1 (propags.F90:718-722, 924-928) and
the dot terms of GRADI + PROPDOT (gradi.F90:113-232, propdot.F90:109-198).  TEST INFRASTRUCTURE: it serves the shapes the fixtures
tests/golden/propags_*.npz do not have, and tests/test_propags_host.py holds it to the fixtures bit for bit.

Indices are 0-based; rows [0, n) have tables, the land row is `nland`, the *_ext arrays cover every row up to it.  Every array is of the working
precision T and every constant is written as T(...), so that each operation rounds once, as the reference's does without contraction."""
import numpy as np

NCFL = 11      # DTC, CFLEA, CFLWE, CFLNO, CFLSO, CFLNO2, CFLSO2, CFLTP, CFLTM, CFLOP, CFLOM
CURRENT_GRADIENT_MAX = 0.00001      # yowcurr.F90:19


def dot_width(nang):
    return 3 * nang + 4


def dot_terms(T, irefra, icase, nland, kxlt, zdello, xdella, circ, cosph, klon, klat, wlat, cosphm1, depth, u, v, sinth, costh):
    """-> THDD [n][K], THDC [n][K], S0 [n][K] (SDOT(IJ,K,NFRE_RED) of propdot.F90:178), OMDD [n]"""
    n = klon.shape[0]
    nang = sinth.shape[0]
    Z = np.zeros(n, T)
    delphi = T(xdella) * T(circ) / T(360.0)
    oneo2delphi = T(0.5) / delphi
    dellam = (zdello.astype(T) * T(circ) / T(360.0))[kxlt]
    ddphi, ddlam, duphi, dulam, dvphi, dvlam = (Z.copy() for _ in range(6))
    w1, w2 = wlat[:, 0], wlat[:, 1]
    one = T(1)
    if irefra in (1, 3):
        ipp, ipm, ipp2, ipm2 = klat[:, 1, 0], klat[:, 0, 0], klat[:, 1, 1], klat[:, 0, 1]
        all4 = (ipp != nland) & (ipm != nland) & (ipp2 != nland) & (ipm2 != nland)
        first = ~all4 & (ipp != nland) & (ipm != nland)
        second = ~all4 & ~first & (ipp2 != nland) & (ipm2 != nland)
        dptp = w2 * depth[ipp] + (one - w2) * depth[ipp2]
        dptm = w1 * depth[ipm] + (one - w1) * depth[ipm2]
        ddphi = np.where(all4, (dptp - dptm) * oneo2delphi, ddphi)
        ddphi = np.where(first, (depth[ipp] - depth[ipm]) * oneo2delphi, ddphi)
        ddphi = np.where(second, (depth[ipp2] - depth[ipm2]) * oneo2delphi, ddphi)
        ilp, ilm = klon[:, 1], klon[:, 0]
        ddlam = np.where((ilp != nland) & (ilm != nland), (depth[ilp] - depth[ilm]) / (T(2) * dellam), ddlam)
    if irefra in (2, 3):
        def undefined(i):      # an exact zero: the current is not defined there (gradi.F90:170-180)
            return np.where((u[i] == 0) & (v[i] == 0), nland, i)
        ipp, ipm, ipp2, ipm2 = (undefined(klat[:, a, b]) for a, b in ((1, 0), (0, 0), (1, 1), (0, 1)))
        all4 = (ipp != nland) & (ipm != nland) & (ipp2 != nland) & (ipm2 != nland)
        first = ~all4 & (ipp != nland) & (ipm != nland)
        up = w2 * u[ipp] + (one - w2) * u[ipp2]
        vp = w2 * v[ipp] + (one - w2) * v[ipp2]
        um = w1 * u[ipm] + (one - w1) * u[ipm2]
        vm = w1 * v[ipm] + (one - w1) * v[ipm2]
        duphi = np.where(all4, (up - um) * oneo2delphi, np.where(first, (u[ipp] - u[ipm]) * oneo2delphi, Z))
        dvphi = np.where(all4, (vp - vm) * oneo2delphi, np.where(first, (v[ipp] - v[ipm]) * oneo2delphi, Z))
        ilp, ilm = undefined(klon[:, 1]), undefined(klon[:, 0])
        both = (ilp != nland) & (ilm != nland)
        dulam = np.where(both, (u[ilp] - u[ilm]) / (T(2) * dellam), Z)
        dvlam = np.where(both, (v[ilp] - v[ilm]) / (T(2) * dellam), Z)
        cgmax = T(CURRENT_GRADIENT_MAX) * cosph.astype(T)[kxlt]
        duphi, dvphi, dulam, dvlam = (np.copysign(np.minimum(np.abs(a), cgmax), a) for a in (duphi, dvphi, dulam, dvlam))
    dco = cosphm1[:n] if icase == 1 else np.ones(n, T)
    omdd = v[:n] * ddphi + u[:n] * ddlam * dco if irefra == 3 else Z.copy()
    thdd, thdc, s0 = (np.zeros((n, nang), T) for _ in range(3))
    for k in range(nang):
        sd, cd = sinth[k], costh[k]
        if irefra in (1, 3):
            thdd[:, k] = sd * ddphi - cd * ddlam * dco
        if irefra in (2, 3):
            ss, sc, cc = sd * sd, sd * cd, cd * cd
            s0[:, k] = -sc * duphi - cc * dvphi - (ss * dulam + sc * dvlam) * dco
            thdc[:, k] = ss * duphi + sc * dvphi - (sc * dulam + cc * dvlam) * dco
    return thdd.astype(T), thdc.astype(T), s0.astype(T), omdd.astype(T)


def dot_row(thdd, thdc, s0, omdd):
    """the row ecwam_hip_propags_dot writes: [n][3 NANG + 4]"""
    n, nang = thdd.shape
    row = np.zeros((n, dot_width(nang)), thdd.dtype)
    row[:, :nang], row[:, nang:2 * nang], row[:, 2 * nang:3 * nang], row[:, 3 * nang] = thdd, thdc, s0, omdd
    return row


def sdot(s0, omdd, cg, om, wn, nr):
    """SDOT [n][K][NFRE_RED], propdot.F90:190-191"""
    n = s0.shape[0]
    return (s0[:, :, None] * cg[:n, None, :nr] + (omdd[:, None] * om[:n, :nr])[:, None, :]) * wn[:n, None, :nr]


def propags(T, f1, *, irefra, icase, irgg, nland, nr, delpro, delphi, kxlt, cosph, sinph, dellam1, cosphm1, klon, klat, wlat, cg, om, wn, u, v, thdd, thdc, s0,
            omdd, obs, sinth, costh, fr, delth, r_earth, zpi, fratio, kijs=0, kijl=None, weights=None):
    """-> F3 [kijl - kijs][K][NFRE_RED], CFL [kijl - kijs][K][11] (zeros on a Cartesian grid).  obs: [n][8][NFRE] (OBSLAT(:,:,1:2), OBSLON(:,:,1:2) first) or None.
    weights: a dict that receives the upwind weights of the section per (K, M) (the coverage conditions of the fixtures read them)."""
    n = klon.shape[0]
    kijl = n if kijl is None else kijl
    A = np.arange(kijs, kijl)
    nang = sinth.shape[0]
    one = T(1)
    delpro, delphi, fratio = T(delpro), T(delphi), T(fratio)
    f3 = np.zeros((A.size, nang, nr), T)
    cfl = np.zeros((A.size, nang, NCFL), T)
    cur = irefra in (2, 3)
    lon1, lon2 = klon[A, 0], klon[A, 1]
    la11, la12, la21, la22 = klat[A, 0, 0], klat[A, 0, 1], klat[A, 1, 0], klat[A, 1, 1]
    della0_all = delpro * dellam1
    della0_all[nland] = T(0)
    delth0 = T(0.25) * delpro / T(delth)
    rec = weights if weights is not None else {}

    def note(name, k, m, val):
        if weights is not None:
            rec.setdefault(name, np.zeros((A.size, nang, nr), T))[:, k, m] = val

    if icase == 1:
        dco = cosphm1
        with np.errstate(divide="ignore", invalid="ignore"):      # the land slot of COSPHM1_EXT is 0; its quotient is not taken
            dp1 = np.where(la11 == nland, one, dco[A] / dco[la11]).astype(T)
            dp2 = np.where(la21 == nland, one, dco[A] / dco[la21]).astype(T)
        tanph = (sinph[kxlt[A]] / cosph[kxlt[A]]).astype(T)
        wl1, wl2 = wlat[A, 0], wlat[A, 1]
        wm1, wm2 = one - wl1, one - wl2
    ob = None if obs is None else obs[A]
    if not cur:
        if icase != 1:
            # ---- section 1
            delph0 = delpro / delphi
            della0 = della0_all[A]
            for k in range(nang):
                kp1, km1 = (k + 1) % nang, (k - 1) % nang
                sd, cd = sinth[k], costh[k]
                ila = lon2 if sd < 0 else lon1
                iph = la21 if cd < 0 else la11
                sd, cd = T(0.5) * sd, T(0.5) * cd
                if irefra == 1:
                    drdp = (thdd[A, k] + thdd[A, kp1]) * delth0
                    drdm = (thdd[A, k] + thdd[A, km1]) * delth0
                for m in range(nr):
                    c0 = cg[A, m]
                    sdd = sd * della0
                    if sd >= 0:
                        dla = sdd * (cg[lon1, m] + c0)
                        dtc = sdd * (cg[lon2, m] + c0)
                    else:
                        dla = -sdd * (cg[lon2, m] + c0)
                        dtc = -sdd * (cg[lon1, m] + c0)
                    cdd = cd * delph0
                    if cd >= 0:
                        dph = cdd * (cg[la11, m] + c0)
                        dtc = dtc + cdd * (cg[la21, m] + c0)
                    else:
                        dph = -cdd * (cg[la21, m] + c0)
                        dtc = dtc - cdd * (cg[la11, m] + c0)
                    if irefra == 1:
                        dthp = om[A, m] * drdp
                        dthm = om[A, m] * drdm
                        dtc = dtc + dthp + np.abs(dthp) - dthm + np.abs(dthm)
                        dtp = -dthp + np.abs(dthp)
                        dtm = dthm + np.abs(dthm)
                        note("DTP", k, m, dtp)
                        note("DTM", k, m, dtm)
                    r = (one - dtc) * f1[A, k, m] + dph * f1[iph, k, m] + dla * f1[ila, k, m]
                    if irefra == 1:
                        r = r + dtp * f1[A, kp1, m] + dtm * f1[A, km1, m]
                    f3[:, k, m] = r
            return f3, cfl
        # ---- section 3
        delph0 = T(0.5) * delpro / delphi
        cgklon = [cg[lon1, :nr] + cg[A, :nr], cg[lon2, :nr] + cg[A, :nr]]
        cgklat = [cg[A, :nr] + dp1[:, None] * (wl1[:, None] * cg[la11, :nr] + wm1[:, None] * cg[la12, :nr]),
                  cg[A, :nr] + dp2[:, None] * (wl2[:, None] * cg[la21, :nr] + wm2[:, None] * cg[la22, :nr])]
        obslon = [cgklon[i] if ob is None else ob[:, 2 + i, :nr] * cgklon[i] for i in range(2)]
        obslat = [cgklat[i] if ob is None else ob[:, i, :nr] * cgklat[i] for i in range(2)]
        dladco = dco[A] * della0_all[A]
        for k in range(nang):
            kp1, km1 = (k + 1) % nang, (k - 1) % nang
            sd, cd = sinth[k], costh[k]
            sda2 = T(0.5) * np.abs(sd)
            delph0_cda = delph0 * np.abs(cd)
            sp = delth0 * (sinth[k] + sinth[kp1]) / T(r_earth)
            sm = delth0 * (sinth[k] + sinth[km1]) / T(r_earth)
            drgp, drgm = tanph * sp, tanph * sm
            ila = lon2 if sd < 0 else lon1
            iph1, iph2 = (la21, la22) if cd < 0 else (la11, la12)
            if irefra == 1:
                drdp = (thdd[A, k] + thdd[A, kp1]) * delth0
                drdm = (thdd[A, k] + thdd[A, km1]) * delth0
            for m in range(nr):
                xx = sda2 * dladco
                if sd > 0:
                    cflea = xx * cgklon[1][:, m]
                    dle = xx * obslon[0][:, m]
                else:
                    cflea = xx * cgklon[0][:, m]
                    dle = xx * obslon[1][:, m]
                dtc = cflea
                if cd > 0:
                    cflno = delph0_cda * cgklat[1][:, m]
                    dtc = dtc + cflno
                    xx = delph0_cda * obslat[0][:, m]
                    dpn, dpn2 = wl1 * xx, wm1 * xx
                else:
                    cflno = delph0_cda * cgklat[0][:, m]
                    dtc = dtc + cflno
                    xx = delph0_cda * obslat[1][:, m]
                    dpn, dpn2 = wl2 * xx, wm2 * xx
                if irefra == 0:
                    dthp = drgp * cg[A, m]
                    dthm = drgm * cg[A, m]
                else:
                    dthp = drgp * cg[A, m] + om[A, m] * drdp
                    dthm = drgm * cg[A, m] + om[A, m] * drdm
                cfltp = dthp + np.abs(dthp)
                cfltm = -dthm + np.abs(dthm)
                dtc = dtc + cfltp + cfltm
                dtp = -dthp + np.abs(dthp)
                dtm = dthm + np.abs(dthm)
                note("DTP", k, m, dtp)
                note("DTM", k, m, dtm)
                f3[:, k, m] = ((one - dtc) * f1[A, k, m] + dpn * f1[iph1, k, m] + dpn2 * f1[iph2, k, m] + dle * f1[ila, k, m] + dtp * f1[A, kp1, m]
                               + dtm * f1[A, km1, m])
                if m == 0:
                    for i, a in enumerate((dtc, cflea, cflea, cflno, cflno, cflno, cflno, cfltp, cfltm, cfltp, cfltm)):
                        cfl[:, k, i] = a
        return f3, cfl
    # ---- sections 2 and 4
    delph0 = T(0.25) * delpro / delphi
    della0_all = T(0.25) * della0_all
    delfr0 = T(0.25) * delpro / ((fratio - one) * T(zpi))
    sd_all = sdot(s0, omdd, cg, om, wn, nr)
    nrow = cg.shape[0]
    for k in range(nang):
        kp1, km1 = (k + 1) % nang, (k - 1) % nang
        sd, cd = sinth[k], costh[k]
        if icase == 1:
            sp = delth0 * (sinth[k] + sinth[kp1]) / T(r_earth)
            sm = delth0 * (sinth[k] + sinth[km1]) / T(r_earth)
            drgp, drgm = tanph * sp, tanph * sm
        drdp = (thdd[A, k] + thdd[A, kp1]) * delth0
        drdm = (thdd[A, k] + thdd[A, km1]) * delth0
        drcp = (thdc[A, k] + thdc[A, kp1]) * delth0
        drcm = (thdc[A, k] + thdc[A, km1]) * delth0
        for m in range(nr):
            mp1, mm1 = min(nr - 1, m + 1), max(0, m - 1)
            dfp = delfr0 / fr[m]
            dfm = delfr0 / fr[mm1]
            dla, dph = np.zeros(nrow, T), np.zeros(nrow, T)
            sea = np.arange(nrow) != nland
            if icase == 1:
                dla[sea] = u[sea] + sd * cg[sea, m]
                dla[nland] = sd * cg[nland, m]
            else:
                dla[sea] = (u[sea] + sd * cg[sea, m]) * della0_all[sea]
                dla[nland] = sd * cg[nland, m] * della0_all[0]
            dph[sea] = (v[sea] + cd * cg[sea, m]) * delph0
            dph[nland] = cd * cg[nland, m] * delph0
            if icase == 1:
                dlwe = (dla[A] + dla[lon1]) * della0_all[A] * dco[A]
                dlea = (dla[A] + dla[lon2]) * della0_all[A] * dco[A]
                o_lon1, o_lon2, o_lat1, o_lat2 = (one,) * 4 if ob is None else (ob[:, 2, m], ob[:, 3, m], ob[:, 0, m], ob[:, 1, m])
                dle = (-dlea + np.abs(dlea)) * o_lon2
                dlw = (dlwe + np.abs(dlwe)) * o_lon1
                cflea = dlea + np.abs(dlea)
                cflwe = -dlwe + np.abs(dlwe)
                dtc = cflea + cflwe
                if irgg == 1:
                    dpno = (dph[A] + dph[la21] * dp2) * wl2
                    dpn = (-dpno + np.abs(dpno)) * o_lat2
                    dpno2 = (dph[A] + dph[la22] * dp2) * wm2
                    dpn2 = (-dpno2 + np.abs(dpno2)) * o_lat2
                    dpso = (dph[A] + dph[la11] * dp1) * wl1
                    dps = (dpso + np.abs(dpso)) * o_lat1
                    dpso2 = (dph[A] + dph[la12] * dp1) * wm1
                    dps2 = (dpso2 + np.abs(dpso2)) * o_lat1
                    cflno = dpno + np.abs(dpno)
                    cflso = -dpso + np.abs(dpso)
                    cflno2 = dpno2 + np.abs(dpno2)
                    cflso2 = -dpso2 + np.abs(dpso2)
                    dtc = dtc + cflno + cflso + cflno2 + cflso2
                else:
                    dpno = dph[A] + dph[la21] * dp2
                    dpn = (-dpno + np.abs(dpno)) * o_lat2
                    dpso = dph[A] + dph[la11] * dp1
                    dps = (dpso + np.abs(dpso)) * o_lat1
                    cflno = dpno + np.abs(dpno)
                    cflso = -dpso + np.abs(dpso)
                    cflno2 = cflso2 = np.zeros(A.size, T)
                    dpn2 = dps2 = np.zeros(A.size, T)
                    dtc = dtc + cflno + cflso
                dthp = drgp * cg[A, m] + om[A, m] * drdp + drcp
                dthm = drgm * cg[A, m] + om[A, m] * drdm + drcm
                cfltp = dthp + np.abs(dthp)
                cfltm = -dthm + np.abs(dthm)
                dtc = dtc + cfltp + cfltm
            else:
                dlwe = dla[A] + dla[lon1]
                dlea = dla[A] + dla[lon2]
                dle = -dlea + np.abs(dlea)
                dlw = dlwe + np.abs(dlwe)
                dtc = dlea + np.abs(dlea) - dlwe + np.abs(dlwe)
                dpso = dph[A] + dph[la11]
                dpno = dph[A] + dph[la21]
                dpn = -dpno + np.abs(dpno)
                dps = dpso + np.abs(dpso)
                dtc = dtc + dpno + np.abs(dpno) - dpso + np.abs(dpso)
                dthp = om[A, m] * drdp + drcp
                dthm = om[A, m] * drdm + drcm
                dtc = dtc + dthp + np.abs(dthp) - dthm + np.abs(dthm)
            dtp = -dthp + np.abs(dthp)
            dtm = dthm + np.abs(dthm)
            dthp = (sd_all[A, k, m] + sd_all[A, k, mp1]) * dfp
            dthm = (sd_all[A, k, m] + sd_all[A, k, mm1]) * dfm
            if icase == 1:
                cflop = dthp + np.abs(dthp)
                cflom = -dthm + np.abs(dthm)
                dtc = dtc + cflop + cflom
            else:
                dtc = dtc + dthp + np.abs(dthp) - dthm + np.abs(dthm)
            dop = (-dthp + np.abs(dthp)) / fratio
            dom = (dthm + np.abs(dthm)) * fratio
            for name, val in (("DTP", dtp), ("DTM", dtm), ("DLE", dle), ("DLW", dlw), ("DPN", dpn), ("DPS", dps), ("DOP", dop), ("DOM", dom)):
                note(name, k, m, val)
            r = (one - dtc) * f1[A, k, m] + dpn * f1[la21, k, m]
            if icase == 1 and irgg == 1:
                note("DPN2", k, m, dpn2)
                note("DPS2", k, m, dps2)
                r = r + dpn2 * f1[la22, k, m] + dps * f1[la11, k, m] + dps2 * f1[la12, k, m]
            else:
                r = r + dps * f1[la11, k, m]
            r = (r + dle * f1[lon2, k, m] + dlw * f1[lon1, k, m] + dtp * f1[A, kp1, m] + dtm * f1[A, km1, m] + dop * f1[A, k, mp1]
                 + dom * f1[A, k, mm1])
            f3[:, k, m] = r
            if m == 0 and icase == 1:
                for i, a in enumerate((dtc, cflea, cflwe, cflno, cflso, cflno2, cflso2, cfltp, cfltm, cflop, cflom)):
                    cfl[:, k, i] = a
    return f3, cfl


# ---- the recorded cases (tools/make_golden_propags.py writes tests/golden/propags_<case>.npz; the tests rebuild the inputs) ------------------------------
import os      # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NANG, NFRE, NFRE_RED = 12, 36, 25
DELPRO, DELPRO_CFL0, DELPRO_CFL3 = 900, 40000, 24000      # IDELPRO of the cases, and the time steps too long for the grid (IREFRA 0, 3)
# name -> ICASE, IRGG, IREFRA, obstructions, IDELPRO
CASES = {
    "sph_irgg1_irefra0": (1, 1, 0, False, DELPRO), "sph_irgg1_irefra1": (1, 1, 1, False, DELPRO), "sph_irgg1_irefra2": (1, 1, 2, False, DELPRO),
    "sph_irgg1_irefra3": (1, 1, 3, False, DELPRO), "sph_irgg0_irefra3": (1, 0, 3, False, DELPRO),
    "sph_obs_irefra0": (1, 1, 0, True, DELPRO), "sph_obs_irefra3": (1, 1, 3, True, DELPRO),
    "cart_irefra0": (2, 1, 0, False, DELPRO), "cart_irefra1": (2, 1, 1, False, DELPRO), "cart_irefra3": (2, 1, 3, False, DELPRO),
    "cfl_irefra0": (1, 1, 0, False, DELPRO_CFL0), "cfl_irefra3": (1, 1, 3, False, DELPRO_CFL3),
}
# the case of the same inputs without obstructions
UNOBSTRUCTED = {"sph_obs_irefra0": "sph_irgg1_irefra0", "sph_obs_irefra3": "sph_irgg1_irefra3"}


def fixture_grid():
    from ecwam_amd import grid

    return grid.build_grid(3, "continents", seed=24, land_fraction=0.4)


def _f32(a):
    """rounded to single precision: both precisions of the reference and of the device see the same numbers"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def tables_of(T, nang=NANG, nfre=NFRE, nfre_red=NFRE_RED, irefra=0):
    from ecwam_amd.tables import Config, Tables

    return Tables(Config(nang=nang, nfre=nfre, nfre_red=nfre_red, irefra=irefra), T)


def make_inputs(T, g, t, icase, irgg, irefra, with_obs, idelpro, seed=7, depth_lo=4.0, cur_amp=1.5, obscor=False):
    """The arguments of dot_terms and propags for grid g and tables t, in the working precision T.  Every field is rounded to single precision first; what
    the reference derives (DELPHI, DELLAM, 1 / DELLAM, 1 / COSPH) is derived here in T, as readmdlconf.F90:136, 145 and mpdecomp.F90:1428-1429 do.
    depth_lo: the shallowest depth drawn; cur_amp: the largest current component; obscor: the planes OBSCOR(1:4) of `obs` are drawn too (they are 1 otherwise:
    the first-order scheme has no corner points).  The defaults are the inputs of the recorded propags_* cases."""
    from ecwam_amd import synthetic as syn

    rng = np.random.default_rng(seed)
    n, nland, nrow = g.nsea, g.nland, g.nsea + 1
    nang, nfre, nr = t.cfg.nang, t.cfg.nfre, t.cfg.nfre_red
    depth = _f32(np.where(rng.uniform(size=nrow) < 0.5, rng.uniform(depth_lo, 40.0, nrow), rng.uniform(40.0, 400.0, nrow)))
    depth[nland] = 999.0
    u = _f32(rng.uniform(-cur_amp, cur_amp, nrow))
    v = _f32(rng.uniform(-cur_amp, cur_amp, nrow))
    undefined = rng.choice(n, 4, replace=False)      # an exact zero: the current is not defined there
    u[undefined] = v[undefined] = 0.0
    u[nland] = v[nland] = 0.0
    props = syn.depth_props(depth, t, np.float64)
    cg, om, wn = (_f32(props[k]).astype(T) for k in ("CGROUP", "OMOSNH2KD", "WAVNUM"))
    f1 = _f32(rng.uniform(0.0, 1.0, (nrow, nang, nfre)) ** 3).astype(T)
    f1[nland] = 0
    obs = None
    if with_obs:
        obs = np.ones((n, 8, nfre))
        obs[:, :4] = _f32(rng.uniform(0.3, 0.95, (n, 4, nfre)))
        if obscor:      # drawn after the four planes above, which keep their values
            obs[:, 4:] = _f32(rng.uniform(0.3, 0.95, (n, 4, nfre)))
        obs = obs.astype(T)
    zdello, cosph, sinph = _f32(g.zdello).astype(T), _f32(g.cosph).astype(T), _f32(g.sinph).astype(T)
    xdella = float(_f32(g.xdella))
    circ = T(t.CIRC)
    delphi = T(xdella) * circ / T(360.0)
    dellam = zdello * circ / T(360.0)
    dellam1, cosphm1 = np.zeros(nrow, T), np.zeros(nrow, T)
    dellam1[:n] = T(1) / dellam[g.kxlt]
    cosphm1[:n] = T(1) / cosph[g.kxlt]
    return dict(irefra=irefra, icase=icase, irgg=irgg, nland=nland, nr=nr, delpro=float(idelpro), delphi=delphi, xdella=xdella, circ=circ, zdello=zdello,
                dellam=dellam, kxlt=g.kxlt.astype(np.int64), cosph=cosph, sinph=sinph, dellam1=dellam1, cosphm1=cosphm1, klon=g.klon.astype(np.int64),
                klat=g.klat.astype(np.int64), wlat=_f32(g.wlat).astype(T), cg=cg, om=om, wn=wn, u=u.astype(T), v=v.astype(T), depth=depth.astype(T), f1=f1, obs=obs,
                sinth=np.asarray(t.SINTH, T), costh=np.asarray(t.COSTH, T), fr=np.asarray(t.FR, T), delth=T(t.DELTH), r_earth=T(t.R), zpi=T(t.ZPI),
                fratio=T(t.FRATIO))


def make_case(name, T):
    icase, irgg, irefra, with_obs, idelpro = CASES[name]
    return make_inputs(T, fixture_grid(), tables_of(T, irefra=irefra), icase, irgg, irefra, with_obs, idelpro)


def restate(c, T, kijs=0, kijl=None, weights=None):
    """-> dict(f3, thdd, thdc, sdot, cfl, dot) of the restatement on the inputs c of make_inputs"""
    thdd, thdc, s0, omdd = dot_terms(T, c["irefra"], c["icase"], c["nland"], c["kxlt"], c["zdello"], c["xdella"], c["circ"], c["cosph"], c["klon"], c["klat"],
                                     c["wlat"], c["cosphm1"], c["depth"], c["u"], c["v"], c["sinth"], c["costh"])
    keys = ("irefra", "icase", "irgg", "nland", "nr", "delpro", "delphi", "kxlt", "cosph", "sinph", "dellam1", "cosphm1", "klon", "klat", "wlat", "cg", "om", "wn", "u",
            "v", "obs", "sinth", "costh", "fr", "delth", "r_earth", "zpi", "fratio")
    f3, cfl = propags(T, c["f1"], thdd=thdd, thdc=thdc, s0=s0, omdd=omdd, kijs=kijs, kijl=kijl, weights=weights, **{k: c[k] for k in keys})
    sd = sdot(s0, omdd, c["cg"], c["om"], c["wn"], c["nr"]) if c["irefra"] in (2, 3) else np.zeros((thdd.shape[0], thdd.shape[1], c["nr"]), T)
    return dict(f3=f3, thdd=thdd, thdc=thdc, sdot=sd.astype(T), cfl=cfl, dot=dot_row(thdd, thdc, s0, omdd))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the coverage conditions of the fixtures: asserted by tools/make_golden_propags.py on what the reference computed, and by tests/test_propags_host.py
# again on the committed files ------------------------------------------------------------------------------------------------------------------------------
def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f"propags_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def grid_coverage(g):
    """Every direction quadrant, both hemispheres, the periodic wrap, a land neighbour on each of the six positions at >= 3 points, WLAT strictly inside (0, 1)
    at a quarter of the points or more."""
    t = tables_of(np.float64)
    quad = sorted({(bool(s < 0), bool(c < 0)) for s, c in zip(t.SINTH, t.COSTH)})
    assert len(quad) == 4, quad
    north, south = int((g.sinph[g.kxlt] > 0).sum()), int((g.sinph[g.kxlt] < 0).sum())
    assert north > 0 and south > 0
    ij = np.arange(g.nsea)
    wrap = int(((g.klon[:, 0] > ij) & (g.klon[:, 0] != g.nland)).sum() + ((g.klon[:, 1] < ij) & (g.klon[:, 1] != g.nland)).sum())
    assert wrap > 0
    land = {"KLON1": g.klon[:, 0], "KLON2": g.klon[:, 1], "KLAT11": g.klat[:, 0, 0], "KLAT12": g.klat[:, 0, 1], "KLAT21": g.klat[:, 1, 0], "KLAT22": g.klat[:, 1, 1]}
    land = {k: int((v == g.nland).sum()) for k, v in land.items()}
    assert min(land.values()) >= 3, land
    inside = float(((g.wlat > 0) & (g.wlat < 1)).any(axis=1).mean())
    assert inside >= 0.25, inside
    return dict(points=int(g.nsea), quadrants=len(quad), north=north, south=south, wrap_neighbours=wrap, land_neighbours=land, wlat_inside=inside)


def coverage(name, fx, unobstructed=None):
    """The conditions on one case's recorded arrays fx (and, for a case with obstructions, the F3 of the case without them) -> what was observed."""
    icase, irgg, irefra, with_obs, idelpro = CASES[name]
    cur = irefra in (2, 3)
    section = (4 if cur else 3) if icase == 1 else (2 if cur else 1)
    obs = dict(section=section, icase=icase, irgg=irgg, irefra=irefra, obstructions=with_obs, idelpro=idelpro, bit_identical={}, zero_fraction={}, cfl_max={},
               cfl_points_above_1={})
    for p, T in (("sp", np.float32), ("dp", np.float64)):
        c = make_case(name, T)
        w = {}
        r = restate(c, T, weights=w)
        same = {k: bool(same_bits(r[k], fx[f"{k}_{p}"])) for k in ("f3", "thdd", "thdc", "sdot", "cfl") if f"{k}_{p}" in fx}
        obs["bit_identical"][p] = same
        if all(same.values()):      # the restatement's weights are the reference's: they gave its F3 and its CFL numbers bit for bit
            expect = ["DTP", "DTM"] if (icase == 1 or irefra != 0) else []
            if cur:
                expect += ["DLE", "DLW", "DPN", "DPS", "DOP", "DOM"] + (["DPN2", "DPS2"] if icase == 1 and irgg == 1 else [])
            assert sorted(w) == sorted(expect), (name, sorted(w))
            zf = {k: float((v == 0).mean()) for k, v in w.items()}
            assert all(0.05 <= z <= 0.95 for z in zf.values()), (name, zf)
            obs["zero_fraction"][p] = zf
        cfl = fx[f"cfl_{p}"].astype(np.float64)
        above = int((cfl.max(axis=(1, 2)) > 1).sum())
        obs["cfl_max"][p] = float(cfl.max())
        obs["cfl_points_above_1"][p] = above
        if name.startswith("cfl_"):
            assert 0 < above < cfl.shape[0] / 2, (name, above)
        else:
            assert above == 0, (name, above)
        if unobstructed is not None:
            assert not np.array_equal(fx[f"f3_{p}"], unobstructed[f"f3_{p}"]), name
    return obs
