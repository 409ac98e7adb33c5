"""numpy restatement of the dual rotated-quadrant propagation scheme (IPROPAGS = 1), statement by statement in the working precision: section 3 of PROPAGS1
(propags1.F90:537-925) with the inputs of CHECKCFL as it passes them at M = 1 (:867-878).  Sections 1 and 2 are those of PROPAGS: propags_ref.propags is
called as it is.  Section 4 differs from PROPAGS in DP1 / DP2 alone (DCO(IJ) * DCOM1(JH), propags1.F90:203-222): propags_ref.propags, which is left as it
is, is called with COSPHM1_EXT wrapped in _ProductDCO below, so that its one quotient DCO(IJ) / DCO(JH) is formed as the product.  TEST INFRASTRUCTURE:
it serves the shapes the fixtures tests/golden/propags1_*.npz do not have, and tests/test_propags1_host.py holds it to the fixtures bit for bit.

The conventions are those of propags_ref.py.  rot: the tables of ecwam_amd.grid.rotated_tables (or the recorded ones): krlat, krlon [n][2][2], wrlat, wrlon
[n][2], cdr, sdr [n + 1][K], prqrt [n], sqrt2.  obs [n][8][NFRE]: OBSLAT(:,:,1:2), OBSLON(:,:,1:2), OBSRLAT(:,:,1:2), OBSRLON(:,:,1:2)."""
import dataclasses
import json
import os

import numpy as np

import propags_ref as P

NCFL = P.NCFL
GOLDEN = P.GOLDEN
same_bits = P.same_bits
ROT_KEYS = ("krlat", "krlon", "wrlat", "wrlon", "cdr", "sdr", "prqrt", "sqrt2")


class _ProductDCO(np.ndarray):
    """COSPHM1_EXT for section 4 of PROPAGS1.  propags_ref.propags divides two elements of this array in one place only, DP1 / DP2 = DCO(IJ) / DCO(JH)
    (propags.F90:217-224): here that quotient is DCO(IJ) * (1 / DCO(JH)), the DCO(IJ) * DCOM1(JH) of propags1.F90:203-222.  Every other operation gives a
    plain array, so nothing else changes (tests/test_propags1_host.py holds the result to the reference's section 4 bit for bit)."""

    def __truediv__(self, other):
        a = np.asarray(self)
        if isinstance(other, _ProductDCO):
            return a * (a.dtype.type(1) / np.asarray(other))
        return a / other

    def __mul__(self, other):
        return np.asarray(self) * other

    __rmul__ = __mul__


def propags1(T, f1, rot, *, irefra, icase, irgg, nland, nr, delpro, delphi, kxlt, cosph, sinph, dellam1, cosphm1, klon, klat, wlat, cg, om, wn, u, v, thdd, thdc,
             s0, omdd, obs, sinth, costh, fr, delth, r_earth, zpi, fratio, kijs=0, kijl=None, choice=None):
    """-> F3 [kijl - kijs][K][NFRE_RED], CFL [kijl - kijs][K][11].  choice: a dict that receives IJRLA and IJRPH [kijl - kijs][K] (1 or 2)."""
    common = dict(irefra=irefra, icase=icase, irgg=irgg, nland=nland, nr=nr, delpro=delpro, delphi=delphi, kxlt=kxlt, cosph=cosph, sinph=sinph, dellam1=dellam1,
                  cosphm1=cosphm1, klon=klon, klat=klat, wlat=wlat, cg=cg, om=om, wn=wn, u=u, v=v, thdd=thdd, thdc=thdc, s0=s0, omdd=omdd, obs=obs, sinth=sinth,
                  costh=costh, fr=fr, delth=delth, r_earth=r_earth, zpi=zpi, fratio=fratio, kijs=kijs, kijl=kijl)
    if icase != 1:      # sections 1 and 2
        return P.propags(T, f1, **common)
    if irefra in (2, 3):      # section 4
        return P.propags(T, f1, **dict(common, cosphm1=np.ascontiguousarray(cosphm1).view(_ProductDCO)))
    # ---- section 3
    n = klon.shape[0]
    kijl = n if kijl is None else kijl
    A = np.arange(kijs, kijl)
    nang = sinth.shape[0]
    one = T(1)
    delpro, delphi = T(delpro), T(delphi)
    f3 = np.zeros((A.size, nang, nr), T)
    cfl = np.zeros((A.size, nang, NCFL), T)
    lon = [klon[A, 0], klon[A, 1]]
    lat = [[klat[A, 0, 0], klat[A, 0, 1]], [klat[A, 1, 0], klat[A, 1, 1]]]
    krlat, krlon = rot["krlat"].astype(np.int64), rot["krlon"].astype(np.int64)
    wrlat, wrlon, cdr, sdr = rot["wrlat"][A], rot["wrlon"][A], rot["cdr"], rot["sdr"]
    prqrt, sqrt2 = rot["prqrt"][A], T(rot["sqrt2"])
    della0 = delpro * dellam1
    dco = cosphm1
    with np.errstate(divide="ignore", invalid="ignore"):      # the land slot of COSPHM1_EXT is 0; its product is not taken
        dcom1 = one / dco
        dp = [np.where(lat[0][0] == nland, one, dco[A] * dcom1[lat[0][0]]).astype(T), np.where(lat[1][0] == nland, one, dco[A] * dcom1[lat[1][0]]).astype(T)]
    tanph = (sinph[kxlt[A]] / cosph[kxlt[A]]).astype(T)
    delth0 = T(0.25) * delpro / T(delth)
    delph0 = T(0.5) * delpro / delphi
    cofdelph0r = T(0.5) * delpro / (sqrt2 * delphi)
    delph0r = prqrt * cofdelph0r
    della0r = delph0r
    dladco = (one - prqrt) * (dco[A] * della0[A])
    wl = [wlat[A, 0], wlat[A, 1]]
    wlm1 = [one - wl[0], one - wl[1]]
    wrlatm1, wrlonm1 = one - wrlat, one - wrlon
    c0 = cg[A, :nr]
    cgklon = [np.where((lon[ic] == nland)[:, None], T(2) * c0, cg[lon[ic], :nr] + c0) for ic in range(2)]
    cgklat = []
    for ic in range(2):
        l1, l2 = lat[ic][0] == nland, lat[ic][1] == nland
        c1, c2 = cg[lat[ic][0], :nr], cg[lat[ic][1], :nr]
        w, wm, d = wl[ic][:, None], wlm1[ic][:, None], dp[ic][:, None]
        both = c0 * (d + one)
        first = c0 + d * (w * c2 + wm * c2)
        second = c0 + d * (w * c1 + wm * c1)
        none = c0 + d * (w * c1 + wm * c2)
        cgklat.append(np.where((l1 & l2)[:, None], both, np.where(l1[:, None], first, np.where(l2[:, None], second, none))).astype(T))
    ob = None if obs is None else obs[A]
    obslon = [cgklon[i] if ob is None else ob[:, 2 + i, :nr] * cgklon[i] for i in range(2)]
    obslat = [cgklat[i] if ob is None else ob[:, i, :nr] * cgklat[i] for i in range(2)]
    obsrlat = [None if ob is None else ob[:, 4 + i, :nr] for i in range(2)]
    obsrlon = [None if ob is None else ob[:, 6 + i, :nr] for i in range(2)]
    # the rotated neighbours of the advection speeds, a land point replaced by the point itself (:766-785)
    sel = lambda tab, ic, j: np.where(tab[A, ic, j] != nland, tab[A, ic, j], A)      # noqa: E731
    kla = [[sel(krlat, ic, 0), sel(krlat, ic, 1)] for ic in range(2)]
    klo = [[sel(krlon, ic, 0), sel(krlon, ic, 1)] for ic in range(2)]
    pick = lambda two, idx: np.where(idx == 0, two[0], two[1])      # noqa: E731
    for k in range(nang):
        kp1, km1 = (k + 1) % nang, (k - 1) % nang
        sd, cd = sinth[k], costh[k]
        ijla, ijph = (1 if sd < 0 else 0), (1 if cd < 0 else 0)
        sda2 = T(0.5) * np.abs(sd)
        cda = np.abs(cd)
        delph0_cda = (one - prqrt) * delph0 * cda
        sddl = sda2 * dladco
        ijrla = np.where(sdr[A, k] < 0, 1, 0)
        ijrph = np.where(cdr[A, k] < 0, 1, 0)
        if choice is not None:
            choice.setdefault("IJRLA", np.zeros((A.size, nang), np.int64))[:, k] = ijrla + 1
            choice.setdefault("IJRPH", np.zeros((A.size, nang), np.int64))[:, k] = ijrph + 1
        sp = delth0 * (sinth[k] + sinth[kp1]) / T(r_earth)
        sm = delth0 * (sinth[k] + sinth[km1]) / T(r_earth)
        drgp, drgm = tanph * sp, tanph * sm
        if irefra == 1:
            drdp = (thdd[A, k] + thdd[A, kp1]) * delth0
            drdm = (thdd[A, k] + thdd[A, km1]) * delth0
        f_lat1, f_lat2, f_lon = lat[ijph][0], lat[ijph][1], lon[ijla]
        f_rla1, f_rla2 = pick([krlat[A, 0, 0], krlat[A, 1, 0]], ijrph), pick([krlat[A, 0, 1], krlat[A, 1, 1]], ijrph)
        f_rlo1, f_rlo2 = pick([krlon[A, 0, 0], krlon[A, 1, 0]], ijrla), pick([krlon[A, 0, 1], krlon[A, 1, 1]], ijrla)
        for m in range(nr):
            cflea = sddl * cgklon[1 - ijla][:, m]
            dtc = cflea
            dle = sddl * obslon[ijla][:, m]
            cflno = delph0_cda * cgklat[1 - ijph][:, m]
            dtc = dtc + cflno
            xx = delph0_cda * obslat[ijph][:, m]
            dpn = wl[ijph] * xx
            dpn2 = wlm1[ijph] * xx
            acgkrlat, acgkrlon = [], []
            for ic in range(2):
                a1, a2 = kla[ic]
                o1, o2 = klo[ic]
                acgkrlat.append(np.abs(cg[A, m] * cdr[A, k] + wrlat[:, ic] * cg[a1, m] * cdr[a1, k] + wrlatm1[:, ic] * cg[a2, m] * cdr[a2, k]))
                acgkrlon.append(np.abs(cg[A, m] * sdr[A, k] + wrlon[:, ic] * cg[o1, m] * sdr[o1, k] + wrlonm1[:, ic] * cg[o2, m] * sdr[o2, k]))
            xx = dco[A] * della0r
            cflear = xx * pick(acgkrlon, 1 - ijrla)
            dtc = dtc + cflear
            ff = xx * pick(acgkrlon, ijrla)
            if ob is not None:
                ff = ff * pick([obsrlon[0][:, m], obsrlon[1][:, m]], ijrla)
            rle = pick([wrlon[:, 0], wrlon[:, 1]], ijrla) * ff
            rle2 = pick([wrlonm1[:, 0], wrlonm1[:, 1]], ijrla) * ff
            xx = dco[A] * delph0r
            cflnor = xx * pick(acgkrlat, 1 - ijrph)
            dtc = dtc + cflnor
            ff = xx * pick(acgkrlat, ijrph)
            if ob is not None:
                ff = ff * pick([obsrlat[0][:, m], obsrlat[1][:, m]], ijrph)
            rpn = pick([wrlat[:, 0], wrlat[:, 1]], ijrph) * ff
            rpn2 = pick([wrlatm1[:, 0], wrlatm1[:, 1]], ijrph) * ff
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
            f3[:, k, m] = ((one - dtc) * f1[A, k, m] + dpn * f1[f_lat1, k, m] + dpn2 * f1[f_lat2, k, m] + dle * f1[f_lon, k, m] + rpn * f1[f_rla1, k, m]
                           + rpn2 * f1[f_rla2, k, m] + rle * f1[f_rlo1, k, m] + rle2 * f1[f_rlo2, k, m] + dtp * f1[A, kp1, m] + dtm * f1[A, km1, m])
            if m == 0:      # :867-878: the unrotated numbers rescaled, a DTC of them alone
                cgomfull = one / (one - prqrt)
                cflea = cflea * cgomfull
                cflno = cflno * cgomfull
                dtc = cflea + cflno + cfltp + cfltm
                for i, a in enumerate((dtc, cflea, cflea, cflno, cflno, cflno, cflno, cfltp, cfltm, cfltp, cfltm)):
                    cfl[:, k, i] = a
    return f3, cfl


# ---- the recorded cases (tools/make_golden_propags1.py writes tests/golden/propags1_<case>.npz; the tests rebuild the inputs) ----------------------------
NANG, NFRE = P.NANG, P.NFRE
# name -> grid, ICASE, IRGG, IREFRA, obstructions, IDELPRO, NFRE_RED
CASES = {
    "rot_irefra0": ("o3", 1, 1, 0, False, P.DELPRO, 25), "rot_irefra1": ("o3", 1, 1, 1, False, P.DELPRO, 25),
    "rot_obs_irefra0": ("o3", 1, 1, 0, True, P.DELPRO, 25), "rot_obs_irefra1": ("o3", 1, 1, 1, True, P.DELPRO, 25),
    "rot_cfl_irefra0": ("o3", 1, 1, 0, False, P.DELPRO_CFL0, 25),
    "rot_hilat_irefra0": ("o5", 1, 1, 0, False, P.DELPRO, 13),
    "sec4_irefra3": ("o3", 1, 1, 3, False, P.DELPRO, 25),
    "cart_irefra1": ("o3", 2, 1, 1, False, P.DELPRO, 25), "cart_irefra3": ("o3", 2, 1, 3, False, P.DELPRO, 25),
}
UNOBSTRUCTED = {"rot_obs_irefra0": "rot_irefra0", "rot_obs_irefra1": "rot_irefra1"}
# the fixture of the IPROPAGS = 0 scheme on the same inputs
PROPAGS0 = {"cart_irefra1": "cart_irefra1", "cart_irefra3": "cart_irefra3", "sec4_irefra3": "sph_irgg1_irefra3"}
TABLES = ("klat", "klon", "krlat", "krlon", "wlat", "wrlat", "wrlon", "cdr", "sdr", "prqrt", "sqrt2")
PREC = {"sp": np.float32, "dp": np.float64}
_GRIDS = {}


def fixture_grid(key):
    from ecwam_amd import grid

    if key not in _GRIDS:
        _GRIDS[key] = P.fixture_grid() if key == "o3" else grid.build_grid(5, "continents", seed=24, land_fraction=0.5)
    return _GRIDS[key]


def rounded_grid(g):
    """g with the increments and COSPH rounded to single precision, as make_inputs hands them to both precisions"""
    return dataclasses.replace(g, zdello=P._f32(g.zdello), xdella=float(P._f32(g.xdella)), cosph=P._f32(g.cosph))


def make_case(name, T):
    key, icase, irgg, irefra, with_obs, idelpro, nr = CASES[name]
    t = P.tables_of(T, nfre_red=nr, irefra=irefra)
    return P.make_inputs(T, fixture_grid(key), t, icase, irgg, irefra, with_obs, idelpro, obscor=with_obs)


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f"propags1_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def recorded_rot(fx, p):
    """the rotated tables of a fixture in precision p, 0-based"""
    rot = {k: fx[f"{k}_{p}"] for k in ROT_KEYS}
    rot["sqrt2"] = rot["sqrt2"].reshape(())[()]
    return rot


def restate(c, T, rot, kijs=0, kijl=None, choice=None):
    """-> dict(f3, cfl) of the restatement on the inputs c of make_inputs and the tables rot"""
    thdd, thdc, s0, omdd = P.dot_terms(T, c["irefra"], c["icase"], c["nland"], c["kxlt"], c["zdello"], c["xdella"], c["circ"], c["cosph"], c["klon"], c["klat"],
                                       c["wlat"], c["cosphm1"], c["depth"], c["u"], c["v"], c["sinth"], c["costh"])
    keys = ("irefra", "icase", "irgg", "nland", "nr", "delpro", "delphi", "kxlt", "cosph", "sinph", "dellam1", "cosphm1", "klon", "klat", "wlat", "cg", "om", "wn", "u",
            "v", "obs", "sinth", "costh", "fr", "delth", "r_earth", "zpi", "fratio")
    f3, cfl = propags1(T, c["f1"], rot, thdd=thdd, thdc=thdc, s0=s0, omdd=omdd, kijs=kijs, kijl=kijl, choice=choice, **{k: c[k] for k in keys})
    return dict(f3=f3, cfl=cfl, dot=P.dot_row(thdd, thdc, s0, omdd))


def ulps(a, b):
    """the largest distance of a and b in units in the last place of their (common) format"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    I = np.int32 if a.dtype == np.float32 else np.int64

    def key(x):
        i = x.view(I).astype(np.int64)
        return np.where(i < 0, np.iinfo(I).min - i, i)
    return int(np.abs(key(a) - key(b)).max()) if a.size else 0


# ---- the coverage conditions: asserted by tools/make_golden_propags1.py on what the reference computed, and by tests/test_propags1_host.py on the committed files
def table_coverage(key, tab, n):
    """The conditions on the recorded tables of one grid in one precision -> what was observed"""
    nl = n
    pos = {"SW": tab["krlon"][:, 0], "SE": tab["krlat"][:, 0], "NW": tab["krlat"][:, 1], "NE": tab["krlon"][:, 1]}
    obs = {}
    for nm, a in pos.items():
        d = dict(land_closest=int((a[:, 0] == nl).sum()), one_land=int(((a[:, 0] == nl) ^ (a[:, 1] == nl)).sum()),
                 two_sea=int(((a[:, 0] != nl) & (a[:, 1] != nl) & (a[:, 0] != a[:, 1])).sum()))
        assert min(d.values()) >= 5, (key, nm, d)
        obs[nm] = d
    for nm, w in (("WRLAT1", tab["wrlat"][:, 0]), ("WRLAT2", tab["wrlat"][:, 1]), ("WRLON1", tab["wrlon"][:, 0]), ("WRLON2", tab["wrlon"][:, 1])):
        inside = float(((w > 0) & (w < 1)).mean())
        assert inside >= 0.25, (key, nm, inside)
        obs[nm + "_inside"] = inside
    pr = tab["prqrt"]
    obs["prqrt_below_half"], obs["prqrt_half"], obs["prqrt_min"] = float((pr < 0.5).mean()), float((pr == 0.5).mean()), float(pr.min())
    if key == "o5":
        assert obs["prqrt_below_half"] >= 0.10 and obs["prqrt_half"] >= 0.10, (key, obs)
    for nm, a in (("IJRLA", tab["sdr"][:n] < 0), ("IJRPH", tab["cdr"][:n] < 0)):
        assert a.any() and not a.all(), (key, nm)
        obs[nm + "_2"] = float(a.mean())
    return obs


def case_coverage(name, fx, unobstructed=None):
    """The conditions on one case's recorded arrays -> what was observed"""
    obs = dict(cfl_max={}, cfl_points_above_1={})
    for p in PREC:
        cfl = fx[f"cfl_{p}"].astype(np.float64)
        above = int((cfl.max(axis=(1, 2)) > 1).sum())
        obs["cfl_max"][p], obs["cfl_points_above_1"][p] = float(cfl.max()), above
        if name == "rot_cfl_irefra0":
            assert 0 < above < cfl.shape[0] / 2, (name, above)
        else:
            assert above == 0, (name, above)
        if unobstructed is not None:
            assert not np.array_equal(fx[f"f3_{p}"], unobstructed[f"f3_{p}"]), name
    return obs


def observed():
    with open(os.path.join(GOLDEN, "propags1_observed.json")) as fh:
        return json.load(fh)
