"""MSTART, UNSETICE, the noise start and the tail of GETSPEC restated in numpy from the reference's Fortran (mstart.F90:104-136 with
peak.F90:88-102, spectra.F90:95-120, jonswap.F90:70-91, spr.F90:69-81; unsetice.F90:79-171; sdepthlim.F90:64-78 with semean.F90:82-120;
getspec.F90:174-188 and 648-659), in the reference's order of operations and in the precision asked for: TEST INFRASTRUCTURE.  It is
written from the Fortran, not from the kernels of csrc/start.hip; tests/test_start_host.py holds it against the reference's own results
(tests/golden/start_*.npz, recorded by tools/make_golden_start.py) and tests/test_gpu_start.py uses it for the properties the fixtures do
not hold.  Spectra are [ij][K][M] (the device layout); every scalar stays in the working precision.

make_cases() builds the inputs of the fixtures; the tool and the tests share it.  The gates of the tests are read from
tests/golden/start_observed.json, which the tool writes from the reference's results and this restatement alone.
"""
from __future__ import annotations

import functools
import glob
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from ecwam_amd.tables import Config, Tables, powi  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
NROW, KIJS, KIJL = 67, 3, 67           # the calls act on rows [3, 67); rows 0..2 are guard rows
NFF = 16
C_WDWAVE, C_CICOVER, C_WSWAVE, C_EMAXDPT, C_DEPTH = 1, 2, 3, 14, 15
# (NANG, NFRE, NFRE_RED)
SHAPES = ((12, 36, 36), (24, 36, 36), (24, 36, 29), (36, 36, 36), (48, 36, 36))
# UNSETICE's variants: (LICERUN, LMASKICE, LBIWBK, which DELPHI).  Every shape runs the first two (LMASKICE and LBIWBK on and off, both
# DELPHI); 36 x 36 runs all five.  The last one has LICERUN off beside LMASKICE on: CILIMIT = 0 (unsetice.F90:90-94), so its points with ice
# below CITHRSH are not reset, where the first variant resets them -- a choice of CILIMIT from LMASKICE alone does not pass it.
UNSETICE_VARIANTS = ((1, 1, 1, "small"), (1, 0, 0, "large"), (1, 0, 1, "large"), (1, 1, 0, "small"), (0, 1, 1, "small"))
# DELPHI [m]: with 1 km every MIN of the fetch (unsetice.F90:119-129) takes its first argument (5 DELPHI < 250 km ... 0.5 DELPHI < 10 km), with
# 1000 km its second
DELPHI = dict(small=1000.0, large=1.0e6)
DEPTHS = (10.0, 50.0, 150.0, 250.0, 5.0, 30.0, 100.0, 200.0, 1000.0)
MARGIN = 1.0e-3                        # [rad] every TH(K) - direction stays this far from +-PI/2


def shape_tag(shape) -> str:
    return f"{shape[0]}x{shape[2]}"


def full_shape(shape):
    return (shape[0], shape[1], shape[1])


def unsetice_variants(shape):
    return UNSETICE_VARIANTS if shape[0] == 36 else UNSETICE_VARIANTS[:2]


def config(shape, licerun=True, lmaskice=True, lbiwbk=True) -> Config:
    return Config(nang=shape[0], nfre=shape[1], nfre_red=shape[2], licerun=bool(licerun), lmaskice=bool(lmaskice), lbiwbk=bool(lbiwbk))


def tables(shape, dtype, licerun=True, lmaskice=True, lbiwbk=True) -> Tables:
    return Tables(config(shape, licerun, lmaskice, lbiwbk), dtype)


def variant(call: str):
    """(LICERUN, LMASKICE, LBIWBK, which DELPHI) of the recorded call unsetice<i>"""
    return UNSETICE_VARIANTS[int(call[len("unsetice"):])]


# ---- the routines ---------------------------------------------------------------------------------------------------------------------------
def _jons(T):
    """yowjons.F90:18-21"""
    return T(2.84), T(0.033), T(-3.0) / T(10.0), T(2.0) / T(3.0)


def peak(t, fetch, fpmax, u10, alphaj):
    """peak.F90:88-102 (and unsetice.F90:133-147, the same lines): FP, ALPHAJ; ALPHAJ is kept where the point is calm."""
    T = t.dtype
    AJ, BJ, DJ, EJ = _jons(T)
    gx = t.G * T(fetch)
    on = u10 > T(0.1e-08)
    u = np.where(on, u10, T(1))
    gxu = gx / (u * u)
    ug = t.G / u
    fp = AJ * np.power(gxu, DJ)
    fp = np.maximum(T(0.13), fp)
    fp = np.minimum(fp, T(fpmax) / ug)
    al = BJ * np.power(fp, EJ)
    al = np.maximum(al, T(0.0081))
    fp = fp * ug
    return np.where(on, fp, T(0)).astype(T), np.where(on, al, alphaj).astype(T)


def jonswap(t, alphaj, zgamma, sa, sb, fp):
    """jonswap.F90:70-91: ET [ij][M]"""
    T = t.dtype
    n = fp.shape[0]
    et = np.zeros((n, t.cfg.nfre), T)
    on = (alphaj != T(0)) & (fp != T(0))
    f = np.where(on, fp, T(1)).astype(T)
    with np.errstate(all="ignore"):
        for m in range(t.cfg.nfre):
            frh = T(t.FR[m])
            g2 = T(1) / (powi(frh, 5) * t.ZPI4GM2)
            sigma = np.where(frh > f, T(sb), T(sa)).astype(T)
            x = (frh - f) / (sigma * f)
            earg = np.minimum(T(0.5) * (x * x), T(50))
            fjon = np.power(T(zgamma), np.exp(-earg))
            fmpf = np.minimum(T(1.25) * powi(f / frh, 4), T(50))
            fjonh = np.exp(-fmpf)
            et[:, m] = np.where(on, alphaj * g2 * fjonh * fjon, T(0))
    assert et.dtype == T
    return et


def spr(t, thetaq):
    """spr.F90:69-81: ST [ij][K]"""
    T = t.dtype
    zdp = T(2) / t.PI
    the = np.cos(t.TH[None, :] - thetaq[:, None])
    st = np.where(the > T(0), zdp * (the * the), T(0)).astype(T)
    st[st < T(0.1e-08)] = T(0)
    return st


def mstart(t, iopti, fetch, frmax, thetaq, fm, alfa, zgamma, sa, sb, wswave, wdwave):
    """mstart.F90:104-136: FL1 [ij][K][M] of the points whose winds are given"""
    T = t.dtype
    ws, wd = np.asarray(wswave, T), np.asarray(wdwave, T)
    n = ws.shape[0]
    if iopti == 1:
        fp, al, thes = np.zeros(n, T), np.zeros(n, T), wd.copy()
    elif iopti == 0:
        fp, al, thes = np.full(n, T(fm)), np.full(n, T(alfa)), np.full(n, T(thetaq))
    else:
        fp, al = np.full(n, T(fm)), np.full(n, T(alfa))
        thes = np.where(ws > T(0.1e-08), wd, T(0)).astype(T)
    if iopti != 0:
        fp, al = peak(t, fetch, frmax, ws, al)
    et = jonswap(t, al, zgamma, sa, sb, fp)
    st = spr(t, thes)
    fl = et[:, None, :] * st[:, :, None]
    assert fl.dtype == T
    return fl


def semean(t, fl):
    """semean.F90:82-120 with LLEPSMIN: the directions summed first, in order, then the frequencies in order"""
    T = t.dtype
    em = np.full(fl.shape[0], t.EPSMIN, T)
    temp = None
    for m in range(t.cfg.nfre):
        temp = fl[:, 0, m].copy()
        for k in range(1, t.cfg.nang):
            temp = temp + fl[:, k, m]
        em = em + t.DFIM[m] * temp
    delt25 = t.WETAIL * t.FR[-1] * t.DELTH
    em = em + delt25 * temp
    assert em.dtype == T
    return em


def sdepthlim(t, emaxdpt, fl):
    """sdepthlim.F90:64-78"""
    T = t.dtype
    em = np.minimum(np.asarray(emaxdpt, T) / semean(t, fl), T(1))
    return np.maximum(fl * em[:, None, None], t.EPSMIN).astype(T)


def unsetice_branches(t, fl, depth, wswave, cicover):
    """The decisions of unsetice.F90:89-147 per point: reset (LICE2SEA and CICOVER <= CILIMIT), the depth class 0..4, the wind test."""
    T = t.dtype
    cilimit = t.CITHRSH if (t.cfg.licerun and t.cfg.lmaskice) else T(0)
    lice2sea = ~(fl > t.EPSMIN).any(axis=(1, 2))
    reset = lice2sea & (np.asarray(cicover, T) <= cilimit)
    d = np.asarray(depth, T)
    cls = np.where(d <= T(10), 0, np.where(d <= T(50), 1, np.where(d <= T(150), 2, np.where(d <= T(250), 3, 4))))
    return reset, cls, np.asarray(wswave, T) > T(0.1e-08)


def unsetice(t, delphi, fl, ff):
    """unsetice.F90:79-171 (LRESTARTED = F, CLDOMAIN /= 's'); LICERUN, LMASKICE and LBIWBK are those of t.cfg.  ff [ij][16]."""
    T = t.dtype
    fl = np.asarray(fl, T)
    wd, ci, ws = (np.asarray(ff[:, c], T) for c in (C_WDWAVE, C_CICOVER, C_WSWAVE))
    emaxdpt, depth = np.asarray(ff[:, C_EMAXDPT], T), np.asarray(ff[:, C_DEPTH], T)
    zdp = T(2) / t.PI
    c = np.maximum(T(0), np.cos(t.TH[None, :] - wd[:, None]))
    cos2noise = (c * c).astype(T)
    sprd = zdp * cos2noise
    reset, cls, _ = unsetice_branches(t, fl, depth, ws, ci)
    d = T(delphi)
    fetches = (min(T(0.5) * d, T(10000)), min(d, T(50000)), min(T(2) * d, T(100000)), min(T(3) * d, T(200000)), min(T(5) * d, T(250000)))
    fpmax = t.FR[-2]
    n = fl.shape[0]
    fpk, alphav = np.full(n, fpmax, T), np.zeros(n, T)
    for i in range(5):
        sel = reset & (cls == i)
        if sel.any():
            f, a = peak(t, fetches[i], fpmax, ws[sel], np.zeros(int(sel.sum()), T))
            fpk[sel], alphav[sel] = f, a
    et = jonswap(t, alphav, T(3.0), T(7.0e-02), T(9.0e-02), fpk)
    out = np.maximum(fl, et[:, None, :] * sprd[:, :, None])
    fllowest = (T(1) - T(0.9) * np.minimum(ci, T(0.99))) * t.FLMIN
    out = np.maximum(out, (fllowest[:, None] * cos2noise)[:, :, None]).astype(T)
    if t.cfg.lbiwbk:
        out = sdepthlim(t, emaxdpt, out)
    assert out.dtype == T
    return out


def getspec_tail(t, nfre_red, fl, emaxdpt):
    """getspec.F90:648-659: the frequencies above NFRE_RED from the last one read, then SDEPTHLIM.  FRM5 = 1 / FR5 (initmdl.F90:465-466)."""
    return sdepthlim(t, emaxdpt, fill_tail(t, nfre_red, fl))


def fill_tail(t, nfre_red, fl):
    """getspec.F90:650-656"""
    T = t.dtype
    out = np.array(fl, T)
    fr5 = powi(t.FR, 5)
    frm5 = T(1) / fr5
    for m in range(nfre_red, t.cfg.nfre):
        out[:, :, m] = out[:, :, nfre_red - 1] * fr5[nfre_red - 1] * frm5[m]
    return out


# ---- the inputs of the fixtures ---------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(np.asarray(x, np.float32), np.float64)


def clear_of_cut(th, wd, margin=MARGIN) -> np.ndarray:
    """per direction wd: every TH(K) - wd is at least `margin` from +-PI/2 (modulo 2 PI), where COS changes its sign"""
    d = np.mod(np.asarray(th, np.float64)[None, :] - np.atleast_1d(np.asarray(wd, np.float64))[:, None], 2 * np.pi)
    return ((np.abs(d - 0.5 * np.pi) >= margin) & (np.abs(d - 1.5 * np.pi) >= margin)).all(axis=1)


def _directions(rng, th, n):
    out = np.empty(n)
    for i in range(n):
        while True:
            w = float(_f32(rng.uniform(0.0, 2 * np.pi)))
            if clear_of_cut(th, w)[0]:
                out[i] = w
                break
    return out


def _sea_spectra(rng, t, n):
    """float32-representable wind-sea spectra: JONSWAP with a cos**2 spread (exact zeros on the lee side)"""
    fp = _f32(rng.uniform(0.06, 0.3, n))
    al = _f32(rng.uniform(0.008, 0.02, n))
    et = jonswap(t, al, 3.0, 0.07, 0.09, fp)
    st = spr(t, _directions(rng, t.TH, n))
    return _f32(et[:, None, :] * st[:, :, None])


def make_cases(shape, seed=20261019):
    """The inputs of one shape, in float64 and float32-representable (both precisions see the same numbers): a dict with
    mstart   ff [67][16], params (FETCH, FRMAX, THETAQ, FM, ALFA, ZGAMMA, SA, SB)
    unsetice ff, fl [67][NANG][NFRE], kind [67] (0 noise, 1 one bin at 2 EPSMIN, 2 a sea)
    tail     ff, fl, nfre_red
    The thresholds of the routines are kept clear: directions MARGIN from the zero of the cosine, winds 0, 1e-9 or >= 0.5 m/s, spectra at
    half of EPSMIN and below or at 2 EPSMIN and above, ice covers 0, 0.1, 0.6, 0.995 against CITHRSH 0.3, depths on the class bounds (which are exact in both
    precisions) or well inside, EMAXDPT 0.4 times the smallest or 2.5 times the largest energy the point can have in any variant."""
    nang, nfre, nfre_red = shape
    rng = np.random.default_rng(seed + 1000 * nang + nfre_red)
    t = tables(shape, np.float64)
    eps = float(t.EPSMIN)
    noise = float(_f32(0.5 * eps))      # below EPSMIN in both precisions (EPSMIN itself is not the same number in the two)
    na = KIJL - KIJS
    winds = np.concatenate(([0.0, float(np.float32(1.0e-9))], _f32(np.geomspace(0.5, 40.0, na - 2))))

    def base_ff(ws):
        ff = _f32(rng.uniform(0.0, 1.0, (NROW, NFF)))
        ff[:, C_WDWAVE] = _directions(rng, t.TH, NROW)
        ff[:, C_WSWAVE] = np.concatenate((_f32(rng.uniform(1.0, 20.0, KIJS)), ws))
        return ff

    # MSTART: calm points, then winds from 0.5 to 40 m/s (both clamps of PEAK are taken at the low end, neither at the high end)
    thetaq = 0.7
    while not clear_of_cut(t.TH, float(np.float32(thetaq)))[0]:
        thetaq += 0.01
    params = tuple(float(np.float32(v)) for v in (30000.0, 0.25, thetaq, 0.1, 0.018, 3.0, 0.07, 0.09))
    out = dict(mstart=dict(ff=base_ff(winds), params=params))

    # UNSETICE.  Every second point holds noise only: the j-th of them has the depth DEPTHS[j % 9] and, by j / 9, no ice (reset whatever the
    # switches), ice below CITHRSH (reset with LICERUN .AND. LMASKICE only: not with either of them off), no ice again (two of them calm), ice above CITHRSH (never reset)
    ws = winds[rng.permutation(na)]
    idx = np.arange(na)
    kind = np.concatenate((np.full(KIJS, 2), np.array([0, 1, 0, 2])[idx % 4]))
    noise_pts = KIJS + np.nonzero(kind[KIJS:] == 0)[0]
    for want, j in ((winds[0], 18), (winds[1], 19)):      # the two calm points among the ones that are reset
        i, o = noise_pts[j] - KIJS, int(np.nonzero(ws == want)[0][0])
        ws[i], ws[o] = ws[o], ws[i]
    ff = base_ff(ws)
    ff[KIJS:, C_CICOVER] = _f32(np.array([0.0, 0.1, 0.6, 0.995, 0.0])[idx % 5])
    ff[KIJS:, C_DEPTH] = np.array(DEPTHS)[idx % 9]
    ff[:KIJS, C_DEPTH] = 77.0
    for j, i in enumerate(noise_pts):
        ff[i, C_DEPTH] = DEPTHS[j % 9]
        ff[i, C_CICOVER] = float(_f32((0.0, 0.1, 0.0, (0.6, 0.995)[j % 2])[j // 9]))
    fl = _sea_spectra(rng, t, NROW)
    for i in np.nonzero(kind < 2)[0]:
        fl[i] = np.where(rng.uniform(size=(nang, nfre)) < 0.5, noise, 0.0)
        if kind[i] == 1:
            fl[i, rng.integers(nang), rng.integers(nfre)] = float(_f32(2 * eps))
    assert (fl == _f32(fl)).all()
    e_lo, e_hi = np.full(NROW, np.inf), np.zeros(NROW)
    for lrun, lmask, _, which in UNSETICE_VARIANTS:
        tv = tables(shape, np.float64, lrun, lmask, False)
        e = semean(tv, unsetice(tv, DELPHI[which], fl, ff))
        e_lo, e_hi = np.minimum(e_lo, e), np.maximum(e_hi, e)
    limited = (np.arange(NROW) % 3) != 0
    ff[:, C_EMAXDPT] = _f32(np.where(limited, 0.4 * e_lo, 2.5 * e_hi))
    out["unsetice"] = dict(ff=ff, fl=fl, kind=kind, limited=limited)

    # the tail of GETSPEC
    ff = base_ff(ws)
    fl = _sea_spectra(rng, t, NROW)
    fl[KIJS + 5] = 0.0                                   # an empty point: energy EPSMIN
    fl[:, :, nfre_red:] = _f32(rng.uniform(0.0, 1.0e-3, (NROW, nang, nfre - nfre_red)))      # what the fill overwrites
    e = semean(t, fill_tail(t, nfre_red, fl))
    ff[:, C_EMAXDPT] = _f32(np.where(limited, 0.4 * e, 2.5 * e))
    out["tail"] = dict(ff=ff, fl=fl, nfre_red=nfre_red, limited=limited)
    if nfre_red != nfre:      # MSTART and UNSETICE do not know NFRE_RED: theirs are the inputs (and the recorded results) of the full shape
        full = make_cases(full_shape(shape), seed)
        out["mstart"], out["unsetice"] = full["mstart"], full["unsetice"]
    return out


@functools.lru_cache(maxsize=None)
def cached_cases(shape):
    """make_cases(shape), built once per process and shared: never modified by its users"""
    return make_cases(tuple(shape))


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------------------
def load_golden(shape):
    """Every array of tests/golden/start_<NANG>x<NFRE_RED>_*.npz in one dict (the tool splits a shape's results over files of at most 0.6 MB).
    A shape with NFRE_RED < NFRE holds its tail only: its MSTART and UNSETICE results are those of the full shape (make_cases)."""
    out = {} if shape == full_shape(shape) else load_golden(full_shape(shape))
    files = sorted(glob.glob(os.path.join(GOLDEN, f"start_{shape_tag(shape)}_*.npz")))
    if not files:
        raise FileNotFoundError(f"no fixture of shape {shape} under {GOLDEN}")
    for f in files:
        with np.load(f) as z:
            out.update({k: z[k] for k in z.files})
    return out


def observed():
    with open(os.path.join(GOLDEN, "start_observed.json")) as fh:
        return json.load(fh)


def calls(shape):
    """The names of a shape's recorded results: mstart0..2, unsetice0.., tail."""
    return [f"mstart{i}" for i in range(3)] + [f"unsetice{i}" for i in range(len(unsetice_variants(shape)))] + ["tail"]


def routine_of(call: str) -> str:
    return call.rstrip("0123456789")


def restate(shape, call, prec, cases=None):
    """The restatement's result of one recorded call on the active rows, in precision `prec`."""
    T = np.float32 if prec == "sp" else np.float64
    cases = cases or make_cases(shape)
    r = routine_of(call)
    a = slice(KIJS, KIJL)
    if r == "mstart":
        c = cases["mstart"]
        return mstart(tables(shape, T), int(call[-1]), *c["params"], c["ff"][a, C_WSWAVE], c["ff"][a, C_WDWAVE])
    if r == "unsetice":
        lrun, lmask, lbiwbk, which = variant(call)
        c = cases["unsetice"]
        return unsetice(tables(shape, T, lrun, lmask, lbiwbk), DELPHI[which], c["fl"][a], c["ff"][a])
    c = cases["tail"]
    return getspec_tail(tables(shape, T), shape[2], c["fl"][a], c["ff"][a, C_EMAXDPT])


def pre_limit_energy(shape, call, prec, cases):
    """SEMEAN of what a recorded call hands to SDEPTHLIM, on the active rows, in precision `prec`"""
    T = np.float32 if prec == "sp" else np.float64
    a = slice(KIJS, KIJL)
    if routine_of(call) == "tail":
        t = tables(shape, T)
        return semean(t, fill_tail(t, shape[2], cases["tail"]["fl"][a]))
    lrun, lmask, _, which = variant(call)
    t = tables(shape, T, lrun, lmask, False)
    return semean(t, unsetice(t, DELPHI[which], cases["unsetice"]["fl"][a], cases["unsetice"]["ff"][a]))


def bin_error(got, ref):
    """per point: the largest |got - ref| over the point's largest |ref| bin (0 where the reference's point is empty and so is got)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    peak_ = np.abs(ref).max(axis=(1, 2))
    d = np.abs(got - ref).max(axis=(1, 2))
    return np.where(peak_ > 0, d / np.where(peak_ > 0, peak_, 1), np.where(d > 0, np.inf, 0.0))


def gate(call, prec, obs=None):
    """Double precision: 10 x the largest difference between this restatement and the reference's double precision results, 8 eps where that
    is exactly 0.  Single precision: 3 x the largest difference between the reference's own single and double precision results.  Per routine."""
    obs = obs or observed()
    r = routine_of(call)
    if prec == "dp":
        v = obs["restatement_vs_reference_dp"][r]
        return 10 * v if v > 0 else 8 * float(np.finfo(np.float64).eps)
    return 3 * obs["reference_sp_vs_dp"][r]
