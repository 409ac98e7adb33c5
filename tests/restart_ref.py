"""The inputs, the cases and a numpy restatement of what include/ecwam_hip_restart.h serves -- BUILDSTRESS with GETSTRESS's statements around it, the
sixteen restart fields and WRITEFL's record -- shared by tools/make_golden_restart.py (which runs the reference on these inputs and records
tests/golden/restart_0.npz and restart_observed.json), tests/test_restart_host.py and tests/test_gpu_restart.py.  Every input is representable in
single precision, so that both precisions of the reference see the same numbers; the constants are those of ecwam_amd.tables in the working
precision, which is what the device's tables hold."""
import json
import os

import numpy as np

import reference_cases as RC
from ecwam_amd.tables import Config, Tables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, NANG, NFRE, NFF = 67, 12, 36, 16
NCELL = 91                      # the cells of the inbound grid: more than the rows, no multiple of 64 or 4
ZMISS, PRCHAR, SENT = -999.0, 0.0185, -7777.0
DATES = ("20261020120000", "20261020180000", "20261021000000", "20261020060000")      # CDTPRO, CDATEWO, CDAWIFL, CDATEFL
# the columns of ff (include/ecwam_hip.h) and the order of the restart fields (savstress.F90:112-127)
AIRD, WDWAVE, CICOVER, WSWAVE, WSTAR, USTRA, VSTRA, UFRIC, TAUW, TAUWDIR, Z0M, Z0B, CHRNCK, CITHICK = range(14)
FF_NAMES = ("AIRD", "WDWAVE", "CICOVER", "WSWAVE", "WSTAR", "USTRA", "VSTRA", "UFRIC", "TAUW", "TAUWDIR", "Z0M", "Z0B", "CHRNCK", "CITHICK")
RESTART_FF_COLUMNS = (3, 1, 7, 8, 9, 10, 11, 12, 0, 4, 2, 13, 5, 6)
GATED = tuple(range(3, 13))     # the ten columns of ff from WSWAVE to CHRNCK: what BUILDSTRESS reads or writes, and the three between them it must not touch
# name: LLCAPCHNK, a plane of drag coefficients, a plane of wind speeds, ZREF (TEMPXNLEV), LNSESTART
CASES = {"A": (True, True, True, 10.0, False), "B": (False, True, True, 10.0, False), "C": (True, True, False, 8.0, False),
         "D": (False, False, True, 10.0, False), "E": (True, False, False, 8.0, False), "F": (False, False, True, 10.0, True)}
# the bits of the branch code the driver and the restatement write per point.  tauw_zero: the argument of MAX(.., 0) in TAUW is at most
# 4 EPSILON UFRIC**2.  Where the Charnock floor wins Z0M, CHARNOCKOG is (ALPHAOG UFRIC**2) / UFRIC**2 rounded, within two roundings of ALPHAOG, so
# that 1 - (ALPHAOG/CHARNOCKOG)**2 is 0 or a few units of roundoff (at most 7, i.e. 3.5 EPSILON), whichever way the last bits of ALPHAOG fall:
# which of the two it is says nothing about a branch, and the reference's own two precisions differ in it.
BR_UWAVE, BR_CD, BR_WSPMIN, BR_Z0MIN, BR_EPSUS, BR_FLOOR_Z0M, BR_TAUW0 = (1 << i for i in range(7))
BRANCH_NAMES = ("uwave_taken", "cd_taken", "wspmin", "z0min", "epsus", "charnock_floor_z0m", "tauw_zero")


def tauw_zero(ff, T):
    """the set of points whose TAUW is clipped: 0, or the roundoff described above"""
    return ff[:, TAUW] <= T(4) * np.finfo(T).eps * (ff[:, UFRIC] * ff[:, UFRIC])


CONSTANTS = ("WSPMIN", "CDMAX", "EPSUS", "EPSU10", "XKAPPA", "RNUM", "ALPHA", "ALPHAMIN", "CHNKMIN_U", "GM1", "G")
C1CD, C2CD, P1CD, P2CD, Z0MIN = 1.03e-3, 0.04e-3, 1.48, -0.21, 0.000001      # yowpcons.F90:61-64, cdustarz0.F90:57


def dtype_of(prec):
    return np.float32 if prec == "sp" else np.float64


def config(llcapchnk=True, nang=NANG):
    return Config(nang=nang, nfre=NFRE, nfre_red=NFRE, llcapchnk=llcapchnk)


_TABLES = {}


def tables(prec, llcapchnk=True, nang=NANG):
    key = (prec, bool(llcapchnk), nang)
    if key not in _TABLES:
        _TABLES[key] = Tables(config(llcapchnk, nang), dtype_of(prec))
    return _TABLES[key]


def permutation(n=N):
    """IJ2NEWIJ, 0-based: fixed, no fixed structure a transposition bug could hide behind (a multiplier coprime to n, then a swap of the ends)."""
    m = 29
    while np.gcd(m, n) != 1:      # coprime to n for every n
        m += 2
    p = (np.arange(n, dtype=np.int64) * m + 11) % n
    p[[0, n - 1]] = p[[n - 1, 0]]
    assert np.array_equal(np.sort(p), np.arange(n)) and not np.array_equal(p, np.arange(n))
    return p.astype(np.int32)


def make_inputs(seed=20261021):
    """ff [N][16], the inbound map, the planes uwave and cd [NCELL], all float32-representable (returned as float64)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    ff = rng.uniform(0.05, 5.0, (N, NFF))
    ff[:, WSWAVE] = rng.uniform(0.2, 45.0, N)                 # both sides of WSPMIN = 1 and of CHNKMIN_U
    ff[:6, WSWAVE] = [0.999, 1.0, 1.001, 0.01, 0.02, 33.0]
    ff[:, WDWAVE] = rng.uniform(0.0, 2 * np.pi, N)
    ff[:, 14] = rng.uniform(0.1, 60.0, N)
    ff[:, 15] = rng.uniform(2.0, 900.0, N)
    map_in = rng.permutation(NCELL)[:N].astype(np.int32)
    uwave = rng.uniform(0.2, 40.0, NCELL)
    uwave[rng.permutation(NCELL)[:20]] = ZMISS
    uwave[rng.permutation(NCELL)[:12]] = 0.0
    uwave[rng.permutation(NCELL)[:6]] = -2.5
    uwave[map_in[3]], uwave[map_in[4]] = ZMISS, 0.0           # rows 3 and 4 keep their 0.01 and 0.02 m/s: CD MAX(U**2, EPSU10**2) below EPSUS
    uwave[map_in[7]] = 0.015                                  # and one row takes such a value from the plane
    cd = 10 ** rng.uniform(np.log10(3.0e-4), np.log10(3.5e-3), NCELL)      # Z0TOT - RNUM/USTAR on both sides of the Charnock floor
    cd[rng.permutation(NCELL)[:15]] = ZMISS
    cd[rng.permutation(NCELL)[:8]] = 0.0
    cd[rng.permutation(NCELL)[:5]] = -1.0e-3
    cd[map_in[3]], cd[map_in[4]], cd[map_in[7]] = 4.0e-4, 6.0e-4, 5.0e-4
    return dict(ff=f32(ff), map_in=map_in, uwave=f32(uwave), cd=f32(cd))


def restart_state():
    """What the restart files hold: FL [N][NANG][NFRE], ff [N][16], ucur, vcur [N] -- every element another number, exact in single precision."""
    ij, k, m = np.meshgrid(np.arange(N), np.arange(NANG), np.arange(NFRE), indexing="ij")
    fl = ij + N * (k + NANG * m) + 0.5
    ff = np.arange(NFF)[None, :] * 1000.0 + np.arange(N)[:, None] + 0.25
    ucur = 20000.0 + np.arange(N) + 0.125
    vcur = -21000.0 - np.arange(N) - 0.375
    assert np.array_equal(fl.astype(np.float32), fl)
    return dict(fl=fl, ff=ff, ucur=ucur, vcur=vcur)


def rfield_of(ff, ucur, vcur, perm=None):
    """The sixteen vectors in the order of savstress.F90:112-127; perm: position p holds row perm[p] (writestress.F90:105)."""
    r = np.stack([ff[:, c] for c in RESTART_FF_COLUMNS] + [ucur, vcur])
    return r if perm is None else r[:, perm]


def record_of(fl, perm=None):
    """(((FL(IJ,K,M),IJ),K),M) of writefl.F90:113, or :117 with perm; fl is [ij][K][M]."""
    a = np.transpose(fl, (2, 1, 0))
    return np.ascontiguousarray(a if perm is None else a[:, :, perm]).reshape(-1)


def buildstress(prec, name, inp=None):
    """BUILDSTRESS 1.2 to 1.5 with GETSTRESS's statements around it in numpy, in the working precision and the reference's order of operations:
    -> (ff [N][16], CD [N], the branch code [N])."""
    T = dtype_of(prec)
    cap, has_cd, has_uw, zref, nse = CASES[name]
    t = tables(prec, cap)
    inp = inp or make_inputs()
    c = {k: T(getattr(t, k)) for k in CONSTANTS}
    ff = inp["ff"].astype(T).copy()
    br = np.zeros(N, np.int32)
    zm = T(ZMISS)
    ff[:, Z0B] = T(0)
    ws = ff[:, WSWAVE].copy()
    if has_uw:
        w = inp["uwave"].astype(T)[inp["map_in"]]
        take = (w != zm) & (w > T(0))
        ws = np.where(take, w, ws)
        br |= np.where(take, BR_UWAVE, 0)
    ff[:, WSWAVE] = ws
    zref = T(zref)
    with np.errstate(over="ignore"):
        u10p = np.maximum(ws, c["WSPMIN"])
        br |= np.where(ws < c["WSPMIN"], BR_WSPMIN, 0)
        cdv = np.minimum((T(C1CD) + T(C2CD) * u10p ** T(P1CD)) * u10p ** T(P2CD), c["CDMAX"])
        ustar = np.maximum(np.sqrt(cdv) * u10p, c["EPSUS"])
        z0 = zref / (np.exp(c["XKAPPA"] * np.minimum(u10p / ustar, T(100))) - T(1))
        br |= np.where(z0 < T(Z0MIN), BR_Z0MIN, 0)
        z0 = np.maximum(z0, T(Z0MIN))
    ff[:, UFRIC], ff[:, Z0M] = ustar, z0
    ff[:, TAUW] = T(0.1) * (ustar * ustar)
    ff[:, TAUWDIR] = ff[:, WDWAVE]
    if has_cd:
        x = inp["cd"].astype(T)[inp["map_in"]]
        take = (x != zm) & (x > T(0))
        cdv = np.where(take, x, cdv)
        br |= np.where(take, BR_CD, 0)
        if cap:
            alphaog = (c["ALPHAMIN"] + (c["ALPHA"] - c["ALPHAMIN"]) * T(0.5) * (T(1) - np.tanh(ws - c["CHNKMIN_U"]))) * c["GM1"]
        else:
            alphaog = np.full(N, c["ALPHA"] * c["GM1"], T)
        uf = cdv * np.maximum(ws * ws, c["EPSU10"] * c["EPSU10"])
        br |= np.where(uf < c["EPSUS"], BR_EPSUS, 0)
        uf = np.maximum(uf, c["EPSUS"])
        us = np.sqrt(uf)
        cdsqrtinv = np.minimum(T(1) / np.sqrt(cdv), T(50))
        z0tot = zref * np.exp(-c["XKAPPA"] * cdsqrtinv)
        a, b = z0tot - c["RNUM"] / us, alphaog * uf
        br |= np.where(a < b, BR_FLOOR_Z0M, 0)
        z0m = np.maximum(a, b)
        ch = z0m / uf
        ch = np.maximum(ch, alphaog)
        q = alphaog / ch
        tw = uf * (T(1) - q * q)
        br |= np.where(tw <= T(4) * np.finfo(T).eps * uf, BR_TAUW0, 0)
        ff[:, Z0M], ff[:, TAUW], ff[:, TAUWDIR], ff[:, CHRNCK], ff[:, UFRIC] = z0m, np.maximum(tw, T(0)), ff[:, WDWAVE], c["G"] * ch, us
    if nse:
        ff[:, CHRNCK] = T(PRCHAR)
        ff[:, TAUW] = T(0)
    assert ff.dtype == T and cdv.dtype == T
    return ff, cdv, br


def rel_error(a, b):
    """per column: |a - b| / max(|b|, the column's largest |b|), the maximum over the column"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.maximum(np.abs(b), np.abs(b).max(axis=0, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(a == b, 0.0, np.abs(a - b) / scale)
    return e.max(axis=0)


_CACHE = {}


def load_golden():
    if "g" not in _CACHE:
        with np.load(os.path.join(GOLDEN, "restart_0.npz")) as z:
            _CACHE["g"] = {k: z[k] for k in z.files}
    return _CACHE["g"]


def observed():
    if "o" not in _CACHE:
        with open(os.path.join(GOLDEN, "restart_observed.json")) as fh:
            _CACHE["o"] = json.load(fh)
    return _CACHE["o"]


def cached_inputs():
    if "i" not in _CACHE:
        _CACHE["i"] = make_inputs()
    return _CACHE["i"]


def device_gate(section, key, prec):
    """The device's gate on a column or array: single precision 4 x the reference's own single against double precision; double precision the
    project's rule (reference_cases.dp_gate_of without a ceiling: 10 x the restatement's distance, DP_ZERO_FLOOR where that is exactly 0)."""
    o = observed()
    if prec == "sp":
        return 4.0 * float(o["reference_sp_vs_dp"][section][key])
    r = float(o["restatement_vs_reference_dp"][section][key])
    return 10.0 * r if r > 0.0 else RC.DP_ZERO_FLOOR


def host_gate(section, key, prec):
    """The restatement on another machine (another numpy, another libm) against the recorded figures: 10 x what the tool observed here; where it
    observed exactly 0, a few units in the last place of the precision (DP_ZERO_FLOOR and its single precision counterpart)."""
    r = float(observed()[f"restatement_vs_reference_{prec}"][section][key])
    if r > 0.0:
        return 10.0 * r
    return 8 * float(np.finfo(np.float32).eps) if prec == "sp" else RC.DP_ZERO_FLOOR


def emaxdpt(depth, prec):
    """initdpthflds.F90:64-73 in the working precision"""
    T = dtype_of(prec)
    d = np.asarray(depth, T)
    g = T(tables(prec).GAM_B_J)
    gam = np.where(d < T(4), g * d / T(4), g)
    return T(0.0625) * (gam * d) ** 2
