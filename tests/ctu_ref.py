"""The recorded cases of the corner-transport path with refraction and sub-grid obstructions (tests/golden/ctu_<case>.npz, written by tools/make_golden_ctu.py
from the reference's own PROPDOT / GRADI, CTUWINI, CTUWDRV / CTUW and PROPAGS2): their inputs, which the tests rebuild, the oracle's run on them, and the
coverage conditions the tool asserts on what the reference alone computed.  TEST INFRASTRUCTURE.

The grid and the fields are those of tests/propags_ref.py (the O3 grid with 61 sea points and the land slot, every field rounded to single precision), with
NFRE_RED 26 -- even bounds, so that the device takes its two-frequencies-per-thread stencil -- depths of 12 m and more, and one time step for all plain cases,
IDELPRO, long enough on this coarse grid that the weights are large: a wrong weight does not hide in the tolerance."""
import os
import types

import numpy as np

import propags_ref as P

GOLDEN = P.GOLDEN
NANG, NFRE, NFRE_RED = 12, 36, 26
IDELPRO = 9600
DEPTH_LO = 12.0
SDOT_M = (1, 13, 26)      # the frequencies (1-based) at which SDOT is recorded
PREC = {"sp": np.float32, "dp": np.float64}
WEIGHTS = ("SUMWN", "WLONN", "WLATN", "WCORN", "WKPMN", "WMPMN")
# name -> IREFRA, obstructions, IFRELFMAX (0: no split; else DELPRO_LF = IDELPRO / 2), the largest current component [m/s]
CASES = {
    "irefra0": (0, False, 0, 1.5), "irefra1": (1, False, 0, 1.5), "irefra2": (2, False, 0, 1.5), "irefra3": (3, False, 0, 1.5),
    "obs_irefra0": (0, True, 0, 1.5), "obs_irefra3": (3, True, 0, 1.5),
    "split6_irefra3": (3, False, 6, 1.5), "split5_irefra3": (3, False, 5, 1.5),
    # currents strong enough that the frequency shift of the first CTUW call leaves [0, 1] at some points; LLCFLCUROFF's second call clears them all
    "cfloff_irefra3": (3, False, 0, 8.0),
}
PLAIN = ("irefra0", "irefra1", "irefra2", "irefra3")
UNOBSTRUCTED = {"obs_irefra0": "irefra0", "obs_irefra3": "irefra3"}
KEYS = ("f3", "thdd", "thdc", "sdot", "fail1", "curmask", "fail")


def delpro_lf(name):
    return IDELPRO / 2 if CASES[name][2] else 0.0


def ranges(name):
    """the CTUWDRV calls of ctuwupdt.F90:220-256 -> [(DELPRO, MSTART, MEND)]"""
    ifm = CASES[name][2]
    return [(float(IDELPRO), 1, NFRE_RED)] if ifm <= 0 else [(float(delpro_lf(name)), 1, ifm), (float(IDELPRO), ifm + 1, NFRE_RED)]


def make_case(name, T):
    irefra, with_obs, ifm, amp = CASES[name]
    c = P.make_inputs(T, P.fixture_grid(), P.tables_of(T, NANG, NFRE, NFRE_RED, irefra), 1, 1, irefra, with_obs, IDELPRO, depth_lo=DEPTH_LO, cur_amp=amp,
                      obscor=True)
    c["wcor"] = P._f32(P.fixture_grid().wcor).astype(T)
    return c


def direction_tables(prec):
    """-> SINTH, COSTH [NANG] as MFREDIR leaves them in the working precision (mfredir.F90:124-129): the oracle's, which takes COS and SIN from the C library
    as the reference's compiler does.  numpy's single-precision COS and SIN, which ecwam_amd.tables uses, differ from them by one unit in the last place in
    a few entries; the recorded cases are the reference's own numbers, so they are fed the reference's own table."""
    from oracle.oracle import Oracle

    T = PREC[prec]
    o = Oracle(P.tables_of(T, NANG, NFRE, NFRE_RED).cfg, prec)
    return o.get("SINTH").astype(T), o.get("COSTH").astype(T)


def grid_view(c, g=None):
    """What Oracle.* and api.grid_to_device read of a grid, in the numbers of the inputs c: the tables rounded to single precision and 1 / COSPH taken in
    the working precision (ecwam_amd.grid.Grid takes it in double)."""
    g = P.fixture_grid() if g is None else g
    return types.SimpleNamespace(nsea=g.nsea, nland=g.nland, ngy=g.ngy, xdella=c["xdella"], kxlt=g.kxlt, klon=g.klon, klat=g.klat, kcor=g.kcor, zdello=c["zdello"],
                                 cosph=c["cosph"], sinph=c["sinph"], wlat=c["wlat"], wcor=c["wcor"], cosphm1_ext=c["cosphm1"])


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f"ctu_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def oracle_run(name, prec):
    """-> dict(f3 [n][K][NFRE_RED], thdd, thdc [n][K], sdot [n][K][3], fail1, curmask, fail [n][2], w: the weight arrays) of the oracle on the case's inputs,
    called as ctuwupdt.F90:207-254 and propag_wam.F90:239-313 order the routines."""
    from oracle.oracle import Oracle

    T = PREC[prec]
    irefra, with_obs, ifm, amp = CASES[name]
    c = make_case(name, T)
    v = grid_view(c)
    n, nr = v.nsea, NFRE_RED
    o = Oracle(P.tables_of(T, NANG, NFRE, nr, irefra).cfg, prec)
    o.set_obstructions(c["obs"])
    dot = o.propdot(v, irefra, c["depth"], c["u"], c["v"], c["wn"], c["cg"], c["om"])
    a = (v, irefra, c["cg"], c["om"], c["u"], c["v"], dot)
    w = None
    fail1, curmask, fail = np.zeros((n, 2), np.int8), np.ones((n, 2), T), np.zeros((n, 2), np.int8)
    for i, (dt, ms, me) in enumerate(ranges(name)):
        first = o.ctu_weights_gen(*a, dt, llcflcuroff=False, mstart=ms, mend=me)
        wi = o.ctu_weights_gen(*a, dt, llcflcuroff=True, mstart=ms, mend=me)
        fail1[:, i], curmask[:, i], fail[:, i] = first["FAIL"], wi["CURMASK"], wi["FAIL"]
        if w is None:
            w = wi
        else:      # each call writes its own frequencies only
            for k in WEIGHTS:
                w[k][:, :, ms - 1:me] = wi[k][:, :, ms - 1:me]
    step = o.propags2_gen if irefra >= 2 else o.propags2
    f3 = step(v, c["f1"], w)
    if ifm:      # the second sub-step of the fast waves: their F1 is the first sub-step's F3, frequency IFRELFMAX + 1 keeps the old time level
        f1 = c["f1"].copy()
        f1[:n, :, :ifm] = f3[:n, :, :ifm]
        f3[:n, :, :ifm] = step(v, f1, w, 1, ifm)[:n, :, :ifm]
    o.set_obstructions(None)
    return dict(f3=f3[:n, :, :nr], thdd=dot["THDD"], thdc=dot["THDC"], sdot=np.ascontiguousarray(dot["SDOT"][:, :, [m - 1 for m in SDOT_M]]),
                fail1=fail1, curmask=curmask, fail=fail, w=w)


# ---- the coverage conditions: asserted by tools/make_golden_ctu.py on what the reference computed -------------------------------------------------------------
def grid_coverage():
    """Every JXO / JYO quadrant, and a land neighbour on each longitude, latitude and corner position."""
    g = P.fixture_grid()
    t = P.tables_of(np.float64, NANG, NFRE, NFRE_RED)
    quad = sorted({(bool(s >= 0), bool(c >= 0)) for s, c in zip(t.SINTH, t.COSTH)})      # the tests of ctuwupdt.F90:124-160
    assert len(quad) == 4, quad
    land = {f"KLON{i + 1}": g.klon[:, i] for i in range(2)}
    land.update({f"KLAT{i + 1}{j + 1}": g.klat[:, i, j] for i in range(2) for j in range(2)})
    land.update({f"KCOR{i + 1}{j + 1}": g.kcor[:, i, j] for i in range(4) for j in range(2)})
    land = {k: int((a == g.nland).sum()) for k, a in land.items()}
    assert min(land.values()) >= 1, land
    return dict(points=int(g.nsea), quadrants=len(quad), land_neighbours=land)


def _zero_fraction(w):
    return {"-1": float((w[..., 0] == 0).mean()), "+1": float((w[..., 2] == 0).mean())}


def coverage(name, ref, unobstructed=None):
    """The conditions on one case: ref[prec] is what the reference returned (the keys of KEYS and the weight arrays), unobstructed[prec] the same of the case
    without obstructions -> what was observed."""
    irefra, with_obs, ifm, amp = CASES[name]
    n = ref["dp"]["f3"].shape[0]
    obs = dict(irefra=irefra, obstructions=with_obs, ifrelfmax=ifm, idelpro=IDELPRO, delpro_lf=delpro_lf(name), current_max=amp)
    for p in PREC:
        r = ref[p]
        d = {}
        assert not r["fail"].any(), name      # CTUWDRV returned
        if name in PLAIN:      # the one time step of the plain cases: nothing fails, and the largest weight of the central point is a quarter or more
            assert not r["fail1"].any(), name
            smax, smin = float(r["SUMWN"].max()), float(r["SUMWN"].min())
            assert smax >= 0.25 and 1.0 - smin >= 0.25, (name, smax, smin)
            d["sumwn_max"], d["sumwn_min"] = smax, smin
        if irefra >= 1:
            d["wkpmn_zero_fraction"] = _zero_fraction(r["WKPMN"])
            assert all(0.05 <= z <= 0.95 for z in d["wkpmn_zero_fraction"].values()), (name, d)
        if irefra >= 2:
            d["wmpmn_zero_fraction"] = _zero_fraction(r["WMPMN"])
            assert all(0.05 <= z <= 0.95 for z in d["wmpmn_zero_fraction"].values()), (name, d)
            sc = np.abs(r["sdot"]).max()
            assert sc > 0
        if unobstructed is not None:
            a, b = r["f3"], unobstructed[p]["f3"]
            assert not np.array_equal(a, b) and (a <= b).all(), name
            d["obstructed_below_open"] = float((a < b).mean())
        masked = int((r["curmask"] == 0).sum())
        if name.startswith("cfloff"):
            assert 0 < masked < n / 2 and int(r["fail1"].sum()) == masked, (name, masked)
        else:
            assert masked == 0, (name, masked)
        d["first_call_failures"], d["masked_points"] = int(r["fail1"].sum()), masked
        obs[p] = d
    return obs
