"""The configurations and sea states of the reference fixtures (tests/golden/reference_*.npz), shared by their generator
(tools/make_golden_reference.py) and by the tests that read them (test_reference_pin.py on the CPU, test_gpu_reference_pin.py on the device).

Every input is float32-representable, so that the single and the double precision builds of the reference, of the oracle and of the device
see the same numbers; the wave-property columns (WVPRPT) are inputs like the spectra -- all three sides are handed the same ones.  The sea
states are those of harness.make_point_case with the modifications of the existing GPU parity tests (tests/test_gpu_parity.py) they stand for.

Point counts: the smallest that fill whole wavefronts of k_implsch4 and leave a remainder -- the kernel carries 2 / 3 / 5 / 10 points per
wavefront at 48 / 36 / 24 / 12 directions (ecwam_amd/csrc/implsch_v4.h:3): 25 at 48 (12 waves + 1), 26 at 36 (8 + 2), 29 at 24 (5 + 4), 64 at 12
(6 + 4) -- and that keep every fixture under the size limit of a committed file and all of them together near 6 MB (64 points at 24 directions,
ten configurations, would add 3 MB).
"""
from __future__ import annotations

import json
import os

import numpy as np

import harness as H
from ecwam_amd import synthetic as syn
from ecwam_amd.tables import Config, Tables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = dict(llgcbz0=True, llnormagam=True)
_24 = dict(nang=24, nfre_red=29)
N_BY_NANG = {48: 25, 36: 26, 24: 29, 12: 64}

# name -> cfg: Config keywords (nfre = 36 everywhere); sea: the sea state; what: the routine; w2n: WAVE2OCEAN columns are inputs and outputs;
# seed: of the fixture (the live test of test_reference_pin.py uses seed + 1000)
CONFIGS = {
    "A36_450": dict(cfg=dict(nang=36, nfre_red=36, idelt=450, idelpro=450), seed=31),
    "B36_450": dict(cfg=dict(nang=36, nfre_red=36, idelt=450, idelpro=450, **B), seed=31),
    "A24x29": dict(cfg=dict(**_24), seed=777),
    "A12x25": dict(cfg=dict(nang=12, nfre_red=25), seed=777),
    "A24x25": dict(cfg=dict(nang=24, nfre_red=25), seed=777),
    "A48x36": dict(cfg=dict(nang=48, nfre_red=36), seed=43),
    "iphys0_12x25": dict(cfg=dict(nang=12, nfre_red=25, iphys=0), seed=61),
    "isnonlin1": dict(cfg=dict(isnonlin=1, **_24), seed=51, sea="depths"),
    "isnonlin2": dict(cfg=dict(isnonlin=2, **_24), seed=51, sea="depths"),
    "ice_ciwa1_3_scal": dict(cfg=dict(lciwa1=True, lciwa3=True, lciscal=True, **_24), seed=21, sea="ice"),
    "ice_ciwa2_nomask": dict(cfg=dict(lciwa2=True, lmaskice=False, **_24), seed=21, sea="ice"),
    "ice_breakup_nemo": dict(cfg=dict(lciwa1=True, lciwa3=True, lciscal=True, lwnemocou=True, lwnemocouibr=True, zalpfacx=2.0, zalpfacb=0.7, **_24),
                             seed=21, sea="ice", w2n=True),
    "icode1": dict(cfg=dict(icode=1, **_24), seed=61, sea="stale_wind"),
    "icode2": dict(cfg=dict(icode=2, **_24), seed=61, sea="stale_wind"),
    "edge": dict(cfg=dict(**_24), seed=3, sea="edge", n=64),
    "wdfluxes_A36": dict(cfg=dict(nang=36, nfre_red=36), seed=12345, what="wdfluxes"),
}


# advection: the smallest "continents" grid of ecwam_amd.grid with land, both polar rows and the periodic seam (34 sea points on two rows)
ADV_NOCT = 2
ADV_IFRELFMAX = 12


def advection_config() -> Config:
    return Config(nang=12, nfre=36, nfre_red=25, idelpro=900)


def fused_config() -> Config:
    return Config(nang=36, nfre=36, nfre_red=36, idelt=450, idelpro=450)


def w8(t, w):
    """The eight weights PROPAGS2 reads out of the reference-shaped weight arrays, [ij][8][K][M]: the device's layout
    (tests/test_gpu_parity.py::test_ctuw_and_propags2_parity)."""
    jx, jy, K = np.asarray(t.JXO)[:, 0] - 1, np.asarray(t.JYO)[:, 0] - 1, np.arange(len(t.JXO))
    sel = [w["SUMWN"], w["WLONN"][:, K, :, jx].transpose(1, 0, 2), w["WLATN"][:, K, :, jy, 0].transpose(1, 0, 2),
           w["WLATN"][:, K, :, jy, 1].transpose(1, 0, 2), w["WCORN"][:, :, :, 0, 0], w["WCORN"][:, :, :, 0, 1], w["WKPMN"][:, :, :, 0],
           w["WKPMN"][:, :, :, 2]]
    return np.stack(sel, 1)


def config(name: str) -> Config:
    return Config(nfre=36, **CONFIGS[name]["cfg"])


def points(name: str) -> int:
    return CONFIGS[name].get("n", N_BY_NANG[CONFIGS[name]["cfg"]["nang"]])


def kind(name: str) -> str:
    return CONFIGS[name].get("what", "implsch")


def make_inputs(name: str, n: int, seed: int) -> dict:
    """n candidate points of a configuration, float32: FL1 [n][NANG][NFRE], WV [n][5][NFRE] (WAVNUM CGROUP CINV XK2CG STOKFAC), ENV [n][2]
    (EMAXDPT DEPTH), FF [n][14], INTF [n][15], and where the configuration reads them W2N [n][13] and IBRMEM [n]."""
    spec = CONFIGS[name]
    cfg = config(name)
    sea = spec.get("sea", "mixed")
    dt = np.float32
    case = H.make_point_case(n, cfg, "sp", seed=seed, spectra="jonswap" if sea == "edge" else "mixed")
    t = case["tables"]
    rng = np.random.default_rng(seed + 5)

    def new_depths(depth):
        case["ENV"][:, 1] = depth.astype(dt)
        case["props"] = syn.depth_props(case["ENV"][:, 1], t, dt)
        case["ENV"][:, 0] = case["props"]["EMAXDPT"]

    if sea == "depths":          # test_implsch_parity_isnonlin_1_2: many intermediate-depth points, 4 m .. 316 m
        new_depths(10.0 ** rng.uniform(0.6, 2.5, n))
    elif sea == "ice":           # test_gpu_parity._ice_case: partial cover, thickness beyond both table ends, broken / solid ice
        case["FF"][:, 2] = np.where(rng.uniform(size=n) < 0.6, rng.uniform(0.0, 1.0, n), 0.0).astype(dt)
        cith = rng.uniform(0.0, 4.2, n)
        cith[rng.uniform(size=n) < 0.1] = 0.0
        case["FF"][:, 13] = cith.astype(dt)
        case["IBRMEM"] = np.where(rng.uniform(size=n) < 0.5, 0.0, 1.0).astype(dt)
    elif sea == "stale_wind":    # test_implsch_parity_friction_velocity_forcing: WSWAVE is an output, only CHNKMIN reads the stale one
        case["FF"][:, 3] = dt(7.0)
    elif sea == "edge":          # test_implsch_edge_cases: ice across CITHRSH, SDIWBK / SBOTTOM depths, noise-floor and huge spectra, calm and storm
        assert n >= 28
        case["FF"][:8, 2] = np.linspace(0.25, 1.0, 8)
        depth = case["ENV"][:, 1].copy()
        depth[8:16] = np.array([2, 3, 5, 8, 12, 20, 35, 49.9], dt)
        new_depths(depth)
        case["FL1"][16:20] = dt(1e-33)
        case["FL1"][20:24] *= dt(50.0)
        case["FF"][24:28, 3] = np.array([1.0, 1.5, 3.9, 39.0], dt)
    pr = case["props"]
    inp = dict(FL1=case["FL1"].astype(dt), WV=np.stack([pr[k] for k in ("WAVNUM", "CGROUP", "CINV", "XK2CG", "STOKFAC")], 1).astype(dt),
               ENV=case["ENV"].astype(dt), FF=case["FF"].astype(dt), INTF=case["INTF"].astype(dt))
    if spec.get("w2n"):
        inp["W2N"] = rng.uniform(-1.0, 1.0, (n, 13)).astype(dt)
    if "IBRMEM" in case:
        inp["IBRMEM"] = case["IBRMEM"].astype(dt)
    return inp


def select(inp: dict, idx) -> dict:
    return {k: np.ascontiguousarray(v[idx]) for k, v in inp.items()}


def run(engine, inp: dict, what: str = "implsch") -> dict:
    """IMPLSCH or WDFLUXES of the inputs through an engine with the call shape of oracle.oracle.Oracle (the oracle, the reference, or
    tests/wdfluxes_ref.py's oracle for WDFLUXES); the engine converts to its own precision."""
    wv = inp["WV"]
    w2n = None if "W2N" not in inp else inp["W2N"].astype(np.float64)
    f = engine.implsch if what == "implsch" else engine.wdfluxes
    return f(inp["FL1"], wv[:, 0], wv[:, 1], wv[:, 2], wv[:, 3], wv[:, 4], inp["ENV"], inp["FF"], inp["INTF"], w2n=w2n, ibrmem=inp.get("IBRMEM"))


def harness_case(name: str, inp: dict, prec: str) -> dict:
    """The inputs as a case of tests/harness.py (gpu_implsch, pack_device_inputs) in the precision asked for."""
    dt = H.np_dtype(prec)
    cfg = config(name)
    wv = inp["WV"].astype(dt)
    case = dict(cfg=cfg, prec=prec, tables=Tables(cfg, dt), n=inp["FL1"].shape[0], FL1=inp["FL1"].astype(dt),
                props={k: np.ascontiguousarray(wv[:, i]) for i, k in enumerate(("WAVNUM", "CGROUP", "CINV", "XK2CG", "STOKFAC"))},
                FF=inp["FF"].astype(dt), INTF=inp["INTF"].astype(dt), ENV=inp["ENV"].astype(dt))
    if "W2N" in inp:
        case["W2N"] = inp["W2N"].astype(np.float64)
    if "IBRMEM" in inp:
        case["IBRMEM"] = inp["IBRMEM"].astype(dt)
    return case


# ---- the fixture files ------------------------------------------------------------------------------------------------------------------
_INPUTS = ("FL1", "WV", "ENV", "FF", "INTF", "W2N", "IBRMEM")


def path(name: str) -> str:
    return os.path.join(GOLDEN, f"reference_{name}.npz")


def save(name: str, inp: dict, out: dict, dropped: float) -> str:
    """out: {"dp": result, "sp": result} of the reference.  MIJ and XLLWS are the same in both (the generator dropped the other points)."""
    d = {"in_" + k: v for k, v in inp.items()}
    assert np.array_equal(out["dp"]["MIJ"], out["sp"]["MIJ"]) and np.array_equal(out["dp"]["XLLWS"], out["sp"]["XLLWS"])
    xl = out["dp"]["XLLWS"]
    assert np.isin(xl, (0.0, 1.0)).all()
    d["MIJ"] = out["dp"]["MIJ"].astype(np.int32)
    d["XLLWS"] = xl.astype(np.uint8)
    for p, T in (("dp", np.float64), ("sp", np.float32)):
        if kind(name) == "implsch":      # (WDFLUXES leaves the spectrum as it is)
            d[f"FL1_{p}"] = out[p]["FL1"].astype(T)
        d[f"FF_{p}"] = out[p]["FF"].astype(T)
        d[f"INTF_{p}"] = out[p]["INTF"].astype(T)
        if "W2N" in out[p]:
            d[f"W2N_{p}"] = out[p]["W2N"].astype(np.float64)      # WAVE2OCEAN is double precision in both builds
    d["meta"] = np.array(json.dumps(dict(name=name, cfg=CONFIGS[name]["cfg"], what=kind(name), dropped=dropped)))
    np.savez_compressed(path(name), **d)
    return path(name)


def load(name: str):
    """(inputs, {"dp": reference result, "sp": reference result}) of a fixture."""
    z = np.load(path(name))
    meta = json.loads(str(z["meta"]))
    assert meta["cfg"] == json.loads(json.dumps(CONFIGS[name]["cfg"])), "the fixture was generated for another configuration: regenerate it"
    inp = {k: z["in_" + k] for k in _INPUTS if "in_" + k in z.files}
    out = {}
    for p, T in (("dp", np.float64), ("sp", np.float32)):
        r = dict(MIJ=z["MIJ"], XLLWS=z["XLLWS"].astype(T), FF=z[f"FF_{p}"], INTF=z[f"INTF_{p}"])
        r["FL1"] = z[f"FL1_{p}"] if f"FL1_{p}" in z.files else inp["FL1"].astype(T)
        if f"W2N_{p}" in z.files:
            r["W2N"] = z[f"W2N_{p}"]
        out[p] = r
    return inp, out


# ---- NEWWIND and DEPTHPRPT: small fixtures of their own (reference_newwind.npz, reference_depthprpt.npz) ------------------------------------
NEWWIND_ICODES = (3, 1, 2)
NEWWIND_N = 67
DEPTHPRPT_KEYS = ("WAVNUM", "CINV", "CGROUP", "XK2CG", "OMOSNH2KD", "STOKFAC", "EMAXDPT")


def newwind_config(icode: int) -> Config:
    return Config(nang=12, nfre=36, nfre_red=25, icode=icode)


def newwind_inputs(seed: int = 1):
    """FF_NOW, FF_NEXT [n][14], float32: wind speeds on both sides of WSPMIN_RESET_TAUW = 4 m/s (ICODE 3), friction velocities on both sides of
    USTMIN_RESET_TAUW = 0.08 m/s (ICODE 1 / 2), a TAUW above and below the cap, CHRNCK in the range the Charnock relation gives."""
    rng = np.random.default_rng(seed)
    n = NEWWIND_N
    ff = rng.uniform(0.05, 5.0, (n, 14))
    ffn = rng.uniform(0.05, 8.0, (n, 14))
    ffn[:, 3] = rng.uniform(0.5, 12.0, n)          # WSWAVE of FF_NEXT: below and above 4
    ffn[:4, 3] = [3.999, 4.0, 4.001, 0.3]
    ff[:, 8] = rng.uniform(0.0, 0.2, n)            # TAUW: above and below the cap WGHT (ACD + BCD U) U^3
    ffn[:, 7] = rng.uniform(0.02, 1.2, n)          # UFRIC of FF_NEXT: below and above 0.08
    ffn[:4, 7] = [0.0799, 0.08, 0.0801, 0.02]
    ff[:, 12] = rng.uniform(0.008, 0.03, n)        # CHRNCK
    return ff.astype(np.float32), ffn.astype(np.float32)


def depthprpt_depths(seed: int = 11):
    """Depths over the whole range, float32, with the branch points of DEPTHPRPT / AKI (the deep-water switch at k d = 10, BATHYMAX)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([10 ** rng.uniform(0.0, 3.0, 64), [998.999, 1.0, 2.5, 7.0, 50.0, 49.999]]).astype(np.float32)


# ---- gates of the oracle (and of a live reference) against the fixtures, shared by tests/test_reference_pin.py and tools/reference_pin_report.py
CEILING = dict(bins=1e-10, swh=1e-10, ff=1e-10, intf=1e-8, w2n=1e-10)      # the device's dp gates against the oracle
DP_ZERO_FLOOR = 8 * np.finfo(np.float64).eps      # asserted only where the observed figure is exactly 0: a few units in the last place of the compared (relative) quantity
OBSERVED = os.path.join(GOLDEN, "reference_pin_observed.json")
_OBS = {}


def observed() -> dict:
    if not _OBS:
        with open(OBSERVED) as fh:
            _OBS.update(json.load(fh))
    return _OBS


def dp_gate_of(obs: float, q: str) -> float:
    """10 x the observed maximum, never looser than the ceiling; where the observed figure is exactly 0 (the oracle reproduces the reference's
    bits on that quantity) 10 x 0 would demand the same bits of another libm: there, and only there, DP_ZERO_FLOOR."""
    return min(CEILING[q], 10.0 * obs if obs > 0.0 else DP_ZERO_FLOOR)


def dp_gate(name: str, q: str) -> float:
    return dp_gate_of(float(observed()[name][q]), q)


def stats(name: str, ref: dict, got: dict, prec: str) -> dict:
    """harness.compare_implsch + the WAVE2OCEAN columns relative to each column's scale."""
    st = H.compare_implsch(ref, got, Tables(config(name), H.np_dtype(prec)))
    st["w2n_max_rel"] = 0.0
    if "W2N" in ref:
        scale = np.maximum(np.abs(ref["W2N"]).max(axis=0, keepdims=True), 1e-12)
        st["w2n_max_rel"] = float(np.max(np.abs(got["W2N"] - ref["W2N"]) / scale))
    return st


def figures(st: dict) -> dict:
    return dict(bins=st["fl1_max_rel_peak_all"], swh=st["swh_max_rel"], ff=st["ff_max_rel_all"], intf=st["intf_max_rel_all"], w2n=st["w2n_max_rel"])


_ORACLES = {}


def oracle_for(name: str, prec: str):
    """One oracle per configuration and precision, shared (WDFLUXES: the oracle's routines under tests/wdfluxes_ref.py's driver)."""
    key = (name, prec)
    if key not in _ORACLES:
        cfg = config(name)
        if kind(name) == "wdfluxes":
            import wdfluxes_ref as W

            _ORACLES[key] = W.WdfluxesOracle(cfg, prec)
        else:
            from oracle.oracle import Oracle

            _ORACLES[key] = Oracle(cfg, prec)
    return _ORACLES[key]
