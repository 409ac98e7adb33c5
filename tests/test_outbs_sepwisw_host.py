"""Wind sea / swell separation and the mean-period / spread parameters of OUTBLOCK (ecwam_hip_outbs_sepwisw): the C ABI declares and
exports the entry point, and the numpy restatement the GPU tests check the kernel against (tests/sepwisw_ref.py) gives the hand results
of spectra whose answer is known.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import harness as H
import sepwisw_ref as S
from ecwam_amd.tables import Config, Tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {f: i for i, f in enumerate(S.FIELDS)}
DEG = 57.295778667    # yowpcons.F90:31


def test_entry_point_is_declared_and_exported():
    from ecwam_amd import api, build, lib

    hdr = open(os.path.join(ROOT, "include", "ecwam_hip.h")).read()
    assert re.search(r"\bint ecwam_hip_outbs_sepwisw\s*\(", hdr)
    assert "ecwam_hip_outbs_sepwisw" in lib.EXPORTS
    assert api.OUTBS_SEP_FIELDS == S.FIELDS
    build.build()
    assert lib.load().ecwam_hip_outbs_sepwisw is not None
    ftn = open(os.path.join(ROOT, "ecwam_amd", "fortran", "ecwam_hip_capi.F90")).read()
    assert "NAME='ecwam_hip_outbs_sepwisw'" in ftn


def _hand_femean(t, f):
    """EM, FM of FEMEAN in double precision without the EPSMIN floors."""
    f = np.asarray(f, np.float64)
    fr, dfim, delth = (np.asarray(x, np.float64) for x in (t.FR, t.DFIM, t.DELTH))
    s = f.sum(-2)                                                   # [.., M]
    em = (s * dfim).sum(-1) + float(t.WETAIL) * fr[-1] * delth * s[..., -1]
    fm = (s * dfim / fr).sum(-1) + float(t.FRTAIL) * delth * s[..., -1]
    return em, em / fm


def known_answer_checks(t, names, fl1, out, extra):
    """The hand results of sepwisw_ref.known_answer_inputs (shared with the device test)."""
    sp = t.dtype == np.float32
    rt = 2e-6 if sp else 1e-12
    o = {nm: out[i].astype(np.float64) for i, nm in enumerate(names)}
    nang = len(t.TH)
    # every XLLWS = 1: the swell part is the EPSMIN floor, the sea part the whole spectrum
    em, fm = _hand_femean(t, fl1[names.index("allsea")])
    floor = float(t.EPSMIN) * nang * (np.sum(np.asarray(t.DFIM, np.float64)) + float(t.WETAIL) * float(t.FR[-1]) * float(t.DELTH))
    a = o["allsea"]
    assert abs(a[COL["shts"]] - 4 * np.sqrt(floor)) < 1e-5 * 4 * np.sqrt(floor), a
    assert abs(a[COL["shww"]] - 4 * np.sqrt(em)) < rt * 4 * np.sqrt(em), (a[COL["shww"]], 4 * np.sqrt(em))
    assert abs(a[COL["mpww"]] - 1 / fm) < rt * (1 / fm)
    assert a[COL["p1swell"]] == 0 and a[COL["p2swell"]] == 0 and a[COL["sprdswell"]] == 0
    # XLLWS = 0 with UFRIC = 0: all swell, the wind-sea direction is WDWAVE (Fortran MOD: the sign of the dividend)
    for nm in names:
        if nm.startswith("allswell"):
            a, wd = o[nm], float(nm[len("allswell"):])
            want = np.fmod(DEG * wd + 180.0, 360.0)
            assert abs(a[COL["mdww"]] - want) < (1e-4 if sp else 1e-9), (nm, a[COL["mdww"]], want)
            assert abs(a[COL["shts"]] - 4 * np.sqrt(em)) < rt * 4 * np.sqrt(em) and a[COL["shww"]] < 1e-10
            assert abs(a[COL["mpts"]] - 1 / fm) < rt * (1 / fm)
    # one bin (K 5, M 9 < NFRE_ODD): both mean periods are 1 / FR(M), the spread is 0 to the square root of the rounding of 1 - x
    a = o["onebin"]
    p = 1.0 / float(t.FR[9])
    assert abs(a[COL["mp1"]] - p) < 4 * rt * p and abs(a[COL["mp2"]] - p) < 4 * rt * p, a
    assert a[COL["wdw"]] < (1e-3 if sp else 1e-7)
    # an isotropic single frequency: spread SQRT(2)
    assert abs(o["iso"][COL["wdw"]] - np.sqrt(2.0)) < (1e-5 if sp else 1e-10)
    # two systems: the swell against the wind at low frequency, the wind sea along it at high frequency, each within a bin
    a = o["twosys"]
    wd = float(extra["wd_sea"])
    dbin = float(np.degrees(float(t.DELTH)))
    for col, th in (("mdww", wd), ("mdts", wd + np.pi)):
        d = abs(a[COL[col]] - np.fmod(DEG * th + 180.0, 360.0)) % 360.0
        assert min(d, 360.0 - d) < dbin, (col, a[COL[col]])
    for col, part in (("mpww", "sea"), ("mpts", "swell")):
        _, fmp = _hand_femean(t, extra[part])
        assert abs(a[COL[col]] * fmp - 1.0) < float(t.FR[1] / t.FR[0]) - 1.0, (col, a[COL[col]], 1 / fmp)
    assert a[COL["shts"]] > a[COL["shww"]] > 0


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_restatement_known_answers(prec):
    t = Tables(Config(nang=36, nfre=36, nfre_red=36), H.np_dtype(prec))
    names, fl1, xl, cinv, uf, wd, extra = S.known_answer_inputs(t)
    out, info = S.sepwisw(t, fl1, xl, cinv, uf, wd)
    assert not info["near"].any()
    known_answer_checks(t, names, fl1, out, extra)


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_restatement_heights_add_up_to_the_total(prec):
    """shww**2 + shts**2 = swh**2 (the EM of FEMEAN): the two parts split the spectrum, the EPSMIN floors are negligible."""
    cfg = Config(nang=36, nfre=36, nfre_red=36)
    case = H.make_point_case(400, cfg, prec, spectra="mixed", seed=5)
    t = case["tables"]
    wv, ff, _ = H.pack_device_inputs(case)
    xl = S.synthetic_xllws(t, ff[:, 1], 0.15)
    out, _ = S.sepwisw(t, case["FL1"], xl, wv[:, 2], ff[:, 7], ff[:, 1])
    em, _ = S._femean(t, case["FL1"])
    swh2 = 16.0 * em.astype(np.float64)
    o = out.astype(np.float64)
    rel = np.abs(o[:, 3] ** 2 + o[:, 4] ** 2 - swh2) / swh2
    assert rel.max() < (2e-6 if prec == "sp" else 1e-12), rel.max()
    assert (o[:, 3] > 1e-3).mean() > 0.5 and (o[:, 4] > 1e-3).mean() > 0.5      # both parts present at most points
