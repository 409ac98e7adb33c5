"""The corner-transport path with refraction and sub-grid obstructions without a GPU: the fixtures tests/golden/ctu_*.npz -- what the reference's own unmodified
PROPDOT / GRADI, CTUWINI, CTUWDRV / CTUW and PROPAGS2 returned behind tools/ctu_driver.F90 -- and the oracle (Oracle.propdot, ctu_weights_gen, propags2 /
propags2_gen, set_obstructions) against them: THE SAME BITS, in both precisions.  These routines hold only correctly rounded operations in a fixed order and
the reference is built without contraction, so nothing less is expected; the weights themselves, too large to commit, were compared array by array when the
fixtures were written (ctu_observed.json).  Nothing here comes from the device."""
import json
import os

import numpy as np
import pytest

import ctu_ref as CT
import propags_ref as P


def _observed():
    with open(os.path.join(CT.GOLDEN, "ctu_observed.json")) as fh:
        return json.load(fh)


def test_the_fixtures_are_the_cases_of_the_issue_and_small():
    files = sorted(f for f in os.listdir(CT.GOLDEN) if f.startswith("ctu_"))
    assert files == sorted([f"ctu_{n}.npz" for n in CT.CASES] + ["ctu_observed.json"])
    for f in files:
        assert os.path.getsize(os.path.join(CT.GOLDEN, f)) <= 600_000, f
    c = CT.CASES
    assert {v[0] for k, v in c.items() if k in CT.PLAIN} == {0, 1, 2, 3} and all(c[k][1:] == (False, 0, 1.5) for k in CT.PLAIN)
    assert {v[0] for v in c.values() if v[1]} == {0, 3}                                      # obstructions at IREFRA 0 and 3
    assert sorted(v[2] for v in c.values() if v[2]) == [5, 6] and all(v[0] == 3 for v in c.values() if v[2])      # an odd and an even IFRELFMAX
    assert [k for k, v in c.items() if v[3] != 1.5] == ["cfloff_irefra3"]
    g = P.fixture_grid()
    assert g.nsea == 61 and (CT.NANG, CT.NFRE, CT.NFRE_RED) == (12, 36, 26) and CT.NFRE_RED % 2 == 0 and CT.IDELPRO % 2 == 0
    assert _observed()["idelpro"] == CT.IDELPRO


def test_the_grid_covers_what_it_claims():
    assert CT.grid_coverage() == _observed()["grid"]


@pytest.mark.parametrize("prec", ["sp", "dp"])
@pytest.mark.parametrize("name", list(CT.CASES))
def test_the_oracle_reproduces_the_reference_bit_for_bit(name, prec):
    """F3, the dot terms, the flags of the first CTUW call, CURMASK and the final flags: the same bits.  The record of the weights says the same of every
    weight array, and the coverage the tool observed on the reference holds on the committed arrays where they show it."""
    T = CT.PREC[prec]
    fx = CT.load_fixture(name)
    assert set(fx) == {f"{k}_{p}" for p in CT.PREC for k in CT.KEYS}
    n = P.fixture_grid().nsea
    shapes = dict(f3=(n, CT.NANG, CT.NFRE_RED), thdd=(n, CT.NANG), thdc=(n, CT.NANG), sdot=(n, CT.NANG, len(CT.SDOT_M)), fail1=(n, 2), curmask=(n, 2), fail=(n, 2))
    for k, shp in shapes.items():
        assert fx[f"{k}_{prec}"].shape == shp and fx[f"{k}_{prec}"].dtype == (np.int8 if k.startswith("fail") else T), k
    o = CT.oracle_run(name, prec)
    for k in CT.KEYS:
        got, want = o[k], fx[f"{k}_{prec}"]
        assert P.same_bits(got, want), (k, "differing elements:", int((got != want).sum()), "largest difference:",
                                        float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
    obs = _observed()["cases"][name][prec]
    assert set(obs["oracle_bit_identical"]) == set(CT.WEIGHTS + ("WLAT", "WCOR") + CT.KEYS) and all(obs["oracle_bit_identical"].values())
    # what the committed arrays themselves show of the coverage
    irefra, with_obs, ifm, amp = CT.CASES[name]
    assert not fx[f"fail_{prec}"].any()
    masked = int((fx[f"curmask_{prec}"] == 0).sum())
    assert masked == obs["masked_points"] == int(fx[f"fail1_{prec}"].sum())
    assert (0 < masked < n / 2) if name.startswith("cfloff") else masked == 0
    for k, on in (("thdd", irefra in (1, 3)), ("thdc", irefra >= 2), ("sdot", irefra >= 2)):      # a term the case has is there; one it has not is zero
        assert (np.abs(fx[f"{k}_{prec}"]).reshape(n * CT.NANG, -1).max(axis=0) > 0).all() if on else not fx[f"{k}_{prec}"].any(), k
    if name in CT.UNOBSTRUCTED:
        open_ = CT.load_fixture(CT.UNOBSTRUCTED[name])[f"f3_{prec}"]
        assert (fx[f"f3_{prec}"] <= open_).all() and float((fx[f"f3_{prec}"] < open_).mean()) == obs["obstructed_below_open"]
    if name in CT.PLAIN:
        assert obs["sumwn_max"] >= 0.25


def test_the_time_step_matters():
    """The recorded F3 of the plain case differs from F1 by far more than any tolerance a test grants: the weights are not small."""
    fx = CT.load_fixture("irefra0")
    c = CT.make_case("irefra0", np.float64)
    n = fx["f3_dp"].shape[0]
    assert np.abs(fx["f3_dp"] - c["f1"][:n, :, :CT.NFRE_RED]).max() > 0.05
