"""The host side of OUTBLOCK as one device call: the parameter table api.OUTBLOCK_PARAMS against the reference's index formulas
(outblock.F90:437-604, mpcrtbl.F90:464-469), ITOBOUT as mpcrtbl.F90:473-502 builds it, and the interface (exports, prototypes, Fortran
bindings).  No GPU."""
import os

import numpy as np
import pytest

from ecwam_amd import api, lib

NTRAIN, NTEWH = 3, 6


def _name(ir):
    return api.OUTBLOCK_PARAMS[ir - 1][1]


def test_table_follows_the_reference_formulas():
    """The formulas are written out here, not taken from the module."""
    P = api.OUTBLOCK_PARAMS
    assert api.NTRAIN == NTRAIN and api.NTEWH == NTEWH
    jppflag = 75 + 3 * NTRAIN + 5
    assert jppflag == 89 == api.JPPFLAG == len(P)
    assert [p[0] for p in P] == list(range(1, jppflag + 1))
    assert len({p[1] for p in P}) == jppflag                      # names are unique
    for itr in range(1, NTRAIN + 1):                                # EMTRAIN, THTRAIN, PMTRAIN (outblock.F90:437-449)
        assert _name(42 + 3 * (itr - 1)) == f"swh{itr}" and _name(43 + 3 * (itr - 1)) == f"mwd{itr}" and _name(44 + 3 * (itr - 1)) == f"mwp{itr}"
    assert 42 + 3 * NTRAIN == 51 and _name(51) == "strn"            # CIMSSTRN / STRNMS
    assert _name(43 + 3 * NTRAIN) == "h10" and 43 + 3 * NTRAIN == 52   # SE10MEAN
    assert (53 + 3 * NTRAIN, 54 + 3 * NTRAIN) == (62, 63) and (_name(62), _name(63)) == ("wefmag", "wefdir")
    assert [54 + 3 * NTRAIN + ih for ih in range(1, NTEWH + 1)] == list(range(64, 70))
    assert [_name(63 + ih) for ih in range(1, NTEWH + 1)] == ["h1012", "h1214", "h1417", "h1721", "h2125", "h2530"]
    b = 3 * NTRAIN + NTEWH
    assert [55 + b, 56 + b, 57 + b] == [70, 71, 72] and [_name(i) for i in (70, 71, 72)] == ["eta_m", "r", "xnslc"]
    assert [58 + b + i for i in range(5)] == [73, 74, 75, 76, 77] and _name(77) == "phiocd"
    assert [63 + b + i for i in range(4)] == [78, 79, 80, 81] and [_name(i) for i in range(78, 82)] == ["tdcmax", "tdhmax", "stcmax", "sthmax"]
    assert 67 + b == 82 and _name(82) == "sibm"                     # IBRMEMOUT
    assert (68 + b, 69 + b) == (83, 84) and (_name(83), _name(84)) == ("xwrs", "ywrs")   # TAUICX, TAUICY
    assert 70 + b == 85 and _name(85) == "ctcor"                    # CTCOR
    assert 71 + b == 86 and _name(86) == "mss_m"                    # MEANSQS at the model's cut-off
    assert [jppflag - 5 + ic for ic in range(1, 6)] == [85, 86, 87, 88, 89]    # the extra fields: 87-89 are filled by nothing
    assert api.OUTBLOCK_NUMBER["swh"] == 1 and api.OUTBLOCK_NUMBER["pp1d"] == 6


def test_masks():
    """IPRMINFO(:,6) and (:,7) as mpcrtbl.F90:92-469 sets them, restated as the sets of parameters WITHOUT the mask."""
    no_ice = {4, 5, 7, 10, 32, 37, 38, 39, 40, 41, 51, 53, 54, 55, 56, 58, 59, 60, 61, 73, 74, 75, 76, 77, 85, 86, 87, 88, 89}
    no_sea = {5, 7, 10, 53, 54, 58, 59, 60, 61, 85, 86, 87, 88, 89}
    for ir, _, ice, sea in api.OUTBLOCK_PARAMS:
        assert ice == (ir not in no_ice), ir
        assert sea == (ir not in no_sea), ir


def test_itobout_of_a_sparse_request():
    ipf, ito, n = api.outblock_tables([82, 5, 1, 44])
    assert n == 4 and ipf.dtype == np.int32 and ito.dtype == np.int32 and ipf.shape == ito.shape == (89,)
    assert {ir: int(ito[ir - 1]) for ir in (1, 5, 44, 82)} == {1: 1, 5: 2, 44: 3, 82: 4}     # in the order of the parameter numbers
    assert int(np.count_nonzero(ito)) == 4 and int(np.count_nonzero(ipf)) == 4
    ipf, ito, n = api.outblock_tables({3: 1, 20: -1, 21: 0})                                  # -1 is on the list, 0 is not
    assert n == 2 and ipf[19] == -1 and ito[19] == 2 and ito[20] == 0 and ipf[20] == 0
    ipf, ito, n = api.outblock_tables(range(1, 90))
    assert n == 89 and list(ito) == list(range(1, 90))
    with pytest.raises(ValueError):
        api.outblock_tables([90])


def test_interface():
    names = ("ecwam_hip_set_outblock", "ecwam_hip_outblock_plan", "ecwam_hip_outblock")
    for name in names:
        assert name in lib.EXPORTS
    assert lib.ABI_VERSION == 6
    root = os.path.join(lib.HERE, "..")
    header = open(os.path.join(root, "include", "ecwam_hip.h")).read()
    for name, nargs in zip(names, (8, 3, 19)):
        proto = header[header.index(f"int {name}("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == nargs, (name, proto)
    fortran = open(os.path.join(lib.HERE, "fortran", "ecwam_hip_capi.F90")).read()
    for name in names:
        assert f"NAME='{name}'" in fortran
    from ecwam_amd import build

    assert "outblock.hip" in build.SOURCES
    assert len(api.OUTBLOCK_CALLS) == 7
    for m in ("set_outblock", "outblock", "outblock_plan"):
        assert callable(getattr(api.HipContext, m))
    from ecwam_amd.wamintgr import Wamintgr

    assert callable(Wamintgr.outblock)
