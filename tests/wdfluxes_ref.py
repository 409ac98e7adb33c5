"""CPU reference of WDFLUXES and SETICE (tests/csrc/wdfluxes_ref.c: the oracle's own routines under the driver of wdfluxes.F90:156-306)
and the oracle-free known answers the host and the GPU tests apply to a WDFLUXES result.  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

import oracle.oracle as _ora

HERE = os.path.dirname(os.path.abspath(__file__))
ORA = os.path.dirname(os.path.abspath(_ora.__file__))
CSRC = os.path.join(HERE, "csrc")
SRC = os.path.join(CSRC, "wdfluxes_ref.c")


def _cflags() -> list:
    """CFLAGS of oracle/Makefile (the bit-reproducible build: no contraction, no fast math)."""
    with open(os.path.join(ORA, "Makefile")) as fh:
        m = re.search(r"^CFLAGS \?= (.*)$", fh.read(), re.M)
    return m.group(1).split()


def lib_path(prec: str) -> str:
    return os.path.join(CSRC, f"libwdfl_{prec}.so")


def build(force: bool = False) -> None:
    deps = [SRC] + [os.path.join(ORA, f) for f in ("ora_implsch.c", "ora_implsch_blk.inc", "ora_tables.c", "ora_propag.c", "ora.h", "Makefile")]
    newest = max(os.path.getmtime(d) for d in deps)
    for prec in ("sp", "dp"):
        out = lib_path(prec)
        if not force and os.path.exists(out) and os.path.getmtime(out) > newest:
            continue
        # (the oracle's file-local routines this driver does not call are unused here: no warning for them)
        cmd = ["gcc", *_cflags(), "-Wno-unused-function", *(["-DORA_SINGLE"] if prec == "sp" else []), "-I", ORA, "-shared", "-o", out + ".tmp", SRC,
               os.path.join(ORA, "ora_tables.c"), os.path.join(ORA, "ora_propag.c"), "-lmvec", "-lm"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"gcc failed for {SRC}:\n{r.stdout}")
        os.replace(out + ".tmp", out)


class WdfluxesOracle(_ora.Oracle):
    """The oracle with ora_wdfluxes and ora_setice_pts: the same sources in one library of the tests' own."""

    def __init__(self, cfg, precision: str = "dp"):
        build()
        super().__init__(cfg, precision)

    def _fresh_copy(self, path: str) -> None:      # (path: the oracle's library of this precision; this class loads its own)
        tmp = tempfile.NamedTemporaryFile(prefix="libwdfl_", suffix=".so", delete=False)
        tmp.close()
        shutil.copy(lib_path(self.precision), tmp.name)
        self.lib = C.CDLL(tmp.name, mode=os.RTLD_LOCAL)
        os.unlink(tmp.name)

    def wdfluxes(self, fl1, wavnum, cgroup, cinv, xk2cg, stokfac, env, ff, intf, w2n=None, ibrmem=None):
        """Returns dict(FL1, FF: the arrays handed to the C routine, as it left them; XLLWS, MIJ, INTF[, W2N])."""
        n = fl1.shape[0]
        T = self.dtype
        fl1 = np.array(fl1, dtype=T, order="C")
        ff = np.array(ff, dtype=T, order="C")
        intf = np.array(intf, dtype=T, order="C")
        xllws = np.zeros_like(fl1)
        mij = np.zeros(n, dtype=np.int32)
        a = [np.ascontiguousarray(x, dtype=T) for x in (wavnum, cgroup, cinv, xk2cg, stokfac, env)]
        ib = None if ibrmem is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ibrmem, dtype=T), (n,)))
        if w2n is not None:
            w2n = np.array(w2n, dtype=np.float64, order="C")
            assert w2n.shape == (n, 13)
        self.lib.ora_wdfluxes.restype = C.c_int
        rc = self.lib.ora_wdfluxes(C.c_int(n), self._p(fl1), *(self._p(x) for x in a), self._p(ff), self._p(intf), self._p(mij), self._p(xllws),
                                   None if w2n is None else w2n.ctypes.data_as(C.c_void_p), None if ib is None else self._p(ib))
        if rc:
            raise RuntimeError(f"ora_wdfluxes abort branch rc={rc}")
        out = dict(FL1=fl1, FF=ff, XLLWS=xllws, MIJ=mij, INTF=intf)
        if w2n is not None:
            out["W2N"] = w2n
        return out

    def setice(self, fl1, ff):
        fl1 = np.array(fl1, dtype=self.dtype, order="C")
        ff = np.ascontiguousarray(ff, dtype=self.dtype)
        assert ff.shape[1] == 14
        self.lib.ora_setice_pts(C.c_int(fl1.shape[0]), self._p(fl1), self._p(ff))
        return fl1


def reference(case: dict, oracle: WdfluxesOracle) -> dict:
    """WDFLUXES of a harness case on the oracle's OWN wave-property tables, as harness.oracle_implsch feeds IMPLSCH."""
    depth = np.ascontiguousarray(case["ENV"][:, 1])
    pr = oracle.depthprpt(depth)
    env = np.stack([pr["EMAXDPT"], depth], 1).astype(case["ENV"].dtype)
    return oracle.wdfluxes(case["FL1"], pr["WAVNUM"], pr["CGROUP"], pr["CINV"], pr["XK2CG"], pr["STOKFAC"], env, case["FF"], case["INTF"],
                           w2n=case.get("W2N"), ibrmem=case.get("IBRMEM"))


# ---- oracle-free known answers (numpy, double precision, from the module tables of ecwam_amd.tables and the inputs alone)
def stokes_known(t, fl1, stokfac, ff):
    """USTOKES, VSTOKES by stokesdrift.F90:89-142 (no LWAMRSETCI reset: callers pass ice-free points or a configuration without it)."""
    f = np.asarray(fl1, np.float64)
    mo = int(t.NFRE_ODD)
    w = np.asarray(stokfac, np.float64)[:, :mo] * np.asarray(t.DFIM_SIM, np.float64)[None, :mo]
    fo = float(t.FR[mo - 1])
    const = 2.0 * float(t.DELTH) * float(t.ZPI) ** 3 / float(t.G) * fo ** 4
    s, c = np.asarray(t.SINTH, np.float64), np.asarray(t.COSTH, np.float64)
    a = np.einsum("nkm,nm->nk", f[:, :, :mo], w) + const * f[:, :, mo - 1]
    return np.clip(a @ s, -1.5, 1.5), np.clip(a @ c, -1.5, 1.5)


def wsemean_known(t, fl1, xllws):
    """WSEMEAN, WSFMEAN by femeanws.F90:84-123 and the WSEMEAN_MIN branch of wdfluxes.F90:288-300."""
    f = np.asarray(fl1, np.float64) * (np.asarray(xllws, np.float64) != 0)
    tot = f.sum(1)      # [n][M]
    dfim, dfimofr = np.asarray(t.DFIM, np.float64), np.asarray(t.DFIMOFR, np.float64)
    frl = float(t.FR[-1])
    delt25 = float(t.WETAIL) * frl * float(t.DELTH)
    delt2 = float(t.FRTAIL) * float(t.DELTH)
    em = float(t.EPSMIN) + tot @ dfim + delt25 * tot[:, -1]
    fm = em / (float(t.EPSMIN) + tot @ dfimofr + delt2 * tot[:, -1])
    small = em < float(t.WSEMEAN_MIN)
    return np.where(small, float(t.WSEMEAN_MIN), em), np.where(small, 2.0 * frl, fm)
