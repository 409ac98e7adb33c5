"""The Fortran side of include/ecwam_hip_restart.h, compiled: the six BIND(C) interfaces of ecwam_hip_capi.F90, ECWAM_HIP_SAVSTRESS / ECWAM_HIP_GETSTRESS and
the LDEVICE path of ECWAM_HIP_WRITEFL (ecwam_hip_restart.F90), through the harness program ecwam_amd/fortran/restart_check.F90.  Without a device the
program calls every interface with a null context and arguments of the declared kinds and reads the error return; on a device (-m gpu) it runs the
wrappers after a WAMINTGR_HIP call against the host paths and stops at the first difference."""
import os
import subprocess

import numpy as np
import pytest

from ecwam_amd import build


def _exe(prec):
    exe = build.fortran_exe(prec, "restart_check")
    if not os.path.exists(exe):
        build.build_fortran()
    return exe


@pytest.mark.parametrize("prec", ["sp", "dp"])
def test_the_interfaces_compile_link_and_refuse_a_null_context(prec):
    """Fails without the feature: the program links against the six symbols through their Fortran interfaces; each call returns 1 with
    "null context" in ecwam_hip_last_error (no device is touched)."""
    r = subprocess.run([_exe(prec), "capi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "restart_check: ok capi" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("prec,nang,nproma", [("sp", 12, 24), ("dp", 12, 24), ("sp", 36, 64)])
def test_the_wrappers_on_the_device(tmp_path, prec, nang, nproma):
    """ECWAM_HIP_WRITEFL with LDEVICE writes the file of its host path, plain and relabelled; ECWAM_HIP_SAVSTRESS and ECWAM_HIP_GETSTRESS agree with
    savstress.F90:112-127 / getstress.F90:150-184 on the host copies (the program compares, a ragged last chunk included); ECWAM_HIP_DEPTHPRPT and
    ECWAM_HIP_BUILDSTRESS run through their interfaces on device rows.  RFIELD of the Fortran side is then read here: columns of real forcing."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_fortran as TF
    from ecwam_amd import grid as G
    from ecwam_amd.tables import Config
    from ecwam_amd.wamintgr import Wamintgr

    idelt = 450 if nang == 36 else 900
    cfg = Config(nang=nang, nfre=36, nfre_red=36 if nang == 36 else 25, idelt=idelt, idelpro=idelt)
    g = G.build_grid(16, mask="continents")
    m = Wamintgr(cfg, g, prec)
    try:
        m.init_synthetic(seed=21)
        n = g.nsea
        assert n % nproma != 0      # a ragged last chunk: pad lanes
        case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        TF._write_case(case, m, cfg, g, nproma, 1)
        r = subprocess.run([_exe(prec), case, out, str(tmp_path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "restart_check: ok device" in r.stdout, r.stdout + r.stderr
        for f in ("bls", "bls_relab"):
            with open(str(tmp_path / f.replace("bls", "bls_host")), "rb") as a, open(str(tmp_path / f.replace("bls", "bls_dev")), "rb") as b:
                x, y = a.read(), b.read()
            assert len(x) == n * nang * 36 * np.dtype(m.npdt).itemsize + 8 and x == y, f
        with open(str(tmp_path / "bls_host"), "rb") as a, open(str(tmp_path / "bls_host_relab"), "rb") as b:
            assert a.read() != b.read()
        rf = np.fromfile(out, m.npdt).reshape(16, n)      # RFIELD(NPTS,16)
        m.step()
        torch.cuda.synchronize()
        ff = m.ff.cpu().numpy()
        from ecwam_amd import lib
        for f, c in enumerate(lib.RESTART_FF_COLUMNS):      # the same step on the Python host: the same forcing rows
            assert np.array_equal(rf[f], ff[:, c]), (f, c)
    finally:
        m.ctx.close()
