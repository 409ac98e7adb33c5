"""Every tools/make_golden_*.py that records a seam's fixtures from the reference's own Fortran, run now into a scratch directory, writes the
committed fixtures of tests/golden again: the same files, in every .npz the same arrays with the same dtypes and bytes, in every
*_observed.json the same figures.  The tools assert on their way what their docstrings say (equal branches in both precisions, margins)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
from oracle import ref_build  # noqa: E402

# the tool -> what its fixture files begin with
TOOLS = {"forcing": "forcing_", "intake": "intake_", "restart": "restart_", "readwind": "readwind_", "start": "start_", "gribout": "gribout_",
         "gribin": "gribin_", "nest": "intspec_", "ctu": "ctu_"}


@pytest.mark.parametrize("tool", list(TOOLS))
def test_the_tool_reproduces_the_fixtures(tool, tmp_path):
    ref = ref_build.reference_root()
    if tool == "gribin":      # compiles the project's own driver only: the Fortran compiler, no reference tree
        if not (shutil.which("amdflang") or os.path.exists("/opt/rocm/lib/llvm/bin/flang")):
            pytest.skip("no Fortran compiler on this machine")
    elif ref is None:
        pytest.skip("no reference tree on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", f"make_golden_{tool}.py"), ref or "-", str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    committed = sorted(f for f in os.listdir(GOLDEN) if f.startswith(TOOLS[tool]))
    assert committed and sorted(os.listdir(tmp_path)) == committed
    for f in committed:
        new, old = os.path.join(tmp_path, f), os.path.join(GOLDEN, f)
        assert os.path.getsize(new) <= 600_000 and os.path.getsize(old) <= 600_000, f
        if f.endswith(".json"):
            with open(new) as a, open(old) as b:
                assert json.load(a) == json.load(b), f
        else:
            with np.load(new) as z, np.load(old) as g:
                assert sorted(z.files) == sorted(g.files), f
                for k in z.files:
                    assert z[k].dtype == g[k].dtype and z[k].shape == g[k].shape and z[k].tobytes() == g[k].tobytes(), (f, k)
