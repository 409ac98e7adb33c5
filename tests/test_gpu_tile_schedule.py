"""GPU tests of the step schedule of the advecting tile load (implsch_v4.h::v4_advect_tile): what a lane's chunk implies is worked out once per
round and the carry-over of frequencies outside [m0, m1) is skipped by a wave-uniform test.  The one-kernel step must stay bit-identical to the
two-kernel step (ecwam_hip_propags2_otf + ecwam_hip_newwind + ecwam_hip_implsch) at every direction count, in every form, with and without
carried-over frequencies, on grids whose last wave is short (the point count is not a multiple of the points per wave) and whose points have
land neighbours.  Halo neighbours: tests/test_gpu_fused.py::test_one_kernel_step_on_a_decomposed_grid_is_bit_identical."""
import pytest

from ecwam_amd.tables import Config

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# points per wave of the one-kernel builds (implsch4a.hip)
PP = {(48, "sp"): 2, (36, "sp"): 3, (24, "sp"): 5, (12, "sp"): 10, (36, "dp"): 3}


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ecwam_amd import api as _api

    return _api


def _run(nang, prec, nfre_red, lfm, subgrid, ngrid):
    from ecwam_amd import grid as G, synthetic as syn
    from ecwam_amd.wamintgr import Wamintgr

    cfg = Config(nang=nang, nfre=36, nfre_red=nfre_red, idelt=450, idelpro=450)
    g = G.build_grid(ngrid, mask="continents")
    assert g.nsea % PP[(nang, prec)] != 0, "the grid must end in a short wave"
    kw = dict(ifrelfmax=lfm, delpro_lf=225.0) if lfm else {}
    ms = []
    for _ in range(2):
        m = Wamintgr(cfg, g, prec, **kw)
        m.init_synthetic(seed=41)
        m.ff_next = m.ff.clone()
        m.ff_next[:, 3] *= 1.03
        ms.append(m)
    two, one = ms
    if subgrid:
        obs = syn.obstructions(g, cfg.nfre, seed=9)
        obs[:, :, nfre_red:] = 1.0
        for m in ms:
            m.set_obstructions(obs)
    assert two.build_weights() == 0 and one.build_weights() == 0 and one.fused_available()
    for _i in range(2):
        two.step()
        one.step(fused=True)
        torch.cuda.synchronize()
        n = one.n
        for name in ("fl1", "ff", "intf", "mij", "xllws"):
            x, y = getattr(two, name)[:n], getattr(one, name)[:n]
            assert torch.equal(x, y), f"{name}: {int((x != y).sum())} of {x.numel()} elements differ"
    assert float(one.fl1[: one.n].abs().max()) > 0 and bool(torch.isfinite(one.fl1).all())
    two.ctx.close(); one.ctx.close()


# (nang, prec, grid size): full rounds and tail steps per point -- 48: 6 rounds + 48 chunks, 36: 5 + 4 (sp) / 10 + 8 (dp), 24: 3 + 24, 12: 1 + 44
CASES = [(48, "sp", 13), (36, "sp", 17), (36, "dp", 14), (24, "sp", 13), (12, "sp", 15)]


@pytest.mark.parametrize("nang,prec,ngrid", CASES)
@pytest.mark.parametrize("nfre_red", [36, 29])
def test_plain_step_every_direction_count(api, nang, prec, ngrid, nfre_red):
    """ADV = 1: all frequencies advected (no carry-over) and the last seven carried over (the per-element selects)."""
    _run(nang, prec, nfre_red, 0, False, ngrid)


@pytest.mark.parametrize("nang,prec,ngrid,lfm,subgrid", [c + f for c in CASES for f in ((5, False), (0, True), (4, True)) if not (c[0] == 48 and f[0])])
def test_fast_wave_and_obstruction_forms(api, nang, prec, ngrid, lfm, subgrid):
    """ADV = 3 / 5 / 7 where a build holds them (48 directions: no fast-wave form)."""
    _run(nang, prec, 36, lfm, subgrid, ngrid)
