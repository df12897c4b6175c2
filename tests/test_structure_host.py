"""Host side of the structure factor (include/kmc.h), no GPU:
kmc_host_structure_factor against the Python reference of _structure.py (exact
equality) and against libm within a derived bound, the values that are exact by
construction, the ligand lattice's Bragg peaks, the error returns, and the
post-processing (analysis.structure_factor / sq_radial)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _kmc import PKG, capi, engine, params
from _structure import (bind_some, check_lattice, lattice_state, positions, ref_structure_factor, selected,
                        snap_to_grid)

analysis = importlib.import_module(PKG + ".analysis")


@pytest.fixture(scope="module")
def random_state():
    """300 receptors + 100 ligands in a 4000 x 5000 box, a few bonds set by hand."""
    p = params(seed=7, n_a=300, n_b=100, box_x=4000.0, box_y=5000.0, box_z=1000.0)
    hs = engine.host_init_random(p)
    bind_some(hs, [(3, 5, 2), (17, 5, 3), (250, 99, 4), (8, 0, 2)])
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs


@pytest.mark.parametrize("select", ["all", "bound"])
@pytest.mark.parametrize("hmax,kmax", [(0, 0), (5, 4)])
def test_host_equals_reference(random_state, hmax, kmax, select):
    p, hs = random_state
    sums, n_sel = engine.host_structure_factor(p, hs, hmax, kmax, select)
    ref, ref_n = ref_structure_factor(p, hs, hmax, kmax, select)
    assert sums.shape == (4, hmax + 1, 2 * kmax + 1) and sums.dtype == np.int64
    assert np.array_equal(n_sel, ref_n) and np.array_equal(sums, ref)
    assert n_sel.tolist() == ([300, 100] if select == "all" else [4, 3])
    # a negative coordinate took the floor modulus somewhere
    assert positions(hs).min() < 0


@pytest.mark.parametrize("select", ["all", "bound"])
def test_host_against_libm(random_state, select):
    # Plain np.cos / np.sin of 2 pi (h x / box_x + k y / box_y) against C / 2^30 and S / 2^30, bound N * 2^-30 per
    # sum, i.e. 2^-30 = 9.3e-10 per term.  The budget per term:
    #   (a) the fixed-point rounding: at most half a unit, 2^-31 = 4.7e-10;
    #   (b) the coordinate quantum: a position moved by up to 2^-11 A moves an axis phase by up to
    #       2 pi * 8 * 2^-11 / 4000 = 6.1e-6 rad at hmax = kmax = 8 and a 4000 A box.  That is four orders above
    #       the other 2^-31, and no admissible box (the engine's are below 1e6 A) brings it under: with arbitrary
    #       positions the bound cannot hold, whatever the code does.  So the state is snapped to the 2^-10 A grid
    #       first (snap_to_grid): x = X / 1024 exactly, and (b) is zero;
    #   (c) double rounding on both routes: numpy's argument takes ~6 roundings of relative 1.1e-16 on a phase
    #       of at most 2 pi * 16 * 1.5 = 151 rad (|x| <= 1.5 box): <= 1e-13; the library's t and a, its cos /
    #       sin (< 1 ulp) and the four products and two sums: < 2e-15.
    # (a) + (c) < 2^-31 + 2e-13 < 2^-30 per term: |C / 2^30 - sum cos| <= N * 2^-30, and the same for S.
    p, hs = random_state
    hs = snap_to_grid(hs.copy())
    assert engine.host_validate(p, hs) == capi.KMC_OK
    hmax = kmax = 8
    assert min(p.box_x, p.box_y) >= 4000.0
    sums, n_sel = engine.host_structure_factor(p, hs, hmax, kmax, select)
    xy = positions(hs)
    assert np.array_equal(xy * 1024.0, np.round(xy * 1024.0))
    keep = selected(hs, select)
    h = np.arange(hmax + 1, dtype=np.float64)[:, None, None]
    k = np.arange(-kmax, kmax + 1, dtype=np.float64)[None, :, None]
    for sp, who in ((0, keep[:hs.n_a]), (1, keep[hs.n_a:])):
        pts = (xy[:hs.n_a] if sp == 0 else xy[hs.n_a:])[who]
        n = len(pts)
        assert n == n_sel[sp]
        arg = 2.0 * np.pi * (h * pts[None, None, :, 0] / p.box_x + k * pts[None, None, :, 1] / p.box_y)
        err_c = np.abs(sums[2 * sp] / 2.0 ** 30 - np.cos(arg).sum(axis=2)).max()
        err_s = np.abs(sums[2 * sp + 1] / 2.0 ** 30 - np.sin(arg).sum(axis=2)).max()
        print(f"select={select} species={sp} n={n}: max |C/2^30 - sum cos| = {err_c:.3e}, S: {err_s:.3e}, "
              f"bound {n * 2.0 ** -30:.3e}")
        assert err_c <= n * 2.0 ** -30 and err_s <= n * 2.0 ** -30


def test_exact_values(random_state):
    p, hs = random_state
    for select in ("all", "bound"):
        sums, n_sel = engine.host_structure_factor(p, hs, 0, 0, select)
        assert sums[:, 0, 0].tolist() == [int(n_sel[0]) << 30, 0, int(n_sel[1]) << 30, 0]
        kmax = 6
        sums, _ = engine.host_structure_factor(p, hs, 2, kmax, select)
        for sp in (0, 1):
            C0, S0 = sums[2 * sp, 0], sums[2 * sp + 1, 0]
            assert np.array_equal(C0[::-1], C0) and np.array_equal(S0[::-1], -S0)  # index k + kmax <-> -k + kmax
            assert S0[kmax] == 0 and np.abs(S0).max() > 0


def test_host_lattice_bragg_peaks():
    nx, ny, hmax, kmax = 8, 4, 16, 8
    p, hs = lattice_state(nx, ny)
    sums, n_sel = engine.host_structure_factor(p, hs, hmax, kmax, "all")
    check_lattice(p, sums, n_sel, nx, ny, hmax, kmax)
    # the peaks are there: |rho_B|^2 / N_B = N_B at a Bragg vector, ~0 off it
    S = analysis.structure_factor(sums, n_sel)["BB"]
    assert abs(S[nx, kmax + ny] - nx * ny) < 1e-6 and S[1, kmax + 1] < 1e-12
    # no ligand holds a bond: the bound selection is empty
    sums, n_sel = engine.host_structure_factor(p, hs, 2, 2, "bound")
    assert n_sel.tolist() == [0, 0] and not sums.any()


def test_host_errors(random_state):
    p, hs = random_state
    for hmax, kmax, select in ((-1, 0, 0), (0, -1, 0), (capi.SK_MAX + 1, 0, 0), (0, capi.SK_MAX + 1, 0), (1, 1, 2),
                               (1, 1, -1)):
        with pytest.raises(engine.KmcError) as e:
            engine.host_structure_factor(p, hs, hmax, kmax, select)
        assert e.value.code == capi.ERR_ARG
    L = engine.load_library()
    v = hs.view()
    buf, n = np.zeros(4, dtype=np.int64), np.zeros(2, dtype=np.int64)
    assert L.kmc_host_structure_factor(C.byref(p), C.byref(v), 0, 0, 0, None, n.ctypes.data) == capi.ERR_ARG
    assert L.kmc_host_structure_factor(C.byref(p), C.byref(v), 0, 0, 0, buf.ctypes.data, None) == capi.ERR_ARG
    assert L.kmc_host_structure_factor(None, C.byref(v), 0, 0, 0, buf.ctypes.data, n.ctypes.data) == capi.ERR_ARG
    # a box below the coordinate quantum: BX = round(box_x * 1024) < 1
    tiny = params(seed=7, n_a=300, n_b=100, box_x=0.0004, box_y=5000.0, box_z=1000.0)
    with pytest.raises(engine.KmcError) as e:
        engine.host_structure_factor(tiny, hs, 1, 1)
    assert e.value.code == capi.ERR_ARG
    # the largest grid is accepted
    sums, _ = engine.host_structure_factor(p, hs, capi.SK_MAX, capi.SK_MAX)
    assert sums.shape == (4, 65, 129)


def test_partials_and_radial_average():
    # a hand-made 2 x 3 grid: h = 0, 1 and k = -1, 0, 1, in units of 2^30
    u = 1 << 30
    ca = np.array([[3, 4, 3], [1, 0, 2]], dtype=np.int64) * u
    sa = np.array([[-1, 0, 1], [2, 1, 0]], dtype=np.int64) * u
    cb = np.array([[0, 2, 0], [1, 1, -1]], dtype=np.int64) * u
    sb = np.array([[2, 0, -2], [0, 3, 1]], dtype=np.int64) * u
    sums = np.stack([ca, sa, cb, sb])
    S = analysis.structure_factor(sums, (4, 2))
    A, B = (ca + 1j * sa) / u, (cb + 1j * sb) / u
    def norm2(z):  # small integers: exact in float64
        return z.real ** 2 + z.imag ** 2

    assert np.array_equal(S["AA"], norm2(A) / 4) and np.array_equal(S["BB"], norm2(B) / 2)
    assert np.allclose(S["AB"], (A * B.conj()).real / np.sqrt(8.0), rtol=1e-15, atol=0)
    assert np.array_equal(S["NN"], norm2(A + B) / 6)
    assert S["AA"][0, 1] == 4.0 and S["BB"][1, 1] == 5.0  # (4 + 0i): 16 / 4; (1 + 3i): 10 / 2
    # empty species give zeros, not NaN
    Z = analysis.structure_factor(sums, (4, 0))
    assert not Z["BB"].any() and not Z["AB"].any() and np.array_equal(Z["AA"], S["AA"])
    assert np.array_equal(Z["NN"], norm2(A + B) / 4)
    assert all(not v.any() for v in analysis.structure_factor(sums, (0, 0)).values())

    # box 2 pi x pi: q = (h, 2 k).  Independent vectors: (0, 1) |q| = 2; (1, -1), (1, 1) |q| = sqrt 5; (1, 0) |q| = 1;
    # left out: q = 0 and (0, -1), the Friedel copy of (0, 1)
    G = np.array([[100.0, 1000.0, 7.0], [2.0, 3.0, 4.0]])
    centres, mean, count = analysis.sq_radial(G, 2 * np.pi, np.pi, nbins=6, q_max=3.0)
    assert np.allclose(centres, [0.25, 0.75, 1.25, 1.75, 2.25, 2.75])
    assert count.tolist() == [0, 0, 1, 0, 3, 0] and count.dtype == np.int64
    assert mean[2] == 3.0 and mean[4] == (7.0 + 2.0 + 4.0) / 3.0
    assert np.isnan(mean[[0, 1, 3, 5]]).all()
    # q_max cuts: |q| = sqrt 5 lies beyond 2.2, |q| = 2 in the last bin [1.1, 2.2)
    _, mean, count = analysis.sq_radial(G, 2 * np.pi, np.pi, nbins=2, q_max=2.2)
    assert count.tolist() == [1, 1] and mean.tolist() == [3.0, 7.0]
    with pytest.raises(ValueError):
        analysis.sq_radial(G[:, :2], 1.0, 1.0, 4, 1.0)
