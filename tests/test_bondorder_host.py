"""Host side of the bond-orientational order (include/kmc.h), no
GPU: kmc_host_bond_order / kmc_host_bond_order_corr against the Python
reference of _bondorder.py (exact equality), the square ligand lattice whose
values are known, the edge cases, the linked neighbour relation on a hand-bound
lattice, the error returns and the post-processing (analysis.bond_order /
bond_order_corr)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _bondorder import bind_network, neighbour_lists, ref_bond_order, ref_bond_order_corr
from _kmc import PKG, capi, engine, params
from _structure import ORIGIN, PITCH, bind_some, lattice_state

analysis = importlib.import_module(PKG + ".analysis")

U = 1 << 30
FOLDS = (1, 4, 6, 12)


def equal_local(got, want):
    hist, out, Cs, Ss, nn = got
    r_hist, r_out, r_C, r_S, r_nn = want
    assert out.as_dict() == r_out
    assert np.array_equal(nn, r_nn) and np.array_equal(Cs, r_C) and np.array_equal(Ss, r_S)
    assert hist.dtype == np.int64 and np.array_equal(hist, r_hist) and hist.sum() == r_out["n_sel"]


@pytest.fixture(scope="module")
def random_state():
    """300 receptors + 100 ligands in a 4000 x 5000 box as host_init_random places them (no bonds)."""
    p = params(seed=7, n_a=300, n_b=100, box_x=4000.0, box_y=5000.0, box_z=1000.0)
    return p, engine.host_init_random(p)


@pytest.fixture(scope="module")
def bound_state(random_state):
    """The same placement with bonds set by hand: bind_some's four R-L bonds and cis pair, and five
    ligand-receptor=receptor-ligand bridges, so both selections and the linked mode have something to find."""
    p, hs = random_state
    hs = hs.copy()
    bind_some(hs, [(3, 5, 2), (17, 5, 3), (250, 99, 4), (8, 0, 2)])
    bind_network(hs, [(10, 2, 100, 101, 11, 2), (11, 3, 102, 103, 12, 2), (12, 3, 104, 105, 10, 3),
                      (20, 4, 106, 107, 21, 4), (30, 2, 108, 109, -1, 0)])
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs


@pytest.mark.parametrize("select", ["all", "bound"])
@pytest.mark.parametrize("which,mode,r_cut", [("A", "within", 400.0), ("B", "within", 1300.0), ("B", "linked", None)])
@pytest.mark.parametrize("state", ["random", "bound"])
def test_host_equals_reference(random_state, bound_state, state, which, mode, r_cut, select):
    p, hs = random_state if state == "random" else bound_state
    nbr = neighbour_lists(p, hs, which, mode, r_cut, select)
    pairs = sum(len(v) for v in nbr.values())
    if state == "bound":
        assert 0 < len(nbr) and pairs > 0
        if select == "bound":
            assert len(nbr) < (p.n_a if which == "A" else p.n_b)
    elif select == "bound" or mode == "linked":
        assert pairs == 0  # no bonds: an empty set, or nobody linked
    for fold in FOLDS:
        equal_local(engine.host_bond_order(p, hs, which, fold, r_cut, mode, select, 50, per_protein=True),
                    ref_bond_order(p, hs, which, fold, r_cut, mode, select, 50, nbr))
        corr = engine.host_bond_order_corr(p, hs, which, fold, 1300.0, r_cut, mode, select, 24)
        assert corr.shape == (2, 24) and corr.dtype == np.int64
        assert np.array_equal(corr, ref_bond_order_corr(p, hs, which, fold, 1300.0, r_cut, mode, select, 24, nbr))
    if state == "bound" and which == "A" and select == "all":
        assert corr[1].sum() > 1000  # the correlation saw pairs
    # without the per-protein arrays the call returns the same histogram and summary
    hist, out = engine.host_bond_order(p, hs, which, 6, r_cut, mode, select, 50)
    full = engine.host_bond_order(p, hs, which, 6, r_cut, mode, select, 50, per_protein=True)
    assert np.array_equal(hist, full[0]) and out.as_dict() == full[1].as_dict()


def test_square_lattice():
    nx, ny = 8, 6
    p, hs = lattice_state(nx, ny)
    n = nx * ny
    # r_cut = the pitch exactly: D2 = RC^2 is included, the four axial neighbours, the seam's among them
    for fold, want in ((4, 4 * U), (8, 4 * U), (2, 0), (6, 0)):
        hist, out, Cs, Ss, nn = engine.host_bond_order(p, hs, "B", fold, PITCH, nbins=32, per_protein=True)
        assert nn.tolist() == [4] * n and Cs.tolist() == [want] * n, fold
        if want:
            assert Ss.tolist() == [0] * n
            assert out.as_dict() == dict(n_sel=n, n_with=n, sum_nn=4 * n, sum_pc=n * 32768, sum_ps=0,
                                         sum_m=n * U)
            only = np.zeros((capi.BO_NN_ROWS, 32), dtype=np.int64)
            only[4, 31] = n  # pc = 32768: the whole histogram in row 4, last bin
            assert np.array_equal(hist, only)
    equal_local(engine.host_bond_order(p, hs, "B", 4, PITCH, nbins=32, per_protein=True),
                ref_bond_order(p, hs, "B", 4, PITCH, nbins=32))
    # just below the pitch nobody has a neighbour; with the diagonals (8 neighbours) fold 4 cancels
    _, out, Cs, _, nn = engine.host_bond_order(p, hs, "B", 4, PITCH - 0.001, per_protein=True)
    assert nn.tolist() == [0] * n and out.n_with == 0
    _, _, Cs, _, nn = engine.host_bond_order(p, hs, "B", 4, 283.0, per_protein=True)
    assert nn.tolist() == [8] * n and Cs.tolist() == [0] * n
    # perfect order: every pair contributes 2^30, and the pair counts are the brute-force ones
    corr = engine.host_bond_order_corr(p, hs, "B", 4, 400.0, PITCH, nbins=16)
    ref = ref_bond_order_corr(p, hs, "B", 4, 400.0, PITCH, nbins=16)
    assert np.array_equal(corr[0], U * corr[1]) and np.array_equal(corr, ref)
    # the pitch falls on the edge of bin 8 (E_8 = 204800 exactly: included), the diagonal 282.8 in bin 11
    assert corr[1].tolist() == [0] * 8 + [2 * n, 0, 0, 2 * n, 0, 0, 0, 0]
    r, g = analysis.bond_order_corr(corr, 400.0)
    assert g[8] == 1.0 and g[11] == 1.0 and np.isnan(g[0]) and r[8] == 8.5 * 25.0
    out = engine.host_bond_order(p, hs, "B", 4, PITCH)[1]
    assert out.n_sel == n and analysis.bond_order(out) == dict(psi_abs=1.0, psi2=1.0, mean_nn=4.0)


def test_edge_cases():
    p, hs = lattice_state(8, 6)
    hs = hs.copy()
    # ligand 1 moved onto ligand 0: coincident points are not neighbours of each other, and each is one
    # neighbour (not two) short of nothing else: the others see both
    hs.rb[:, 1] += np.tile(hs.rb[0:3, 0] - hs.rb[0:3, 1], hs.rb.shape[0] // 3)
    assert hs.rb[0, 1] == hs.rb[0, 0] and hs.rb[1, 1] == hs.rb[1, 0]
    got = engine.host_bond_order(p, hs, "B", 4, PITCH, nbins=8, per_protein=True)
    equal_local(got, ref_bond_order(p, hs, "B", 4, PITCH, nbins=8))
    nn = got[4]
    assert nn[0] == nn[1] and sorted(set(nn.tolist())) == [3, 4, 5]  # the vacated site's neighbours lose one
    # receptors with a tiny cutoff: nobody has a neighbour — row 0, bin 0
    hist, out, Cs, Ss, nn = engine.host_bond_order(p, hs, "A", 6, 0.01, nbins=8, per_protein=True)
    assert not nn.any() and not Cs.any() and not Ss.any()
    assert hist[0, 0] == p.n_a and hist.sum() == p.n_a
    assert out.as_dict() == dict(n_sel=p.n_a, n_with=0, sum_nn=0, sum_pc=0, sum_ps=0, sum_m=0)
    assert not engine.host_bond_order_corr(p, hs, "A", 6, 100.0, 0.01).any()
    # an empty selection
    hist, out = engine.host_bond_order(p, hs, "B", 6, PITCH, select="bound")
    assert not hist.any() and out.n_sel == 0


def lattice_site(hs, nx, ny):
    """{(i, j): ligand} of lattice_state's ligands, from their positions."""
    site = {}
    for b in range(hs.n_b):
        i = int(round((hs.rb[0, b] - ORIGIN[0]) / PITCH)) % nx
        j = int(round((hs.rb[1, b] - ORIGIN[1]) / PITCH)) % ny
        site[(i, j)] = b
    assert len(site) == nx * ny
    return site


def linked_lattice(nx=8, ny=6):
    """lattice_state with bridges along lattice edges: every horizontal edge (site 2 to the right, site 3 to the
    left; the seam's too), one vertical edge, a second bridge between (0, 0) and (1, 0) — a doubly linked pair —
    and a ligand whose receptor's cis partner holds no ligand."""
    p, hs = lattice_state(nx, ny, n_a=2 * nx * ny + 6)
    at = lattice_site(hs, nx, ny)
    bridges, r = [], 0
    for j in range(ny):
        for i in range(nx):
            bridges.append((at[(i, j)], 2, r, r + 1, at[((i + 1) % nx, j)], 3))
            r += 2
    bridges.append((at[(0, 0)], 4, r, r + 1, at[(1, 0)], 4))
    bridges.append((at[(3, 2)], 4, r + 2, r + 3, at[(3, 3)], 4))
    bridges.append((at[(2, 1)], 4, r + 4, r + 5, -1, 0))
    bind_network(hs, bridges)
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs, at


@pytest.mark.parametrize("select", ["all", "bound"])
def test_linked_on_a_hand_bound_lattice(select):
    p, hs, at = linked_lattice()
    nbr = neighbour_lists(p, hs, "B", "linked", None, select)
    pairs = sum(len(v) for v in nbr.values())
    assert pairs >= 2 * 10
    # by hand: two horizontal neighbours each; (0, 0) and (1, 0) see each other twice; the vertical edge adds one to
    # both ends; the partner without a ligand adds none
    want = {b: 2 for b in range(p.n_b)}
    for ij in ((0, 0), (1, 0), (3, 2), (3, 3)):
        want[at[ij]] += 1
    assert {b: len(v) for b, v in nbr.items()} == want
    assert [j for j, _, _ in nbr[at[(0, 0)]]].count(at[(1, 0)]) == 2
    for fold in (2, 6):
        got = engine.host_bond_order(p, hs, "B", fold, None, "linked", select, 16, per_protein=True)
        equal_local(got, ref_bond_order(p, hs, "B", fold, None, "linked", select, 16, nbr))
        assert got[4].tolist() == [want[b] for b in range(p.n_b)]
        assert np.array_equal(engine.host_bond_order_corr(p, hs, "B", fold, 400.0, None, "linked", select, 16),
                              ref_bond_order_corr(p, hs, "B", fold, 400.0, None, "linked", select, 16, nbr))
    # r_cut is ignored
    a = engine.host_bond_order(p, hs, "B", 6, 1e9, "linked", select, 16, per_protein=True)
    assert np.array_equal(a[2], got[2]) and np.array_equal(a[0], got[0])


def code(f, *a, **kw):
    with pytest.raises(engine.KmcError) as e:
        f(*a, **kw)
    return e.value.code


def test_host_errors(bound_state):
    p, hs = bound_state
    bo, co = engine.host_bond_order, engine.host_bond_order_corr
    assert bo(p, hs, "B", 12, 1300.0, nbins=capi.BO_HIST_BINS)[0].shape == (16, 1024)  # the limits are accepted
    assert co(p, hs, "B", 1, 1333.0, 1333.0, nbins=capi.BO_CORR_BINS).shape == (2, 4096)
    for kw in (dict(which=2), dict(which=-1), dict(mode=2), dict(fold=0), dict(fold=capi.BO_MAX_FOLD + 1),
               dict(select=2), dict(select=-1), dict(which="A", mode="linked"), dict(r_cut=None), dict(r_cut=0.0),
               dict(r_cut=-1.0), dict(r_cut=float("nan")), dict(r_cut=float("inf")), dict(r_cut=1334.0),
               dict(r_cut=0.0004), dict(nbins=0), dict(nbins=capi.BO_HIST_BINS + 1)):
        a = dict(which="B", fold=6, r_cut=400.0, mode="within", select="all", nbins=8)
        a.update(kw)
        assert code(bo, p, hs, **a) == capi.ERR_ARG, kw
        if "nbins" not in kw:
            assert code(co, p, hs, r_max=500.0, **a) == capi.ERR_ARG, kw
    for kw in (dict(nbins=0), dict(nbins=capi.BO_CORR_BINS + 1), dict(r_max=0.0), dict(r_max=-3.0),
               dict(r_max=float("nan")), dict(r_max=float("inf")), dict(r_max=1334.0), dict(r_max=0.0004)):
        a = dict(which="B", fold=6, r_cut=400.0, r_max=500.0, nbins=8)
        a.update(kw)
        assert code(co, p, hs, **a) == capi.ERR_ARG, kw
    L = engine.load_library()
    v = hs.view()
    hist, corr, out = np.zeros(16 * 8, dtype=np.int64), np.zeros(2 * 8, dtype=np.int64), capi.BondOrderOut()
    tail = (hist.ctypes.data, C.byref(out), None, None, None)
    assert L.kmc_host_bond_order(C.byref(p), C.byref(v), 1, 0, 6, 400.0, 0, 8, *tail) == capi.KMC_OK
    assert L.kmc_host_bond_order(C.byref(p), C.byref(v), 1, 0, 6, 400.0, 0, 8, None, C.byref(out), None, None,
                                 None) == capi.KMC_OK  # the histogram may be left out
    assert L.kmc_host_bond_order(None, C.byref(v), 1, 0, 6, 400.0, 0, 8, *tail) == capi.ERR_ARG
    assert L.kmc_host_bond_order(C.byref(p), None, 1, 0, 6, 400.0, 0, 8, *tail) == capi.ERR_ARG
    assert L.kmc_host_bond_order(C.byref(p), C.byref(v), 1, 0, 6, 400.0, 0, 8, hist.ctypes.data, None, None, None,
                                 None) == capi.ERR_ARG
    assert L.kmc_host_bond_order_corr(C.byref(p), C.byref(v), 1, 0, 6, 400.0, 0, 500.0, 8, None) == capi.ERR_ARG
    assert L.kmc_host_bond_order_corr(C.byref(p), C.byref(v), 1, 0, 6, 400.0, 0, 500.0, 8,
                                      corr.ctypes.data) == capi.KMC_OK
    # a box below the coordinate quantum
    tiny = params(seed=7, n_a=300, n_b=100, box_x=0.0004, box_y=5000.0, box_z=1000.0)
    assert code(bo, tiny, hs, "B", 6, 0.0001) == capi.ERR_ARG
    # a link that leaves the state, followed by the linked mode only
    n = p.n_a + p.n_b
    for arr, row, col, bad in (("b_int", 5, 10, n + 5), ("b_int", 5, 10, -2), ("b_int", 5, 10, p.n_a + 1),
                               ("a_int", 4, 100, n + 1), ("a_int", 2, 101, 7), ("a_int", 2, 101, n + 1)):
        broken = hs.copy()
        getattr(broken, arr)[row, col] = bad
        assert code(bo, p, broken, "B", 6, None, "linked") == capi.ERR_STATE, (arr, row, bad)
        assert code(co, p, broken, "B", 6, 500.0, None, "linked") == capi.ERR_STATE
        bo(p, broken, "B", 6, 1300.0)


def test_too_many_neighbours():
    # 65537 ligands within one cutoff of each other: the first centre already has 65536 neighbours
    n = capi.BO_NN_ROWS * 4096 + 1
    p = params(seed=5, n_a=1, n_b=n, box_x=30000.0, box_y=30000.0, box_z=1000.0)
    hs = capi.HostState(p.n_a, p.n_b)
    i = np.arange(n)
    hs.rb[0] = (i % 300) * 0.25
    hs.rb[1] = (i // 300) * 0.25
    assert code(engine.host_bond_order, p, hs, "B", 6, 500.0) == capi.ERR_CAPACITY
    assert code(engine.host_bond_order_corr, p, hs, "B", 6, 500.0, 500.0) == capi.ERR_CAPACITY


def test_post_processing():
    out = dict(n_sel=10, n_with=4, sum_nn=18, sum_pc=3 * 32768, sum_ps=-4 * 32768, sum_m=2 * (1 << 30))
    assert analysis.bond_order(out) == dict(psi_abs=1.25, psi2=0.5, mean_nn=1.8)
    o = capi.BondOrderOut(**out)
    assert analysis.bond_order(o) == analysis.bond_order(out)
    assert analysis.bond_order(capi.BondOrderOut()) == dict(psi_abs=0.0, psi2=0.0, mean_nn=0.0)
    corr = np.array([[U, -U // 2, 0, 3 * U], [2, 1, 0, 3]], dtype=np.int64)
    r, g = analysis.bond_order_corr(corr, 40.0)
    assert r.tolist() == [5.0, 15.0, 25.0, 35.0]
    assert g[[0, 1, 3]].tolist() == [0.5, -0.5, 1.0] and np.isnan(g[2])
    with pytest.raises(ValueError):
        analysis.bond_order_corr(corr[0], 40.0)
    with pytest.raises(ValueError):
        analysis.bond_order_corr(corr, 0.0)
    # replicas add: the summed histogram and corr are those of the pooled proteins and pairs
    assert np.array_equal(analysis.reduce_counts(corr), corr)
