"""The read-only layers over the step engine at the sizes where their kernels
change code path: grid-stride loops over more workgroups than a
launch holds, the tracker's reduction tree with a third level, the cell grids
clamped to AN_NC_MAX / BO_NC_MAX cells per axis, cell scans of several tiles
and of more than 256 tiles.  Every result is compared with the sequential host
counterpart (or the numpy reference) on the state read back with get_state();
every comparison is exact equality, doubles as bit patterns.  Each test first
asserts, as arithmetic on its shapes, that the path it is there for engages.

States (tests/_scale.py), each evolved once on the device:
  M  65 600 + 21 900 proteins: 342 blocks of 256, the receptors alone 257
  L  524 400 + 174 800 proteins: 2732 blocks, the receptors 2049 (the last ragged)
  P  the 3000 + 600 state of test_gpu_analysis.py as a patch across the corner
     of a 330 000 x 310 000 box (and, for the bond order's grid, across its origin)"""
import numpy as np
import pytest

from _analysis import np_bin, np_d2, summary_dict
from _coag import ARRAYS as CF_ARRAYS
from _coag import table_differences
from _dynamics import Tracker, bits, same_info, same_sample
from _geometry import ROW, row_dicts, table_tuples
from _geometry import summary_dict as geom_summary
from _kinetics import ARRAYS as KIN_ARRAYS
from _kmc import DENSE, capi, engine, params
from _scale import blocks, env, evolve, facts_hold, list_rows, patch_in_large_box, scale_params

pytestmark = pytest.mark.gpu

AN_WG_MAX = 2048     # kmc_analysis.hip: workgroups of k_an_census, k_an_pairs, k_trk_sample, k_kin_sample
BO_WG_MAX = 2048     # kmc_bondorder.hip: workgroups of k_bo_reduce up to 64 bins, of k_bo_corr
BO_REDUCE_WIDE = 256  # kmc_observe.hip bo_reduce: workgroups of k_bo_reduce above 64 bins
GEO_TABLE_WG = 256   # kmc_geometry.hip: workgroups of k_geo_table
TRK_T = 256          # kmc_dynamics.hip: the width of one level of k_trk_tree
NC_MAX = 2048        # AN_NC_MAX (kmc_analysis.hip), BO_NC_MAX (kmc_bondorder.h): cells per axis
SCAN_TILE = 4096     # kmc_kernels.hip: counts per tile of bins_scan; k_scan_top takes 256 tiles an iteration

CHUNK, MOST = 2000, 10  # the evolution: at most 20 000 steps, looked at every 2000
RESORT, EVERY, UPDATES = 5, 4, 3  # the recorders' window: re-sorts before steps 2, 7 and 12, updates after 4, 8, 12


def _state(n_a, n_b, seed):
    p = scale_params(n_a, n_b, seed)
    sim, hs, f = evolve(p, CHUNK, MOST)
    print(f"{n_a}+{n_b}: {hs.step} steps, {f}")
    return p, sim, hs, f


@pytest.fixture(scope="module")
def state_m():
    s = _state(65_600, 21_900, 5)
    yield s
    s[1].close()


@pytest.fixture(scope="module")
def state_l():
    s = _state(524_400, 174_800, 5)
    yield s
    s[1].close()


@pytest.fixture(scope="module")
def states(request):
    """'M' or 'L' -> its fixture, made when first asked for."""
    return lambda name: request.getfixturevalue("state_" + name.lower())


@pytest.mark.parametrize("name", ["M", "L"])
def test_states_hold_what_the_layers_need(states, name):
    p, _, hs, f = states(name)
    assert f["rl"] > 0 and f["cis"] > 0, f
    assert f["max_size"] >= 3, f       # a component of three or more proteins
    assert f["cis_dimers"] > 0, f      # a ligand-free cis dimer
    assert f["bonds"] > 0 and facts_hold(f), f
    assert engine.host_validate(p, hs) == capi.KMC_OK
    n = p.n_a + p.n_b
    if name == "M":
        assert blocks(n) > TRK_T and blocks(p.n_a) > BO_REDUCE_WIDE
    else:
        assert blocks(p.n_a) > AN_WG_MAX and p.n_a % 256 != 0


# ---------------------------------------------------------------- census, components
def test_census_and_components_on_l(state_l):
    p, sim, hs, _ = state_l
    assert blocks(p.n_a + p.n_b) > AN_WG_MAX  # k_an_census strides over the blocks
    label = sim.components()
    for max_r, max_l in ((16, 8), (63, 63)):
        h_label, h_hist, h_out = engine.host_census(p, hs, max_r, max_l)
        hist, out = sim.census(max_r, max_l)
        assert np.array_equal(label, h_label)
        assert np.array_equal(hist, h_hist) and summary_dict(out) == summary_dict(h_out)
        assert hist.sum() == out.n_components
    assert out.max_size >= 3 and hist[2, 0] > 0


# ---------------------------------------------------------------- geometry
def _geometry_equals_host(p, sim, hs):
    label, shift, span = sim.unwrap()
    for max_size in (64, capi.GEOM_MAX_SIZE):
        h_label, h_shift, h_span, h_table, h_out = engine.host_cluster_geometry(p, hs, max_size)
        table, out = sim.cluster_geometry(max_size)
        assert table_tuples(table) == table_tuples(h_table)
        assert geom_summary(out) == geom_summary(h_out)
    assert np.array_equal(label, h_label) and np.array_equal(shift, h_shift) and np.array_equal(span, h_span)
    assert out.n_measured > 0 and table["count"][3:].sum() > 0
    rows = sim.cluster_list(2, cap=int(out.n_measured + out.n_spanning))
    want = list_rows(p, hs, h_label, h_shift, h_span, 2)
    assert len(rows) == out.n_measured + out.n_spanning
    assert [tuple(r[k] for k in ROW) for r in row_dicts(rows)] == want
    return shift, [r[0] for r in want]


@pytest.mark.parametrize("name", ["M", "L"])
def test_geometry_equals_host(states, name):
    # (the step takes no minimum image, so no bond forms across a seam, and after 2000 steps no bonded pair has
    # drifted across one: every shift is 0 here.  The patch P below has the shifts.)
    p, sim, hs, _ = states(name)
    assert blocks(p.n_a + p.n_b) > GEO_TABLE_WG  # k_geo_table strides over the blocks
    _, labels = _geometry_equals_host(p, sim, hs)
    if name == "L":
        # a component's root is its smallest index, a receptor: on M the later passes of the stride hold 64
        # receptors and the ligands, no root of a measured component; on L 4.6 · 10^5 receptors lie there
        assert sum(1 for r in labels if r > GEO_TABLE_WG * 256) > 100


# ---------------------------------------------------------------- bond order
def _same_bond_order(dev, host):
    assert dev[1].as_dict() == host[1].as_dict()
    for a, b in zip(dev[2:], host[2:]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(dev[0], host[0]) and dev[0].sum() == host[1].n_sel


def test_bond_order_on_m(state_m):
    p, sim, hs, _ = state_m
    # above 64 bins k_bo_reduce runs in 256 workgroups: the receptors are more blocks than that
    assert blocks(p.n_a) > BO_REDUCE_WIDE
    for nbins in (128, 64):
        dev = sim.bond_order("A", 6, 150.0, "within", "all", nbins, per_protein=True)
        _same_bond_order(dev, engine.host_bond_order(p, hs, "A", 6, 150.0, "within", "all", nbins, per_protein=True))
        assert dev[1].n_sel == p.n_a and dev[1].n_with > 1000
    dev = sim.bond_order("B", 6, None, "linked", "all", 64, per_protein=True)
    _same_bond_order(dev, engine.host_bond_order(p, hs, "B", 6, None, "linked", "all", 64, per_protein=True))
    corr = sim.bond_order_corr("B", 6, 600.0, 150.0)
    assert np.array_equal(corr, engine.host_bond_order_corr(p, hs, "B", 6, 600.0, 150.0))
    assert corr[1].sum() > 1000


def test_bond_order_on_l(state_l):
    p, sim, hs, _ = state_l
    assert blocks(p.n_a) > BO_WG_MAX  # k_bo_reduce strides over the blocks at 64 bins too
    dev = sim.bond_order("A", 6, 150.0, "within", "all", 64, per_protein=True)
    _same_bond_order(dev, engine.host_bond_order(p, hs, "A", 6, 150.0, "within", "all", 64, per_protein=True))
    assert dev[1].n_sel == p.n_a and dev[1].n_with > 1000


# ---------------------------------------------------------------- structure factor
@pytest.mark.parametrize("name", ["M", "L"])
def test_structure_factor_equals_host(states, name):
    p, sim, hs, _ = states(name)
    # 81 wave vectors are one q-block: its SK_WG = 1024 workgroups take the 32-protein tiles in a stride loop
    assert (p.n_a + 31) // 32 > 1024
    for select in ("all", "bound"):
        sums, n_sel = sim.structure_factor(4, 4, select)
        h_sums, h_n = engine.host_structure_factor(p, hs, 4, 4, select)
        assert np.array_equal(n_sel, h_n) and np.array_equal(sums, h_sums)
        assert sums[:, 0, 4].tolist() == [int(n_sel[0]) << 30, 0, int(n_sel[1]) << 30, 0]
    assert 0 < n_sel[0] < p.n_a and 0 < n_sel[1] < p.n_b


# ---------------------------------------------------------------- the three recorders
@pytest.mark.parametrize("name", ["M", "L"])
def test_recorders_side_by_side(states, name):
    p0, _, hs0, _ = states(name)
    p = scale_params(p0.n_a, p0.n_b, p0.seed, fast=True)
    n = p.n_a + p.n_b
    # k_trk_tree: more than 256 first-level sums make nout > 1 (the part[s * n + idx] layout, both ping-pong
    # buffers) and a third level; on L k_trk_sample, k_kin_sample and k_an_census stride over the blocks
    assert blocks(n) > TRK_T and blocks(blocks(n)) > 1
    if name == "L":
        assert blocks(n) > AN_WG_MAX and blocks(p.n_a) > AN_WG_MAX
    with env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.set_timing(("slot_resort",))  # event brackets only: counts the steps' re-sort launches
        sim.track_begin()
        sim.kin_begin()
        sim.cf_begin(16)
        trk, kin, cf = Tracker(p, hs0), engine.HostKinetics(p, hs0), engine.HostCoag(p, hs0, 16)
        recs, resorts = [], []
        for piece in range(1, UPDATES + 1):
            recs.append(sim.step(EVERY))
            info, k_out, c_out = sim.track_update(), sim.kin_update(), sim.cf_update()
            hs = sim.get_state()  # one transfer an update, shared by the three references
            resorts.append(sim.kernel_times().get("slot_resort", (0.0, 0))[1])
            # the tracker
            want = trk.update(hs)
            assert same_info(info, want), (piece, info.as_dict(), want)
            u, flags = sim.track_displacements()
            assert np.array_equal(bits(u), bits(trk.u)) and np.array_equal(flags, trk.flags), piece
            out, vh = sim.track_sample(200.0, 40)
            want_s, want_vh = trk.sample(hs, 200.0, 40)  # its sums are _dynamics.tree_sum's, compared as bits
            assert same_sample(out.as_dict(), want_s), (piece, out.as_dict(), want_s)
            assert np.array_equal(vh, want_vh), piece
            # the bond kinetics
            kin.update(hs)
            assert k_out.as_dict() == kin.acc.as_dict(), piece
            got = sim.kin_arrays()
            assert all(np.array_equal(getattr(got, k), getattr(kin.arrays, k)) for k in KIN_ARRAYS), piece
            k_s, k_hist = sim.kin_sample()
            want_k, want_hist = kin.sample()
            assert k_s.as_dict() == want_k.as_dict() and np.array_equal(k_hist, want_hist), piece
            # the cluster growth
            cf.update(hs)
            assert c_out.as_dict() == cf.acc.as_dict(), piece
            got = sim.cf_arrays()
            assert all(np.array_equal(getattr(got, k), getattr(cf.arrays, k)) for k in CF_ARRAYS), piece
            c_s, c_t = sim.cf_sample()
            want_c, want_t = cf.sample()
            assert c_s.as_dict() == want_c.as_dict() and table_differences(c_t, want_t.as_dict()) == [], piece
        final = engine.state_hash(p, hs)
    # the window saw what the recorders record
    print(name, info.as_dict(), "wraps", trk.n_wraps, "ended", k_hist[:5].sum(axis=1).tolist(), "merge",
          want_t.merge_pieces.tolist(), "frag", want_t.frag_pieces.tolist(), "resorts", resorts)
    assert resorts[-1] > resorts[0], "no re-sort between two updates"
    assert info.n_changed > 0 and trk.n_wraps >= 1
    assert want_vh.sum() > 0 and want_s["sum_u2"].sum() > 0.0
    assert k_hist[:5].sum() >= 1, "no R-L or cis bond ended in the window"  # rows 0..4: ended bonds by kind
    assert want_t.merge_pieces.sum() + want_t.frag_pieces.sum() >= 1, "no merger and no fragmentation"
    # the same run without recorders
    with env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        plain = [sim.step(EVERY) for _ in range(UPDATES)]
        assert np.array_equal(np.concatenate(plain), np.concatenate(recs))
        assert engine.state_hash(p, sim.get_state()) == final


# ---------------------------------------------------------------- the patch in a very large box
BIG_X, BIG_Y = 330_000.0, 310_000.0


@pytest.fixture(scope="module")
def patch():
    """(params, state) in the original 4000 x 3000 box, (params, state) of the patch P across the corner of the
    large box, the brute-force squared distances of P by species pair, and (params, state) of the same patch left
    across the origin of the large box."""
    kw = dict(DENSE)
    kw.update(box_x=4000.0, box_y=3000.0, box_z=250.0)
    p0 = params(seed=31, n_a=3000, n_b=600, **kw)
    with engine.Simulation(p0) as sim:  # test_gpu_analysis.py's evolved fixture
        sim.set_state(engine.host_init_random(p0))
        for _ in range(100):
            sim.step(100)
        hs0 = sim.get_state()
    p, hs = patch_in_large_box(p0, hs0, BIG_X, BIG_Y)
    assert engine.host_validate(p, hs) == capi.KMC_OK
    for arr, box in ((hs.ra[0], BIG_X), (hs.ra[1], BIG_Y), (hs.rb[0], BIG_X), (hs.rb[1], BIG_Y)):
        assert arr.min() < -box / 2 + 3500 and arr.max() > box / 2 - 3500  # the patch lies on both sides of the seam
    cache = {which: np_d2(hs, p, which) for which in ("AA", "AB", "BB")}
    print("P: pairs counted", {(w, r): int(np_bin(cache[w], r, n).sum())
                               for w in cache for r, n in ((150.0, 30), (40.0, 20))})
    return (p0, hs0), (p, hs), cache, patch_in_large_box(p0, hs0, BIG_X, BIG_Y, inset=None)


def test_geometry_across_the_corner(patch):
    # the patch's components lie across both seams of the large box: shifts of both signs on both axes
    p, hs = patch[1]
    with engine.Simulation(p) as sim:
        sim.set_state(hs)
        shift, _ = _geometry_equals_host(p, sim, hs)
    assert shift[:, 0].any() and shift[:, 1].any(), "no component lies across a seam"


# AA at r_max = 40 is left out: no two receptors of P lie within 40 A of each other, the reference counts 0 pairs
# (in the 4000 x 3000 box the receptors closer than that are neighbours through its seams only, where the step
# takes no minimum image; the patch is cut out of that box).  Pairs counted by the reference for the others:
# AA 24 384, AB 8 698, BB 682 at 150; AB 591, BB 12 at 40
@pytest.mark.parametrize("which,r_max,nbins", [("AA", 150.0, 30), ("AB", 150.0, 30), ("BB", 150.0, 30),
                                               ("AB", 40.0, 20), ("BB", 40.0, 20)])
def test_pair_counts_in_a_clamped_grid(patch, which, r_max, nbins):
    p, hs = patch[1]
    fx, fy = int(p.box_x // r_max), int(p.box_y // r_max)
    assert fx > NC_MAX and fy > NC_MAX  # AN_NC_MAX clamps both axes: cells wider than r_max
    ncnt = (2 if which == "AB" else 1) * NC_MAX * NC_MAX + 1
    assert NC_MAX * NC_MAX > AN_WG_MAX              # k_an_pairs strides over the cells
    assert (ncnt + SCAN_TILE - 1) // SCAN_TILE > 256  # k_scan_top carries from one iteration to the next
    want = np_bin(patch[2][which], r_max, nbins)
    assert want.sum() > 0
    with engine.Simulation(p) as sim:
        sim.set_state(hs)
        assert np.array_equal(sim.pair_counts(which, r_max, nbins), want)
        assert sim.get_state().equal(hs)


@pytest.mark.parametrize("which", ["AA", "AB"])
def test_pair_counts_over_many_unclamped_cells(patch, which):
    p, hs = patch[0]
    r_max, nbins = 40.0, 20
    ncx, ncy = int(p.box_x // r_max), int(p.box_y // r_max)
    assert (ncx, ncy) == (100, 75) and max(ncx, ncy) <= NC_MAX  # unclamped
    assert ncx * ncy > AN_WG_MAX and ncx * ncy + 1 > SCAN_TILE  # a stride over the cells, a scan of several tiles
    want = np_bin(np_d2(hs, p, which), r_max, nbins)
    assert want.sum() > 0
    with engine.Simulation(p) as sim:
        sim.set_state(hs)
        assert np.array_equal(sim.pair_counts(which, r_max, nbins), want)


@pytest.mark.parametrize("where", ["corner", "origin"])
def test_bond_order_in_a_clamped_grid(patch, where):
    # across the corner the displacements fold over the large box; the bond order's cells bin the coordinate
    # modulo the box, so their first and last rows and columns meet at the origin: the patch left there has its
    # neighbours in the clamped grid's wrapped cells
    p, hs = patch[1] if where == "corner" else patch[3]
    assert int(p.box_x // 150.0) > NC_MAX and int(p.box_y // 150.0) > NC_MAX  # BO_NC_MAX clamps the neighbour grid
    assert int(p.box_x // 600.0) <= NC_MAX  # the correlation's own grid (cells of r_max) is not clamped
    if where == "origin":
        assert engine.host_validate(p, hs) == capi.KMC_OK
        assert all(a.min() < -150.0 and a.max() > 150.0 for a in (hs.rb[0], hs.rb[1]))
    with engine.Simulation(p) as sim:
        sim.set_state(hs)
        dev = sim.bond_order("B", 6, 150.0, per_protein=True)
        _same_bond_order(dev, engine.host_bond_order(p, hs, "B", 6, 150.0, per_protein=True))
        assert dev[1].n_with > 100
        corr = sim.bond_order_corr("B", 6, 600.0, 150.0)
        assert np.array_equal(corr, engine.host_bond_order_corr(p, hs, "B", 6, 600.0, 150.0))
        assert corr[1].sum() > 100
