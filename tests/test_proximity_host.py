"""The sequential proximity clusters (kmc_host_prox_clusters; include/kmc.h,
DESIGN.md §23) against the Python reference of _proximity.py, and the analysis
helpers on states whose answer is known in closed form.  No device.  Every
count is an integer: every comparison of counts is exact equality."""
import numpy as np
import pytest

from _bondorder import place_ligands
from _kmc import DENSE, PKG, capi, engine, params
from _proximity import BORDER_ORDER, border_line, line_state, ref_prox_clusters, same
from _structure import PITCH, bind_some, lattice_state

import importlib

analysis = importlib.import_module(PKG + ".analysis")

Q = 2.0 ** -10


def host(p, hs, *a, **kw):
    return engine.host_prox_clusters(p, hs, *a, per_protein=True, **kw)


@pytest.fixture(scope="module")
def placed():
    """150 + 50 proteins placed at random in 1000 x 1000, with a few bonds by hand."""
    p = params(seed=11, n_a=150, n_b=50, **DENSE)
    hs = engine.host_init_random(p)
    bind_some(hs, [(0, 0, 2), (1, 0, 3), (5, 7, 2), (9, 7, 4), (20, 30, 2)])
    return p, hs


@pytest.mark.parametrize("which", ["A", "B", "AB"])
@pytest.mark.parametrize("select", ["all", "bound"])
def test_placed_state_equals_reference(placed, which, select):
    p, hs = placed
    for eps, min_pts in ((40.0, 1), (60.0, 3), (150.0, 5)):
        got = host(p, hs, which, eps, min_pts, select, max_size=12, nbins=16)
        same(got, ref_prox_clusters(p, hs, which, eps, min_pts, select, max_size=12, nbins=16))
    if select == "all":
        assert got[3].n_sel == {"A": 150, "B": 50, "AB": 200}[which] and got[3].n_core > 0


def test_mask(placed):
    p, hs = placed
    mask = np.random.default_rng(3).random(p.n_a + p.n_b) < 0.5
    got = host(p, hs, "AB", 60.0, 3, mask=mask)
    same(got, ref_prox_clusters(p, hs, "AB", 60.0, 3, mask=mask))
    assert got[3].n_sel == mask.sum() and not got[6][~mask].any() and got[6][mask].all()
    none = host(p, hs, "AB", 60.0, 3, mask=np.zeros(p.n_a + p.n_b))
    assert not any(none[3].as_dict().values()) and not any(a.any() for a in none[:3] + none[4:])


def test_border_rule():
    p, hs = border_line(50.0)
    size_hist, _, _, out, label, nn, kind = got = host(p, hs, "B", 30.0, 4)
    same(got, ref_prox_clusters(p, hs, "B", 30.0, 4))
    # the point at 50 has two neighbours, the cores at 25 and 75, equidistant: a border point, and the core with
    # the smaller reference index takes it into the cluster with the LARGER label.  A label is 1 + n_a + b
    assert kind[1:].tolist() == [3] * 8 + [2] and nn[9] == 2 and out.n_border == 1 and out.n_clusters == 2
    assert label[1:].tolist() == [2, 3, 2, 2, 3, 3, 2, 3, 3] and size_hist[4] == 1 and size_hist[5] == 1
    assert out.max_size == 5 and out.max_label == 3
    # at 51 the core at 75 is nearer, whichever of the two has the smaller index
    for order, want in ((BORDER_ORDER, 3), (range(8), 6)):
        p, hs = border_line(51.0, order)
        got = host(p, hs, "B", 30.0, 4)
        same(got, ref_prox_clusters(p, hs, "B", 30.0, 4))
        assert got[4][1 + 8] == want and got[6][1 + 8] == 2


def test_chain_closes_around_the_box():
    n = 1200
    order = np.random.default_rng(7).permutation(n)
    p, hs = line_state(2.5 * np.arange(n) - 1500.0, order, box_y=9000.0)  # (room for the random placement)
    size_hist, nn_hist, nnd_hist, out, label, nn, kind = host(p, hs, "B", 2.5, 3, max_size=2000, nbins=4)
    assert out.n_clusters == 1 and out.max_size == n and out.max_label == 2 and out.n_core_edges == n
    assert size_hist[n] == 1 and nn_hist[2] == n and nnd_hist[3] == n and set(label[1:]) == {2}
    assert host(p, hs, "B", 2.5, 4)[3].n_noise == n
    alone = host(p, hs, "B", 2.5 - Q, 1)[3]
    assert alone.n_alone == n and alone.n_clusters == n and alone.n_multi == 0


def test_coincident_points_are_neighbours():
    p, hs = line_state([10.0, 10.0, 500.0])
    _, nn_hist, nnd_hist, out, label, nn, kind = host(p, hs, "B", 5.0, 2, nbins=8)
    assert nn[1:].tolist() == [1, 1, 0] and nnd_hist.tolist() == [2] + [0] * 7 and out.n_alone == 1
    assert label[1:].tolist() == [2, 2, 0] and kind[1:].tolist() == [3, 3, 1]


def test_relabelling_invariance():
    # which ligand sits at which position permutes label / kind / nn and changes no histogram and no count
    # (no bonds: the labels' values are indices, so they are compared as partitions)
    rng = np.random.default_rng(12)
    n = 150
    xs, ys = rng.random(n) * 600.0, rng.random(n) * 600.0
    res = []
    for perm in (np.arange(n), rng.permutation(n)):
        p = params(seed=5, n_a=1, n_b=n, box_x=3000.0, box_y=3000.0, box_z=250.0)
        hs = engine.host_init_random(p)
        x, y = np.zeros(n), np.zeros(n)
        x[perm], y[perm] = xs, ys
        place_ligands(hs, x, y)
        r = host(p, hs, "B", 40.0, 3, max_size=40, nbins=16)
        same(r, ref_prox_clusters(p, hs, "B", 40.0, 3, max_size=40, nbins=16))
        res.append((r, perm))
    (a, pa), (b, pb) = res
    da, db = a[3].as_dict(), b[3].as_dict()
    da.pop("max_label"), db.pop("max_label")
    assert da == db and a[3].n_border > 0 and a[3].n_noise > 0 and a[3].n_multi > 0
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))
    la, lb = a[4][1:][pa], b[4][1:][pb]  # by position
    assert np.array_equal(a[5][1:][pa], b[5][1:][pb]) and np.array_equal(a[6][1:][pa], b[6][1:][pb])
    assert np.array_equal(la == 0, lb == 0) and len(set(zip(la.tolist(), lb.tolist()))) == len(set(la.tolist()))


def test_lattice_and_the_analysis_helpers():
    nx, ny = 8, 6
    n = nx * ny
    p, hs = lattice_state(nx, ny, n_a=4)
    size_hist, nn_hist, nnd_hist, out, label, nn, kind = host(p, hs, "B", PITCH, 1, max_size=n, nbins=10)
    assert out.n_clusters == 1 and size_hist[n] == 1 and nn[4:].tolist() == [4] * n and out.sum_nn == 4 * n
    # every nearest neighbour is one pitch away: E_9^2 <= M, the last bin
    r, pdf, cdf, alone = analysis.nn_distance(nnd_hist, PITCH, out)
    assert nnd_hist.tolist() == [0] * 9 + [n] and alone == 0.0 and cdf[-1] == 1.0 and cdf[-2] == 0.0
    assert pdf[-1] == 1.0 / (PITCH / 10) and r[-1] == 0.95 * PITCH
    apart = host(p, hs, "B", PITCH - Q, 1, max_size=n, nbins=10)
    assert apart[3].n_clusters == n and apart[3].n_multi == 0 and apart[3].n_alone == n and apart[0][1] == n
    assert analysis.nn_distance(apart[2], PITCH - Q, apart[3])[3] == 1.0
    # Ripley's K of the lattice from the shell counts: 4 neighbours at 1, 4 at sqrt 2, 4 at 2 pitches
    nb = 21
    r_max = 2.1 * PITCH
    counts = np.zeros(nb, dtype=np.int64)
    for d, k in ((1.0, 4), (2.0 ** 0.5, 4), (2.0, 4)):
        counts[int(d * PITCH / (r_max / nb))] += k * n // 2  # unordered pairs
    r, K, L, H = analysis.ripley(counts, "BB", p, r_max)
    area = p.box_x * p.box_y
    want = np.zeros(nb)
    want[10:] += 4 * n
    want[14:] += 4 * n
    want[20:] += 4 * n
    assert np.array_equal(K, area * want / (n * (n - 1.0))) and np.allclose(L, np.sqrt(K / np.pi))
    assert np.allclose(H, L - r) and np.allclose(r, (np.arange(nb) + 1) * r_max / nb)
    ab = analysis.ripley(np.ones(4), "AB", p, 100.0)[1]
    assert np.allclose(ab, area * np.arange(1, 5) / (4.0 * n))


def test_prox_summary_ratios_and_zero_denominators():
    out = dict(n_sel=10, n_core=4, n_border=2, n_noise=4, n_alone=1, n_clusters=3, n_multi=2, sum_nn=12,
               n_core_edges=3, n_pure=1, n_whole=1, n_bond_multi=4, n_bond_kept=3, max_size=3, max_label=1)
    s = analysis.prox_summary(out, np.array([0, 1, 1, 1, 0]))
    assert s == dict(clustered=0.6, mean_size=2.0, mean_size_w=14.0 / 6.0, recovery=0.25, over_merge=0.5,
                     over_split=0.25)
    z = analysis.prox_summary(capi.ProxOut(), np.zeros(5, dtype=np.int64))
    assert all(np.isnan(v) for v in z.values())
    r, pdf, cdf, alone = analysis.nn_distance(np.zeros(4), 10.0, capi.ProxOut())
    assert not pdf.any() and not cdf.any() and np.isnan(alone)


def test_bad_arguments(placed):
    p, hs = placed
    for kw in (dict(which=3), dict(select=2), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")),
               dict(eps=float("inf")), dict(eps=334.0), dict(min_pts=0), dict(max_size=0),
               dict(max_size=capi.PX_MAX_SIZE + 1), dict(nbins=0), dict(nbins=capi.PX_NND_BINS + 1)):
        a = dict(which="B", eps=60.0, min_pts=3, select="all", max_size=16, nbins=8)
        a.update(kw)
        with pytest.raises(engine.KmcError) as e:
            engine.host_prox_clusters(p, hs, **a)
        assert e.value.code == capi.ERR_ARG, kw
    engine.host_prox_clusters(p, hs, "B", 333.0)  # a third of the box is accepted
