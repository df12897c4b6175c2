"""Python reference of the proximity clusters (include/kmc.h),
shared by test_proximity_host.py and test_gpu_proximity.py and written from the
definitions, not from the C code: integer coordinates with numpy (round_ through
engine.math, the host kmc_math.h), a brute-force D2 matrix over the selected
points (no cell grid), a dict union-find over the core pairs, the nearest-core
border rule, and the purity from engine.host_census' labels.  Every comparison
against it is exact equality."""
import numpy as np

from _bondorder import place_ligands
from _kmc import capi, engine, params
from _structure import positions, selected

NN_ROWS = 64
FIELDS = ("n_sel", "n_core", "n_border", "n_noise", "n_alone", "n_clusters", "n_multi", "sum_nn", "n_core_edges",
          "n_pure", "n_whole", "n_bond_multi", "n_bond_kept", "max_size", "max_label")


def _round(a):
    """The library's round_ (half away from zero) as int64."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return engine.math(6, a.ravel()).reshape(a.shape).astype(np.int64)


def point_set(p, hs, which, select="all", mask=None):
    """The reference indices (0-based, increasing) of the set: the species, the selection and the mask."""
    n = hs.n_a + hs.n_b
    w = capi.px_which(which)
    keep = np.zeros(n, dtype=bool)
    if w in (capi.PX_A, capi.PX_AB):
        keep[:hs.n_a] = True
    if w in (capi.PX_B, capi.PX_AB):
        keep[hs.n_a:] = True
    keep &= np.asarray(selected(hs, select), dtype=bool)
    if mask is not None:
        keep &= np.asarray(mask) != 0
    return np.flatnonzero(keep)


def d2_matrix(p, hs, who):
    """D2[len(who), len(who)] int64 of the periodic integer displacements."""
    xy = positions(hs)[who]
    B = _round(np.array([p.box_x * 1024.0, p.box_y * 1024.0]))
    assert 1 <= B.min() and B.max() < 2 ** 31
    D2 = np.zeros((len(who), len(who)), dtype=np.int64)
    for ax in range(2):
        X = _round(xy[:, ax] * 1024.0)
        d = np.mod(X[None, :] - X[:, None], B[ax])  # numpy's mod is the floor modulus
        d = np.where(2 * d >= B[ax], d - B[ax], d)
        D2 += d * d
    return D2


def ref_prox_clusters(p, hs, which, eps, min_pts=1, select="all", mask=None, max_size=256, nbins=64):
    """(size_hist, nn_hist, nnd_hist, out dict, label, nn, kind) as Simulation.prox_clusters(per_protein=True)
    returns them (out as ProxOut.as_dict())."""
    n = hs.n_a + hs.n_b
    who = point_set(p, hs, which, select, mask)
    m = len(who)
    EPS = int(_round(np.array([eps * 1024.0]))[0])
    assert EPS >= 1
    D2 = d2_matrix(p, hs, who)
    near = D2 <= EPS * EPS
    np.fill_diagonal(near, False)  # j != i; coincident points stay neighbours
    N = near.sum(axis=1)
    core = N + 1 >= min_pts
    label, nn, kind = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    nn[who] = N
    # clusters: components of the cores, named by their smallest reference index
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    edges = 0
    ii, jj = np.nonzero(near & core[:, None] & core[None, :])
    for a, b in zip(ii.tolist(), jj.tolist()):
        if b < a:
            edges += 1
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    lab = np.zeros(m, dtype=np.int64)
    knd = np.ones(m, dtype=np.int64)
    for a in range(m):
        if core[a]:
            lab[a] = who[find(a)] + 1  # who is increasing: the smallest position is the smallest reference index
            knd[a] = 3
    for a in range(m):
        if core[a]:
            continue
        cand = np.flatnonzero(near[a] & core)
        if cand.size:
            best = min(cand.tolist(), key=lambda j: (int(D2[a, j]), int(who[j])))
            lab[a], knd[a] = lab[best], 2
    label[who], kind[who] = lab, knd
    # histograms
    nn_hist = np.bincount(np.minimum(N, NN_ROWS - 1), minlength=NN_ROWS).astype(np.int64)
    dr = eps / nbins
    E = [int(v) for v in _round(np.array([(float(k) * dr) * 1024.0 for k in range(nbins)]))]
    nnd_hist = np.zeros(nbins, dtype=np.int64)
    for a in np.flatnonzero(N > 0).tolist():
        M = int(D2[a][near[a]].min())
        nnd_hist[sum(1 for k in range(1, nbins) if E[k] * E[k] <= M)] += 1
    sizes = {}
    for L in lab[lab > 0].tolist():
        sizes[L] = sizes.get(L, 0) + 1
    size_hist = np.zeros(max_size + 1, dtype=np.int64)
    for s in sizes.values():
        size_hist[min(s, max_size)] += 1
    # purity against the bond graph
    c = engine.host_census(p, hs, 0, 0)[0][who].tolist()
    members, comp = {}, {}
    for a in range(m):
        comp.setdefault(c[a], []).append(int(lab[a]))
        if lab[a] > 0:
            members.setdefault(int(lab[a]), []).append(c[a])
    n_sel_c = {k: len(v) for k, v in comp.items()}
    pure = [L for L, cs in members.items() if len(cs) >= 2 and len(set(cs)) == 1]
    big = max(sizes.values()) if sizes else 0
    out = dict(n_sel=m, n_core=int(core.sum()), n_border=int((knd == 2).sum()), n_noise=int((knd == 1).sum()),
               n_alone=int((N == 0).sum()), n_clusters=len(sizes), n_multi=sum(1 for s in sizes.values() if s >= 2),
               sum_nn=int(N.sum()), n_core_edges=edges, n_pure=len(pure),
               n_whole=sum(1 for L in pure if sizes[L] == n_sel_c[members[L][0]]),
               n_bond_multi=sum(1 for v in comp.values() if len(v) >= 2),
               n_bond_kept=sum(1 for v in comp.values() if len(v) >= 2 and len(set(v)) == 1 and v[0] != 0),
               max_size=big, max_label=min([L for L, s in sizes.items() if s == big], default=0))
    return size_hist, nn_hist, nnd_hist, out, label, nn, kind


def same(got, want):
    """A prox_clusters(per_protein=True) result against another, or against ref_prox_clusters'."""
    d = want[3] if isinstance(want[3], dict) else want[3].as_dict()
    assert got[3].as_dict() == d
    for a, b in zip(got[:3] + got[4:], want[:3] + want[4:]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[0].sum() == got[3].n_clusters and got[1].sum() == got[3].n_sel
    assert got[2].sum() == got[3].n_sel - got[3].n_alone
    assert got[3].n_sel == got[3].n_core + got[3].n_border + got[3].n_noise


# ------------------------------------------------------------------ hand-made lines of ligands
def line_state(xs, order=None, n_a=1, box=3000.0, y=7.5, box_y=None):
    """Ligands on one line: position k (xs[k], y) holds ligand order[k] (0-based); one receptor far away."""
    n = len(xs)
    p = params(seed=5, n_a=n_a, n_b=n, box_x=box, box_y=box_y or box, box_z=250.0)
    hs = engine.host_init_random(p)
    order = np.arange(n) if order is None else np.asarray(order)
    x = np.zeros(n)
    x[order] = np.asarray(xs, dtype=np.float64)
    place_ligands(hs, x, np.full(n, y))
    return p, hs


BORDER_XS = [0.0, 5.0, 10.0, 25.0, 75.0, 90.0, 95.0, 100.0]
# the ligand at each of BORDER_XS: the core at 75 (ligand 5) has a smaller index than the core at 25 (ligand 6),
# but its cluster {5, 1, 4, 7} has the larger label (2 + 1) — the left one {0, 2, 3, 6} holds ligand 0 (label 2)
BORDER_ORDER = [0, 2, 3, 6, 5, 1, 4, 7]


def border_line(x_mid, order=BORDER_ORDER):
    """Cores at BORDER_XS (eps 30, min_pts 4: each has three neighbours at least) and ligand 8 at x_mid."""
    return line_state(BORDER_XS + [x_mid], list(order) + [8])
