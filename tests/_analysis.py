"""numpy references of the structure analysis (include/kmc.h),
shared by test_analysis_host.py and test_gpu_analysis.py: a plain union-find
over a host state's ints and a brute-force O(n²) pair loop.  Integer results,
compared by exact equality."""
import numpy as np

from _kmc import capi, engine, params

SUMMARY = ("n_components", "n_complexes", "proteins_in_complexes", "n_cis_dimers", "max_size", "max_receptors",
           "max_ligands", "max_label")


def np_components(hs) -> np.ndarray:
    """label[i] = smallest reference index (1-based) of protein i+1's component."""
    na, nb = hs.n_a, hs.n_b
    parent = list(range(na + nb))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    links = [(i, int(v)) for row in (2, 4) for i, v in enumerate(hs.a_int[row]) if v]          # nei2, nei3
    links += [(na + b, int(v)) for row in (5, 6, 7) for b, v in enumerate(hs.b_int[row]) if v]  # nei2..4
    for i, v in links:
        a, b = find(i), find(v - 1)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) + 1 for i in range(na + nb)], dtype=np.int32)


def np_census(hs, label, max_r, max_l):
    """(hist[max_r + 1, max_l + 1], summary dict) from the labels."""
    na, n = hs.n_a, hs.n_a + hs.n_b
    nr = np.bincount(label[:na] - 1, minlength=n)
    nl = np.bincount(label[na:] - 1, minlength=n)
    roots = np.flatnonzero(label == np.arange(1, n + 1))
    assert np.array_equal(roots, np.flatnonzero(nr + nl))
    r, l = nr[roots], nl[roots]
    size = r + l
    hist = np.zeros((max_r + 1, max_l + 1), dtype=np.int64)
    np.add.at(hist, (np.minimum(r, max_r), np.minimum(l, max_l)), 1)
    cx = (l >= 1) & (size > 1)
    big = int(np.argmax(size))  # the first (smallest label) of the largest
    summary = dict(n_components=len(roots), n_complexes=int(cx.sum()), proteins_in_complexes=int(size[cx].sum()),
                   n_cis_dimers=int(((l == 0) & (r == 2)).sum()), max_size=int(size[big]), max_receptors=int(r[big]),
                   max_ligands=int(l[big]), max_label=int(roots[big]) + 1)
    return hist, summary


def xy(hs, which):
    """(x, y) of bead [1][1] of the i side and the j side of species pair `which`."""
    a = np.stack([hs.ra[0], hs.ra[1]], axis=1)
    b = np.stack([hs.rb[0], hs.rb[1]], axis=1)
    return {"AA": (a, a), "AB": (a, b), "BB": (b, b)}[which]


def np_d2(hs, p, which) -> np.ndarray:
    """Squared lateral distances of all pairs, brute force, with the expressions
    of include/kmc.h: round_ is the library's (half away from zero; np.round
    rounds half to even).  AA / BB: each unordered pair once."""
    pi, pj = xy(hs, which)
    d = pi[:, None, :] - pj[None, :, :]
    box = (p.box_x, p.box_y)
    for c in (0, 1):
        q = d[:, :, c] / box[c]
        d[:, :, c] = d[:, :, c] - box[c] * engine.math(6, q.ravel()).reshape(q.shape)
    d2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]
    return d2[np.triu_indices(len(pi), k=1)] if which != "AB" else d2.ravel()


def np_bin(d2, r_max, nbins) -> np.ndarray:
    """counts[k], k = #{m in 1..nbins : edges2[m] <= d2}, counted when k < nbins."""
    dr = r_max / nbins
    m = np.arange(nbins + 1, dtype=np.float64)
    edges2 = (m * dr) * (m * dr)
    k = np.searchsorted(edges2[1:], d2, side="right")
    return np.bincount(k[k < nbins], minlength=nbins).astype(np.int64)


def chain_state(seed=5):
    """One component of 1200 receptors and 600 ligands: ligand k binds receptors
    π(2k-1), π(2k) at sites 2 and 3, π(2k) is cis-bound to π(2k+1); π is a
    seeded permutation, so the smallest label has to travel both ways."""
    p = params(seed=seed, n_a=1200, n_b=600, box_x=6000.0, box_y=6000.0, box_z=1000.0)
    hs = engine.host_init_random(p)
    na, nb = p.n_a, p.n_b
    pi = np.random.default_rng(seed).permutation(na) + 1  # pi[m-1] = π(m), 1-based receptors
    hs.a_int[:] = 0
    hs.b_int[:] = 0
    for k in range(1, nb + 1):
        for site, rec in ((2, pi[2 * k - 2]), (3, pi[2 * k - 1])):
            hs.b_int[site - 1, k - 1] = 1
            hs.b_int[4 + site - 1, k - 1] = rec
            hs.a_int[0, rec - 1] = 1          # st2
            hs.a_int[2, rec - 1] = na + k     # nei2
            hs.a_int[3, rec - 1] = site       # nei4: the ligand's site
        if k < nb:
            u, v = pi[2 * k - 1], pi[2 * k]   # π(2k) – π(2k+1)
            hs.a_int[1, u - 1] = hs.a_int[1, v - 1] = 1
            hs.a_int[4, u - 1] = v
            hs.a_int[4, v - 1] = u
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs


def summary_dict(c) -> dict:
    return {k: int(getattr(c, k)) for k in SUMMARY}
