"""Python reference of the ligand network and its rings (include/kmc.h,
DESIGN.md §17), shared by test_rings_host.py and test_gpu_rings.py and
independent of the C code: the bridges are built from the HostState arrays, the
rings are found by a plain depth-first search from every ligand in both
directions and de-duplicated as frozensets of bridges (deliberately not the
library's rule of the smallest ligand and the ordered site pair), the chord rule
is set membership.  Integers, compared by exact equality.  Also the hand-built
network states both test files use."""
import numpy as np

from _analysis import np_components
from _bondorder import bind_network
from _kmc import capi, engine, params

RING_MAX = 12
COUNTERS = ("n_bridges", "n_loops", "n_half", "n_free_dimers", "n_vertices", "n_net_components", "cycle_rank")


# ------------------------------------------------------------------ the reference
def hop(hs, b, s):
    """(l, s') of ligand b (0-based), site s: l the 0-based ligand, None without a bridge; 'half' for a half bridge."""
    na = hs.n_a
    r = int(hs.b_int[4 + s - 1, b])
    if r == 0:
        return None
    r2 = int(hs.a_int[4, r - 1])
    if r2 == 0:
        return None
    l = int(hs.a_int[2, r2 - 1])
    if l == 0:
        return "half"
    return l - na - 1, int(hs.a_int[3, r2 - 1])


def bridges(hs):
    """(the set of bridges, each the frozenset of its two ends (b, s) — a loop's ends share b —, the number of half
    bridges)."""
    out, half = set(), 0
    for b in range(hs.n_b):
        for s in (2, 3, 4):
            h = hop(hs, b, s)
            if h == "half":
                half += 1
            elif h is not None:
                out.add(frozenset({(b, s), h}))
    return out, half


def ref_network(hs):
    """dict of the counters, rec[4], lig_hist[4, 4], adj_lig / adj_site[n_b, 3]."""
    na, nb = hs.n_a, hs.n_b
    E, half = bridges(hs)
    nei2, nei3 = hs.a_int[2], hs.a_int[4]
    rec = np.bincount((nei2 != 0) + 2 * (nei3 != 0), minlength=4).astype(np.int64)
    free = sum(1 for i in range(na) if nei3[i] and not nei2[i] and not nei2[nei3[i] - 1] and i + 1 < nei3[i])
    adj_lig, adj_site = np.zeros((nb, 3), dtype=np.int32), np.zeros((nb, 3), dtype=np.int32)
    hist = np.zeros((4, 4), dtype=np.int64)
    ends = np.zeros(nb, dtype=np.int64)
    for b in range(nb):
        for s in (2, 3, 4):
            h = hop(hs, b, s)
            if h not in (None, "half"):
                adj_lig[b, s - 2], adj_site[b, s - 2] = h[0] + 1, h[1]
                ends[b] += 1
        hist[int((hs.b_int[5:8, b] != 0).sum()), ends[b]] += 1
    label = np_components(hs)
    nv = int((ends > 0).sum())
    ncomp = len(set(label[na:][ends > 0].tolist()))
    loops = sum(1 for e in E if len({b for b, _ in e}) == 1)
    return dict(n_bridges=len(E), n_loops=loops, n_half=half, n_free_dimers=free, n_vertices=nv,
                n_net_components=ncomp, cycle_rank=len(E) - nv + ncomp, rec=rec.tolist(), lig_hist=hist,
                adj_lig=adj_lig, adj_site=adj_site)


def ref_rings(hs, max_len):
    """(counts[2, RING_MAX + 1] int64, member[2, n_b] uint32): every closed walk over distinct ligands and distinct
    bridges, from every ligand, as the set of its bridges."""
    nb = hs.n_b
    E, _ = bridges(hs)
    adj = [[] for _ in range(nb)]  # (bridge, the ligand at its other end)
    for e in E:
        ligs = sorted({b for b, _ in e})
        if len(ligs) == 1:
            adj[ligs[0]].append((e, ligs[0]))
        else:
            adj[ligs[0]].append((e, ligs[1]))
            adj[ligs[1]].append((e, ligs[0]))
    rings = {}  # bridge set -> ligand set

    def walk(v0, cur, path, used):
        for e, w in adj[cur]:
            if e in used:
                continue
            if w == v0:
                rings[frozenset(used + [e])] = frozenset(path)
            elif w not in path and len(path) < max_len:
                walk(v0, w, path + [w], used + [e])

    for v in range(nb):
        walk(v, v, [v], [])
    counts = np.zeros((2, RING_MAX + 1), dtype=np.int64)
    member = np.zeros((2, nb), dtype=np.uint32)
    for es, vs in rings.items():
        L = len(es)
        assert L == len(vs) and L <= max_len
        chord = any(e not in es and {b for b, _ in e} <= vs for e in E)
        for row in (0,) if chord else (0, 1):
            counts[row, L] += 1
            member[row, list(vs)] |= np.uint32(1 << L)
    return counts, member


def net_dict(out, hist, adj_lig, adj_site):
    """What engine.host_network / Simulation.network return, shaped as ref_network's dict."""
    d = out.as_dict()
    d.update(lig_hist=hist, adj_lig=adj_lig, adj_site=adj_site)
    return d


def same_network(got: dict, want: dict) -> bool:
    return all(np.array_equal(got[k], want[k]) for k in want) and set(got) == set(want)


# ------------------------------------------------------------------ hand-built states
def blank(n_b, n_a, seed=3):
    """A random placement of n_a receptors and n_b ligands without a bond, to be bound by hand.  No layer under
    test reads a position, so the bonds need not be within reach."""
    side = 400.0 * max(4.0, float(np.ceil(np.sqrt(n_a + n_b))))
    p = params(seed=seed, n_a=n_a, n_b=n_b, box_x=side, box_y=side, box_z=1000.0)
    hs = engine.host_init_random(p)
    hs.a_int[:] = 0
    hs.b_int[:] = 0
    return p, hs


def network_state(n_b, edges, half=(), extra_receptors=0, free_dimers=0, single=(), seed=3):
    """n_b ligands bridged by `edges` = [(b, s, b2, s2), ...] (0-based ligands, sites 2..4), with half bridges
    `half` = [(b, s), ...], `single` = [(b, s), ...] receptors bound to a ligand without a cis partner, free_dimers
    ligand-free cis pairs and extra_receptors free receptors.  The receptors are taken in a seeded random order."""
    n_a = 2 * len(edges) + 2 * len(half) + len(single) + 2 * free_dimers + extra_receptors
    p, hs = blank(n_b, max(n_a, 1), seed)
    rec = np.random.default_rng(seed).permutation(hs.n_a).tolist()
    bind_network(hs, [(b, s, rec.pop(), rec.pop(), b2, s2) for b, s, b2, s2 in edges])
    bind_network(hs, [(b, s, rec.pop(), rec.pop(), -1, 0) for b, s in half])
    for b, s in single:
        r = rec.pop()
        hs.a_int[0, r] = 1
        hs.a_int[2, r] = hs.n_a + b + 1
        hs.a_int[3, r] = s
        hs.b_int[s - 1, b] = 1
        hs.b_int[4 + s - 1, b] = r + 1
    for _ in range(free_dimers):
        r, r2 = rec.pop(), rec.pop()
        hs.a_int[1, r] = hs.a_int[1, r2] = 1
        hs.a_int[4, r] = r2 + 1
        hs.a_int[4, r2] = r + 1
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs


def cycle(L, first=0):
    """The edges of one ring over ligands first .. first + L - 1: site 2 to the next ligand's site 3 (a loop for L = 1;
    for L = 2 the second bridge runs back the same way)."""
    return [(first + i, 2, first + (i + 1) % L, 3) for i in range(L)]


K4 = [(0, 2, 1, 2), (0, 3, 2, 2), (0, 4, 3, 2), (1, 3, 2, 3), (1, 4, 3, 3), (2, 4, 3, 4)]
THETA = [(0, 2, 1, 2), (1, 3, 2, 2), (2, 3, 5, 2),   # two trivalent ligands 0 and 5 joined by three paths:
         (0, 3, 3, 2), (3, 3, 5, 3),                 # over 1, 2; over 3; over 4
         (0, 4, 4, 2), (4, 3, 5, 4)]

HAND = {
    "none": dict(n_b=5, edges=[], single=[(0, 2), (3, 4)], free_dimers=2, extra_receptors=3),
    "one_ligand": dict(n_b=1, edges=[], extra_receptors=2),
    "loop": dict(n_b=3, edges=[(1, 2, 1, 4), (1, 3, 2, 2)], half=[(0, 3)]),
    "double": dict(n_b=4, edges=[(0, 2, 2, 4), (0, 4, 2, 3), (2, 2, 3, 2)]),
    "triple": dict(n_b=3, edges=[(0, 2, 2, 4), (0, 3, 2, 3), (0, 4, 2, 2)]),
    "triangle": dict(n_b=4, edges=cycle(3, 1), extra_receptors=1),
    "k4": dict(n_b=4, edges=K4),
    "theta": dict(n_b=6, edges=THETA),
    # a hexagon with a pendant tree (6 - 7, 7 - 8, 7 - 9), two half bridges, a receptor without partner, a free dimer
    "pendant": dict(n_b=11, edges=cycle(6) + [(0, 4, 6, 2), (6, 3, 7, 2), (7, 3, 8, 2), (7, 4, 9, 3)],
                    half=[(3, 4), (8, 4)], single=[(9, 2), (10, 3)], free_dimers=1),
}


def hand_state(name):
    return network_state(**HAND[name])


def permuted(p, hs, seed=23):
    """The same network with the receptors and the ligands renumbered at random: (state, pl) with pl[old ligand] =
    new ligand."""
    na, nb = hs.n_a, hs.n_b
    rng = np.random.default_rng(seed)
    pa, pl = rng.permutation(na), rng.permutation(nb)
    out = capi.HostState(na, nb)
    out.ra[:, pa] = hs.ra
    out.rb[:, pl] = hs.rb
    a, b = hs.a_int.copy(), hs.b_int.copy()
    a[2] = np.where(a[2] != 0, na + pl[np.maximum(a[2] - na - 1, 0)] + 1, 0)
    a[4] = np.where(a[4] != 0, pa[np.maximum(a[4] - 1, 0)] + 1, 0)
    for row in (4, 5, 6, 7):
        b[row] = np.where(b[row] != 0, pa[np.maximum(b[row] - 1, 0)] + 1, 0)
    out.a_int[:, pa] = a
    out.b_int[:, pl] = b
    out.counters[:] = hs.counters
    out.step = hs.step
    assert engine.host_validate(p, out) == capi.KMC_OK
    return out, pl


# the brick-wall lattice of _geometry.lattice_state(keep_x, keep_y): lengths -> (all, chordless), and the cycle rank
LATTICE = {
    (True, True): ({6: (1024, 1024), 10: (3072, 0), 12: (2048, 2048)}, 1025),
    (False, False): ({6: (961, 961), 10: (2760, 0), 12: (1800, 1800)}, 961),
    (True, False): ({6: (992, 992), 10: (2912, 0), 12: (1920, 1920)}, 993),
}


def lattice_counts(key):
    counts = np.zeros((2, RING_MAX + 1), dtype=np.int64)
    for L, (a, c) in LATTICE[key][0].items():
        counts[0, L], counts[1, L] = a, c
    return counts
