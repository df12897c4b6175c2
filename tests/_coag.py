"""A plain-Python cluster growth recorder, written from the
definitions of include/kmc.h and not from csrc/kmc_coag.h: the bonds of a look
as Python sets of pairs, the three partitions by union-find, and the filing
cluster by cluster (the library files core by core).  Python ints throughout.
Also the hand-made sequence of looks with its values worked out by hand, and
the two ways the graph states of the other helpers are cut."""
import numpy as np

from _kmc import capi

COUNTERS = ("origin_step", "last_step", "n_updates", "max_size", "formed_rl", "formed_cis", "broken_rl", "broken_cis",
            "n_cores", "n_clusters", "cycles_closed", "cycles_opened", "max_cluster")
TABLES = ("merge", "frag", "merge_kind", "frag_kind", "merge_pieces", "frag_pieces", "merge_product", "frag_parent",
          "n_s", "expo")
ARRAYS = ("rl_lig", "cis_with", "prev_label")


def bonds(hs):
    """(R–L bonds, cis bonds) of a host state as sets of pairs (lo, hi) of 1-based reference indices."""
    na = hs.a_int.shape[1]
    rl, cis = set(), set()
    for i in range(na):
        lig, partner = int(hs.a_int[2, i]), int(hs.a_int[4, i])
        if lig:
            rl.add((i + 1, lig))
        if partner:
            cis.add((min(i + 1, partner), max(i + 1, partner)))
    return rl, cis


def partition(n, edges):
    """label[v] (1-based, index 0 unused) = the smallest member of v's component under `edges`."""
    parent = list(range(n + 1))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return [find(v) for v in range(n + 1)]


def members(label):
    m = {}
    for v in range(1, len(label)):
        m.setdefault(label[v], []).append(v)
    return m


def cycle_rank(n, edges):
    return len(edges) - n + len(members(partition(n, edges)))


class Recorder:
    def __init__(self, p, hs, max_size):
        self.na, self.n, self.S = p.n_a, p.n_a + p.n_b, int(max_size)
        self.rl, self.cis = bonds(hs)
        self.label = partition(self.n, self.rl | self.cis)
        s1 = self.S + 1
        self.t = {k: np.zeros((s1, s1), dtype=np.int64) for k in ("merge", "frag")}
        self.t.update({k: np.zeros((4, 4), dtype=np.int64) for k in ("merge_kind", "frag_kind")})
        self.t.update({k: np.zeros(9, dtype=np.int64) for k in ("merge_pieces", "frag_pieces")})
        self.t.update({k: np.zeros(s1, dtype=np.int64) for k in ("merge_product", "frag_parent", "expo")})
        self.expo2 = [[0] * s1 for _ in range(s1)]
        self.c = dict.fromkeys(COUNTERS, 0)
        self.c.update(origin_step=int(hs.step), last_step=int(hs.step), max_size=self.S)
        self.looks = [(int(hs.step), self._look())]  # (step, n_s) of every look: the exposures are recomputed from it

    def _look(self):
        sizes = [len(m) for m in members(self.label).values()]
        self.n_s = np.bincount(np.minimum(sizes, self.S), minlength=self.S + 1).astype(np.int64)
        self.c["n_clusters"], self.c["max_cluster"] = len(sizes), max(sizes)
        return self.n_s.copy()

    def _kind(self, piece):
        nr = sum(1 for v in piece if v <= self.na)
        nl = len(piece) - nr
        return {(1, 0): 0, (0, 1): 1, (2, 0): 2}.get((nr, nl), 3)

    def _file(self, side, which, label, core_label):
        """Every cluster of partition `label` that holds two or more cores files into the `side` tables."""
        cores = members(core_label)
        inside = {}
        for root in cores:
            inside.setdefault(label[root], []).append(root)
        whole = members(label)
        for lab, roots in inside.items():
            k = len(roots)
            if k < 2:
                continue
            self.t[side + "_pieces"][min(k, 8)] += 1
            self.t[which][min(len(whole[lab]), self.S)] += 1
            if k == 2:
                a, b = cores[roots[0]], cores[roots[1]]
                sa, sb = sorted((min(len(a), self.S), min(len(b), self.S)))
                self.t[side][sa, sb] += 1
                ka, kb = sorted((self._kind(a), self._kind(b)))
                self.t[side + "_kind"][ka, kb] += 1

    def update(self, hs):
        if int(hs.step) == self.c["last_step"]:  # a second update at the same step changes nothing but n_updates
            self.c["n_updates"] += 1
            return
        rl, cis = bonds(hs)
        e0, e1 = self.rl | self.cis, rl | cis
        kept = e0 & e1
        cur, core = partition(self.n, e1), partition(self.n, kept)
        self._file("frag", "frag_parent", self.label, core)
        self._file("merge", "merge_product", cur, core)
        c = self.c
        c["formed_rl"] += len(rl - self.rl)
        c["formed_cis"] += len(cis - self.cis)
        c["broken_rl"] += len(self.rl - rl)
        c["broken_cis"] += len(self.cis - cis)
        c["n_cores"] = len(members(core))
        c["cycles_closed"] += cycle_rank(self.n, e1) - cycle_rank(self.n, kept)
        c["cycles_opened"] += cycle_rank(self.n, e0) - cycle_rank(self.n, kept)
        dt, n = int(hs.step) - c["last_step"], [int(x) for x in self.n_s]
        for a in range(1, self.S + 1):
            self.t["expo"][a] += dt * n[a]
            self.expo2[a][a] += dt * (n[a] * (n[a] - 1) // 2)
            for b in range(a + 1, self.S + 1):
                self.expo2[a][b] += dt * n[a] * n[b]
        self.rl, self.cis, self.label = rl, cis, cur
        c["last_step"] = int(hs.step)
        c["n_updates"] += 1
        self.looks.append((int(hs.step), self._look()))

    def out(self) -> dict:
        return dict(self.c)

    def tables(self) -> dict:
        d = {k: v.copy() for k, v in self.t.items()}
        d["n_s"] = self.n_s.copy()
        d["expo2"] = [row[:] for row in self.expo2]
        return d

    def arrays(self) -> dict:
        rl_lig, cis_with = np.zeros(self.na, dtype=np.int32), np.zeros(self.na, dtype=np.int32)
        for r, lig in self.rl:
            rl_lig[r - 1] = lig
        for a, b in self.cis:
            cis_with[a - 1], cis_with[b - 1] = b, a
        return dict(rl_lig=rl_lig, cis_with=cis_with, prev_label=np.array(self.label[1:], dtype=np.int32))


def same_arrays(got, want: Recorder) -> bool:
    w = want.arrays()
    return all(np.array_equal(getattr(got, k), w[k]) for k in ARRAYS)


def table_differences(got, want: dict) -> list:
    """Names of the tables of a capi.CfTables that differ from a Recorder's tables() (or another as_dict())."""
    g = got.as_dict()
    bad = [k for k in TABLES if not np.array_equal(g[k], want[k])]
    if [list(r) for r in g["expo2"]] != [list(r) for r in want["expo2"]]:
        bad.append("expo2")
    return bad


def state(p, step, links):
    """A host state that holds only what the recorder reads: links[i] = (lig, site, cis) of receptor i + 1."""
    hs = capi.HostState(p.n_a, p.n_b)
    for i, (lig, site, cis) in enumerate(links):
        hs.a_int[2, i], hs.a_int[3, i], hs.a_int[4, i] = lig, site, cis
        hs.a_int[0, i], hs.a_int[1, i] = lig != 0, cis != 0
    hs.step = step
    return hs


def without_cis(hs, receptors):
    """A copy of hs with the cis bond of every listed receptor (1-based) removed, at both ends."""
    out = hs.copy()
    for r in receptors:
        partner = int(out.a_int[4, r - 1])
        assert partner, r
        for x in (r, partner):
            out.a_int[1, x - 1] = 0
            out.a_int[4, x - 1] = 0
    return out


def cis_bonds(hs):
    return sorted(bonds(hs)[1])


def chain_cuts(p, seed=5, at=(100, 300, 450)):
    """Receptors of _analysis.chain_state(seed) whose cis bonds lie at the chain positions `at` (the bond π(2k) –
    π(2k+1) after ligand k): without them the chain is four pieces of 300, 600, 450 and 450 proteins."""
    pi = np.random.default_rng(seed).permutation(p.n_a) + 1
    return [int(pi[2 * k - 1]) for k in at]


# ---- the hand-made sequence: receptors 1..6, ligands 7, 8, 9, S = 5; (lig, site, cis) per receptor at each look
F = (0, 0, 0)
HAND_S = 5
SEQUENCE = [
    # begin: {1, 2, 7} and six single proteins
    (100, [(7, 2, 0), (7, 3, 0), F, F, F, F]),
    # a binary merger: receptor 3 joins {1, 2, 7}: sizes (1, 3), kinds (receptor, other)
    (103, [(7, 2, 0), (7, 3, 0), (7, 4, 0), F, F, F]),
    # a binary fragmentation: receptor 1 leaves {1, 2, 3, 7}, filed by the core {2, 3, 7} (root 2, the label is 1);
    # receptor 2 moves to another site of ligand 7: a kept edge
    (104, [F, (7, 2, 0), (7, 4, 0), F, F, F]),
    # a 4-piece merger: {2, 3, 7}, 4, 5 and 8 form one cluster of 6 (index 5: the clamp) over 4-8, 5-8 and 3~4
    (110, [F, (7, 2, 0), (7, 4, 4), (8, 2, 3), (8, 3, 0), F]),
    # a 3-piece fragmentation of that cluster: 3~4 and 5-8 break; {2, 3, 7}, {4, 8}, {5}
    (111, [F, (7, 2, 0), (7, 4, 0), (8, 2, 0), F, F]),
    # a fragmentation and a merger of different clusters in one look: {2, 3, 7} loses 2, {4, 8} gains 5
    (115, [F, F, (7, 4, 0), (8, 2, 0), (8, 3, 0), F]),
    # {4, 5, 8} loses 5 and gains 6 in one look: a fragmentation (1, 2) and a merger (1, 2) of the same core;
    # receptor 3 swaps ligand 7 for ligand 9: {3, 7} falls into (1, 1), kinds (receptor, ligand), {3, 9} forms
    (117, [F, F, (9, 2, 0), (8, 2, 0), F, (8, 3, 0)]),
    # a cycle closes: 4 ~ 6 inside {4, 6, 8}; no cluster changes
    (120, [F, F, (9, 2, 0), (8, 2, 6), F, (8, 3, 4)]),
    # and opens again: 6-8 breaks, {4, 6, 8} holds over 4 ~ 6
    (121, [F, F, (9, 2, 0), (8, 2, 6), F, (0, 0, 4)]),
]
# after the update at each step: (formed_rl, formed_cis, broken_rl, broken_cis, n_cores, n_clusters, closed, opened,
# max_cluster), n_s[1..5], expo[1..5]
HAND_LOOKS = {
    103: ((1, 0, 0, 0, 7, 6, 0, 0, 4), [5, 0, 0, 1, 0], [18, 0, 3, 0, 0]),
    104: ((1, 0, 1, 0, 7, 7, 0, 0, 3), [6, 0, 1, 0, 0], [23, 0, 3, 1, 0]),
    110: ((3, 1, 1, 0, 7, 4, 0, 0, 6), [3, 0, 0, 0, 1], [59, 0, 9, 1, 0]),
    111: ((3, 1, 2, 1, 6, 6, 0, 0, 3), [4, 1, 1, 0, 0], [62, 0, 9, 1, 1]),
    115: ((4, 1, 3, 1, 7, 6, 0, 0, 3), [4, 1, 1, 0, 0], [78, 4, 13, 1, 1]),
    117: ((6, 1, 5, 1, 8, 6, 0, 0, 3), [4, 1, 1, 0, 0], [86, 6, 15, 1, 1]),
    120: ((6, 2, 5, 1, 6, 6, 1, 0, 3), [4, 1, 1, 0, 0], [98, 9, 18, 1, 1]),
    121: ((6, 2, 6, 1, 6, 6, 1, 1, 3), [4, 1, 1, 0, 0], [102, 10, 19, 1, 1]),
}
# the tables after the last look: {table: {index: count}}, everything else zero
HAND_TABLES = {
    "merge": {(1, 3): 1, (1, 2): 2, (1, 1): 1},
    "merge_kind": {(0, 3): 3, (0, 1): 1},
    "merge_pieces": {2: 4, 4: 1},
    "merge_product": {4: 1, 5: 1, 3: 2, 2: 1},
    "frag": {(1, 3): 1, (1, 2): 2, (1, 1): 1},
    "frag_kind": {(0, 3): 3, (0, 1): 1},
    "frag_pieces": {2: 4, 3: 1},
    "frag_parent": {4: 1, 5: 1, 3: 2, 2: 1},
}
HAND_EXPO2 = {(1, 1): 208, (1, 2): 40, (1, 3): 94, (1, 4): 5, (1, 5): 3, (2, 3): 10}
