"""Helpers of test_big_complexes_fixture.py and test_gpu_complex_sizes.py: the
fixture states at which the step engine's complex chain changes code path
(tests/golden/make_big_complexes.py writes them) and a plain
union-find over a state's link arrays, independent of the library's census."""
import json
import os

import numpy as np

from _kmc import GOLDEN, capi, params

FIXTURE = os.path.join(GOLDEN, "big_complexes.npz")
CXL = 16       # kmc_kernels.hip: members of a complex on the streamed / staged path
BFS_QCAP = 32  # kmc_kernels.hip: members of a component that fit bfs_one's LDS queue


def components(hs) -> np.ndarray:
    """root[i] of protein i (0-based; receptors, then ligands): the smallest index of its component."""
    na, nb = hs.n_a, hs.n_b
    parent = np.arange(na + nb)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    pairs = [(i, int(v) - 1) for row in (2, 4) for i, v in enumerate(hs.a_int[row]) if v]
    pairs += [(na + b, int(v) - 1) for row in (5, 6, 7) for b, v in enumerate(hs.b_int[row]) if v]
    for i, j in pairs:
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(na + nb)])


def sizes(hs) -> list:
    """Member counts of the components with a ligand and more than one member (the engine's complexes), descending."""
    root = components(hs)
    n = np.bincount(root, minlength=hs.n_a + hs.n_b)
    nl = np.bincount(root[hs.n_a:], minlength=hs.n_a + hs.n_b)
    return sorted(n[(n > 1) & (nl > 0)].tolist(), reverse=True)


def ligands_of_largest(hs) -> int:
    """Ligands of the largest component: with two or more, the BFS enters it from a ligand that is not its root."""
    root = components(hs)
    n = np.bincount(root, minlength=hs.n_a + hs.n_b)
    return int(np.count_nonzero(root[hs.n_a:] == int(np.argmax(n))))


def bond_links(hs):
    """The state's links as a set of (lower, higher) index pairs."""
    na = hs.n_a
    out = set()
    for row in (2, 4):
        for i, v in enumerate(hs.a_int[row]):
            if v:
                out.add((min(i, int(v) - 1), max(i, int(v) - 1)))
    for row in (5, 6, 7):
        for b, v in enumerate(hs.b_int[row]):
            if v:
                out.add((min(na + b, int(v) - 1), max(na + b, int(v) - 1)))
    return out


def names():
    with np.load(FIXTURE, allow_pickle=False) as g:
        return json.loads(str(g["names"]))


def load(name, **overrides):
    """(params, state) of fixture state `name`; overrides replace stored parameters."""
    with np.load(FIXTURE, allow_pickle=False) as g:
        kw = json.loads(str(g[name + "_params"]))
        kw.update(overrides)
        p = params(**kw)
        hs = capi.HostState(p.n_a, p.n_b)
        for f in ("ra", "rb", "a_int", "b_int", "counters"):
            getattr(hs, f)[...] = g[f"{name}_{f}"]
        hs.step = int(g[name + "_step"])
    return p, hs


def stored(key):
    with np.load(FIXTURE, allow_pickle=False) as g:
        return g[key].copy()


def break_and_merge(prev, cur, limit=CXL):
    """(breaks, merges) between two consecutive states: components of more than `limit` members in prev that lost a
    link and left only pieces of at most `limit`; components of more than `limit` in cur whose members all were in
    components of at most `limit`."""
    rp, rc = components(prev), components(cur)
    sp, sc = np.bincount(rp)[rp], np.bincount(rc)[rc]
    lost = bond_links(prev) - bond_links(cur)
    breaks = sum(1 for r in {int(rp[i]) for i, _ in lost} if sp[r] > limit and sc[rp == r].max() <= limit)
    merges = sum(1 for r in np.unique(rc[sc > limit]) if sp[rc == r].max() <= limit)
    return breaks, merges


def neighbours(hs, x):
    """The bonded neighbours of protein x (0-based) in the engine's BFS order (nbrs3): a receptor's ligand, then its
    cis partner; a ligand's receptors at sites 2, 3, 4."""
    na = hs.n_a
    v = [hs.a_int[2, x], hs.a_int[4, x]] if x < na else [hs.b_int[r, x - na] for r in (5, 6, 7)]
    return [int(y) - 1 for y in v if y]


def expected_overflow(hs) -> int:
    """Ligands whose BFS fills the BFS_QCAP queue, meets one more member and has seen no lower ligand by then: the
    entries bfs_one appends to the overflow list on a step that rebuilds every complex (reference indices; the
    state's own numbering, which set_state keeps as the proteins' identities)."""
    na, n = hs.n_a, 0
    for b in range(hs.n_b):
        q = [na + b]
        head = 0
        while head < len(q):
            for v in neighbours(hs, q[head]):
                if v in q:
                    continue
                if len(q) == BFS_QCAP:
                    n += not any(na <= m < na + b for m in q + [v])
                    head = len(q)
                    break
                q.append(v)
            head += 1
    return n


def unit_rows(row_len, members) -> dict:
    """{ligand: its member row as bytes} of kmc_get_clusters' / Oracle.clusters' format (rows and member order)."""
    off = np.concatenate([[0], np.cumsum(row_len)])
    return {int(b): members[off[b]:off[b + 1]].tobytes() for b in np.flatnonzero(row_len > 0)}


def changed_sizes(prev, cur) -> list:
    """Member counts of the complexes of prev (components with a ligand and more than one member) of which a bead
    differs in cur: a move that was committed."""
    na = prev.n_a
    root = components(prev)
    out = []
    for r in np.unique(root[na:]):
        m = np.flatnonzero(root == r)
        a, b = m[m < na], m[m >= na] - na
        if m.size > 1 and not (np.array_equal(prev.ra[:, a], cur.ra[:, a]) and np.array_equal(prev.rb[:, b], cur.rb[:, b])):
            out.append(int(m.size))
    return out
