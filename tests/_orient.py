"""Python reference of the orientation layer (include/kmc.h),
shared by test_orient_host.py and test_gpu_orient.py and independent of the C
code: the vectors in numpy int64, every sum in Python integers, round_ through
engine.math (the host kmc_math.h) as _lagcorr.py does, and a schedule of its own
written from the definitions of the header's comment — each stored origin
carries the update it was stored at, and every correlation asserts that the
slot the definition names holds the origin of update n - j 2^l.  Every
comparison against it is exact equality."""
import numpy as np

from _kmc import capi, engine

CLASSES, VECS = 5, 2
LIMIT = 1 << 16
BAD = 1 << 63
COUNTS = ("n_all", "n_clean")
SUMS = ("s1_all", "s1_clean", "s2_clean")


def _round(a):
    """The library's round_ (half away from zero; np.round rounds half to even)."""
    return engine.math(6, np.ascontiguousarray(a, dtype=np.float64).ravel()).reshape(np.shape(a))


def _q(x):
    return _round(np.asarray(x, dtype=np.float64) * 1024.0).astype(np.int64)


def _bead_a(hs, j, k):
    """q of receptor bead [j][k]: [n_a, 3]."""
    r = ((j - 1) * 4 + (k - 1)) * 3
    return _q(np.stack([hs.ra[r], hs.ra[r + 1], hs.ra[r + 2]], axis=1))


def _bead_b(hs, j, k):
    r = ((j - 1) * 2 + (k - 1)) * 3
    return _q(np.stack([hs.rb[r], hs.rb[r + 1], hs.rb[r + 2]], axis=1))


def vectors(hs):
    """(U[N, 2, 3] int64: vector v of protein i (v = 1 of a receptor is zero), chi[N], bad[N], Z[n_b], for a state."""
    n_a, n_b = hs.n_a, hs.n_b
    U = np.zeros((n_a + n_b, VECS, 3), dtype=np.int64)
    H = _bead_a(hs, 3, 2) - _bead_a(hs, 3, 1)
    H[:, 2] = 0  # the xy projection
    U[:n_a, 0] = H
    o = _bead_b(hs, 1, 1)
    N, A, Cv = _bead_b(hs, 1, 2) - o, _bead_b(hs, 2, 1) - o, _bead_b(hs, 3, 1) - o
    U[n_a:, 0], U[n_a:, 1] = N, A
    bad = np.zeros(n_a + n_b, dtype=bool)
    bad[:n_a] = (np.abs(H) >= LIMIT).any(axis=1)
    bad[n_a:] = (np.abs(N) >= LIMIT).any(axis=1) | (np.abs(A) >= LIMIT).any(axis=1) | (np.abs(Cv) >= LIMIT).any(axis=1)
    chi = np.zeros(n_a + n_b, dtype=np.int64)
    # the triple product is below 2^51 for a ligand that is not bad: exact in int64 (a bad one's is discarded)
    t = (N * np.cross(A, Cv)).sum(axis=1)
    chi[n_a:] = np.where(bad[n_a:], 0, np.sign(t))
    return U, chi, bad, o[:, 2]


def pack(U, bad, n_a):
    """The packed words [n_a + 2 n_b] of vectors(): headings, axes, arms; BAD for a bad protein."""
    def word(v):
        w = 0
        for k in range(3):
            w |= (int(v[k]) & 0x1FFFFF) << 21 * k
        return w
    n = len(U)
    out = [BAD if bad[i] else word(U[i, 0]) for i in range(n_a)]
    out += [BAD if bad[i] else word(U[i, 0]) for i in range(n_a, n)]
    out += [BAD if bad[i] else word(U[i, 1]) for i in range(n_a, n)]
    return np.array(out, dtype=np.uint64)


def links(hs) -> np.ndarray:
    """l[N, 3] as the tracker names them: receptor nei2, nei4, nei3; ligand nei2..4; a link out of range is none."""
    n = hs.n_a + hs.n_b
    a = np.stack([hs.a_int[2], hs.a_int[3], hs.a_int[4]], axis=1).astype(np.int64)
    b = np.stack([hs.b_int[5], hs.b_int[6], hs.b_int[7]], axis=1).astype(np.int64)
    for arr, cols in ((a, (0, 2)), (b, (0, 1, 2))):
        for c in cols:
            arr[:, c] = np.where((arr[:, c] >= 1) & (arr[:, c] <= n), arr[:, c], 0)
    return np.concatenate([a, b])


def classes(l, n_a) -> np.ndarray:
    c = np.empty(len(l), dtype=np.int64)
    c[:n_a] = np.where(l[:n_a, 0] != 0, 2, np.where(l[:n_a, 2] != 0, 1, 0))
    c[n_a:] = np.where((l[n_a:] != 0).any(axis=1), 4, 3)
    return c


def isum(d: np.ndarray) -> int:
    """The sum of int64 values of magnitude below 2^34 as a Python int (fewer than 2^28 of them: no wrap)."""
    assert len(d) < 1 << 28 and (np.abs(d) < 1 << 34).all()
    return int(np.sum(d, dtype=np.int64))


def isum_sq(d: np.ndarray) -> int:
    """The sum of d^2 (below 2^68 each) as a Python int: |d| = h 2^20 + l, with h^2, h l and l^2 summed apart in int64
    (h < 2^14, l < 2^20; fewer than 2^22 terms: no wrap)."""
    assert len(d) < 1 << 22 and (np.abs(d) < 1 << 34).all()
    m = np.abs(d)
    h, l = m >> 20, m & ((1 << 20) - 1)
    return (int(np.sum(h * h)) << 40) + (int(np.sum(h * l)) << 21) + int(np.sum(l * l))


def n_rows(L: int, P: int) -> int:
    return P + (L - 1) * (P // 2)


def row_of(l: int, j: int, P: int) -> int:
    return j - 1 if l == 0 else P + (l - 1) * (P // 2) + (j - P // 2 - 1)


class RefRot:
    """The recorder of include/kmc.h on host states.  log (when a list): (n, n_k, row, i, v, clean) of every pair."""

    def __init__(self, p, hs, every, levels, slots, log=None):
        self.p, self.every, self.L, self.P = p, every, levels, slots
        self.rows = n_rows(levels, slots)
        self.n_a = hs.n_a
        self.U, self.chi, self.bad, _ = vectors(hs)
        self.links = links(hs)
        self.last_event = np.zeros(len(self.U), dtype=np.int64)
        self.n = 0
        self.origin_step = self.last_step = hs.step
        # ring[l][slot] = (the update it was stored at, U then, bad then); begin stores update 0 in slot 0 of every level
        self.ring = [[None] * slots for _ in range(levels)]
        for l in range(levels):
            self.ring[l][0] = (0, self.U.copy(), self.bad.copy())
        self.n_pairs = [0] * self.rows
        self.t = {k: [[[0] * VECS for _ in range(CLASSES)] for _ in range(self.rows)] for k in COUNTS + SUMS}
        self.log = log
        self.last_tasks = self.last_events = self.last_flips = self.last_bad = 0
        self.flips_total = 0

    def update(self, hs):
        assert hs.step == self.last_step + self.every
        self.n += 1
        n, L, P = self.n, self.L, self.P
        self.U, chi, self.bad, _ = vectors(hs)
        l_now = links(hs)
        flip = chi != self.chi
        ev = flip | (l_now != self.links).any(axis=1)
        self.links, self.chi = l_now, chi
        self.last_event[ev] = n
        self.last_events, self.last_flips, self.last_bad = int(ev.sum()), int(flip.sum()), int(self.bad.sum())
        self.flips_total += self.last_flips
        cls = classes(l_now, self.n_a)
        self.last_tasks = 0
        for l in range(L):
            if n % 2 ** l != 0:
                continue
            t = n >> l
            for j in (range(1, P + 1) if l == 0 else range(P // 2 + 1, P + 1)):
                if j > t:
                    continue
                nk, O, obad = self.ring[l][(t - j) % P]
                assert nk == n - j * 2 ** l, (n, l, j, nk)
                self._file(row_of(l, j, P), nk, O, obad, cls)
                self.last_tasks += 1
        for l in range(L):
            if n % 2 ** l == 0:
                self.ring[l][(n >> l) % P] = (n, self.U.copy(), self.bad.copy())
        self.last_step = hs.step

    def _file(self, row, nk, O, obad, cls):
        self.n_pairs[row] += 1
        filed = ~self.bad & ~obad
        clean = filed & (self.last_event <= nk)
        for v in range(VECS):
            d = (self.U[:, v] * O[:, v]).sum(axis=1)  # |d| < 3 2^32 where filed
            for c in range(CLASSES):
                if v == 1 and c < 3:
                    continue
                a, k = filed & (cls == c), clean & (cls == c)
                cell = lambda name: self.t[name][row][c]
                cell("n_all")[v] += int(a.sum())
                cell("n_clean")[v] += int(k.sum())
                cell("s1_all")[v] += isum(d[a])
                cell("s1_clean")[v] += isum(d[k])
                cell("s2_clean")[v] += isum_sq(d[k])
            if self.log is not None:
                self.log += [(self.n, nk, row, i, v, bool(clean[i])) for i in np.flatnonzero(filed)
                             if v == 0 or i >= self.n_a]

    def tables(self) -> dict:
        d = {k: v for k, v in self.t.items()}
        d["n_pairs"] = self.n_pairs
        return d

    def words(self):
        return pack(self.U, self.bad, self.n_a)


def add_tables(a: dict, b: dict) -> dict:
    def add(x, y):
        return [add(u, v) for u, v in zip(x, y)] if isinstance(x, list) else x + y
    return {k: add(a[k], b[k]) for k in a}


def sample_tables(s) -> dict:
    """A capi.RotSample as nested lists of Python ints, RefRot.tables()' shape."""
    d = {k: [[[int(v) for v in cell] for cell in row] for row in getattr(s, k)] for k in COUNTS + SUMS}
    d["n_pairs"] = [int(v) for v in s.n_pairs]
    return d


def first_difference(got: dict, want: dict):
    for k in want:
        if got[k] != want[k]:
            for r, (g, w) in enumerate(zip(got[k], want[k])):
                if g != w:
                    return k, r, g, w
    return None


def same_sample(s, ref: RefRot) -> bool:
    got, want = sample_tables(s), ref.tables()
    assert got == want, first_difference(got, want)
    assert (s.every, s.levels, s.slots, s.rows) == (ref.every, ref.L, ref.P, ref.rows)
    assert (s.origin_step, s.last_step, s.n_updates) == (ref.origin_step, ref.last_step, ref.n)
    return True


def same_arrays(vec, last_event, chi, ref: RefRot) -> bool:
    want = ref.words()
    assert np.array_equal(vec, want), np.flatnonzero(vec != want)[:8]
    assert np.array_equal(last_event, ref.last_event), np.flatnonzero(last_event != ref.last_event)[:8]
    assert np.array_equal(chi, ref.chi), np.flatnonzero(chi != ref.chi)[:8]
    return True


def same_info(info, ref: RefRot) -> bool:
    got = (info.n_updates, info.n_tasks, info.n_events, info.n_flips, info.n_bad)
    assert got == (ref.n, ref.last_tasks, ref.last_events, ref.last_flips, ref.last_bad), got
    return True


def pose(p, hs, nz, nc):
    """(hist[4][nz][nc] as nested lists, chi_pos[4], chi_neg[4], n_bad) from the definitions, in Python ints."""
    U, chi, bad, Z = vectors(hs)
    n_a = hs.n_a
    k = (links(hs)[n_a:] != 0).sum(axis=1)
    BZ, Lq = int(_q(p.box_z)), int(_q(p.rb_radius))
    hist = [[[0] * nc for _ in range(nz)] for _ in range(4)]
    pos, neg, n_bad = [0] * 4, [0] * 4, 0
    for b in range(hs.n_b):
        if bad[n_a + b]:
            n_bad += 1
            continue
        z, nzq = int(Z[b]), int(U[n_a + b, 0, 2])
        zb = 0 if z <= 0 else nz - 1 if z >= BZ else min(nz - 1, z * nz // BZ)
        tb = min(nc - 1, max(0, (nzq + Lq) * nc // (2 * Lq + 1)))
        hist[int(k[b])][zb][tb] += 1
        pos[int(k[b])] += int(chi[n_a + b] > 0)
        neg[int(k[b])] += int(chi[n_a + b] < 0)
    return hist, pos, neg, n_bad


def same_pose(got, p, hs, nz, nc) -> bool:
    hist, out = got
    want = pose(p, hs, nz, nc)
    assert hist.tolist() == want[0]
    assert ([int(x) for x in out.chi_pos], [int(x) for x in out.chi_neg], int(out.n_bad)) == want[1:]
    return True
