"""Python reference of the multi-origin lag correlator (include/kmc.h, DESIGN.md
§18), shared by test_lagcorr_host.py and test_gpu_lagcorr.py and independent of
the C code: the coordinates in numpy int64, every sum in Python integers (or in
split words that cannot wrap), round_ and cos through engine.math (the host
kmc_math.h) as _structure.py does, and the schedule written from the
definitions of the header's comment — each stored origin carries the update it
was stored at, and every correlation asserts that the slot the definition names
holds the origin of update n - j 2^l.  Every comparison against it is exact
equality."""
import numpy as np

from _kmc import capi, engine

TWO_PI = 6.283185307179586
SCALE = 1073741824.0  # 2^30
CLASSES = 5
COUNTS = ("n_all", "n_clean", "n_far")
SUMS = ("m2_all", "m2_clean", "m4_clean")


def _round(a):
    """The library's round_ (half away from zero; np.round rounds half to even)."""
    return engine.math(6, np.ascontiguousarray(a, dtype=np.float64).ravel()).reshape(np.shape(a))


def icoords(hs) -> np.ndarray:
    """X[N, 2] int64 of bead [1][1], receptors then ligands."""
    xy = np.concatenate([np.stack([hs.ra[0], hs.ra[1]], axis=1), np.stack([hs.rb[0], hs.rb[1]], axis=1)])
    return _round(xy * 1024.0).astype(np.int64)


def links(hs) -> np.ndarray:
    """l[N, 3] as the tracker names them: receptor nei2, nei4, nei3; ligand nei2..4 (reference index + 1)."""
    a = np.stack([hs.a_int[2], hs.a_int[3], hs.a_int[4]], axis=1)
    b = np.stack([hs.b_int[5], hs.b_int[6], hs.b_int[7]], axis=1)
    return np.concatenate([a, b]).astype(np.int64)


def classes(hs) -> np.ndarray:
    l = links(hs)
    n_a = hs.n_a
    c = np.empty(len(l), dtype=np.int64)
    c[:n_a] = np.where(l[:n_a, 0] != 0, 2, np.where(l[:n_a, 2] != 0, 1, 0))
    c[n_a:] = np.where((l[n_a:] != 0).any(axis=1), 4, 3)
    return c


def min_image(d: np.ndarray, B: int) -> np.ndarray:
    m = np.mod(d, np.int64(B))  # numpy's integer mod is the floor modulus
    return np.where(2 * m >= B, m - B, m)


def isum(a: np.ndarray) -> int:
    """The sum of non-negative int64 values below 2^62 as a Python int, in two words that cannot wrap."""
    a = np.asarray(a, dtype=np.int64)
    return (int(np.sum(a >> 31)) << 31) + int(np.sum(a & 0x7FFFFFFF))


def n_rows(L: int, P: int) -> int:
    return P + (L - 1) * (P // 2)


def row_of(l: int, j: int, P: int) -> int:
    return j - 1 if l == 0 else P + (l - 1) * (P // 2) + (j - P // 2 - 1)


def pairs_closed_form(L: int, P: int, n_updates: int) -> list:
    """n_pairs per row after n_updates updates: the count of n <= n_updates with n mod 2^l = 0 and n >= j 2^l."""
    out = [0] * n_rows(L, P)
    for l in range(L):
        for j in (range(1, P + 1) if l == 0 else range(P // 2 + 1, P + 1)):
            out[row_of(l, j, P)] = sum(1 for n in range(1, n_updates + 1) if n % 2 ** l == 0 and n >= j * 2 ** l)
    return out


class RefLag:
    """The recorder of include/kmc.h on host states.  log (when a list): (n, n_k, row, i, far, clean) of every pair."""

    def __init__(self, p, hs, every, levels, slots, max_jump=0.0, max_disp=0.0, h=(), log=None):
        self.p, self.every, self.L, self.P, self.h = p, every, levels, slots, [int(x) for x in h]
        half = 0.5 * min(p.box_x, p.box_y)
        self.max_jump = max_jump if max_jump > 0.0 else 0.5 * half
        self.max_disp = max_disp if max_disp > 0.0 else 16384.0
        self.J = int(_round(np.array([self.max_jump * 1024.0]))[0])
        self.F = int(_round(np.array([self.max_disp * 1024.0]))[0])
        self.B = [int(_round(np.array([b * 1024.0]))[0]) for b in (p.box_x, p.box_y)]
        self.rows = n_rows(levels, slots)
        self.n_a = hs.n_a
        self.prev = icoords(hs)
        self.U = self.prev.copy()
        self.links = links(hs)
        self.last_event = np.zeros(len(self.U), dtype=np.int64)
        self.n = 0
        self.origin_step = self.last_step = hs.step
        # ring[l][slot] = (the update it was stored at, U then); begin stores update 0 in slot 0 of every level
        self.ring = [[None] * slots for _ in range(levels)]
        for l in range(levels):
            self.ring[l][0] = (0, self.U.copy())
        self.n_pairs = [0] * self.rows
        self.t = {k: [[0] * CLASSES for _ in range(self.rows)] for k in COUNTS + SUMS}
        self.fs = [[[0] * len(self.h) for _ in range(CLASSES)] for _ in range(self.rows)]
        self.crossed = np.zeros(len(self.U), dtype=bool)  # a protein whose wrapped coordinate jumped across the seam
        self.log = log
        self.last_tasks = self.last_events = 0

    def _cos_fixed(self, h, D, B):
        r = np.mod(h * D, np.int64(B))
        r = np.where(2 * r >= B, r - B, r)
        a = TWO_PI * (r.astype(np.float64) / np.float64(B))
        return _round(engine.math(1, a) * SCALE).astype(np.int64)

    def update(self, hs):
        assert hs.step == self.last_step + self.every
        self.n += 1
        n, L, P = self.n, self.L, self.P
        X = icoords(hs)
        raw = X - self.prev
        d = np.stack([min_image(raw[:, 0], self.B[0]), min_image(raw[:, 1], self.B[1])], axis=1)
        self.crossed |= (raw != d).any(axis=1)
        self.U = self.U + d
        self.prev = X
        l_now = links(hs)
        ev = (np.abs(d) >= self.J).any(axis=1) | (l_now != self.links).any(axis=1)
        self.links = l_now
        self.last_event[ev] = n
        self.last_events = int(ev.sum())
        cls = classes(hs)
        self.last_tasks = 0
        for l in range(L):
            if n % 2 ** l != 0:
                continue
            t = n >> l
            for j in (range(1, P + 1) if l == 0 else range(P // 2 + 1, P + 1)):
                if j > t:
                    continue
                nk, O = self.ring[l][(t - j) % P]
                assert nk == n - j * 2 ** l, (n, l, j, nk)
                self._file(row_of(l, j, P), nk, O, cls)
                self.last_tasks += 1
        for l in range(L):
            if n % 2 ** l == 0:
                self.ring[l][(n >> l) % P] = (n, self.U.copy())
        self.last_step = hs.step

    def _file(self, row, nk, O, cls):
        D = self.U - O
        far = (np.abs(D) >= self.F).any(axis=1)
        clean = ~far & (self.last_event <= nk)
        q = D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]  # below 2^49 where not far
        self.n_pairs[row] += 1
        if self.log is not None:
            self.log += [(self.n, nk, row, i, bool(far[i]), bool(clean[i])) for i in range(len(D))]
        for c in range(CLASSES):
            m = cls == c
            if not m.any():
                continue
            a, k = m & ~far, m & clean
            self.t["n_far"][row][c] += int((m & far).sum())
            self.t["n_all"][row][c] += int(a.sum())
            self.t["n_clean"][row][c] += int(k.sum())
            self.t["m2_all"][row][c] += isum(q[a])
            self.t["m2_clean"][row][c] += isum(q[k])
            self.t["m4_clean"][row][c] += sum(int(v) * int(v) for v in q[k])
            for x, h in enumerate(self.h if k.any() else []):
                term = self._cos_fixed(h, D[k, 0], self.B[0]) + self._cos_fixed(h, D[k, 1], self.B[1])
                self.fs[row][c][x] += sum(int(v) for v in term)

    def tables(self) -> dict:
        d = {k: v for k, v in self.t.items()}
        d["fs"] = self.fs
        d["n_pairs"] = self.n_pairs
        return d


def add_tables(a: dict, b: dict) -> dict:
    """The cell-wise sum of two RefLag.tables() in Python ints."""
    def add(x, y):
        return [add(u, v) for u, v in zip(x, y)] if isinstance(x, list) else x + y
    return {k: add(a[k], b[k]) for k in a}


def sample_tables(s) -> dict:
    """A capi.LagSample as nested lists of Python ints, RefLag.tables()' shape."""
    d = {k: [[int(v) for v in row] for row in getattr(s, k)] for k in COUNTS + SUMS}
    d["fs"] = [[[int(v) for v in cell] for cell in row] for row in s.fs]
    d["n_pairs"] = [int(v) for v in s.n_pairs]
    return d


def first_difference(got: dict, want: dict):
    for k in want:
        if got[k] != want[k]:
            for r, (g, w) in enumerate(zip(got[k], want[k])):
                if g != w:
                    return k, r, g, w
    return None


def same_sample(s, ref: RefLag) -> bool:
    """The sample's table, n_pairs, integer bounds and steps against the reference's."""
    got, want = sample_tables(s), ref.tables()
    assert got == want, first_difference(got, want)
    assert (s.J, s.F, s.BX, s.BY, s.rows) == (ref.J, ref.F, ref.B[0], ref.B[1], ref.rows)
    assert (s.origin_step, s.last_step, s.n_updates) == (ref.origin_step, ref.last_step, ref.n)
    assert (s.max_jump, s.max_disp) == (ref.max_jump, ref.max_disp)
    return True


def same_arrays(U, last_event, ref: RefLag) -> bool:
    assert np.array_equal(U, ref.U), np.flatnonzero((U != ref.U).any(axis=1))[:8]
    assert np.array_equal(last_event, ref.last_event), np.flatnonzero(last_event != ref.last_event)[:8]
    return True
