"""Python reference of the pair dynamics (include/kmc.h), shared
by test_pairdyn_host.py and test_gpu_pairdyn.py and independent of the C code:
the coordinates in numpy int64, every sum in Python integers (or in split words
that cannot wrap), round_ through engine.math (the host kmc_math.h).  It knows
no cells: both parts are a brute-force pass over all N^2 pairs, in blocks of
rows to bound the memory.  Every comparison against it is exact equality."""
import numpy as np

from _kmc import capi, engine
from _lagcorr import icoords, min_image

COUNTS = ("n_pairs", "n_valid")
SUMS = ("dot", "sq")
SPLIT = 24  # a term t = (t >> 24) * 2^24 + (t & (2^24 - 1)): both words of 2^24 terms below 2^50 stay below 2^63
ROWS = 256  # rows of the pair matrix taken at a time


def _round(a):
    """The library's round_ (half away from zero; np.round rounds half to even)."""
    return engine.math(6, np.ascontiguousarray(a, dtype=np.float64).ravel()).reshape(np.shape(a))


def edges(r_max, nbins):
    """E[0..nbins] as Python ints: round_(m * (r_max / nbins) * 1024)."""
    dr = np.float64(r_max) / np.float64(nbins)
    return [int(x) for x in _round(np.arange(nbins + 1, dtype=np.float64) * dr * 1024.0)]


def bins_of(d2, E2):
    """k = #{m in 1..nbins : E[m]^2 <= d2} of int64 d2; E2 the int64 squared edges [nbins + 1]."""
    return np.searchsorted(E2[1:], d2, side="right")


class RefPd:
    """The recorder of include/kmc.h on host states."""

    def __init__(self, p, hs, every, nbins, r_max, max_jump=0.0, max_disp=0.0):
        self.p, self.every, self.nbins, self.r_max = p, every, nbins, r_max
        half = 0.5 * min(p.box_x, p.box_y)
        self.max_jump = max_jump if max_jump > 0.0 else 0.5 * half
        self.max_disp = max_disp if max_disp > 0.0 else 16384.0
        self.J = int(_round(np.array([self.max_jump * 1024.0]))[0])
        self.F = int(_round(np.array([self.max_disp * 1024.0]))[0])
        self.B = [int(_round(np.array([b * 1024.0]))[0]) for b in (p.box_x, p.box_y)]
        self.E = edges(r_max, nbins)
        assert all(b > a for a, b in zip(self.E, self.E[1:]))
        self.n_a = hs.n_a
        self.X0 = icoords(hs)
        self.prev = self.X0.copy()
        self.U = self.X0.copy()
        self.jumped = np.zeros(len(self.U), dtype=bool)
        self.crossed = np.zeros(len(self.U), dtype=bool)  # a protein whose wrapped coordinate jumped across the seam
        self.n = 0
        self._cache = (-1, None)  # the last tables() of all proteins, by update
        self.origin_step = self.last_step = hs.step

    def update(self, hs):
        assert hs.step == self.last_step + self.every
        X = icoords(hs)
        raw = X - self.prev
        d = np.stack([min_image(raw[:, c], self.B[c]) for c in range(2)], axis=1)
        self.crossed |= (d != raw).any(axis=1)
        self.U += d
        self.prev = X
        self.jumped |= (np.abs(d) >= self.J).any(axis=1)
        self.n += 1
        self.last_step = hs.step

    def flags(self):
        return self.jumped.astype(np.uint8) * capi.PD_JUMPED

    def valid(self):
        u = self.U - self.X0
        return ~self.jumped & (np.abs(u) < self.F).all(axis=1)

    def tables(self, keep=None):
        """gd [4][nbins], gs [2][nbins] and n_pairs, n_valid, dot, sq [3][nbins] as lists of Python ints; seam_a /
        seam_b: the counted pairs of part A / B whose minimum image is not the plain difference.  keep: a boolean
        mask of the proteins taken (all when None)."""
        if keep is None and self._cache[0] == self.n:
            return self._cache[1]
        nb, na = self.nbins, self.n_a
        idx = np.arange(len(self.U)) if keep is None else np.flatnonzero(keep)
        N = len(idx)
        E2 = np.array([e * e for e in self.E], dtype=np.int64)
        BX, BY = self.B
        fU = np.stack([np.mod(self.U[idx, 0], BX), np.mod(self.U[idx, 1], BY)], axis=1)
        f0 = np.stack([np.mod(self.X0[idx, 0], BX), np.mod(self.X0[idx, 1], BY)], axis=1)
        ok = self.valid()[idx]
        u = np.where(ok[:, None], (self.U - self.X0)[idx], 0)
        sp = (idx >= na).astype(np.int64)
        a_cnt = np.zeros(6 * nb, dtype=np.int64)
        b_cnt = {k: np.zeros(3 * nb, dtype=np.int64) for k in COUNTS}
        b_sum = {k: [np.zeros(3 * nb, dtype=np.int64), np.zeros(3 * nb, dtype=np.int64)] for k in SUMS}
        seam_a = seam_b = 0
        col = np.arange(N)
        for r0 in range(0, N, ROWS):
            r = np.arange(r0, min(r0 + ROWS, N))
            # part A: origin i (rows) against now j (columns), ordered
            rx, ry = fU[None, :, 0] - f0[r, None, 0], fU[None, :, 1] - f0[r, None, 1]
            Dx, Dy = min_image(rx, BX), min_image(ry, BY)
            k = bins_of(Dx * Dx + Dy * Dy, E2)
            m = k < nb
            table = np.where(r[:, None] == col[None, :], 4 + sp[r, None], 2 * sp[r, None] + sp[None, :])
            a_cnt += np.bincount((table * nb + k)[m], minlength=6 * nb)
            seam_a += int(np.count_nonzero(m & ((Dx != rx) | (Dy != ry))))
            # part B: unordered pairs i < j of the origin positions
            rx, ry = f0[None, :, 0] - f0[r, None, 0], f0[None, :, 1] - f0[r, None, 1]
            Dx, Dy = min_image(rx, BX), min_image(ry, BY)
            k = bins_of(Dx * Dx + Dy * Dy, E2)
            m = (k < nb) & (col[None, :] > r[:, None])
            cell = (sp[r, None] + sp[None, :]) * nb + k
            b_cnt["n_pairs"] += np.bincount(cell[m], minlength=3 * nb)
            seam_b += int(np.count_nonzero(m & ((Dx != rx) | (Dy != ry))))
            m &= ok[r, None] & ok[None, :]
            b_cnt["n_valid"] += np.bincount(cell[m], minlength=3 * nb)
            at = cell[m]
            dot = (u[r, None, 0] * u[None, :, 0] + u[r, None, 1] * u[None, :, 1])[m]
            uu = (u * u).sum(axis=1)
            sq = (uu[r, None] + uu[None, :])[m]
            for name, t in (("dot", dot), ("sq", sq)):
                assert np.abs(t).max(initial=0) < 1 << 50
                np.add.at(b_sum[name][0], at, t >> SPLIT)
                np.add.at(b_sum[name][1], at, t & ((1 << SPLIT) - 1))
        out = {"gd": [[int(x) for x in a_cnt[t * nb:(t + 1) * nb]] for t in range(4)],
               "gs": [[int(x) for x in a_cnt[(4 + t) * nb:(5 + t) * nb]] for t in range(2)],
               "seam_a": seam_a, "seam_b": seam_b}
        for name in COUNTS:
            out[name] = [[int(x) for x in b_cnt[name][t * nb:(t + 1) * nb]] for t in range(3)]
        for name in SUMS:
            hi, lo = b_sum[name]
            out[name] = [[(int(hi[t * nb + k]) << SPLIT) + int(lo[t * nb + k]) for k in range(nb)] for t in range(3)]
        if keep is None:
            self._cache = (self.n, out)
        return out


def sample_tables(s):
    """A capi.PdSample's tables as the lists RefPd.tables() returns."""
    out = {"gd": [[int(x) for x in row] for row in s.gd], "gs": [[int(x) for x in row] for row in s.gs]}
    for name in COUNTS + SUMS:
        out[name] = [[int(x) for x in row] for row in getattr(s, name)]
    return out


def same_sample(s, ref, keep=None):
    want = ref.tables(keep)
    got = sample_tables(s)
    return all(got[k] == want[k] for k in got) and (s.J, s.F, s.BX, s.BY) == (ref.J, ref.F, ref.B[0], ref.B[1]) and (
        s.origin_step, s.last_step, s.n_updates) == (ref.origin_step, ref.last_step, ref.n)


def same_arrays(U, X0, flags, ref):
    return np.array_equal(U, ref.U) and np.array_equal(X0, ref.X0) and np.array_equal(flags, ref.flags())
