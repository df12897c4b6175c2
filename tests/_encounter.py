"""Plain-Python reference of the encounter layer (include/kmc.h):
a brute-force reach census and the R-L encounter recorder, written from the
definitions with numpy float64 in the engine's expression order, math.acos and
180/3.14159, no minimum image.  It shares no code with the library.

Python's acos may differ from the library's in the last ulp, so everything here
also keeps `margin`: the smallest relative distance of any tested d2, angle or
angle bin value to the cutoff or bin edge it was compared with.  A test
requires margin > 1e-9 (and picks another seed otherwise)."""
import math

import numpy as np

SLOTS, BINS, HISTS = 4, 256, 9
CENSORED, GEMINATE, REACTIVE, WAS_REACTIVE = 1, 2, 4, 8
BOUND, SEPARATED, LOST_RECEPTOR, LOST_SITE, CENSORED_ENDED, GEM_REBOUND, GEM_ESCAPED, GEM_LOST, ALIVE = range(9)
RL, MONO, CX = 0, 1, 2
ARRAYS = ("lig", "site", "key", "since", "nreact", "flags")
COUNTERS = ("origin_step", "last_step", "n_updates", "on_from_encounter", "on_direct", "n_opened", "n_ended",
            "exp_reach", "exp_reactive", "exp_free_receptor", "n_overflow", "occ_reach", "occ_reactive",
            "occ_free_receptor", "n_censored_alive", "every", "slots")


def dur_bin(v: int) -> int:
    """The kinetics bin rule (§15): exact below 16, then eight bins per octave, clamped."""
    if v < 16:
        return max(int(v), 0)
    e = int(v).bit_length() - 1
    return min(16 + 8 * (e - 4) + ((int(v) >> (e - 3)) & 7), BINS - 1)


def sqrt_threshold(c: float) -> float:
    """The smallest double T with sqrt(T) >= c."""
    t = c * c
    while math.sqrt(t) >= c:
        t = math.nextafter(t, 0.0)
    while math.sqrt(t) < c:
        t = math.nextafter(t, math.inf)
    return t


def theta(p0, p2) -> float:
    """gettheta with p1 the origin (main.cpp:2329-2366)."""
    lx0, ly0, lz0 = 0.0 - p0[0], 0.0 - p0[1], 0.0 - p0[2]
    lr0 = math.sqrt(lx0 * lx0 + ly0 * ly0 + lz0 * lz0)
    lx1, ly1, lz1 = p2[0] - 0.0, p2[1] - 0.0, p2[2] - 0.0
    lr1 = math.sqrt(lx1 * lx1 + ly1 * ly1 + lz1 * lz1)
    conv = 180 / 3.14159
    doth1 = -(lx1 * lx0 + ly0 * ly1 + lz0 * lz1)
    doth2 = doth1 / (lr1 * lr0)
    if doth2 > 1:
        doth2 = 1
    if doth2 < -1:
        doth2 = -1
    return math.acos(doth2) * conv


def bead_a(hs, j, k):
    """[3, n_a] float64: R[.][j][k] of the receptors."""
    o = ((j - 1) * 4 + (k - 1)) * 3
    return hs.ra[o:o + 3]


def bead_b(hs, j, k):
    o = ((j - 1) * 2 + (k - 1)) * 3
    return hs.rb[o:o + 3]


def _sub(a, b):
    return (float(a[0]) - float(b[0]), float(a[1]) - float(b[1]), float(a[2]) - float(b[2]))


class Margin:
    def __init__(self):
        self.value = math.inf

    def against(self, x, edge):
        """x (scalar or array) was compared with edge."""
        x = np.asarray(x, dtype=np.float64)
        if x.size:
            self.value = min(self.value, float(np.min(np.abs(x - edge)) / max(abs(edge), 1e-300)))

    def bins(self, v):
        """v = x * scale was truncated to a bin: its distance to the nearest integer edge >= 1."""
        m = max(round(v), 1)
        self.value = min(self.value, abs(v - m) / m)


def rl_in_reach(p, hs, margin):
    """The in-reach R-L triples as a list of (i, b, k, d2) (0-based i and b, k in 2..4), in any order."""
    na, nb = p.n_a, p.n_b
    T = sqrt_threshold(p.bond_dist_cutoff)
    free_r = hs.a_int[0] == 0
    site = bead_a(hs, 3, 2)
    hits = []
    for k in (2, 3, 4):
        free_s = hs.b_int[k - 1] == 0
        pt = bead_b(hs, k, 2)
        dx = pt[0][None, :] - site[0][:, None]
        dy = pt[1][None, :] - site[1][:, None]
        dz = pt[2][None, :] - site[2][:, None]
        d2 = dx * dx + dy * dy + dz * dz
        ok = free_r[:, None] & free_s[None, :]
        margin.against(d2[ok], T)
        for i, b in np.argwhere(ok & (d2 < T)):
            hits.append((int(i), int(b), k, float(d2[i, b])))
    assert na == hs.a_int.shape[1] and nb == hs.b_int.shape[1]
    return hits


def rl_angles(hs, i, b, k):
    """(|theta_pd|, |theta_ot - 180|) of the triple."""
    r31, r32, r34 = bead_a(hs, 3, 1)[:, i], bead_a(hs, 3, 2)[:, i], bead_a(hs, 3, 4)[:, i]
    lk1, lk2 = bead_b(hs, k, 1)[:, b], bead_b(hs, k, 2)[:, b]
    l11, l12 = bead_b(hs, 1, 1)[:, b], bead_b(hs, 1, 2)[:, b]
    ot = theta(_sub(r31, r32), _sub(lk1, lk2))
    pd = theta(_sub(r31, r34), _sub(l11, l12))
    return abs(pd), abs(ot - 180)


def rl_reactive(p, pd, ot, margin):
    margin.against(pd, p.bond_thetapd_cutoff)
    margin.against(ot, p.bond_thetaot_cutoff)
    return pd < p.bond_thetapd_cutoff and ot < p.bond_thetaot_cutoff


def _dist_bin(E2, d2, margin):
    for e in E2[1:]:
        margin.against(d2, e)
    return sum(1 for e in E2[1:] if e <= d2)


def _ang_bin(x, na, margin):
    v = x * (na / 180.0)
    margin.bins(v)
    return min(int(v), na - 1)


def census(p, hs, nd, na):
    """(out dict, hist_d[3, 2, nd], hist_a_rl[na, na], hist_a_cis[2, na], margin) of the state."""
    margin = Margin()
    hist_d = np.zeros((3, 2, nd), dtype=np.int64)
    hist_a_rl = np.zeros((na, na), dtype=np.int64)
    hist_a_cis = np.zeros((2, na), dtype=np.int64)
    n_reach, n_reactive = [0, 0, 0], [0, 0, 0]
    E2 = [[0.0] + [(c * m / nd) * (c * m / nd) for m in range(1, nd)]
          for c in (p.bond_dist_cutoff, p.cis_dist_cutoff, p.cis_dist_cutoff)]
    partners, sites = {}, set()
    for i, b, k, d2 in rl_in_reach(p, hs, margin):
        pd, ot = rl_angles(hs, i, b, k)
        r = rl_reactive(p, pd, ot, margin)
        n_reach[RL] += 1
        n_reactive[RL] += r
        hist_d[RL, int(r), _dist_bin(E2[RL], d2, margin)] += 1
        hist_a_rl[_ang_bin(pd, na, margin), _ang_bin(ot, na, margin)] += 1
        partners[i] = partners.get(i, 0) + 1
        sites.add((b, k))
    T = sqrt_threshold(p.cis_dist_cutoff)
    s33, s31 = bead_a(hs, 3, 3), bead_a(hs, 3, 1)
    free = np.flatnonzero(hs.a_int[1] == 0)
    for n, i in enumerate(free):
        js = free[n + 1:]
        dx, dy, dz = s33[0][js] - s33[0][i], s33[1][js] - s33[1][i], s33[2][js] - s33[2][i]
        d2 = dx * dx + dy * dy + dz * dz
        margin.against(d2, T)
        for j, q in zip(js[d2 < T], d2[d2 < T]):
            ot = abs(theta(_sub(s31[:, i], s33[:, i]), _sub(s31[:, j], s33[:, j])) - 180)
            margin.against(ot, p.cis_thetaot_cutoff)
            r = ot < p.cis_thetaot_cutoff
            ch = CX if hs.a_int[0, i] != 0 or hs.a_int[0, j] != 0 else MONO
            n_reach[ch] += 1
            n_reactive[ch] += r
            hist_d[ch, int(r), _dist_bin(E2[ch], float(q), margin)] += 1
            hist_a_cis[ch - MONO, _ang_bin(ot, na, margin)] += 1
    out = dict(n_reach=n_reach, n_reactive=n_reactive,
               rl_free_receptors=int(np.count_nonzero(hs.a_int[0] == 0)),
               rl_free_sites=int(np.count_nonzero(hs.b_int[1:4] == 0)),
               rl_receptors_in_reach=len(partners), rl_sites_in_reach=len(sites),
               rl_max_partners=max(partners.values(), default=0))
    return out, hist_d, hist_a_rl, hist_a_cis, margin.value


class Recorder:
    """The R-L encounter recorder of include/kmc.h on host states."""

    def __init__(self, p, hs, every=1, slots=SLOTS):
        self.p, self.every, self.nslots = p, every, slots
        self.margin = Margin()
        self.hist = np.zeros((HISTS - 1 + 2, BINS), dtype=np.int64)  # rows 0-7, then react_hist's two
        self.origin = self.last = hs.step
        self.n_updates = 0
        self.ev = dict(on_from_encounter=0, on_direct=0, n_opened=0, n_ended=0, n_overflow=0)
        self.exp = [0, 0, 0]
        links, sets, cut = self._look(hs)
        self.link = links
        self.slots = [[dict(key=k, since=hs.step, nreact=int(r), flags=CENSORED | (REACTIVE | WAS_REACTIVE if r else 0))
                       for k, r in s] for s in sets]
        self.ev["n_overflow"] += cut
        self._occupancy()

    def _look(self, hs):
        """Per receptor: its link (lig, site), its in-reach triples cut to the smallest keys [(key, reactive)], and
        the number of entries cut."""
        p = self.p
        links = [(int(hs.a_int[2, i]), int(hs.a_int[3, i])) if hs.a_int[2, i] else (0, 0) for i in range(p.n_a)]
        per = [[] for _ in range(p.n_a)]
        for i, b, k, _ in rl_in_reach(p, hs, self.margin):
            pd, ot = rl_angles(hs, i, b, k)
            per[i].append(((b + 1) << 2 | (k - 2), rl_reactive(p, pd, ot, self.margin)))
        cut = sum(max(len(s) - self.nslots, 0) for s in per)
        return links, [sorted(s)[:self.nslots] for s in per], cut

    def _occupancy(self):
        self.occ = [sum(len(s) for s in self.slots), sum(1 for s in self.slots for e in s if e["flags"] & REACTIVE),
                    sum(1 for l in self.link if l[0] == 0)]

    def update(self, hs):
        p, t = self.p, hs.step
        dt = t - self.last
        if dt == 0:
            self.n_updates += 1
            return
        assert dt == self.every
        links, sets, cut = self._look(hs)
        for k in range(3):
            self.exp[k] += dt * self.occ[k]
        for i in range(p.n_a):
            lig, site = links[i]
            cur = dict(sets[i])
            old = self.slots[i]
            born = lig != 0 and (lig, site) != self.link[i]
            bkey = (lig - p.n_a) << 2 | (site - 2) if born else None
            gkey = (self.link[i][0] - p.n_a) << 2 | (self.link[i][1] - 2) if self.link[i][0] else None
            matched = False
            for s in old:
                if born and s["key"] == bkey:
                    matched = True
                    row, bound = (GEM_REBOUND if s["flags"] & GEMINATE else BOUND), True
                elif s["key"] in cur:
                    continue
                else:
                    b, k = s["key"] >> 2, 2 + (s["key"] & 3)
                    outcome = LOST_RECEPTOR if lig != 0 else LOST_SITE if hs.b_int[k - 1, b - 1] != 0 else SEPARATED
                    if s["flags"] & CENSORED:
                        row = CENSORED_ENDED
                    elif s["flags"] & GEMINATE:
                        row = GEM_ESCAPED if outcome == SEPARATED else GEM_LOST
                    else:
                        row = outcome
                    bound = False
                self.hist[row, dur_bin(t - s["since"])] += 1
                self.hist[HISTS - 1 + (0 if bound else 1), dur_bin(s["nreact"])] += 1
                self.ev["n_ended"] += 1
            if born:
                self.ev["on_from_encounter" if matched else "on_direct"] += 1
            was = {s["key"]: s for s in old}
            new = []
            for key, r in sets[i]:
                now = REACTIVE | WAS_REACTIVE if r else 0
                if key in was:
                    s = was[key]
                    new.append(dict(key=key, since=s["since"], nreact=s["nreact"] + int(r),
                                    flags=(s["flags"] & (CENSORED | GEMINATE | WAS_REACTIVE)) | now))
                else:
                    new.append(dict(key=key, since=t, nreact=int(r), flags=(GEMINATE if key == gkey else 0) | now))
                    self.ev["n_opened"] += 1
            self.slots[i] = new
        self.link = links
        self.ev["n_overflow"] += cut
        self._occupancy()
        self.last = t
        self.n_updates += 1

    def arrays(self) -> dict:
        na = self.p.n_a
        a = dict(lig=np.array([l[0] for l in self.link], dtype=np.int32).reshape(na),
                 site=np.array([l[1] for l in self.link], dtype=np.int32).reshape(na),
                 key=np.zeros((na, SLOTS), dtype=np.int32), since=np.zeros((na, SLOTS), dtype=np.int64),
                 nreact=np.zeros((na, SLOTS), dtype=np.int32), flags=np.zeros((na, SLOTS), dtype=np.uint8))
        for i, s in enumerate(self.slots):
            for q, e in enumerate(s):
                for name in ("key", "since", "nreact", "flags"):
                    a[name][i, q] = e[name]
        return a

    def out(self, alive=0) -> dict:
        d = dict(origin_step=self.origin, last_step=self.last, n_updates=self.n_updates, **self.ev,
                 exp_reach=self.exp[0], exp_reactive=self.exp[1], exp_free_receptor=self.exp[2],
                 occ_reach=self.occ[0], occ_reactive=self.occ[1], occ_free_receptor=self.occ[2],
                 n_censored_alive=alive, every=self.every, slots=self.nslots)
        return {k: d[k] for k in COUNTERS}

    def sample(self):
        """(out dict, hist[9, 256], react_hist[2, 256])."""
        hist = np.zeros((HISTS, BINS), dtype=np.int64)
        hist[:HISTS - 1] = self.hist[:HISTS - 1]
        alive = 0
        for s in self.slots:
            for e in s:
                if e["flags"] & CENSORED:
                    alive += 1
                else:
                    hist[ALIVE, dur_bin(self.last - e["since"])] += 1
        return self.out(alive), hist, self.hist[HISTS - 1:].copy()


# ---------------------------------------------------------------- hand-made states
def place(hs, i, b, k, off):
    """Bead [k][2] of ligand b (0-based) goes to bead [3][2] of receptor i (0-based) + off."""
    o = ((k - 1) * 2 + 1) * 3
    for c in range(3):
        hs.rb[o + c, b] = hs.ra[((3 - 1) * 4 + 1) * 3 + c, i] + off[c]


def bind(hs, i, b, k):
    n_a = hs.a_int.shape[1]
    hs.a_int[0, i], hs.a_int[2, i], hs.a_int[3, i] = 1, n_a + b + 1, k
    hs.b_int[k - 1, b], hs.b_int[4 + k - 1, b] = 1, i + 1


def unbind(hs, i, b, k):
    hs.a_int[0, i] = hs.a_int[2, i] = hs.a_int[3, i] = 0
    hs.b_int[k - 1, b] = hs.b_int[4 + k - 1, b] = 0


def same_arrays(got, rec) -> bool:
    want = rec.arrays() if hasattr(rec, "arrays") and callable(rec.arrays) else None
    if want is None:
        want = {k: getattr(rec.arrays, k) for k in ARRAYS}
    return all(np.array_equal(getattr(got, k), want[k]) for k in ARRAYS)


def first_difference(got, rec):
    want = rec.arrays() if callable(getattr(rec, "arrays", None)) else {k: getattr(rec.arrays, k) for k in ARRAYS}
    for k in ARRAYS:
        g = getattr(got, k)
        bad = np.argwhere(g != want[k])
        if bad.size:
            at = tuple(int(x) for x in bad[0])
            return k, at, int(g[at]), int(want[k][at])
    return None
