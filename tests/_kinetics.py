"""A plain-Python recorder of the bond kinetics with the definitions of
include/kmc.h, fed with host states: what the device recorder
(kmc_kinetics.hip) and the host counterpart (kmc_host_kin_*) are compared
against, by equality.  Written from the definitions, one receptor after the
other; it shares no code with the library."""
import numpy as np

BINS, HISTS = 256, 9
RL_CENS, CIS_CENS, COMPLEX = 1, 2, 4
EVENTS = ("rl_on", "rl_off", "rl_swap", "cis_on", "cis_off_mono", "cis_off_cx", "cis_swap")
EXPOSURES = ("exp_rl", "exp_mono", "exp_cx", "exp_free_receptor", "exp_free_site")
OCCUPANCY = ("occ_rl", "occ_mono", "occ_cx", "occ_free_receptor", "occ_free_site")
ARRAYS = ("rl_lig", "rl_site", "rl_since", "cis_with", "cis_since", "last_lig", "free_since", "bits")


def kin_bin(v: int) -> int:
    """The bin of a lifetime or waiting time v >= 0."""
    v = int(v)
    if v < 16:
        return v
    e = v.bit_length() - 1
    return min(16 + 8 * (e - 4) + ((v >> (e - 3)) & 7), BINS - 1)


def _links(hs):
    """(lig, site, cis) of every receptor, as Python ints."""
    return ([int(x) for x in hs.a_int[2]], [int(x) for x in hs.a_int[3]], [int(x) for x in hs.a_int[4]])


class Recorder:
    def __init__(self, p, hs):
        self.n_a, self.n_b = p.n_a, p.n_b
        n, t = p.n_a, int(hs.step)
        lig, site, cis = _links(hs)
        self.rl_lig, self.rl_site, self.cis_with = list(lig), list(site), list(cis)
        self.rl_since, self.cis_since, self.free_since = [t] * n, [t] * n, [t] * n
        self.last_lig = [0] * n
        self.bits = [(RL_CENS if lig[i] else 0) | (CIS_CENS if cis[i] else 0) | self._kind(lig, cis, i)
                     for i in range(n)]
        self.hist = np.zeros((HISTS - 2, BINS), dtype=np.int64)
        self.c = dict.fromkeys(("n_updates",) + EVENTS + EXPOSURES, 0)
        self.c.update(origin_step=t, last_step=t)
        self._count(lig, cis)

    @staticmethod
    def _kind(lig, cis, i):
        j = cis[i]
        return COMPLEX if j and (lig[i] or lig[j - 1]) else 0

    def _count(self, lig, cis):
        rl = sum(1 for x in lig if x)
        mono = cx = 0
        for i in range(self.n_a):
            if cis[i] and i + 1 < cis[i]:
                if self._kind(lig, cis, i):
                    cx += 1
                else:
                    mono += 1
        self.c.update(occ_rl=rl, occ_mono=mono, occ_cx=cx, occ_free_receptor=self.n_a - rl,
                      occ_free_site=3 * self.n_b - rl)

    def update(self, hs) -> dict:
        c, t = self.c, int(hs.step)
        dt = t - c["last_step"]
        for e, o in zip(EXPOSURES, OCCUPANCY):
            c[e] += dt * c[o]
        lig, site, cis = _links(hs)
        for i in range(self.n_a):
            me = i + 1
            differs = (lig[i], site[i]) != (self.rl_lig[i], self.rl_site[i])
            if self.rl_lig[i] and differs:  # R-L ended
                self.hist[1 if self.bits[i] & RL_CENS else 0, kin_bin(t - self.rl_since[i])] += 1
                c["rl_off"] += 1
                self.last_lig[i], self.free_since[i] = self.rl_lig[i], t
                if lig[i]:
                    c["rl_swap"] += 1
            if lig[i] and differs:  # R-L born
                c["rl_on"] += 1
                if self.last_lig[i]:
                    self.hist[5 if lig[i] == self.last_lig[i] else 6, kin_bin(t - self.free_since[i])] += 1
                self.rl_since[i] = t
                self.bits[i] &= ~RL_CENS
            old = self.cis_with[i]
            if old and me < old and cis[i] != old:  # cis ended
                cx = bool(self.bits[i] & COMPLEX)
                row = 4 if self.bits[i] & CIS_CENS else 3 if cx else 2
                self.hist[row, kin_bin(t - self.cis_since[i])] += 1
                c["cis_off_cx" if cx else "cis_off_mono"] += 1
                if cis[i]:
                    c["cis_swap"] += 1
            if cis[i] and cis[i] != old:  # cis born
                self.cis_since[i] = t
                self.bits[i] &= ~CIS_CENS
                if me < cis[i]:
                    c["cis_on"] += 1
            self.rl_lig[i], self.rl_site[i], self.cis_with[i] = lig[i], site[i], cis[i]
            self.bits[i] = (self.bits[i] & ~COMPLEX) | self._kind(lig, cis, i)
        self._count(lig, cis)
        c["last_step"] = t
        c["n_updates"] += 1
        return self.out()

    def out(self) -> dict:
        d = dict(self.c)
        d.update(n_rl_censored_alive=0, n_cis_censored_alive=0)
        return d

    def sample(self):
        """(out, hist[9, 256]) as of the last update."""
        d = self.out()
        hist = np.zeros((HISTS, BINS), dtype=np.int64)
        hist[:HISTS - 2] = self.hist
        t = d["last_step"]
        for i in range(self.n_a):
            if self.rl_lig[i]:
                if self.bits[i] & RL_CENS:
                    d["n_rl_censored_alive"] += 1
                else:
                    hist[7, kin_bin(t - self.rl_since[i])] += 1
            if self.cis_with[i] and i + 1 < self.cis_with[i]:
                if self.bits[i] & CIS_CENS:
                    d["n_cis_censored_alive"] += 1
                else:
                    hist[8, kin_bin(t - self.cis_since[i])] += 1
        return d, hist

    def arrays(self) -> dict:
        return {k: np.array(getattr(self, k), dtype=np.int64) for k in ARRAYS}


def same_arrays(got, want: Recorder) -> bool:
    """A capi.KinArrays against the recorder's lists."""
    w = want.arrays()
    return all(np.array_equal(np.asarray(getattr(got, k), dtype=np.int64), w[k]) for k in ARRAYS)


def first_difference(got, want: Recorder) -> str:
    w = want.arrays()
    for k in ARRAYS:
        g = np.asarray(getattr(got, k), dtype=np.int64)
        bad = np.flatnonzero(g != w[k])
        if bad.size:
            return f"{k}[{bad[0]}]: {g[bad[0]]} != {w[k][bad[0]]}"
    return ""
