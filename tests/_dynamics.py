"""numpy reference of the displacement tracker (include/kmc.h),
shared by test_dynamics_host.py and test_gpu_dynamics.py: the definitions of
kmc_track_begin / update / sample applied to a sequence of host states
(get_state() snapshots).  round_ is the library's (engine.math op 6, half away
from zero), every product and sum is a separate numpy operation (no fused
multiply-add), and the sums follow the halving tree over blocks of 256 — so
every result is compared by exact equality, doubles as bit patterns."""
import numpy as np

from _kmc import capi, engine

CLASSES = 5
SURVIVAL = ("rl0", "rl_now", "rl_kept", "cis0", "cis_now", "cis_kept")


def positions(hs) -> np.ndarray:
    """(x, y) of bead [1][1] by reference index: [N, 2]."""
    return np.stack([np.concatenate([hs.ra[0], hs.rb[0]]), np.concatenate([hs.ra[1], hs.rb[1]])], axis=1)


def links(hs) -> np.ndarray:
    """[N, 3] links as get_state() returns them (reference index, 1-based): a
    receptor's nei2, nei4, nei3; a ligand's nei2, nei3, nei4."""
    a = np.stack([hs.a_int[2], hs.a_int[3], hs.a_int[4]], axis=1)
    b = np.stack([hs.b_int[5], hs.b_int[6], hs.b_int[7]], axis=1)
    return np.concatenate([a, b]).astype(np.int64)


def classes(hs) -> np.ndarray:
    l = links(hs)
    na = hs.n_a
    ca = np.where(l[:na, 0] != 0, 2, np.where(l[:na, 2] != 0, 1, 0))
    cb = np.where((l[na:] != 0).any(axis=1), 4, 3)
    return np.concatenate([ca, cb]).astype(np.int64)


def tree_sum(v) -> np.float64:
    """The reduction of include/kmc.h: pad with 0.0 to a multiple of 256, reduce
    each block of 256 by the halving tree, repeat on the block results."""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return np.float64(0.0)
    while True:
        pad = (-v.size) % 256
        a = np.concatenate([v, np.zeros(pad)]).reshape(-1, 256)
        h = 128
        while h >= 1:
            a = a[:, :h] + a[:, h:2 * h]
            h //= 2
        v = a[:, 0]
        if v.size == 1:
            return v[0]


def min_image(d: np.ndarray, box: float):
    """(d − box · round_(d / box), round_(d / box)) with the library's round_."""
    r = engine.math(6, d / box)
    return d - box * r, r


class Tracker:
    def __init__(self, p, hs, max_jump=0.0):
        self.box = (p.box_x, p.box_y)
        self.na = hs.n_a
        self.max_jump = min(p.box_x, p.box_y) / 4 if max_jump <= 0 else max_jump
        self.prev = positions(hs)
        self.u = np.zeros_like(self.prev)
        self.flags = np.zeros(len(self.prev), dtype=np.uint8)
        self.link0 = links(hs)
        self.cls = classes(hs)
        self.rl_changed = np.zeros(self.na, dtype=bool)   # nei2 / nei4 differed at some update
        self.cis_changed = np.zeros(self.na, dtype=bool)  # nei3 did
        self.origin_step = self.last_step = int(hs.step)
        self.n_updates = 0
        self.max_d = [0.0, 0.0]
        self.n_wraps = 0  # (protein, axis, update) events with round_ != 0: the input crossed the box edge

    def update(self, hs) -> dict:
        pos = positions(hs)
        jumped = np.zeros(len(pos), dtype=bool)
        for c in (0, 1):
            d, r = min_image(pos[:, c] - self.prev[:, c], self.box[c])
            self.u[:, c] = self.u[:, c] + d
            self.n_wraps += int(np.count_nonzero(r))
            jumped |= np.abs(d) >= self.max_jump
            self.max_d[c] = max(self.max_d[c], float(np.abs(d).max())) if len(d) else self.max_d[c]
        self.prev = pos
        diff = links(hs) != self.link0
        self.rl_changed |= diff[:self.na, 0] | diff[:self.na, 1]
        self.cis_changed |= diff[:self.na, 2]
        self.flags[diff.any(axis=1)] |= capi.TRACK_CHANGED
        self.flags[jumped] |= capi.TRACK_JUMPED
        self.last_step = int(hs.step)
        self.n_updates += 1
        return dict(origin_step=self.origin_step, last_step=self.last_step, n_updates=self.n_updates,
                    max_dx=self.max_d[0], max_dy=self.max_d[1],
                    n_jumped=int(np.count_nonzero(self.flags & capi.TRACK_JUMPED)),
                    n_changed=int(np.count_nonzero(self.flags & capi.TRACK_CHANGED)))

    def sample(self, hs, r_max, nbins):
        """(dict like capi.TrackSample.as_dict(), vanhove[CLASSES, nbins]); hs is the current state."""
        q = self.u[:, 0] * self.u[:, 0] + self.u[:, 1] * self.u[:, 1]
        clean = self.flags == 0
        out = dict(origin_step=self.origin_step, last_step=self.last_step,
                   n=np.zeros(CLASSES, dtype=np.int64), n_clean=np.zeros(CLASSES, dtype=np.int64),
                   sum_u2=np.zeros(CLASSES), sum_u2_clean=np.zeros(CLASSES))
        dr = r_max / nbins
        m = np.arange(nbins + 1, dtype=np.float64)
        edges2 = (m * dr) * (m * dr)
        vh = np.zeros((CLASSES, nbins), dtype=np.int64)
        for c in range(CLASSES):
            member = self.cls == c
            out["n"][c] = np.count_nonzero(member)
            out["n_clean"][c] = np.count_nonzero(member & clean)
            out["sum_u2"][c] = tree_sum(np.where(member, q, 0.0))
            out["sum_u2_clean"][c] = tree_sum(np.where(member & clean, q, 0.0))
            k = np.searchsorted(edges2[1:], q[member & clean], side="right")
            vh[c] = np.bincount(k[k < nbins], minlength=nbins)
        na = self.na
        now = links(hs)[:na] == self.link0[:na]
        rl = self.link0[:na, 0] != 0
        cis = (self.link0[:na, 2] != 0) & (np.arange(1, na + 1) < self.link0[:na, 2])
        out.update(rl0=int(rl.sum()), rl_now=int((rl & now[:, 0] & now[:, 1]).sum()),
                   rl_kept=int((rl & ~self.rl_changed).sum()), cis0=int(cis.sum()),
                   cis_now=int((cis & now[:, 2]).sum()), cis_kept=int((cis & ~self.cis_changed).sum()))
        return out, vh


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_sample(got: dict, want: dict) -> bool:
    """Exact equality of two sample dicts: ints, and doubles as bit patterns."""
    return (all(int(got[k]) == int(want[k]) for k in SURVIVAL + ("origin_step", "last_step"))
            and all(np.array_equal(got[k], want[k]) for k in ("n", "n_clean"))
            and all(np.array_equal(bits(got[k]), bits(want[k])) for k in ("sum_u2", "sum_u2_clean")))


def same_info(info, want: dict) -> bool:
    got = info.as_dict()
    return (all(int(got[k]) == int(want[k]) for k in ("origin_step", "last_step", "n_updates", "n_jumped", "n_changed"))
            and all(np.array_equal(bits([got[k]]), bits([want[k]])) for k in ("max_dx", "max_dy")))
