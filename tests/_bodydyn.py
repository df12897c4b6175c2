"""Python reference of the body dynamics (include/kmc.h), shared
by test_bodydyn_host.py and test_gpu_bodydyn.py and independent of the C code:
components by a breadth-first walk, the image shifts of tests/_geometry.py's
reference, coordinates in numpy int64, every body's sums in Python integers as
the definition writes them (D = D0 + u - u_r member by member, no
rearrangement), round_, atan2 and cos through engine.math (the host
kmc_math.h).  Every comparison against it is exact equality.

Also the hand-built graphs of the tests: paths of receptors and ligands of any
length (path_state)."""
import numpy as np

from _geometry import ref_geometry
from _kmc import capi, engine
from _lagcorr import icoords, links, min_image

COUNTS = capi.BD_COUNTS
SUMS = capi.BD_SUMS
ROW = ("label", "n_r", "n_l", "bits", "status", "is_", "cur_label", "cur_size", "su_x", "su_y", "C", "S")


def _round(a):
    """The library's round_ (half away from zero; np.round rounds half to even)."""
    return engine.math(6, np.ascontiguousarray(a, dtype=np.float64).ravel()).reshape(np.shape(a))


def _round1(x) -> int:
    return int(_round(np.array([x], dtype=np.float64))[0])


def bfs_labels(hs) -> np.ndarray:
    """label[i] (1-based): the smallest reference index of protein i's component, by a breadth-first walk."""
    na, n = hs.n_a, hs.n_a + hs.n_b
    l = links(hs)
    adj = [[] for _ in range(n)]
    for i in range(n):
        for k in ((0, 2) if i < na else (0, 1, 2)):  # (a receptor's middle entry is the ligand's site, no link)
            if l[i, k]:
                adj[i].append(int(l[i, k]) - 1)
    label = np.zeros(n, dtype=np.int32)
    for r in range(n):
        if label[r]:
            continue
        label[r] = r + 1
        queue = [r]
        for q in queue:
            for j in adj[q]:
                if not label[j]:
                    label[j] = r + 1
                    queue.append(j)
    return label


def rot_terms(C: int, S: int):
    """(c1, c2, p) of C, S not both zero."""
    phi = engine.math(2, np.array([float(S)]), np.array([float(C)]))  # atan2(S, C)
    c1 = _round1(engine.math(1, phi)[0] * 1073741824.0)
    c2 = _round1(engine.math(1, 2.0 * phi)[0] * 1073741824.0)
    return c1, c2, _round1(phi[0] * 16777216.0), float(phi[0])


class RefBd:
    """The recorder of include/kmc.h on host states."""

    def __init__(self, p, hs, every, max_size, max_jump=0.0, max_disp=0.0):
        self.p, self.every, self.max_size = p, every, max_size
        half = 0.5 * min(p.box_x, p.box_y)
        self.max_jump = max_jump if max_jump > 0.0 else 0.5 * half
        self.max_disp = max_disp if max_disp > 0.0 else 16384.0
        self.J = _round1(self.max_jump * 1024.0)
        self.F = _round1(self.max_disp * 1024.0)
        self.B = [_round1(b * 1024.0) for b in (p.box_x, p.box_y)]
        self.n_a = hs.n_a
        self.X0 = icoords(hs)
        self.prev = self.X0.copy()
        self.U = self.X0.copy()
        self.links = links(hs)
        self.flags = np.zeros(len(self.U), dtype=np.uint8)
        geo = ref_geometry(p, hs)
        self.label = geo["label"].astype(np.int32)
        assert np.array_equal(self.label, bfs_labels(hs))
        self.shift = geo["shift"].astype(np.int64)  # (zero in a spanning component)
        root = self.label.astype(np.int64) - 1
        self.D0 = self.X0 + self.shift * np.array(self.B, dtype=np.int64) - self.X0[root]
        wide_root = np.zeros(len(self.U), dtype=bool)
        wide_root[root[(np.abs(self.D0) >= 1 << 24).any(axis=1)]] = True
        self.bits = (geo["span"].astype(np.uint8) | (wide_root[root] * capi.BD_WIDE).astype(np.uint8))
        self.members = {}
        for i, r in enumerate(root.tolist()):
            self.members.setdefault(r, []).append(i)
        self.n = 0
        self.crossed = np.zeros(len(self.U), dtype=bool)  # a protein whose wrapped coordinate jumped across the seam
        self.origin_step = self.last_step = hs.step

    def update(self, hs):
        """Returns (newly jumped, newly changed)."""
        assert hs.step == self.last_step + self.every
        X = icoords(hs)
        raw = X - self.prev
        d = np.stack([min_image(raw[:, c], self.B[c]) for c in range(2)], axis=1)
        self.crossed |= (d != raw).any(axis=1)
        self.U += d
        self.prev = X
        l_now = links(hs)
        f = ((np.abs(d) >= self.J).any(axis=1) * capi.BD_JUMPED | (l_now != self.links).any(axis=1) * capi.BD_CHANGED)
        f = f.astype(np.uint8)
        self.links = l_now
        fresh = f & ~self.flags
        self.flags |= f
        self.n += 1
        self.last_step = hs.step
        return int(np.count_nonzero(fresh & capi.BD_JUMPED)), int(np.count_nonzero(fresh & capi.BD_CHANGED))

    def rows(self, hs, min_size=1):
        """One dict per body of at least min_size members, by label, with phi (a float, None without a rotation)."""
        assert hs.step == self.last_step
        cur = bfs_labels(hs)
        size = np.bincount(cur, minlength=len(cur) + 1)
        u = (self.U - self.X0).tolist()
        D0 = self.D0.tolist()
        out = []
        for r in sorted(self.members):
            mem = self.members[r]
            n = len(mem)
            if n < min_size:
                continue
            n_r = sum(1 for i in mem if i < self.n_a)
            bits = int(self.bits[r])
            L = sorted({int(cur[i]) for i in mem})
            status = capi.BD_BROKEN if len(L) > 1 else capi.BD_INTACT if int(size[L[0]]) == n else capi.BD_GROWN
            row = dict(label=r + 1, n_r=n_r, n_l=n - n_r, bits=bits, status=status, is_=0, cur_label=L[0],
                       cur_size=int(size[L[0]]), su_x=0, su_y=0, C=0, S=0, phi=None)
            if not any(self.flags[i] for i in mem):
                row["is_"] |= capi.BD_IS_PRISTINE
                if all(abs(u[i][0]) < self.F and abs(u[i][1]) < self.F for i in mem):
                    row["is_"] |= capi.BD_IS_VALID
                    row["su_x"] = sum(u[i][0] for i in mem)
                    row["su_y"] = sum(u[i][1] for i in mem)
                    if 2 <= n <= capi.BD_ROT_MAX and not bits:
                        row["is_"] |= capi.BD_IS_ROT
                        for i in mem:
                            dx, dy = D0[i][0] + u[i][0] - u[r][0], D0[i][1] + u[i][1] - u[r][1]
                            row["C"] += D0[i][0] * dx + D0[i][1] * dy
                            row["S"] += D0[i][0] * dy - D0[i][1] * dx
                        assert abs(row["C"]) < 1 << 61 and abs(row["S"]) < 1 << 61
            out.append(row)
        return out

    def table(self, hs):
        """{field: [2][max_size + 1] Python ints} and the rows it was made of."""
        ms = self.max_size
        t = {name: [[0] * (ms + 1) for _ in range(2)] for name in COUNTS + SUMS}
        rows = self.rows(hs)
        for b in rows:
            n = b["n_r"] + b["n_l"]
            at = (int(b["n_l"] > 0), min(n, ms))

            def add(name, v=1):
                t[name][at[0]][at[1]] += v

            add("n_bodies")
            add("sum_size", n)
            add(("n_intact", "n_grown", "n_broken")[b["status"]])
            if b["is_"] & capi.BD_IS_PRISTINE:
                add("n_pristine")
            if not b["is_"] & capi.BD_IS_VALID:
                continue
            add("n_valid")
            add("m2", b["su_x"] ** 2 + b["su_y"] ** 2)
            if not b["is_"] & capi.BD_IS_ROT:
                if n >= 2:
                    add("n_rot_skipped")
                continue
            if b["C"] == 0 and b["S"] == 0:
                add("n_rot_null")
                continue
            c1, c2, ph, b["phi"] = rot_terms(b["C"], b["S"])
            add("n_rot")
            add("c1", c1)
            add("c2", c2)
            add("phi2", ph * ph)
        return t, rows


def sample_table(s):
    """A capi.BdSample's table as the lists RefBd.table() returns."""
    return {name: [[int(x) for x in row] for row in getattr(s, name)] for name in COUNTS + SUMS}


def same_sample(s, ref, table):
    return sample_table(s) == table and (s.J, s.F, s.BX, s.BY) == (ref.J, ref.F, ref.B[0], ref.B[1]) and (
        s.origin_step, s.last_step, s.total_bodies) == (ref.origin_step, ref.last_step, len(ref.members))


def body_tuples(bodies):
    """The record array of bd_bodies as tuples in ROW's order."""
    return [tuple(r[:8]) + (r[8][0], r[8][1], r[9], r[10]) for r in bodies.tolist()]


def row_tuples(rows):
    return [tuple(r[k] for k in ROW) for r in rows]


def same_arrays(U, X0, flags, label, D0, ref):
    return (np.array_equal(U, ref.U) and np.array_equal(X0, ref.X0) and np.array_equal(flags, ref.flags) and
            np.array_equal(label, ref.label) and np.array_equal(D0, ref.D0))


def identities(t):
    """The table's identities (include/kmc.h) on the lists of RefBd.table() / sample_table()."""
    for hl in range(2):
        for k in range(len(t["n_bodies"][0])):
            g = lambda name: t[name][hl][k]
            assert g("n_intact") + g("n_grown") + g("n_broken") == g("n_bodies")
            assert g("n_valid") <= g("n_pristine") <= g("n_bodies")
            assert g("n_rot") + g("n_rot_null") + g("n_rot_skipped") <= g("n_valid")
            if k == 0:
                assert all(t[name][hl][0] == 0 for name in t)


# ---------------------------------------------------------------- hand-built graphs
def blank_state(p, step=0):
    """A host state with no bond, every bead at the origin; the tests place bead [1][1] and bind."""
    hs = capi.HostState(p.n_a, p.n_b)
    hs.step = step
    return hs


def set_xy(hs, i, x, y):
    """Bead [1][1] of the protein with 0-based reference index i."""
    if i < hs.n_a:
        hs.ra[0, i], hs.ra[1, i] = x, y
    else:
        hs.rb[0, i - hs.n_a], hs.rb[1, i - hs.n_a] = x, y


def get_xy(hs):
    return np.concatenate([np.stack([hs.ra[0], hs.ra[1]], axis=1), np.stack([hs.rb[0], hs.rb[1]], axis=1)])


def put_xy(hs, xy):
    na = hs.n_a
    hs.ra[0], hs.ra[1] = xy[:na, 0], xy[:na, 1]
    hs.rb[0], hs.rb[1] = xy[na:, 0], xy[na:, 1]


def bind(hs, r, b, site):
    """Receptor r (0-based) on site 2..4 of ligand b (0-based among the ligands)."""
    hs.a_int[0, r] = 1
    hs.a_int[2, r] = hs.n_a + b + 1
    hs.a_int[3, r] = site
    hs.b_int[site - 1, b] = 1
    hs.b_int[4 + site - 1, b] = r + 1


def unbind(hs, r):
    b, site = int(hs.a_int[2, r]) - hs.n_a - 1, int(hs.a_int[3, r])
    hs.a_int[0, r] = hs.a_int[2, r] = hs.a_int[3, r] = 0
    hs.b_int[site - 1, b] = hs.b_int[4 + site - 1, b] = 0


def cis(hs, r1, r2):
    hs.a_int[1, r1] = hs.a_int[1, r2] = 1
    hs.a_int[4, r1] = r2 + 1
    hs.a_int[4, r2] = r1 + 1


def uncis(hs, r1):
    r2 = int(hs.a_int[4, r1]) - 1
    hs.a_int[1, r1] = hs.a_int[1, r2] = 0
    hs.a_int[4, r1] = hs.a_int[4, r2] = 0


def path(hs, rec, lig, size):
    """Binds a path of `size` proteins R - L - R = R - L - R = ... (- a ligand bond on sites 2 and 3, = a cis bond)
    from the iterators rec and lig of free 0-based receptor / ligand indices; returns the members' reference indices
    in path order.  Any size >= 1 is a connected body."""
    mem, prev_r, cur_l = [], None, None
    for t in range(size):
        kind = t % 3
        if kind == 1:
            cur_l = next(lig)
            bind(hs, prev_r, cur_l, 2)
            mem.append(hs.n_a + cur_l)
            continue
        r = next(rec)
        if kind == 2:
            bind(hs, r, cur_l, 3)
        elif prev_r is not None:
            cis(hs, prev_r, r)
        prev_r = r
        mem.append(r)
    return mem
