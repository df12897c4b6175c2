"""Python reference of the structure factor (include/kmc.h),
shared by test_structure_host.py and test_gpu_structure.py and independent of
the C code: the phases' moduli in Python integers, t and a in numpy float64
(elementwise numpy does not fuse), cos / sin / round_ through engine.math (the
host kmc_math.h), the products in numpy and the sums in Python integers.  Also
the ligand lattice whose Bragg peaks are known.  Every comparison against it is
exact equality."""
import numpy as np

from _kmc import capi, engine, params

TWO_PI = 6.283185307179586
SCALE = 1073741824.0  # 2^30


def _round(a):
    """The library's round_ (half away from zero; np.round rounds half to even)."""
    return engine.math(6, np.ascontiguousarray(a, dtype=np.float64).ravel()).reshape(np.shape(a))


def positions(hs) -> np.ndarray:
    """xy[N, 2] of bead [1][1], receptors then ligands."""
    return np.concatenate([np.stack([hs.ra[0], hs.ra[1]], axis=1), np.stack([hs.rb[0], hs.rb[1]], axis=1)])


def selected(hs, select) -> np.ndarray:
    """bool[N]: the proteins kmc_structure_factor sums over."""
    n = hs.n_a + hs.n_b
    if capi.sk_select(select) == capi.SK_ALL:
        return np.ones(n, dtype=bool)
    a = (hs.a_int[2] != 0) | (hs.a_int[4] != 0)                          # nei2, nei3
    b = (hs.b_int[5] != 0) | (hs.b_int[6] != 0) | (hs.b_int[7] != 0)      # nei2..4
    return np.concatenate([a, b])


def axis_tables(coord, box, mmax):
    """(c[mmax + 1, n], s[mmax + 1, n]) of the axis phases of the multipliers 0..mmax."""
    X = [int(v) for v in _round(np.asarray(coord, dtype=np.float64) * 1024.0)]
    B = int(_round(np.array([box * 1024.0]))[0])
    assert B >= 1
    p = np.empty((mmax + 1, len(X)), dtype=np.float64)
    for m in range(mmax + 1):
        for i, x in enumerate(X):
            r = (m * x) % B  # Python's modulus is the floor modulus
            if 2 * r >= B:
                r -= B
            p[m, i] = float(r)  # |r| < 2^53: exact
    t = p / np.float64(B)
    a = TWO_PI * t
    return engine.math(1, a.ravel()).reshape(a.shape), engine.math(0, a.ravel()).reshape(a.shape)


def terms(cx, sx, cy, sy, k):
    """(tc, ts) int64 arrays over the proteins at one h (cx, sx) and one k (cy, sy of |k|)."""
    if k < 0:
        sy = -sy
    re = cx * cy - sx * sy
    im = sx * cy + cx * sy
    return _round(re * SCALE).astype(np.int64), _round(im * SCALE).astype(np.int64)


def ref_structure_factor(p, hs, hmax, kmax, select="all"):
    """(sums[4, hmax + 1, 2 kmax + 1] int64, n_sel[2]) as Simulation.structure_factor returns them."""
    xy = positions(hs)
    keep = selected(hs, select)
    species = np.arange(hs.n_a + hs.n_b) >= hs.n_a
    sums = np.zeros((4, hmax + 1, 2 * kmax + 1), dtype=np.int64)
    n_sel = np.zeros(2, dtype=np.int64)
    for sp in (0, 1):
        who = np.flatnonzero(keep & (species == bool(sp)))
        n_sel[sp] = len(who)
        cx, sx = axis_tables(xy[who, 0], p.box_x, hmax)
        cy, sy = axis_tables(xy[who, 1], p.box_y, kmax)
        for h in range(hmax + 1):
            for k in range(-kmax, kmax + 1):
                tc, ts = terms(cx[h], sx[h], cy[abs(k)], sy[abs(k)], k)
                sums[2 * sp, h, k + kmax] = sum(int(v) for v in tc)
                sums[2 * sp + 1, h, k + kmax] = sum(int(v) for v in ts)
    return sums, n_sel


def one_term(p, x, y, h, k):
    """(tc, ts) Python ints of a single protein at (x, y)."""
    cx, sx = axis_tables([x], p.box_x, h)
    cy, sy = axis_tables([y], p.box_y, abs(k))
    tc, ts = terms(cx[h], sx[h], cy[abs(k)], sy[abs(k)], k)
    return int(tc[0]), int(ts[0])


def bind_some(hs, pairs):
    """R–L bonds by hand, as _geometry.lattice_state sets them: (receptor, ligand, site), 0-based, and a cis
    bond between the first two receptors."""
    nr = hs.n_a
    for r, b, site in pairs:
        hs.a_int[0, r] = 1
        hs.a_int[2, r] = nr + b + 1
        hs.a_int[3, r] = site
        hs.b_int[site - 1, b] = 1
        hs.b_int[4 + site - 1, b] = r + 1
    r0, r1 = pairs[0][0], pairs[1][0]
    hs.a_int[1, r0] = hs.a_int[1, r1] = 1
    hs.a_int[4, r0] = r1 + 1
    hs.a_int[4, r1] = r0 + 1


def snap_to_grid(hs):
    """Translates every rigid body so that bead [1][1] lies on the 2^-10 A grid of the integer coordinates
    (by less than 2^-11 A per axis): X / 1024 is then the position itself."""
    for arr in (hs.ra, hs.rb):
        target = np.round(arr[0:2] * 1024.0) / 1024.0
        d = target - arr[0:2]
        arr[0::3] += d[0]
        arr[1::3] += d[1]
        arr[0:2] = target  # exactly: old + (target - old) may be an ulp off
    return hs


# ------------------------------------------------------------------ ligand lattice
PITCH = 200.0
ORIGIN = (0.25, -0.5)


def lattice_state(nx, ny, n_a=16, seed=17):
    """nx x ny ligands with bead [1][1] exactly on ORIGIN + PITCH (i, j), wrapped into the periodic box of
    exactly nx x ny pitches (every coordinate a multiple of 2^-10 A: the wrap is exact); each rigid body is
    translated as a whole.  The receptors stay where host_init_random put them.  No bonds."""
    p = params(seed=seed, n_a=n_a, n_b=nx * ny, box_x=nx * PITCH, box_y=ny * PITCH, box_z=1000.0)
    hs = engine.host_init_random(p)
    box = np.array([p.box_x, p.box_y])
    lig = np.random.default_rng(seed).permutation(nx * ny)  # lattice point i * ny + j -> ligand
    for i in range(nx):
        for j in range(ny):
            v = np.array(ORIGIN) + PITCH * np.array([i, j], dtype=np.float64)
            target = v - box * np.floor(v / box + 0.5)
            col = lig[i * ny + j]
            d = target - hs.rb[0:2, col]
            hs.rb[0::3, col] += d[0]
            hs.rb[1::3, col] += d[1]
            hs.rb[0:2, col] = target  # exactly: old + (target - old) may be an ulp off
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs


def check_lattice(p, sums, n_sel, nx, ny, hmax, kmax):
    """The ligand sums of lattice_state: n_b times one ligand's term at the Bragg vectors, within n_b of zero
    elsewhere (the exact sum is 0 there and each term is off by less than 0.51)."""
    n_b = nx * ny
    assert int(n_sel[1]) == n_b
    assert hmax >= nx and kmax >= ny  # a Bragg vector besides q = 0 on either axis
    for h in range(hmax + 1):
        for k in range(-kmax, kmax + 1):
            C, S = int(sums[2, h, k + kmax]), int(sums[3, h, k + kmax])
            if h % nx == 0 and k % ny == 0:
                tc0, ts0 = one_term(p, ORIGIN[0], ORIGIN[1], h, k)
                assert (C, S) == (n_b * tc0, n_b * ts0), (h, k)
            else:
                assert abs(C) <= n_b and abs(S) <= n_b, (h, k)
