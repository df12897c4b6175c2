"""Python reference of the bond-orientational order (include/kmc.h, DESIGN.md
§14), shared by test_bondorder_host.py and test_gpu_bondorder.py and
independent of the C code: coordinates, moduli and every comparison in Python
integers, brute force over all pairs (no cell grid); atan2 / cos / sin /
division / round_ through engine.math (the host kmc_math.h), the products
n theta and cos 2^30 in numpy float64 (elementwise numpy does not fuse), the
sums in Python integers.  Every comparison against it is exact equality."""
import numpy as np

from _kmc import capi, engine
from _structure import positions, selected

SCALE = 1073741824.0  # 2^30
ROWS = 16


def _round(a):
    """The library's round_ (half away from zero) as a list of Python ints."""
    return [int(v) for v in engine.math(6, np.ascontiguousarray(a, dtype=np.float64).ravel())]


def int_coords(p, hs, which):
    """(X, Y, BX, BY, sel): Python-int coordinates of the species' bead [1][1] and its selection flags (for both
    selections: sel["all"], sel["bound"])."""
    xy = positions(hs)
    lo, hi = (0, hs.n_a) if capi.bo_which(which) == capi.BO_A else (hs.n_a, hs.n_a + hs.n_b)
    X = _round(xy[lo:hi, 0] * 1024.0)
    Y = _round(xy[lo:hi, 1] * 1024.0)
    BX, BY = _round(np.array([p.box_x * 1024.0, p.box_y * 1024.0]))
    sel = {s: [bool(v) for v in selected(hs, s)[lo:hi]] for s in ("all", "bound")}
    return X, Y, BX, BY, sel


def disp(d, B):
    d %= B  # Python's modulus is the floor modulus
    return d - B if 2 * d >= B else d


def neighbour_lists(p, hs, which, mode, r_cut, select):
    """{i: [(j, DX, DY), ...]} for every selected protein i of the species (by its reference index), in the
    definition's order for the linked mode."""
    X, Y, BX, BY, sel = int_coords(p, hs, which)
    sel = sel[select if isinstance(select, str) else ("all", "bound")[select]]
    who = [i for i in range(len(X)) if sel[i]]
    out = {i: [] for i in who}
    if capi.bo_mode(mode) == capi.BO_WITHIN:
        RC = _round(np.array([r_cut * 1024.0]))[0]
        assert RC >= 1 and BX // RC >= 3 and BY // RC >= 3
        for i in who:
            for j in who:
                DX, DY = disp(X[j] - X[i], BX), disp(Y[j] - Y[i], BY)
                if 0 < DX * DX + DY * DY <= RC * RC:
                    out[i].append((j, DX, DY))
        return out
    assert capi.bo_which(which) == capi.BO_B
    na = hs.n_a
    for b in who:
        for site in (2, 3, 4):
            r = int(hs.b_int[4 + site - 1, b])
            if r == 0:
                continue
            r2 = int(hs.a_int[4, r - 1])  # the receptor's nei3: its cis partner
            if r2 == 0:
                continue
            l = int(hs.a_int[2, r2 - 1])  # the partner's nei2: its ligand
            if l == 0:
                continue
            b2 = l - 1 - na
            if b2 == b or not sel[b2]:
                continue
            DX, DY = disp(X[b2] - X[b], BX), disp(Y[b2] - Y[b], BY)
            if DX == 0 and DY == 0:
                continue
            out[b].append((b2, DX, DY))
    return out


def local_sums(nbr, n, fold):
    """(C[n], S[n], nn[n]) Python-int lists from neighbour lists; zeros outside the set."""
    flat = [(i, DX, DY) for i, lst in nbr.items() for _, DX, DY in lst]
    C, S, nn = [0] * n, [0] * n, [0] * n
    if flat:
        DX = np.array([f[1] for f in flat], dtype=np.float64)
        DY = np.array([f[2] for f in flat], dtype=np.float64)
        theta = engine.math(2, DY, DX)  # atan2(y, x)
        a = np.float64(fold) * theta
        tc = _round(engine.math(1, a) * SCALE)
        ts = _round(engine.math(0, a) * SCALE)
        for (i, _, _), c, s in zip(flat, tc, ts):
            C[i] += c
            S[i] += s
            nn[i] += 1
    return C, S, nn


def normalised(C, S, nn):
    """(pc, ps) Python-int lists: round_(C / (N * 32768.0)), zero where N = 0."""
    idx = [i for i in range(len(nn)) if nn[i] > 0]
    pc, ps = [0] * len(nn), [0] * len(nn)
    if idx:
        den = np.array([float(nn[i]) for i in idx]) * 32768.0
        qc = _round(engine.math(5, np.array([float(C[i]) for i in idx]), den))
        qs = _round(engine.math(5, np.array([float(S[i]) for i in idx]), den))
        for i, c, s in zip(idx, qc, qs):
            pc[i], ps[i] = c, s
    return pc, ps


def mag_bin(m, nbins):
    return sum(1 for k in range(1, nbins) if k * k * (1 << 30) <= nbins * nbins * m)


def ref_bond_order(p, hs, which, fold, r_cut=None, mode="within", select="all", nbins=64, nbr=None):
    """(hist[16, nbins] int64, summary dict, C, S, nn) as Simulation.bond_order(per_protein=True) returns them
    (the summary as BondOrderOut.as_dict())."""
    nbr = neighbour_lists(p, hs, which, mode, r_cut, select) if nbr is None else nbr
    n = hs.n_a if capi.bo_which(which) == capi.BO_A else hs.n_b
    C, S, nn = local_sums(nbr, n, fold)
    pc, ps = normalised(C, S, nn)
    hist = np.zeros((ROWS, nbins), dtype=np.int64)
    out = dict(n_sel=0, n_with=0, sum_nn=0, sum_pc=0, sum_ps=0, sum_m=0)
    for i in nbr:
        m = pc[i] * pc[i] + ps[i] * ps[i]
        out["n_sel"] += 1
        out["n_with"] += nn[i] > 0
        out["sum_nn"] += nn[i]
        out["sum_pc"] += pc[i]
        out["sum_ps"] += ps[i]
        out["sum_m"] += m
        hist[min(nn[i], ROWS - 1), mag_bin(m, nbins)] += 1
    return hist, out, np.array(C, dtype=np.int64), np.array(S, dtype=np.int64), np.array(nn, dtype=np.int32)


def corr_edges(r_max, nbins):
    dr = np.float64(r_max) / np.float64(nbins)
    return _round((np.arange(nbins + 1, dtype=np.float64) * dr) * 1024.0)


def ref_bond_order_corr(p, hs, which, fold, r_max, r_cut=None, mode="within", select="all", nbins=64, nbr=None):
    """corr[2, nbins] int64 as Simulation.bond_order_corr returns it: brute force over all pairs i < j."""
    nbr = neighbour_lists(p, hs, which, mode, r_cut, select) if nbr is None else nbr
    n = hs.n_a if capi.bo_which(which) == capi.BO_A else hs.n_b
    C, S, nn = local_sums(nbr, n, fold)
    pc, ps = normalised(C, S, nn)
    X, Y, BX, BY, _ = int_coords(p, hs, which)
    E2 = [e * e for e in corr_edges(r_max, nbins)]
    who = [i for i in sorted(nbr) if nn[i] > 0]
    num, cnt = [0] * nbins, [0] * nbins
    for a, i in enumerate(who):
        for j in who[a + 1:]:
            DX, DY = disp(X[j] - X[i], BX), disp(Y[j] - Y[i], BY)
            D2 = DX * DX + DY * DY
            if D2 >= E2[nbins]:
                continue
            k = sum(1 for m in range(1, nbins + 1) if E2[m] <= D2)
            if k < nbins:
                num[k] += pc[i] * pc[j] + ps[i] * ps[j]
                cnt[k] += 1
    return np.array([num, cnt], dtype=np.int64)


def bind_network(hs, triples):
    """Ligand–receptor=receptor–ligand bridges by hand: (ligand b, site sb, receptor r, receptor r2, ligand b2, site
    sb2), 0-based indices; b2 < 0 leaves the cis partner r2 without a ligand.  Every receptor is used once."""
    nr = hs.n_a
    for b, sb, r, r2, b2, sb2 in triples:
        for lig, site, rec in ((b, sb, r), (b2, sb2, r2)):
            if lig < 0:
                continue
            hs.a_int[0, rec] = 1
            hs.a_int[2, rec] = nr + lig + 1
            hs.a_int[3, rec] = site
            hs.b_int[site - 1, lig] = 1
            hs.b_int[4 + site - 1, lig] = rec + 1
        hs.a_int[1, r] = hs.a_int[1, r2] = 1
        hs.a_int[4, r] = r2 + 1
        hs.a_int[4, r2] = r + 1


def place_ligands(hs, x, y):
    """Translates every ligand as a rigid body so that bead [1][1] lies exactly at (x[b], y[b])."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    hs.rb[0::3] += (x - hs.rb[0])[None, :]
    hs.rb[1::3] += (y - hs.rb[1])[None, :]
    hs.rb[0], hs.rb[1] = x, y  # exactly: old + (target - old) may be an ulp off
    return hs
