"""Python-integer reference of the cluster geometry (include/kmc.h, DESIGN.md
§12), shared by test_geometry_host.py and test_gpu_geometry.py: a breadth-first
walk from each label that takes the image shifts from the edge rule, a pass over
every edge for the spanning bits, and the moments and the table in Python
integers.  Also the brick-wall lattice states.  Every comparison against it is
exact equality."""
import numpy as np

from _analysis import chain_state
from _kmc import capi, engine, params

SUMMARY = ("n_measured", "n_spanning", "n_span_x", "n_span_y", "proteins_in_spanning", "largest_label",
           "largest_size", "largest_span")
ROW = ("label", "n_r", "n_l", "span", "s1x", "s1y", "s2xx", "s2yy", "s2xy")


def _round(a):
    """The library's round_ (half away from zero; np.round rounds half to even)."""
    return engine.math(6, np.ascontiguousarray(a, dtype=np.float64).ravel()).reshape(np.shape(a))


def positions(hs) -> np.ndarray:
    """xy[N, 2] of bead [1][1], receptors then ligands."""
    return np.concatenate([np.stack([hs.ra[0], hs.ra[1]], axis=1), np.stack([hs.rb[0], hs.rb[1]], axis=1)])


def ref_geometry(p, hs) -> dict:
    """label[N] (1-based), shift[N, 2], span[N] and one record per component."""
    na, n = hs.n_a, hs.n_a + hs.n_b
    xy = positions(hs)
    box = (p.box_x, p.box_y)
    src = np.concatenate([np.arange(na)] * 2 + [na + np.arange(hs.n_b)] * 3)
    dst = np.concatenate([hs.a_int[2], hs.a_int[4], hs.b_int[5], hs.b_int[6], hs.b_int[7]]).astype(np.int64) - 1
    keep = dst >= 0
    src, dst = src[keep], dst[keep]
    # n(i->j) = -(int) round_((x_j - x_i) / box), in doubles
    shift_e = np.stack([-_round((xy[dst, c] - xy[src, c]) / box[c]).astype(np.int64) for c in (0, 1)], axis=1)
    adj = [[] for _ in range(n)]
    for s, d, e in zip(src.tolist(), dst.tolist(), shift_e.tolist()):
        adj[s].append((d, e[0], e[1]))
    X = [_round(xy[:, c] * 1024.0).astype(np.int64).tolist() for c in (0, 1)]
    B = [int(_round(np.array([b * 1024.0]))[0]) for b in box]
    label = np.zeros(n, dtype=np.int32)
    off = [[0, 0] for _ in range(n)]
    span = np.zeros(n, dtype=np.uint8)
    comps = []
    for r in range(n):
        if label[r]:
            continue
        label[r] = r + 1
        queue = [r]
        for q in queue:
            for j, ex, ey in adj[q]:
                if not label[j]:
                    label[j] = r + 1
                    off[j] = [off[q][0] + ex, off[q][1] + ey]
                    queue.append(j)
        bits = 0
        for q in queue:
            for j, ex, ey in adj[q]:
                bits |= 1 if off[j][0] - off[q][0] != ex else 0
                bits |= 2 if off[j][1] - off[q][1] != ey else 0
        c = dict(label=r + 1, n_r=sum(1 for q in queue if q < na), n_l=sum(1 for q in queue if q >= na), span=bits,
                 s1x=0, s1y=0, s2xx=0, s2yy=0, s2xy=0)
        if bits:
            for q in queue:
                off[q] = [0, 0]
                span[q] = bits
        else:
            for q in queue:
                dx = X[0][q] + off[q][0] * B[0] - X[0][r]
                dy = X[1][q] + off[q][1] * B[1] - X[1][r]
                c["s1x"] += dx
                c["s1y"] += dy
                c["s2xx"] += dx * dx
                c["s2yy"] += dy * dy
                c["s2xy"] += dx * dy
        comps.append(c)
    return dict(label=label, shift=np.array(off, dtype=np.int32).reshape(n, 2), span=span, comps=comps)


def comp_m(c) -> int:
    n = c["n_r"] + c["n_l"]
    return n * (c["s2xx"] + c["s2yy"]) - (c["s1x"] ** 2 + c["s1y"] ** 2)


def ref_table(ref, max_size):
    """[(count, sum_size, sum_m)] for the bins 0..max_size, Python ints."""
    t = [[0, 0, 0] for _ in range(max_size + 1)]
    for c in ref["comps"]:
        n = c["n_r"] + c["n_l"]
        if c["span"] or n < 2:
            continue
        m = comp_m(c)
        assert m >= 0
        b = t[min(n, max_size)]
        b[0] += 1
        b[1] += n
        b[2] += m
    return [tuple(b) for b in t]


def ref_summary(ref) -> dict:
    cs = ref["comps"]
    size = [c["n_r"] + c["n_l"] for c in cs]
    big = max(range(len(cs)), key=lambda k: (size[k], -cs[k]["label"]))
    sp = [k for k, c in enumerate(cs) if c["span"]]
    return dict(n_measured=sum(1 for k, c in enumerate(cs) if not c["span"] and size[k] >= 2), n_spanning=len(sp),
                n_span_x=sum(1 for k in sp if cs[k]["span"] & 1), n_span_y=sum(1 for k in sp if cs[k]["span"] & 2),
                proteins_in_spanning=sum(size[k] for k in sp), largest_label=cs[big]["label"], largest_size=size[big],
                largest_span=cs[big]["span"])


def ref_rows(ref, min_size):
    """kmc_cluster_list's rows as dicts, in label order."""
    return [c for c in ref["comps"] if c["n_r"] + c["n_l"] >= min_size]


def table_tuples(table):
    """A capi.GEOM_BIN_DTYPE table as [(count, sum_size, sum_m)] with Python ints."""
    return [(int(c), int(s), m) for c, s, m in zip(table["count"], table["sum_size"], capi.geom_m(table))]


def summary_dict(g) -> dict:
    return {k: int(getattr(g, k)) for k in SUMMARY}


def row_dicts(rows):
    return [{k: r.as_dict()[k] for k in ROW} for r in rows]


def check_against(ref, label, shift, span, tables, summary, rows=None, min_size=None):
    """label / shift / span, {max_size: table}, the summary and (optionally) the list rows equal the reference."""
    assert np.array_equal(label, ref["label"])
    assert np.array_equal(shift, ref["shift"])
    assert np.array_equal(span, ref["span"])
    for max_size, table in tables.items():
        assert table_tuples(table) == ref_table(ref, max_size)
    assert summary_dict(summary) == ref_summary(ref)
    if rows is not None:
        assert row_dicts(rows) == ref_rows(ref, min_size)


# ------------------------------------------------------------------ brick-wall lattice
NX, NY, PITCH = 64, 32, 200.0


def lattice_state(keep_x: bool, keep_y: bool, seed=11):
    """One component of NX x NY ligands on a brick-wall lattice (every ligand has
    three edges: left, right, and up or down by the parity of i + j) in a periodic
    box of exactly NX x NY pitches; an edge is one receptor on each ligand, the
    two cis-bound.  keep_x / keep_y keep the cis bonds of the edges that close the
    lattice around the box along x / y: the component then wraps the box on that
    axis.  The lattice's own seam lies in the middle of the box and the box's
    seam (x = +-box/2) in the middle of the lattice, so the open lattice
    straddles both seams of the box.  Indices are permuted.  Positions: a random
    placement, each rigid body translated so that bead [1][1] lands on its
    lattice point (a ligand) or a third of the way along its edge (a receptor).
    host_init_random places this density (one ligand per 200 x 200) as it is."""
    nl, nr = NX * NY, 3 * NX * NY
    p = params(seed=seed, n_a=nr, n_b=nl, box_x=NX * PITCH, box_y=NY * PITCH, box_z=1000.0)
    hs = engine.host_init_random(p)
    rng = np.random.default_rng(seed)
    lig = rng.permutation(nl)  # lattice point i * NY + j -> ligand
    rec = (rng.permutation(nr) + 1).tolist()  # receptors in the order they are used
    hs.a_int[:] = 0
    hs.b_int[:] = 0
    # lattice point (i, j) at origin + pitch * (i, j), wrapped into [-box/2, box/2): the columns past NX/2 and the rows
    # past NY/2 lie beyond the box's seam
    origin = np.array([-13.37, -7.77])
    box = np.array([p.box_x, p.box_y])

    def wrap(v):
        return v - box * np.floor(v / box + 0.5)

    def move(arr, col, target):
        d = target - arr[0:2, col]
        arr[0::3, col] += d[0]
        arr[1::3, col] += d[1]

    def bind(r, b, site):
        hs.a_int[0, r - 1] = 1
        hs.a_int[2, r - 1] = nr + b + 1
        hs.a_int[3, r - 1] = site
        hs.b_int[site - 1, b] = 1
        hs.b_int[4 + site - 1, b] = r

    for i in range(NX):
        for j in range(NY):
            a = np.array([i, j])
            move(hs.rb, lig[i * NY + j], wrap(origin + PITCH * a))
            # the edges this point starts: to the right (site 2 -> the neighbour's site 3), and up (site 4 both) when i + j is even
            for step, sa, sb in (((1, 0), 2, 3),) + ((((0, 1), 4, 4),) if (i + j) % 2 == 0 else ()):
                i2, j2 = i + step[0], j + step[1]
                closes = (i2 == NX, j2 == NY)
                ra, rb_ = rec.pop(), rec.pop()
                bind(ra, lig[i * NY + j], sa)
                bind(rb_, lig[(i2 % NX) * NY + j2 % NY], sb)
                move(hs.ra, ra - 1, wrap(origin + PITCH * (a + np.array(step) / 3.0)))
                move(hs.ra, rb_ - 1, wrap(origin + PITCH * (a + 2.0 * np.array(step) / 3.0)))
                if (closes[0] and not keep_x) or (closes[1] and not keep_y):
                    continue
                hs.a_int[1, ra - 1] = hs.a_int[1, rb_ - 1] = 1
                hs.a_int[4, ra - 1] = rb_
                hs.a_int[4, rb_ - 1] = ra
    assert not rec
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs


def far_chain_state(scale=64.0):
    """_analysis.chain_state() with every rigid body moved to `scale` times its position in a box as many times
    larger: the same graph and the same image shifts, but squared distances that pass 2^64 one by one."""
    p, hs = chain_state()
    p.box_x, p.box_y = p.box_x * scale, p.box_y * scale
    for arr in (hs.ra, hs.rb):
        d = arr[0:2] * (scale - 1.0)
        arr[0::3] += d[0]
        arr[1::3] += d[1]
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs
