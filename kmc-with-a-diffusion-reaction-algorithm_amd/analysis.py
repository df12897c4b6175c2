"""Post-processing of the on-device structure analysis (engine.Simulation.census /
pair_counts) and displacement tracking (track_sample): g(r) from the lateral
pair counts, per-class mean-squared displacements and the diffusion fit, the
radius of gyration by cluster size, the fractal fit and the cluster shapes from
the cluster geometry (cluster_geometry / cluster_list), the partial static
structure factors S(q) and their radial average from the integer sums of
structure_factor, the global bond-orientational order and its correlation
G_n(r) from the integers of bond_order / bond_order_corr, the effective on- and
off-rates, the rebinding fraction and the Kaplan–Meier survival of bond
lifetimes from the bond kinetics recorder (kin_sample), the coagulation and
fragmentation kernels K(a, b), F(a, b) and the growth modes from the cluster
growth recorder (cf_sample), the hexagon fraction and ring densities of the
ligand network from the ring counts (rings), the distinct van Hove function
G_d(r, t) and the displacement correlation C_u(r, t) from the pair dynamics
(pd_sample), the centre-of-mass MSD, diffusion coefficient, rotation and
survival of clusters by size from the body dynamics (bd_sample), and the replica sums of integer histograms,
float64 sums and geometry tables.

The counts and sums themselves come from libkmc (kmc_analysis.hip,
kmc_dynamics.hip, kmc_geometry.hip, kmc_structure.hip, kmc_bondorder.hip,
kmc_kinetics.hip, kmc_coag.hip, kmc_rings.hip, kmc_pairdyn.hip, kmc_bodydyn.hip);
nothing here touches a trajectory.
"""
from __future__ import annotations

import numpy as np

from . import capi


def rdf(counts, n_i: int, n_j: int, box_x: float, box_y: float, r_max: float, same: bool) -> np.ndarray:
    """Lateral pair correlation g(r) per bin from kmc_pair_counts' histogram.

    Bin k covers [k·dr, (k+1)·dr), dr = r_max / nbins.  An ideal gas of the same
    densities in the periodic box_x × box_y plane puts
    pairs · π(r_{k+1}² − r_k²) / (box_x · box_y) pairs into it, where pairs is
    n_i (n_i − 1) / 2 unordered pairs of one species (`same`: AA, BB) or
    n_i · n_j receptor–ligand pairs (AB); g is the count over that number
    (zeros when there is no pair at all).
    """
    counts = np.asarray(counts, dtype=np.float64)
    nbins = counts.size
    dr = r_max / nbins
    edges = np.arange(nbins + 1, dtype=np.float64) * dr
    area = np.pi * (edges[1:] ** 2 - edges[:-1] ** 2)
    pairs = n_i * (n_i - 1) / 2.0 if same else float(n_i) * float(n_j)
    ideal = pairs * area / (box_x * box_y)
    return np.divide(counts, ideal, out=np.zeros_like(counts), where=ideal > 0)


def reduce_counts(array, device=None, group=None) -> np.ndarray:
    """SUM all-reduce of an int64 histogram (census bins, pair counts) over the
    ranks of an ensemble, the way ensemble.reduce sums the observables: RCCL
    (`torch.distributed` backend "nccl") on device tensors, gloo on CPU.
    Without an initialised process group the array comes back unchanged."""
    import torch
    import torch.distributed as dist

    a = np.ascontiguousarray(array, dtype=np.int64)
    t = torch.from_numpy(a.copy())
    if device is not None:
        t = t.to(device)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t.cpu().numpy()


def msd(sample, clean: bool = True) -> np.ndarray:
    """Mean-squared displacement per class from a track_sample result (a
    capi.TrackSample or its as_dict()): sum_u2_clean / n_clean, the proteins
    that neither changed their bonds nor jumped (`clean=False`: sum_u2 / n,
    every member of the origin class).  Empty classes give 0."""
    get = sample.get if isinstance(sample, dict) else lambda k: getattr(sample, k)
    s = np.array(list(get("sum_u2_clean" if clean else "sum_u2")), dtype=np.float64)
    n = np.array(list(get("n_clean" if clean else "n")), dtype=np.float64)
    return np.divide(s, n, out=np.zeros_like(s), where=n > 0)


def diffusion_fit(t, msd_values) -> float:
    """Lateral diffusion coefficient from MSD(t) = 4 D t + c in two dimensions:
    the least-squares slope of msd_values over t, divided by 4 (units of the
    inputs: A^2 / ns for t in ns).  Needs two distinct times."""
    t = np.asarray(t, dtype=np.float64)
    m = np.asarray(msd_values, dtype=np.float64)
    if t.shape != m.shape or t.ndim != 1 or t.size < 2:
        raise ValueError("diffusion_fit: t and msd as 1-d arrays of one length >= 2")
    tc = t - t.mean()
    den = float(np.dot(tc, tc))
    if den == 0.0:
        raise ValueError("diffusion_fit: all times are equal")
    return float(np.dot(tc, m - m.mean()) / den / 4.0)


def reduce_sums(array, device=None, group=None) -> np.ndarray:
    """SUM all-reduce of float64 sums (track_sample's sum_u2) over the ranks of
    an ensemble: the counterpart of reduce_counts, whose int64 path serves the
    counts and the van Hove bins.  Without an initialised process group the
    array comes back unchanged."""
    import torch
    import torch.distributed as dist

    a = np.ascontiguousarray(array, dtype=np.float64)
    t = torch.from_numpy(a.copy())
    if device is not None:
        t = t.to(device)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t.cpu().numpy()


# ---------------------------------------------------------------- cluster geometry
def rg_by_size(table):
    """Mean squared radius of gyration by cluster size from kmc_cluster_geometry's
    table (capi.GEOM_BIN_DTYPE, bin k = min(size, max_size)).

    Returns (sizes, counts, rg2, overflow): the sizes 2 .. max_size − 1 that hold a
    cluster, their counts and mean Rg² in Å² — sum_m / (count · n² · 2^20), the
    integer quotient rounded once — and the last bin apart, as a dict with its
    count, sum_size and rg2.  That bin mixes every size >= max_size; its rg2 is
    given only when sum_size == count · max_size (all of them are exactly
    max_size), else None."""
    table = np.asarray(table)
    max_size = len(table) - 1
    m = capi.geom_m(table)
    sizes, counts, rg2 = [], [], []
    for k in range(2, max_size):
        c = int(table["count"][k])
        if c:
            sizes.append(k)
            counts.append(c)
            rg2.append(m[k] / (c * k * k * (1 << 20)))
    c, ss = int(table["count"][max_size]), int(table["sum_size"][max_size])
    over = dict(count=c, sum_size=ss, rg2=m[max_size] / (c * max_size * max_size * (1 << 20))
                if c and ss == c * max_size else None)
    return (np.array(sizes, dtype=np.int64), np.array(counts, dtype=np.int64), np.array(rg2, dtype=np.float64), over)


def fractal_fit(sizes, rg2, counts, min_size: int = 2):
    """Fractal dimension from Rg ∝ n^(1/d_f): the least-squares line of log Rg
    (= log(rg2) / 2) over log n, every size >= min_size with rg2 > 0 weighted by
    its count.  Returns (slope, intercept, d_f = 1 / slope).  Needs two sizes."""
    n = np.asarray(sizes, dtype=np.float64)
    r2 = np.asarray(rg2, dtype=np.float64)
    w = np.asarray(counts, dtype=np.float64)
    keep = (n >= min_size) & (r2 > 0) & (w > 0)
    if np.count_nonzero(keep) < 2:
        raise ValueError("fractal_fit: fewer than two sizes to fit")
    x, y, w = np.log(n[keep]), 0.5 * np.log(r2[keep]), w[keep]
    xm, ym = np.sum(w * x) / w.sum(), np.sum(w * y) / w.sum()
    slope = float(np.sum(w * (x - xm) * (y - ym)) / np.sum(w * (x - xm) ** 2))
    return slope, float(ym - slope * xm), 1.0 / slope


def cluster_shapes(rows, params, xy):
    """Shape of each row of kmc_cluster_list (capi.Cluster) in float64 from its
    integer sums.  xy[N, 2] are the positions (bead [1][1], Å) by reference
    index: a row's sums are taken against its label's position.

    Returns a dict of arrays over the rows: label, size, span, centre[., 2] (the
    centre of mass wrapped into the box), rg (Å), lam1 >= lam2 (the eigenvalues
    of the gyration tensor, Å²; rg² = lam1 + lam2) and asphericity
    ((lam1 − lam2)² / (lam1 + lam2)²: 0 a disc, 1 a rod).  Spanning rows have
    no shape: NaN."""
    xy = np.asarray(xy, dtype=np.float64)
    box = (params.box_x, params.box_y)
    q = float(1 << 20)
    out = dict(label=[], size=[], span=[], centre=[], rg=[], lam1=[], lam2=[], asphericity=[])
    for r in rows:
        d = r.as_dict()
        n = d["n_r"] + d["n_l"]
        out["label"].append(d["label"])
        out["size"].append(n)
        out["span"].append(d["span"])
        if d["span"]:
            out["centre"].append((np.nan, np.nan))
            for k in ("rg", "lam1", "lam2", "asphericity"):
                out[k].append(np.nan)
            continue
        c = []
        for ax, s1 in enumerate((d["s1x"], d["s1y"])):
            xr = np.round(xy[d["label"] - 1, ax] * 1024.0)  # X_r (half-way cases never matter at 2^-10 Å)
            v = (xr + s1 / n) / 1024.0
            c.append(v - box[ax] * np.floor(v / box[ax] + 0.5))
        gxx = (n * d["s2xx"] - d["s1x"] ** 2) / (n * n) / q
        gyy = (n * d["s2yy"] - d["s1y"] ** 2) / (n * n) / q
        gxy = (n * d["s2xy"] - d["s1x"] * d["s1y"]) / (n * n) / q
        half, det = 0.5 * (gxx + gyy), np.hypot(0.5 * (gxx - gyy), gxy)
        l1, l2 = half + det, max(half - det, 0.0)
        out["centre"].append(tuple(c))
        out["rg"].append(np.sqrt(gxx + gyy))
        out["lam1"].append(l1)
        out["lam2"].append(l2)
        out["asphericity"].append(((l1 - l2) / (l1 + l2)) ** 2 if l1 + l2 > 0 else 0.0)
    return {k: np.array(v, dtype=np.int64 if k in ("label", "size", "span") else np.float64) for k, v in out.items()}


def reduce_geom(table, device=None, group=None) -> np.ndarray:
    """SUM all-reduce of kmc_cluster_geometry tables over the ranks of an
    ensemble.  count and sum_size go as they are; the 128-bit sum of m goes as
    int64 columns that cannot overflow — the two 32-bit halves of its low word
    and the high word — summed by reduce_counts and put together again as
    Python integers on the host.  Without an initialised process group the
    table comes back unchanged."""
    table = np.ascontiguousarray(table, dtype=capi.GEOM_BIN_DTYPE)
    lo = table["sum_m_lo"].astype(np.uint64)
    cols = np.stack([table["count"], table["sum_size"], (lo & np.uint64(0xFFFFFFFF)).astype(np.int64),
                     (lo >> np.uint64(32)).astype(np.int64), table["sum_m_hi"]])
    cols = reduce_counts(cols, device=device, group=group)
    out = np.zeros(len(table), dtype=table.dtype)
    out["count"], out["sum_size"] = cols[0], cols[1]
    for k in range(len(table)):
        m = ((int(cols[4][k]) << 64) + (int(cols[3][k]) << 32) + int(cols[2][k])) & ((1 << 128) - 1)
        out["sum_m_lo"][k] = m & 0xFFFFFFFFFFFFFFFF
        hi = m >> 64
        out["sum_m_hi"][k] = hi - (1 << 64) if hi >> 63 else hi
    return out


# ---------------------------------------------------------------- structure factor
def structure_factor(sums, n_sel) -> dict:
    """The partial structure factors from kmc_structure_factor's integer sums
    (sums[4, ...]: C_A, S_A, C_B, S_B; n_sel = the receptors and ligands summed
    over).  With rho = (C + iS) / 2^30, float64 arrays of the sums' grid:
      AA = |rho_A|^2 / N_A,  BB = |rho_B|^2 / N_B,
      AB = Re(rho_A conj rho_B) / sqrt(N_A N_B),  NN = |rho_A + rho_B|^2 / (N_A + N_B).
    A partial whose species is empty is all zeros.

    Replicas: S(q) of an ensemble is the float64 mean of the per-replica values
    — sum them with reduce_sums and divide by the number of replicas.  The
    integer sums of different replicas must NOT be added: they are amplitudes
    of unrelated configurations, and their sum's square is not a sum of squares."""
    sums = np.asarray(sums)
    if sums.shape[0] != 4:
        raise ValueError("structure_factor: sums is [4, ...] (C_A, S_A, C_B, S_B)")
    ca, sa, cb, sb = (sums[i].astype(np.float64) / float(1 << 30) for i in range(4))
    n_a, n_b = float(n_sel[0]), float(n_sel[1])
    zero = np.zeros_like(ca)
    return {
        "AA": (ca * ca + sa * sa) / n_a if n_a > 0 else zero.copy(),
        "BB": (cb * cb + sb * sb) / n_b if n_b > 0 else zero.copy(),
        "AB": (ca * cb + sa * sb) / np.sqrt(n_a * n_b) if n_a > 0 and n_b > 0 else zero.copy(),
        "NN": ((ca + cb) ** 2 + (sa + sb) ** 2) / (n_a + n_b) if n_a + n_b > 0 else zero.copy(),
    }


def sq_radial(S, box_x: float, box_y: float, nbins: int, q_max: float):
    """Radial average of one partial S[hmax + 1, 2 kmax + 1] (structure_factor's
    grid: h = 0..hmax, k = -kmax..kmax) over |q|, q = 2 pi (h / box_x, k / box_y).

    Bin b covers [b dq, (b + 1) dq), dq = q_max / nbins.  Every independent wave
    vector counts once: q = 0 is left out; of the h = 0 row only k > 0 is used
    (k < 0 are its Friedel copies, S(-q) = S(q)); every h > 0 vector is used.
    Returns (bin centres, the mean S per bin — NaN where a bin is empty —, the
    number of wave vectors per bin)."""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim != 2 or S.shape[1] % 2 != 1 or nbins < 1 or not q_max > 0:
        raise ValueError("sq_radial: S is [hmax + 1, 2 kmax + 1], nbins >= 1, q_max > 0")
    kmax = S.shape[1] // 2
    h = np.arange(S.shape[0], dtype=np.float64)[:, None]
    k = np.arange(-kmax, kmax + 1, dtype=np.float64)[None, :]
    q = 2.0 * np.pi * np.sqrt((h / box_x) ** 2 + (k / box_y) ** 2)
    use = (h > 0) | (k > 0)
    dq = q_max / nbins
    b = np.floor(q / dq).astype(np.int64)
    use &= b < nbins
    count = np.bincount(b[use], minlength=nbins).astype(np.int64)
    total = np.bincount(b[use], weights=S[use], minlength=nbins)
    mean = np.divide(total, count, out=np.full(nbins, np.nan), where=count > 0)
    return (np.arange(nbins, dtype=np.float64) + 0.5) * dq, mean, count


# ---------------------------------------------------------------- bond-orientational order
def bond_order(summary) -> dict:
    """The global numbers from kmc_bond_order's summary (a capi.BondOrderOut or
    its as_dict()), float64:
      psi_abs  = |sum_i psi_i| / n_with — the global |Psi_n|: the modulus of the
                 mean local order over the proteins that have a neighbour,
      psi2     = sum_i |psi_i|^2 / n_with — the mean local |psi|^2,
      mean_nn  = sum_nn / n_sel — the mean neighbour count of the selected set,
    with psi_i = (pc_i + i ps_i) / 2^15 (zeros when the denominators are zero).

    Replicas: the summary's fields, the histogram hist[16, nbins] and corr are
    plain integer sums over proteins or pairs, so those of several replicas are
    additive — sum them with reduce_counts and post-process the totals."""
    d = summary.as_dict() if hasattr(summary, "as_dict") else dict(summary)
    n_with, n_sel = float(d["n_with"]), float(d["n_sel"])
    u = 32768.0
    re, im = float(d["sum_pc"]) / u, float(d["sum_ps"]) / u
    return {
        "psi_abs": float(np.hypot(re, im) / n_with) if n_with > 0 else 0.0,
        "psi2": float(d["sum_m"]) / (u * u) / n_with if n_with > 0 else 0.0,
        "mean_nn": float(d["sum_nn"]) / n_sel if n_sel > 0 else 0.0,
    }


def bond_order_corr(corr, r_max: float):
    """(r, G_n) from kmc_bond_order_corr's corr[2, nbins]: r the bin centres
    (k + 1/2) r_max / nbins, G_n(r_k) = corr[0, k] / corr[1, k] / 2^30 — the
    real part of <psi_n(i) psi_n*(j)> at separation r —, NaN where a bin holds
    no pair.  corr is additive over replicas (reduce_counts) before this call."""
    corr = np.asarray(corr)
    if corr.ndim != 2 or corr.shape[0] != 2 or not r_max > 0:
        raise ValueError("bond_order_corr: corr is [2, nbins], r_max > 0")
    nbins = corr.shape[1]
    num, cnt = corr[0].astype(np.float64), corr[1].astype(np.float64)
    g = np.divide(num, cnt, out=np.full(nbins, np.nan), where=cnt > 0) / float(1 << 30)
    return (np.arange(nbins, dtype=np.float64) + 0.5) * (r_max / nbins), g


# ---------------------------------------------------------------- bond kinetics
def kin_bin_edges() -> np.ndarray:
    """The lower edges (int64, in steps) of the KIN_BINS bins of every lifetime and
    waiting time of the kinetics histogram: b below 16; else (8 + m) << (e - 3)
    with e = 4 + (b - 16) // 8, m = (b - 16) % 8 — eight bins per octave.  The
    last bin is open: it also takes every value from 2^34 on."""
    b = np.arange(capi.KIN_BINS, dtype=np.int64)
    e, m = 4 + (b - 16) // 8, (b - 16) % 8
    return np.where(b < 16, b, (8 + m) << np.maximum(e - 3, 0))


def kinetics_rates(out, time_step: float, hist=None) -> dict:
    """The effective rates from a kin_sample / kin_update result (a capi.KinOut
    or its as_dict()), float64, zeros where a denominator is zero:
      rl_off, cis_off_mono, cis_off_cx   events per bond-step: rl_off / exp_rl,
                                         cis_off_mono / exp_mono, cis_off_cx / exp_cx,
      rl_on                              per free receptor-step: rl_on / exp_free_receptor,
      *_per_ns                           the same four divided by time_step (ns),
    and with hist (kin_sample's histogram) rebinding_fraction: of the receptors
    that bound again after a loss, the share that took the same ligand back,
    row 5 / (row 5 + row 6).  The inputs are additive over replicas
    (reduce_counts) before this call."""
    d = out.as_dict() if hasattr(out, "as_dict") else dict(out)

    def ratio(num, den):
        return float(num) / float(den) if den else 0.0

    r = {
        "rl_off": ratio(d["rl_off"], d["exp_rl"]),
        "cis_off_mono": ratio(d["cis_off_mono"], d["exp_mono"]),
        "cis_off_cx": ratio(d["cis_off_cx"], d["exp_cx"]),
        "rl_on": ratio(d["rl_on"], d["exp_free_receptor"]),
    }
    for k in list(r):
        r[k + "_per_ns"] = r[k] / float(time_step) if time_step else 0.0
    if hist is not None:
        h = np.asarray(hist)
        same, other = int(h[5].sum()), int(h[6].sum())
        r["rebinding_fraction"] = ratio(same, same + other)
    return r


def lifetime_survival(ended_row, alive_row):
    """Kaplan–Meier survival of bond lifetimes over the kinetics bins: ended_row
    the lifetimes of the bonds that ended (rows 0, 2 or 3 of the histogram),
    alive_row the ages of those still alive (rows 7 or 8: right-censored).
    With d_b the ended and n_b the ended plus alive entries in bins >= b,
      S_b = prod_{b' <= b} (1 - d_b' / n_b')
    (a bin nobody reached contributes the factor 1).  Returns (the bins' lower
    edges, S): S_b estimates the share of bonds that outlive bin b."""
    d = np.asarray(ended_row, dtype=np.float64)
    a = np.asarray(alive_row, dtype=np.float64)
    if d.shape != a.shape or d.ndim != 1:
        raise ValueError("lifetime_survival: two rows of one length")
    at_risk = np.cumsum((d + a)[::-1])[::-1]
    factor = 1.0 - np.divide(d, at_risk, out=np.zeros_like(d), where=at_risk > 0)
    edges = kin_bin_edges() if d.size == capi.KIN_BINS else np.arange(d.size, dtype=np.int64)
    return edges, np.cumprod(factor)


# ---------------------------------------------------------------- encounter statistics
def _ratio(num, den) -> float:
    return float(num) / float(den) if den else 0.0


def reach_factors(out, hist_d, cutoffs) -> dict:
    """From a reach_census (capi.ReachOut or its as_dict(), hist_d[3, 2, nd]) and cutoffs = (bond_dist_cutoff,
    cis_dist_cutoff), per channel (RL, MONO, CX):
      orientation_factor [3]   n_reactive / n_reach: the share of in-reach pairs whose orientation gates are open,
      r [3, nd]                the centres of the distance bins (the channel's cutoff / nd wide),
      profile [3, nd]          the in-reach pairs per distance bin (reactive or not),
      reactive_share [3, nd]   the reactive share of each bin.
    Zeros where a denominator is zero.  Sum the counts of replicas (reduce_counts) before this call."""
    d = out.as_dict() if hasattr(out, "as_dict") else dict(out)
    h = np.asarray(hist_d, dtype=np.float64)
    nd = h.shape[2]
    cut = np.array([cutoffs[0], cutoffs[1], cutoffs[1]], dtype=np.float64)
    profile = h.sum(axis=1)
    return {
        "orientation_factor": np.array([_ratio(a, b) for a, b in zip(d["n_reactive"], d["n_reach"])]),
        "r": (np.arange(nd, dtype=np.float64) + 0.5)[None, :] * (cut / nd)[:, None],
        "profile": profile,
        "reactive_share": np.divide(h[:, 1], profile, out=np.zeros_like(profile), where=profile > 0),
    }


def encounter_rates(out, time_step: float, ass_rate=None) -> dict:
    """From an enc_sample / enc_update result (capi.EncOut, capi.EncSample or a dict), float64, zeros where a
    denominator is zero:
      encounter_rate         encounters opened per free receptor-step, n_opened / exp_free_receptor,
      encounter_rate_per_ns  the same divided by time_step (ns),
      mean_dwell             steps in reach per encounter, exp_reach / n_opened,
      capture_probability    bonds per encounter, on_from_encounter / n_opened,
      on_per_reactive_step   on_from_encounter / exp_reactive — beside model_probability = ass_rate * time_step
                             (with ass_rate), the draw an open gate wins per step,
      direct_share           on_direct / (on_from_encounter + on_direct): the bonds no look saw coming (the pair
                             met and bound between two updates).
    Whether the on-rate is limited by diffusion (few encounters, each captured) or by reaction (many encounters,
    few captures) reads off encounter_rate and capture_probability."""
    d = out.as_dict() if hasattr(out, "as_dict") else dict(out)
    r = {
        "encounter_rate": _ratio(d["n_opened"], d["exp_free_receptor"]),
        "mean_dwell": _ratio(d["exp_reach"], d["n_opened"]),
        "capture_probability": _ratio(d["on_from_encounter"], d["n_opened"]),
        "on_per_reactive_step": _ratio(d["on_from_encounter"], d["exp_reactive"]),
        "direct_share": _ratio(d["on_direct"], d["on_from_encounter"] + d["on_direct"]),
    }
    r["encounter_rate_per_ns"] = r["encounter_rate"] / float(time_step) if time_step else 0.0
    if ass_rate is not None:
        r["model_probability"] = float(ass_rate) * float(time_step)
    return r


def escape_probability(hist) -> dict:
    """From an enc_sample's hist[ENC_HISTS, ENC_BINS]: of the geminate encounters (a bond ended and the pair was
    still in reach) that have ended,
      escape_probability     GEM_ESCAPED / (GEM_REBOUND + GEM_ESCAPED + GEM_LOST): the factor between the
                             microscopic diss_rate and the observed off-rate,
      rebinding_probability  GEM_REBOUND over the same,
      edges, survival        the share of them still open after the durations of each bin (lower edges in steps)."""
    h = np.asarray(hist)
    reb, esc, lost = int(h[5].sum()), int(h[6].sum()), int(h[7].sum())
    n = reb + esc + lost
    ended = (h[5] + h[6] + h[7]).astype(np.float64)
    return {
        "escape_probability": _ratio(esc, n),
        "rebinding_probability": _ratio(reb, n),
        "edges": kin_bin_edges() if ended.size == capi.KIN_BINS else np.arange(ended.size, dtype=np.int64),
        "survival": 1.0 - np.cumsum(ended) / n if n else np.ones_like(ended),
    }


# ---------------------------------------------------------------- cluster growth kinetics
def _cf_expo2(expo2) -> list:
    """expo2 as rows of Python ints: from capi.I128_DTYPE records (the two words), or ints already."""
    a = np.asarray(expo2) if not isinstance(expo2, list) else None
    if a is not None and a.dtype.names:
        return [[(int(w["hi"]) << 64) + int(w["lo"]) for w in row] for row in a]
    return [[int(x) for x in row] for row in expo2]


def coag_kernel(merge, expo2) -> np.ndarray:
    """The coagulation kernel K[a][b] = merge[a][b] / expo2[a][b] from a cf_sample's tables: binary mergers of
    a cluster of size a with one of size b per pair of such clusters and step, float64 [S+1, S+1], symmetric;
    nan where no such pair was ever exposed.  expo2 is capi.CfTables.expo2 (the 128-bit words, divided as
    Python ints and rounded once) or rows of ints.  The last index stands for every size from S on.  Sum the
    tables of replicas (reduce_counts for merge, Python ints for expo2) before this call."""
    m = np.asarray(merge)
    e = _cf_expo2(expo2)
    s1 = m.shape[0]
    k = np.full((s1, s1), np.nan)
    for a in range(1, s1):
        for b in range(a, s1):
            if e[a][b] > 0:
                k[a, b] = k[b, a] = int(m[a, b]) / e[a][b]
    return k


def frag_kernel(frag, expo) -> np.ndarray:
    """The fragmentation kernel F[a][b] = frag[a][b] / expo[a + b] for a + b < S: binary fragmentations of a
    cluster of size a + b into sizes a and b per such cluster and step, float64 [S+1, S+1], symmetric; nan
    where a + b >= S (the parent's size is not resolved) or no such cluster was ever exposed."""
    f, x = np.asarray(frag), np.asarray(expo)
    s1 = f.shape[0]
    k = np.full((s1, s1), np.nan)
    for a in range(1, s1):
        for b in range(a, s1):
            if a + b < s1 - 1 and x[a + b] > 0:
                k[a, b] = k[b, a] = int(f[a, b]) / int(x[a + b])
    return k


def growth_modes(out, merge_kind) -> dict:
    """How the clusters grew, from a cf_sample's counters (a capi.CfOut or its as_dict()) and merge_kind: of
    the binary mergers the shares in which one side was a single receptor (receptor_addition), a single
    ligand (ligand_addition; a receptor meeting a ligand counts as the receptor's addition), and in which
    both sides were clusters of two or more (cluster_cluster); binary_mergers, their number; and the cycle
    counts cycles_closed / cycles_opened with ring_fraction = cycles_closed / bonds formed.  Zeros where a
    denominator is zero."""
    d = out.as_dict() if hasattr(out, "as_dict") else dict(out)
    k = np.asarray(merge_kind, dtype=np.int64)
    total = int(np.triu(k).sum())
    rec = int(k[0, :].sum())
    lig = int(k[1, 1:].sum())
    formed = d["formed_rl"] + d["formed_cis"]

    def ratio(num, den):
        return float(num) / float(den) if den else 0.0

    return dict(binary_mergers=total, receptor_addition=ratio(rec, total), ligand_addition=ratio(lig, total),
                cluster_cluster=ratio(total - rec - lig, total), cycles_closed=d["cycles_closed"],
                cycles_opened=d["cycles_opened"], ring_fraction=ratio(d["cycles_closed"], formed))


def ring_stats(counts, net) -> dict:
    """The ring statistics of the ligand network from kmc_rings' counts[2, RING_MAX + 1] (all, chordless) and the
    network's counters (a capi.NetOut, its as_dict(), or any mapping with n_vertices and cycle_rank):
    hexagon_fraction = 2 chordless[6] / n_vertices, the share of the network ligands' ring positions that hexagons
    fill (a ligand of the honeycomb lies on three hexagons of six ligands each: 1 for the perfect lattice);
    rings_per_vertex = sum of the chordless rings / n_vertices; mean_ring_length, of the chordless rings;
    rings_per_cycle = sum of the chordless rings / cycle_rank (1 when the chordless rings are a basis of the
    network's cycles).  Zeros where a denominator is zero.  Sum counts and the counters over replicas
    (reduce_counts) before the call: every input is additive."""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 2 or c.shape[0] != 2 or c.shape[1] != capi.RING_MAX + 1:
        raise ValueError("ring_stats: counts is [2, RING_MAX + 1]")
    d = net.as_dict() if hasattr(net, "as_dict") else dict(net)
    nv, rank = int(d["n_vertices"]), int(d["cycle_rank"])
    chordless = c[1]
    total = int(chordless.sum())
    lengths = int((chordless * np.arange(capi.RING_MAX + 1, dtype=np.int64)).sum())

    def ratio(num, den):
        return float(num) / float(den) if den else 0.0

    return dict(hexagon_fraction=ratio(2 * int(chordless[6]), nv), rings_per_vertex=ratio(total, nv),
                mean_ring_length=ratio(lengths, total), rings_per_cycle=ratio(total, rank))


def lag_curves(sample, time_step: float) -> dict:
    """MSD, alpha_2 and F_s by lag time from a lag_sample (a capi.LagSample; sum samples over replicas or windows
    first: reduce_counts on counts(), then from_counts).  Per row r and class c, over the clean pairs:
      tau[r]        = lag[r] * every * time_step,
      msd[r, c]     = m2_clean / (2^20 n_clean)                          (A^2),
      alpha2[r, c]  = <q^2> / (2 <q>^2) - 1 = m4_clean n_clean / (2 m2_clean^2) - 1   (the two-dimensional form),
      fs[r, c, k]   = fs / (2 * 2^30 * n_clean): the mean of cos(q_k dx) and cos(q_k dy), q[k] = (2 pi h_k / box_x,
                      2 pi h_k / box_y) with the box as the recorder saw it (BX, BY / 1024),
      clean_fraction[r, c] = n_clean / (n_all + n_far), of every pair filed,
      msd_all[r, c] = m2_all / (2^20 n_all), the pairs with events included,
    and n_clean, n_pairs as float arrays.  Zeros where a denominator is zero.  The integer sums are divided whole
    (Python ints), so no sum is rounded before its quotient is."""
    s = sample
    rows, nq = s.rows, s.nq
    shape = (rows, capi.LAG_CLASSES)
    out = dict(tau=np.asarray(s.lags, dtype=np.float64) * float(s.every) * float(time_step),
               msd=np.zeros(shape), msd_all=np.zeros(shape), alpha2=np.zeros(shape), fs=np.zeros(shape + (nq,)),
               clean_fraction=np.zeros(shape), n_clean=np.zeros(shape),
               n_pairs=np.array([float(x) for x in s.n_pairs]),
               q=np.array([[2.0 * np.pi * h * 1024.0 / s.BX, 2.0 * np.pi * h * 1024.0 / s.BY] for h in s.h]).reshape(nq, 2))
    for r in range(rows):
        for c in range(capi.LAG_CLASSES):
            n, na, nf = int(s.n_clean[r, c]), int(s.n_all[r, c]), int(s.n_far[r, c])
            m2, m4 = int(s.m2_clean[r, c]), int(s.m4_clean[r, c])
            out["n_clean"][r, c] = n
            if na:
                out["msd_all"][r, c] = int(s.m2_all[r, c]) / (na << 20)
            if na + nf:
                out["clean_fraction"][r, c] = n / (na + nf)
            if n:
                out["msd"][r, c] = m2 / (n << 20)
                for k in range(nq):
                    out["fs"][r, c, k] = int(s.fs[r, c, k]) / (n << 31)
            if m2:
                out["alpha2"][r, c] = (m4 * n) / (2 * m2 * m2) - 1.0
    return out


def rot_lengths(p) -> np.ndarray:
    """|u|^2 [5, 2] in quanta^2 (2^-20 A^2) per class and vector from the nominal lengths of the parameters: R_A for a
    heading, R_B for a ligand's axis, 2 R_B / sqrt 3 for its arm; 0 for v = 1 of a receptor class."""
    ra2 = (float(p.ra_radius) * 1024.0) ** 2
    rb2 = (float(p.rb_radius) * 1024.0) ** 2
    return np.array([[ra2, 0.0]] * 3 + [[rb2, 4.0 * rb2 / 3.0]] * 2)


def rot_curves(sample, p) -> dict:
    """C_1 and C_2 by lag time from a rot_sample (a capi.RotSample; sum samples over replicas or windows first:
    reduce_counts on counts(), then from_counts); p: the parameters (time_step, ra_radius, rb_radius).  Per row r,
    class c and vector v (0: heading / axis, 1: arm), over the clean pairs, with d = u(t) . u(0):
      tau[r]          = lag[r] * every * time_step,
      c1[r, c, v]     = s1_clean / (n_clean |u|^2)                         = <cos>,
      c2[r, c, v]     = 2 s2_clean / (n_clean |u|^4) - 1 for a heading (c < 3; two dimensions: <cos 2 phi>),
                        (3 s2_clean / (n_clean |u|^4) - 1) / 2 for a ligand's vectors (<P_2(cos)>),
      c1_all[r, c, v] = s1_all / (n_all |u|^2), the pairs with events (link changes, reflections) included,
      clean_fraction[r, c, v] = n_clean / n_all,
    and n_clean, n_pairs as float arrays.  Zeros where a denominator is zero.  |u| is the NOMINAL length (rot_lengths),
    not the quantised one: each component of a vector is the difference of two coordinates rounded to 2^-10 A, off by
    at most 2^-10 A, so d is off by at most 2 sqrt(3) 2^-10 |u| + 3 2^-20 A^2 and c1 of a pair at rest reads 1 within
    2 sqrt(3) 2^-10 / |u| + 3 2^-20 / |u|^2 (2e-4 at R_A = 20 A).  The integer sums are divided whole (Python ints
    to float once)."""
    s = sample
    shape = (s.rows, capi.LAG_CLASSES, capi.ROT_VECS)
    u2 = rot_lengths(p)
    out = dict(tau=np.asarray(s.lags, dtype=np.float64) * float(s.every) * float(p.time_step),
               c1=np.zeros(shape), c2=np.zeros(shape), c1_all=np.zeros(shape), clean_fraction=np.zeros(shape),
               n_clean=np.zeros(shape), n_pairs=np.array([float(x) for x in s.n_pairs]))
    for r, c, v in np.ndindex(*shape):
        n, na, L2 = int(s.n_clean[r, c, v]), int(s.n_all[r, c, v]), float(u2[c, v])
        out["n_clean"][r, c, v] = n
        if L2 == 0.0:
            continue
        if na:
            out["c1_all"][r, c, v] = int(s.s1_all[r, c, v]) / (na * L2)
            out["clean_fraction"][r, c, v] = n / na
        if n:
            out["c1"][r, c, v] = int(s.s1_clean[r, c, v]) / (n * L2)
            m = int(s.s2_clean[r, c, v]) / (n * L2 * L2)
            out["c2"][r, c, v] = 2.0 * m - 1.0 if c < 3 else (3.0 * m - 1.0) / 2.0
    return out


def pose_profile(hist, p) -> dict:
    """The ligands' pose census (Simulation.ligand_pose's hist [4, nz, nc]) normalised: z[nz] the centres of the
    height bins of bead [1][1] in A over [0, box_z], cos[nc] the centres of the tilt bins as N_z / R_B over [-1, 1]
    (the integers N_z = -Lq .. Lq taken as unit cells around themselves, bin k covers (k .. k + 1) (2 Lq + 1) / nc - Lq
    - 1/2 quanta, Lq = round(1024 R_B): the bins are symmetric about 0), n[4] the ligands per number of
    occupied sites, pdf[4, nz, nc] = hist / n (zeros where n is zero), and its marginals pdf_z[4, nz], pdf_cos[4, nc]."""
    h = np.asarray(hist, dtype=np.float64)
    _, nz, nc = h.shape
    lq = float(np.floor(float(p.rb_radius) * 1024.0 + 0.5))
    edges = np.arange(nc + 1) * (2.0 * lq + 1.0) / nc - lq - 0.5
    n = h.sum(axis=(1, 2))
    pdf = np.divide(h, n[:, None, None], out=np.zeros_like(h), where=n[:, None, None] > 0)
    return dict(z=(np.arange(nz) + 0.5) * float(p.box_z) / nz, cos=0.5 * (edges[:-1] + edges[1:]) / lq, n=n, pdf=pdf,
                pdf_z=pdf.sum(axis=2), pdf_cos=pdf.sum(axis=1))


def van_hove_distinct(sample, p):
    """(r[nbins], gd[4, nbins], gs[2, nbins]) from a capi.PdSample: r the bin centres in A; gd the distinct part of the
    van Hove function G_d(r, t) per ordered kind 2 species(i) + species(j), normalised like rdf — the count over the
    ordered pairs n_i (n_j - [same species]) times the exact annulus area over the box area, the ideal density of the
    j species — so that G_d(r, 0) is g(r); gs the (folded) self part as the fraction of the species' proteins per
    bin.  Zeros where there is no pair."""
    nb = sample.nbins
    edges = np.arange(nb + 1, dtype=np.float64) * (sample.r_max / nb)
    area = np.pi * (edges[1:] ** 2 - edges[:-1] ** 2)
    n = (float(p.n_a), float(p.n_b))
    gd = np.zeros((4, nb))
    for si in range(2):
        for sj in range(2):
            ideal = n[si] * (n[sj] - (si == sj)) * area / (float(p.box_x) * float(p.box_y))
            c = np.array([int(x) for x in sample.gd[2 * si + sj]], dtype=np.float64)
            gd[2 * si + sj] = np.divide(c, ideal, out=np.zeros(nb), where=ideal > 0)
    gs = np.zeros((2, nb))
    for s in range(2):
        if n[s] > 0:
            gs[s] = np.array([int(x) for x in sample.gs[s]], dtype=np.float64) / n[s]
    return 0.5 * (edges[:-1] + edges[1:]), gd, gs


def displacement_corr(sample):
    """(r[nbins], cu[3, nbins], valid[3, nbins]) from a capi.PdSample: C_u = 2 dot / sq per kind (AA, AB, BB), which is
    1 for rigid co-translation, by the pair distance at the origin, and the valid fraction n_valid / n_pairs; zeros
    where a denominator is zero."""
    nb = sample.nbins
    edges = np.arange(nb + 1, dtype=np.float64) * (sample.r_max / nb)
    cu, valid = np.zeros((3, nb)), np.zeros((3, nb))
    for kind in range(3):
        for k in range(nb):
            sq, n = int(sample.sq[kind, k]), int(sample.n_pairs[kind, k])
            if sq:
                cu[kind, k] = 2 * int(sample.dot[kind, k]) / sq
            if n:
                valid[kind, k] = int(sample.n_valid[kind, k]) / n
    return 0.5 * (edges[:-1] + edges[1:]), cu, valid


def _bd_rows_ok(sample):
    """[2, max_size + 1] bool: the rows that hold one size only — every row but the overflow row, and that one too
    when all its bodies have max_size members."""
    ok = np.ones((2, sample.max_size + 1), dtype=bool)
    ok[:, 0] = False
    for hl in range(2):
        ok[hl, -1] = int(sample.sum_size[hl, -1]) == int(sample.n_bodies[hl, -1]) * sample.max_size
    return ok


def body_msd(sample):
    """(msd[2, max_size + 1], n_valid[2, max_size + 1]) from a capi.BdSample: the mean squared displacement of the
    centre of mass in A^2 by (holds a ligand, size) over the VALID bodies, m2 / n_valid / size^2 / 2^20; NaN where no
    body is valid and in an overflow row that mixes sizes."""
    ms = sample.max_size
    msd = np.full((2, ms + 1), np.nan)
    n_valid = np.zeros((2, ms + 1), dtype=np.int64)
    ok = _bd_rows_ok(sample)
    for hl in range(2):
        for k in range(1, ms + 1):
            nv = int(sample.n_valid[hl, k])
            n_valid[hl, k] = nv
            if nv and ok[hl, k]:
                msd[hl, k] = int(sample.m2[hl, k]) / nv / (k * k) / 2.0 ** 20
    return msd, n_valid


def body_diffusion(samples_with_lags, time_step):
    """D(s) from capi.BdSamples of one configuration at several lags: samples_with_lags is an iterable of (lag in
    steps, sample), time_step the time of one step.  Per (holds a ligand, size) the least-squares line through the
    origin MSD = 4 D t over the lags that have valid bodies, D in A^2 per time unit (NaN without any), and per hl the
    exponent gamma of D ~ s^-gamma, the slope of log D against log s over the sizes with D > 0 (NaN below two of
    them).  Returns dict(size, D[2, max_size + 1], n_lags, gamma[2])."""
    pairs = [(float(lag) * float(time_step), body_msd(s)[0]) for lag, s in samples_with_lags]
    if not pairs:
        raise ValueError("body_diffusion: no sample")
    shape = pairs[0][1].shape
    num, den, cnt = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64)
    for t, msd in pairs:
        if msd.shape != shape:
            raise ValueError("body_diffusion: samples of different max_size")
        have = np.isfinite(msd) & (t > 0)
        num[have] += t * msd[have]
        den[have] += t * t
        cnt[have] += 1
    D = np.divide(num, 4.0 * den, out=np.full(shape, np.nan), where=den > 0)
    size = np.arange(shape[1])
    gamma = np.full(2, np.nan)
    for hl in range(2):
        use = np.isfinite(D[hl]) & (D[hl] > 0) & (size >= 1)
        if use.sum() >= 2:
            gamma[hl] = -np.polyfit(np.log(size[use]), np.log(D[hl][use]), 1)[0]
    return dict(size=size, D=D, n_lags=cnt, gamma=gamma)


def body_rotation(sample):
    """dict(c1, c2, phi2, n_rot)[2, max_size + 1] from a capi.BdSample: the rotational correlators C_1 = <cos phi>
    and C_2 = <cos 2 phi> and the mean squared angle <phi^2> in rad^2 (phi wrapped to (-pi, pi]) over the bodies
    with a rotation, by (holds a ligand, size); NaN where there is none and in an overflow row that mixes sizes."""
    ms = sample.max_size
    out = dict(c1=np.full((2, ms + 1), np.nan), c2=np.full((2, ms + 1), np.nan), phi2=np.full((2, ms + 1), np.nan),
               n_rot=np.zeros((2, ms + 1), dtype=np.int64))
    ok = _bd_rows_ok(sample)
    for hl in range(2):
        for k in range(1, ms + 1):
            n = int(sample.n_rot[hl, k])
            out["n_rot"][hl, k] = n
            if n and ok[hl, k]:
                out["c1"][hl, k] = int(sample.c1[hl, k]) / n / 2.0 ** 30
                out["c2"][hl, k] = int(sample.c2[hl, k]) / n / 2.0 ** 30
                out["phi2"][hl, k] = int(sample.phi2[hl, k]) / n / 2.0 ** 48
    return out


def body_survival(sample):
    """dict(pristine, intact, grown, broken, n_bodies)[2, max_size + 1] from a capi.BdSample: the fractions of the
    origin's bodies by (holds a ligand, size) that are untouched, that have the same members, that are together in a
    larger cluster, and that have fallen apart; intact + grown + broken = 1; NaN where there is no body."""
    ms = sample.max_size
    n = np.array([[int(x) for x in row] for row in sample.n_bodies], dtype=np.float64)
    out = dict(n_bodies=n.astype(np.int64))
    for name in ("pristine", "intact", "grown", "broken"):
        c = np.array([[int(x) for x in row] for row in getattr(sample, "n_" + name)], dtype=np.float64)
        out[name] = np.divide(c, n, out=np.full((2, ms + 1), np.nan), where=n > 0)
    return out


def prox_summary(out, size_hist) -> dict:
    """The ratios of one prox_clusters result (a capi.ProxOut or its as_dict(), size_hist[max_size + 1]):
    clustered = (cores + borders) / selected; mean_size (number-weighted) and mean_size_w (member-weighted:
    sum s^2 n_s / sum s n_s) over the bins below the clamp bin, which mixes sizes; recovery = n_whole /
    n_bond_multi, the bonded oligomers recovered exactly; over_merge = 1 - n_pure / n_multi, the clusters that mix
    oligomers; over_split = 1 - n_bond_kept / n_bond_multi, the oligomers not kept in one cluster.  A zero
    denominator gives nan."""
    d = out if isinstance(out, dict) else out.as_dict()
    h = np.asarray(size_hist, dtype=np.float64)
    s = np.arange(h.size - 1, dtype=np.float64)
    body = h[:-1]

    def ratio(a, b):
        return float(a) / float(b) if b else float("nan")

    return dict(clustered=ratio(d["n_core"] + d["n_border"], d["n_sel"]),
                mean_size=ratio(np.dot(s, body), body.sum()),
                mean_size_w=ratio(np.dot(s * s, body), np.dot(s, body)),
                recovery=ratio(d["n_whole"], d["n_bond_multi"]),
                over_merge=1.0 - ratio(d["n_pure"], d["n_multi"]),
                over_split=1.0 - ratio(d["n_bond_kept"], d["n_bond_multi"]))


def nn_distance(nnd_hist, eps: float, out):
    """(r, pdf, cdf, alone) from prox_clusters' nnd_hist[nbins]: r the bin centres (bin k covers [k dr, (k + 1) dr),
    dr = eps / nbins, the last bin closed at eps), pdf the density of the nearest-neighbour distance among the
    points that have a neighbour within eps (it integrates to 1; zeros when there is none), cdf its integral at the
    upper bin edges, alone = n_alone / n_sel, the points without one (nan for an empty set)."""
    h = np.asarray(nnd_hist, dtype=np.float64)
    d = out if isinstance(out, dict) else out.as_dict()
    if h.ndim != 1 or h.size < 1 or not eps > 0:
        raise ValueError("nn_distance: nnd_hist is [nbins], eps > 0")
    dr = eps / h.size
    r = (np.arange(h.size, dtype=np.float64) + 0.5) * dr
    tot = h.sum()
    pdf = h / (tot * dr) if tot > 0 else np.zeros_like(h)
    cdf = np.cumsum(h) / tot if tot > 0 else np.zeros_like(h)
    alone = d["n_alone"] / d["n_sel"] if d["n_sel"] else float("nan")
    return r, pdf, cdf, alone


def ripley(counts, which, p, r_max: float):
    """(r, K, L, H) from kmc_pair_counts' histogram: Ripley's K(r) = area / pairs * #{ordered pairs closer than r} at
    the upper bin edges r, with area = box_x * box_y, the unordered AA / BB counts doubled over pairs = n (n - 1),
    the AB counts over n_a n_b; L = sqrt(K / pi) and H = L - r (0 for an ideal gas, > 0 where points cluster).
    Pure post-processing of the integers; nan without a pair."""
    c = np.asarray(counts, dtype=np.float64)
    which = capi.PAIRS[which] if isinstance(which, str) else int(which)
    if c.ndim != 1 or c.size < 1 or not r_max > 0:
        raise ValueError("ripley: counts is [nbins], r_max > 0")
    if which == capi.PAIR_AB:
        ordered, pairs = np.cumsum(c), float(p.n_a) * float(p.n_b)
    else:
        n = p.n_a if which == capi.PAIR_AA else p.n_b
        ordered, pairs = 2.0 * np.cumsum(c), float(n) * float(n - 1)
    r = np.arange(1, c.size + 1, dtype=np.float64) * (r_max / c.size)
    K = p.box_x * p.box_y * ordered / pairs if pairs > 0 else np.full_like(c, np.nan)
    L = np.sqrt(K / np.pi)
    return r, K, L, L - r
