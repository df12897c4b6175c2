"""Post-processing of the on-device structure analysis (engine.Simulation.census /
pair_counts) and displacement tracking (track_sample): g(r) from the lateral
pair counts, per-class mean-squared displacements and the diffusion fit, and
the replica sums of integer histograms and float64 sums.

The counts and sums themselves come from libkmc (kmc_analysis.hip,
kmc_dynamics.hip); nothing here touches a trajectory.
"""
from __future__ import annotations

import numpy as np


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
