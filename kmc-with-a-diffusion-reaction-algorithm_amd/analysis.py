"""Post-processing of the on-device structure analysis (engine.Simulation.census /
pair_counts): g(r) from the lateral pair counts, and the replica sum of an
integer histogram.

The counts themselves come from libkmc (kmc_analysis.hip); nothing here
touches a trajectory.
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
