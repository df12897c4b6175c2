"""Helpers of test_gpu_layers_scale.py: the states at which the read-only layers
change code path.  The density recipe is test_gpu_resort.py's, the
rates are _kmc.DENSE's without its box, the raised dissociation rates are
test_gpu_dynamics.py's."""
import contextlib
import math
import os

import numpy as np

from _kmc import DENSE, capi, engine, params

FAST = 5e-4
RATES = {k: v for k, v in DENSE.items() if not k.startswith("box_")}
T = 256  # threads per workgroup of every layer kernel (AN_T, TRK_T, KIN_T, CF_T, BO_T)


def blocks(n):
    return (n + T - 1) // T


@contextlib.contextmanager
def env(**kw):
    """Environment variables set for the block; None removes one."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def scale_params(n_a, n_b, seed, fast=False):
    side = 5773.0 * math.sqrt((n_a + n_b) / 2000)
    kw = dict(RATES)
    if fast:
        kw.update(diss_rate=FAST, cis_diss_rate=FAST, mono_cis_diss_rate=FAST)
    return params(seed=seed, n_a=n_a, n_b=n_b, box_x=side, box_y=side, box_z=1000.0, **kw)


def state_facts(p, hs):
    """What an evolved state must hold before a layer is compared on it."""
    _, _, cs = engine.host_census(p, hs, 4, 4)
    return dict(rl=int(np.count_nonzero(hs.a_int[2])), cis=int(np.count_nonzero(hs.a_int[4])) // 2,
                max_size=int(cs.max_size), cis_dimers=int(cs.n_cis_dimers), bonds=int(hs.counters[0]))


def facts_hold(f):
    return f["rl"] > 0 and f["cis"] > 0 and f["max_size"] >= 3 and f["cis_dimers"] > 0 and f["bonds"] > 0


def evolve(p, chunk, most):
    """(simulation, state, facts): the random placement stepped on the device, `chunk` steps at a time and at most
    `most` chunks, until facts_hold."""
    sim = engine.Simulation(p)
    sim.set_state(engine.host_init_random(p))
    for _ in range(most):
        sim.step(chunk)
        hs = sim.get_state()
        f = state_facts(p, hs)
        if facts_hold(f):
            break
    return sim, hs, f


def patch_in_large_box(p0, hs0, box_x, box_y, inset=700.0):
    """(params, state): hs0 re-declared in a box_x x box_y box, every rigid body translated by (box / 2 - inset) and
    wrapped by its bead [1][1] into [-box/2, box/2) (as _geometry.lattice_state wraps): the patch straddles the
    corner of the large box, which is both of its seams.  inset=None translates nothing: the patch stays across
    the origin, where the cell grids of the bond order begin (they bin the coordinate modulo the box)."""
    p = capi.Params.from_buffer_copy(p0)
    p.box_x, p.box_y = box_x, box_y
    hs = hs0.copy()
    if inset is None:
        return p, hs
    for arr in (hs.ra, hs.rb):
        for c, box in ((0, box_x), (1, box_y)):
            v = arr[c] + (box / 2 - inset)
            d = (v - box * np.floor(v / box + 0.5)) - arr[c]
            arr[c::3] += d[None, :]
    return p, hs


def list_rows(p, hs, label, shift, span, min_size):
    """kmc_cluster_list's rows from a state and its labels, shifts and span bits (those of
    kmc_host_cluster_geometry), in int64 with the expressions of include/kmc.h: a list of tuples in _geometry.ROW's
    order, by label.  Exact while every |dx| stays below 2^31 (asserted)."""
    na, n = hs.n_a, hs.n_a + hs.n_b
    root = label.astype(np.int64) - 1
    size = np.bincount(root, minlength=n)
    n_r = np.bincount(root[:na], minlength=n)
    keep = np.flatnonzero(size[root] >= min_size)  # members of the listed components
    acc = np.zeros((5, n), dtype=np.int64)
    m = keep[span[keep] == 0]
    d = []
    for c, box in ((0, p.box_x), (1, p.box_y)):
        xy = np.concatenate([hs.ra[c], hs.rb[c]])
        X = engine.math(6, xy * 1024.0).astype(np.int64)
        B = int(engine.math(6, np.array([box * 1024.0]))[0])
        d.append(X[m] + shift[m, c].astype(np.int64) * B - X[root[m]])
        assert np.abs(d[-1]).max(initial=0) < 1 << 31
    for k, v in enumerate((d[0], d[1], d[0] * d[0], d[1] * d[1], d[0] * d[1])):
        np.add.at(acc[k], root[m], v)
    roots = np.flatnonzero((size >= min_size) & (root == np.arange(n)))
    return [(int(r) + 1, int(n_r[r]), int(size[r] - n_r[r]), int(span[r])) + tuple(int(acc[k, r]) for k in range(5))
            for r in roots]
