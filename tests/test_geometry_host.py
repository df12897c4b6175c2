"""Host side of the cluster geometry (include/kmc.h), no GPU:
kmc_host_cluster_geometry against the Python-integer reference of _geometry.py
on the brick-wall lattices and the chain, its error returns, the Rg² table
post-processing and the replica sum of a table over gloo."""
import ctypes as C
import importlib
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from _analysis import chain_state, np_components
from _geometry import (check_against, comp_m, far_chain_state, lattice_state, positions, ref_geometry, ref_rows, ref_summary,
                       table_tuples)
from _kmc import PKG, capi, engine

analysis = importlib.import_module(PKG + ".analysis")


@pytest.fixture(scope="module")
def chain():
    p, hs = chain_state()
    return p, hs, ref_geometry(p, hs)


@pytest.mark.parametrize("keep_x,keep_y", [(False, False), (True, False), (False, True), (True, True)])
def test_host_lattice_spanning_bits(keep_x, keep_y):
    p, hs = lattice_state(keep_x, keep_y)
    ref = ref_geometry(p, hs)
    bits = int(keep_x) + 2 * int(keep_y)
    n = p.n_a + p.n_b
    assert len(ref["comps"]) == 1 and ref["comps"][0]["span"] == bits  # the reference itself sees the wrap
    label, shift, span, table, out = engine.host_cluster_geometry(p, hs, 64)
    check_against(ref, label, shift, span, {64: table}, out)
    assert np.all(label == 1) and np.all(span == bits)
    assert (out.largest_label, out.largest_size, out.largest_span) == (1, n, bits)
    if bits:
        assert (out.n_spanning, out.n_measured, out.proteins_in_spanning) == (1, 0, n)
        assert (out.n_span_x, out.n_span_y) == (int(keep_x), int(keep_y))
        assert not shift.any() and table["count"].sum() == 0
        return
    # the open lattice straddles both seams of the box: members beyond them carry a shift on each axis, and the
    # unwrapped sheet has the radius of gyration of a 64 x 32 grid of pitch a, a^2 (64^2 - 1 + 32^2 - 1) / 12, inside
    # the box (the receptors sit on the grid's edges and change it by 0.02 %)
    for c in (0, 1):  # (+1 or -1 by the side of the seam the label lies on)
        assert len(np.unique(shift[:, c])) == 2 and np.abs(shift[:, c]).max() == 1
    assert table_tuples(table)[64] == (1, n, comp_m(ref["comps"][0]))
    rg2 = comp_m(ref["comps"][0]) / n ** 2 / 2 ** 20
    assert abs(rg2 - 200.0 ** 2 * (64 ** 2 - 1 + 32 ** 2 - 1) / 12) < 1e-3 * rg2
    assert np.sqrt(rg2) < 0.5 * p.box_x


def test_host_chain_shifts_and_table(chain):
    p, hs, ref = chain
    label, shift, span, table, out = engine.host_cluster_geometry(p, hs, 64)
    check_against(ref, label, shift, span, {64: table}, out)
    assert np.array_equal(label, np_components(hs)) and not span.any()
    # a random walk of 1800 bonds over a 6000 box: shifts in the tens, and m needs the high word
    assert np.abs(shift).max() >= 10
    c = ref["comps"][0]
    assert comp_m(c) >= 1 << 64
    assert table_tuples(table)[64] == (1, 1800, comp_m(c))
    _, _, _, t2, out2 = engine.host_cluster_geometry(p, hs, 2)  # the clamp: everything in the last bin
    assert table_tuples(t2) == [(0, 0, 0), (0, 0, 0), (1, 1800, comp_m(c))]
    assert ref_summary(ref) == {k: int(getattr(out2, k)) for k in ref_summary(ref)}


def test_host_far_chain_terms_past_64_bits():
    # the chain blown up 64 times: single squares pass 2^64, so the sums carry into the high word term by term
    p, hs = far_chain_state()
    ref = ref_geometry(p, hs)
    c = ref["comps"][0]
    assert min(c["s2xx"], c["s2yy"]) >= 1 << 70 and c["s2xy"] != 0 and not c["span"]
    label, shift, span, table, out = engine.host_cluster_geometry(p, hs, 64)
    check_against(ref, label, shift, span, {64: table}, out)


def test_host_null_outputs_and_bad_arguments(chain):
    p, hs, ref = chain
    L = engine.load_library()
    v = hs.view()
    out = capi.Geom()
    args = (C.byref(p), C.byref(v), None, None, None)
    assert L.kmc_host_cluster_geometry(*args, 8, None, C.byref(out)) == capi.KMC_OK
    assert {k: int(getattr(out, k)) for k in ref_summary(ref)} == ref_summary(ref)
    assert L.kmc_host_cluster_geometry(*args, 8, None, None) == capi.ERR_ARG
    assert L.kmc_host_cluster_geometry(*args, 1, None, C.byref(out)) == capi.ERR_ARG
    assert L.kmc_host_cluster_geometry(*args, 0, None, C.byref(out)) == capi.ERR_ARG
    assert L.kmc_host_cluster_geometry(None, C.byref(v), None, None, None, 8, None, C.byref(out)) == capi.ERR_ARG
    bad = hs.copy()
    bad.a_int[2, 0] = p.n_a + p.n_b + 1  # a link past the last protein
    with pytest.raises(engine.KmcError) as e:
        engine.host_cluster_geometry(p, bad, 8)
    assert e.value.code == capi.ERR_STATE


def test_geometry_layouts_match_header():
    assert C.sizeof(capi.I128) == 16 and C.sizeof(capi.GeomBin) == 32
    assert C.sizeof(capi.Geom) == 56 and capi.Geom.largest_label.offset == 40
    assert C.sizeof(capi.Cluster) == 80 and capi.Cluster.s1x.offset == 16 and capi.Cluster.s2xy.offset == 64
    assert int(capi.I128(lo=(1 << 64) - 1, hi=-1)) == -1 and int(capi.I128(lo=5, hi=2)) == (2 << 64) + 5


def _hand_table():
    # sizes 2, 3, 5 with Rg^2 = 100, 225, 625 A^2 exactly; max_size 8, the last bin mixed
    t = np.zeros(9, dtype=capi.GEOM_BIN_DTYPE)
    for n, count, rg2 in ((2, 7, 100), (3, 4, 225), (5, 2, 625)):
        m = count * rg2 * n * n << 20
        t[n] = (count, count * n, m & (2 ** 64 - 1), m >> 64)
    big = 3 * (1 << 100)  # a sum of m that needs the high word
    t[8] = (2, 8 + 11, big & (2 ** 64 - 1), big >> 64)
    return t


def test_rg_by_size_and_fractal_fit():
    t = _hand_table()
    sizes, counts, rg2, over = analysis.rg_by_size(t)
    assert sizes.tolist() == [2, 3, 5] and counts.tolist() == [7, 4, 2]
    assert rg2.tolist() == [100.0, 225.0, 625.0]
    assert over == dict(count=2, sum_size=19, rg2=None)  # sizes 8 and 11 share the bin: no single n to divide by
    t[8]["sum_size"] = 16
    over = analysis.rg_by_size(t)[3]
    assert over["rg2"] == 3 * (1 << 100) / (2 * 64 * (1 << 20))
    # Rg = 5 n exactly... not a power law; Rg^2 = 25 n^(2/1.6) is one: the fit returns the exponent
    n = np.array([2, 4, 8, 16, 64], dtype=np.float64)
    slope, icpt, df = analysis.fractal_fit(n, 25.0 * n ** (2 / 1.6), np.array([9, 5, 3, 2, 1]), min_size=2)
    assert abs(df - 1.6) < 1e-12 and abs(slope - 1 / 1.6) < 1e-12 and abs(icpt - np.log(5.0)) < 1e-12
    # min_size drops the small sizes; fewer than two left is an error
    assert abs(analysis.fractal_fit(n, 25.0 * n ** (2 / 1.6), np.ones(5), min_size=16)[2] - 1.6) < 1e-12
    with pytest.raises(ValueError):
        analysis.fractal_fit(n, 25.0 * n, np.ones(5), min_size=64)


def test_cluster_shapes_of_the_open_lattice():
    p, hs = lattice_state(False, False)
    ref = ref_geometry(p, hs)
    rows = [capi.Cluster(label=c["label"], n_r=c["n_r"], n_l=c["n_l"], span=c["span"], s1x=c["s1x"], s1y=c["s1y"],
                         **{k: capi.I128(lo=c[k] & (2 ** 64 - 1), hi=c[k] >> 64) for k in ("s2xx", "s2yy", "s2xy")})
            for c in ref_rows(ref, 2)]
    sh = analysis.cluster_shapes(rows, p, positions(hs))
    assert sh["size"].tolist() == [p.n_a + p.n_b] and sh["span"].tolist() == [0]
    # the centre: every member's minimum image around the middle of the sheet's extent — columns -1/3 .. 63 1/3 and rows
    # -1/3 .. 31 1/3 (an open edge's receptors stay with their ligands) from the origin (-13.37, -7.77), less than a box wide — averaged and wrapped (the integer
    # coordinates are within 2^-11 A of the doubles)
    box = np.array([p.box_x, p.box_y])
    mid = np.array([-13.37, -7.77]) + 100.0 * np.array([63.0, 31.0])
    d = positions(hs) - mid
    want = mid + (d - box * np.floor(d / box + 0.5)).mean(axis=0)
    want = want - box * np.floor(want / box + 0.5)
    assert np.abs(sh["centre"][0] - want).max() < 2e-3
    assert abs(sh["rg"][0] ** 2 - (sh["lam1"][0] + sh["lam2"][0])) < 1e-6 * sh["rg"][0] ** 2
    # a 64 x 32 grid of pitch 200: eigenvalues a^2 (64^2 - 1) / 12 and a^2 (32^2 - 1) / 12, receptors aside
    assert abs(sh["lam1"][0] - 200.0 ** 2 * (64 ** 2 - 1) / 12) < 5e-3 * sh["lam1"][0]
    assert abs(sh["lam2"][0] - 200.0 ** 2 * (32 ** 2 - 1) / 12) < 5e-3 * sh["lam2"][0]
    assert 0.3 < sh["asphericity"][0] < 0.45  # ((4095 - 1023) / (4095 + 1023))^2 = 0.36
    # a spanning row has no shape
    rows[0].span = 1
    assert np.isnan(analysis.cluster_shapes(rows, p, positions(hs))["rg"][0])


def _worker(rank, world, port, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = analysis.reduce_geom(_hand_table())
    if rank == 0:
        np.save(out, got)
    dist.destroy_process_group()


def test_reduce_geom_world_one(tmp_path):
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    out = str(tmp_path / "sum.npy")
    mp.spawn(_worker, args=(1, port, out), nprocs=1, join=True)
    t = _hand_table()
    got = np.load(out)
    assert got.dtype == capi.GEOM_BIN_DTYPE and table_tuples(got) == table_tuples(t)
    # no process group: the table unchanged, a negative and a carrying 128-bit word included
    t[4] = (1, 4, 2 ** 64 - 1, -1)
    t[6] = (1, 6, 2 ** 63, 2 ** 62)
    assert table_tuples(analysis.reduce_geom(t)) == table_tuples(t)
