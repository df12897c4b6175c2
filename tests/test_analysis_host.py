"""Host side of the structure analysis (include/kmc.h), no GPU:
kmc_host_census against a numpy union-find, the g(r) normalisation, and the
replica sum of a histogram over gloo."""
import importlib
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from _analysis import chain_state, np_census, np_components, summary_dict
from _kmc import PKG, capi, engine, golden, scenarios, state_from_dump

analysis = importlib.import_module(PKG + ".analysis")


def _golden_state():
    sc = scenarios()["dense"]
    p = capi.default_params(**sc["params"])
    return p, state_from_dump(golden("dense")["state_20000"], sc["n_a"], sc["n_b"])


@pytest.fixture(scope="module", params=["chain", "golden"])
def case(request):
    p, hs = chain_state() if request.param == "chain" else _golden_state()
    return request.param, p, hs, np_components(hs)


@pytest.mark.parametrize("max_r,max_l", [(16, 8), (2, 1)])
def test_host_census_equals_union_find(case, max_r, max_l):
    name, p, hs, ref = case
    label, hist, out = engine.host_census(p, hs, max_r, max_l)
    ref_hist, ref_sum = np_census(hs, ref, max_r, max_l)
    assert np.array_equal(label, ref)
    assert np.array_equal(hist, ref_hist)  # (2, 1): everything larger clamped into the last row / column
    assert summary_dict(out) == ref_sum
    assert hist.sum() == out.n_components == len(np.unique(ref))
    if name == "chain":
        assert out.n_components == 1 and out.n_complexes == 1 and out.proteins_in_complexes == 1800
        assert (out.max_size, out.max_receptors, out.max_ligands, out.max_label) == (1800, 1200, 600, 1)
        assert hist[-1, -1] == 1
    else:
        # bond-rich: ligand complexes, and receptor-only cis dimers, which the BFS rows never show
        assert hs.counters[0] > 0 and out.n_complexes > 0 and out.n_cis_dimers > 0


def test_host_census_null_outputs_and_bad_arguments():
    import ctypes as C

    p, hs = _golden_state()
    L = engine.load_library()
    v = hs.view()
    out = capi.Census()
    assert L.kmc_host_census(C.byref(p), C.byref(v), None, 4, 4, None, C.byref(out)) == capi.KMC_OK
    assert summary_dict(out) == np_census(hs, np_components(hs), 4, 4)[1]
    assert L.kmc_host_census(C.byref(p), C.byref(v), None, 4, 4, None, None) == capi.ERR_ARG
    assert L.kmc_host_census(C.byref(p), C.byref(v), None, -1, 4, None, C.byref(out)) == capi.ERR_ARG
    bad = hs.copy()
    bad.a_int[2, 0] = p.n_a + p.n_b + 1  # a link past the last protein
    with pytest.raises(engine.KmcError) as e:
        engine.host_census(p, bad, 4, 4)
    assert e.value.code == capi.ERR_STATE


def test_census_layout_matches_header():
    import ctypes as C

    assert C.sizeof(capi.Census) == 48
    assert capi.Census.max_size.offset == 32 and capi.Census.max_label.offset == 44


def test_rdf_normalisation():
    counts = np.array([3, 0, 17, 40, 52, 61, 80, 91], dtype=np.int64)
    n_i, n_j, bx, by, r_max = 300, 100, 4000.0, 3000.0, 400.0
    for same in (True, False):
        g = analysis.rdf(counts, n_i, n_j, bx, by, r_max, same)
        pairs = n_i * (n_i - 1) / 2 if same else n_i * n_j
        want = []
        for k, c in enumerate(counts):
            r0, r1 = k * (r_max / 8), (k + 1) * (r_max / 8)
            want.append(c / (pairs * np.pi * (r1 * r1 - r0 * r0) / (bx * by)))
        assert np.allclose(g, want, rtol=1e-12, atol=0.0)
    assert np.array_equal(analysis.rdf(counts, 1, 0, bx, by, r_max, True), np.zeros(8))  # no pair at all


def _worker(rank, world, port, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    hist = np.arange(12, dtype=np.int64).reshape(3, 4) * (rank + 1) + (1 << 40) * rank
    got = analysis.reduce_counts(hist)
    if rank == 0:
        np.save(out, got)
    dist.destroy_process_group()


def test_reduce_counts_two_ranks(tmp_path):
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    out = str(tmp_path / "sum.npy")
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    base = np.arange(12, dtype=np.int64).reshape(3, 4)
    assert np.array_equal(np.load(out), base * 3 + (1 << 40))  # int64 all the way: no float round trip
    # no process group: the histogram unchanged
    assert np.array_equal(analysis.reduce_counts(base), base)
