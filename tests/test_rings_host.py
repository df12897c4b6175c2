"""Host side of the ligand network and its rings (include/kmc.h),
no GPU: the sequential kmc_host_network / kmc_host_rings against the Python
reference of tests/_rings.py on hand-bound networks, the closed forms of the
brick-wall lattice, every error return and analysis.ring_stats.  Every
comparison is exact equality."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _geometry import lattice_state
from _kmc import PKG, capi, engine
from _rings import (COUNTERS, HAND, LATTICE, RING_MAX, cycle, hand_state, lattice_counts, net_dict, network_state,
                    permuted, ref_network, ref_rings, same_network)

analysis = importlib.import_module(PKG + ".analysis")


def check_state(p, hs, max_len=RING_MAX):
    """host twin == reference: the network, the ring counts and the members; returns (counts, member, out)."""
    want_net = ref_network(hs)
    assert same_network(net_dict(*engine.host_network(p, hs)), want_net)
    counts, member, out = engine.host_rings(p, hs, max_len, members=True)
    want_counts, want_member = ref_rings(hs, max_len)
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    assert np.array_equal(member, want_member)
    assert out.as_dict() == {k: want_net[k] for k in COUNTERS + ("rec",)}
    counts_only, out2 = engine.host_rings(p, hs, max_len)  # member left out
    assert np.array_equal(counts_only, counts) and out2.as_dict() == out.as_dict()
    return counts, member, out


def lengths(row):
    return {L: int(c) for L, c in enumerate(row) if c}


def test_constants_and_layout():
    assert capi.RING_MAX == RING_MAX == 12
    assert C.sizeof(capi.NetOut) == 11 * 8


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_networks(name):
    p, hs = hand_state(name)
    counts, member, out = check_state(p, hs)
    d = out.as_dict()
    if name in ("none", "one_ligand"):
        assert not counts.any() and not member.any()
        assert d["n_bridges"] == d["n_vertices"] == d["n_net_components"] == d["cycle_rank"] == 0
    if name == "none":
        assert d["n_free_dimers"] == 2 and d["rec"] == [3, 2, 4, 0]
    if name == "loop":
        assert lengths(counts[0]) == lengths(counts[1]) == {1: 1}
        assert (d["n_loops"], d["n_bridges"], d["n_half"], d["cycle_rank"]) == (1, 2, 1, 1)
        assert member[0].tolist() == [0, 2, 0]
    if name == "double":
        assert lengths(counts[0]) == lengths(counts[1]) == {2: 1}
        assert member[1].tolist() == [4, 0, 4, 0]
    if name == "triple":
        assert lengths(counts[0]) == {2: 3} and not counts[1].any()
        assert member[0].tolist() == [4, 0, 4] and not member[1].any()
        assert d["cycle_rank"] == 2
    if name == "triangle":
        assert lengths(counts[0]) == lengths(counts[1]) == {3: 1}
    if name == "k4":
        assert lengths(counts[0]) == {3: 4, 4: 3} and lengths(counts[1]) == {3: 4}
        assert d["cycle_rank"] == 3
    if name == "theta":
        assert lengths(counts[0]) == lengths(counts[1]) == {4: 1, 5: 2}  # no path is a single bridge: no chord
    if name == "pendant":
        assert lengths(counts[0]) == lengths(counts[1]) == {6: 1}
        assert (d["n_half"], d["n_free_dimers"], d["n_vertices"], d["cycle_rank"]) == (2, 1, 10, 1)
        assert member[0].tolist() == [64] * 6 + [0] * 5


@pytest.mark.parametrize("L", range(3, 14))
def test_single_cycles(L):
    p, hs = network_state(L + 1, cycle(L, 1))
    counts, member, out = check_state(p, hs)
    if L <= RING_MAX:
        assert lengths(counts[0]) == lengths(counts[1]) == {L: 1}
        assert member[0].tolist() == [0] + [1 << L] * L
    else:
        assert not counts.any() and not member.any()  # C_13 is a cycle of the graph, but no ring of <= 12
    assert out.cycle_rank == 1


def test_max_len_cuts_the_search():
    p, hs = network_state(6, cycle(6))
    assert not check_state(p, hs, 5)[0].any()
    assert lengths(check_state(p, hs, 6)[0][1]) == {6: 1}
    p, hs = hand_state("k4")
    full = engine.host_rings(p, hs, RING_MAX)[0]
    for m in range(1, RING_MAX + 1):
        want = full.copy()
        want[:, m + 1:] = 0
        assert np.array_equal(engine.host_rings(p, hs, m)[0], want), m


@pytest.mark.parametrize("name", ["k4", "theta", "pendant", "loop", "triple"])
def test_renumbering_the_proteins(name):
    p, hs = hand_state(name)
    counts, member, out = engine.host_rings(p, hs, RING_MAX, members=True)
    hs2, pl = permuted(p, hs)
    counts2, member2, out2 = check_state(p, hs2)
    assert np.array_equal(counts2, counts)
    assert np.array_equal(member2[:, pl], member)
    assert out2.as_dict() == out.as_dict()


@pytest.mark.parametrize("key", sorted(LATTICE))
def test_brick_wall_lattice(key):
    p, hs = lattice_state(*key)
    counts, member, out = engine.host_rings(p, hs, RING_MAX, members=True)
    assert np.array_equal(counts, lattice_counts(key)), (lengths(counts[0]), lengths(counts[1]))
    assert out.cycle_rank == LATTICE[key][1]
    assert out.n_vertices == p.n_b and out.n_net_components == 1
    assert out.n_loops == out.n_free_dimers == out.n_half == 0
    net, hist, adj_lig, adj_site = engine.host_network(p, hs)
    assert net.as_dict() == out.as_dict()
    assert int(hist.sum()) == p.n_b and int(hist[3].sum()) == p.n_b  # every site of every ligand is occupied
    if key == (True, True):
        assert (member[0] & 64).all() and (member[1] & 64).all()  # every ligand of the torus lies on a hexagon
        assert int(hist[3, 3]) == p.n_b and (adj_lig > 0).all()
        st = analysis.ring_stats(counts, out)
        assert st["hexagon_fraction"] == 1.0 and st["rings_per_cycle"] == 3072 / 1025
    else:
        assert out.rec[1] == 2 * (3 * p.n_b // 2 - out.n_bridges)  # an opened edge leaves two receptors without partner


def code(f, *a, **kw):
    with pytest.raises(engine.KmcError) as e:
        f(*a, **kw)
    return e.value.code


def test_host_errors():
    p, hs = hand_state("pendant")
    for m in (0, -1, RING_MAX + 1):
        assert code(engine.host_rings, p, hs, m) == capi.ERR_ARG
    L = engine.load_library()
    v = hs.view()
    counts, out = np.zeros(2 * (RING_MAX + 1), dtype=np.int64), capi.NetOut()
    assert L.kmc_host_rings(C.byref(p), C.byref(v), 6, counts.ctypes.data, None, None) == capi.KMC_OK  # out may be left out
    assert L.kmc_host_rings(C.byref(p), C.byref(v), 6, None, None, C.byref(out)) == capi.ERR_ARG
    assert L.kmc_host_rings(None, C.byref(v), 6, counts.ctypes.data, None, C.byref(out)) == capi.ERR_ARG
    assert L.kmc_host_rings(C.byref(p), None, 6, counts.ctypes.data, None, C.byref(out)) == capi.ERR_ARG
    assert L.kmc_host_network(C.byref(p), C.byref(v), None, None, None, None) == capi.KMC_OK  # every array may be NULL
    assert L.kmc_host_network(None, C.byref(v), C.byref(out), None, None, None) == capi.ERR_ARG
    assert L.kmc_host_network(C.byref(p), None, C.byref(out), None, None, None) == capi.ERR_ARG
    # links of the wrong kind and asymmetric bridges on a view nobody validated
    na, n = p.n_a, p.n_a + p.n_b
    r = int(hs.b_int[5, 0])           # the receptor on ligand 0's site 2: part of a bridge of the hexagon
    r2 = int(hs.a_int[4, r - 1])      # its cis partner, on ligand 1's site 3
    other = int(hs.b_int[5, 7])       # a receptor of another bridge
    cases = [("b_int", 5, 0, n + 5), ("b_int", 5, 0, -2), ("b_int", 5, 0, na + 1),     # a ligand's link: no receptor
             ("b_int", 5, 0, other),                                                      # not the receptor's ligand
             ("a_int", 4, r - 1, n + 1), ("a_int", 4, r - 1, -1), ("a_int", 4, r - 1, r),  # a cis link: no other receptor
             ("a_int", 4, r - 1, other),                                                  # a cis link nobody returns
             ("a_int", 2, r2 - 1, 7), ("a_int", 2, r2 - 1, n + 1),                        # a receptor's ligand: none
             ("a_int", 2, r2 - 1, na + 3),                                                # the bridge ends elsewhere
             ("a_int", 3, r2 - 1, 2), ("a_int", 3, r2 - 1, 5), ("a_int", 3, r2 - 1, 0),   # ... or at another site
             ("a_int", 3, r - 1, 4)]
    for arr, row, col, bad in cases:
        broken = hs.copy()
        assert getattr(broken, arr)[row, col] != bad
        getattr(broken, arr)[row, col] = bad
        assert code(engine.host_network, p, broken) == capi.ERR_STATE, (arr, row, col, bad)
        assert code(engine.host_rings, p, broken, 6) == capi.ERR_STATE, (arr, row, col, bad)
    # a free dimer whose cis link is not returned
    fd = [i for i in range(na) if hs.a_int[4, i] and not hs.a_int[2, i] and not hs.a_int[2, hs.a_int[4, i] - 1]]
    broken = hs.copy()
    broken.a_int[4, fd[0]] = 0
    assert code(engine.host_network, p, broken) == capi.ERR_STATE


def test_ring_stats():
    counts = np.zeros((2, RING_MAX + 1), dtype=np.int64)
    counts[0, 6], counts[0, 10] = 5, 3
    counts[1, 6], counts[1, 4] = 4, 2
    st = analysis.ring_stats(counts, dict(n_vertices=16, cycle_rank=8))
    assert st == dict(hexagon_fraction=0.5, rings_per_vertex=6 / 16, mean_ring_length=32 / 6, rings_per_cycle=0.75)
    zero = analysis.ring_stats(np.zeros_like(counts), dict(n_vertices=0, cycle_rank=0))
    assert zero == dict(hexagon_fraction=0.0, rings_per_vertex=0.0, mean_ring_length=0.0, rings_per_cycle=0.0)
    assert analysis.ring_stats(counts, dict(n_vertices=16, cycle_rank=0))["rings_per_cycle"] == 0.0
    with pytest.raises(ValueError):
        analysis.ring_stats(counts[0], dict(n_vertices=1, cycle_rank=1))
    # additive over replicas: the sums of two states' counts and counters give the pooled numbers
    parts = [engine.host_rings(*hand_state(name), RING_MAX) for name in ("k4", "pendant")]
    total = sum(c for c, _ in parts)
    net = {k: sum(o.as_dict()[k] for _, o in parts) for k in ("n_vertices", "cycle_rank")}
    assert np.array_equal(analysis.reduce_counts(total), total)
    st = analysis.ring_stats(total, net)
    assert st["rings_per_vertex"] == 5 / 14 and st["rings_per_cycle"] == 5 / 4 and st["hexagon_fraction"] == 2 / 14
    p, hs = hand_state("k4")
    c, o = engine.host_rings(p, hs, RING_MAX)
    assert analysis.ring_stats(c, o) == analysis.ring_stats(c, o.as_dict())
