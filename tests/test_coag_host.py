"""Host side of the cluster growth kinetics: the sequential
counterpart kmc_host_cf_* (engine.HostCoag, breadth-first walks) and the
plain-Python recorder of tests/_coag.py (sets and union-find) on a hand-made
sequence with values worked out by hand, on the graph states of the other
helpers, on a trajectory of the CPU oracle, and analysis.coag_kernel /
frag_kernel / growth_modes.  Every comparison is integer equality.  No device
needed."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import _analysis
import _coag as cg
import _geometry
from _kmc import DENSE, PKG, REPO, O, capi, engine, params

analysis = importlib.import_module(PKG + ".analysis")

FAST = 5e-3
LOOK = ("formed_rl", "formed_cis", "broken_rl", "broken_cis", "n_cores", "n_clusters", "cycles_closed",
        "cycles_opened", "max_cluster")


def _both(p, hs, S):
    return engine.HostCoag(p, hs, S), cg.Recorder(p, hs, S)


def _same(host, rec, out=None):
    """The host recorder's arrays, counters and tables against the Python one's."""
    assert cg.same_arrays(host.arrays, rec)
    want = rec.out()
    got = (out if out is not None else host.acc).as_dict()
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert cg.table_differences(host.tables, rec.tables()) == []


def _filled(shape, entries):
    w = np.zeros(shape, dtype=np.int64)
    for idx, c in entries.items():
        w[idx] = c
    return w


def test_hand_made_sequence():
    p = params(n_a=6, n_b=3)
    S = cg.HAND_S
    host, rec = _both(p, cg.state(p, *cg.SEQUENCE[0]), S)
    _same(host, rec)
    d = rec.out()
    assert (d["origin_step"], d["last_step"], d["n_updates"], d["max_size"]) == (100, 100, 0, S)
    assert (d["n_clusters"], d["max_cluster"], d["n_cores"]) == (7, 3, 0) and rec.n_s.tolist() == [0, 6, 0, 1, 0, 0]
    assert rec.arrays()["prev_label"].tolist() == [1, 1, 3, 4, 5, 6, 1, 8, 9]
    updates = 0
    for step, links in cg.SEQUENCE[1:]:
        hs = cg.state(p, step, links)
        out = host.update(hs)
        rec.update(hs)
        updates += 1
        _same(host, rec, out)
        d = rec.out()
        got = (tuple(d[k] for k in LOOK), rec.n_s[1:].tolist(), rec.t["expo"][1:].tolist())
        assert got == cg.HAND_LOOKS[step], step
        if step == 104:
            # the site change of receptor 2 is a kept edge: one fragmentation (1, 3), nothing formed
            assert rec.t["frag"].sum() == 1 and rec.t["frag"][1, 3] == 1 and rec.t["frag_kind"][0, 3] == 1
        if step == 115:
            # a second update at the same step changes nothing but n_updates
            before = (rec.arrays(), rec.tables(), rec.out())
            out = host.update(hs)
            rec.update(hs)
            updates += 1
            _same(host, rec, out)
            after = rec.out()
            assert after.pop("n_updates") == before[2].pop("n_updates") + 1 and after == before[2]
            assert all(np.array_equal(rec.arrays()[k], before[0][k]) for k in cg.ARRAYS)
            assert all(np.array_equal(rec.tables()[k], before[1][k]) for k in cg.TABLES)
            assert rec.tables()["expo2"] == before[1]["expo2"]
    out, tables = host.sample()
    assert out.as_dict() == rec.out() and cg.table_differences(tables, rec.tables()) == []
    assert (out.origin_step, out.last_step, out.n_updates) == (100, 121, updates) and updates == 9
    s1 = S + 1
    shapes = dict(merge=(s1, s1), frag=(s1, s1), merge_kind=(4, 4), frag_kind=(4, 4), merge_pieces=9, frag_pieces=9,
                  merge_product=s1, frag_parent=s1)
    for name, entries in cg.HAND_TABLES.items():
        assert np.array_equal(getattr(tables, name), _filled(shapes[name], entries)), name
    want2 = [[0] * s1 for _ in range(s1)]
    for (a, b), c in cg.HAND_EXPO2.items():
        want2[a][b] = c
    assert tables.expo2_int() == want2
    assert tables.n_s.tolist() == [0, 4, 1, 1, 0, 0]
    a = rec.arrays()
    assert a["rl_lig"].tolist() == [0, 0, 9, 8, 0, 0] and a["cis_with"].tolist() == [0, 0, 0, 6, 0, 4]
    assert a["prev_label"].tolist() == [1, 2, 3, 4, 5, 4, 7, 4, 3]
    m = analysis.growth_modes(out, tables.merge_kind)
    assert m["binary_mergers"] == 4 and m["receptor_addition"] == 1.0 and m["cluster_cluster"] == 0.0
    assert (m["cycles_closed"], m["cycles_opened"], m["ring_fraction"]) == (1, 1, 0.125)


def _cut_and_join(p, whole, cut, S):
    """whole -> cut (a fragmentation) with one pair of recorders, cut -> whole (the merger) with another."""
    a, b = whole.copy(), cut.copy()
    a.step, b.step = 10, 17
    host, rec = _both(p, a, S)
    out = host.update(b)
    rec.update(b)
    _same(host, rec, out)
    b.step, a.step = 10, 17
    host2, rec2 = _both(p, b, S)
    out2 = host2.update(a)
    rec2.update(a)
    _same(host2, rec2, out2)
    return rec, rec2


def test_chain_falls_into_four_pieces_and_joins_again():
    p, hs = _analysis.chain_state()
    assert len(cg.cis_bonds(hs)) == 599
    cut = cg.without_cis(hs, cg.chain_cuts(p))
    S = 16
    frag, merge = _cut_and_join(p, hs, cut, S)
    d, t = frag.out(), frag.tables()
    assert t["frag_pieces"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0] and t["frag_parent"][S] == 1
    assert t["frag_parent"].sum() == 1 and not t["frag"].any() and not t["merge_pieces"].any()
    assert (d["broken_cis"], d["n_cores"], d["n_clusters"], d["cycles_opened"], d["cycles_closed"]) == (3, 4, 4, 0, 0)
    assert t["n_s"].tolist() == [0] * S + [4] and t["expo"][S] == 7 and d["max_cluster"] < 1800
    d, t = merge.out(), merge.tables()
    assert t["merge_pieces"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0] and t["merge_product"][S] == 1
    assert not t["merge"].any() and not t["frag_pieces"].any()
    assert (d["formed_cis"], d["n_cores"], d["n_clusters"], d["cycles_closed"], d["max_cluster"]) == (3, 4, 1, 0, 1800)
    assert t["expo"][S] == 28 and t["expo2"][S][S] == 7 * 6


def test_lattice_opens_and_closes_a_cycle():
    p, hs = _geometry.lattice_state(True, True)
    cut = cg.without_cis(hs, [cg.cis_bonds(hs)[1234][0]])
    opened, closed = _cut_and_join(p, hs, cut, 8)
    d, t = opened.out(), opened.tables()
    assert (d["cycles_opened"], d["cycles_closed"], d["broken_cis"], d["n_cores"], d["n_clusters"]) == (1, 0, 1, 1, 1)
    assert not t["frag_pieces"].any() and not t["merge_pieces"].any() and not t["frag"].any()
    d, t = closed.out(), closed.tables()
    assert (d["cycles_closed"], d["cycles_opened"], d["formed_cis"], d["n_cores"], d["n_clusters"]) == (1, 0, 1, 1, 1)
    assert not t["frag_pieces"].any() and not t["merge_pieces"].any() and not t["merge"].any()


@pytest.fixture(scope="module")
def oracle_run():
    """DENSE, seed 23: 6000 steps of the oracle, then 600 with the dissociation rates raised to 5e-3, recorded
    by both recorders after every step and, in a second pair, after every 5 steps, with S = 16 and with S = 4.
    Everything is compared on the way; returns (params, first state, last state, {(every, S): Python recorder})."""
    p0 = params(seed=23, **DENSE)
    o = O.Oracle(p0)
    o.init_placement()
    o.step(6000, want_hashes=False)
    st = o.get_state()
    fast = dict(DENSE)
    fast.update(diss_rate=FAST, cis_diss_rate=FAST, mono_cis_diss_rate=FAST)
    p = params(seed=23, **fast)
    o = O.Oracle(p)
    o.set_state(st)
    pairs = {(every, S): _both(p, st, S) for every in (1, 5) for S in (16, 4)}
    hs = st
    for k in range(1, 601):
        o.step(1, want_hashes=False)
        hs = o.get_state()
        assert hs.step == st.step + k
        for (every, S), (host, rec) in pairs.items():
            if k % every == 0:
                out = host.update(hs)
                rec.update(hs)
                if every == 5 or k % 10 == 0 or k < 50:
                    _same(host, rec, out)
    for host, rec in pairs.values():
        _same(host, rec)
        out, tables = host.sample()
        assert out.as_dict() == rec.out() and cg.table_differences(tables, rec.tables()) == []
    return p, st, hs, {k: v[1] for k, v in pairs.items()}


def _upper(t):
    return int(np.triu(t).sum())


def test_oracle_trajectory_event_floors(oracle_run):
    p, st, end, recs = oracle_run
    t1, t5 = recs[(1, 16)].tables(), recs[(5, 16)].tables()
    d1 = recs[(1, 16)].out()
    print("every step:", {k: d1[k] for k in LOOK}, "merge", _upper(t1["merge"]), "frag", _upper(t1["frag"]),
          "pieces", t1["merge_pieces"].tolist(), t1["frag_pieces"].tolist())
    print("every 5:", "merge", _upper(t5["merge"]), "frag", _upper(t5["frag"]), "pieces", t5["merge_pieces"].tolist(),
          t5["frag_pieces"].tolist())
    print("merge rows a = 1:", t1["merge"][1].tolist())
    assert d1["n_updates"] == 600 and recs[(5, 16)].out()["n_updates"] == 120
    assert _upper(t1["merge"]) >= 100 and _upper(t1["frag"]) >= 100
    assert _upper(t1["merge"][2:]) >= 5 and _upper(t1["frag"][2:]) >= 5, "binary events of two clusters (a >= 2)"
    assert t1["frag_pieces"][3:].sum() >= 3 and t1["merge_pieces"][3:].sum() >= 2, "multi-piece events"
    assert t5["frag_pieces"][4] >= 1
    # the stroboscopic recorder sees no more bonds change than the exact one
    d5 = recs[(5, 16)].out()
    assert d5["formed_rl"] + d5["formed_cis"] <= d1["formed_rl"] + d1["formed_cis"]
    assert d5["broken_rl"] + d5["broken_cis"] <= d1["broken_rl"] + d1["broken_cis"]


@pytest.mark.parametrize("every", [1, 5])
def test_oracle_trajectory_identities(oracle_run, every):
    p, st, end, recs = oracle_run
    rec = recs[(every, 16)]
    d, t = rec.out(), rec.tables()
    n = p.n_a + p.n_b
    assert all(ns[16] == 0 for _, ns in rec.looks), "nothing is clamped at S = 16"
    assert t["merge_pieces"][8] == 0 and t["frag_pieces"][8] == 0
    e0, e1 = set.union(*cg.bonds(st)), set.union(*cg.bonds(end))
    c0, c1 = (len(cg.members(cg.partition(n, e))) for e in (e0, e1))
    k = np.arange(9) - 1
    assert _upper(t["merge"]) == t["merge_pieces"][2] and _upper(t["frag"]) == t["frag_pieces"][2]
    assert _upper(t["merge_kind"]) == t["merge_pieces"][2] and _upper(t["frag_kind"]) == t["frag_pieces"][2]
    assert t["merge_product"].sum() == t["merge_pieces"].sum() and t["frag_parent"].sum() == t["frag_pieces"].sum()
    assert d["formed_rl"] + d["formed_cis"] - d["broken_rl"] - d["broken_cis"] == len(e1) - len(e0)
    assert (k * t["frag_pieces"]).sum() - (k * t["merge_pieces"]).sum() == c1 - c0
    assert d["cycles_closed"] - d["cycles_opened"] == cg.cycle_rank(n, e1) - cg.cycle_rank(n, e0)
    assert d["cycles_closed"] >= 0 and d["cycles_opened"] >= 0
    assert d["n_clusters"] == c1
    assert all(int((np.arange(17) * ns).sum()) == n for _, ns in rec.looks)
    # the exposures from the size histogram of every look
    expo = np.zeros(17, dtype=np.int64)
    expo2 = [[0] * 17 for _ in range(17)]
    for (s0, ns), (s1, _) in zip(rec.looks, rec.looks[1:]):
        expo += (s1 - s0) * ns
        for a in range(1, 17):
            for b in range(a, 17):
                na, nb = int(ns[a]), int(ns[b])
                expo2[a][b] += (s1 - s0) * (na * (na - 1) // 2 if a == b else na * nb)
    assert np.array_equal(expo, t["expo"]) and expo2 == t["expo2"]
    assert expo.sum() > 0 and expo2[1][1] > 0


def test_oracle_trajectory_clamp_bins_fill(oracle_run):
    p, st, end, recs = oracle_run
    for every in (1, 5):
        wide, tight = recs[(every, 16)].tables(), recs[(every, 4)].tables()
        # the clamped tables are the unclamped ones folded at S = 4
        fold = np.minimum(np.arange(17), 4)
        for name in ("merge", "frag"):
            want = np.zeros((5, 5), dtype=np.int64)
            np.add.at(want, (fold[:, None], fold[None, :]), wide[name])
            assert np.array_equal(np.triu(want) + np.tril(want, -1).T, tight[name]), name
        for name in ("merge_product", "frag_parent", "n_s", "expo"):
            assert np.array_equal(np.bincount(fold, weights=wide[name], minlength=5).astype(np.int64), tight[name])
        for name in ("merge_kind", "frag_kind", "merge_pieces", "frag_pieces"):
            assert np.array_equal(wide[name], tight[name])
        assert recs[(every, 4)].out() == dict(recs[(every, 16)].out(), max_size=4)
    tight = recs[(1, 4)].tables()
    assert tight["merge_product"][4] > 0 and tight["frag_parent"][4] > 0 and tight["expo"][4] > 0
    assert tight["merge"][:, 4].sum() > 0 and tight["frag"][:, 4].sum() > 0


def test_link_out_of_range_is_refused():
    p = params(n_a=6, n_b=3)
    F = cg.F
    good = cg.state(p, 0, [(7, 2, 0), F, F, F, F, F])
    for bad in ([(6, 2, 0)] + [F] * 5, [(10, 2, 0)] + [F] * 5, [(0, 0, 7)] + [F] * 5, [(0, 0, 1)] + [F] * 5,
                [(-1, 0, 0)] + [F] * 5, [F] * 5 + [(0, 0, -2)]):
        with pytest.raises(engine.KmcError) as e:
            engine.HostCoag(p, cg.state(p, 0, bad), 4)
        assert e.value.code == capi.ERR_STATE
        host = engine.HostCoag(p, good, 4)
        before = {k: getattr(host.arrays, k).copy() for k in cg.ARRAYS}
        with pytest.raises(engine.KmcError) as e:
            host.update(cg.state(p, 3, bad))
        assert e.value.code == capi.ERR_STATE
        assert all(np.array_equal(getattr(host.arrays, k), before[k]) for k in cg.ARRAYS) and host.acc.n_updates == 0
    for S in (1, 64, -3):
        with pytest.raises(engine.KmcError) as e:
            engine.HostCoag(p, good, S)
        assert e.value.code == capi.ERR_ARG
    # a recorder whose label is not its class' smallest member
    host = engine.HostCoag(p, good, 4)
    host.arrays.prev_label[0] = 7
    with pytest.raises(engine.KmcError) as e:
        host.update(cg.state(p, 2, [(7, 2, 0), F, F, F, F, F]))
    assert e.value.code == capi.ERR_STATE
    L = engine.load_library()
    v = good.view()
    assert L.kmc_host_cf_begin(C.byref(p), C.byref(v), 4, None, None, None) == capi.ERR_ARG
    assert L.kmc_host_cf_update(C.byref(p), C.byref(v), None, None, None) == capi.ERR_ARG


def test_cf_struct_layouts_match_header(tmp_path):
    structs = {"kmc_cf_out": capi.CfOut, "kmc_cf_view": capi.CfView, "kmc_cf_tables": capi.CfTablesView}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(REPO, "include", "kmc.h")}"',
             "int main(void){"]
    for st, cls in structs.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("consts %d %d %d %zu\\n", KMC_CF_MAX_SIZE, KMC_CF_PIECES, KMC_CF_KINDS, sizeof(kmc_i128));')
    lines.append("return 0;}")
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-O0", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True,
                                                               check=True).stdout.splitlines()}
    for st, cls in structs.items():
        assert int(got[st][0]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{st}.{f}"][0]) == getattr(cls, f).offset, f"{st}.{f}"
    assert [int(x) for x in got["consts"]] == [capi.CF_MAX_SIZE, capi.CF_PIECES, capi.CF_KINDS,
                                               capi.I128_DTYPE.itemsize]
    assert len(capi.CF_KIND_NAMES) == capi.CF_KINDS and tuple(cg.COUNTERS) == tuple(
        f for f, _ in capi.CfOut._fields_)


def test_analysis_helpers_on_hand_values():
    merge = np.zeros((5, 5), dtype=np.int64)
    merge[1, 1], merge[1, 2], merge[2, 4] = 6, 3, 5
    expo2 = np.zeros((5, 5), dtype=capi.I128_DTYPE)
    expo2[1, 1] = (12, 0)
    expo2[1, 2] = (0, 3)              # 3 * 2^64: passes 64 bits
    expo2[2, 4] = (2 ** 63, 0)        # the low word's top bit is not a sign
    K = analysis.coag_kernel(merge, expo2)
    assert K[1, 1] == 0.5 and K[1, 2] == K[2, 1] == 3 / (3 * 2 ** 64) == 2.0 ** -64
    assert K[2, 4] == K[4, 2] == 5 / 2 ** 63 and np.isnan(K[3, 3]) and np.isnan(K[0, 0])
    assert np.array_equal(analysis.coag_kernel(merge, [[int(w["hi"]) * 2 ** 64 + int(w["lo"]) for w in row]
                                                       for row in expo2]), K, equal_nan=True)
    frag = np.zeros((5, 5), dtype=np.int64)
    frag[1, 1], frag[1, 2], frag[2, 2], frag[1, 4] = 4, 9, 7, 1
    expo = np.array([0, 100, 16, 36, 50], dtype=np.int64)
    Fk = analysis.frag_kernel(frag, expo)
    assert Fk[1, 1] == 0.25 and Fk[1, 2] == Fk[2, 1] == 0.25
    assert np.isnan(Fk[2, 2]) and np.isnan(Fk[1, 4]) and np.isnan(Fk[1, 3])  # a + b >= S: the parent is clamped
    kind = np.zeros((4, 4), dtype=np.int64)
    kind[0, 0], kind[0, 1], kind[0, 3], kind[1, 3], kind[2, 3], kind[3, 3] = 2, 4, 6, 3, 1, 4
    out = dict(formed_rl=30, formed_cis=10, cycles_closed=4, cycles_opened=1)
    m = analysis.growth_modes(out, kind)
    assert m["binary_mergers"] == 20 and m["receptor_addition"] == 0.6 and m["ligand_addition"] == 0.15
    assert m["cluster_cluster"] == 0.25 and m["ring_fraction"] == 0.1
    assert (m["cycles_closed"], m["cycles_opened"]) == (4, 1)
    assert analysis.growth_modes(capi.CfOut(), np.zeros((4, 4)))["receptor_addition"] == 0.0
    # the int64 tables add over replicas unchanged
    r = analysis.reduce_counts(merge)
    assert r.dtype == np.int64 and np.array_equal(r, merge) and r is not merge
