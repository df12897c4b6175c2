"""Host side of the bond kinetics: the sequential counterpart
kmc_host_kin_* (engine.HostKinetics) and the plain-Python recorder of
tests/_kinetics.py on hand-made sequences with values worked out by hand, on
a trajectory of the CPU oracle, the bin rule, and analysis.kinetics_rates /
lifetime_survival / kin_bin_edges.  Every comparison of the two recorders is
exact equality.  No device needed."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

from _kinetics import ARRAYS, EVENTS, Recorder, first_difference, kin_bin, same_arrays
from _kmc import DENSE, PKG, REPO, O, capi, engine, params

analysis = importlib.import_module(PKG + ".analysis")

FAST = 5e-3


def _state(p, step, links):
    """A host state that holds only what the recorder reads: links[i] = (lig, site, cis) of receptor i + 1."""
    hs = capi.HostState(p.n_a, p.n_b)
    for i, (lig, site, cis) in enumerate(links):
        hs.a_int[2, i], hs.a_int[3, i], hs.a_int[4, i] = lig, site, cis
    hs.step = step
    return hs


def _both(p, hs):
    return engine.HostKinetics(p, hs), Recorder(p, hs)


def _same(host, rec, out=None):
    """The host recorder's arrays, counters and rows against the Python one's."""
    assert same_arrays(host.arrays, rec), first_difference(host.arrays, rec)
    want = rec.out()
    got = (out if out is not None else host.acc).as_dict()
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert np.array_equal(host.hist, rec.hist)


def _same_sample(host, rec):
    out, hist = host.sample()
    want, want_hist = rec.sample()
    assert out.as_dict() == want, {k: (out.as_dict()[k], want[k]) for k in want if out.as_dict()[k] != want[k]}
    assert np.array_equal(hist, want_hist)
    return want, want_hist


# receptors 1..4, ligands 5 and 6; (lig, site, cis) per receptor at each look, irregular gaps
F = (0, 0, 0)
SEQUENCE = [
    # begin: R1 holds ligand 5 (left-censored), the cis bond {3, 4} exists (left-censored, mono)
    (10, [(5, 2, 0), F, (0, 0, 4), (0, 0, 3)]),
    # R1 loses its ligand after 3 steps (row 1); R2 binds ligand 6 (a first bond: no waiting time)
    (13, [F, (6, 2, 0), (0, 0, 4), (0, 0, 3)]),
    # R1 takes ligand 5 back after 1 step, at another site (row 5)
    (14, [(5, 3, 0), (6, 2, 0), (0, 0, 4), (0, 0, 3)]),
    # R1: the same ligand at another site — a new bond and a swap, L = 6, W = 0 (row 5); R2 loses ligand 6, L = 7
    (20, [(5, 2, 0), F, (0, 0, 4), (0, 0, 3)]),
    # R2 binds another ligand than the one it lost, W = 1 (row 6); receptor 3 leaves partner 4 for partner 1:
    # the censored bond {3, 4} ends at 3 after 11 steps (row 4, a swap), {1, 3} is born at 1 — complex, R1 holds 5
    (21, [(5, 2, 3), (5, 4, 0), (0, 0, 1), F]),
    # R2 loses ligand 5, L = 4, and pairs with R4: {2, 4} is born mono
    (25, [(5, 2, 3), (0, 0, 4), (0, 0, 1), (0, 0, 2)]),
    # R4 binds ligand 6: {2, 4} turns complex
    (30, [(5, 2, 3), (0, 0, 4), (0, 0, 1), (6, 3, 2)]),
    # {2, 4} ends after 8 steps as a complex bond (row 3); R1 loses ligand 5, L = 13: {1, 3} turns mono
    (33, [(0, 0, 3), F, (0, 0, 1), (6, 3, 0)]),
    # {1, 3} ends mono after 19 steps (row 2, bin 17); R4 swaps ligand 6 for ligand 5: L = 10, W = 0 (row 6)
    (40, [F, F, F, (5, 3, 0)]),
]
EXPOSURE = {  # (rl, mono, cx, free_receptor, free_site) after the update at each step
    13: (3, 3, 0, 9, 15), 14: (4, 4, 0, 12, 20), 20: (16, 10, 0, 24, 44), 21: (17, 11, 0, 27, 49),
    25: (25, 11, 4, 35, 65), 30: (30, 16, 9, 50, 90), 33: (36, 16, 15, 56, 102), 40: (43, 23, 15, 77, 137),
}
OCCUPANCY = {  # (rl, mono, cx) at each look
    10: (1, 1, 0), 13: (1, 1, 0), 14: (2, 1, 0), 20: (1, 1, 0), 21: (2, 0, 1), 25: (1, 1, 1), 30: (2, 0, 2),
    33: (1, 1, 0), 40: (1, 0, 0),
}


def test_hand_made_sequence():
    p = params(n_a=4, n_b=2)
    host, rec = _both(p, _state(p, *SEQUENCE[0]))
    _same(host, rec)
    d, hist = _same_sample(host, rec)
    assert (d["n_rl_censored_alive"], d["n_cis_censored_alive"]) == (1, 1) and not hist.any()
    assert (d["origin_step"], d["last_step"], d["n_updates"]) == (10, 10, 0)
    updates = 0
    for step, links in SEQUENCE[1:]:
        hs = _state(p, step, links)
        out = host.update(hs)
        rec.update(hs)
        updates += 1
        _same(host, rec, out)
        d = rec.out()
        assert tuple(d[k] for k in ("exp_rl", "exp_mono", "exp_cx", "exp_free_receptor", "exp_free_site")) == \
            EXPOSURE[step], step
        assert (d["occ_rl"], d["occ_mono"], d["occ_cx"]) == OCCUPANCY[step], step
        assert (d["occ_free_receptor"], d["occ_free_site"]) == (4 - d["occ_rl"], 6 - d["occ_rl"])
        if step == 14:
            d, hist = _same_sample(host, rec)
            assert (d["n_rl_censored_alive"], d["n_cis_censored_alive"]) == (0, 1)
            assert hist[7, 0] == 1 and hist[7, 1] == 1 and hist[7].sum() == 2 and hist[8].sum() == 0
        if step == 20:
            # a second update at the same step changes nothing but n_updates
            before = (rec.arrays(), rec.hist.copy(), rec.out())
            out = host.update(hs)
            rec.update(hs)
            updates += 1
            _same(host, rec, out)
            after = rec.out()
            assert after.pop("n_updates") == before[2].pop("n_updates") + 1 and after == before[2]
            assert all(np.array_equal(rec.arrays()[k], before[0][k]) for k in ARRAYS)
            assert np.array_equal(rec.hist, before[1])
        if step == 30:
            d, hist = _same_sample(host, rec)
            # alive: R1's bond since 20 and R4's since 30; {1, 3} since 21 and {2, 4} since 25
            assert hist[7, 10] == 1 and hist[7, 0] == 1 and hist[7].sum() == 2
            assert hist[8, 9] == 1 and hist[8, 5] == 1 and hist[8].sum() == 2
            assert (d["n_rl_censored_alive"], d["n_cis_censored_alive"]) == (0, 0)
    d, hist = _same_sample(host, rec)
    assert [d[k] for k in EVENTS] == [6, 6, 2, 2, 2, 1, 1]  # rl_on rl_off rl_swap cis_on off_mono off_cx cis_swap
    assert (d["origin_step"], d["last_step"], d["n_updates"]) == (10, 40, updates) and updates == 9
    want = np.zeros((9, 256), dtype=np.int64)
    for row, b in ((0, 6), (0, 7), (0, 4), (0, 13), (0, 10), (1, 3), (2, 17), (3, 8), (4, 11), (5, 1), (5, 0), (6, 1),
                   (6, 0), (7, 0)):
        want[row, b] += 1
    assert np.array_equal(hist, want)
    a = rec.arrays()
    assert a["rl_lig"].tolist() == [0, 0, 0, 5] and a["rl_site"].tolist() == [0, 0, 0, 3]
    assert a["rl_since"].tolist() == [20, 21, 10, 40] and a["cis_with"].tolist() == [0, 0, 0, 0]
    assert a["cis_since"].tolist() == [21, 25, 21, 25] and a["last_lig"].tolist() == [5, 5, 0, 6]
    assert a["free_since"].tolist() == [33, 25, 10, 40] and a["bits"].tolist() == [0, 0, 0, 0]


def test_bin_rule_through_the_step_counter():
    # a left-censored bond that ends after v steps lands in row 1, bin(v); the large v only through hs.step
    p = params(n_a=4, n_b=2)
    cases = {0: 0, 15: 15, 16: 16, 17: 16, 31: 23, 32: 24, 2 ** 34 - 1: 255, 2 ** 34: 255, 2 ** 40: 255}
    for v, b in cases.items():
        host, rec = _both(p, _state(p, 0, [(5, 2, 0), F, F, F]))
        hs = _state(p, v, [F, F, F, F])
        out = host.update(hs)
        rec.update(hs)
        _same(host, rec, out)
        assert kin_bin(v) == b
        assert host.hist[1, b] == 1 and host.hist.sum() == 1, v
        assert out.exp_rl == v and out.exp_free_receptor == 3 * v and out.exp_free_site == 5 * v
    # the last regular bin ends where the clamp begins
    assert kin_bin(2 ** 34 - 2 ** 30 - 1) == 254 and kin_bin(2 ** 34 - 2 ** 30) == 255


def test_bin_edges_invert_the_bin_rule():
    edges = analysis.kin_bin_edges()
    assert edges.dtype == np.int64 and edges.shape == (capi.KIN_BINS,)
    assert edges[:18].tolist() == list(range(16)) + [16, 18] and edges[24] == 32 and edges[255] == 15 << 30
    for b in range(capi.KIN_BINS):
        assert kin_bin(int(edges[b])) == b
        if b:
            assert kin_bin(int(edges[b]) - 1) == b - 1


def test_link_out_of_range_is_refused():
    p = params(n_a=4, n_b=2)
    good = _state(p, 0, [(5, 2, 0), F, F, F])
    for bad in ([(4, 2, 0), F, F, F], [(7, 2, 0), F, F, F], [(0, 0, 5), F, F, F], [(0, 0, 1), F, F, F],
                [(5, 5, 0), F, F, F], [(-1, 0, 0), F, F, F]):
        with pytest.raises(engine.KmcError) as e:
            engine.HostKinetics(p, _state(p, 0, bad))
        assert e.value.code == capi.ERR_STATE
        host = engine.HostKinetics(p, good)
        before = {k: getattr(host.arrays, k).copy() for k in ARRAYS}
        with pytest.raises(engine.KmcError) as e:
            host.update(_state(p, 3, bad))
        assert e.value.code == capi.ERR_STATE
        assert all(np.array_equal(getattr(host.arrays, k), before[k]) for k in ARRAYS) and host.acc.n_updates == 0
    L = engine.load_library()
    v = good.view()
    assert L.kmc_host_kin_begin(C.byref(p), C.byref(v), None, None, None) == capi.ERR_ARG


@pytest.fixture(scope="module")
def oracle_run():
    """DENSE, seed 23: 6000 steps of the oracle, then 600 with the dissociation rates raised to 5e-3, recorded
    by both recorders after every step and, in a second pair, after every 5 steps.  Everything is compared on the
    way; returns (params, the every-step Python recorder, the every-5 one)."""
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
    host1, rec1 = _both(p, st)
    host5, rec5 = _both(p, st)
    for k in range(1, 601):
        o.step(1, want_hashes=False)
        hs = o.get_state()
        assert hs.step == st.step + k
        out = host1.update(hs)
        rec1.update(hs)
        _same(host1, rec1, out)
        if k % 5 == 0:
            out = host5.update(hs)
            rec5.update(hs)
            _same(host5, rec5, out)
        if k % 100 == 0:
            _same_sample(host1, rec1)
            _same_sample(host5, rec5)
    return p, rec1, rec5


def test_oracle_trajectory_exercises_every_row(oracle_run):
    p, rec1, rec5 = oracle_run
    d, hist = rec1.sample()
    rows = hist.sum(axis=1)
    print("rows", rows.tolist(), {k: d[k] for k in EVENTS})
    assert rows[0] >= 30, "completed R-L lifetimes"
    assert rows[1] >= 5, "censored R-L bonds ended"
    assert rows[2] >= 15, "mono cis lifetimes"
    assert rows[3] >= 5, "complex cis lifetimes"
    assert rows[4] >= 5, "censored cis bonds ended"
    assert rows[5] >= 30, "rebinding to the same ligand"
    assert d["n_updates"] == 600 and rec5.out()["n_updates"] == 120
    # what every look counts: each ended bond once, each waiting time at most once per birth
    assert rows[0] + rows[1] == d["rl_off"] and rows[2] + rows[3] + rows[4] == d["cis_off_mono"] + d["cis_off_cx"]
    assert rows[5] + rows[6] <= d["rl_on"]
    assert rows[7] + d["n_rl_censored_alive"] == d["occ_rl"]
    assert rows[8] + d["n_cis_censored_alive"] == d["occ_mono"] + d["occ_cx"]
    # the stroboscopic recorder sees no more events than the exact one, and lifetimes in multiples of 5 only
    d5, hist5 = rec5.sample()
    assert d5["rl_off"] <= d["rl_off"] and d5["exp_rl"] > 0
    assert not hist5[:5, 1:5].any() and not hist5[:5, 6:10].any()


def test_rates_against_the_model(oracle_run):
    # statements about the reference's algorithm: one draw per step for an R-L bond, two for a cis bond (its
    # dissociation loop visits both partners), each with p = rate * time_step
    p, rec1, _ = oracle_run
    d = rec1.out()
    pr = FAST * p.time_step
    assert pr == 0.05
    p2 = 1.0 - (1.0 - pr) ** 2
    for name, off, exposure, prob in (("rl", d["rl_off"], d["exp_rl"], pr),
                                      ("mono", d["cis_off_mono"], d["exp_mono"], p2),
                                      ("complex", d["cis_off_cx"], d["exp_cx"], p2)):
        sd = math.sqrt(prob * (1.0 - prob) * exposure)
        print(name, off, exposure, "z = %.2f" % ((off - prob * exposure) / sd))
        assert abs(off - prob * exposure) <= 4.0 * sd, name


def test_kinetics_rates_and_survival():
    out = dict(rl_off=10, exp_rl=200, cis_off_mono=3, exp_mono=30, cis_off_cx=0, exp_cx=0, rl_on=5,
               exp_free_receptor=1000)
    hist = np.zeros((capi.KIN_HISTS, capi.KIN_BINS), dtype=np.int64)
    hist[5, 0], hist[5, 3], hist[6, 7] = 2, 1, 1
    r = analysis.kinetics_rates(out, 10.0, hist)
    assert r["rl_off"] == 0.05 and r["cis_off_mono"] == 0.1 and r["cis_off_cx"] == 0.0 and r["rl_on"] == 0.005
    assert r["rl_off_per_ns"] == 0.005 and r["cis_off_mono_per_ns"] == 0.01 and r["rl_on_per_ns"] == 0.0005
    assert r["rebinding_fraction"] == 0.75
    assert "rebinding_fraction" not in analysis.kinetics_rates(out, 10.0)
    assert analysis.kinetics_rates(out, 10.0, np.zeros_like(hist))["rebinding_fraction"] == 0.0
    ko = capi.KinOut()
    ko.rl_off, ko.exp_rl = 1, 4
    assert analysis.kinetics_rates(ko, 2.0)["rl_off_per_ns"] == 0.125
    # three bins by hand: at risk 5, 4, 1; one of five, then two of four end
    edges, S = analysis.lifetime_survival([1, 2, 0], [0, 1, 1])
    assert edges.tolist() == [0, 1, 2] and S.tolist() == [0.8, 0.4, 0.4]
    edges, S = analysis.lifetime_survival(np.zeros(capi.KIN_BINS), hist[5])
    assert np.array_equal(edges, analysis.kin_bin_edges()) and np.all(S == 1.0)  # all alive
    edges, S = analysis.lifetime_survival(hist[5], np.zeros(capi.KIN_BINS))
    assert S[0] == 1.0 - 2.0 / 3.0 and np.all(S[3:] == 0.0)
    with pytest.raises(ValueError):
        analysis.lifetime_survival([1, 2], [1, 2, 3])


def test_outputs_are_additive():
    p = params(n_a=4, n_b=2)
    host, rec = _both(p, _state(p, *SEQUENCE[0]))
    for step, links in SEQUENCE[1:]:
        host.update(_state(p, step, links))
    out, hist = host.sample()
    r = analysis.reduce_counts(hist)
    assert r.dtype == np.int64 and np.array_equal(r, hist) and r is not hist
    vec = np.array(list(out.as_dict().values()), dtype=np.int64)
    assert np.array_equal(analysis.reduce_counts(vec), vec)


def test_kin_struct_layouts_match_header(tmp_path):
    structs = {"kmc_kin_out": capi.KinOut, "kmc_kin_view": capi.KinView}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(REPO, "include", "kmc.h")}"',
             "int main(void){"]
    for st, cls in structs.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("bins %d\\nhists %d\\nbits %d\\n", KMC_KIN_BINS, KMC_KIN_HISTS, '
                 "KMC_KIN_RL_CENSORED | KMC_KIN_CIS_CENSORED << 4 | KMC_KIN_COMPLEX << 8);")
    lines.append("return 0;}")
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-O0", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True,
                                                 check=True).stdout.splitlines())
    for st, cls in structs.items():
        assert int(got[st]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"
    assert (int(got["bins"]), int(got["hists"])) == (capi.KIN_BINS, capi.KIN_HISTS)
    assert int(got["bits"]) == capi.KIN_RL_CENSORED | capi.KIN_CIS_CENSORED << 4 | capi.KIN_COMPLEX << 8
    assert len(capi.KIN_ROWS) == capi.KIN_HISTS
