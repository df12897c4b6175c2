"""Host side of the encounter layer: the sequential counterparts
kmc_host_reach_census / kmc_host_enc_* (engine.host_reach_census, engine.HostEnc)
against the plain-Python census and recorder of tests/_encounter.py, on a
trajectory of the CPU oracle and on a hand-made sequence of states whose rows
are worked out by hand; analysis.reach_factors / encounter_rates /
escape_probability.  Every comparison of the two sides is exact equality of
integers; each requires the Python side's margin (the smallest relative
distance of a compared value to its cutoff or bin edge) to exceed 1e-9.  No
device needed."""
import contextlib
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import _encounter as E
from _encounter import bind, place, unbind
from _kmc import DENSE, PKG, REPO, O, capi, engine, params

analysis = importlib.import_module(PKG + ".analysis")

FAST = 5e-3
SEED = 59  # an encounter is open after 6000 steps (CENSORED_ENDED >= 1): 2 of 48 seeds tried have one
MARGIN = 1e-9


@contextlib.contextmanager
def _slots_knob(n):
    old = os.environ.get("KMC_DEBUG_ENC_SLOTS")
    os.environ["KMC_DEBUG_ENC_SLOTS"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("KMC_DEBUG_ENC_SLOTS", None)
        else:
            os.environ["KMC_DEBUG_ENC_SLOTS"] = old


def _both(p, hs, every=1, slots=4):
    if slots != 4:
        with _slots_knob(slots):
            host = engine.HostEnc(p, hs, capi.enc_config(every))
    else:
        host = engine.HostEnc(p, hs, capi.enc_config(every))
    assert host.acc.slots == slots and host.acc.every == every
    return host, E.Recorder(p, hs, every, slots)


def _same(host, rec, out=None):
    assert E.same_arrays(host.arrays, rec), E.first_difference(host.arrays, rec)
    want = rec.out()
    got = (out if out is not None else host.acc).as_dict()
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert np.array_equal(host.hist, rec.hist)


def _same_sample(host, rec):
    s = host.sample()
    want, hist, react = rec.sample()
    assert s.as_dict() == want, {k: (s.as_dict()[k], want[k]) for k in want if s.as_dict()[k] != want[k]}
    assert np.array_equal(s.hist, hist) and np.array_equal(s.react_hist, react)
    return s


def _same_census(p, hs, nd=16, na=18):
    out, hd, harl, hacis = engine.host_reach_census(p, hs, nd, na)
    want, whd, wharl, whacis, margin = E.census(p, hs, nd, na)
    assert margin > MARGIN, margin
    assert out.as_dict() == want
    assert np.array_equal(hd, whd) and np.array_equal(harl, wharl) and np.array_equal(hacis, whacis)
    assert hd.sum(axis=(1, 2)).tolist() == want["n_reach"] and hd[:, 1].sum(axis=1).tolist() == want["n_reactive"]
    assert harl.sum() == want["n_reach"][0] and hacis.sum(axis=1).tolist() == want["n_reach"][1:]
    return out.as_dict()


@pytest.fixture(scope="module")
def oracle_states():
    """DENSE, seed SEED: 6000 steps of the oracle, then 600 with the dissociation rates raised to 5e-3.  Returns
    (params, the 601 states from step 6000 on)."""
    p0 = params(seed=SEED, **DENSE)
    o = O.Oracle(p0)
    o.init_placement()
    o.step(6000, want_hashes=False)
    st = o.get_state()
    fast = dict(DENSE)
    fast.update(diss_rate=FAST, cis_diss_rate=FAST, mono_cis_diss_rate=FAST)
    p = params(seed=SEED, **fast)
    o = O.Oracle(p)
    o.set_state(st)
    states = [st]
    for k in range(1, 601):
        o.step(1, want_hashes=False)
        states.append(o.get_state())
        assert states[-1].step == st.step + k
    return p, states


@pytest.fixture(scope="module")
def oracle_run(oracle_states):
    """Both recorders after every step and, in a second pair, after every 4 steps, compared on the way."""
    p, states = oracle_states
    host1, rec1 = _both(p, states[0])
    host4, rec4 = _both(p, states[0], every=4)
    _same(host1, rec1)
    _same_sample(host1, rec1)
    for k in range(1, 601):
        out = host1.update(states[k])
        rec1.update(states[k])
        _same(host1, rec1, out)
        if k % 4 == 0:
            out = host4.update(states[k])
            rec4.update(states[k])
            _same(host4, rec4, out)
        if k % 100 == 0:
            _same_sample(host1, rec1)
            _same_sample(host4, rec4)
    assert rec1.margin.value > MARGIN and rec4.margin.value > MARGIN
    return p, host1, rec1, host4, rec4


def test_oracle_trajectory_rows(oracle_run):
    p, host1, rec1, host4, rec4 = oracle_run
    d, hist, react = rec1.sample()
    rows = hist.sum(axis=1)
    print("rows", rows.tolist(), react.sum(axis=1).tolist(), d)
    # the counts this trajectory gives on the host are the floors
    assert rows[E.BOUND] >= 10 and rows[E.SEPARATED] >= 58 and rows[E.CENSORED_ENDED] >= 1
    assert rows[E.GEM_REBOUND] >= 90 and rows[E.GEM_ESCAPED] >= 48
    assert d["on_from_encounter"] >= 100 and d["on_direct"] >= 23
    assert d["n_updates"] == 600 and rec4.out()["n_updates"] == 150
    # each ended slot is filed once in a row and once in react_hist; the bound ones are the encounters' captures
    assert rows[:8].sum() == d["n_ended"] == react.sum()
    assert react[0].sum() == d["on_from_encounter"] == rows[E.BOUND] + rows[E.GEM_REBOUND]
    assert d["n_opened"] + rows[E.CENSORED_ENDED] + d["n_censored_alive"] == d["n_ended"] + d["occ_reach"]
    assert rows[E.ALIVE] + d["n_censored_alive"] == d["occ_reach"]
    assert d["exp_reactive"] <= d["exp_reach"] and d["exp_free_receptor"] <= 600 * p.n_a
    # the stroboscopic recorder: durations in multiples of 4 only
    d4, hist4, _ = rec4.sample()
    assert d4["on_from_encounter"] + d4["on_direct"] >= 1
    assert not hist4[:8, 1:4].any() and not hist4[:8, 5:8].any()


def test_update_rules(oracle_states):
    p, states = oracle_states
    host, rec = _both(p, states[0], every=4)
    with pytest.raises(engine.KmcError) as e:  # not due yet
        host.update(states[3])
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(engine.KmcError) as e:  # overdue
        host.update(states[5])
    assert e.value.code == capi.ERR_ARG
    out = host.update(states[4])
    rec.update(states[4])
    _same(host, rec, out)
    before = (rec.arrays(), rec.hist.copy(), rec.out())
    out = host.update(states[4])  # a second update at the same step moves only the count
    rec.update(states[4])
    _same(host, rec, out)
    after = rec.out()
    assert after.pop("n_updates") == before[2].pop("n_updates") + 1 and after == before[2]
    assert all(np.array_equal(rec.arrays()[k], before[0][k]) for k in E.ARRAYS) and np.array_equal(rec.hist, before[1])
    with pytest.raises(engine.KmcError) as e:
        engine.HostEnc(p, states[0], capi.enc_config(0))
    assert e.value.code == capi.ERR_ARG
    L = engine.load_library()
    v = states[0].view()
    assert L.kmc_host_enc_begin(C.byref(p), C.byref(v), None, None, None, None) == capi.ERR_ARG
    assert L.kmc_host_reach_census(C.byref(p), C.byref(v), 16, 18, None, None, None, None) == capi.ERR_ARG
    out = capi.ReachOut()
    assert L.kmc_host_reach_census(C.byref(p), C.byref(v), 16, 18, C.byref(out), None, None, None) == capi.KMC_OK
    for nd, na in ((0, 18), (65, 18), (16, 0), (16, 37)):
        assert L.kmc_host_reach_census(C.byref(p), C.byref(v), nd, na, C.byref(out), None, None, None) == capi.ERR_ARG
    bad = states[0].copy()
    bad.a_int[2, 0], bad.a_int[3, 0] = p.n_a + 1, 1  # a bond at site 1
    with pytest.raises(engine.KmcError) as e:
        engine.HostEnc(p, bad)
    assert e.value.code == capi.ERR_STATE


def test_slots_knob_on_the_trajectory(oracle_states):
    p, states = oracle_states
    host, rec = _both(p, states[0], slots=1)
    for k in range(1, 201):
        out = host.update(states[k])
        rec.update(states[k])
        _same(host, rec, out)
    _same_sample(host, rec)
    assert not host.arrays.key[:, 1:].any()


def test_census_on_the_trajectory(oracle_states):
    # a bond holds its two sites 9 A apart, and a pair whose bond has just ended is still there: d2 within an ulp
    # of 81, edge 8 of 16 over the 18 A cutoff.  So nd = 15 serves at every state, and nd = 16 and 64 at states
    # that hold R-L pairs in reach but none of these (the margin is required at each)
    p, states = oracle_states
    total = np.zeros(3, dtype=np.int64)
    reactive = np.zeros(3, dtype=np.int64)
    for k in range(0, 601, 25):
        d = _same_census(p, states[k], 15, 18)
        total += d["n_reach"]
        reactive += d["n_reactive"]
        assert d["rl_receptors_in_reach"] <= d["n_reach"][0] and d["rl_sites_in_reach"] <= d["n_reach"][0]
        assert d["rl_free_receptors"] == np.count_nonzero(states[k].a_int[0] == 0)
    print("census", total.tolist(), reactive.tolist())
    assert total.tolist() == [13, 46, 7] and reactive.tolist() == [11, 10, 2]  # (what this trajectory gives)
    for k in (0, 75, 350, 375):
        assert _same_census(p, states[k], 16, 18)["n_reach"][0] + (k == 75) >= 1
        _same_census(p, states[k], 64, 36)
    _same_census(p, states[0], 1, 1)
    _same_census(p, states[300], 7, 5)


# ---------------------------------------------------------------- a hand-made sequence
def hand_made_states(p, base):
    """Seven states from `base` (a random placement: no bonds, nothing in reach): receptor R meets
    three sites, loses one to receptor R2, binds the second (the third is lost with it), unbinds (a geminate and a
    new encounter open), then loses the geminate site to receptor R3.  R, R2, R3 = receptors 1, 2, 3; the sites are
    (ligand 1, 2), (ligand 2, 3), (ligand 3, 4): keys 4, 9, 14."""
    s = base.copy()
    assert not s.a_int.any() and not s.b_int.any()
    far = E.census(p, s, 1, 1)[0]
    assert far["n_reach"][0] == 0, "the base state has R-L pairs in reach: choose another base"
    t0 = s.step
    seq = [s]

    def nxt():
        n = seq[-1].copy()
        n.step = seq[-1].step + 1
        seq.append(n)
        return n

    n = nxt()  # t0 + 1: the three sites come into reach
    place(n, 0, 0, 2, (3.0, 2.0, 1.0))
    place(n, 0, 1, 3, (-4.0, 1.0, 2.0))
    place(n, 0, 2, 4, (1.0, -5.0, 3.0))
    n = nxt()  # t0 + 2: R2 takes (ligand 1, 2)
    bind(n, 1, 0, 2)
    n = nxt()  # t0 + 3: R binds (ligand 2, 3)
    bind(n, 0, 1, 3)
    n = nxt()  # t0 + 4: the bond ends; both sites are still in reach
    unbind(n, 0, 1, 3)
    n = nxt()  # t0 + 5: R3 takes (ligand 2, 3)
    bind(n, 2, 1, 3)
    n = nxt()  # t0 + 6: the last site leaves
    place(n, 0, 2, 4, (100.0, 0.0, 0.0))
    assert seq[-1].step == t0 + 6
    return seq


@pytest.mark.parametrize("slots", [4, 1])
def test_hand_made_sequence(slots):
    p = params(seed=SEED, **DENSE)
    seq = hand_made_states(p, engine.host_init_random(p))
    host, rec = _both(p, seq[0], slots=slots)
    for hs in seq[1:]:
        out = host.update(hs)
        rec.update(hs)
        _same(host, rec, out)
        _same_census(p, hs)
    s = _same_sample(host, rec)
    assert rec.margin.value > MARGIN
    rows, d = s.hist.sum(axis=1).tolist(), s.as_dict()
    t0 = seq[0].step
    if slots == 4:
        # opened: three at t0 + 1, two at t0 + 4; ended: LOST_SITE 1 (after 1 step), BOUND 1 (2 steps) with
        # LOST_RECEPTOR 1 (2 steps), GEM_LOST 1 (1 step), SEPARATED 1 (2 steps)
        assert rows == [1, 1, 1, 1, 0, 0, 0, 1, 0]
        assert s.hist[E.LOST_SITE, 1] == 1 and s.hist[E.BOUND, 2] == 1 and s.hist[E.LOST_RECEPTOR, 2] == 1
        assert s.hist[E.GEM_LOST, 1] == 1 and s.hist[E.SEPARATED, 2] == 1
        assert (d["n_opened"], d["n_ended"], d["n_overflow"]) == (5, 5, 0)
        assert (d["on_from_encounter"], d["on_direct"]) == (1, 2)  # R from its encounter; R2 and R3 directly
        # slot-steps: 3 + 2 + 0 + 2 + 1; free receptors: n_a, n_a, n_a - 1, n_a - 2, n_a - 1, n_a - 2
        assert d["exp_reach"] == 8 and d["exp_free_receptor"] == 6 * p.n_a - 6
    else:
        # one slot: the smallest key is kept, the others are cut at every look they are in reach
        assert d["n_overflow"] == 2 + 1 + 0 + 1 + 0 + 0 and d["n_overflow"] >= 1
        # t0 + 1 opens key 4; t0 + 2: key 4 LOST_SITE, key 9 opens; t0 + 3: key 9 BOUND; t0 + 4: key 9 opens
        # geminate; t0 + 5: key 9 GEM_LOST, key 14 opens; t0 + 6: key 14 SEPARATED
        assert rows == [1, 1, 0, 1, 0, 0, 0, 1, 0]
        assert not host.arrays.key[:, 1:].any()
    assert host.arrays.key.any() == False  # noqa: E712  (every encounter has ended)
    # the kept slot is the smallest key: replay the looks with four slots and compare
    full, _ = _both(p, seq[0])
    one, _ = _both(p, seq[0], slots=1)
    for hs in seq[1:]:
        full.update(hs)
        one.update(hs)
        assert np.array_equal(one.arrays.key[:, 0], full.arrays.key[:, 0])
        assert t0 < hs.step


# ---------------------------------------------------------------- post-processing
def test_analysis_functions():
    out = capi.ReachOut()
    out.n_reach[:] = [10, 4, 0]
    out.n_reactive[:] = [5, 1, 0]
    hd = np.zeros((3, 2, 4), dtype=np.int64)
    hd[0, 0] = [0, 1, 2, 2]
    hd[0, 1] = [1, 1, 1, 2]
    r = analysis.reach_factors(out, hd, (18.0, 15.0))
    assert r["orientation_factor"].tolist() == [0.5, 0.25, 0.0]
    assert r["r"].shape == (3, 4) and r["r"][0].tolist() == [2.25, 6.75, 11.25, 15.75] and r["r"][1, 0] == 1.875
    assert r["profile"][0].tolist() == [1, 2, 3, 4] and r["reactive_share"][0].tolist() == [1.0, 0.5, 1 / 3, 0.5]
    d = dict(on_from_encounter=6, on_direct=2, n_opened=20, n_ended=18, exp_reach=60, exp_reactive=30,
             exp_free_receptor=1000)
    e = analysis.encounter_rates(d, 8.0, ass_rate=0.025)
    assert e["encounter_rate"] == 0.02 and e["encounter_rate_per_ns"] == 0.0025 and e["mean_dwell"] == 3.0
    assert e["capture_probability"] == 0.3 and e["on_per_reactive_step"] == 0.2 and e["model_probability"] == 0.2
    assert e["direct_share"] == 0.25
    assert analysis.encounter_rates(dict.fromkeys(d, 0), 10.0)["mean_dwell"] == 0.0
    hist = np.zeros((capi.ENC_HISTS, capi.ENC_BINS), dtype=np.int64)
    hist[E.GEM_REBOUND, 1], hist[E.GEM_ESCAPED, 2], hist[E.GEM_LOST, 2] = 2, 1, 1
    g = analysis.escape_probability(hist)
    assert g["escape_probability"] == 0.25 and g["rebinding_probability"] == 0.5
    assert g["survival"][:3].tolist() == [1.0, 0.5, 0.0] and g["edges"][:3].tolist() == [0, 1, 2]
    assert analysis.escape_probability(np.zeros_like(hist))["escape_probability"] == 0.0


def test_outputs_are_additive(oracle_run):
    _, host1, _, _, _ = oracle_run
    s = host1.sample()
    v = s.counts()
    assert v.dtype == np.int64 and np.array_equal(analysis.reduce_counts(v), v)
    back = capi.EncSample.from_counts(v + v)
    assert np.array_equal(back.hist, 2 * s.hist) and back.out.n_opened == 2 * s.out.n_opened
    assert np.array_equal(back.react_hist, 2 * s.react_hist)


def test_enc_struct_layouts_match_header(tmp_path):
    structs = {"kmc_enc_out": capi.EncOut, "kmc_enc_view": capi.EncView, "kmc_enc_config": capi.EncConfig,
               "kmc_reach_out": capi.ReachOut}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(REPO, "include", "kmc.h")}"',
             "int main(void){"]
    for st, cls in structs.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, *_ in cls._fields_]
    lines.append('printf("consts %d %d %d %d %d %d\\n", KMC_ENC_SLOTS, KMC_ENC_BINS, KMC_ENC_HISTS, KMC_REACH_MAX_ND, '
                 "KMC_REACH_MAX_NA, KMC_ENC_CENSORED | KMC_ENC_GEMINATE << 4 | KMC_ENC_REACTIVE << 8 | "
                 "KMC_ENC_WAS_REACTIVE << 12);")
    lines.append("return 0;}")
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-O0", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True,
                                                                check=True).stdout.splitlines()}
    for st, cls in structs.items():
        assert int(got[st][0]) == C.sizeof(cls)
        for f, *_ in cls._fields_:
            assert int(got[f"{st}.{f}"][0]) == getattr(cls, f).offset, f"{st}.{f}"
    assert [int(x) for x in got["consts"]] == [
        capi.ENC_SLOTS, capi.ENC_BINS, capi.ENC_HISTS, capi.REACH_MAX_ND, capi.REACH_MAX_NA,
        capi.ENC_CENSORED | capi.ENC_GEMINATE << 4 | capi.ENC_REACTIVE << 8 | capi.ENC_WAS_REACTIVE << 12]
    assert len(capi.ENC_ROWS) == capi.ENC_HISTS
