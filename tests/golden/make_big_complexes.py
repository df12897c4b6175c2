"""Generate tests/golden/big_complexes.npz: exact states at which the step
engine's complex chain changes code path, made by the keyed
CPU oracle alone (cell-list mode), no GPU.

  S16  150 + 50 proteins, _kmc.DENSE with ass_rate = 0.09 and every
       dissociation rate 0, seed 12, the keyed placement advanced until the
       complexes include sizes 15, 16 and 17 or more at once (checked every
       1000 steps; this build: step 161 000, sizes 17, 17, 16, 15).  CXL = 16
       is the last size of the streamed path, 17 the first of the
       global-memory path.
       Continued at the raised dissociation rates (_scale.FAST) its first
       300 steps hold complexes of 17 or more that lose a bond and leave
       pieces of 16 or fewer, and merges from 16 or fewer to 17 or more.
       The state is jammed: both complexes of 17, and every other but one of
       11, collide on every step.
  S17  hand-linked like S32 below, among 60 free receptors and 12 free
       ligands: three rings of four ligands and eight receptors with 3 and 4
       single receptors and with a pendant ligand and 2, so 15, 16 and 17
       members.  A ring of four does not come to rest: each is re-aligned on
       every step, and in 200 steps each size is both rejected and accepted
       with changed beads (seed 4: 79 / 121, 78 / 122, 176 / 24).
  S32  a hand-linked network in a 3000 x 3000 x 250 box among 60 free
       receptors and 21 free ligands: a chain of ten ligands (out at sites 2
       and 4 in turn, in at site 3) with 22 receptors, exactly 32 members — the
       last size that fits bfs_one's queue —, and a ring of six ligands (out at
       site 2, in at site 3) with three pendant ligands, 33 members — the first
       on the overflow list.  No rate of the stored parameters lets a reaction
       change a complex.
  S64  likewise among 60 and 16: a ring of six with two shells of pendants, 24
       ligands and 48 receptors, 72 members.

Evolution alone does not reach 33 members at a size that can be committed: with
150 + 50 up to 600 + 200 proteins at the dense density and up to twice it,
every association rate at 0.9 / time_step and time steps of 10 to 400 ns, the
largest complex stays between 18 and 26 once the free units are used up
(complexes of several ligands do not diffuse).  Hence the hand-linked networks,
grown one link at a time with the oracle stepping in between (network()).  At
the raised dissociation rates S32's 33 falls below 33, and complexes fall below
and merge past 17 (asserted before anything is written).

Stored per state: ra, rb, a_int, b_int, counters, step and the parameters
(JSON of the default_params overrides); for S16 the hashes of its next 50
oracle steps.  The archive is written with fixed timestamps, so a rerun gives
a byte-identical file.  Run time: about a minute on one core, nearly all of it S16's evolution.

Usage: python tests/golden/make_big_complexes.py [out]
"""
from __future__ import annotations

import io
import json
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, _p)

import _complex as CX  # noqa: E402
from _bondorder import bind_network  # noqa: E402
from _kmc import DENSE, O, capi, engine, params  # noqa: E402
from _rings import cycle, ref_rings  # noqa: E402
from _scale import FAST  # noqa: E402

OUT = os.path.join(HERE, "big_complexes.npz")
STAGE_STEPS, QUIET = 300, 5
NO_DISS = dict(diss_rate=0.0, cis_diss_rate=0.0, mono_cis_diss_rate=0.0)
# test_large_complex_breaks_and_merges' parameters over a state's own
FAST_KW = dict(ass_rate=0.09, cis_ass_rate=DENSE["cis_ass_rate"], mono_cis_ass_rate=DENSE["mono_cis_ass_rate"],
               diss_rate=FAST, cis_diss_rate=FAST, mono_cis_diss_rate=FAST)
S16_KW = dict(seed=12, **{**DENSE, "ass_rate": 0.09, **NO_DISS})
RATES = {k: v for k, v in DENSE.items() if not k.startswith("box_")}
NET_KW = dict(box_z=250.0, **{**RATES, "ass_rate": 0.0, "cis_ass_rate": 0.0, "mono_cis_ass_rate": 0.09,
                              "diss_rate": 0.0, "cis_diss_rate": 0.0})


def oracle(p, hs=None):
    o = O.Oracle(p, rng_mode=O.RNG_KEYED, nbmode=O.NB_CELLS)
    if hs is None:
        o.init_placement()
    else:
        o.set_state(hs)
    return o


def s16_holds(s):
    return 15 in s and 16 in s and s[0] >= 17


def make_s16():
    o = oracle(params(**S16_KW))
    for _ in range(400):
        o.step(1000, want_hashes=False)
        hs = o.get_state()
        if s16_holds(CX.sizes(hs)):
            return hs
    raise SystemExit("S16: the sizes 15, 16 and 17 or more never occurred at once")


def fast_events(kw, hs, limit, steps=300):
    """(breaks, merges) across `limit` (_complex.break_and_merge) of `steps` oracle steps at the FAST dissociation
    rates and the dense association rates."""
    o = oracle(params(**{**kw, **FAST_KW}), hs)
    prev, broke, merged = hs, 0, 0
    for _ in range(steps):
        o.step(1, want_hashes=False)
        cur = o.get_state()
        b, m = CX.break_and_merge(prev, cur, limit)
        broke, merged, prev = broke + b, merged + m, cur
    return broke, merged


# ---------------------------------------------------------------- hand-linked networks
def straight(first, n):
    """Bridges of a chain of n ligands that runs straight: in at site 3, out at sites 2 and 4 in turn."""
    return [(first + i, 2 if i % 2 == 0 else 4, first + i + 1, 3) for i in range(n - 1)]


def network(seed, n_free_a, n_free_b, box, stages):
    """(params kwargs, state): the keyed placement of the box, no rate but the free receptors' cis rates, with the
    bridges and single receptors of `stages` linked by hand, one stage at a time as a complex grows: each stage is
    (edges, single) with edges (b, s, b2, s2: a bridge ligand b site s - receptor = receptor - ligand b2 site s2) and
    single (b, s: one receptor at ligand b's site s).  After each stage the oracle steps until the alignment has
    nothing to snap for QUIET steps, at most STAGE_STEPS steps (linked all at once, the scattered members are
    snapped onto each other, overlap, and the complex is rejected on every step).  Ligands and receptors are
    taken in a seeded random order."""
    n_lig = 1 + max(max(e[0], e[2]) for ed, _ in stages for e in ed)
    n_rec = sum(2 * len(ed) + len(si) for ed, si in stages)
    kw = dict(seed=seed, n_a=n_rec + n_free_a, n_b=n_lig + n_free_b, box_x=box, box_y=box, **NET_KW)
    p = params(**{**kw, "mono_cis_ass_rate": 0.0})  # (no free receptor pairs up before it is linked)
    hs = engine.host_init_random(p)
    hs.a_int[:] = 0
    hs.b_int[:] = 0
    hs.counters[:] = 0
    rng = np.random.default_rng(seed)
    rec = rng.permutation(p.n_a).tolist()
    lig = rng.permutation(p.n_b).tolist()
    for edges, single in stages:
        bind_network(hs, [(lig[b], s, rec.pop(), rec.pop(), lig[b2], s2) for b, s, b2, s2 in edges])
        for b, s in single:
            r = rec.pop()
            hs.a_int[0, r] = 1
            hs.a_int[2, r] = p.n_a + lig[b] + 1
            hs.a_int[3, r] = s
            hs.b_int[s - 1, lig[b]] = 1
            hs.b_int[4 + s - 1, lig[b]] = r + 1
        hs.counters[1] = int(np.count_nonzero(hs.a_int[2]))       # bond_num_rl
        hs.counters[2] = int(np.count_nonzero(hs.a_int[4])) // 2  # bond_num_cis (every pair here has a ligand)
        hs.counters[0] = hs.counters[1] + hs.counters[2]          # bond_num
        assert engine.host_validate(p, hs) == capi.KMC_OK
        o = oracle(p, hs)
        quiet, n, prev = 0, 0, o.stats()
        while n < STAGE_STEPS and quiet < QUIET:
            o.step(1, want_hashes=False)
            n += 1
            cur = o.stats()
            snaps = cur["snap_bond"] + cur["snap_cis"] - prev["snap_bond"] - prev["snap_cis"]
            quiet, prev = (quiet + 1 if snaps == 0 else 0), cur
        hs = o.get_state()
    assert engine.host_validate(params(**kw), hs) == capi.KMC_OK
    return kw, hs


def one_by_one(edges=(), single=()):
    return [([e], []) for e in edges] + [([], [s]) for s in single]


def make_s32():
    # ligands 0..9: the chain, 10 + 18 + 4 = 32; 10..15: the ring, 16..18: pendants at ring sites 4, 18 + 9 + 6 = 33
    stages = one_by_one(straight(0, 10), [(0, 3), (0, 4), (9, 2), (5, 2)])
    stages += one_by_one(cycle(6, 10) + [(10, 4, 16, 2), (12, 4, 17, 2), (14, 4, 18, 2)],
                         [(16, 3), (16, 4), (17, 3), (17, 4), (18, 3), (18, 4)])
    return network(5, 60, 21, 3000.0, stages)


def make_s17():
    # three rings of four ligands and eight receptors: with three single receptors 15 members, with four 16, with a
    # pendant ligand and two 17.  A ring of four cannot close at rest: its complex is re-aligned on every step, some
    # proposals collide and some are committed (the seed is one at which all three sizes do both)
    stages = one_by_one(cycle(4, 0), [(0, 4), (1, 4), (2, 4)])
    stages += one_by_one(cycle(4, 4), [(4, 4), (5, 4), (6, 4), (7, 4)])
    stages += one_by_one(cycle(4, 8) + [(8, 4, 12, 2)], [(9, 4), (12, 3)])
    return network(4, 60, 12, 3000.0, stages)


def outcomes(kw, hs, steps=200):
    """(rejected, accepted) by member count of the complexes' collision tests over `steps` oracle steps."""
    o = oracle(params(**kw), hs)
    o.step(steps, want_hashes=False)
    return o.complex_outcomes()


def make_s64():
    # the ring 0..5, a pendant 6..11 at every ring site 4, two more 12..23 at every pendant: 24 ligands, 24 bridges
    edges = cycle(6) + [(i, 4, 6 + i, 2) for i in range(6)]
    edges += [(6 + i, s, 12 + 2 * i + (s - 3), 2) for i in range(6) for s in (3, 4)]
    return network(7, 60, 16, 3000.0, one_by_one(edges))


# ---------------------------------------------------------------- the archive
def npy_bytes(a) -> bytes:
    b = io.BytesIO()
    np.lib.format.write_array(b, np.asanyarray(a), allow_pickle=False)
    return b.getvalue()


def write_npz(path, arrays: dict):
    """np.load-compatible, with fixed timestamps: the same arrays give the same bytes."""
    tmp = path + ".tmp"
    with zipfile.ZipFile(tmp, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, npy_bytes(arrays[k]), compresslevel=9)
    os.replace(tmp, path)


def put(arrays, name, kw, hs):
    for f in ("ra", "rb", "a_int", "b_int", "counters"):
        arrays[f"{name}_{f}"] = getattr(hs, f)
    arrays[name + "_step"] = np.int64(hs.step)
    arrays[name + "_params"] = np.array(json.dumps(kw, sort_keys=True))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    t0 = time.time()
    arrays, states = {}, {}
    s16 = make_s16()
    states["S16"] = (S16_KW, s16)
    print(f"S16 step {s16.step} sizes {CX.sizes(s16)[:6]} {time.time() - t0:.0f}s", flush=True)
    states["S17"] = make_s17()
    states["S32"] = make_s32()
    states["S64"] = make_s64()
    for name in ("S17", "S32", "S64"):
        print(name, "sizes", CX.sizes(states[name][1])[:6], f"{time.time() - t0:.0f}s", flush=True)

    # the sizes each state is there for, before anything is written
    s = CX.sizes(s16)
    assert s16_holds(s), s
    ev = {name: (fast_events(*states[name], CX.CXL), fast_events(*states[name], CX.BFS_QCAP)) for name in states}
    print("breaks and merges across 16 | 17 and 32 | 33 at the FAST rates:", ev, flush=True)
    assert min(ev["S16"][0]) > 0 and min(ev["S32"][0]) > 0 and ev["S32"][1][0] > 0, ev
    assert CX.sizes(states["S17"][1]) == [17, 16, 15]
    rej, acc = outcomes(*states["S17"])
    print("S17: rejected", rej[15:18], "accepted", acc[15:18], "in 200 steps", flush=True)
    assert rej[15:18].min() > 0 and acc[15:18].min() > 0
    rej, acc = outcomes(*states["S16"])
    assert rej[17] == 400 and acc[17] == 0, (rej[17], acc[17])  # the jam: both complexes of 17 rejected on every step
    s = CX.sizes(states["S32"][1])
    assert s.count(CX.BFS_QCAP) == 1 and s[0] == CX.BFS_QCAP + 1 and CX.ligands_of_largest(states["S32"][1]) >= 2, s
    s = CX.sizes(states["S64"][1])
    assert s[0] > 64 and CX.ligands_of_largest(states["S64"][1]) >= 2, s
    for name in ("S32", "S64"):  # the ring of six
        assert ref_rings(states[name][1], 6)[0][0, 6] == 1
    for name in ("S17", "S32", "S64"):  # the networks keep their sizes through a test window (no rate can change them)
        kw, hs = states[name]
        o = oracle(params(**kw), hs)
        o.step(400, want_hashes=False)
        assert CX.sizes(o.get_state()) == CX.sizes(hs), name

    for name, (kw, hs) in states.items():
        put(arrays, name, kw, hs)
    arrays["names"] = np.array(json.dumps(list(states)))
    o = oracle(params(**S16_KW), s16)
    arrays["S16_hashes50"] = o.step(50)[1]
    write_npz(out, arrays)
    print("wrote", out, os.path.getsize(out), "bytes", f"{time.time() - t0:.0f}s")


if __name__ == "__main__":
    main()
