"""Host side of the displacement tracking: the numpy tracker
that the GPU tests compare against (tests/_dynamics.py) on a hand-made
trajectory with known true displacements, and analysis.msd / diffusion_fit /
reduce_sums.  No device needed."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from _dynamics import Tracker, bits, tree_sum
from _kmc import PKG, REPO, capi, params

analysis = importlib.import_module(PKG + ".analysis")

BOX_X, BOX_Y = 64.0, 32.0  # powers of two: every wrap below is exact in binary


def _state(p, true_xy, step):
    """A host state whose bead [1][1] positions are the true ones wrapped into the box."""
    hs = capi.HostState(p.n_a, p.n_b)
    w = true_xy.copy()
    w[:, 0] -= BOX_X * np.floor(w[:, 0] / BOX_X + 0.5)
    w[:, 1] -= BOX_Y * np.floor(w[:, 1] / BOX_Y + 0.5)
    assert np.all(np.abs(w[:, 0]) <= BOX_X / 2) and np.all(np.abs(w[:, 1]) <= BOX_Y / 2)
    hs.ra[0], hs.ra[1] = w[:p.n_a, 0], w[:p.n_a, 1]
    hs.rb[0], hs.rb[1] = w[p.n_a:, 0], w[p.n_a:, 1]
    hs.step = step
    return hs


def test_tracker_recovers_true_displacements_across_every_edge():
    # five points with constant dyadic velocities: +x, −x, +y, −y and a diagonal;
    # 40 steps carry each of them across its box edge several times
    p = params(n_a=3, n_b=2, box_x=BOX_X, box_y=BOX_Y, box_z=100.0)
    start = np.array([[1.5, -3.25], [-20.0, 7.5], [30.75, 15.0], [0.125, -15.5], [31.5, 15.75]])
    vel = np.array([[9.75, 0.0], [-7.5, 0.0], [0.0, 5.25], [0.0, -6.125], [11.375, -4.625]])
    trk = Tracker(p, _state(p, start, 0))
    crossings = np.zeros(2, dtype=int)
    for t in range(1, 41):
        true = start + vel * t
        hs = _state(p, true, t)
        info = trk.update(hs)
        assert np.array_equal(bits(trk.u), bits(true - start)), t
        assert info["n_updates"] == t and info["last_step"] == t and info["origin_step"] == 0
    for c, box in ((0, BOX_X), (1, BOX_Y)):
        crossings[c] = np.abs(np.floor((start[:, c] + vel[:, c] * 40) / box + 0.5)).sum()
    assert trk.n_wraps == crossings.sum() and crossings[0] >= 6 and crossings[1] >= 6
    assert (info["max_dx"], info["max_dy"]) == (11.375, 6.125)
    assert info["n_jumped"] == 2 and info["n_changed"] == 0  # |d| >= 8 = min(box) / 4: points 0 and 4
    out, vh = trk.sample(hs, 512.0, 8)
    q = ((vel * 40) ** 2).sum(axis=1)
    assert np.array_equal(out["n"], [3, 0, 0, 2, 0]) and np.array_equal(out["n_clean"], [2, 0, 0, 1, 0])
    assert out["sum_u2"][0] == q[0] + q[1] + q[2] and out["sum_u2"][3] == q[3] + q[4]
    assert out["sum_u2_clean"][0] == q[1] + q[2] and out["sum_u2_clean"][3] == q[3]
    want = np.zeros((5, 8), dtype=np.int64)
    for c, i in ((0, 1), (0, 2), (3, 3)):
        want[c, int(np.sqrt(q[i]) // 64.0)] += 1
    assert np.array_equal(vh, want) and vh.sum() == 3
    assert [out[k] for k in ("rl0", "rl_now", "rl_kept", "cis0", "cis_now", "cis_kept")] == [0] * 6
    # a second update at the same step adds nothing
    trk.update(hs)
    assert np.array_equal(bits(trk.u), bits(true - start))


def test_tracker_flags_and_survival():
    # receptors 1-2 cis-bound, receptor 3 bound to ligand 4's site 2; then the cis bond breaks
    p = params(n_a=3, n_b=2, box_x=BOX_X, box_y=BOX_Y, box_z=100.0)
    xy = np.zeros((5, 2))
    hs0 = _state(p, xy, 10)
    hs0.a_int[4, 0], hs0.a_int[4, 1] = 2, 1
    hs0.a_int[2, 2], hs0.a_int[3, 2] = 4, 2
    hs0.b_int[5, 0] = 3
    trk = Tracker(p, hs0)
    assert np.array_equal(trk.cls, [1, 1, 2, 4, 3])
    hs1 = hs0.copy()
    hs1.step = 11
    hs1.a_int[4, 0] = hs1.a_int[4, 1] = 0
    info = trk.update(hs1)
    assert info["n_changed"] == 2 and np.array_equal(trk.flags, [1, 1, 0, 0, 0])
    # the bond re-forms: "now" recovers, "kept" does not
    hs2 = hs0.copy()
    hs2.step = 12
    trk.update(hs2)
    out, _ = trk.sample(hs2, 10.0, 4)
    assert (out["rl0"], out["rl_now"], out["rl_kept"]) == (1, 1, 1)
    assert (out["cis0"], out["cis_now"], out["cis_kept"]) == (1, 1, 0)
    assert np.array_equal(out["n"], [0, 2, 1, 1, 1]) and np.array_equal(out["n_clean"], [0, 0, 1, 1, 1])


def test_tree_sum_is_the_halving_tree():
    rng = np.random.default_rng(3)
    v = rng.random(256 * 3 + 17) * 1e3
    blocks = np.concatenate([v, np.zeros(256 * 4 - v.size)]).reshape(4, 256)

    def halve(t):
        t = list(t)
        h = 128
        while h >= 1:
            for j in range(h):
                t[j] = t[j] + t[j + h]
            h //= 2
        return t[0]

    top = [halve(b) for b in blocks] + [0.0] * 252
    assert bits([tree_sum(v)])[0] == bits([halve(top)])[0]
    assert tree_sum(np.zeros(0)) == 0.0 and tree_sum([2.5]) == 2.5


def test_msd_and_diffusion_fit():
    s = capi.TrackSample()
    for c, (n, nc, su, sc) in enumerate([(4, 2, 10.0, 3.0), (0, 0, 0.0, 0.0), (5, 0, 7.5, 0.0), (1, 1, 2.0, 2.0),
                                         (2, 2, 9.0, 9.0)]):
        s.n[c], s.n_clean[c], s.sum_u2[c], s.sum_u2_clean[c] = n, nc, su, sc
    assert np.array_equal(analysis.msd(s), [1.5, 0.0, 0.0, 2.0, 4.5])
    assert np.array_equal(analysis.msd(s, clean=False), [2.5, 0.0, 1.5, 2.0, 4.5])
    assert np.array_equal(analysis.msd(s.as_dict()), analysis.msd(s))
    t = np.array([10.0, 20.0, 30.0, 40.0])
    assert analysis.diffusion_fit(t, 4 * 0.75 * t + 3.0) == pytest.approx(0.75, rel=1e-14)
    assert analysis.diffusion_fit(t, np.full(4, 2.0)) == 0.0
    for bad in ((t, t[:3]), ([1.0], [1.0]), ([2.0, 2.0], [1.0, 3.0])):
        with pytest.raises(ValueError):
            analysis.diffusion_fit(*bad)


def test_track_struct_layouts_match_header(tmp_path):
    structs = {"kmc_track_info": capi.TrackInfo, "kmc_track_sample_t": capi.TrackSample}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(REPO, "include", "kmc.h")}"',
             "int main(void){"]
    for st, cls in structs.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("classes %d\\nbins %d\\nbits %d\\n", KMC_TRACK_CLASSES, KMC_TRACK_MAX_BINS, '
                 "KMC_TRACK_CHANGED | KMC_TRACK_JUMPED << 4);")
    lines.append("return 0;}")
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-O0", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    out = subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True, check=True).stdout
    got = dict(l.split() for l in out.splitlines())
    for st, cls in structs.items():
        assert int(got[st]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"
    assert (int(got["classes"]), int(got["bins"])) == (capi.TRACK_CLASSES, capi.TRACK_MAX_BINS)
    assert int(got["bits"]) == capi.TRACK_CHANGED | capi.TRACK_JUMPED << 4


def test_reduce_sums_without_process_group():
    a = np.array([[0.1, 2.5e300], [-3.0, 0.0]])
    r = analysis.reduce_sums(a)
    assert r.dtype == np.float64 and np.array_equal(bits(r), bits(a))
    assert r is not a
