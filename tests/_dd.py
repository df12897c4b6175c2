"""Shared by the slab tests (test_slabs.py, test_gpu_slabs.py, test_gpu_dd.py):
the scenarios, the whole-box oracle they are compared with, and the G windows
of one global state set on a *family* of handles — engine.Simulation on the
device, or keyed oracle windows (oracle_dd_*, the sequential restatement that
is the reference of every comparison) — with the rows moved as the driver
moves them.

The windows are built by the driver's own code (SlabRank.start: make_plan,
window_state, ctl5, the send / receive ids in its order), so that the two
families hold exactly what a decomposed run holds; only the per-step protocol
is spelt out here (lockstep), one entry point at a time.
"""
import functools
import importlib

import numpy as np
# before libkmc.so is loaded (the first engine call): a ROCm build of torch
# brings its own HIP runtime, which finds no device once another copy has
# been initialised in the process; loaded first, it serves libkmc.so as well
import torch

from _kmc import DENSE, PKG, O, engine, params

slabs = importlib.import_module(PKG + ".slabs")
capi = importlib.import_module(PKG + ".capi")

ROW = capi.DD_ROW
RATES = {k: v for k, v in DENSE.items() if not k.startswith("box")}
REPORT_FIELDS = ("bad", "differed", "links", "n_jump", "n_xb", "xcol", "xbond")


class OracleWindow(O.Oracle):
    """An oracle over one slab's window (cell-list mode)."""

    def __init__(self, q):
        super().__init__(q, rng_mode=O.RNG_KEYED, nbmode=O.NB_CELLS)

    def step(self, n):
        return super().step(n, want_hashes=False)[0]  # the records, as engine.Simulation.step

    def close(self):
        pass


def scenario(n_a=4000, n_b=1500, L=6000.0, seed=9):
    p = params(n_a=n_a, n_b=n_b, seed=seed, box_x=L, box_y=L, box_z=250.0, **RATES)
    return p, engine.host_init_random(p)


def whole_box(p, st, steps):
    o = O.Oracle(p, nbmode=O.NB_CELLS)
    o.set_state(st)
    return o.step(steps)


@functools.lru_cache(maxsize=None)
def whole_box_small(steps):
    """(params, state, records, hashes) of the recovery tests' scenario (2000 +
    700 proteins, 4500 Å, seed 17) over `steps` steps of the whole-box oracle:
    computed once, shared, never changed."""
    p, st = scenario(2000, 700, 4500.0, seed=17)
    ref, hashes = whole_box(p, st, steps)
    return p, st, ref, hashes


@functools.lru_cache(maxsize=None)
def evolved(steps=300):
    """The CPU slab tests' scenario (4000 + 1500, 6000 Å, seed 9) after `steps`
    steps of the whole-box oracle: bonds and complexes exist.  Shared; a test
    takes a copy."""
    p, st = scenario()
    o = O.Oracle(p, nbmode=O.NB_CELLS)
    o.set_state(st)
    o.step(steps, want_hashes=False)
    return p, o.get_state()


class CountsJumpers:
    """Mixed into a window handle: keeps the n_jump of its last report."""

    last_n_jump = 0

    def dd_finish(self):
        rep = super().dd_finish()
        self.last_n_jump = int(rep.n_jump)
        return rep


def jumper_spy(monkeypatch) -> list:
    """Spy on SlabRank._jumper_check over CountsJumpers handles: the returned
    list gets (distinct ids checked, that rank's n_jump) per call."""
    orig = slabs.SlabRank._jumper_check
    calls = []

    def spy(self, ids, xs):
        calls.append((int(np.unique(ids).size), self.eng.last_n_jump))
        return orig(self, ids, xs)

    monkeypatch.setattr(slabs.SlabRank, "_jumper_check", spy)
    return calls


class _World:
    """What SlabRank needs of a comm to build its window: the world size."""

    def __init__(self, world):
        self.world = world


class Rows:
    """n exchange rows in the memory a handle's dd_* calls address: a
    torch.uint8 tensor on the engine's device, a numpy array for an oracle
    window.  ptr is the dst of dd_pack / dd_step and the src of dd_unpack."""

    def __init__(self, eng, n):
        self.n = n
        dev = getattr(eng, "device", None)
        if dev is None:
            self.t = None
            self.a = np.zeros(max(n, 1) * ROW, dtype=np.uint8)
            self.ptr = self.a.ctypes.data
        else:
            self.t = torch.zeros(max(n, 1) * ROW, dtype=torch.uint8, device=torch.device("cuda", dev))
            self.ptr = self.t.data_ptr()

    def get(self) -> np.ndarray:
        """The n rows on the host, [n, ROW] bytes (a copy)."""
        a = self.a if self.t is None else self.t.cpu().numpy()
        return a[: self.n * ROW].reshape(self.n, ROW).copy()

    def put(self, rows: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1)
        assert rows.size == self.n * ROW
        if self.t is None:
            self.a[: rows.size] = rows
        else:
            self.t[: rows.size] = torch.from_numpy(rows).to(self.t.device)
            torch.cuda.synchronize(self.t.device)


class Family:
    """The G windows of one global state on one kind of handle."""

    def __init__(self, p, hs, G, make, halo=900.0, margin=None):
        world = _World(G)
        self.G = G
        self.ranks = [slabs.SlabRank(p, r, world, make, halo=halo, margin=margin) for r in range(G)]
        for r in self.ranks:
            r.start(hs)
        self.send = [Rows(r.eng, r.n_send) for r in self.ranks]
        self.x0 = [slabs.ref_x(hs)[r.win.gids] for r in self.ranks]  # x of [1][1] when the windows were set

    def recv_ids(self, k) -> np.ndarray:
        """Window k's received local ids, in the order of its receive plan."""
        me = self.ranks[k]
        src_of, own = me.plan.owner[me.win.gids], me.win.own == 1
        return np.concatenate([np.flatnonzero((src_of == s) & ~own) for s in range(self.G) if s != k]).astype(np.int32)

    def received(self, k) -> np.ndarray:
        """The rows window k receives, [n_recv, ROW], from the send buffers as
        they stand (the last step's)."""
        me = self.ranks[k]
        out = np.zeros((me.n_recv, ROW), dtype=np.uint8)
        for s in range(self.G):
            n = me.recv_n[s]
            if s != k and n:
                f = self.ranks[s].send_first[k]
                out[me.recv_first[s]:me.recv_first[s] + n] = self.send[s].get()[f:f + n]
        return out

    def step(self, S):
        """One step of the protocol as LocalComm runs it: every window steps and
        packs into its send buffer, unpacks its neighbours' rows in place, and
        finishes.  Returns (records, reports)."""
        recs = [r.eng.dd_step(b.ptr, S)[0].copy() for r, b in zip(self.ranks, self.send)]
        for k, me in enumerate(self.ranks):
            for s in range(self.G):
                n = me.recv_n[s]
                if s != k and n:
                    me.eng.dd_unpack(self.send[s].ptr + self.ranks[s].send_first[k] * ROW, me.recv_first[s], n)
        return recs, [r.eng.dd_finish() for r in self.ranks]

    def unpack(self, k, rows: np.ndarray, first: int):
        """rows [n, ROW] over window k's receive plan from `first`; its report."""
        eng = self.ranks[k].eng
        buf = Rows(eng, rows.shape[0])
        buf.put(rows)
        eng.dd_unpack(buf.ptr, first, rows.shape[0])
        return eng.dd_finish()  # waits for the unpack: buf may go

    def export_all(self, k):
        n = self.ranks[k].win.gids.size
        return self.ranks[k].eng.dd_export(np.arange(n, dtype=np.int32))

    def close(self):
        for r in self.ranks:
            r.close()


def report_fields(rep) -> dict:
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS}


def jumper_set(ids, xs) -> set:
    """{(local id, x bits)}"""
    return set(zip(np.asarray(ids).tolist(), np.asarray(xs, dtype=np.float64).view(np.int64).tolist()))


def bond_set(rep) -> set:
    """The listed cross-slab bonds as unordered pairs (kmc.h fixes no order
    within a pair, and slabs.py reads them as the edges of an undirected graph)."""
    return {tuple(sorted(int(v) for v in pr)) for pr in rep.cross_bonds()}


def same_export(a, b) -> bool:
    """dd_export results equal: beads bit for bit (the sign of zero included), ints."""
    return np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1])


def run_and_compare(p, st, ref, hashes, G, steps, make, **kw):
    """A decomposed run of `steps` steps over make's handles against the
    whole-box oracle's records and per-step state hashes; returns the ranks
    (still open: the caller reads their handles, then closes them)."""
    got_h = []
    recs, ranks = slabs.run_local(p, st, G, steps, make, gather_every=1,
                                  on_step=lambda me, k, rec: got_h.append(engine.state_hash(p, me.last_global)),
                                  **kw)
    bad = [k + 1 for k in range(steps) if recs[k] != ref[k] or got_h[k] != int(hashes[k])]
    assert not bad, f"G={G}: steps {bad[:10]} differ from the whole-box oracle"
    return ranks
