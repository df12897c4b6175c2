"""ctypes mirror of include/kmc.h (the C-ABI of libkmc).

Struct layouts here must match include/kmc.h field for field; the
`tests/test_host.py::test_ctypes_layouts_match_header` CPU test checks sizes/offsets against the compiled
library.  Nothing in this module computes anything: it only marshals host
buffers (numpy arrays) across the C boundary.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# KMC_LIB_PATH: diagnostic builds only (e.g. the -DKMC_STAMPS timing build, the
# A/B variants of tools/build_variants.py).  It is honoured only together with
# KMC_DIAG=1, so a stray variable cannot make tests or benchmarks load a
# library other than the in-tree build.
if os.environ.get("KMC_LIB_PATH") and os.environ.get("KMC_DIAG") != "1":
    raise RuntimeError("KMC_LIB_PATH is set without KMC_DIAG=1: refusing to load a non-default libkmc")
LIB_PATH = os.environ.get("KMC_LIB_PATH") or os.path.join(HERE, "lib", "libkmc.so")

KMC_OK = 0
ERRORS = {
    -1: "KMC_ERR_ARG",
    -2: "KMC_ERR_IO",
    -3: "KMC_ERR_FORMAT",
    -4: "KMC_ERR_STATE",
    -5: "KMC_ERR_PLACEMENT",
    -6: "KMC_ERR_CAPACITY",
    -7: "KMC_ERR_HIP",
    -8: "KMC_ERR_GEOMETRY",
    -9: "KMC_ERR_NODEVICE",
}
# KMC_ERR_* as module constants (ERR_ARG = -1, ...)
globals().update({name[4:]: code for code, name in ERRORS.items()})


class Params(C.Structure):
    """kmc_params — reference globals main.cpp:39-99 as a runtime struct."""

    _fields_ = [
        ("n_a", C.c_int32),
        ("n_b", C.c_int32),
        ("time_step", C.c_double),
        ("box_x", C.c_double),
        ("box_y", C.c_double),
        ("box_z", C.c_double),
        ("pai", C.c_double),
        ("ra_radius", C.c_double),
        ("ra_D", C.c_double),
        ("ra_rot_D", C.c_double),
        ("rb_radius", C.c_double),
        ("rb_D", C.c_double),
        ("rb_rot_D", C.c_double),
        ("mono_cis_ass_rate", C.c_double),
        ("mono_cis_diss_rate", C.c_double),
        ("cis_D", C.c_double),
        ("cis_rot_D", C.c_double),
        ("cis_ass_rate", C.c_double),
        ("cis_diss_rate", C.c_double),
        ("bond_D", C.c_double),
        ("bond_rot_D", C.c_double),
        ("ass_rate", C.c_double),
        ("diss_rate", C.c_double),
        ("bond_dist_cutoff", C.c_double),
        ("bond_thetapd_cutoff", C.c_double),
        ("bond_thetaot_cutoff", C.c_double),
        ("cis_thetaot_cutoff", C.c_double),
        ("cis_dist_cutoff", C.c_double),
        ("simu_step", C.c_int64),
        ("out_interval", C.c_int32),
        ("reserved0", C.c_int32),
        ("seed", C.c_uint64),
        ("replica", C.c_uint32),
        ("reserved1", C.c_int32),
    ]


class Obs(C.Structure):
    """kmc_obs — one bond.dat record (main.cpp:2251) + raw cluster sums."""

    _fields_ = [
        ("step", C.c_int64),
        ("t", C.c_double),
        ("bond_num_rl", C.c_int32),
        ("bond_num_mono_cis", C.c_int32),
        ("bond_num_cis", C.c_int32),
        ("bond_num", C.c_int32),
        ("cluster_size", C.c_double),
        ("protein_num_in_max_complex", C.c_int32),
        ("tot_proteins_in_cluster", C.c_int32),
        ("tot_cluster_num", C.c_int32),
        ("reserved", C.c_int32),
    ]


OBS_DTYPE = np.dtype(
    [
        ("step", "<i8"),
        ("t", "<f8"),
        ("bond_num_rl", "<i4"),
        ("bond_num_mono_cis", "<i4"),
        ("bond_num_cis", "<i4"),
        ("bond_num", "<i4"),
        ("cluster_size", "<f8"),
        ("protein_num_in_max_complex", "<i4"),
        ("tot_proteins_in_cluster", "<i4"),
        ("tot_cluster_num", "<i4"),
        ("reserved", "<i4"),
    ]
)
assert OBS_DTYPE.itemsize == C.sizeof(Obs)


class StateView(C.Structure):
    """kmc_state_view — host SoA buffers, reference bead order (kmc.h)."""

    _fields_ = [
        ("ra", C.POINTER(C.c_double)),
        ("rb", C.POINTER(C.c_double)),
        ("a_int", C.POINTER(C.c_int32)),
        ("b_int", C.POINTER(C.c_int32)),
        ("counters", C.c_int32 * 5),
        ("reserved", C.c_int32),
        ("step", C.c_int64),
    ]


class Census(C.Structure):
    """kmc_census — summary of the bond graph's components (kmc_oligomer_census)."""

    _fields_ = [
        ("n_components", C.c_int64),
        ("n_complexes", C.c_int64),
        ("proteins_in_complexes", C.c_int64),
        ("n_cis_dimers", C.c_int64),
        ("max_size", C.c_int32),
        ("max_receptors", C.c_int32),
        ("max_ligands", C.c_int32),
        ("max_label", C.c_int32),
    ]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


PAIR_AA, PAIR_AB, PAIR_BB = 0, 1, 2   # KMC_PAIR_*
PAIRS = {"AA": PAIR_AA, "AB": PAIR_AB, "BB": PAIR_BB}
CENSUS_MAX_BINS = 4096                # KMC_CENSUS_MAX_BINS (device histogram)
PAIR_MAX_BINS = 4096                  # KMC_PAIR_MAX_BINS

TRACK_CLASSES = 5                     # KMC_TRACK_CLASSES
TRACK_MAX_BINS = 512                  # KMC_TRACK_MAX_BINS
TRACK_CHANGED, TRACK_JUMPED = 1, 2    # KMC_TRACK_CHANGED / KMC_TRACK_JUMPED (flag bits)


class TrackInfo(C.Structure):
    """kmc_track_info — what kmc_track_update reports."""

    _fields_ = [
        ("origin_step", C.c_int64),
        ("last_step", C.c_int64),
        ("n_updates", C.c_int64),
        ("max_dx", C.c_double),
        ("max_dy", C.c_double),
        ("n_jumped", C.c_int64),
        ("n_changed", C.c_int64),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrackSample(C.Structure):
    """kmc_track_sample_t — per-class counts and sums of squared displacements, bond survival."""

    _fields_ = [
        ("origin_step", C.c_int64),
        ("last_step", C.c_int64),
        ("n", C.c_int64 * TRACK_CLASSES),
        ("n_clean", C.c_int64 * TRACK_CLASSES),
        ("sum_u2", C.c_double * TRACK_CLASSES),
        ("sum_u2_clean", C.c_double * TRACK_CLASSES),
        ("rl0", C.c_int64),
        ("rl_now", C.c_int64),
        ("rl_kept", C.c_int64),
        ("cis0", C.c_int64),
        ("cis_now", C.c_int64),
        ("cis_kept", C.c_int64),
    ]

    SURVIVAL = ("rl0", "rl_now", "rl_kept", "cis0", "cis_now", "cis_kept")

    def as_dict(self) -> dict:
        """Plain Python / numpy values: the arrays as int64 / float64 numpy arrays."""
        d = {"origin_step": int(self.origin_step), "last_step": int(self.last_step)}
        for k in ("n", "n_clean"):
            d[k] = np.array(list(getattr(self, k)), dtype=np.int64)
        for k in ("sum_u2", "sum_u2_clean"):
            d[k] = np.array(list(getattr(self, k)), dtype=np.float64)
        for k in self.SURVIVAL:
            d[k] = int(getattr(self, k))
        return d


KIN_BINS, KIN_HISTS = 256, 9          # KMC_KIN_BINS / KMC_KIN_HISTS
KIN_RL_CENSORED, KIN_CIS_CENSORED, KIN_COMPLEX = 1, 2, 4  # KMC_KIN_* (bits of a receptor's record)
# rows of the kinetics histogram
KIN_ROWS = ("rl", "rl_censored", "cis_mono", "cis_cx", "cis_censored", "rebind_same", "rebind_other", "rl_alive",
            "cis_alive")


class KinOut(C.Structure):
    """kmc_kin_out — steps, event counters, exposures and occupancy of the bond kinetics recorder."""

    _fields_ = [(name, C.c_int64) for name in (
        "origin_step", "last_step", "n_updates",
        "rl_on", "rl_off", "rl_swap", "cis_on", "cis_off_mono", "cis_off_cx", "cis_swap",
        "exp_rl", "exp_mono", "exp_cx", "exp_free_receptor", "exp_free_site",
        "occ_rl", "occ_mono", "occ_cx", "occ_free_receptor", "occ_free_site",
        "n_rl_censored_alive", "n_cis_censored_alive")]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class KinView(C.Structure):
    """kmc_kin_view — caller-owned per-receptor arrays of the recorder."""

    _fields_ = [
        ("rl_lig", C.POINTER(C.c_int32)),
        ("rl_site", C.POINTER(C.c_int32)),
        ("rl_since", C.POINTER(C.c_int64)),
        ("cis_with", C.POINTER(C.c_int32)),
        ("cis_since", C.POINTER(C.c_int64)),
        ("last_lig", C.POINTER(C.c_int32)),
        ("free_since", C.POINTER(C.c_int64)),
        ("bits", C.POINTER(C.c_uint8)),
    ]


class KinArrays:
    """numpy-backed kmc_kin_view for n_a receptors: the eight arrays as attributes."""

    DTYPES = dict(rl_lig=np.int32, rl_site=np.int32, rl_since=np.int64, cis_with=np.int32, cis_since=np.int64,
                  last_lig=np.int32, free_since=np.int64, bits=np.uint8)

    def __init__(self, n_a: int):
        for name, dt in self.DTYPES.items():
            setattr(self, name, np.zeros(n_a, dtype=dt))

    def view(self) -> KinView:
        v = KinView()
        for name, ptr in KinView._fields_:
            setattr(v, name, getattr(self, name).ctypes.data_as(ptr))
        return v

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name in self.DTYPES}


GEOM_MAX_SIZE = 1023                  # KMC_GEOM_MAX_SIZE (device table bins)
SPAN_X, SPAN_Y = 1, 2                 # KMC_SPAN_X / KMC_SPAN_Y (spanning bits)


class I128(C.Structure):
    """kmc_i128 — the two's-complement number hi * 2^64 + lo."""

    _fields_ = [("lo", C.c_uint64), ("hi", C.c_int64)]

    def __int__(self) -> int:
        return (int(self.hi) << 64) + int(self.lo)


class GeomBin(C.Structure):
    """kmc_geom_bin — one size bin of kmc_cluster_geometry's table."""

    _fields_ = [("count", C.c_int64), ("sum_size", C.c_int64), ("sum_m", I128)]


# kmc_geom_bin as a numpy record: the 128-bit sum as its two words
GEOM_BIN_DTYPE = np.dtype([("count", "<i8"), ("sum_size", "<i8"), ("sum_m_lo", "<u8"), ("sum_m_hi", "<i8")])
assert GEOM_BIN_DTYPE.itemsize == C.sizeof(GeomBin)


class Geom(C.Structure):
    """kmc_geom — summary of kmc_cluster_geometry."""

    _fields_ = [
        ("n_measured", C.c_int64),
        ("n_spanning", C.c_int64),
        ("n_span_x", C.c_int64),
        ("n_span_y", C.c_int64),
        ("proteins_in_spanning", C.c_int64),
        ("largest_label", C.c_int32),
        ("largest_size", C.c_int32),
        ("largest_span", C.c_int32),
        ("reserved", C.c_int32),
    ]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class Cluster(C.Structure):
    """kmc_cluster — one row of kmc_cluster_list."""

    _fields_ = [
        ("label", C.c_int32),
        ("n_r", C.c_int32),
        ("n_l", C.c_int32),
        ("span", C.c_int32),
        ("s1x", C.c_int64),
        ("s1y", C.c_int64),
        ("s2xx", I128),
        ("s2yy", I128),
        ("s2xy", I128),
    ]

    def as_dict(self) -> dict:
        """Plain Python ints, the 128-bit sums whole."""
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


CF_MAX_SIZE, CF_PIECES, CF_KINDS = 63, 9, 4   # KMC_CF_MAX_SIZE / KMC_CF_PIECES / KMC_CF_KINDS
# kinds of a piece of a binary merger / fragmentation
CF_KIND_NAMES = ("receptor", "ligand", "receptor_pair", "other")


class CfOut(C.Structure):
    """kmc_cf_out — steps and counters of the cluster growth recorder."""

    _fields_ = [(name, C.c_int64) for name in (
        "origin_step", "last_step", "n_updates", "max_size",
        "formed_rl", "formed_cis", "broken_rl", "broken_cis",
        "n_cores", "n_clusters", "cycles_closed", "cycles_opened", "max_cluster")]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class CfView(C.Structure):
    """kmc_cf_view — caller-owned per-protein arrays of the growth recorder."""

    _fields_ = [
        ("rl_lig", C.POINTER(C.c_int32)),
        ("cis_with", C.POINTER(C.c_int32)),
        ("prev_label", C.POINTER(C.c_int32)),
    ]


class CfArrays:
    """numpy-backed kmc_cf_view: rl_lig[n_a], cis_with[n_a], prev_label[n_a + n_b] as attributes."""

    NAMES = ("rl_lig", "cis_with", "prev_label")

    def __init__(self, n_a: int, n_b: int):
        self.rl_lig = np.zeros(n_a, dtype=np.int32)
        self.cis_with = np.zeros(n_a, dtype=np.int32)
        self.prev_label = np.zeros(n_a + n_b, dtype=np.int32)

    def view(self) -> CfView:
        v = CfView()
        for name, ptr in CfView._fields_:
            setattr(v, name, getattr(self, name).ctypes.data_as(ptr))
        return v

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name in self.NAMES}


class CfTablesView(C.Structure):
    """kmc_cf_tables — caller-owned tables of the growth recorder."""

    _fields_ = [(name, C.POINTER(C.c_int64)) for name in (
        "merge", "frag", "merge_kind", "frag_kind", "merge_pieces", "frag_pieces", "merge_product", "frag_parent",
        "n_s", "expo")] + [("expo2", C.POINTER(I128))]


# kmc_i128 as a numpy record: its two words
I128_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<i8")])
assert I128_DTYPE.itemsize == C.sizeof(I128)


class CfTables:
    """numpy-backed kmc_cf_tables for the size clamp S: merge, frag [S+1, S+1] (upper triangle), merge_kind,
    frag_kind [4, 4], merge_pieces, frag_pieces [9], merge_product, frag_parent, n_s, expo [S+1] int64, and
    expo2 [S+1, S+1] as I128_DTYPE records (expo2_int(): Python ints)."""

    INT64 = ("merge", "frag", "merge_kind", "frag_kind", "merge_pieces", "frag_pieces", "merge_product",
             "frag_parent", "n_s", "expo")

    def __init__(self, max_size: int):
        s1 = int(max_size) + 1
        self.max_size = int(max_size)
        self.merge = np.zeros((s1, s1), dtype=np.int64)
        self.frag = np.zeros((s1, s1), dtype=np.int64)
        self.merge_kind = np.zeros((CF_KINDS, CF_KINDS), dtype=np.int64)
        self.frag_kind = np.zeros((CF_KINDS, CF_KINDS), dtype=np.int64)
        self.merge_pieces = np.zeros(CF_PIECES, dtype=np.int64)
        self.frag_pieces = np.zeros(CF_PIECES, dtype=np.int64)
        self.merge_product = np.zeros(s1, dtype=np.int64)
        self.frag_parent = np.zeros(s1, dtype=np.int64)
        self.n_s = np.zeros(s1, dtype=np.int64)
        self.expo = np.zeros(s1, dtype=np.int64)
        self.expo2 = np.zeros((s1, s1), dtype=I128_DTYPE)

    def view(self) -> CfTablesView:
        v = CfTablesView()
        for name, ptr in CfTablesView._fields_:
            setattr(v, name, getattr(self, name).ctypes.data_as(ptr))
        return v

    def expo2_int(self) -> list:
        """expo2 as rows of Python ints (the 128-bit words whole)."""
        return [[(int(w["hi"]) << 64) + int(w["lo"]) for w in row] for row in self.expo2]

    def as_dict(self) -> dict:
        """The int64 tables by name (what analysis.reduce_counts adds over replicas) and expo2 as Python ints."""
        d = {name: getattr(self, name) for name in self.INT64}
        d["expo2"] = self.expo2_int()
        return d


def geom_m(table) -> list:
    """The 128-bit sum of m of every bin of a GEOM_BIN_DTYPE table, as Python ints."""
    return [(int(hi) << 64) + int(lo) for lo, hi in zip(table["sum_m_lo"], table["sum_m_hi"])]


SK_MAX = 64                           # KMC_SK_MAX: largest hmax / kmax of kmc_structure_factor
SK_ALL, SK_BOUND = 0, 1               # KMC_SK_ALL / KMC_SK_BOUND (the proteins summed over)
SK_SELECT = {"all": SK_ALL, "bound": SK_BOUND}


def sk_select(select) -> int:
    """'all' / 'bound' or the KMC_SK_* number itself, as the int32 the library takes."""
    return SK_SELECT[select] if isinstance(select, str) else int(select)


BO_A, BO_B = 0, 1                     # KMC_BO_A / KMC_BO_B (the species whose order is measured)
BO_WITHIN, BO_LINKED = 0, 1           # KMC_BO_WITHIN / KMC_BO_LINKED (the neighbour relation)
BO_ALL, BO_BOUND = 0, 1               # KMC_BO_ALL / KMC_BO_BOUND (KMC_SK_BOUND's rule)
BO_MAX_FOLD = 12                      # KMC_BO_MAX_FOLD
BO_NN_ROWS = 16                       # KMC_BO_NN_ROWS: histogram rows, neighbour counts clamp into the last
BO_HIST_BINS, BO_CORR_BINS = 1024, 4096  # most bins of kmc_bond_order / kmc_bond_order_corr
BO_WHICH = {"A": BO_A, "B": BO_B}
BO_MODE = {"within": BO_WITHIN, "linked": BO_LINKED}


def bo_which(which) -> int:
    """'A' / 'B' or the KMC_BO_* number itself."""
    return BO_WHICH[which] if isinstance(which, str) else int(which)


def bo_mode(mode) -> int:
    """'within' / 'linked' or the KMC_BO_* number itself."""
    return BO_MODE[mode] if isinstance(mode, str) else int(mode)


class BondOrderOut(C.Structure):
    """kmc_bond_order_out — the global sums of kmc_bond_order."""

    _fields_ = [(name, C.c_int64) for name in ("n_sel", "n_with", "sum_nn", "sum_pc", "sum_ps", "sum_m")]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


RING_MAX = 12  # KMC_RING_MAX: the longest ring kmc_rings counts


class NetOut(C.Structure):
    """kmc_net_out — the counters of the ligand network (kmc_network, kmc_rings) and the receptors' valency bins."""

    _fields_ = [(name, C.c_int64) for name in ("n_bridges", "n_loops", "n_half", "n_free_dimers", "n_vertices",
                                               "n_net_components", "cycle_rank")] + [("rec", C.c_int64 * 4)]

    def as_dict(self) -> dict:
        d = {name: int(getattr(self, name)) for name, _ in self._fields_[:-1]}
        d["rec"] = [int(x) for x in self.rec]
        return d


LAG_MAX_LEVELS, LAG_MAX_SLOTS, LAG_MAX_Q, LAG_CLASSES, LAG_MAX_ROWS = 20, 16, 4, 5, 168  # KMC_LAG_*


class LagConfig(C.Structure):
    """kmc_lag_config — the lag correlator's configuration."""

    _fields_ = [("every", C.c_int32), ("levels", C.c_int32), ("slots", C.c_int32), ("nq", C.c_int32),
                ("max_jump", C.c_double), ("max_disp", C.c_double), ("h", C.c_int32 * LAG_MAX_Q)]


def lag_config(every: int, levels: int, slots: int, max_jump: float = 0.0, max_disp: float = 0.0, h=()) -> LagConfig:
    """A LagConfig from its parts; h: the multipliers of F_s (nq = len(h))."""
    h = [int(x) for x in h]
    if len(h) > LAG_MAX_Q:
        raise ValueError("lag: at most %d multipliers" % LAG_MAX_Q)
    c = LagConfig(int(every), int(levels), int(slots), len(h), float(max_jump), float(max_disp))
    for k, x in enumerate(h):
        c.h[k] = x
    return c


class LagInfo(C.Structure):
    """kmc_lag_info — one update: its number n, the (level, j) pairs filed, the proteins with an event."""

    _fields_ = [(name, C.c_int64) for name in ("n_updates", "n_tasks", "n_events")]


class LagOut(C.Structure):
    """kmc_lag_out — the configuration in effect, the integer bounds and box, the steps and the update count."""

    _fields_ = [("cfg", LagConfig)] + [(name, C.c_int64) for name in (
        "J", "F", "BX", "BY", "origin_step", "last_step", "n_updates", "rows")]


class LagView(C.Structure):
    """kmc_lag_view — caller-owned arrays of the recorder on the host."""

    _fields_ = [("prev", C.POINTER(C.c_int64)), ("U", C.POINTER(C.c_int64)), ("links", C.POINTER(C.c_int32)),
                ("last_event", C.POINTER(C.c_int32)), ("ring", C.POINTER(C.c_int64)), ("table", C.c_void_p),
                ("n_pairs", C.POINTER(C.c_int64))]


# kmc_lag_cell as a numpy record
LAG_CELL_DTYPE = np.dtype([("n_all", "<i8"), ("n_clean", "<i8"), ("n_far", "<i8"), ("m2_all", I128_DTYPE),
                           ("m2_clean", I128_DTYPE), ("m4_clean", I128_DTYPE), ("fs", I128_DTYPE, (LAG_MAX_Q,))])
assert LAG_CELL_DTYPE.itemsize == 136
LAG_COUNTS = ("n_all", "n_clean", "n_far")
LAG_SUMS = ("m2_all", "m2_clean", "m4_clean")
LAG_LIMBS = 4  # a 128-bit sum as four 32-bit limbs, the top one signed: limbs add without a carry


def lag_rows(levels: int, slots: int) -> int:
    return slots + (levels - 1) * (slots // 2)


def lag_row_lags(levels: int, slots: int) -> np.ndarray:
    """The lag of every row in updates: j at level 0, j 2^l above."""
    lags = list(range(1, slots + 1))
    for l in range(1, levels):
        lags += [j << l for j in range(slots // 2 + 1, slots + 1)]
    return np.array(lags, dtype=np.int64)


def _i128_ints(a: np.ndarray) -> np.ndarray:
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = (int(a[idx]["hi"]) << 64) + int(a[idx]["lo"])
    return out


class LagSample:
    """One kmc_lag_sample: the configuration and steps (as attributes and in .out), n_pairs [rows] and, as arrays of
    Python ints (the 128-bit sums whole): n_all, n_clean, n_far, m2_all, m2_clean, m4_clean [rows, 5] and
    fs [rows, 5, nq].  counts() / from_counts(): the sample as one int64 vector that adds (analysis.reduce_counts)."""

    def __init__(self, out: LagOut, table: np.ndarray, n_pairs: np.ndarray):
        self.out = out
        self.every, self.levels, self.slots, self.nq = out.cfg.every, out.cfg.levels, out.cfg.slots, out.cfg.nq
        self.h = [int(out.cfg.h[k]) for k in range(self.nq)]
        self.max_jump, self.max_disp = out.cfg.max_jump, out.cfg.max_disp
        for name in ("J", "F", "BX", "BY", "origin_step", "last_step", "n_updates", "rows"):
            setattr(self, name, int(getattr(out, name)))
        self.lags = lag_row_lags(self.levels, self.slots)
        self.n_pairs = np.array([int(x) for x in n_pairs], dtype=object)
        for name in LAG_COUNTS:
            setattr(self, name, table[name].astype(object))
        for name in LAG_SUMS:
            setattr(self, name, _i128_ints(table[name]))
        self.fs = _i128_ints(table["fs"][:, :, :self.nq])

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name in LAG_COUNTS + LAG_SUMS + ("fs", "n_pairs")}

    def counts(self) -> np.ndarray:
        """[rows + rows * 5 * (3 + 4 * (3 + nq))] int64: n_pairs, then per cell the counts and every sum's limbs."""
        v = [int(x) for x in self.n_pairs]
        for r in range(self.rows):
            for c in range(LAG_CLASSES):
                v += [int(getattr(self, name)[r, c]) for name in LAG_COUNTS]
                for x in [getattr(self, name)[r, c] for name in LAG_SUMS] + list(self.fs[r, c]):
                    x = int(x)
                    v += [x >> 32 * k & 0xFFFFFFFF for k in range(LAG_LIMBS - 1)] + [x >> 32 * (LAG_LIMBS - 1)]
        return np.array(v, dtype=np.int64)

    def from_counts(self, counts) -> "LagSample":
        """A sample of this one's configuration holding the (summed) counts() vector."""
        import copy
        s = copy.copy(self)
        it = iter(int(x) for x in np.asarray(counts).ravel())
        s.n_pairs = np.array([next(it) for _ in range(self.rows)], dtype=object)
        shape = (self.rows, LAG_CLASSES)
        for name in LAG_COUNTS + LAG_SUMS:
            setattr(s, name, np.zeros(shape, dtype=object))
        s.fs = np.zeros(shape + (self.nq,), dtype=object)
        limbs = lambda: sum(next(it) << 32 * k for k in range(LAG_LIMBS))
        for r in range(self.rows):
            for c in range(LAG_CLASSES):
                for name in LAG_COUNTS:
                    getattr(s, name)[r, c] = next(it)
                for name in LAG_SUMS:
                    getattr(s, name)[r, c] = limbs()
                for k in range(self.nq):
                    s.fs[r, c, k] = limbs()
        return s


class LagArrays:
    """numpy-backed kmc_lag_view for n proteins: prev, U [n, 2], links [3, n], last_event [n], ring [levels, slots, n, 2],
    table [rows, 5] (LAG_CELL_DTYPE), n_pairs [rows]."""

    def __init__(self, n: int, levels: int, slots: int):
        rows = lag_rows(levels, slots)
        self.prev = np.zeros((n, 2), dtype=np.int64)
        self.U = np.zeros((n, 2), dtype=np.int64)
        self.links = np.zeros((3, n), dtype=np.int32)
        self.last_event = np.zeros(n, dtype=np.int32)
        self.ring = np.zeros((levels, slots, n, 2), dtype=np.int64)
        self.table = np.zeros((rows, LAG_CLASSES), dtype=LAG_CELL_DTYPE)
        self.n_pairs = np.zeros(rows, dtype=np.int64)

    def view(self) -> LagView:
        v = LagView()
        for name, ptr in LagView._fields_:
            a = getattr(self, name)
            setattr(v, name, a.ctypes.data if ptr is C.c_void_p else a.ctypes.data_as(ptr))
        return v


PD_MAX_BINS, PD_JUMPED = 256, 1  # KMC_PD_MAX_BINS, KMC_PD_JUMPED


class PdConfig(C.Structure):
    """kmc_pd_config — the pair dynamics' configuration."""

    _fields_ = [("every", C.c_int32), ("nbins", C.c_int32), ("r_max", C.c_double), ("max_jump", C.c_double),
                ("max_disp", C.c_double)]


def pd_config(every: int, nbins: int, r_max: float, max_jump: float = 0.0, max_disp: float = 0.0) -> PdConfig:
    return PdConfig(int(every), int(nbins), float(r_max), float(max_jump), float(max_disp))


class PdInfo(C.Structure):
    """kmc_pd_info — one update: its number n and the proteins flagged jumped after it."""

    _fields_ = [(name, C.c_int64) for name in ("n_updates", "n_jumped")]


class PdOut(C.Structure):
    """kmc_pd_out — the configuration in effect, the integer bounds and box, the search grid, the steps."""

    _fields_ = [("cfg", PdConfig)] + [(name, C.c_int64) for name in (
        "J", "F", "BX", "BY", "ncx", "ncy", "origin_step", "last_step", "n_updates")]


class PdView(C.Structure):
    """kmc_pd_view — caller-owned arrays of the recorder on the host."""

    _fields_ = [("prev", C.POINTER(C.c_int64)), ("U", C.POINTER(C.c_int64)), ("X0", C.POINTER(C.c_int64)),
                ("flags", C.POINTER(C.c_uint8))]


# kmc_pd_cell as a numpy record
PD_CELL_DTYPE = np.dtype([("n_pairs", "<i8"), ("n_valid", "<i8"), ("dot", I128_DTYPE), ("sq", I128_DTYPE)])
assert PD_CELL_DTYPE.itemsize == 48
PD_COUNTS = ("n_pairs", "n_valid")
PD_SUMS = ("dot", "sq")


class PdSample:
    """One kmc_pd_sample: the configuration and steps (as attributes and in .out) and, as arrays of Python ints,
    gd [4, nbins] (kind 2 species(i) + species(j)), gs [2, nbins] and part B's n_pairs, n_valid, dot, sq [3, nbins]
    (AA, AB, BB; the 128-bit sums whole).  lag_steps = last_step - origin_step.  counts() / from_counts(): the
    sample as one int64 vector that adds (analysis.reduce_counts)."""

    def __init__(self, out: PdOut, gd: np.ndarray, gs: np.ndarray, cu: np.ndarray):
        self.out = out
        self.every, self.nbins, self.r_max = out.cfg.every, out.cfg.nbins, out.cfg.r_max
        self.max_jump, self.max_disp = out.cfg.max_jump, out.cfg.max_disp
        for name in ("J", "F", "BX", "BY", "ncx", "ncy", "origin_step", "last_step", "n_updates"):
            setattr(self, name, int(getattr(out, name)))
        self.lag_steps = self.last_step - self.origin_step
        self.gd = gd.astype(object)
        self.gs = gs.astype(object)
        for name in PD_COUNTS:
            setattr(self, name, cu[name].astype(object))
        for name in PD_SUMS:
            setattr(self, name, _i128_ints(cu[name]))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name in ("gd", "gs") + PD_COUNTS + PD_SUMS}

    def counts(self) -> np.ndarray:
        """[nbins * (6 + 3 * (2 + 2 * 4))] int64: gd, gs, then per cell of part B the counts and both sums' limbs."""
        v = [int(x) for x in self.gd.ravel()] + [int(x) for x in self.gs.ravel()]
        for kind in range(3):
            for k in range(self.nbins):
                v += [int(getattr(self, name)[kind, k]) for name in PD_COUNTS]
                for name in PD_SUMS:
                    x = int(getattr(self, name)[kind, k])
                    v += [x >> 32 * m & 0xFFFFFFFF for m in range(LAG_LIMBS - 1)] + [x >> 32 * (LAG_LIMBS - 1)]
        return np.array(v, dtype=np.int64)

    def from_counts(self, counts) -> "PdSample":
        """A sample of this one's configuration holding the (summed) counts() vector."""
        import copy
        s = copy.copy(self)
        it = iter(int(x) for x in np.asarray(counts).ravel())
        nb = self.nbins
        s.gd = np.array([next(it) for _ in range(4 * nb)], dtype=object).reshape(4, nb)
        s.gs = np.array([next(it) for _ in range(2 * nb)], dtype=object).reshape(2, nb)
        for name in PD_COUNTS + PD_SUMS:
            setattr(s, name, np.zeros((3, nb), dtype=object))
        for kind in range(3):
            for k in range(nb):
                for name in PD_COUNTS:
                    getattr(s, name)[kind, k] = next(it)
                for name in PD_SUMS:
                    getattr(s, name)[kind, k] = sum(next(it) << 32 * m for m in range(LAG_LIMBS))
        return s


class PdArrays:
    """numpy-backed kmc_pd_view for n proteins: prev, U, X0 [n, 2] int64 and flags [n] uint8."""

    def __init__(self, n: int):
        self.prev = np.zeros((n, 2), dtype=np.int64)
        self.U = np.zeros((n, 2), dtype=np.int64)
        self.X0 = np.zeros((n, 2), dtype=np.int64)
        self.flags = np.zeros(n, dtype=np.uint8)

    def view(self) -> PdView:
        v = PdView()
        for name, ptr in PdView._fields_:
            setattr(v, name, getattr(self, name).ctypes.data_as(ptr))
        return v


BD_MAX_SIZE, BD_ROT_MAX = 255, 1023                 # KMC_BD_MAX_SIZE, KMC_BD_ROT_MAX
BD_JUMPED, BD_CHANGED, BD_WIDE = 1, 2, 4            # KMC_BD_JUMPED, KMC_BD_CHANGED; KMC_BD_WIDE beside SPAN_X, SPAN_Y
BD_INTACT, BD_GROWN, BD_BROKEN = 0, 1, 2            # a body's status
BD_IS_PRISTINE, BD_IS_VALID, BD_IS_ROT = 1, 2, 4    # the bits of kmc_bd_body.is


class BdConfig(C.Structure):
    """kmc_bd_config — the body dynamics' configuration."""

    _fields_ = [("every", C.c_int32), ("max_size", C.c_int32), ("max_jump", C.c_double), ("max_disp", C.c_double)]


def bd_config(every: int, max_size: int, max_jump: float = 0.0, max_disp: float = 0.0) -> BdConfig:
    return BdConfig(int(every), int(max_size), float(max_jump), float(max_disp))


class BdInfo(C.Structure):
    """kmc_bd_info — one update: its number n and the proteins it flagged jumped / changed for the first time."""

    _fields_ = [(name, C.c_int64) for name in ("n_updates", "n_jumped", "n_changed")]


class BdOut(C.Structure):
    """kmc_bd_out — the configuration in effect, the integer bounds and box, the steps, the number of bodies."""

    _fields_ = [("cfg", BdConfig)] + [(name, C.c_int64) for name in (
        "J", "F", "BX", "BY", "origin_step", "last_step", "n_updates", "n_bodies")]


class BdBody(C.Structure):
    """kmc_bd_body — one body of the origin in a sample (bd_bodies)."""

    _fields_ = [(name, C.c_int32) for name in ("label", "n_r", "n_l", "bits", "status", "is_", "cur_label",
                                               "cur_size")] + [("su", C.c_int64 * 2), ("C", C.c_int64), ("S", C.c_int64)]

    def as_tuple(self):
        return (self.label, self.n_r, self.n_l, self.bits, self.status, self.is_, self.cur_label, self.cur_size,
                self.su[0], self.su[1], self.C, self.S)


assert C.sizeof(BdBody) == 64
BD_BODY_DTYPE = np.dtype(BdBody)  # the rows of bd_bodies as a numpy record array: the same fields, su [2]


class BdView(C.Structure):
    """kmc_bd_view — caller-owned arrays of the recorder on the host."""

    _fields_ = [("prev", C.POINTER(C.c_int64)), ("U", C.POINTER(C.c_int64)), ("X0", C.POINTER(C.c_int64)),
                ("links", C.POINTER(C.c_int32)), ("flags", C.POINTER(C.c_uint8)), ("label", C.POINTER(C.c_int32)),
                ("D0", C.POINTER(C.c_int64)), ("bits", C.POINTER(C.c_uint8))]


BD_COUNTS = ("n_bodies", "sum_size", "n_pristine", "n_intact", "n_grown", "n_broken", "n_valid", "n_rot", "n_rot_null",
             "n_rot_skipped", "c1", "c2")
BD_SUMS = ("m2", "phi2")
# kmc_bd_cell as a numpy record
BD_CELL_DTYPE = np.dtype([(name, "<i8") for name in BD_COUNTS] + [(name, I128_DTYPE) for name in BD_SUMS])
assert BD_CELL_DTYPE.itemsize == 128


class BdSample:
    """One kmc_bd_sample: the configuration and steps (as attributes and in .out) and, as [2, max_size + 1] arrays of
    Python ints indexed by (holds a ligand, min(size, max_size)), the fields of kmc_bd_cell (the 128-bit sums whole).
    lag_steps = last_step - origin_step.  counts() / from_counts(): the sample as one int64 vector that adds
    (analysis.reduce_counts) — over replicas, and over recorders sampled at the same lag."""

    def __init__(self, out: BdOut, table: np.ndarray):
        self.out = out
        self.every, self.max_size = out.cfg.every, out.cfg.max_size
        self.max_jump, self.max_disp = out.cfg.max_jump, out.cfg.max_disp
        for name in ("J", "F", "BX", "BY", "origin_step", "last_step", "n_updates"):
            setattr(self, name, int(getattr(out, name)))
        self.total_bodies = int(out.n_bodies)
        self.lag_steps = self.last_step - self.origin_step
        for name in BD_COUNTS:
            setattr(self, name, table[name].astype(object))
        for name in BD_SUMS:
            setattr(self, name, _i128_ints(table[name]))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name in BD_COUNTS + BD_SUMS}

    def counts(self) -> np.ndarray:
        """[2 * (max_size + 1) * (12 + 2 * 4)] int64: per cell the counts, then both sums' limbs."""
        v = []
        for idx in np.ndindex(2, self.max_size + 1):
            v += [int(getattr(self, name)[idx]) for name in BD_COUNTS]
            for name in BD_SUMS:
                x = int(getattr(self, name)[idx])
                v += [x >> 32 * m & 0xFFFFFFFF for m in range(LAG_LIMBS - 1)] + [x >> 32 * (LAG_LIMBS - 1)]
        return np.array(v, dtype=np.int64)

    def from_counts(self, counts) -> "BdSample":
        """A sample of this one's configuration holding the (summed) counts() vector."""
        import copy
        s = copy.copy(self)
        it = iter(int(x) for x in np.asarray(counts).ravel())
        for name in BD_COUNTS + BD_SUMS:
            setattr(s, name, np.zeros((2, self.max_size + 1), dtype=object))
        for idx in np.ndindex(2, self.max_size + 1):
            for name in BD_COUNTS:
                getattr(s, name)[idx] = next(it)
            for name in BD_SUMS:
                getattr(s, name)[idx] = sum(next(it) << 32 * m for m in range(LAG_LIMBS))
        return s


class BdArrays:
    """numpy-backed kmc_bd_view for n proteins: prev, U, X0, D0 [n, 2] int64, links [3, n] int32, flags, bits [n]
    uint8 and label [n] int32 (1-based)."""

    def __init__(self, n: int):
        self.prev = np.zeros((n, 2), dtype=np.int64)
        self.U = np.zeros((n, 2), dtype=np.int64)
        self.X0 = np.zeros((n, 2), dtype=np.int64)
        self.links = np.zeros((3, n), dtype=np.int32)
        self.flags = np.zeros(n, dtype=np.uint8)
        self.label = np.zeros(n, dtype=np.int32)
        self.D0 = np.zeros((n, 2), dtype=np.int64)
        self.bits = np.zeros(n, dtype=np.uint8)

    def view(self) -> BdView:
        v = BdView()
        for name, ptr in BdView._fields_:
            setattr(v, name, getattr(self, name).ctypes.data_as(ptr))
        return v


ROT_VECS, POSE_MAX_BINS, POSE_CLASSES = 2, 64, 4  # KMC_ROT_VECS, KMC_POSE_MAX_BINS, KMC_POSE_CLASSES
ROT_BAD = 1 << 63                                  # KMC_ROT_BAD: the packed word of a bad protein's vector


class RotConfig(C.Structure):
    """kmc_rot_config — the orientation recorder's configuration."""

    _fields_ = [("every", C.c_int32), ("levels", C.c_int32), ("slots", C.c_int32)]


def rot_config(every: int, levels: int, slots: int) -> RotConfig:
    return RotConfig(int(every), int(levels), int(slots))


class RotInfo(C.Structure):
    """kmc_rot_info — one update: its number n, the (level, j) pairs filed, the proteins with an event, the ligands
    whose handedness flipped, the bad proteins."""

    _fields_ = [(name, C.c_int64) for name in ("n_updates", "n_tasks", "n_events", "n_flips", "n_bad")]


class RotOut(C.Structure):
    """kmc_rot_out — the configuration, the steps and the update count."""

    _fields_ = [("cfg", RotConfig), ("pad_", C.c_int32)] + [(name, C.c_int64) for name in (
        "origin_step", "last_step", "n_updates", "rows")]


class RotView(C.Structure):
    """kmc_rot_view — caller-owned arrays of the recorder on the host."""

    _fields_ = [("vec", C.POINTER(C.c_uint64)), ("links", C.POINTER(C.c_int32)), ("last_event", C.POINTER(C.c_int32)),
                ("chi", C.POINTER(C.c_int8)), ("ring", C.POINTER(C.c_uint64)), ("table", C.c_void_p),
                ("n_pairs", C.POINTER(C.c_int64))]


class PoseOut(C.Structure):
    """kmc_pose_out — the ligands of chi = +1 / -1 per number of occupied sites, and the bad ones."""

    _fields_ = [("chi_pos", C.c_int64 * POSE_CLASSES), ("chi_neg", C.c_int64 * POSE_CLASSES), ("n_bad", C.c_int64)]

    def as_dict(self) -> dict:
        return {"chi_pos": [int(x) for x in self.chi_pos], "chi_neg": [int(x) for x in self.chi_neg],
                "n_bad": int(self.n_bad)}


# kmc_rot_cell as a numpy record
ROT_CELL_DTYPE = np.dtype([("n_all", "<i8"), ("n_clean", "<i8"), ("s1_all", I128_DTYPE), ("s1_clean", I128_DTYPE),
                           ("s2_clean", I128_DTYPE)])
assert ROT_CELL_DTYPE.itemsize == 64
ROT_COUNTS = ("n_all", "n_clean")
ROT_SUMS = ("s1_all", "s1_clean", "s2_clean")


def rot_unpack(words) -> np.ndarray:
    """[..., 3] int64 (x, y, z) of packed vector words (three signed 21-bit fields); a ROT_BAD word is not a vector."""
    w = np.asarray(words, dtype=np.uint64)
    f = [(w >> np.uint64(s) & np.uint64(0x1FFFFF)).astype(np.int64) for s in (0, 21, 42)]
    return np.stack([np.where(x >= 1 << 20, x - (1 << 21), x) for x in f], axis=-1)


class RotSample:
    """One kmc_rot_sample: the configuration and steps (as attributes and in .out), n_pairs [rows] and, as arrays of
    Python ints (the 128-bit sums whole): n_all, n_clean, s1_all, s1_clean, s2_clean [rows, 5, 2] (class, vector:
    0 heading / axis, 1 arm).  counts() / from_counts(): the sample as one int64 vector that adds
    (analysis.reduce_counts)."""

    def __init__(self, out: RotOut, table: np.ndarray, n_pairs: np.ndarray):
        self.out = out
        self.every, self.levels, self.slots = out.cfg.every, out.cfg.levels, out.cfg.slots
        for name in ("origin_step", "last_step", "n_updates", "rows"):
            setattr(self, name, int(getattr(out, name)))
        self.lags = lag_row_lags(self.levels, self.slots)
        self.n_pairs = np.array([int(x) for x in n_pairs], dtype=object)
        for name in ROT_COUNTS:
            setattr(self, name, table[name].astype(object))
        for name in ROT_SUMS:
            setattr(self, name, _i128_ints(table[name]))

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name in ROT_COUNTS + ROT_SUMS + ("n_pairs",)}

    def counts(self) -> np.ndarray:
        """[rows + rows * 5 * 2 * (2 + 4 * 3)] int64: n_pairs, then per cell the counts and every sum's limbs."""
        v = [int(x) for x in self.n_pairs]
        for idx in np.ndindex(self.rows, LAG_CLASSES, ROT_VECS):
            v += [int(getattr(self, name)[idx]) for name in ROT_COUNTS]
            for name in ROT_SUMS:
                x = int(getattr(self, name)[idx])
                v += [x >> 32 * k & 0xFFFFFFFF for k in range(LAG_LIMBS - 1)] + [x >> 32 * (LAG_LIMBS - 1)]
        return np.array(v, dtype=np.int64)

    def from_counts(self, counts) -> "RotSample":
        """A sample of this one's configuration holding the (summed) counts() vector."""
        import copy
        s = copy.copy(self)
        it = iter(int(x) for x in np.asarray(counts).ravel())
        s.n_pairs = np.array([next(it) for _ in range(self.rows)], dtype=object)
        shape = (self.rows, LAG_CLASSES, ROT_VECS)
        for name in ROT_COUNTS + ROT_SUMS:
            setattr(s, name, np.zeros(shape, dtype=object))
        for idx in np.ndindex(*shape):
            for name in ROT_COUNTS:
                getattr(s, name)[idx] = next(it)
            for name in ROT_SUMS:
                getattr(s, name)[idx] = sum(next(it) << 32 * k for k in range(LAG_LIMBS))
        return s


class RotArrays:
    """numpy-backed kmc_rot_view for n_a receptors and n_b ligands: vec [n_a + 2 n_b] (headings, axes, arms), links
    [3, n], last_event [n], chi [n], ring [levels, slots, n_a + 2 n_b], table [rows, 5, 2] (ROT_CELL_DTYPE), n_pairs
    [rows]."""

    def __init__(self, n_a: int, n_b: int, levels: int, slots: int):
        rows, n, w = lag_rows(levels, slots), n_a + n_b, n_a + 2 * n_b
        self.vec = np.zeros(w, dtype=np.uint64)
        self.links = np.zeros((3, n), dtype=np.int32)
        self.last_event = np.zeros(n, dtype=np.int32)
        self.chi = np.zeros(n, dtype=np.int8)
        self.ring = np.zeros((levels, slots, w), dtype=np.uint64)
        self.table = np.zeros((rows, LAG_CLASSES, ROT_VECS), dtype=ROT_CELL_DTYPE)
        self.n_pairs = np.zeros(rows, dtype=np.int64)

    def view(self) -> RotView:
        v = RotView()
        for name, ptr in RotView._fields_:
            a = getattr(self, name)
            setattr(v, name, a.ctypes.data if ptr is C.c_void_p else a.ctypes.data_as(ptr))
        return v


DD_ROW = 416     # KMC_DD_ROW: one exchanged protein (48 doubles + 8 int32)
DD_JCAP = 256    # KMC_DD_JCAP
DD_XCAP = 64     # KMC_DD_XCAP


class DDReport(C.Structure):
    """kmc_dd_report — one slab window's checks after a step's halo exchange."""

    _fields_ = [
        ("xcol", C.c_int64),
        ("xbond", C.c_int64),
        ("bad", C.c_int32),
        ("differed", C.c_int32),
        ("links", C.c_int32),
        ("n_jump", C.c_int32),
        ("n_xb", C.c_int32),
        ("reserved", C.c_int32),
        ("jump_id", C.c_int32 * DD_JCAP),
        ("jump_x", C.c_double * DD_JCAP),
        ("xb", (C.c_int32 * 2) * DD_XCAP),
    ]

    def jumpers(self):
        """(local ids, x) of the listed jumpers."""
        n = min(self.n_jump, DD_JCAP)
        return (np.ctypeslib.as_array(self.jump_id)[:n].copy(), np.ctypeslib.as_array(self.jump_x)[:n].copy())

    def cross_bonds(self) -> np.ndarray:
        """[n, 2] local ids of the listed cross-slab bonds."""
        n = min(self.n_xb, DD_XCAP)
        return np.ctypeslib.as_array(self.xb).reshape(-1, 2)[:n].copy()


def default_params(**overrides) -> Params:
    """Reference defaults, main.cpp:39-99 (mirrors kmc_params_default)."""
    p = Params()
    p.n_a, p.n_b = 150, 50
    p.time_step = 10.0
    p.box_x, p.box_y, p.box_z = 5773.0, 5773.0, 1000.0
    p.pai = 3.1415926
    p.ra_radius, p.ra_D, p.ra_rot_D = 20.0, 1.0, 0.0174
    p.rb_radius, p.rb_D, p.rb_rot_D = 30.0, 7.2614, 0.0061209
    p.mono_cis_ass_rate, p.mono_cis_diss_rate = 0.000047, 0.000000000000112
    p.cis_D, p.cis_rot_D, p.cis_ass_rate, p.cis_diss_rate = 0.5, 0.005, 0.00096, 0.000000000000112
    p.bond_D, p.bond_rot_D, p.ass_rate, p.diss_rate = 0.5, 0.005, 0.04, 0.000000000000348
    p.bond_dist_cutoff = 18.0
    p.bond_thetapd_cutoff = 45.0
    p.bond_thetaot_cutoff = 90.0
    p.cis_thetaot_cutoff = 10.0
    p.cis_dist_cutoff = 15.0
    p.simu_step = 20000000
    p.out_interval = 5000
    p.seed = 1
    p.replica = 0
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


ENC_SLOTS, ENC_BINS, ENC_HISTS = 4, 256, 9    # KMC_ENC_SLOTS / KMC_ENC_BINS / KMC_ENC_HISTS
ENC_CENSORED, ENC_GEMINATE, ENC_REACTIVE, ENC_WAS_REACTIVE = 1, 2, 4, 8  # KMC_ENC_* (bits of a slot)
REACH_RL, REACH_MONO, REACH_CX = 0, 1, 2      # KMC_REACH_* (channels of the reach census)
REACH_MAX_ND, REACH_MAX_NA = 64, 36           # KMC_REACH_MAX_ND / KMC_REACH_MAX_NA
REACH_CHANNELS = ("rl", "mono", "cx")
# rows of the encounter histogram
ENC_ROWS = ("bound", "separated", "lost_receptor", "lost_site", "censored_ended", "gem_rebound", "gem_escaped",
            "gem_lost", "alive")


class ReachOut(C.Structure):
    """kmc_reach_out — the reach census' counts: n_reach, n_reactive per channel (RL, MONO, CX) and the R–L summary."""

    _fields_ = [("n_reach", C.c_int64 * 3), ("n_reactive", C.c_int64 * 3)] + [(name, C.c_int64) for name in (
        "rl_free_receptors", "rl_free_sites", "rl_receptors_in_reach", "rl_sites_in_reach", "rl_max_partners")]

    def as_dict(self) -> dict:
        d = {"n_reach": [int(x) for x in self.n_reach], "n_reactive": [int(x) for x in self.n_reactive]}
        d.update({name: int(getattr(self, name)) for name, _ in self._fields_[2:]})
        return d


class EncConfig(C.Structure):
    """kmc_enc_config — steps between two updates of the encounter recorder."""

    _fields_ = [("every", C.c_int32), ("reserved", C.c_int32)]


def enc_config(every: int = 1) -> EncConfig:
    c = EncConfig()
    c.every = int(every)
    return c


class EncOut(C.Structure):
    """kmc_enc_out — steps, event counters, exposures and occupancy of the encounter recorder."""

    _fields_ = [(name, C.c_int64) for name in (
        "origin_step", "last_step", "n_updates",
        "on_from_encounter", "on_direct", "n_opened", "n_ended",
        "exp_reach", "exp_reactive", "exp_free_receptor",
        "n_overflow",
        "occ_reach", "occ_reactive", "occ_free_receptor",
        "n_censored_alive",
        "every", "slots")]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class EncView(C.Structure):
    """kmc_enc_view — caller-owned per-receptor arrays of the encounter recorder."""

    _fields_ = [
        ("lig", C.POINTER(C.c_int32)),
        ("site", C.POINTER(C.c_int32)),
        ("key", C.POINTER(C.c_int32)),
        ("since", C.POINTER(C.c_int64)),
        ("nreact", C.POINTER(C.c_int32)),
        ("flags", C.POINTER(C.c_uint8)),
    ]


class EncArrays:
    """numpy-backed kmc_enc_view for n_a receptors: lig, site [n_a] and key, since, nreact, flags [n_a, ENC_SLOTS]."""

    DTYPES = dict(lig=np.int32, site=np.int32, key=np.int32, since=np.int64, nreact=np.int32, flags=np.uint8)

    def __init__(self, n_a: int):
        for name, dt in self.DTYPES.items():
            shape = (n_a,) if name in ("lig", "site") else (n_a, ENC_SLOTS)
            setattr(self, name, np.zeros(shape, dtype=dt))

    def view(self) -> EncView:
        v = EncView()
        for name, ptr in EncView._fields_:
            setattr(v, name, getattr(self, name).ctypes.data_as(ptr))
        return v


class EncSample:
    """One kmc_enc_sample: out (capi.EncOut), hist [ENC_HISTS, ENC_BINS] and react_hist [2, ENC_BINS] int64.
    counts(): the sample as one int64 vector that adds over replicas (analysis.reduce_counts) — the counters
    (steps and configuration excluded), then the two histograms."""

    ADDITIVE = ("n_updates", "on_from_encounter", "on_direct", "n_opened", "n_ended", "exp_reach", "exp_reactive",
                "exp_free_receptor", "n_overflow", "occ_reach", "occ_reactive", "occ_free_receptor",
                "n_censored_alive")

    def __init__(self, out: EncOut, hist: np.ndarray, react_hist: np.ndarray):
        self.out, self.hist, self.react_hist = out, hist, react_hist

    def as_dict(self) -> dict:
        return self.out.as_dict()

    def counts(self) -> np.ndarray:
        d = self.out.as_dict()
        return np.concatenate([np.array([d[k] for k in self.ADDITIVE], dtype=np.int64), self.hist.ravel(),
                               self.react_hist.ravel()])

    @classmethod
    def from_counts(cls, counts) -> "EncSample":
        v = np.asarray(counts, dtype=np.int64)
        n = len(cls.ADDITIVE)
        out = EncOut()
        for k, x in zip(cls.ADDITIVE, v[:n]):
            setattr(out, k, int(x))
        h = v[n:n + ENC_HISTS * ENC_BINS].reshape(ENC_HISTS, ENC_BINS).copy()
        r = v[n + ENC_HISTS * ENC_BINS:].reshape(2, ENC_BINS).copy()
        return cls(out, h, r)


PX_A, PX_B, PX_AB = 0, 1, 2           # KMC_PX_A / KMC_PX_B / KMC_PX_AB (the point set of kmc_prox_clusters)
PX_NN_ROWS = 64                       # KMC_PX_NN_ROWS: neighbour counts clamp into the last bin
PX_MAX_SIZE, PX_NND_BINS = 65535, 4096  # KMC_PX_MAX_SIZE / KMC_PX_NND_BINS
PX_WHICH = {"A": PX_A, "B": PX_B, "AB": PX_AB}


def px_which(which) -> int:
    """'A' / 'B' / 'AB' or the KMC_PX_* number itself."""
    return PX_WHICH[which] if isinstance(which, str) else int(which)


class ProxOut(C.Structure):
    """kmc_prox_out — the counts of kmc_prox_clusters: the points by kind, the clusters, the pairs, the purity
    against the bond graph and the largest cluster."""

    _fields_ = [(name, C.c_int64) for name in (
        "n_sel", "n_core", "n_border", "n_noise", "n_alone", "n_clusters",
        "n_multi", "sum_nn", "n_core_edges",
        "n_pure", "n_whole", "n_bond_multi", "n_bond_kept")] + [("max_size", C.c_int32), ("max_label", C.c_int32)]

    # the fields that add over replicas and successive calls (the largest cluster does not)
    ADDITIVE = tuple(name for name, _ in _fields_[:13])

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}

    def counts(self) -> np.ndarray:
        """The additive fields as one int64 vector (analysis.reduce_counts)."""
        return np.array([int(getattr(self, k)) for k in self.ADDITIVE], dtype=np.int64)


class HostState:
    """numpy-backed kmc_state_view for n_a receptors and n_b ligands."""

    def __init__(self, n_a: int, n_b: int):
        self.n_a, self.n_b = n_a, n_b
        self.ra = np.zeros((48, n_a), dtype=np.float64)
        self.rb = np.zeros((24, n_b), dtype=np.float64)
        self.a_int = np.zeros((5, n_a), dtype=np.int32)
        self.b_int = np.zeros((8, n_b), dtype=np.int32)
        self.counters = np.zeros(5, dtype=np.int32)
        self.step = 0

    def view(self) -> StateView:
        v = StateView()
        v.ra = self.ra.ctypes.data_as(C.POINTER(C.c_double))
        v.rb = self.rb.ctypes.data_as(C.POINTER(C.c_double))
        v.a_int = self.a_int.ctypes.data_as(C.POINTER(C.c_int32))
        v.b_int = self.b_int.ctypes.data_as(C.POINTER(C.c_int32))
        for i in range(5):
            v.counters[i] = int(self.counters[i])
        v.step = int(self.step)
        return v

    def pull(self, v: StateView) -> None:
        self.counters[:] = list(v.counters)
        self.step = int(v.step)

    def copy(self) -> "HostState":
        h = HostState(self.n_a, self.n_b)
        h.ra[:] = self.ra
        h.rb[:] = self.rb
        h.a_int[:] = self.a_int
        h.b_int[:] = self.b_int
        h.counters[:] = self.counters
        h.step = self.step
        return h

    def equal(self, other: "HostState") -> bool:
        """Bitwise equality (coordinates compared as IEEE bit patterns)."""
        return (
            np.array_equal(self.ra.view(np.uint64), other.ra.view(np.uint64))
            and np.array_equal(self.rb.view(np.uint64), other.rb.view(np.uint64))
            and np.array_equal(self.a_int, other.a_int)
            and np.array_equal(self.b_int, other.b_int)
            and np.array_equal(self.counters, other.counters)
            and self.step == other.step
        )


def _fnv_bytes(h: int, data: bytes) -> int:
    for c in data:
        h ^= c
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
