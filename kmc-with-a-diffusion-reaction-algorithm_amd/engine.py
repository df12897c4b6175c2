"""Python host mirror of the reference's step-loop contract over libkmc.

The reference is one process that owns its state in globals and talks
through files (main.cpp:169-278, 2206-2305).  `Simulation` is the same
contract as an object: construct with the physics parameters (the
reference's compile-time globals, main.cpp:39-99), obtain an initial state
(random placement, main.cpp:281-447, or position.cpt, main.cpp:226-270),
advance the diffusion–reaction loop (main.cpp:461-2308) on the GPU, read the
bond.dat observables, write position.cpt.

Everything runs in libkmc (HIP kernels on gfx950); this module only
marshals host buffers.  There is no CPU fallback: if the library or a gfx950
device is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import capi

_lib = None


class KmcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{capi.ERRORS.get(code, code)}: {msg}")
        self.code = code


def load_library(path: Optional[str] = None):
    """Load libkmc.so (built in-tree by build.py).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or capi.LIB_PATH
    if not os.path.exists(path):
        raise KmcError(-9, f"{path} not built (run __graft_entry__.build())")
    L = C.CDLL(path)
    P = C.POINTER
    L.kmc_params_default.argtypes = [P(capi.Params)]
    L.kmc_create.argtypes = [P(capi.Params), C.c_int, P(C.c_void_p)]
    L.kmc_destroy.argtypes = [C.c_void_p]
    L.kmc_last_error.restype = C.c_char_p
    L.kmc_last_error.argtypes = [C.c_void_p]
    L.kmc_init_random.argtypes = [C.c_void_p]
    L.kmc_load_cpt.argtypes = [C.c_void_p, C.c_char_p]
    L.kmc_write_cpt.argtypes = [C.c_void_p, C.c_char_p]
    L.kmc_set_state.argtypes = [C.c_void_p, P(capi.StateView)]
    L.kmc_get_state.argtypes = [C.c_void_p, P(capi.StateView)]
    L.kmc_step.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.kmc_current_step.restype = C.c_int64
    L.kmc_current_step.argtypes = [C.c_void_p]
    L.kmc_set_timing.argtypes = [C.c_void_p, C.c_uint64]
    L.kmc_set_timing_period.argtypes = [C.c_void_p, C.c_int32]
    L.kmc_kernel_times.argtypes = [C.c_void_p, P(C.c_double), P(C.c_int64), C.c_int32]
    L.kmc_kernel_name.restype = C.c_char_p
    L.kmc_kernel_name.argtypes = [C.c_int32]
    L.kmc_format_bond_line.argtypes = [P(capi.Params), P(capi.Obs), C.c_char_p, C.c_size_t]
    L.kmc_state_hash.restype = C.c_uint64
    L.kmc_state_hash.argtypes = [P(capi.Params), P(capi.StateView)]
    L.kmc_host_last_error.restype = C.c_char_p
    L.kmc_host_load_cpt.argtypes = [P(capi.Params), C.c_char_p, P(capi.StateView)]
    L.kmc_host_write_cpt.argtypes = [P(capi.Params), P(capi.StateView), C.c_char_p]
    L.kmc_host_init_random.argtypes = [P(capi.Params), P(capi.StateView)]
    L.kmc_host_validate.argtypes = [P(capi.Params), P(capi.StateView)]
    L.kmc_host_check_params.argtypes = [P(capi.Params)]
    L.kmc_host_dd_check.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    L.kmc_host_save_state.argtypes = [P(capi.Params), P(capi.StateView), C.c_char_p]
    L.kmc_host_load_state.argtypes = [P(capi.Params), C.c_char_p, P(capi.StateView)]
    L.kmc_save_state.argtypes = [C.c_void_p, C.c_char_p]
    L.kmc_load_state.argtypes = [C.c_void_p, C.c_char_p]
    L.kmc_get_clusters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_host_write_parameter_log.argtypes = [P(capi.Params), C.c_char_p]
    L.kmc_host_append_gro.argtypes = [P(capi.Params), P(capi.StateView), C.c_char_p]
    L.kmc_host_append_cluster_log.argtypes = [P(capi.Params), C.c_int64, C.c_void_p, C.c_void_p, C.c_char_p]
    L.kmc_dd_set_state.argtypes = [C.c_void_p, P(capi.StateView), C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_dd_export.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_dd_import.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_dd_drift.argtypes = [C.c_void_p, P(C.c_double)]
    L.kmc_dd_counters.argtypes = [C.c_void_p, C.c_void_p]
    L.kmc_dd_jumpers.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, P(C.c_int32)]
    L.kmc_dd_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_dd_pack.argtypes = [C.c_void_p, C.c_void_p]
    L.kmc_dd_send_buffer.restype = C.c_void_p
    L.kmc_dd_send_buffer.argtypes = [C.c_void_p]
    L.kmc_dd_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    L.kmc_dd_finish.argtypes = [C.c_void_p, P(capi.DDReport)]
    L.kmc_dd_step.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    L.kmc_dd_cut_count.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, P(C.c_int32)]
    L.kmc_list_growth.argtypes = [C.c_void_p]
    L.kmc_set_list_growth.argtypes = [C.c_void_p, C.c_int32]
    L.kmc_components.argtypes = [C.c_void_p, C.c_void_p]
    L.kmc_oligomer_census.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, P(capi.Census)]
    L.kmc_pair_counts.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p]
    L.kmc_host_census.argtypes = [P(capi.Params), P(capi.StateView), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                  P(capi.Census)]
    L.kmc_analysis_ms.restype = C.c_double
    L.kmc_analysis_ms.argtypes = [C.c_void_p]
    L.kmc_track_begin.argtypes = [C.c_void_p, C.c_double]
    L.kmc_track_update.argtypes = [C.c_void_p, P(capi.TrackInfo)]
    L.kmc_track_sample.argtypes = [C.c_void_p, C.c_double, C.c_int32, P(capi.TrackSample), C.c_void_p]
    L.kmc_track_displacements.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_track_end.argtypes = [C.c_void_p]
    L.kmc_kin_begin.argtypes = [C.c_void_p]
    L.kmc_kin_update.argtypes = [C.c_void_p, P(capi.KinOut)]
    L.kmc_kin_sample.argtypes = [C.c_void_p, P(capi.KinOut), C.c_void_p]
    L.kmc_kin_get.argtypes = [C.c_void_p, P(capi.KinView)]
    L.kmc_kin_end.argtypes = [C.c_void_p]
    L.kmc_host_kin_begin.argtypes = [P(capi.Params), P(capi.StateView), P(capi.KinView), P(capi.KinOut), C.c_void_p]
    L.kmc_host_kin_update.argtypes = [P(capi.Params), P(capi.StateView), P(capi.KinView), P(capi.KinOut), C.c_void_p]
    L.kmc_host_kin_sample.argtypes = [P(capi.Params), P(capi.KinView), P(capi.KinOut), C.c_void_p, P(capi.KinOut),
                                      C.c_void_p]
    L.kmc_cf_begin.argtypes = [C.c_void_p, C.c_int32]
    L.kmc_cf_update.argtypes = [C.c_void_p, P(capi.CfOut)]
    L.kmc_cf_sample.argtypes = [C.c_void_p, P(capi.CfOut), P(capi.CfTablesView)]
    L.kmc_cf_get.argtypes = [C.c_void_p, P(capi.CfView)]
    L.kmc_cf_put.argtypes = [C.c_void_p, P(capi.CfView), C.c_int64]
    L.kmc_cf_end.argtypes = [C.c_void_p]
    L.kmc_host_cf_begin.argtypes = [P(capi.Params), P(capi.StateView), C.c_int32, P(capi.CfView), P(capi.CfOut),
                                    P(capi.CfTablesView)]
    L.kmc_host_cf_update.argtypes = [P(capi.Params), P(capi.StateView), P(capi.CfView), P(capi.CfOut),
                                     P(capi.CfTablesView)]
    L.kmc_host_cf_sample.argtypes = [P(capi.Params), P(capi.CfView), P(capi.CfOut), P(capi.CfTablesView),
                                     P(capi.CfOut), P(capi.CfTablesView)]
    L.kmc_unwrap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_cluster_geometry.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, P(capi.Geom)]
    L.kmc_cluster_list.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, P(C.c_int64)]
    L.kmc_host_cluster_geometry.argtypes = [P(capi.Params), P(capi.StateView), C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_void_p, P(capi.Geom)]
    L.kmc_structure_factor.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.kmc_host_structure_factor.argtypes = [P(capi.Params), P(capi.StateView), C.c_int32, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p]
    bo = [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32]  # which, mode, fold, r_cut, select
    bo_local = bo + [C.c_int32, C.c_void_p, P(capi.BondOrderOut), C.c_void_p, C.c_void_p, C.c_void_p]
    bo_corr = bo + [C.c_double, C.c_int32, C.c_void_p]
    L.kmc_bond_order.argtypes = [C.c_void_p] + bo_local
    L.kmc_bond_order_corr.argtypes = [C.c_void_p] + bo_corr
    L.kmc_host_bond_order.argtypes = [P(capi.Params), P(capi.StateView)] + bo_local
    L.kmc_host_bond_order_corr.argtypes = [P(capi.Params), P(capi.StateView)] + bo_corr
    net = [P(capi.NetOut), C.c_void_p, C.c_void_p, C.c_void_p]  # out, lig_hist, adj_lig, adj_site
    rings = [C.c_int32, C.c_void_p, C.c_void_p, P(capi.NetOut)]  # max_len, counts, member, out
    L.kmc_network.argtypes = [C.c_void_p] + net
    L.kmc_rings.argtypes = [C.c_void_p] + rings
    L.kmc_rings_hops.restype = C.c_int64
    L.kmc_rings_hops.argtypes = [C.c_void_p]
    L.kmc_host_network.argtypes = [P(capi.Params), P(capi.StateView)] + net
    L.kmc_host_rings.argtypes = [P(capi.Params), P(capi.StateView)] + rings
    L.kmc_lag_begin.argtypes = [C.c_void_p, P(capi.LagConfig)]
    L.kmc_lag_update.argtypes = [C.c_void_p, P(capi.LagInfo)]
    L.kmc_lag_sample.argtypes = [C.c_void_p, P(capi.LagOut), C.c_void_p, C.c_void_p]
    L.kmc_lag_arrays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_lag_end.argtypes = [C.c_void_p]
    L.kmc_pd_begin.argtypes = [C.c_void_p, P(capi.PdConfig)]
    L.kmc_pd_update.argtypes = [C.c_void_p, P(capi.PdInfo)]
    L.kmc_pd_sample.argtypes = [C.c_void_p, P(capi.PdOut), C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_pd_arrays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_pd_end.argtypes = [C.c_void_p]
    L.kmc_host_pd_begin.argtypes = [P(capi.Params), P(capi.StateView), P(capi.PdConfig), P(capi.PdView), P(capi.PdOut)]
    L.kmc_host_pd_update.argtypes = [P(capi.Params), P(capi.StateView), P(capi.PdView), P(capi.PdOut), P(capi.PdInfo)]
    L.kmc_host_pd_sample.argtypes = [P(capi.Params), P(capi.PdView), P(capi.PdOut), P(capi.PdOut), C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    L.kmc_bd_begin.argtypes = [C.c_void_p, P(capi.BdConfig)]
    L.kmc_bd_update.argtypes = [C.c_void_p, P(capi.BdInfo)]
    L.kmc_bd_sample.argtypes = [C.c_void_p, P(capi.BdOut), C.c_void_p]
    L.kmc_bd_sample_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.kmc_bd_bodies.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, P(C.c_int64)]
    L.kmc_bd_arrays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_bd_get.argtypes = [C.c_void_p, P(capi.BdView)]
    L.kmc_bd_put.argtypes = [C.c_void_p, P(capi.BdView), C.c_int64]
    L.kmc_bd_end.argtypes = [C.c_void_p]
    L.kmc_host_bd_begin.argtypes = [P(capi.Params), P(capi.StateView), P(capi.BdConfig), P(capi.BdView), P(capi.BdOut)]
    L.kmc_host_bd_update.argtypes = [P(capi.Params), P(capi.StateView), P(capi.BdView), P(capi.BdOut), P(capi.BdInfo)]
    L.kmc_host_bd_sample.argtypes = [P(capi.Params), P(capi.StateView), P(capi.BdView), P(capi.BdOut), P(capi.BdOut),
                                     C.c_void_p]
    L.kmc_host_bd_bodies.argtypes = [P(capi.Params), P(capi.StateView), P(capi.BdView), P(capi.BdOut), C.c_int32,
                                     C.c_int64, C.c_void_p, P(C.c_int64)]
    L.kmc_host_lag_begin.argtypes = [P(capi.Params), P(capi.StateView), P(capi.LagConfig), P(capi.LagView),
                                     P(capi.LagOut)]
    L.kmc_host_lag_update.argtypes = [P(capi.Params), P(capi.StateView), P(capi.LagView), P(capi.LagOut),
                                      P(capi.LagInfo)]
    L.kmc_host_lag_sample.argtypes = [P(capi.Params), P(capi.LagView), P(capi.LagOut), P(capi.LagOut), C.c_void_p,
                                      C.c_void_p]
    L.kmc_rot_begin.argtypes = [C.c_void_p, P(capi.RotConfig)]
    L.kmc_rot_update.argtypes = [C.c_void_p, P(capi.RotInfo)]
    L.kmc_rot_sample.argtypes = [C.c_void_p, P(capi.RotOut), C.c_void_p, C.c_void_p]
    L.kmc_rot_arrays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_rot_end.argtypes = [C.c_void_p]
    L.kmc_ligand_pose.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, P(capi.PoseOut)]
    L.kmc_host_rot_begin.argtypes = [P(capi.Params), P(capi.StateView), P(capi.RotConfig), P(capi.RotView),
                                     P(capi.RotOut)]
    L.kmc_host_rot_update.argtypes = [P(capi.Params), P(capi.StateView), P(capi.RotView), P(capi.RotOut),
                                      P(capi.RotInfo)]
    L.kmc_host_rot_sample.argtypes = [P(capi.Params), P(capi.RotView), P(capi.RotOut), P(capi.RotOut), C.c_void_p,
                                      C.c_void_p]
    L.kmc_host_ligand_pose.argtypes = [P(capi.Params), P(capi.StateView), C.c_int32, C.c_int32, C.c_void_p,
                                       P(capi.PoseOut)]
    L.kmc_reach_census.argtypes = [C.c_void_p, C.c_int32, C.c_int32, P(capi.ReachOut), C.c_void_p, C.c_void_p,
                                   C.c_void_p]
    L.kmc_enc_begin.argtypes = [C.c_void_p, P(capi.EncConfig)]
    L.kmc_enc_update.argtypes = [C.c_void_p, P(capi.EncOut)]
    L.kmc_enc_sample.argtypes = [C.c_void_p, P(capi.EncOut), C.c_void_p, C.c_void_p]
    L.kmc_enc_arrays.argtypes = [C.c_void_p, P(capi.EncView)]
    L.kmc_enc_end.argtypes = [C.c_void_p]
    L.kmc_enc_phase_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.kmc_host_reach_census.argtypes = [P(capi.Params), P(capi.StateView), C.c_int32, C.c_int32, P(capi.ReachOut),
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmc_host_enc_begin.argtypes = [P(capi.Params), P(capi.StateView), P(capi.EncConfig), P(capi.EncView),
                                     P(capi.EncOut), C.c_void_p]
    L.kmc_host_enc_update.argtypes = [P(capi.Params), P(capi.StateView), P(capi.EncView), P(capi.EncOut), C.c_void_p]
    L.kmc_host_enc_sample.argtypes = [P(capi.Params), P(capi.EncView), P(capi.EncOut), C.c_void_p, P(capi.EncOut),
                                      C.c_void_p, C.c_void_p]
    px = [C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_int32, P(capi.ProxOut)] + \
        [C.c_void_p] * 6
    L.kmc_prox_clusters.argtypes = [C.c_void_p] + px
    L.kmc_host_prox_clusters.argtypes = [P(capi.Params), P(capi.StateView)] + px
    L.kmc_prox_phase_ms.argtypes = [C.c_void_p, C.c_void_p]
    for f in ("kmc_host_math", "kmc_device_math"):
        getattr(L, f).argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    _lib = L
    return L


def _host_check(rc: int):
    if rc != 0:
        raise KmcError(rc, load_library().kmc_host_last_error().decode())


# ---------------------------------------------------------------- host-only
def host_init_random(params: capi.Params) -> capi.HostState:
    """Random placement (main.cpp:281-447, keyed draws) into host buffers."""
    hs = capi.HostState(params.n_a, params.n_b)
    v = hs.view()
    _host_check(load_library().kmc_host_init_random(C.byref(params), C.byref(v)))
    hs.pull(v)
    return hs


def host_load_cpt(params: capi.Params, path: str) -> capi.HostState:
    """position.cpt → host state (main.cpp:226-270)."""
    hs = capi.HostState(params.n_a, params.n_b)
    v = hs.view()
    _host_check(load_library().kmc_host_load_cpt(C.byref(params), os.fsencode(path), C.byref(v)))
    hs.pull(v)
    return hs


def host_write_cpt(params: capi.Params, hs: capi.HostState, path: str) -> None:
    """host state → position.cpt (main.cpp:2206-2244)."""
    v = hs.view()
    _host_check(load_library().kmc_host_write_cpt(C.byref(params), C.byref(v), os.fsencode(path)))


def host_save_state(params: capi.Params, hs: capi.HostState, path: str) -> None:
    """host state → exact binary checkpoint (KMCSTAT1, include/kmc.h)."""
    v = hs.view()
    _host_check(load_library().kmc_host_save_state(C.byref(params), C.byref(v), os.fsencode(path)))


def host_load_state(params: capi.Params, path: str) -> capi.HostState:
    """exact binary checkpoint → host state (refuses another trajectory's file)."""
    hs = capi.HostState(params.n_a, params.n_b)
    v = hs.view()
    _host_check(load_library().kmc_host_load_state(C.byref(params), os.fsencode(path), C.byref(v)))
    hs.pull(v)
    return hs


def host_validate(params: capi.Params, hs: capi.HostState) -> int:
    v = hs.view()
    return int(load_library().kmc_host_validate(C.byref(params), C.byref(v)))


def host_check_params(params: capi.Params) -> int:
    """The parameter envelope kmc_create accepts (include/kmc.h): KMC_OK or KMC_ERR_ARG."""
    return int(load_library().kmc_host_check_params(C.byref(params)))


def host_census(params: capi.Params, hs: capi.HostState, max_r: int, max_l: int):
    """Components of a host state's bond graph, sequentially (kmc_host_census):
    (label[n_a + n_b] 1-based, hist[max_r + 1, max_l + 1] int64, capi.Census)."""
    label = np.zeros(params.n_a + params.n_b, dtype=np.int32)
    hist = np.zeros((max_r + 1, max_l + 1), dtype=np.int64)
    out = capi.Census()
    v = hs.view()
    _host_check(load_library().kmc_host_census(C.byref(params), C.byref(v), label.ctypes.data, max_r, max_l,
                                               hist.ctypes.data, C.byref(out)))
    return label, hist, out


def host_cluster_geometry(params: capi.Params, hs: capi.HostState, max_size: int):
    """Cluster geometry of a host state, sequentially (kmc_host_cluster_geometry): (label[N] 1-based,
    shift[N, 2] int32, span[N] uint8, table[max_size + 1] capi.GEOM_BIN_DTYPE, capi.Geom)."""
    n = params.n_a + params.n_b
    label = np.zeros(n, dtype=np.int32)
    shift = np.zeros((2, n), dtype=np.int32)
    span = np.zeros(n, dtype=np.uint8)
    table = np.zeros(max(int(max_size), 0) + 1, dtype=capi.GEOM_BIN_DTYPE)
    out = capi.Geom()
    v = hs.view()
    _host_check(load_library().kmc_host_cluster_geometry(C.byref(params), C.byref(v), label.ctypes.data,
                                                         shift.ctypes.data, span.ctypes.data, int(max_size),
                                                         table.ctypes.data, C.byref(out)))
    return label, np.ascontiguousarray(shift.T), span, table, out


def _sk_buffers(hmax: int, kmax: int):
    """(sums[4, hmax + 1, 2 kmax + 1] int64, n_sel[2] int64) for a structure factor call; a grid out of range
    gets the smallest buffers (the library refuses the call before it writes)."""
    ok = 0 <= int(hmax) <= capi.SK_MAX and 0 <= int(kmax) <= capi.SK_MAX
    shape = (4, int(hmax) + 1, 2 * int(kmax) + 1) if ok else (4, 1, 1)
    return np.zeros(shape, dtype=np.int64), np.zeros(2, dtype=np.int64)


def host_structure_factor(params: capi.Params, hs: capi.HostState, hmax: int, kmax: int, select="all"):
    """Structure factor sums of a host state, sequentially (kmc_host_structure_factor): (sums[4, hmax + 1,
    2 kmax + 1] int64 — C_A, S_A, C_B, S_B —, n_sel[2] int64), as Simulation.structure_factor."""
    sums, n_sel = _sk_buffers(hmax, kmax)
    v = hs.view()
    _host_check(load_library().kmc_host_structure_factor(C.byref(params), C.byref(v), int(hmax), int(kmax),
                                                         capi.sk_select(select), sums.ctypes.data,
                                                         n_sel.ctypes.data))
    return sums, n_sel


def _bo_args(which, fold, r_cut, mode, select):
    """The five arguments both bond order calls share, as the library takes them (r_cut None: 0.0, which only the
    linked mode accepts)."""
    return (capi.bo_which(which), capi.bo_mode(mode), int(fold), 0.0 if r_cut is None else float(r_cut),
            capi.sk_select(select))


def _bo_call(f, head, n, which, fold, r_cut, mode, select, nbins, per_protein):
    """One kmc_bond_order / kmc_host_bond_order call: (hist[16, nbins] int64, capi.BondOrderOut) and, with
    per_protein, (C[n], S[n] int64, nn[n] int32) by the species' reference index; a bin count out of range gets the
    smallest buffer (the library refuses the call before it writes)."""
    ok = 1 <= int(nbins) <= capi.BO_HIST_BINS
    hist = np.zeros((capi.BO_NN_ROWS, int(nbins) if ok else 1), dtype=np.int64)
    out = capi.BondOrderOut()
    Cs, Ss, nn = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    ptr = (lambda a: a.ctypes.data if per_protein and n else None)
    rc = f(*head, *_bo_args(which, fold, r_cut, mode, select), int(nbins), hist.ctypes.data, C.byref(out), ptr(Cs),
           ptr(Ss), ptr(nn))
    return rc, ((hist, out, Cs, Ss, nn) if per_protein else (hist, out))


def host_bond_order(params: capi.Params, hs: capi.HostState, which, fold: int, r_cut=None, mode="within",
                    select="all", nbins: int = 64, per_protein: bool = False):
    """Bond-orientational order of a host state, sequentially (kmc_host_bond_order): as Simulation.bond_order."""
    v = hs.view()
    n = params.n_a if capi.bo_which(which) == capi.BO_A else params.n_b
    rc, res = _bo_call(load_library().kmc_host_bond_order, (C.byref(params), C.byref(v)), n, which, fold, r_cut, mode,
                       select, nbins, per_protein)
    _host_check(rc)
    return res


def host_bond_order_corr(params: capi.Params, hs: capi.HostState, which, fold: int, r_max: float, r_cut=None,
                         mode="within", select="all", nbins: int = 64) -> np.ndarray:
    """corr[2, nbins] int64 of a host state, sequentially (kmc_host_bond_order_corr): as
    Simulation.bond_order_corr."""
    v = hs.view()
    corr = np.zeros((2, int(nbins) if 1 <= int(nbins) <= capi.BO_CORR_BINS else 1), dtype=np.int64)
    _host_check(load_library().kmc_host_bond_order_corr(C.byref(params), C.byref(v),
                                                        *_bo_args(which, fold, r_cut, mode, select), float(r_max),
                                                        int(nbins), corr.ctypes.data))
    return corr


def _net_call(f, head, n_b):
    """One kmc_network / kmc_host_network call: rc and (capi.NetOut, lig_hist[4, 4] int64, adj_lig[n_b, 3] int32,
    adj_site[n_b, 3] int32)."""
    out = capi.NetOut()
    hist = np.zeros((4, 4), dtype=np.int64)
    adj_lig, adj_site = np.zeros((n_b, 3), dtype=np.int32), np.zeros((n_b, 3), dtype=np.int32)
    rc = f(*head, C.byref(out), hist.ctypes.data, adj_lig.ctypes.data if n_b else None,
           adj_site.ctypes.data if n_b else None)
    return rc, (out, hist, adj_lig, adj_site)


def _rings_call(f, head, n_b, max_len, members):
    """One kmc_rings / kmc_host_rings call: rc and (counts[2, RING_MAX + 1] int64, capi.NetOut) or, with members,
    (counts, member[2, n_b] uint32, capi.NetOut)."""
    out = capi.NetOut()
    counts = np.zeros((2, capi.RING_MAX + 1), dtype=np.int64)
    member = np.zeros((2, n_b), dtype=np.uint32)
    rc = f(*head, int(max_len), counts.ctypes.data, member.ctypes.data if members and n_b else None, C.byref(out))
    return rc, ((counts, member, out) if members else (counts, out))


def host_network(params: capi.Params, hs: capi.HostState):
    """The ligand network of a host state, sequentially (kmc_host_network): as Simulation.network."""
    v = hs.view()
    rc, res = _net_call(load_library().kmc_host_network, (C.byref(params), C.byref(v)), params.n_b)
    _host_check(rc)
    return res


def host_rings(params: capi.Params, hs: capi.HostState, max_len: int = 8, members: bool = False):
    """The rings of a host state's ligand network, sequentially (kmc_host_rings): as Simulation.rings."""
    v = hs.view()
    rc, res = _rings_call(load_library().kmc_host_rings, (C.byref(params), C.byref(v)), params.n_b, max_len, members)
    _host_check(rc)
    return res


def _reach_call(f, head, nd, na):
    """One kmc_reach_census / kmc_host_reach_census call: rc and (capi.ReachOut, hist_d[3, 2, nd], hist_a_rl[na, na],
    hist_a_cis[2, na], int64)."""
    ok = 1 <= nd <= capi.REACH_MAX_ND and 1 <= na <= capi.REACH_MAX_NA
    out = capi.ReachOut()
    hist_d = np.zeros((3, 2, nd) if ok else (1,), dtype=np.int64)
    hist_a_rl = np.zeros((na, na) if ok else (1,), dtype=np.int64)
    hist_a_cis = np.zeros((2, na) if ok else (1,), dtype=np.int64)
    rc = f(*head, int(nd), int(na), C.byref(out), hist_d.ctypes.data, hist_a_rl.ctypes.data, hist_a_cis.ctypes.data)
    return rc, (out, hist_d, hist_a_rl, hist_a_cis)


def host_reach_census(params: capi.Params, hs: capi.HostState, nd: int = 16, na: int = 18):
    """The reach census of a host state, sequentially (kmc_host_reach_census): as Simulation.reach_census."""
    v = hs.view()
    rc, res = _reach_call(load_library().kmc_host_reach_census, (C.byref(params), C.byref(v)), nd, na)
    _host_check(rc)
    return res


def _prox_call(f, head, n, which, eps, min_pts, select, mask, max_size, nbins, per_protein):
    """One kmc_prox_clusters / kmc_host_prox_clusters call: rc and (size_hist[max_size + 1], nn_hist[64],
    nnd_hist[nbins] int64, capi.ProxOut) and, with per_protein, (label[n], nn[n] int32, kind[n] uint8) by reference
    index; a size out of range gets the smallest buffer (the library refuses the call before it writes)."""
    ok = 1 <= int(max_size) <= capi.PX_MAX_SIZE and 1 <= int(nbins) <= capi.PX_NND_BINS
    size_hist = np.zeros(int(max_size) + 1 if ok else 1, dtype=np.int64)
    nn_hist = np.zeros(capi.PX_NN_ROWS, dtype=np.int64)
    nnd_hist = np.zeros(int(nbins) if ok else 1, dtype=np.int64)
    out = capi.ProxOut()
    label, nn, kind = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != (n,):
            raise ValueError("prox_clusters: mask has n_a + n_b entries, by reference index")
    ptr = (lambda a: a.ctypes.data if per_protein and n else None)
    rc = f(*head, capi.px_which(which), capi.sk_select(select), m.ctypes.data if m is not None and n else None,
           float(eps), int(min_pts), int(max_size), int(nbins), C.byref(out), size_hist.ctypes.data,
           nn_hist.ctypes.data, nnd_hist.ctypes.data, ptr(label), ptr(nn), ptr(kind))
    res = (size_hist, nn_hist, nnd_hist, out)
    return rc, (res + (label, nn, kind) if per_protein else res)


def host_prox_clusters(params: capi.Params, hs: capi.HostState, which, eps: float, min_pts: int = 1, select="all",
                       mask=None, max_size: int = 256, nbins: int = 64, per_protein: bool = False):
    """Proximity clusters of a host state, sequentially (kmc_host_prox_clusters): as Simulation.prox_clusters."""
    v = hs.view()
    rc, res = _prox_call(load_library().kmc_host_prox_clusters, (C.byref(params), C.byref(v)),
                         params.n_a + params.n_b, which, eps, min_pts, select, mask, max_size, nbins, per_protein)
    _host_check(rc)
    return res


class HostEnc:
    """The encounter recorder on host states, sequentially (kmc_host_enc_*): Simulation.enc_*'s counterpart
    without a device.  The recorder begins at hs; update(hs) advances it to a later state of the trajectory."""

    def __init__(self, params: capi.Params, hs: capi.HostState, cfg: capi.EncConfig = None):
        self.params = params
        self.arrays = capi.EncArrays(params.n_a)
        self.acc = capi.EncOut()
        self.hist = np.zeros((capi.ENC_HISTS - 1 + 2, capi.ENC_BINS), dtype=np.int64)
        cfg = cfg if cfg is not None else capi.enc_config(1)
        v = hs.view()
        _host_check(load_library().kmc_host_enc_begin(C.byref(params), C.byref(v), C.byref(cfg),
                                                      C.byref(self.arrays.view()), C.byref(self.acc),
                                                      self.hist.ctypes.data))

    def update(self, hs: capi.HostState) -> capi.EncOut:
        """Advance the recorder to hs (kmc_host_enc_update); returns the counters as of this update."""
        v = hs.view()
        _host_check(load_library().kmc_host_enc_update(C.byref(self.params), C.byref(v),
                                                       C.byref(self.arrays.view()), C.byref(self.acc),
                                                       self.hist.ctypes.data))
        out = capi.EncOut()
        C.memmove(C.byref(out), C.byref(self.acc), C.sizeof(out))
        return out

    def sample(self) -> capi.EncSample:
        """capi.EncSample as of the last update — kmc_host_enc_sample."""
        out = capi.EncOut()
        hist = np.zeros((capi.ENC_HISTS, capi.ENC_BINS), dtype=np.int64)
        react = np.zeros((2, capi.ENC_BINS), dtype=np.int64)
        _host_check(load_library().kmc_host_enc_sample(C.byref(self.params), C.byref(self.arrays.view()),
                                                       C.byref(self.acc), self.hist.ctypes.data, C.byref(out),
                                                       hist.ctypes.data, react.ctypes.data))
        return capi.EncSample(out, hist, react)


class HostKinetics:
    """The bond kinetics recorder on host states, sequentially (kmc_host_kin_*): Simulation.kin_*'s counterpart
    without a device.  The recorder begins at hs; update(hs) advances it to a later state of the trajectory."""

    def __init__(self, params: capi.Params, hs: capi.HostState):
        self.params = params
        self.arrays = capi.KinArrays(params.n_a)
        self.acc = capi.KinOut()
        self.hist = np.zeros((capi.KIN_HISTS - 2, capi.KIN_BINS), dtype=np.int64)
        v = hs.view()
        _host_check(load_library().kmc_host_kin_begin(C.byref(params), C.byref(v), C.byref(self.arrays.view()),
                                                      C.byref(self.acc), self.hist.ctypes.data))

    def update(self, hs: capi.HostState) -> capi.KinOut:
        """Advance the recorder to hs (kmc_host_kin_update); returns the counters as of this update."""
        v = hs.view()
        _host_check(load_library().kmc_host_kin_update(C.byref(self.params), C.byref(v),
                                                       C.byref(self.arrays.view()), C.byref(self.acc),
                                                       self.hist.ctypes.data))
        out = capi.KinOut()
        C.memmove(C.byref(out), C.byref(self.acc), C.sizeof(out))
        return out

    def sample(self):
        """(capi.KinOut, hist[KIN_HISTS, KIN_BINS] int64) as of the last update — kmc_host_kin_sample."""
        out = capi.KinOut()
        hist = np.zeros((capi.KIN_HISTS, capi.KIN_BINS), dtype=np.int64)
        _host_check(load_library().kmc_host_kin_sample(C.byref(self.params), C.byref(self.arrays.view()),
                                                       C.byref(self.acc), self.hist.ctypes.data, C.byref(out),
                                                       hist.ctypes.data))
        return out, hist


class HostCoag:
    """The cluster growth recorder on host states, sequentially (kmc_host_cf_*): Simulation.cf_*'s counterpart
    without a device.  The recorder begins at hs; update(hs) advances it to a later state of the trajectory.
    arrays (capi.CfArrays) is what Simulation.cf_put takes."""

    def __init__(self, params: capi.Params, hs: capi.HostState, max_size: int):
        self.params = params
        self.arrays = capi.CfArrays(params.n_a, params.n_b)
        self.acc = capi.CfOut()
        self.tables = capi.CfTables(max_size) if 2 <= max_size <= capi.CF_MAX_SIZE else capi.CfTables(2)
        v = hs.view()
        _host_check(load_library().kmc_host_cf_begin(C.byref(params), C.byref(v), int(max_size),
                                                     C.byref(self.arrays.view()), C.byref(self.acc),
                                                     C.byref(self.tables.view())))

    def update(self, hs: capi.HostState) -> capi.CfOut:
        """Advance the recorder to hs (kmc_host_cf_update); returns the counters as of this update."""
        v = hs.view()
        _host_check(load_library().kmc_host_cf_update(C.byref(self.params), C.byref(v), C.byref(self.arrays.view()),
                                                      C.byref(self.acc), C.byref(self.tables.view())))
        out = capi.CfOut()
        C.memmove(C.byref(out), C.byref(self.acc), C.sizeof(out))
        return out

    def sample(self):
        """(capi.CfOut, capi.CfTables) as of the last look — kmc_host_cf_sample; the tables are a copy."""
        out = capi.CfOut()
        t = capi.CfTables(self.tables.max_size)
        _host_check(load_library().kmc_host_cf_sample(C.byref(self.params), C.byref(self.arrays.view()),
                                                      C.byref(self.acc), C.byref(self.tables.view()), C.byref(out),
                                                      C.byref(t.view())))
        return out, t


class HostLag:
    """The lag correlator on host states, sequentially (kmc_host_lag_*): Simulation.lag_*'s counterpart without a
    device.  The recorder begins at hs (update 0); update(hs) advances it to the state `every` steps later.
    arrays (capi.LagArrays) holds its per-protein state, the rings and the table."""

    def __init__(self, params: capi.Params, hs: capi.HostState, config: capi.LagConfig):
        self.params = params
        ok = 1 <= config.levels <= capi.LAG_MAX_LEVELS and 2 <= config.slots <= capi.LAG_MAX_SLOTS
        self.arrays = capi.LagArrays(params.n_a + params.n_b, config.levels if ok else 1, config.slots if ok else 2)
        self.acc = capi.LagOut()
        v = hs.view()
        _host_check(load_library().kmc_host_lag_begin(C.byref(params), C.byref(v), C.byref(config),
                                                      C.byref(self.arrays.view()), C.byref(self.acc)))

    def update(self, hs: capi.HostState) -> capi.LagInfo:
        """Advance the recorder to hs (kmc_host_lag_update)."""
        v = hs.view()
        info = capi.LagInfo()
        _host_check(load_library().kmc_host_lag_update(C.byref(self.params), C.byref(v), C.byref(self.arrays.view()),
                                                       C.byref(self.acc), C.byref(info)))
        return info

    def sample(self) -> capi.LagSample:
        """The table as of the last update — kmc_host_lag_sample; a copy."""
        out = capi.LagOut()
        table = np.zeros_like(self.arrays.table)
        n_pairs = np.zeros_like(self.arrays.n_pairs)
        _host_check(load_library().kmc_host_lag_sample(C.byref(self.params), C.byref(self.arrays.view()),
                                                       C.byref(self.acc), C.byref(out), table.ctypes.data,
                                                       n_pairs.ctypes.data))
        return capi.LagSample(out, table, n_pairs)


def _pd_tables(nbins: int):
    nb = max(1, min(int(nbins), capi.PD_MAX_BINS))
    return (np.zeros((4, nb), dtype=np.int64), np.zeros((2, nb), dtype=np.int64),
            np.zeros((3, nb), dtype=capi.PD_CELL_DTYPE))


class HostPd:
    """Pair dynamics on host states, sequentially (kmc_host_pd_*): Simulation.pd_*'s counterpart without a device.
    The recorder begins at hs (update 0); update(hs) advances it to the state `every` steps later.  arrays
    (capi.PdArrays) holds its per-protein state."""

    def __init__(self, params: capi.Params, hs: capi.HostState, config: capi.PdConfig):
        self.params = params
        self.arrays = capi.PdArrays(params.n_a + params.n_b)
        self.acc = capi.PdOut()
        v = hs.view()
        _host_check(load_library().kmc_host_pd_begin(C.byref(params), C.byref(v), C.byref(config),
                                                     C.byref(self.arrays.view()), C.byref(self.acc)))

    def update(self, hs: capi.HostState) -> capi.PdInfo:
        """Advance the recorder to hs (kmc_host_pd_update)."""
        v = hs.view()
        info = capi.PdInfo()
        _host_check(load_library().kmc_host_pd_update(C.byref(self.params), C.byref(v), C.byref(self.arrays.view()),
                                                      C.byref(self.acc), C.byref(info)))
        return info

    def sample(self) -> capi.PdSample:
        """The tables of the state as of the last update — kmc_host_pd_sample."""
        out = capi.PdOut()
        gd, gs, cu = _pd_tables(self.acc.cfg.nbins)
        _host_check(load_library().kmc_host_pd_sample(C.byref(self.params), C.byref(self.arrays.view()),
                                                      C.byref(self.acc), C.byref(out), gd.ctypes.data, gs.ctypes.data,
                                                      cu.ctypes.data))
        return capi.PdSample(out, gd, gs, cu)


def _bd_table(max_size: int) -> np.ndarray:
    return np.zeros((2, max(2, min(int(max_size), capi.BD_MAX_SIZE)) + 1), dtype=capi.BD_CELL_DTYPE)


class HostBd:
    """Body dynamics on host states, sequentially (kmc_host_bd_*): Simulation.bd_*'s counterpart without a device.
    The recorder begins at hs (update 0); update(hs) advances it to the state `every` steps later; sample(hs) and
    bodies(hs) take the state of the last update again, for its components.  arrays (capi.BdArrays) holds the
    per-protein state and may be edited between the calls."""

    def __init__(self, params: capi.Params, hs: capi.HostState, config: capi.BdConfig):
        self.params = params
        self.arrays = capi.BdArrays(params.n_a + params.n_b)
        self.acc = capi.BdOut()
        v = hs.view()
        _host_check(load_library().kmc_host_bd_begin(C.byref(params), C.byref(v), C.byref(config),
                                                     C.byref(self.arrays.view()), C.byref(self.acc)))

    def update(self, hs: capi.HostState) -> capi.BdInfo:
        """Advance the recorder to hs (kmc_host_bd_update)."""
        v = hs.view()
        info = capi.BdInfo()
        _host_check(load_library().kmc_host_bd_update(C.byref(self.params), C.byref(v), C.byref(self.arrays.view()),
                                                      C.byref(self.acc), C.byref(info)))
        return info

    def sample(self, hs: capi.HostState) -> capi.BdSample:
        """The table of hs, the state of the last update — kmc_host_bd_sample."""
        v = hs.view()
        out = capi.BdOut()
        table = _bd_table(self.acc.cfg.max_size)
        _host_check(load_library().kmc_host_bd_sample(C.byref(self.params), C.byref(v), C.byref(self.arrays.view()),
                                                      C.byref(self.acc), C.byref(out), table.ctypes.data))
        return capi.BdSample(out, table)

    def bodies(self, hs: capi.HostState, min_size: int = 1, cap: Optional[int] = None):
        """The bodies of at least min_size members, by label, as a record array (capi.BD_BODY_DTYPE, the fields of
        capi.BdBody) — kmc_host_bd_bodies."""
        v = hs.view()
        cap = self.params.n_a + self.params.n_b if cap is None else int(cap)
        rows = np.zeros(max(cap, 1), dtype=capi.BD_BODY_DTYPE)
        n = C.c_int64(0)
        _host_check(load_library().kmc_host_bd_bodies(C.byref(self.params), C.byref(v), C.byref(self.arrays.view()),
                                                      C.byref(self.acc), int(min_size), cap, rows.ctypes.data,
                                                      C.byref(n)))
        return rows[:n.value].copy()


class HostRot:
    """The orientation recorder on host states, sequentially (kmc_host_rot_*): Simulation.rot_*'s counterpart without
    a device.  The recorder begins at hs (update 0); update(hs) advances it to the state `every` steps later.
    arrays (capi.RotArrays) holds its per-protein state, the rings and the table."""

    def __init__(self, params: capi.Params, hs: capi.HostState, config: capi.RotConfig):
        self.params = params
        ok = 1 <= config.levels <= capi.LAG_MAX_LEVELS and 2 <= config.slots <= capi.LAG_MAX_SLOTS
        self.arrays = capi.RotArrays(params.n_a, params.n_b, config.levels if ok else 1, config.slots if ok else 2)
        self.acc = capi.RotOut()
        v = hs.view()
        _host_check(load_library().kmc_host_rot_begin(C.byref(params), C.byref(v), C.byref(config),
                                                      C.byref(self.arrays.view()), C.byref(self.acc)))

    def update(self, hs: capi.HostState) -> capi.RotInfo:
        """Advance the recorder to hs (kmc_host_rot_update)."""
        v = hs.view()
        info = capi.RotInfo()
        _host_check(load_library().kmc_host_rot_update(C.byref(self.params), C.byref(v), C.byref(self.arrays.view()),
                                                       C.byref(self.acc), C.byref(info)))
        return info

    def sample(self) -> capi.RotSample:
        """The table as of the last update — kmc_host_rot_sample; a copy."""
        out = capi.RotOut()
        table = np.zeros_like(self.arrays.table)
        n_pairs = np.zeros_like(self.arrays.n_pairs)
        _host_check(load_library().kmc_host_rot_sample(C.byref(self.params), C.byref(self.arrays.view()),
                                                       C.byref(self.acc), C.byref(out), table.ctypes.data,
                                                       n_pairs.ctypes.data))
        return capi.RotSample(out, table, n_pairs)


def host_ligand_pose(params: capi.Params, hs: capi.HostState, nz: int, nc: int):
    """(hist[4, nz, nc] int64, capi.PoseOut) of a host state, sequentially (kmc_host_ligand_pose)."""
    ok = 1 <= nz <= capi.POSE_MAX_BINS and 1 <= nc <= capi.POSE_MAX_BINS
    hist = np.zeros((capi.POSE_CLASSES, nz, nc) if ok else (1,), dtype=np.int64)
    out = capi.PoseOut()
    v = hs.view()
    _host_check(load_library().kmc_host_ligand_pose(C.byref(params), C.byref(v), int(nz), int(nc), hist.ctypes.data,
                                                    C.byref(out)))
    return hist, out


def host_dd_check(gid: np.ndarray, own: np.ndarray) -> int:
    """kmc_dd_set_state's argument check on the host: 0 or KMC_ERR_ARG."""
    gid = np.ascontiguousarray(gid, dtype=np.int32)
    own = np.ascontiguousarray(own, dtype=np.uint8)
    if gid.size != own.size:
        raise ValueError("gid / own of one window")
    return int(load_library().kmc_host_dd_check(gid.size, gid.ctypes.data, own.ctypes.data))


def state_hash(params: capi.Params, hs: capi.HostState) -> int:
    v = hs.view()
    return int(load_library().kmc_state_hash(C.byref(params), C.byref(v)))


def bond_line(params: capi.Params, rec) -> str:
    """One bond.dat line (main.cpp:2251) from a kmc_obs record."""
    o = capi.Obs()
    for name in capi.OBS_DTYPE.names:
        setattr(o, name, rec[name].item() if hasattr(rec[name], "item") else rec[name])
    buf = C.create_string_buffer(256)
    n = load_library().kmc_format_bond_line(C.byref(params), C.byref(o), buf, 256)
    return buf.value[:n].decode()


def write_parameter_log(params: capi.Params, path: str) -> None:
    """parameter.log (main.cpp:178-205)."""
    _host_check(load_library().kmc_host_write_parameter_log(C.byref(params), os.fsencode(path)))


def append_gro(params: capi.Params, hs: capi.HostState, path: str) -> None:
    """one test.gro frame (main.cpp:2258-2287)."""
    v = hs.view()
    _host_check(load_library().kmc_host_append_gro(C.byref(params), C.byref(v), os.fsencode(path)))


def append_cluster_log(params: capi.Params, step: int, row_len: np.ndarray, members: np.ndarray, path: str) -> None:
    """one cluster.log block (main.cpp:2291-2305)."""
    row_len = np.ascontiguousarray(row_len, dtype=np.int32)
    members = np.ascontiguousarray(members, dtype=np.int32)
    _host_check(load_library().kmc_host_append_cluster_log(C.byref(params), step, row_len.ctypes.data,
                                                           members.ctypes.data, os.fsencode(path)))


def math(op: int, x: np.ndarray, y: Optional[np.ndarray] = None, device: bool = False) -> np.ndarray:
    """Portable libm (kmc_math.h) on host or device — numerics diagnostics."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, dtype=np.float64)
    out = np.empty_like(x)
    L = load_library()
    f = L.kmc_device_math if device else L.kmc_host_math
    rc = f(op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size)
    if rc != 0:
        raise KmcError(rc, "math diagnostic failed")
    return out


# ---------------------------------------------------------------- device sim
class Simulation:
    """One trajectory on one GPU (handle = kmc_sim*)."""

    def __init__(self, params: capi.Params, device: int = 0):
        self.params = params
        self.device = device  # HIP ordinal: the decomposed mode's exchange buffers live there
        L = load_library()
        h = C.c_void_p()
        rc = L.kmc_create(C.byref(params), device, C.byref(h))
        if rc != 0:
            raise KmcError(rc, "kmc_create failed (needs a gfx950 device)")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            load_library().kmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            raise KmcError(rc, load_library().kmc_last_error(self._h).decode())

    def init_random(self):
        self._check(load_library().kmc_init_random(self._h))

    def load_cpt(self, path: str):
        self._check(load_library().kmc_load_cpt(self._h, os.fsencode(path)))

    def write_cpt(self, path: str):
        self._check(load_library().kmc_write_cpt(self._h, os.fsencode(path)))

    def save_state(self, path: str):
        """Exact checkpoint: a later load_state continues the trajectory bit for bit."""
        self._check(load_library().kmc_save_state(self._h, os.fsencode(path)))

    def load_state(self, path: str):
        self._check(load_library().kmc_load_state(self._h, os.fsencode(path)))

    def set_state(self, hs: capi.HostState):
        v = hs.view()
        self._check(load_library().kmc_set_state(self._h, C.byref(v)))

    def get_state(self) -> capi.HostState:
        hs = capi.HostState(self.params.n_a, self.params.n_b)
        v = hs.view()
        self._check(load_library().kmc_get_state(self._h, C.byref(v)))
        hs.pull(v)
        return hs

    def step(self, n: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Advance n steps; returns the n bond.dat records (capi.OBS_DTYPE)."""
        if out is None:
            out = np.zeros(n, dtype=capi.OBS_DTYPE)
        elif out.dtype != capi.OBS_DTYPE or not out.flags.c_contiguous or not out.flags.writeable or len(out) < n:
            # kmc_step writes n records of sizeof(kmc_obs) through the pointer
            raise ValueError(f"out must be a writeable C-contiguous capi.OBS_DTYPE array of length >= {n}")
        self._check(load_library().kmc_step(self._h, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def clusters(self):
        """BFS member rows of the last step: (row_len[n_b], members) — kmc_get_clusters."""
        n_b = self.params.n_b
        row = np.zeros(max(1, n_b), dtype=np.int32)  # (never an empty buffer: the library refuses a null pointer)
        mem = np.zeros(self.params.n_a + n_b, dtype=np.int32)
        self._check(load_library().kmc_get_clusters(self._h, row.ctypes.data, mem.ctypes.data))
        return row[:n_b], mem[: int(row[:n_b].sum())]

    # ---- structure analysis of the current state (kmc_analysis.hip; works before any step)
    def components(self) -> np.ndarray:
        """label[i] = smallest reference index (1-based) in protein i+1's bond-graph component."""
        label = np.zeros(self.params.n_a + self.params.n_b, dtype=np.int32)
        self._check(load_library().kmc_components(self._h, label.ctypes.data))
        return label

    def census(self, max_r: int, max_l: int):
        """(hist[max_r + 1, max_l + 1] int64 of components by (receptors, ligands), larger counts clamped
        into the last row / column; capi.Census summary) — kmc_oligomer_census."""
        if max_r < 0 or max_l < 0:
            raise ValueError("census: max_r, max_l >= 0")
        hist = np.zeros((max_r + 1, max_l + 1), dtype=np.int64)
        out = capi.Census()
        self._check(load_library().kmc_oligomer_census(self._h, max_r, max_l, hist.ctypes.data, C.byref(out)))
        return hist, out

    def pair_counts(self, which, r_max: float, nbins: int) -> np.ndarray:
        """Lateral pair-distance counts[nbins] (int64) of species pair `which` ("AA", "AB", "BB" or
        capi.PAIR_*) below r_max — kmc_pair_counts; analysis.rdf turns them into g(r)."""
        which = capi.PAIRS.get(which, which) if isinstance(which, str) else which
        counts = np.zeros(max(int(nbins), 1), dtype=np.int64)
        self._check(load_library().kmc_pair_counts(self._h, int(which), float(r_max), int(nbins),
                                                   counts.ctypes.data))
        return counts

    # ---- cluster geometry of the current state (kmc_geometry.hip)
    def unwrap(self):
        """(label[N] 1-based as components(), shift[N, 2] int32 periodic image of every protein against its
        label, span[N] uint8 spanning bits of its component: capi.SPAN_X | capi.SPAN_Y) — kmc_unwrap."""
        n = self.params.n_a + self.params.n_b
        label = np.zeros(n, dtype=np.int32)
        shift = np.zeros((2, n), dtype=np.int32)
        span = np.zeros(n, dtype=np.uint8)
        self._check(load_library().kmc_unwrap(self._h, label.ctypes.data, shift.ctypes.data, span.ctypes.data))
        return label, np.ascontiguousarray(shift.T), span

    def cluster_geometry(self, max_size: int):
        """(table[max_size + 1] capi.GEOM_BIN_DTYPE by cluster size, larger sizes clamped into the last bin;
        capi.Geom summary) — kmc_cluster_geometry; analysis.rg_by_size turns the table into Rg²(n)."""
        table = np.zeros(max(int(max_size), 0) + 1, dtype=capi.GEOM_BIN_DTYPE)
        out = capi.Geom()
        self._check(load_library().kmc_cluster_geometry(self._h, int(max_size), table.ctypes.data, C.byref(out)))
        return table, out

    def cluster_list(self, min_size: int, cap: int = 4096):
        """Rows (a capi.Cluster array, sorted by label) of the components of at least min_size members —
        kmc_cluster_list; when more than cap qualify, the call is repeated once with the count it returned."""
        L = load_library()
        n = C.c_int64()
        for _ in range(2):
            rows = (capi.Cluster * max(int(cap), 1))()
            rc = L.kmc_cluster_list(self._h, int(min_size), int(cap), rows, C.byref(n))
            if rc != capi.ERR_CAPACITY or n.value <= cap:
                break
            cap = n.value
        self._check(rc)
        return rows[: n.value]

    # ---- static structure factor of the current state (kmc_structure.hip)
    def structure_factor(self, hmax: int, kmax: int, select="all"):
        """(sums[4, hmax + 1, 2 kmax + 1] int64: C_A, S_A, C_B, S_B at q = 2 pi (h / box_x, k / box_y), h = 0..hmax,
        k = -kmax..kmax; n_sel[2] int64: the receptors and ligands summed over) — kmc_structure_factor.  select:
        "all", or "bound" for the proteins that hold a bond.  The sums are exact integers (terms in units of
        2^-30); analysis.structure_factor turns them into the partial S(q)."""
        sums, n_sel = _sk_buffers(hmax, kmax)
        self._check(load_library().kmc_structure_factor(self._h, int(hmax), int(kmax), capi.sk_select(select),
                                                        sums.ctypes.data, n_sel.ctypes.data))
        return sums, n_sel

    # ---- bond-orientational order of the current state (kmc_bondorder.hip)
    def bond_order(self, which, fold: int, r_cut=None, mode="within", select="all", nbins: int = 64,
                   per_protein: bool = False):
        """The local fold-fold bond-orientational order of species which ("A" receptors, "B" ligands) —
        kmc_bond_order: (hist[16, nbins] int64 of the selected proteins by (min(neighbours, 15), bin of |psi|),
        capi.BondOrderOut global sums), and with per_protein also (C[n], S[n] int64, nn[n] int32) by the species'
        reference index: the sums of cos / sin (n theta) in units of 2^-30 over a protein's neighbours, and their
        number.  mode "within": the neighbours within r_cut; "linked" (ligands): the ligands reached over a
        receptor and its cis partner, r_cut ignored.  select "all" or "bound".  Exact integers, additive over
        replicas (analysis.reduce_counts); analysis.bond_order turns the summary into |Psi_n|."""
        n = self.params.n_a if capi.bo_which(which) == capi.BO_A else self.params.n_b
        rc, res = _bo_call(load_library().kmc_bond_order, (self._h,), n, which, fold, r_cut, mode, select, nbins,
                           per_protein)
        self._check(rc)
        return res

    def bond_order_corr(self, which, fold: int, r_max: float, r_cut=None, mode="within", select="all",
                        nbins: int = 64) -> np.ndarray:
        """corr[2, nbins] int64 — kmc_bond_order_corr: over the unordered pairs of the set's proteins that have a
        neighbour, by lateral distance below r_max: corr[0] the sums of Re(psi_i conj psi_j) in units of 2^-30,
        corr[1] the pair counts.  The other arguments as bond_order (the call runs the local pass itself).  Additive
        over replicas (analysis.reduce_counts); analysis.bond_order_corr turns it into (r, G_n)."""
        corr = np.zeros((2, int(nbins) if 1 <= int(nbins) <= capi.BO_CORR_BINS else 1), dtype=np.int64)
        self._check(load_library().kmc_bond_order_corr(self._h, *_bo_args(which, fold, r_cut, mode, select),
                                                       float(r_max), int(nbins), corr.ctypes.data))
        return corr

    # ---- ligand network and its rings in the current state (kmc_rings.hip)
    def network(self):
        """(capi.NetOut, lig_hist[4, 4] int64, adj_lig[n_b, 3] int32, adj_site[n_b, 3] int32) — kmc_network: the
        counters of the ligand – receptor = receptor – ligand bridges (bridges, loops, half bridges, free cis dimers,
        network ligands and components, cycle rank) with the receptors' valency bins rec[(nei2 != 0) + 2 (nei3 !=
        0)]; the ligands by [occupied sites, bridge ends]; and per ligand (reference index) and site - 2 the ligand
        bridged to it (1-based ligand number, 0: none) and the site it arrives at.  Exact integers; the counters and
        the bins are additive over replicas (analysis.reduce_counts)."""
        rc, res = _net_call(load_library().kmc_network, (self._h,), self.params.n_b)
        self._check(rc)
        return res

    def rings(self, max_len: int = 8, members: bool = False):
        """(counts[2, RING_MAX + 1] int64, capi.NetOut) — kmc_rings: counts[0, L] the closed rings of L bridges over L
        distinct ligands, counts[1, L] the chordless ones, for 1 <= L <= max_len <= capi.RING_MAX (the other entries
        are zero).  With members: (counts, member[2, n_b] uint32, NetOut), bit L of member[0 / 1, b] set iff ligand b
        (reference index) lies on such a ring of length L.  Additive over replicas (analysis.reduce_counts);
        analysis.ring_stats turns counts and the NetOut into the hexagon fraction and the ring densities."""
        rc, res = _rings_call(load_library().kmc_rings, (self._h,), self.params.n_b, max_len, members)
        self._check(rc)
        return res

    @property
    def rings_hops(self) -> int:
        """Adjacency rows the last rings call gathered along its paths (kmc_rings_hops): its work, beside analysis_ms."""
        return int(load_library().kmc_rings_hops(self._h))

    @property
    def analysis_ms(self) -> float:
        """Device milliseconds (HIP events) of the last components / census / pair_counts / track_* / kin_* / cf_* / lag_* / rot_* / pd_* / bd_* / ligand_pose / unwrap /
        cluster_* / structure_factor / bond_order / bond_order_corr / network / rings / prox_clusters call."""
        return float(load_library().kmc_analysis_ms(self._h))

    # ---- displacement tracking since a time origin (kmc_dynamics.hip)
    def track_begin(self, max_jump: float = 0.0) -> None:
        """The current state becomes the origin (max_jump <= 0: a quarter of the shorter box side)."""
        self._check(load_library().kmc_track_begin(self._h, float(max_jump)))

    def track_update(self) -> capi.TrackInfo:
        """Add the minimum-image displacement since the last update to every protein's u; call it between
        step() calls, often enough that no protein moves half a box in between."""
        info = capi.TrackInfo()
        self._check(load_library().kmc_track_update(self._h, C.byref(info)))
        return info

    def track_sample(self, r_max: float, nbins: int):
        """(capi.TrackSample, vanhove[TRACK_CLASSES, nbins] int64) of the tracker as of the last update —
        kmc_track_sample; analysis.msd turns the sample into per-class means."""
        vh = np.zeros((capi.TRACK_CLASSES, max(int(nbins), 1)), dtype=np.int64)
        out = capi.TrackSample()
        self._check(load_library().kmc_track_sample(self._h, float(r_max), int(nbins), C.byref(out), vh.ctypes.data))
        return out, vh

    def track_displacements(self):
        """(u[N, 2] float64, flags[N] uint8: capi.TRACK_CHANGED | capi.TRACK_JUMPED) by reference index."""
        n = self.params.n_a + self.params.n_b
        u = np.zeros((2, n), dtype=np.float64)
        flags = np.zeros(n, dtype=np.uint8)
        self._check(load_library().kmc_track_displacements(self._h, u.ctypes.data, flags.ctypes.data))
        return np.ascontiguousarray(u.T), flags

    def track_end(self) -> None:
        self._check(load_library().kmc_track_end(self._h))

    def run_tracked(self, nsteps: int, every: int, sample_every: int, r_max: float, nbins: int):
        """Advance nsteps steps in pieces of at most `every` steps with a track_update after each piece,
        sampling whenever `sample_every` more steps have passed (a multiple of `every` keeps the samples
        evenly spaced).  The tracker must have been begun.  Returns (records[nsteps], samples), samples =
        [(step, capi.TrackSample, vanhove)]."""
        if nsteps < 0 or every < 1 or sample_every < 1:
            raise ValueError("run_tracked: nsteps >= 0, every >= 1, sample_every >= 1")
        recs = np.zeros(nsteps, dtype=capi.OBS_DTYPE)
        samples = []
        done = since = 0
        while done < nsteps:
            n = min(every, nsteps - done)
            self.step(n, recs[done:done + n])
            done += n
            since += n
            self.track_update()
            if since >= sample_every:
                since = 0
                samples.append((self.current_step,) + self.track_sample(r_max, nbins))
        return recs, samples

    # ---- bond kinetics since a begin (kmc_kinetics.hip)
    def kin_begin(self) -> None:
        """Start the bond kinetics recorder at the current state: the bonds that exist are left-censored."""
        self._check(load_library().kmc_kin_begin(self._h))

    def kin_update(self) -> capi.KinOut:
        """Record the bonds that ended or were born since the last update; call it between step() calls — after
        every step for exact lifetimes (every k steps: stroboscopic ones)."""
        out = capi.KinOut()
        self._check(load_library().kmc_kin_update(self._h, C.byref(out)))
        return out

    def kin_sample(self):
        """(capi.KinOut, hist[KIN_HISTS, KIN_BINS] int64) of the recorder as of the last update — kmc_kin_sample;
        analysis.kinetics_rates and analysis.lifetime_survival post-process them."""
        out = capi.KinOut()
        hist = np.zeros((capi.KIN_HISTS, capi.KIN_BINS), dtype=np.int64)
        self._check(load_library().kmc_kin_sample(self._h, C.byref(out), hist.ctypes.data))
        return out, hist

    def kin_arrays(self) -> capi.KinArrays:
        """The recorder's per-receptor arrays by reference index (kmc_kin_get): diagnostics and tests."""
        a = capi.KinArrays(self.params.n_a)
        self._check(load_library().kmc_kin_get(self._h, C.byref(a.view())))
        return a

    def kin_end(self) -> None:
        self._check(load_library().kmc_kin_end(self._h))

    def run_kinetics(self, nsteps: int, every: int = 1):
        """Advance nsteps steps in pieces of at most `every` steps with a kin_update after each piece.  The
        recorder must have been begun.  Returns (records[nsteps], the last update's capi.KinOut or None)."""
        if nsteps < 0 or every < 1:
            raise ValueError("run_kinetics: nsteps >= 0, every >= 1")
        recs = np.zeros(nsteps, dtype=capi.OBS_DTYPE)
        done, out = 0, None
        while done < nsteps:
            n = min(every, nsteps - done)
            self.step(n, recs[done:done + n])
            done += n
            out = self.kin_update()
        return recs, out


    # ---- cluster growth kinetics since a begin (kmc_coag.hip)
    def cf_begin(self, max_size: int = 16) -> None:
        """Start the cluster growth recorder at the current state; sizes from max_size on share the last index."""
        self._check(load_library().kmc_cf_begin(self._h, int(max_size)))

    def cf_update(self) -> capi.CfOut:
        """File the mergers and fragmentations since the last look; call it between step() calls — after every
        step for events exact up to simultaneous ones (every k steps: stroboscopic ones)."""
        out = capi.CfOut()
        self._check(load_library().kmc_cf_update(self._h, C.byref(out)))
        return out

    def cf_sample(self):
        """(capi.CfOut, capi.CfTables) of the recorder as of the last look — kmc_cf_sample; analysis.coag_kernel,
        analysis.frag_kernel and analysis.growth_modes post-process them."""
        out = capi.CfOut()
        self._check(load_library().kmc_cf_sample(self._h, C.byref(out), None))
        t = capi.CfTables(int(out.max_size))
        self._check(load_library().kmc_cf_sample(self._h, C.byref(out), C.byref(t.view())))
        return out, t

    def cf_arrays(self) -> capi.CfArrays:
        """The recorder's per-protein state by reference index (kmc_cf_get): the stored bonds and the labels of
        the last look.  With the step of that look it is what cf_put takes."""
        a = capi.CfArrays(self.params.n_a, self.params.n_b)
        self._check(load_library().kmc_cf_get(self._h, C.byref(a.view())))
        return a

    def cf_put(self, arrays: capi.CfArrays, last_step: int) -> None:
        """Load a recorder state saved by cf_arrays or built by HostCoag, as of step last_step (kmc_cf_put): the
        tables and counters start again at zero."""
        a = capi.CfArrays(self.params.n_a, self.params.n_b)
        for name in a.NAMES:
            src = np.ascontiguousarray(getattr(arrays, name), dtype=np.int32)
            if src.shape != getattr(a, name).shape:
                raise ValueError("cf_put: " + name + " has the wrong length")
            setattr(a, name, src)
        self._check(load_library().kmc_cf_put(self._h, C.byref(a.view()), int(last_step)))

    def cf_end(self) -> None:
        self._check(load_library().kmc_cf_end(self._h))

    def run_coag(self, nsteps: int, every: int = 1):
        """Advance nsteps steps in pieces of at most `every` steps with a cf_update after each piece.  The
        recorder must have been begun.  Returns (records[nsteps], the last update's capi.CfOut or None)."""
        if nsteps < 0 or every < 1:
            raise ValueError("run_coag: nsteps >= 0, every >= 1")
        recs = np.zeros(nsteps, dtype=capi.OBS_DTYPE)
        done, out = 0, None
        while done < nsteps:
            n = min(every, nsteps - done)
            self.step(n, recs[done:done + n])
            done += n
            out = self.cf_update()
        return recs, out

    # ---- multi-origin lag correlator since a begin (kmc_lagcorr.hip)
    def lag_begin(self, config: capi.LagConfig) -> None:
        """Start the lag correlator at the current state (update 0; capi.lag_config builds the configuration).  It
        allocates levels * slots * 16 bytes per protein, freed by lag_end."""
        self._check(load_library().kmc_lag_begin(self._h, C.byref(config)))

    def lag_update(self) -> capi.LagInfo:
        """Correlate the current positions with every stored origin that is due and store the new origins; legal
        exactly `every` steps after the last update (or the begin)."""
        info = capi.LagInfo()
        self._check(load_library().kmc_lag_update(self._h, C.byref(info)))
        return info

    def lag_sample(self) -> capi.LagSample:
        """The table accumulated since lag_begin — kmc_lag_sample; analysis.lag_curves turns it into MSD, alpha_2
        and F_s by lag time."""
        out = capi.LagOut()
        self._check(load_library().kmc_lag_sample(self._h, C.byref(out), None, None))
        table = np.zeros((int(out.rows), capi.LAG_CLASSES), dtype=capi.LAG_CELL_DTYPE)
        n_pairs = np.zeros(int(out.rows), dtype=np.int64)
        self._check(load_library().kmc_lag_sample(self._h, C.byref(out), table.ctypes.data, n_pairs.ctypes.data))
        return capi.LagSample(out, table, n_pairs)

    def lag_arrays(self):
        """(U[N, 2] int64, last_event[N] int32) by reference index (kmc_lag_arrays): diagnostics and tests."""
        n = self.params.n_a + self.params.n_b
        U = np.zeros((n, 2), dtype=np.int64)
        last_event = np.zeros(n, dtype=np.int32)
        self._check(load_library().kmc_lag_arrays(self._h, U.ctypes.data, last_event.ctypes.data))
        return U, last_event

    def lag_end(self) -> None:
        self._check(load_library().kmc_lag_end(self._h))

    def run_lagged(self, nsteps: int):
        """Advance nsteps steps, `every` of the begun recorder's configuration at a time, with a lag_update after
        each piece (nsteps must be a multiple of every).  Returns (records[nsteps], the last capi.LagInfo or None)."""
        out = capi.LagOut()
        self._check(load_library().kmc_lag_sample(self._h, C.byref(out), None, None))
        every = int(out.cfg.every)
        if nsteps < 0 or nsteps % every:
            raise ValueError("run_lagged: nsteps >= 0, a multiple of the recorder's every")
        recs = np.zeros(nsteps, dtype=capi.OBS_DTYPE)
        done, info = 0, None
        while done < nsteps:
            self.step(every, recs[done:done + every])
            done += every
            info = self.lag_update()
        return recs, info

    # ---- pair dynamics since a begin: distinct van Hove and displacement correlation (kmc_pairdyn.hip)
    def pd_begin(self, config: capi.PdConfig) -> None:
        """Start the pair dynamics at the current state (update 0; capi.pd_config builds the configuration).  It
        allocates 109 bytes per protein and 12 per cell of the search grid, freed by pd_end."""
        self._check(load_library().kmc_pd_begin(self._h, C.byref(config)))

    def pd_update(self) -> capi.PdInfo:
        """Advance the unwrapped positions; legal exactly `every` steps after the last update (or the begin)."""
        info = capi.PdInfo()
        self._check(load_library().kmc_pd_update(self._h, C.byref(info)))
        return info

    def pd_sample(self) -> capi.PdSample:
        """The tables of the state as of the last update — kmc_pd_sample; analysis.van_hove_distinct and
        analysis.displacement_corr turn them into G_d(r, t) and C_u(r, t)."""
        out = capi.PdOut()
        self._check(load_library().kmc_pd_sample(self._h, C.byref(out), None, None, None))
        gd, gs, cu = _pd_tables(out.cfg.nbins)
        self._check(load_library().kmc_pd_sample(self._h, C.byref(out), gd.ctypes.data, gs.ctypes.data, cu.ctypes.data))
        return capi.PdSample(out, gd, gs, cu)

    def pd_arrays(self):
        """(U[N, 2] int64, X0[N, 2] int64, flags[N] uint8: capi.PD_JUMPED) by reference index (kmc_pd_arrays)."""
        n = self.params.n_a + self.params.n_b
        U = np.zeros((n, 2), dtype=np.int64)
        X0 = np.zeros((n, 2), dtype=np.int64)
        flags = np.zeros(n, dtype=np.uint8)
        self._check(load_library().kmc_pd_arrays(self._h, U.ctypes.data, X0.ctypes.data, flags.ctypes.data))
        return U, X0, flags

    def pd_end(self) -> None:
        self._check(load_library().kmc_pd_end(self._h))

    def run_paired(self, nsteps: int, sample_every: int):
        """Advance nsteps steps, `every` of the begun recorder's configuration at a time, with a pd_update after each
        piece and a pd_sample after every sample_every-th update (nsteps must be a multiple of every).  Returns
        (records[nsteps], the list of capi.PdSample)."""
        out = capi.PdOut()
        self._check(load_library().kmc_pd_sample(self._h, C.byref(out), None, None, None))
        every = int(out.cfg.every)
        if nsteps < 0 or nsteps % every or sample_every < 1:
            raise ValueError("run_paired: nsteps >= 0, a multiple of the recorder's every; sample_every >= 1")
        recs = np.zeros(nsteps, dtype=capi.OBS_DTYPE)
        done, samples = 0, []
        while done < nsteps:
            self.step(every, recs[done:done + every])
            done += every
            if self.pd_update().n_updates % sample_every == 0:
                samples.append(self.pd_sample())
        return recs, samples

    # ---- body dynamics since a begin: D(s), rotation and survival of clusters by size (kmc_bodydyn.hip)
    def bd_begin(self, config: capi.BdConfig) -> None:
        """Start the body dynamics at the current state (update 0; capi.bd_config builds the configuration): the
        clusters of this state are the bodies.  It allocates 189 bytes per protein, freed by bd_end."""
        self._check(load_library().kmc_bd_begin(self._h, C.byref(config)))

    def bd_update(self) -> capi.BdInfo:
        """Advance the unwrapped positions and the flags; legal exactly `every` steps after the last update."""
        info = capi.BdInfo()
        self._check(load_library().kmc_bd_update(self._h, C.byref(info)))
        return info

    def bd_sample(self) -> capi.BdSample:
        """The table of the current state, which must be that of the last update — kmc_bd_sample; analysis.body_msd,
        body_rotation and body_survival read it."""
        out = capi.BdOut()
        self._check(load_library().kmc_bd_sample(self._h, C.byref(out), None))
        table = _bd_table(out.cfg.max_size)
        self._check(load_library().kmc_bd_sample(self._h, C.byref(out), table.ctypes.data))
        return capi.BdSample(out, table)

    def bd_sample_ms(self):
        """(components, reduce, finish): device milliseconds of the parts of the last bd_sample (kmc_bd_sample_ms)."""
        ms = (C.c_double * 3)()
        self._check(load_library().kmc_bd_sample_ms(self._h, ms))
        return tuple(ms)

    def bd_bodies(self, min_size: int = 1, cap: Optional[int] = None):
        """The bodies of at least min_size members, by label, as a record array (capi.BD_BODY_DTYPE, the fields of
        capi.BdBody) — kmc_bd_bodies."""
        cap = self.params.n_a + self.params.n_b if cap is None else int(cap)
        rows = np.zeros(max(cap, 1), dtype=capi.BD_BODY_DTYPE)
        n = C.c_int64(0)
        self._check(load_library().kmc_bd_bodies(self._h, int(min_size), cap, rows.ctypes.data, C.byref(n)))
        return rows[:n.value].copy()

    def bd_arrays(self):
        """(U[N, 2], X0[N, 2] int64, flags[N] uint8, label[N] int32 1-based, D0[N, 2] int64) by reference index."""
        n = self.params.n_a + self.params.n_b
        U, X0, D0 = (np.zeros((n, 2), dtype=np.int64) for _ in range(3))
        flags = np.zeros(n, dtype=np.uint8)
        label = np.zeros(n, dtype=np.int32)
        self._check(load_library().kmc_bd_arrays(self._h, U.ctypes.data, X0.ctypes.data, flags.ctypes.data,
                                                 label.ctypes.data, D0.ctypes.data))
        return U, X0, flags, label, D0

    def bd_get(self) -> capi.BdArrays:
        """The recorder's per-protein state and its static arrays as a capi.BdArrays (kmc_bd_get)."""
        a = capi.BdArrays(self.params.n_a + self.params.n_b)
        self._check(load_library().kmc_bd_get(self._h, C.byref(a.view())))
        return a

    def bd_put(self, arrays: capi.BdArrays, last_step: Optional[int] = None) -> None:
        """Load prev, U, links and flags of `arrays` into the recorder, which was begun on the current state, and set
        the step of its last update (default: the current step) — kmc_bd_put."""
        step = self.current_step if last_step is None else int(last_step)
        self._check(load_library().kmc_bd_put(self._h, C.byref(arrays.view()), step))

    def bd_end(self) -> None:
        self._check(load_library().kmc_bd_end(self._h))

    def run_bodies(self, nsteps: int, sample_every: int):
        """Advance nsteps steps, `every` of the begun recorder's configuration at a time, with a bd_update after each
        piece and a bd_sample after every sample_every-th update (nsteps must be a multiple of every).  Returns
        (records[nsteps], the list of capi.BdSample)."""
        out = capi.BdOut()
        self._check(load_library().kmc_bd_sample(self._h, C.byref(out), None))
        every = int(out.cfg.every)
        if nsteps < 0 or nsteps % every or sample_every < 1:
            raise ValueError("run_bodies: nsteps >= 0, a multiple of the recorder's every; sample_every >= 1")
        recs = np.zeros(nsteps, dtype=capi.OBS_DTYPE)
        done, samples = 0, []
        while done < nsteps:
            self.step(every, recs[done:done + every])
            done += every
            if self.bd_update().n_updates % sample_every == 0:
                samples.append(self.bd_sample())
        return recs, samples

    # ---- orientation: the rotational lag correlator and the ligands' poses (kmc_orient.hip)
    def rot_begin(self, config: capi.RotConfig) -> None:
        """Start the orientation recorder at the current state (update 0; capi.rot_config builds the configuration).
        It allocates levels * slots * (8 n_a + 16 n_b) bytes, freed by rot_end."""
        self._check(load_library().kmc_rot_begin(self._h, C.byref(config)))

    def rot_update(self) -> capi.RotInfo:
        """Correlate the current body vectors with every stored origin that is due and store the new origins; legal
        exactly `every` steps after the last update (or the begin)."""
        info = capi.RotInfo()
        self._check(load_library().kmc_rot_update(self._h, C.byref(info)))
        return info

    def rot_sample(self) -> capi.RotSample:
        """The table accumulated since rot_begin — kmc_rot_sample; analysis.rot_curves turns it into C_1 and C_2 by
        lag time."""
        out = capi.RotOut()
        self._check(load_library().kmc_rot_sample(self._h, C.byref(out), None, None))
        table = np.zeros((int(out.rows), capi.LAG_CLASSES, capi.ROT_VECS), dtype=capi.ROT_CELL_DTYPE)
        n_pairs = np.zeros(int(out.rows), dtype=np.int64)
        self._check(load_library().kmc_rot_sample(self._h, C.byref(out), table.ctypes.data, n_pairs.ctypes.data))
        return capi.RotSample(out, table, n_pairs)

    def rot_arrays(self):
        """(vec[n_a + 2 n_b] uint64: packed headings, axes, arms (capi.rot_unpack); last_event[N] int32; chi[N] int8)
        by reference index (kmc_rot_arrays): diagnostics and tests."""
        n_a, n_b = self.params.n_a, self.params.n_b
        vec = np.zeros(n_a + 2 * n_b, dtype=np.uint64)
        last_event = np.zeros(n_a + n_b, dtype=np.int32)
        chi = np.zeros(n_a + n_b, dtype=np.int8)
        self._check(load_library().kmc_rot_arrays(self._h, vec.ctypes.data, last_event.ctypes.data, chi.ctypes.data))
        return vec, last_event, chi

    def rot_end(self) -> None:
        self._check(load_library().kmc_rot_end(self._h))

    def run_rotated(self, nsteps: int):
        """Advance nsteps steps, `every` of the begun recorder's configuration at a time, with a rot_update after
        each piece (nsteps must be a multiple of every).  Returns (records[nsteps], the last capi.RotInfo or None)."""
        out = capi.RotOut()
        self._check(load_library().kmc_rot_sample(self._h, C.byref(out), None, None))
        every = int(out.cfg.every)
        if nsteps < 0 or nsteps % every:
            raise ValueError("run_rotated: nsteps >= 0, a multiple of the recorder's every")
        recs = np.zeros(nsteps, dtype=capi.OBS_DTYPE)
        done, info = 0, None
        while done < nsteps:
            self.step(every, recs[done:done + every])
            done += every
            info = self.rot_update()
        return recs, info

    def ligand_pose(self, nz: int, nc: int):
        """(hist[4, nz, nc] int64, capi.PoseOut): the ligands of the current state by occupied sites, height of bead
        [1][1] and z component of the axis (kmc_ligand_pose); analysis.pose_profile normalises it."""
        ok = 1 <= nz <= capi.POSE_MAX_BINS and 1 <= nc <= capi.POSE_MAX_BINS
        hist = np.zeros((capi.POSE_CLASSES, nz, nc) if ok else (1,), dtype=np.int64)
        out = capi.PoseOut()
        self._check(load_library().kmc_ligand_pose(self._h, int(nz), int(nc), hist.ctypes.data, C.byref(out)))
        return hist, out

    # ---- encounter statistics (kmc_encounter.hip)
    def reach_census(self, nd: int = 16, na: int = 18):
        """(capi.ReachOut, hist_d[3, 2, nd], hist_a_rl[na, na], hist_a_cis[2, na]) of the current state: the R–L
        triples and cis pairs within the engine's reaction distance, by channel (RL, MONO, CX), reactive flag and
        distance bin, and over the gate angles (kmc_reach_census); analysis.reach_factors post-processes them."""
        rc, res = _reach_call(load_library().kmc_reach_census, (self._h,), nd, na)
        self._check(rc)
        return res

    def enc_begin(self, cfg: capi.EncConfig = None) -> None:
        """Start the R–L encounter recorder at the current state: the encounters that are open are left-censored."""
        cfg = cfg if cfg is not None else capi.enc_config(1)
        self._check(load_library().kmc_enc_begin(self._h, C.byref(cfg)))

    def enc_update(self) -> capi.EncOut:
        """Record the encounters that opened, continued or ended since the last update; due exactly cfg.every steps
        after it."""
        out = capi.EncOut()
        self._check(load_library().kmc_enc_update(self._h, C.byref(out)))
        return out

    def enc_sample(self) -> capi.EncSample:
        """capi.EncSample of the recorder as of the last update — kmc_enc_sample; analysis.encounter_rates and
        analysis.escape_probability post-process it."""
        out = capi.EncOut()
        hist = np.zeros((capi.ENC_HISTS, capi.ENC_BINS), dtype=np.int64)
        react = np.zeros((2, capi.ENC_BINS), dtype=np.int64)
        self._check(load_library().kmc_enc_sample(self._h, C.byref(out), hist.ctypes.data, react.ctypes.data))
        return capi.EncSample(out, hist, react)

    def enc_arrays(self) -> capi.EncArrays:
        """The recorder's per-receptor arrays by reference index (kmc_enc_arrays): diagnostics and tests."""
        a = capi.EncArrays(self.params.n_a)
        self._check(load_library().kmc_enc_arrays(self._h, C.byref(a.view())))
        return a

    def enc_end(self) -> None:
        self._check(load_library().kmc_enc_end(self._h))

    @property
    def enc_phase_ms(self):
        """Device milliseconds of the last reach_census / enc_begin / enc_update: (binning and the distance walk,
        the gates, the rest)."""
        ms = (C.c_double * 3)()
        load_library().kmc_enc_phase_ms(self._h, ms)
        return tuple(float(x) for x in ms)

    # ---- proximity clusters (kmc_proximity.hip)
    def prox_clusters(self, which, eps: float, min_pts: int = 1, select="all", mask=None, max_size: int = 256,
                      nbins: int = 64, per_protein: bool = False):
        """DBSCAN / friends-of-friends clusters of the current state at the search radius eps — kmc_prox_clusters:
        (size_hist[max_size + 1], nn_hist[64], nnd_hist[nbins] int64, capi.ProxOut) and, with per_protein,
        (label[N], nn[N] int32, kind[N] uint8) by reference index, N = n_a + n_b.  which 'A', 'B' or 'AB' (both
        species as one point set); select 'all' or 'bound'; mask: None or N entries by reference index, non-zero
        keeps the protein (labelling efficiency); min_pts = 1 is friends-of-friends.  The histograms and
        out.counts() add over replicas (analysis.reduce_counts); analysis.prox_summary and analysis.nn_distance
        post-process them."""
        rc, res = _prox_call(load_library().kmc_prox_clusters, (self._h,), self.params.n_a + self.params.n_b, which,
                             eps, min_pts, select, mask, max_size, nbins, per_protein)
        self._check(rc)
        return res

    @property
    def prox_phase_ms(self):
        """Device milliseconds of the last prox_clusters: (select and bin, the count walk, the union walk and the
        flatten, the border walk with the bond components and the reduces)."""
        ms = (C.c_double * 4)()
        load_library().kmc_prox_phase_ms(self._h, ms)
        return tuple(float(x) for x in ms)

    def run_encounters(self, nsteps: int, every: int = 1):
        """Advance nsteps steps (a multiple of every) in pieces of `every` steps with an enc_update after each.
        The recorder must have been begun with that `every`.  Returns (records[nsteps], the last update's
        capi.EncOut or None)."""
        if nsteps < 0 or every < 1 or nsteps % every:
            raise ValueError("run_encounters: nsteps >= 0 a multiple of every >= 1")
        recs = np.zeros(nsteps, dtype=capi.OBS_DTYPE)
        done, out = 0, None
        while done < nsteps:
            self.step(every, recs[done:done + every])
            done += every
            out = self.enc_update()
        return recs, out

    @property
    def current_step(self) -> int:
        return int(load_library().kmc_current_step(self._h))

    # ---- one slab's window of a decomposed trajectory (kmc_dd_*, slabs.py)
    def dd_set_state(self, hs: capi.HostState, gid: np.ndarray, own: np.ndarray, ctl5) -> None:
        gid = np.ascontiguousarray(gid, dtype=np.int32)
        own = np.ascontiguousarray(own, dtype=np.uint8)
        c5 = np.ascontiguousarray(ctl5, dtype=np.int32)
        n = self.params.n_a + self.params.n_b
        if gid.size != n or own.size != n or c5.size != 5:
            raise ValueError("dd_set_state: gid / own sized n_a + n_b, ctl5 five values")
        v = hs.view()
        self._check(load_library().kmc_dd_set_state(self._h, C.byref(v), gid.ctypes.data, own.ctypes.data,
                                                    c5.ctypes.data))

    def dd_export(self, ids: np.ndarray):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        beads = np.zeros((ids.size, 48), dtype=np.float64)
        ints = np.zeros((ids.size, 8), dtype=np.int32)
        self._check(load_library().kmc_dd_export(self._h, ids.size, ids.ctypes.data, beads.ctypes.data,
                                                 ints.ctypes.data))
        return beads, ints

    def dd_import(self, ids: np.ndarray, beads: np.ndarray, ints: np.ndarray) -> np.ndarray:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        beads = np.ascontiguousarray(beads, dtype=np.float64)
        ints = np.ascontiguousarray(ints, dtype=np.int32)
        if beads.shape != (ids.size, 48) or ints.shape != (ids.size, 8):
            raise ValueError("dd_import: beads [n, 48], ints [n, 8]")
        flags = np.zeros(ids.size, dtype=np.uint8)
        self._check(load_library().kmc_dd_import(self._h, ids.size, ids.ctypes.data, beads.ctypes.data,
                                                 ints.ctypes.data, flags.ctypes.data))
        return flags

    def dd_drift(self) -> float:
        x = C.c_double()
        self._check(load_library().kmc_dd_drift(self._h, C.byref(x)))
        return float(x.value)

    def dd_counters(self):
        out = np.zeros(2, dtype=np.int64)
        self._check(load_library().kmc_dd_counters(self._h, out.ctypes.data))
        return int(out[0]), int(out[1])

    def dd_jumpers(self, S: float):
        """(local ids, x) of the owned proteins displaced more than S Å."""
        cap = 256
        while True:
            ids = np.zeros(cap, dtype=np.int32)
            xs = np.zeros(cap, dtype=np.float64)
            n = C.c_int32()
            self._check(load_library().kmc_dd_jumpers(self._h, S, cap, ids.ctypes.data, xs.ctypes.data, C.byref(n)))
            if n.value <= cap:
                return ids[: n.value], xs[: n.value]
            cap = n.value

    # the device-resident exchange (kmc_dd_plan / pack / unpack / finish)
    def dd_plan(self, send_ids: np.ndarray, recv_ids: np.ndarray, own: np.ndarray, band: np.ndarray) -> None:
        send_ids = np.ascontiguousarray(send_ids, dtype=np.int32)
        recv_ids = np.ascontiguousarray(recv_ids, dtype=np.int32)
        own = np.ascontiguousarray(own, dtype=np.uint8)
        band = np.ascontiguousarray(band, dtype=np.uint8)
        n = self.params.n_a + self.params.n_b
        if own.size != n or band.size != n:
            raise ValueError("dd_plan: own / band sized n_a + n_b")
        self._check(load_library().kmc_dd_plan(self._h, send_ids.size, send_ids.ctypes.data, recv_ids.size,
                                               recv_ids.ctypes.data, own.ctypes.data, band.ctypes.data))

    def dd_pack(self, dst: int = 0) -> int:
        """Pack the plan's rows into device address dst (0: the handle's own
        send buffer); returns the address written."""
        L = load_library()
        self._check(L.kmc_dd_pack(self._h, dst or None))
        return dst or int(L.kmc_dd_send_buffer(self._h) or 0)

    def dd_unpack(self, src: int, first: int, n: int) -> None:
        self._check(load_library().kmc_dd_unpack(self._h, src, first, n))

    def dd_step(self, dst: int, S: float) -> np.ndarray:
        """One step of the window, its exchange rows packed into device
        address dst (0: the handle's send buffer) and its jumpers beyond S
        listed, in one wait; returns the step's record."""
        out = np.zeros(1, dtype=capi.OBS_DTYPE)
        self._check(load_library().kmc_dd_step(self._h, dst or None, S, out.ctypes.data_as(C.c_void_p)))
        return out

    def dd_send_address(self) -> int:
        return int(load_library().kmc_dd_send_buffer(self._h) or 0)

    def dd_finish(self) -> capi.DDReport:
        rep = capi.DDReport()
        self._check(load_library().kmc_dd_finish(self._h, C.byref(rep)))
        return rep

    def dd_cut_count(self, ids: np.ndarray) -> int:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        c = C.c_int32()
        self._check(load_library().kmc_dd_cut_count(self._h, ids.size, ids.ctypes.data, C.byref(c)))
        return int(c.value)

    @property
    def list_growth(self) -> int:
        return int(load_library().kmc_list_growth(self._h))

    def set_list_growth(self, level: int) -> None:
        self._check(load_library().kmc_set_list_growth(self._h, level))

    def set_timing(self, kernels=(), every: int = 1):
        """Bracket the named kernels with HIP events (empty: off), in every
        `every`-th step only."""
        names = kernel_names()
        mask = 0
        for k in kernels:
            mask |= 1 << names.index(k)
        self._check(load_library().kmc_set_timing(self._h, mask))
        self._check(load_library().kmc_set_timing_period(self._h, every))

    def kernel_times(self) -> dict:
        """{kernel: (total_ms, launches)} accumulated since set_timing."""
        ms = (C.c_double * 64)()
        cnt = (C.c_int64 * 64)()
        n = load_library().kmc_kernel_times(self._h, ms, cnt, 64)
        names = kernel_names()
        return {names[i]: (ms[i], cnt[i]) for i in range(n) if cnt[i]}


def kernel_names():
    L = load_library()
    out = []
    i = 0
    while True:
        nm = L.kmc_kernel_name(i).decode()
        if not nm:
            return out
        out.append(nm)
        i += 1
