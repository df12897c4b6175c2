/* kmc.h — C-ABI of libkmc, the MI355X (gfx950) engine for the per-timestep
 * KMC diffusion–reaction loop of xiaopuren/KMC-with-a-diffusion-reaction-
 * algorithm.
 *
 * The reference has no plugin/FFI surface: its "interface"
 * is the set of global arrays main() mutates (main.cpp:102-168) and the
 * process/file contract (position.cpt in, bond.dat/position.cpt out,
 * main.cpp:226-270, 2206-2253).  This header is the drop-in boundary a host
 * program binds instead: plain pointers and sizes, no torch types, int return
 * codes (0 = ok, < 0 = error; kmc_last_error() has the message).  One handle
 * per GPU; a handle is used by one host thread at a time.
 *
 * Indices inside state buffers follow the reference exactly: proteins are
 * 1-based, receptors ("protein_A") are 1..n_a, ligands ("protein_B") are
 * n_a+1..n_a+n_b, and 0 means "no neighbour" (main.cpp:117, 1926-1928).
 */
#ifndef KMC_H
#define KMC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMC_OK 0
#define KMC_ERR_ARG (-1)       /* bad argument / size mismatch */
#define KMC_ERR_IO (-2)        /* file could not be opened or written */
#define KMC_ERR_FORMAT (-3)    /* malformed position.cpt */
#define KMC_ERR_STATE (-4)     /* bond links inconsistent (status vs res_nei) */
#define KMC_ERR_PLACEMENT (-5) /* random placement exhausted its attempts */
#define KMC_ERR_CAPACITY (-6)  /* a fixed device capacity was exceeded */
#define KMC_ERR_HIP (-7)       /* HIP runtime error */
#define KMC_ERR_GEOMETRY (-8)  /* a rigid body left the cell-list extent bound */
#define KMC_ERR_NODEVICE (-9)  /* no gfx950 device / kernels not loaded */

/* Physics + run parameters.  Defaults (kmc_params_default) equal the
 * reference globals at main.cpp:39-99. */
typedef struct kmc_params {
  int32_t n_a;               /* protein_A_tot_num (main.cpp:48) */
  int32_t n_b;               /* protein_B_tot_num (main.cpp:57) */
  double time_step;          /* ns (main.cpp:40) */
  double box_x, box_y, box_z;/* cell_range_x/y/z (main.cpp:43-45) */
  double pai;                /* 3.1415926 (main.cpp:71) */
  double ra_radius, ra_D, ra_rot_D;      /* main.cpp:72-74 */
  double rb_radius, rb_D, rb_rot_D;      /* main.cpp:76-78 */
  double mono_cis_ass_rate, mono_cis_diss_rate;           /* main.cpp:80-81 */
  double cis_D, cis_rot_D, cis_ass_rate, cis_diss_rate;   /* main.cpp:83-86 */
  double bond_D, bond_rot_D, ass_rate, diss_rate;         /* main.cpp:88-91 */
  double bond_dist_cutoff;   /* 18  (main.cpp:93) */
  double bond_thetapd_cutoff;/* 45  (main.cpp:95) */
  double bond_thetaot_cutoff;/* 90  (main.cpp:97) */
  double cis_thetaot_cutoff; /* 10  (main.cpp:98) */
  double cis_dist_cutoff;    /* 15  (main.cpp:99) */
  int64_t simu_step;         /* last step of a full run (main.cpp:39) */
  int32_t out_interval;      /* checkpoint / bond.dat cadence, 5000 (main.cpp:2206) */
  int32_t reserved0;
  uint64_t seed;             /* Philox key (replaces the clock seed of rand2) */
  uint32_t replica;          /* independent trajectory id (ensembles) */
  int32_t reserved1;
} kmc_params;

/* One record per simulated step: the bond.dat columns (main.cpp:2251) plus
 * the raw cluster sums they come from. */
typedef struct kmc_obs {
  int64_t step;                 /* mc_time_step */
  double t;                     /* mc_time_step * time_step */
  int32_t bond_num_rl;
  int32_t bond_num_mono_cis;
  int32_t bond_num_cis;
  int32_t bond_num;
  double cluster_size;          /* tot_proteins_in_cluster / tot_cluster_num */
  int32_t protein_num_in_max_complex;
  int32_t tot_proteins_in_cluster;
  int32_t tot_cluster_num;
  int32_t reserved;
} kmc_obs;

/* Host-side state buffers (caller-owned), structure-of-arrays, fp64.
 *   ra  : 48 * n_a doubles, ra[(((j-1)*4 + (k-1))*3 + c) * n_a + (i-1)]
 *         = R_{x,y,z}[i][j][k] of receptor i (j,k = 1..4; c = 0,1,2 → x,y,z)
 *   rb  : 24 * n_b doubles, rb[(((j-1)*2 + (k-1))*3 + c) * n_b + (b-1)]
 *         = R_{x,y,z}[n_a+b][j][k] of ligand b (j = 1..4, k = 1..2)
 *   a_int: 5 * n_a int32 in checkpoint order: protein_status[i][2],
 *         protein_status[i][3], res_nei[i][2], res_nei[i][4], res_nei[i][3]
 *         (a_int[f * n_a + (i-1)], main.cpp:240-244)
 *   b_int: 8 * n_b int32: protein_status[.][1..4] then res_nei[.][1..4]
 *   counters: bond_num, bond_num_rl, bond_num_cis, bond_num_mono_cis,
 *         protein_num_in_Max_Complex (main.cpp:261-265)
 *   step: the last completed mc_time_step (0 for a fresh configuration). */
typedef struct kmc_state_view {
  double* ra;
  double* rb;
  int32_t* a_int;
  int32_t* b_int;
  int32_t counters[5];
  int32_t reserved;
  int64_t step;
} kmc_state_view;

typedef struct kmc_sim kmc_sim;

/* Reference defaults (main.cpp:39-99); out_interval 5000, seed 1, replica 0. */
void kmc_params_default(kmc_params* p);

/* Create a simulation on HIP device `device` (-1 = current).
 *
 * Parameters outside this envelope are refused with KMC_ERR_ARG, before any
 * device is touched (inside it the engine is verified bit for bit against the
 * CPU restatement of the reference, which applies the same rule):
 *   - n_a >= 0, n_b >= 0, 1 <= n_a + n_b <= 2^24 (one species may be absent);
 *   - every double field finite: NaN and +-inf are refused everywhere;
 *   - box_x, box_y, box_z, time_step, pai, ra_radius, rb_radius,
 *     bond_dist_cutoff, cis_dist_cutoff, bond_thetapd_cutoff,
 *     bond_thetaot_cutoff, cis_thetaot_cutoff > 0;
 *   - ra_radius <= 20, rb_radius <= 30, bond_dist_cutoff <= 18,
 *     cis_dist_cutoff <= 15 (the reference's values, accepted exactly);
 *   - every D, rot_D and rate >= 0 (0 switches the move or reaction off). */
int kmc_create(const kmc_params* p, int device, kmc_sim** out);
int kmc_destroy(kmc_sim* s);
const char* kmc_last_error(const kmc_sim* s);

/* Random initial configuration with the reference's placement rules
 * (main.cpp:281-447: rejection of overlapping receptors / ligands, random
 * orientations), drawn from the keyed RNG; O(N) with a hash grid, so it also
 * serves the 1e6–1e7-particle configurations the reference's O(N^2) goto
 * sampler cannot reach.  Resets counters and sets step = 0. */
int kmc_init_random(kmc_sim* s);

/* position.cpt reader / writer, byte-compatible with main.cpp:226-270 and
 * main.cpp:2206-2244.  After a load the next simulated step is saved+1
 * (main.cpp:267). */
int kmc_load_cpt(kmc_sim* s, const char* path);
int kmc_write_cpt(kmc_sim* s, const char* path);

/* Exact checkpoint: the full-precision state, counters,
 * step, seed and replica in a binary file (KMCSTAT1 layout, FNV-1a trailer).
 * With the keyed random streams a load continues the trajectory bit for bit;
 * a file of another size, seed or replica is refused (KMC_ERR_ARG), a corrupt
 * one gives KMC_ERR_FORMAT.  position.cpt (3 decimals) cannot do this
 * (main.cpp:2208-2209). */
int kmc_save_state(kmc_sim* s, const char* path);
int kmc_load_state(kmc_sim* s, const char* path);

/* Copy the state in / out of the device (host buffers sized as above). */
int kmc_set_state(kmc_sim* s, const kmc_state_view* v);
int kmc_get_state(kmc_sim* s, kmc_state_view* v);

/* Advance nsteps time steps of the diffusion–reaction loop (main.cpp:461-2308)
 * on the GPU.  `out` (may be NULL) receives nsteps records. */
int kmc_step(kmc_sim* s, int64_t nsteps, kmc_obs* out);

/* Last completed step number. */
int64_t kmc_current_step(const kmc_sim* s);

/* Per-kernel device time, measured with HIP events on the handle's stream:
 * kmc_set_timing(s, mask) brackets the launches of the kernels whose id bit
 * is set (ids: kmc_kernel_name(0..n-1); 0 disables and resets; returns 0),
 * kmc_set_timing_period(s, every) brackets them only in every `every`-th step
 * (default 1: every step; an event pair costs a few microseconds of queue
 * time), and kmc_kernel_times returns the accumulated milliseconds and
 * launch counts since set_timing (returns the number of kernel ids).  Used
 * by bench.py for the roofline of the dominant kernel. */
int kmc_set_timing(kmc_sim* s, uint64_t kernel_mask);
int kmc_set_timing_period(kmc_sim* s, int32_t every);
int kmc_kernel_times(const kmc_sim* s, double* total_ms, int64_t* launches, int32_t n);
const char* kmc_kernel_name(int32_t id);

/* BFS member rows of the last simulated step (results[i][.] of main.cpp:537,
 * after the multi-ligand shuffles): for each ligand b, row_len[b] members
 * (reference 1-based indices) are appended to `members` (n_a+n_b capacity);
 * non-root ligands have row_len 0.  Feeds cluster.log (main.cpp:2291-2305).
 * KMC_ERR_ARG before the first step after a state was set, and after a
 * kmc_step that failed without keeping a step (the rows would not describe
 * the current state). */
int kmc_get_clusters(kmc_sim* s, int32_t* row_len, int32_t* members);

/* Structure analysis of the CURRENT state — what kmc_get_state would return —
 * computed on the device.  The calls work on any handle that
 * has a state, straight after kmc_set_state / kmc_load_* included (no step
 * needed, unlike kmc_get_clusters); they launch nothing inside kmc_step, read
 * no step-internal table and leave the state, the step counter and
 * kmc_get_clusters' validity untouched.  KMC_ERR_ARG for a null / out-of-range
 * argument, a handle without state and a decomposed (kmc_dd_set_state) handle;
 * KMC_ERR_STATE when a bond link leaves [0, n_a + n_b] or the links do not
 * form finite chains (the device loops are bounded, they cannot hang).
 *
 * The bond graph: vertices are the n_a + n_b proteins; a receptor's edges are
 * res_nei[.][2] (its ligand) and res_nei[.][3] (its cis partner), a ligand's
 * res_nei[.][2..4] — the links the reference's BFS follows (main.cpp:543-551),
 * but started from every protein, so receptor-only cis dimers are components
 * too.
 *   kmc_components       label[i-1] = the smallest reference index (1-based)
 *                        in protein i's component; label may be NULL (the
 *                        links are only checked).
 *   kmc_oligomer_census  hist[r * (max_l+1) + l] = components with r receptors
 *                        and l ligands, counts above max_r / max_l clamped
 *                        into the last row / column, so the bins sum to
 *                        n_components; hist may be NULL; at most
 *                        KMC_CENSUS_MAX_BINS bins on the device.  A "complex"
 *                        is the reference's cluster: at least one ligand and
 *                        more than one protein (tot_cluster_num,
 *                        tot_proteins_in_cluster of the NEXT step's record,
 *                        whose BFS starts from this state, main.cpp:514-562).
 *   kmc_pair_counts      lateral pair-distance histogram for g(r), species
 *                        pair `which`.  A protein's position is (x, y) of its
 *                        bead [1][1]; for a pair,
 *                          dx = xi - xj; dx = dx - box_x * round(dx / box_x)
 *                        (round half away from zero; the same in y),
 *                          d2 = dx*dx + dy*dy        (no fused multiply-add)
 *                        and with dr = r_max / nbins, edges2[m] = (m*dr)*(m*dr)
 *                        in double, the pair falls into bin
 *                          k = #{m in 1..nbins : edges2[m] <= d2}
 *                        and is counted when k < nbins.  AA and BB count each
 *                        unordered pair once, AB every (receptor, ligand)
 *                        pair once.  floor(box / r_max) must be >= 3 along x
 *                        and y, nbins <= KMC_PAIR_MAX_BINS.
 *   kmc_host_census      the same labels, histogram and summary from a host
 *                        state view, sequential, no device and no bin limit
 *                        (label, hist may be NULL). */
typedef struct kmc_census {
  int64_t n_components;          /* every component, free monomers included */
  int64_t n_complexes;           /* >= 1 ligand and size > 1 (the reference's "cluster") */
  int64_t proteins_in_complexes;
  int64_t n_cis_dimers;          /* receptor-only components of size 2 */
  int32_t max_size, max_receptors, max_ligands, max_label; /* largest component; ties: smallest label */
} kmc_census;
#define KMC_PAIR_AA 0
#define KMC_PAIR_AB 1
#define KMC_PAIR_BB 2
#define KMC_CENSUS_MAX_BINS 4096
#define KMC_PAIR_MAX_BINS 4096
int kmc_components(kmc_sim* s, int32_t* label);
int kmc_oligomer_census(kmc_sim* s, int32_t max_r, int32_t max_l, int64_t* hist, kmc_census* out);
int kmc_pair_counts(kmc_sim* s, int32_t which, double r_max, int32_t nbins, int64_t* counts);
int kmc_host_census(const kmc_params* p, const kmc_state_view* v, int32_t* label, int32_t max_r, int32_t max_l,
                    int64_t* hist, kmc_census* out);
/* Device milliseconds of the last kmc_components / kmc_oligomer_census /
 * kmc_pair_counts / kmc_track_* / kmc_kin_* / kmc_cf_* / kmc_unwrap / kmc_cluster_* / kmc_structure_factor /
 * kmc_bond_order / kmc_bond_order_corr / kmc_network / kmc_rings / kmc_reach_census / kmc_enc_* / kmc_prox_clusters call: HIP events on the handle's stream around
 * its kernels and clears (the result copies to the host excluded); 0 before
 * the first. */
double kmc_analysis_ms(const kmc_sim* s);

/* Displacement tracking: unwrapped displacements since a time
 * origin, for the mean-squared displacement and the self part of the van Hove
 * function, and the survival of the bonds that existed at the origin.  Like
 * the structure analysis the calls read the CURRENT state, launch nothing
 * inside kmc_step and leave the state, the step counter and kmc_get_clusters'
 * validity untouched; the caller places kmc_track_update between kmc_step
 * calls (kmc_step may replay steps internally, and slots are re-sorted: the
 * tracker is a layer of its own, indexed by reference index i = 0..N-1,
 * receptors first, then ligands).  A protein's position is (x, y) of its bead
 * [1][1], as in kmc_pair_counts.  One origin per handle.
 *
 *   kmc_track_begin   the current state becomes the origin: per protein
 *                     prev = position, u = (0, 0), flags = 0, the origin links
 *                     as reference indices (receptor: nei2, nei4, nei3; ligand:
 *                     nei2..4) and the origin class.  max_jump <= 0 means
 *                     min(box_x, box_y) / 4, else 0 < max_jump <= min(box) / 2.
 *                     Scratch is allocated by the first call, freed by
 *                     kmc_track_end / kmc_destroy.
 *   classes           0 receptor with nei2 == 0 and nei3 == 0 (free)
 *                     1 receptor with nei2 == 0 and nei3 != 0 (cis only)
 *                     2 receptor with nei2 != 0 (bound to a ligand)
 *                     3 ligand without a link     4 ligand with a link
 *                     — fixed at the origin.
 *   kmc_track_update  per protein, in double, no fused multiply-add:
 *                       dx = x - prev.x; dx = dx - box_x * round(dx / box_x)
 *                     (round half away from zero; the same in y),
 *                       u.x = u.x + dx; u.y = u.y + dy; prev = (x, y);
 *                     flags |= 2 ("jumped") when |dx| >= max_jump or |dy| >=
 *                     max_jump; flags |= 1 ("changed") when a current link (as
 *                     a reference index) or the receptor's nei4 differs from
 *                     the origin's.  Both bits are sticky.  info (may be NULL)
 *                     receives the steps, the number of updates, the largest
 *                     |dx| and |dy| of any update since begin, and how many
 *                     proteins carry each bit.  A second call at the same step
 *                     adds d = 0.
 *                     CAVEAT: a large minimum-image displacement is not an
 *                     error.  The model moves a cis dimer or a complex that
 *                     wraps around the box by up to sqrt(rot_D * time_step) * L
 *                     tangentially in that one step, far more
 *                     than diffusion does; such proteins are flagged "jumped"
 *                     and left out of the clean sums.
 *   kmc_track_sample  read-only over the tracker as of the last update.  With
 *                     q[i] = u.x*u.x + u.y*u.y: per class n, n_clean (flags ==
 *                     0), sum_u2 and sum_u2_clean; the survival counters — R–L
 *                     bonds counted at the receptor: rl0 (origin nei2 != 0),
 *                     rl_now (the current nei2 and nei4 equal the origin's),
 *                     rl_kept (they did at every update so far); cis bonds at
 *                     the lower-index receptor: cis0, cis_now, cis_kept (nei3).
 *                     The ten double sums are defined bit for bit: the term of
 *                     protein i is q[i] if it belongs to the sum's set, else
 *                     0.0; the vector is padded with 0.0 to a multiple of 256;
 *                     each block of 256 is reduced by the halving tree — for
 *                     h = 128, 64, ..., 1: t[j] = t[j] + t[j + h] for j < h —
 *                     and the block results form the next vector, until one
 *                     value is left.
 *                     vanhove (may be NULL) [KMC_TRACK_CLASSES][nbins]: the
 *                     clean members of each class by q, with kmc_pair_counts'
 *                     bin rule: dr = r_max / nbins, edges2[m] = (m*dr)*(m*dr),
 *                     k = #{m in 1..nbins : edges2[m] <= q}, counted when
 *                     k < nbins; 1 <= nbins <= KMC_TRACK_MAX_BINS, r_max > 0.
 *   kmc_track_displacements  u as ux[N] then uy[N], and the flags (may be
 *                     NULL): diagnostics and tests.
 *   kmc_track_end     drops the tracker and frees its scratch.
 * KMC_ERR_ARG for a null / out-of-range argument, a handle without state, a
 * decomposed window and a tracker that was not begun; kmc_set_state,
 * kmc_load_*, kmc_init_random and kmc_dd_set_state drop the tracker (its
 * origin described another state). */
#define KMC_TRACK_CLASSES 5
#define KMC_TRACK_MAX_BINS 512
#define KMC_TRACK_CHANGED 1
#define KMC_TRACK_JUMPED 2
typedef struct kmc_track_info {
  int64_t origin_step, last_step; /* step of kmc_track_begin / of the last update */
  int64_t n_updates;
  double max_dx, max_dy;          /* largest |dx|, |dy| of one update since begin */
  int64_t n_jumped, n_changed;    /* proteins carrying the bit now */
} kmc_track_info;
typedef struct kmc_track_sample_t {
  int64_t origin_step, last_step;
  int64_t n[KMC_TRACK_CLASSES], n_clean[KMC_TRACK_CLASSES];
  double sum_u2[KMC_TRACK_CLASSES], sum_u2_clean[KMC_TRACK_CLASSES];
  int64_t rl0, rl_now, rl_kept, cis0, cis_now, cis_kept;
} kmc_track_sample_t;
int kmc_track_begin(kmc_sim* s, double max_jump);
int kmc_track_update(kmc_sim* s, kmc_track_info* info);
int kmc_track_sample(kmc_sim* s, double r_max, int32_t nbins, kmc_track_sample_t* out, int64_t* vanhove);
int kmc_track_displacements(kmc_sim* s, double* u, uint8_t* flags);
int kmc_track_end(kmc_sim* s);

/* Bond kinetics: the lifetime of every R–L and cis bond —
 * those born after the recorder began included, which the tracker's survival
 * counters cannot see —, the waiting time until a receptor that lost its
 * ligand binds again, to the same ligand or to another, and the event counts
 * and exposures behind the effective on- and off-rates.  Like the tracker the
 * recorder is a stateful layer of its own, independent of it (both may be
 * active at once): its calls read the CURRENT state, launch nothing inside
 * kmc_step, leave the state, the step counter and kmc_get_clusters' validity
 * untouched and are timed by kmc_analysis_ms; the caller places
 * kmc_kin_update between kmc_step calls.  All arithmetic is integer: the
 * device, kmc_host_kin_* and the tests agree by equality, and every output is
 * a plain sum, so the outputs of replicas add.  One recorder per handle.
 *
 * Bonds are named at receptors, by reference index i = 1..n_a, links as
 * reference indices (what kmc_get_state returns):
 *   R–L bond of i   the pair (lig, site) = (res_nei[i][2], res_nei[i][4]); it
 *                   is "the same bond" only while both are unchanged.
 *   cis bond {i, j} recorded at its lower-index member (i < j = res_nei[i][3]).
 *                   Its kind at an update is COMPLEX when res_nei[i][2] != 0 or
 *                   res_nei[j][2] != 0, else MONO — the reference's two
 *                   dissociation classes (cis_diss_rate / mono_cis_diss_rate).
 * The recorder, per receptor (kmc_kin_view):
 *   rl_lig, rl_site  int32  the current R–L bond (0, . : none)
 *   rl_since         int64  step at which the current R–L bond was first seen
 *   cis_with         int32  the current cis partner
 *   cis_since        int64  step at which the current cis bond was first seen
 *   last_lig         int32  ligand of the last ended R–L bond; 0: none since begin
 *   free_since       int64  step at which that loss was seen
 *   bits             uint8  KMC_KIN_RL_CENSORED: the R–L bond existed at begin
 *                           (left-censored); KMC_KIN_CIS_CENSORED: the cis bond
 *                           did; KMC_KIN_COMPLEX: the cis kind at the last
 *                           update was complex.  A censored bit is cleared
 *                           when the next bond of its sort is born.
 *
 *   kmc_kin_begin   the current links are stored; since = free_since = the
 *                   current step; last_lig = 0; bits = censored where a bond
 *                   exists, plus the kind bit; the occupancy is counted; every
 *                   histogram row and counter is zeroed.  Scratch is the
 *                   recorder's own: allocated by the first begin, freed by
 *                   kmc_kin_end / kmc_destroy.
 *   kmc_kin_update  at step t, with D = t - last_step, in this order:
 *                   1. exp_k += D * occ_k (the occupancy of the previous
 *                      update) for k = rl, mono, cx, free_receptor, free_site.
 *                   2. per receptor i, with cur = its current (lig, site, cis):
 *                      R–L ended (rl_lig != 0 and (lig, site) differs):
 *                        L = t - rl_since into row 1 if censored, else row 0;
 *                        rl_off++; last_lig = rl_lig; free_since = t; if
 *                        cur.lig != 0 also rl_swap++.
 *                      R–L born (cur.lig != 0 and (lig, site) differs):
 *                        rl_on++; if last_lig != 0, W = t - free_since into
 *                        row 5 when cur.lig == last_lig, else row 6;
 *                        rl_since = t; the censored bit is cleared.
 *                      cis ended (old = cis_with != 0, i < old, cur.cis != old):
 *                        L = t - cis_since into row 4 if censored, else row 3
 *                        if the kind bit says complex, else row 2;
 *                        cis_off_cx++ or cis_off_mono++ by the kind bit
 *                        (censored bonds included); if cur.cis != 0 also
 *                        cis_swap++.
 *                      cis born (cur.cis != 0 and cur.cis != old):
 *                        cis_since = t; the censored bit is cleared; if
 *                        i < cur.cis, cis_on++.
 *                      Then the stored links are replaced, the kind bit is set
 *                      from the current state and the occupancy counted:
 *                      occ_rl receptors with lig != 0; occ_mono / occ_cx cis
 *                      bonds at their lower member by kind; occ_free_receptor
 *                      = n_a - occ_rl; occ_free_site = 3 n_b - occ_rl.
 *                   A second update at the same step changes nothing but
 *                   n_updates.  out (may be NULL) receives the counters as of
 *                   this update (n_*_censored_alive are a sample's: 0 here).
 *                   With an update after every step the lifetimes are exact.
 *                   With one every k steps they are STROBOSCOPIC: a bond that
 *                   breaks and forms again identically between two looks
 *                   counts as unbroken, and lifetimes are multiples of k.
 *   bin rule        of every lifetime and waiting time v >= 0: b = v below 16;
 *                   else, with e the index of v's top bit,
 *                     b = 16 + 8 (e - 4) + ((v >> (e - 3)) & 7),
 *                   clamped to KMC_KIN_BINS - 1: eight bins per octave, exact
 *                   below 16; v >= 2^34 falls into the last bin.
 *   kmc_kin_sample  read-only over the recorder as of the last update: out, and
 *                   hist (may be NULL) [KMC_KIN_HISTS][KMC_KIN_BINS]: rows 0-6
 *                   as accumulated by the updates; row 7 the ages last_step -
 *                   rl_since of the living non-censored R–L bonds, row 8 those
 *                   of the living non-censored cis bonds at their lower member
 *                   — the right-censored observations of a survival estimate.
 *                   n_rl_censored_alive / n_cis_censored_alive count the
 *                   living bonds that rows 7 / 8 leave out.
 *   kmc_kin_get     copies the per-receptor arrays out (every pointer of the
 *                   view is needed, n_a entries each): tests and diagnostics.
 *   kmc_kin_end     drops the recorder and frees its scratch.
 *   kmc_host_kin_*  the same, sequentially, from host state views, no device:
 *                   the recorder is the caller's view, acc and hist7
 *                   [7][KMC_KIN_BINS]; begin fills them from state v (origin
 *                   v->step), update advances them to state v, sample writes
 *                   out and hist9 [9][KMC_KIN_BINS] (may be NULL).
 * KMC_ERR_ARG for a null argument, a handle without state, a decomposed window
 * and a recorder that was not begun; kmc_set_state, kmc_load_*,
 * kmc_init_random and kmc_dd_set_state drop the recorder.  KMC_ERR_STATE when
 * a receptor's link leaves its range — res_nei[i][2] in {0} or (n_a, n_a +
 * n_b], res_nei[i][3] in {0} or [1, n_a] and not i, res_nei[i][4] in [0, 4] —
 * nothing is read through such a link, and the recorder is dropped. */
#define KMC_KIN_BINS 256
#define KMC_KIN_HISTS 9
#define KMC_KIN_RL_CENSORED 1
#define KMC_KIN_CIS_CENSORED 2
#define KMC_KIN_COMPLEX 4
typedef struct kmc_kin_out {
  int64_t origin_step, last_step; /* step of kmc_kin_begin / of the last update */
  int64_t n_updates;
  int64_t rl_on, rl_off, rl_swap, cis_on, cis_off_mono, cis_off_cx, cis_swap; /* events since begin */
  int64_t exp_rl, exp_mono, exp_cx, exp_free_receptor, exp_free_site;         /* bond-steps / free steps since begin */
  int64_t occ_rl, occ_mono, occ_cx, occ_free_receptor, occ_free_site;         /* at the last update */
  int64_t n_rl_censored_alive, n_cis_censored_alive;                          /* kmc_kin_sample only */
} kmc_kin_out;
typedef struct kmc_kin_view {
  int32_t *rl_lig, *rl_site;
  int64_t* rl_since;
  int32_t* cis_with;
  int64_t* cis_since;
  int32_t* last_lig;
  int64_t* free_since;
  uint8_t* bits;
} kmc_kin_view;
int kmc_kin_begin(kmc_sim* s);
int kmc_kin_update(kmc_sim* s, kmc_kin_out* out);
int kmc_kin_sample(kmc_sim* s, kmc_kin_out* out, int64_t* hist);
int kmc_kin_get(kmc_sim* s, const kmc_kin_view* view);
int kmc_kin_end(kmc_sim* s);
int kmc_host_kin_begin(const kmc_params* p, const kmc_state_view* v, const kmc_kin_view* view, kmc_kin_out* acc,
                       int64_t* hist7);
int kmc_host_kin_update(const kmc_params* p, const kmc_state_view* v, const kmc_kin_view* view, kmc_kin_out* acc,
                        int64_t* hist7);
int kmc_host_kin_sample(const kmc_params* p, const kmc_kin_view* view, const kmc_kin_out* acc, const int64_t* hist7,
                        kmc_kin_out* out, int64_t* hist9);

/* Cluster geometry: a periodic image for every protein, the
 * spanning (percolation) bits of every component, and the exact integer
 * moments behind the radius of gyration and the gyration tensor.  Like the
 * structure analysis the calls read the CURRENT state on the device in a
 * fixed number of launches, launch nothing inside kmc_step, leave the state,
 * the step counter and kmc_get_clusters' validity untouched and are timed by
 * kmc_analysis_ms; their scratch is their own (allocated by the first call,
 * freed by kmc_destroy), so they interleave freely with kmc_components /
 * kmc_oligomer_census / kmc_pair_counts / kmc_track_*.
 *
 * Definitions — the device, kmc_host_cluster_geometry and the tests share
 * them bit for bit (doubles, no fused multiply-add, round = half away from
 * zero):
 *   graph, position   the bond graph of kmc_components; a protein's position
 *                     is (x, y) of its bead [1][1], as in kmc_pair_counts.
 *   integer coords    X_i = (int64) round(x_i * 1024.0), BX = (int64)
 *                     round(box_x * 1024.0); the same in y.  The quantum is
 *                     2^-10 A; the product is exact.
 *   edge shift        for a bond i-j seen from i,
 *                       n_x(i->j) = -(int) round((x_j - x_i) / box_x)
 *                     (the same in y); n(j->i) = -n(i->j), ties at half a box
 *                     included.
 *   image shift       with r the component's label (its smallest reference
 *                     index): off(r) = (0, 0) and off(j) = off(i) + n(i->j)
 *                     along any bond path; the unwrapped coordinate is
 *                     U_i = X_i + off_x(i) * BX.
 *   spanning bits     a component carries bit 1 when some bond cycle has a
 *                     non-zero total n_x, bit 2 for n_y: for the offsets of
 *                     any spanning tree, some edge has off(j) - off(i) !=
 *                     n(i->j) on that axis.  The bits do not depend on the
 *                     tree.  The offsets of a spanning component are not
 *                     unique: its members report shift (0, 0) and it is left
 *                     out of all moments.
 *   moments           for a component of size n >= 2 without spanning bits,
 *                     D_i = U_i - U_r per axis:
 *                       S1x = sum Dx, S1y = sum Dy                  (int64)
 *                       S2xx = sum Dx^2, S2yy = sum Dy^2, S2xy = sum Dx*Dy
 *                                          (128 bits, terms and sums exact)
 *                       m = n * (S2xx + S2yy) - (S1x^2 + S1y^2)  (128 bits, >= 0)
 *                       Rg^2 = m / n^2 / 2^20                       (A^2)
 *                     A kmc_i128 is the two's-complement number hi * 2^64 + lo.
 *
 *   kmc_unwrap            label[i-1] as kmc_components; shift = sx[N] then
 *                         sy[N], the image shift of every protein ((0, 0) in
 *                         a spanning component); span[i-1] = the bits of
 *                         protein i's component.  Every output may be NULL.
 *   kmc_cluster_geometry  table[k], k = min(size, max_size), over the
 *                         components without spanning bits and size >= 2:
 *                         their number, the sum of their sizes and the sum of
 *                         their m (bins 0 and 1 stay zero; the last bin is
 *                         the overflow bin: it holds one size only when
 *                         sum_size == count * max_size).  2 <= max_size <=
 *                         KMC_GEOM_MAX_SIZE; table may be NULL.  out: the
 *                         measured and the spanning components, and the
 *                         census' largest component (ties: smallest label)
 *                         with its bits.
 *   kmc_cluster_list      one row per component of at least min_size (>= 2)
 *                         members, spanning ones included (their sums are
 *                         zero), sorted by label.  When more than cap
 *                         qualify: KMC_ERR_CAPACITY, *n = the true count and
 *                         rows unspecified; otherwise *n rows are written.
 *                         rows may be NULL when cap is 0.
 *   kmc_host_cluster_geometry  kmc_unwrap's and kmc_cluster_geometry's
 *                         outputs from a host state view: a sequential
 *                         breadth-first walk from each label, no device, no
 *                         bin limit (every output but out may be NULL).
 * KMC_ERR_ARG for a null / out-of-range argument, a handle without state and a
 * decomposed window; KMC_ERR_STATE when a bond link leaves [0, n_a + n_b] or
 * the links do not form finite chains (every device loop is bounded by
 * n_a + n_b: none can hang); KMC_ERR_CAPACITY when an edge or an accumulated
 * image shift leaves [-32767, 32767] (the device keeps them as int16). */
#define KMC_GEOM_MAX_SIZE 1023
#define KMC_SPAN_X 1
#define KMC_SPAN_Y 2
typedef struct kmc_i128 { uint64_t lo; int64_t hi; } kmc_i128;
typedef struct kmc_geom_bin { int64_t count, sum_size; kmc_i128 sum_m; } kmc_geom_bin;
typedef struct kmc_geom {
  int64_t n_measured;            /* components without spanning bits and size >= 2 */
  int64_t n_spanning, n_span_x, n_span_y, proteins_in_spanning;
  int32_t largest_label, largest_size, largest_span, reserved; /* the census' largest component and its bits */
} kmc_geom;
typedef struct kmc_cluster {
  int32_t label, n_r, n_l, span;
  int64_t s1x, s1y;
  kmc_i128 s2xx, s2yy, s2xy;     /* zero when span != 0 */
} kmc_cluster;
int kmc_unwrap(kmc_sim* s, int32_t* label, int32_t* shift, uint8_t* span);
int kmc_cluster_geometry(kmc_sim* s, int32_t max_size, kmc_geom_bin* table, kmc_geom* out);
int kmc_cluster_list(kmc_sim* s, int32_t min_size, int64_t cap, kmc_cluster* rows, int64_t* n);
int kmc_host_cluster_geometry(const kmc_params* p, const kmc_state_view* v, int32_t* label, int32_t* shift,
                              uint8_t* span, int32_t max_size, kmc_geom_bin* table, kmc_geom* out);

/* Cluster growth kinetics: which clusters merged and which
 * fell apart between two looks, by size — the size-resolved coagulation and
 * fragmentation events ("cf") behind K(a, b) and F(a, b), how many pieces an
 * event had, of what kind the pieces of a binary event were, and how often a
 * new bond closed a ring instead of joining two clusters.  Like the kinetics
 * recorder it is a stateful layer of its own, independent of it and of the
 * tracker (all three may be active at once): its calls read the CURRENT state,
 * launch nothing inside kmc_step, leave the state, the step counter and
 * kmc_get_clusters' validity untouched and are timed by kmc_analysis_ms; the
 * caller places kmc_cf_update between kmc_step calls.  All arithmetic is
 * integer: the device, kmc_host_cf_* and the tests agree by equality, and
 * every table and counter but n_cores, n_clusters, max_cluster and n_s is a
 * plain sum, so the outputs of replicas add.  One recorder per handle.
 *
 * Graphs.  The vertices are the N proteins by reference index 1..N.  A bond
 * is an unordered pair: a receptor's R–L bond {i, res_nei[i][2]} (the site is
 * not part of it: the same ligand at another site is the same edge) and its
 * cis bond {i, res_nei[i][3]}.  E0 is the set of bonds stored at the last look
 * (begin, update or put), E1 that of the current state, K = E0 ∩ E1 the kept
 * bonds.  The PREVIOUS clusters are the components of E0, the CURRENT clusters
 * those of E1, the CORES those of K; a core lies inside exactly one previous
 * and one current cluster.  A label is the component's smallest reference
 * index (kmc_components').  The interval between two looks is read as "all
 * breaks, then all bonds formed": previous clusters fall into their cores,
 * cores join into current clusters.
 *
 * Events of one update.  With k0(P) the number of cores of previous cluster P
 * and k1(C) that of current cluster C: P fragments iff k0(P) >= 2, C is the
 * product of a merger iff k1(C) >= 2.  A size n has the index min(n, S), S
 * the max_size of the begin (index S: "S or more"; index 0 is unused); the
 * tables hold (S + 1)^2 bins [lo][hi] of which the upper triangle lo <= hi is
 * used.  The kind of a piece follows from its (receptors, ligands): 0 a single
 * receptor, 1 a single ligand, 2 a receptor-only pair, 3 anything else.
 *   every fragmenting P   frag_pieces[min(k0, 8)] += 1, frag_parent[|P|] += 1
 *                         (filed by the core whose root is P's label)
 *   k0(P) == 2            also frag[a][b] += 1 for the two pieces' sizes a <= b
 *                         and frag_kind[k_lo][k_hi] += 1 for their kinds (filed
 *                         by the core whose root is not P's label)
 *   every merged C        merge_pieces[min(k1, 8)], merge_product[|C|], and with
 *   k1(C) == 2            merge[a][b], merge_kind[k_lo][k_hi]: the mirror image.
 * Counters: formed_rl, formed_cis, broken_rl, broken_cis = |E1 \ E0| and
 * |E0 \ E1| by sort since begin; n_cores and n_clusters of the last update;
 * the change of the bond graph's cycle rank,
 *   cycles_closed += formed - (n_cores - n_clusters_current)
 *   cycles_opened += broken - (n_cores - n_clusters_previous)
 * (formed, broken: of this update); max_cluster, the largest current cluster.
 * Occupancy and exposure: n_s[S + 1] the current cluster-size histogram; with
 * D = step - last_step and n the n_s of the previous look,
 *   expo[s] += D n_s;  expo2[a][b] += D n_a n_b (a < b);
 *   expo2[a][a] += D n_a (n_a - 1) / 2          (a kmc_i128 per bin)
 * so that K(a, b) = merge[a][b] / expo2[a][b] and F(a, b) = frag[a][b] /
 * expo[a + b] per pair (per cluster) and step.
 *
 *   kmc_cf_begin    2 <= max_size <= KMC_CF_MAX_SIZE.  The current bonds and
 *                   clusters are stored, n_s counted, every table and counter
 *                   zeroed.  Scratch is the recorder's own: allocated by the
 *                   first begin, freed by kmc_cf_end / kmc_destroy.
 *   kmc_cf_update   files the events between the last look and the current
 *                   state as above; out (may be NULL) receives the counters.
 *                   With an update after every step the events are exact up to
 *                   simultaneous events inside one step; with one every k
 *                   steps they are STROBOSCOPIC: a bond that broke and formed
 *                   again between two looks is kept.  A second update at the
 *                   same step changes nothing but n_updates (the state is the
 *                   last look's: it is not read again).
 *   kmc_cf_sample  read-only over the recorder as of the last look: out, and
 *                   the tables (tables and each of its pointers may be NULL).
 *   kmc_cf_get      copies the recorder's per-protein state out: the stored
 *                   bonds rl_lig[n_a], cis_with[n_a] and the labels of the
 *                   last look prev_label[n_a + n_b] (all three are needed).
 *   kmc_cf_put      the mirror of get: loads a recorder state saved earlier or
 *                   built by kmc_host_cf_*, as of step last_step <= the current
 *                   step.  A recorder must have been begun (its max_size
 *                   stays).  The previous clusters' counts and n_s are
 *                   recounted, origin_step = last_step, every table and
 *                   counter is zeroed: totals add on the caller's side, as
 *                   those of replicas do.  It makes a recorder resumable
 *                   across a saved state.  The labels must be those of the
 *                   stored bonds' components; checked is that every label is
 *                   in [1, N] and the smallest member of its class and every
 *                   link in its range, else KMC_ERR_STATE (the recorder stays
 *                   as it was).
 *   kmc_cf_end      drops the recorder and frees its scratch.
 *   kmc_host_cf_*   the same, sequentially (breadth-first walks), from host
 *                   state views, no device: the recorder is the caller's view,
 *                   acc and tables (every pointer needed); begin fills them
 *                   from state v (origin v->step), update advances them to
 *                   state v, sample copies acc to out and the tables to
 *                   tables_out (may be NULL, and so may its pointers).
 * KMC_ERR_ARG for a null argument, a handle without state, a decomposed window
 * and a recorder that was not begun; kmc_set_state, kmc_load_*,
 * kmc_init_random and kmc_dd_set_state drop the recorder.  KMC_ERR_STATE when
 * a receptor's link leaves its range — res_nei[i][2] in {0} or (n_a, n_a +
 * n_b], res_nei[i][3] in {0} or [1, n_a] and not i — or a link chain does not
 * end: nothing is read through such a link, and the recorder is dropped. */
#define KMC_CF_MAX_SIZE 63
#define KMC_CF_PIECES 9
#define KMC_CF_KINDS 4
typedef struct kmc_cf_out {
  int64_t origin_step, last_step; /* step of kmc_cf_begin (or put) / of the last look */
  int64_t n_updates;
  int64_t max_size;                                     /* S */
  int64_t formed_rl, formed_cis, broken_rl, broken_cis; /* bonds since begin */
  int64_t n_cores, n_clusters;                          /* of the last update (n_cores: 0 before the first) */
  int64_t cycles_closed, cycles_opened;                 /* since begin */
  int64_t max_cluster;                                  /* largest current cluster */
} kmc_cf_out;
typedef struct kmc_cf_view {
  int32_t *rl_lig, *cis_with; /* [n_a] */
  int32_t* prev_label;        /* [n_a + n_b] */
} kmc_cf_view;
typedef struct kmc_cf_tables {
  int64_t *merge, *frag;                 /* [(S + 1)^2] */
  int64_t *merge_kind, *frag_kind;       /* [KMC_CF_KINDS^2] */
  int64_t *merge_pieces, *frag_pieces;   /* [KMC_CF_PIECES] */
  int64_t *merge_product, *frag_parent;  /* [S + 1] */
  int64_t *n_s, *expo;                   /* [S + 1] */
  kmc_i128* expo2;                       /* [(S + 1)^2] */
} kmc_cf_tables;
int kmc_cf_begin(kmc_sim* s, int32_t max_size);
int kmc_cf_update(kmc_sim* s, kmc_cf_out* out);
int kmc_cf_sample(kmc_sim* s, kmc_cf_out* out, const kmc_cf_tables* tables);
int kmc_cf_get(kmc_sim* s, const kmc_cf_view* view);
int kmc_cf_put(kmc_sim* s, const kmc_cf_view* view, int64_t last_step);
int kmc_cf_end(kmc_sim* s);
int kmc_host_cf_begin(const kmc_params* p, const kmc_state_view* v, int32_t max_size, const kmc_cf_view* view,
                      kmc_cf_out* acc, const kmc_cf_tables* tables);
int kmc_host_cf_update(const kmc_params* p, const kmc_state_view* v, const kmc_cf_view* view, kmc_cf_out* acc,
                       const kmc_cf_tables* tables);
int kmc_host_cf_sample(const kmc_params* p, const kmc_cf_view* view, const kmc_cf_out* acc,
                       const kmc_cf_tables* tables, kmc_cf_out* out, const kmc_cf_tables* tables_out);

/* Static structure factor: per species the sums of every
 * selected protein's (cos, sin) of q . r at the wave vectors of the half plane,
 * as exact integers.  Like the structure analysis the call reads the CURRENT
 * state on the device (valid straight after kmc_set_state / kmc_load_*),
 * launches nothing inside kmc_step, leaves the state, the step counter, the
 * tracker and kmc_get_clusters' validity untouched and is timed by
 * kmc_analysis_ms; its scratch is its own (allocated by the first call, freed
 * by kmc_destroy).
 *
 * Definitions — the device, kmc_host_structure_factor and the tests share
 * them bit for bit (doubles, no fused multiply-add; round = half away from
 * zero, sin and cos the library's own, kmc_math.h):
 *   position        (x, y) of bead [1][1], as in kmc_pair_counts.
 *   integer coords  X_i = (int64) round(x_i * 1024.0), BX = (int64)
 *                   round(box_x * 1024.0); the same in y (§12's 2^-10 A).
 *                   KMC_ERR_ARG when BX < 1 or BY < 1.
 *   wave vectors    q(h, k) = 2 pi (h / box_x, k / box_y), h = 0..hmax,
 *                   k = -kmax..kmax (the half plane: rho(-q) = conj rho(q));
 *                   0 <= hmax, kmax <= KMC_SK_MAX; nq = (hmax + 1)(2 kmax + 1),
 *                   (h, k) has index h (2 kmax + 1) + (k + kmax).
 *   axis phase      for a multiplier m >= 0 (h, or |k|), coordinate X, box B:
 *                     p = (m X) mod B in [0, B) (the floor modulus: X may be
 *                     negative); if (2 p >= B) p -= B;
 *                     t = (double) p / (double) B; a = 6.283185307179586 * t;
 *                     c = cos(a), s = sin(a)
 *                   — (cx, sx) from (h, X_i, BX), (cy, sy) from (|k|, Y_i, BY);
 *                   for k < 0, sy = -sy and cy is unchanged.
 *   term            re = cx*cy - sx*sy, im = sx*cy + cx*sy;
 *                   tc = (int64) round(re * 1073741824.0), ts = (int64)
 *                   round(im * 1073741824.0) (2^30: product and conversion
 *                   are exact).
 *   sums            C_A(q) = sum tc, S_A(q) = sum ts over the selected
 *                   receptors, C_B, S_B over the selected ligands: int64,
 *                   exact, the same bits in any order of summation;
 *                   |sum| < 2^62 for every N the engine accepts.
 *   selection       KMC_SK_ALL: every protein.  KMC_SK_BOUND: the receptors
 *                   with nei2 != 0 or nei3 != 0 and the ligands with any of
 *                   nei2..4 != 0 (the clustered phase).
 * sums is [4][nq]: C_A, S_A, C_B, S_B; n_sel = the receptors and the ligands
 * selected.  With rho = (C + i S) / 2^30 the partials are S_AA = |rho_A|^2 /
 * N_A, S_BB = |rho_B|^2 / N_B, S_AB = Re(rho_A conj rho_B) / sqrt(N_A N_B) and
 * S_NN = |rho_A + rho_B|^2 / (N_A + N_B).
 * kmc_host_structure_factor: the same from a host state view, sequentially, no
 * device.  KMC_ERR_ARG for a null / out-of-range argument, a handle without
 * state and a decomposed window. */
#define KMC_SK_MAX 64
#define KMC_SK_ALL 0
#define KMC_SK_BOUND 1
int kmc_structure_factor(kmc_sim* s, int32_t hmax, int32_t kmax, int32_t select,
                         int64_t* sums /* [4][nq]: C_A, S_A, C_B, S_B */, int64_t n_sel[2]);
int kmc_host_structure_factor(const kmc_params* p, const kmc_state_view* v, int32_t hmax, int32_t kmax,
                              int32_t select, int64_t* sums, int64_t n_sel[2]);

/* Bond-orientational order: the local n-fold order
 * psi_n(i) = (1/N_i) sum_j exp(i n theta_ij) of every selected protein of one
 * species, its histogram by neighbour count and |psi|, its global sums, and
 * the spatial correlation G_n(r) = <psi_n(i) psi_n*(j)>, as exact integers.
 * Like the other analyses the calls read the CURRENT state on the device
 * (valid straight after kmc_set_state / kmc_load_*), launch nothing inside
 * kmc_step, leave the state, the step counter, the tracker, kmc_get_clusters'
 * validity and the other analyses' scratch untouched and are timed by
 * kmc_analysis_ms; their scratch is their own (allocated by the first call,
 * freed by kmc_destroy).
 *
 * Definitions — the device, kmc_host_bond_order* and the tests share them bit
 * for bit (doubles, no fused multiply-add; round = half away from zero, atan2,
 * sin and cos the library's own, kmc_math.h):
 *   position        (x, y) of bead [1][1], as in kmc_pair_counts.
 *   integer coords  X = (int64) round(x * 1024.0), BX = (int64) round(box_x *
 *                   1024.0); the same in y (§12's 2^-10 A).  KMC_ERR_ARG
 *                   unless 1 <= BX, BY < 2^31.
 *   set             which = KMC_BO_A (receptors) or KMC_BO_B (ligands); select
 *                   = KMC_BO_ALL, or KMC_BO_BOUND: KMC_SK_BOUND's rule (a
 *                   receptor with nei2 != 0 or nei3 != 0, a ligand with any
 *                   of nei2..4 != 0).  Centres and neighbours both come from
 *                   this set.
 *   displacement    i -> j: DX = (X_j - X_i) mod BX in [0, BX) (the floor
 *                   modulus); if (2 DX >= BX) DX -= BX; the same in y;
 *                   D2 = DX*DX + DY*DY in int64.
 *   neighbours      KMC_BO_WITHIN: every j != i of the set with 0 < D2 <= RC^2,
 *                   RC = (int64) round(r_cut * 1024.0) — an integer test,
 *                   inclusive and symmetric; coincident points (D2 = 0) are
 *                   not neighbours.  Needs r_cut > 0 and floor(BX / RC) >= 3,
 *                   floor(BY / RC) >= 3 (integer division), else KMC_ERR_ARG.
 *                   KMC_BO_LINKED (ligands only; which = KMC_BO_A is
 *                   KMC_ERR_ARG; r_cut is ignored): for each link r != 0 of
 *                   ligand b's nei2..4: r' = receptor r's nei3 (its cis
 *                   partner; skipped when 0), b' = receptor r''s nei2
 *                   (skipped when 0, when b' = b, or when b' is not in the
 *                   set); b' is a neighbour.  At most three; a ligand reached
 *                   by two paths counts twice; a neighbour with D2 = 0 is
 *                   skipped.  The network's own neighbour relation.
 *   term            theta = atan2((double) DY, (double) DX); a = (double) n *
 *                   theta, 1 <= n = fold <= KMC_BO_MAX_FOLD;
 *                   tc = (int64) round(cos(a) * 1073741824.0), ts = (int64)
 *                   round(sin(a) * 1073741824.0) (2^30).  Every ordered pair
 *                   is evaluated from its centre's side: the term of j -> i
 *                   is not derived from that of i -> j.
 *   per protein     C_i = sum tc, S_i = sum ts, N_i = the number of neighbours
 *                   — int64, exact, the same bits in any order of summation.
 *                   N_i > 65535 anywhere: KMC_ERR_CAPACITY.  For N_i > 0
 *                   pc_i = (int64) round((double) C_i / ((double) N_i *
 *                   32768.0)), ps_i likewise from S_i (psi_i ~ (pc_i + i ps_i)
 *                   / 2^15; the operands are exact doubles); for N_i = 0
 *                   pc_i = ps_i = 0.  m_i = pc_i^2 + ps_i^2.
 *   histogram       hist[KMC_BO_NN_ROWS][nbins], 1 <= nbins <= 1024: every
 *                   selected protein in row min(N_i, 15), bin b = #{k in
 *                   1..nbins-1 : k^2 2^30 <= nbins^2 m_i} — a bin in |psi|
 *                   decided by integer comparison; the bins sum to n_sel.
 *   summary         kmc_bond_order_out: n_sel, n_with (N_i > 0), sum_nn = sum
 *                   N_i, sum_pc, sum_ps, sum_m over the selected proteins.
 *   per protein out C[n], S[n] (int64), nn[n] (int32) by the species' reference
 *                   index (n = n_a or n_b), zero for unselected proteins; a
 *                   NULL pointer skips that copy.  hist may be NULL too.
 *   correlation     corr[2][nbins], 1 <= nbins <= 4096, over the unordered
 *                   pairs i < j of the set with N_i > 0 and N_j > 0: dr =
 *                   r_max / nbins, E_m = (int64) round(((double) m * dr) *
 *                   1024.0), bin k = #{m in 1..nbins : E_m^2 <= D2}; counted
 *                   when k < nbins: corr[0][k] += pc_i pc_j + ps_i ps_j,
 *                   corr[1][k] += 1.  Needs r_max > 0, floor(box / r_max) >= 3
 *                   and floor(BX / E_nbins) >= 3 on both axes, else
 *                   KMC_ERR_ARG.  G_n(r_k) = corr[0][k] / corr[1][k] / 2^30;
 *                   only the real part: the imaginary part changes sign with
 *                   the order of the pair.
 * kmc_bond_order_corr is self-contained: it runs the local pass itself.
 * kmc_host_bond_order / kmc_host_bond_order_corr: the same from a host state
 * view, sequentially on a cell grid of their own, no device.
 * KMC_ERR_ARG for a null / out-of-range argument, a handle without state and a
 * decomposed window; KMC_ERR_STATE (KMC_BO_LINKED) when a ligand's link is not
 * a receptor in [0, n_a], a receptor's nei3 not a receptor or its nei2 not 0
 * or a ligand in (n_a, n_a + n_b]; every device loop is bounded, so a bad link
 * ends the call and cannot hang. */
#define KMC_BO_A 0
#define KMC_BO_B 1
#define KMC_BO_WITHIN 0
#define KMC_BO_LINKED 1
#define KMC_BO_ALL 0
#define KMC_BO_BOUND 1
#define KMC_BO_MAX_FOLD 12
#define KMC_BO_NN_ROWS 16
typedef struct kmc_bond_order_out {
  int64_t n_sel, n_with, sum_nn, sum_pc, sum_ps, sum_m;
} kmc_bond_order_out;
int kmc_bond_order(kmc_sim* s, int32_t which, int32_t mode, int32_t fold, double r_cut, int32_t select,
                   int32_t nbins, int64_t* hist /* [KMC_BO_NN_ROWS][nbins] */, kmc_bond_order_out* out,
                   int64_t* C, int64_t* S, int32_t* nn);
int kmc_bond_order_corr(kmc_sim* s, int32_t which, int32_t mode, int32_t fold, double r_cut, int32_t select,
                        double r_max, int32_t nbins, int64_t* corr /* [2][nbins] */);
int kmc_host_bond_order(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t mode, int32_t fold,
                        double r_cut, int32_t select, int32_t nbins, int64_t* hist, kmc_bond_order_out* out,
                        int64_t* C, int64_t* S, int32_t* nn);
int kmc_host_bond_order_corr(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t mode,
                             int32_t fold, double r_cut, int32_t select, double r_max, int32_t nbins,
                             int64_t* corr);

/* Ring statistics and valency census of the ligand network:
 * the graph the bonds draw — its ligand – receptor = receptor – ligand bridges,
 * how many of a ligand's sites are occupied and continue to another ligand,
 * and its closed rings by length, hexagons among them.  Like the other
 * analyses the calls read the CURRENT state on the device (valid straight
 * after kmc_set_state / kmc_load_*), launch nothing inside kmc_step, leave the
 * state, the step counter, the recorders, kmc_get_clusters' validity and the
 * other analyses' scratch untouched and are timed by kmc_analysis_ms; their
 * scratch is their own (allocated by the first call, freed by kmc_destroy).
 *
 * Definitions — the device, kmc_host_network / kmc_host_rings and the tests
 * share them; integers only, no position is read:
 *   hop             from ligand b (reference index) by site s in {2, 3, 4},
 *                   a zero link at any stage meaning no bridge:
 *                     r  = res_nei[b][s]    the receptor on the site,
 *                     r' = res_nei[r][3]    its cis partner,
 *                     l  = res_nei[r'][2]   the partner's ligand (0: r' holds
 *                                           none — a HALF BRIDGE),
 *                     s' = res_nei[r'][4]   the site of l it sits on;
 *                   the hop returns (l, s').
 *   consistency     every bond is checked from its other side: r is 0 or a
 *                   receptor with res_nei[r][2] = b and res_nei[r][4] = s; r'
 *                   is 0 or another receptor with res_nei[r'][3] = r; l is 0
 *                   or a ligand with s' in 2..4 and res_nei[l][s'] = r'.  Then
 *                   the hop from (l, s') returns (b, s).  Likewise a
 *                   receptor's nei2 is 0 or a ligand and its nei3 0 or
 *                   another receptor whose nei3 points back.  Anything else —
 *                   a link of the wrong kind, an asymmetric bridge — is
 *                   KMC_ERR_STATE; nothing is read through a bad link.
 *   bridge          the unordered pair {(b, s), (l, s')} of a hop with l != 0.
 *                   l = b is a LOOP (then s' != s).
 *   ligand graph G  a multigraph: the ligands are its vertices, the bridges
 *                   its edges; a loop adds 2 to its ligand's degree, so every
 *                   degree is at most 3.
 *   ring of length L  L distinct ligands v_0 .. v_{L-1} and L distinct bridges
 *                   e_i, e_i joining v_i and v_{(i+1) mod L}.  L = 1 is a loop,
 *                   L = 2 two distinct bridges between the same two ligands.
 *                   Two descriptions are the same ring iff their bridge sets
 *                   are equal: parallel bridges give distinct rings.
 *   chordless ring  no bridge outside the ring has both its ends at ligands of
 *                   the ring.  (A ring's ligand uses two sites on the ring: it
 *                   has at most one bridge off the ring and cannot carry a
 *                   loop.)  The rule holds for every L: a double bridge beside
 *                   a third parallel bridge is not chordless.
 *   valency census  rec[(nei2 != 0) + 2 (nei3 != 0)] counts the receptors;
 *                   lig_hist[occupied sites][bridge ends] the ligands (a
 *                   ligand's bridge ends: its sites whose hop has l != 0).
 *   counters        n_bridges (a loop counts once), n_loops, n_half (receptors
 *                   with a ligand whose cis partner has none), n_free_dimers
 *                   (cis pairs with no ligand on either side), n_vertices
 *                   (ligands with >= 1 bridge end), n_net_components
 *                   (kmc_components labels that hold >= 1 bridge), cycle_rank
 *                   = n_bridges - n_vertices + n_net_components.
 *   kmc_network     out: the counters and rec; lig_hist[4][4]; adj_lig[n_b][3]
 *                   and adj_site[n_b][3] by the ligand's reference index and
 *                   site - 2: the hop's l as a 1-based ligand number (1..n_b,
 *                   0: none) and s' (0: none).  Every array may be NULL.
 *   kmc_rings       1 <= max_len <= KMC_RING_MAX.  counts[2][KMC_RING_MAX + 1]:
 *                   row 0 the rings of each length, row 1 the chordless ones;
 *                   index 0 and the entries above max_len are zero.  member[2]
 *                   [n_b] (uint32, by the ligand's reference index; may be
 *                   NULL): bit L is set iff the ligand lies on at least one
 *                   such ring of length L.  out (may be NULL) as kmc_network's.
 *                   Each ring is counted once; the counts do not depend on the
 *                   order of the proteins.  A call follows at most 3 *
 *                   2^(max_len - 1) hops per ligand.
 * kmc_host_network / kmc_host_rings: the same from a host state view,
 * sequentially, no device.
 * KMC_ERR_ARG for a null / out-of-range argument, a handle without state and a
 * decomposed window; KMC_ERR_STATE as above; every loop is bounded, so a bad
 * link ends the call and cannot hang. */
#define KMC_RING_MAX 12
typedef struct kmc_net_out {
  int64_t n_bridges, n_loops, n_half, n_free_dimers, n_vertices, n_net_components, cycle_rank;
  int64_t rec[4];
} kmc_net_out;
int kmc_network(kmc_sim* s, kmc_net_out* out, int64_t* lig_hist /* [4][4] */, int32_t* adj_lig /* [n_b][3] */,
                int32_t* adj_site /* [n_b][3] */);
int kmc_rings(kmc_sim* s, int32_t max_len, int64_t* counts /* [2][KMC_RING_MAX + 1] */,
              uint32_t* member /* [2][n_b] */, kmc_net_out* out);
/* Adjacency rows the last successful kmc_rings call gathered along its paths (its hops; 0 before the first): the
 * work the call did, for a rate beside kmc_analysis_ms.  Unlike the counts it depends on the order of the slots. */
int64_t kmc_rings_hops(const kmc_sim* s);
int kmc_host_network(const kmc_params* p, const kmc_state_view* v, kmc_net_out* out, int64_t* lig_hist,
                     int32_t* adj_lig, int32_t* adj_site);
int kmc_host_rings(const kmc_params* p, const kmc_state_view* v, int32_t max_len, int64_t* counts, uint32_t* member,
                   kmc_net_out* out);

/* Multi-origin lag correlator: the mean-squared displacement,
 * the non-Gaussian parameter and the self-intermediate scattering function by
 * lag time, averaged over every time origin the run offers.  Where the tracker
 * (§11) relates every sample to the one origin of kmc_track_begin, this
 * recorder keeps rings of origins at log-spaced strides (a multiple-tau, or
 * order-n, correlator) and correlates the current positions with each stored
 * origin at every update.  Like the tracker it reads the CURRENT state,
 * launches nothing inside kmc_step and leaves the state, the step counter and
 * kmc_get_clusters' validity untouched; its arrays are indexed by reference
 * index i = 0..N-1 (receptors first), a protein's position is (x, y) of its
 * bead [1][1].  It is independent of the tracker: both may run on one handle.
 * All results are integers: the device, kmc_host_lag_* and the tests agree by
 * equality, no order of summation exists, and the tables of replicas (and of
 * consecutive recorders) add.
 *
 * Definitions — the device, kmc_host_lag_* and the tests share them:
 *   integer coords  X = (int64) round(x * 1024.0), BX = (int64) round(box_x *
 *                   1024.0); the same in y (§12's 2^-10 A).  KMC_ERR_ARG when
 *                   BX < 1 or BY < 1.
 *   minimum image   of a difference d with box B: m = d mod B (floor modulus),
 *                   m -= B when 2 m >= B — the folding of the structure
 *                   factor's axis phase.
 *   configuration   (kmc_lag_config) every >= 1 steps between updates; levels
 *                   L in 1..KMC_LAG_MAX_LEVELS; slots P even in
 *                   2..KMC_LAG_MAX_SLOTS; max_jump in A, <= 0 meaning min(box)
 *                   / 4, else at most min(box) / 2 (as §11's); max_disp in A,
 *                   <= 0 meaning 16384, else at most 16384; nq in
 *                   0..KMC_LAG_MAX_Q multipliers h[k] in 1..64.  J = (int64)
 *                   round(max_jump * 1024.0), F = (int64) round(max_disp *
 *                   1024.0) <= 2^24.
 *   per protein     prev = (X, Y) at the last update; the unwrapped U (int64
 *                   x 2); the three links as the tracker names them (receptor:
 *                   nei2 as reference index + 1, nei4, nei3 as reference index
 *                   + 1; ligand: nei2..4 as reference index + 1) as of the
 *                   last update; last_event (int32).
 *   kmc_lag_begin   is update n = 0: U = prev = (X, Y), the links are the
 *                   current ones, last_event = 0, and U is stored as the origin
 *                   of update 0 in slot 0 of every level.  The table is zeroed.
 *                   The rings — levels * slots * 16 bytes per protein — and the
 *                   rest are allocated here and freed by kmc_lag_end /
 *                   kmc_destroy; a failed allocation is KMC_ERR_HIP with the
 *                   recorder off.
 *   kmc_lag_update  n >= 1, legal only when kmc_current_step() == the step of
 *                   the last update + every (else KMC_ERR_ARG, nothing
 *                   changes).  Per protein:
 *                     1. d = minimum image of (X - prev.X); the same in y;
 *                     2. U += d; prev = (X, Y);
 *                     3. last_event = n when |dx| >= J or |dy| >= J or any of
 *                        the three links differs from the stored ones; the
 *                        stored links become the current ones;
 *                     4. the class is that of the CURRENT state, §11's five:
 *                        0 receptor without a link, 1 receptor with only a cis
 *                        partner, 2 receptor with a ligand, 3 ligand without a
 *                        link, 4 ligand with a link.
 *                   Level l (0 <= l < L) fires when n mod 2^l == 0.  With t =
 *                   n >> l it correlates with the origin of update n - j 2^l,
 *                   which sits in slot (t - j) mod P, for every j in J(l) with
 *                   j <= t: J(0) = 1..P, J(l >= 1) = P/2 + 1..P (the smaller j
 *                   of a higher level repeat lags the level below holds).
 *                   Afterwards the level stores U in slot t mod P.
 *   rows            pair (l, j) has row j - 1 at level 0 and P + (l - 1) P/2 +
 *                   (j - P/2 - 1) above; rows = P + (L - 1) P/2 <=
 *                   KMC_LAG_MAX_ROWS; its lag is j 2^l updates.
 *   pair term       of protein i against the origin U_k stored at update n_k:
 *                   Dx = U.x - U_k.x, Dy = U.y - U_k.y.  FAR when |Dx| >= F or
 *                   |Dy| >= F: the pair counts in n_far[row][class] and nowhere
 *                   else.  Otherwise q = Dx^2 + Dy^2 (< 2^49, in units of 2^-20
 *                   A^2), and the pair is CLEAN when last_event[i] <= n_k:
 *                   neither a jump nor a change of links was seen at an update
 *                   after the origin was stored, so a clean pair's class is its
 *                   class at the origin too.  Per (row, class): n_all += 1,
 *                   m2_all += q; for a clean pair n_clean += 1, m2_clean += q,
 *                   m4_clean += q^2, and for each k < nq
 *                     fs[k] += (int64) round(cos_x * 2^30) + (int64) round(
 *                              cos_y * 2^30),
 *                   cos_x the cosine of the structure factor's axis phase 2 pi
 *                   ((h[k] Dx) mod BX folded into [-BX/2, BX/2)) / BX in double
 *                   (the library's cos), cos_y the same of (h[k], Dy, BY).
 *                   n_pairs[row] counts the (origin, update) pairs filed.
 *                   The F bound keeps every kmc_i128 from overflowing below
 *                   2^29 terms at the bound (q^2 < 2^98); overflow is not
 *                   checked.
 *                   CAVEAT: a bond that opens and closes again with the same
 *                   partner between two updates is not seen, as in §11.
 *   kmc_lag_sample  copies the table [rows][KMC_LAG_CLASSES] and n_pairs[rows]
 *                   (either may be NULL) out, with the configuration in effect,
 *                   J, F, BX, BY, rows, origin_step, last_step and n_updates.
 *                   The table accumulates from begin until end.
 *   kmc_lag_arrays  U [N][2] and last_event [N] (either may be NULL) by
 *                   reference index: diagnostics and tests.
 *   kmc_lag_end     drops the recorder and frees its memory; idempotent.
 * kmc_analysis_ms covers the last call.  The recorder is not checkpointed.
 * kmc_host_lag_*: the same from host state views, sequentially, no device; the
 * caller owns the arrays of the kmc_lag_view (ring [L][P][N][2], table [rows]
 * [5], n_pairs [rows]) and the kmc_lag_out that carries the recorder between
 * the calls.
 * KMC_ERR_ARG for a null / out-of-range argument (odd slots, a NaN or too large
 * max_jump / max_disp, h out of range), a handle without state, a decomposed
 * window, an update off the stride and a recorder that was not begun;
 * kmc_set_state, kmc_load_*, kmc_init_random and kmc_dd_set_state drop the
 * recorder. */
#define KMC_LAG_MAX_LEVELS 20
#define KMC_LAG_MAX_SLOTS 16
#define KMC_LAG_MAX_Q 4
#define KMC_LAG_CLASSES 5
#define KMC_LAG_MAX_ROWS 168
typedef struct kmc_lag_config {
  int32_t every, levels, slots, nq;
  double max_jump, max_disp;
  int32_t h[KMC_LAG_MAX_Q];
} kmc_lag_config;
typedef struct kmc_lag_info {
  int64_t n_updates; /* n of this update */
  int64_t n_tasks;   /* (level, j) pairs it filed */
  int64_t n_events;  /* proteins with last_event = n */
} kmc_lag_info;
typedef struct kmc_lag_cell {
  int64_t n_all, n_clean, n_far;
  kmc_i128 m2_all, m2_clean, m4_clean, fs[KMC_LAG_MAX_Q];
} kmc_lag_cell;
typedef struct kmc_lag_out {
  kmc_lag_config cfg; /* as in effect: max_jump and max_disp resolved */
  int64_t J, F, BX, BY;
  int64_t origin_step, last_step, n_updates;
  int64_t rows;
} kmc_lag_out;
typedef struct kmc_lag_view {
  int64_t* prev;        /* [N][2] */
  int64_t* U;           /* [N][2] */
  int32_t* links;       /* [3][N] */
  int32_t* last_event;  /* [N] */
  int64_t* ring;        /* [levels][slots][N][2] */
  kmc_lag_cell* table;  /* [rows][KMC_LAG_CLASSES] */
  int64_t* n_pairs;     /* [rows] */
} kmc_lag_view;
int kmc_lag_begin(kmc_sim* s, const kmc_lag_config* cfg);
int kmc_lag_update(kmc_sim* s, kmc_lag_info* info);
int kmc_lag_sample(kmc_sim* s, kmc_lag_out* out, kmc_lag_cell* table /* [rows][5] */, int64_t* n_pairs /* [rows] */);
int kmc_lag_arrays(kmc_sim* s, int64_t* U /* [N][2] */, int32_t* last_event /* [N] */);
int kmc_lag_end(kmc_sim* s);
int kmc_host_lag_begin(const kmc_params* p, const kmc_state_view* v, const kmc_lag_config* cfg,
                       const kmc_lag_view* view, kmc_lag_out* acc);
int kmc_host_lag_update(const kmc_params* p, const kmc_state_view* v, const kmc_lag_view* view, kmc_lag_out* acc,
                        kmc_lag_info* info);
int kmc_host_lag_sample(const kmc_params* p, const kmc_lag_view* view, const kmc_lag_out* acc, kmc_lag_out* out,
                        kmc_lag_cell* table, int64_t* n_pairs);

/* Orientation layer: the rotational counterpart of the lag
 * correlator, and a one-shot census of the ligands' poses.  Every layer above
 * reads one point per protein; this one reads the rigid bodies' own vectors.
 * kmc_rot_* keeps rings of packed body vectors on §18's multiple-tau schedule
 * and correlates the current vectors with each stored origin that is due: per
 * lag, class and vector the counts and the exact sums of d = u(t) . u(0) and of
 * d^2, from which C_1 and C_2 follow.  It reads the CURRENT state, launches
 * nothing inside kmc_step and leaves the state, the step counter and
 * kmc_get_clusters' validity untouched; it is independent of the tracker and
 * of the lag correlator.  All results are integers: the device, kmc_host_rot_*
 * and the tests agree by equality, and the tables of replicas (and of
 * consecutive recorders) add.
 *
 * Definitions — the device, the host counterparts and the tests share them:
 *   quantisation    q(x) = (int64) round(x * 1024.0) per bead coordinate; a
 *                   vector is the difference of two quantised beads.
 *   receptor        heading H = (q[3][2] - q[3][1]) in x and y, z = 0 by
 *                   definition: the xy projection (receptors stay vertical).
 *   ligand          axis N = q[1][2] - q[1][1] (v = 0), arm A = q[2][1] -
 *                   q[1][1] (v = 1), and C = q[3][1] - q[1][1]; the handedness
 *                   chi = sign(N . (A x C)), an exact integer below 2^51.
 *   bad             a protein with a component of H (or of N, A, C) of
 *                   magnitude >= 2^16 quanta.  No valid state has one
 *                   (ra_radius <= 20, rb_radius <= 30: the longest vector is the
 *                   arm, 2 * 30 / sqrt 3 A = 35 473 quanta).  Its packed words
 *                   are KMC_ROT_BAD, its chi is 0, it counts in n_bad and files
 *                   no pair; a pair with a bad origin is not filed either.
 *   packing         x, y, z as three signed 21-bit fields of one 64-bit word
 *                   (x lowest); bit 63 is clear.  vec holds the current words:
 *                   [n_a] headings, then [n_b] axes, then [n_b] arms; a ring
 *                   entry is one such array, 8 n_a + 16 n_b bytes.
 *   configuration   (kmc_rot_config) every >= 1; levels in 1..
 *                   KMC_LAG_MAX_LEVELS; slots even in 2..KMC_LAG_MAX_SLOTS.
 *   schedule, rows  kmc_lag_update's: levels, slots, tasks and rows alike.
 *   kmc_rot_begin   is update n = 0: the current words are stored as the origin
 *                   of update 0 in slot 0 of every level; the links and chi are
 *                   the current ones, last_event = 0, the table is zeroed.
 *   kmc_rot_update  n >= 1, legal `every` steps after the last update.  Per
 *                   protein: an EVENT is a change of any of its three links (as
 *                   the tracker names them) since the last update or, for a
 *                   ligand, a chi that differs from the last update's (a FLIP:
 *                   the mirror reflection at z = 0 and z = box_z is no
 *                   rotation); last_event = n then.  The class is the lag
 *                   correlator's, of the CURRENT state.  A pair of protein i
 *                   with the origin stored at update n_k is CLEAN when
 *                   last_event[i] <= n_k.  There is no jump test and no minimum
 *                   image: a rigid body is wrapped as a whole.  Per (row,
 *                   class, v) with d = u_v(n) . u_v(n_k), |d| < 3 2^32:
 *                   n_all += 1, s1_all += d; for a clean pair n_clean += 1,
 *                   s1_clean += d, s2_clean += d^2 (< 2^68).  n_pairs[row]
 *                   counts the (origin, update) pairs filed.  Afterwards every
 *                   level that fired stores the current words.  info: n of this
 *                   update, its tasks, the proteins with an event, the flips
 *                   and the bad proteins of this update.
 *   kmc_rot_sample  copies the table [rows][KMC_LAG_CLASSES][KMC_ROT_VECS]
 *                   (v = 1 of the receptor classes stays zero) and n_pairs
 *                   [rows] (either may be NULL) out.
 *   kmc_rot_arrays  vec [n_a + 2 n_b], last_event [N] and chi [N] (0 for a
 *                   receptor; each may be NULL) by reference index.
 *   kmc_rot_end     drops the recorder and frees its memory; idempotent.
 *   kmc_ligand_pose one-shot, no recorder: for every ligand that is not bad one
 *                   count in hist[k][z bin][tilt bin] (hist [4][nz][nc], zeroed
 *                   by the call; may be NULL), k = its occupied sites 0..3 (the
 *                   links in range).  With BZ = q(box_z), Lq = q(rb_radius), Z
 *                   = q(z of [1][1]): z bin = 0 for Z <= 0, nz - 1 for Z >= BZ,
 *                   else min(nz - 1, Z nz / BZ); tilt bin = (N_z + Lq) nc /
 *                   (2 Lq + 1) clamped to [0, nc - 1] (a laid-down ligand, N_z
 *                   = Lq, lies in the top bin).  out: the ligands of chi = +1
 *                   and chi = -1 per k, and n_bad.  1 <= nz, nc <=
 *                   KMC_POSE_MAX_BINS.
 * kmc_analysis_ms covers the last call.  The recorder is not checkpointed.
 * kmc_host_rot_* / kmc_host_ligand_pose: the same from host state views,
 * sequentially, no device; the caller owns the arrays of the kmc_rot_view.
 * KMC_ERR_ARG for a null / out-of-range argument, a handle without state, a
 * decomposed window, an update off the stride and a recorder that was not
 * begun; a new state drops the recorder. */
#define KMC_ROT_VECS 2
#define KMC_ROT_BAD 0x8000000000000000ull
#define KMC_POSE_MAX_BINS 64
#define KMC_POSE_CLASSES 4
typedef struct kmc_rot_config {
  int32_t every, levels, slots;
} kmc_rot_config;
typedef struct kmc_rot_info {
  int64_t n_updates; /* n of this update */
  int64_t n_tasks;   /* (level, j) pairs it filed */
  int64_t n_events;  /* proteins with last_event = n */
  int64_t n_flips;   /* ligands whose chi changed */
  int64_t n_bad;     /* bad proteins of this update */
} kmc_rot_info;
typedef struct kmc_rot_cell {
  int64_t n_all, n_clean;
  kmc_i128 s1_all, s1_clean, s2_clean;
} kmc_rot_cell;
typedef struct kmc_rot_out {
  kmc_rot_config cfg;
  int32_t pad_;
  int64_t origin_step, last_step, n_updates;
  int64_t rows;
} kmc_rot_out;
typedef struct kmc_rot_view {
  uint64_t* vec;        /* [n_a + 2 n_b] */
  int32_t* links;       /* [3][N] */
  int32_t* last_event;  /* [N] */
  int8_t* chi;          /* [N] */
  uint64_t* ring;       /* [levels][slots][n_a + 2 n_b] */
  kmc_rot_cell* table;  /* [rows][KMC_LAG_CLASSES][KMC_ROT_VECS] */
  int64_t* n_pairs;     /* [rows] */
} kmc_rot_view;
typedef struct kmc_pose_out {
  int64_t chi_pos[KMC_POSE_CLASSES], chi_neg[KMC_POSE_CLASSES];
  int64_t n_bad;
} kmc_pose_out;
int kmc_rot_begin(kmc_sim* s, const kmc_rot_config* cfg);
int kmc_rot_update(kmc_sim* s, kmc_rot_info* info);
int kmc_rot_sample(kmc_sim* s, kmc_rot_out* out, kmc_rot_cell* table /* [rows][5][2] */, int64_t* n_pairs /* [rows] */);
int kmc_rot_arrays(kmc_sim* s, uint64_t* vec /* [n_a + 2 n_b] */, int32_t* last_event /* [N] */, int8_t* chi /* [N] */);
int kmc_rot_end(kmc_sim* s);
int kmc_ligand_pose(kmc_sim* s, int32_t nz, int32_t nc, int64_t* hist /* [4][nz][nc] */, kmc_pose_out* out);
int kmc_host_rot_begin(const kmc_params* p, const kmc_state_view* v, const kmc_rot_config* cfg,
                       const kmc_rot_view* view, kmc_rot_out* acc);
int kmc_host_rot_update(const kmc_params* p, const kmc_state_view* v, const kmc_rot_view* view, kmc_rot_out* acc,
                        kmc_rot_info* info);
int kmc_host_rot_sample(const kmc_params* p, const kmc_rot_view* view, const kmc_rot_out* acc, kmc_rot_out* out,
                        kmc_rot_cell* table, int64_t* n_pairs);
int kmc_host_ligand_pose(const kmc_params* p, const kmc_state_view* v, int32_t nz, int32_t nc, int64_t* hist,
                         kmc_pose_out* out);

/* Pair dynamics: the two-body half of the dynamic set.  Part A
 * is the van Hove function split into its distinct part G_d(r, t) — the
 * density of OTHER proteins at distance r, now, from where a protein was at
 * the origin — and its (folded) self part; part B is the spatial correlation of
 * displacements C_u(r, t) = <u_i . u_j> over pairs that were r apart at the
 * origin.  One origin, that of kmc_pd_begin.  Like the lag correlator it reads
 * the CURRENT state, launches nothing inside kmc_step and leaves the state,
 * the step counter and kmc_get_clusters' validity untouched; its arrays are
 * indexed by reference index i = 0..N-1 (receptors first), a protein's
 * position is (x, y) of its bead [1][1].  All results are integers: the
 * device, kmc_host_pd_* and the tests agree by equality, and the tables of
 * replicas (and of consecutive recorders sampled at the same lag) add.
 *
 * Definitions — the device, kmc_host_pd_* and the tests share them:
 *   integer coords  kmc_lag_*'s: X = (int64) round(x * 1024.0), BX = (int64)
 *                   round(box_x * 1024.0), the same in y; its minimum image;
 *                   fold(X) = X mod BX, the floor modulus into [0, BX).
 *                   KMC_ERR_ARG when BX < 1, BY < 1 or a box of 2^21 A or more.
 *   configuration   (kmc_pd_config) every >= 1 steps between updates; nbins in
 *                   1..KMC_PD_MAX_BINS; r_max > 0; max_jump and max_disp as
 *                   kmc_lag_config's (<= 0: min(box) / 4 and 16384 A), J and F
 *                   their integers, F <= 2^24.
 *   bins            E[m] = (int64) round(m * (r_max / nbins) * 1024.0), m =
 *                   0..nbins, strictly increasing (else KMC_ERR_ARG).  A pair
 *                   with d2 = dx^2 + dy^2 (integers) is in bin k = #{m in
 *                   1..nbins : E[m]^2 <= d2} and is counted when k < nbins.  No
 *                   square root decides a bin.
 *   search grid     ncx = floor(BX / E[nbins]), ncy alike, both >= 3 (else
 *                   KMC_ERR_ARG), both capped at 2048; cell = floor(fold(X) *
 *                   ncx / BX).  No result depends on it.
 *   per protein     X0 = (X, Y) at kmc_pd_begin; prev, the unwrapped U and the
 *                   step d = minimum image of (X - prev), U += d, prev = X of
 *                   kmc_lag_update; flags |= KMC_PD_JUMPED (sticky) when |dx| >=
 *                   J or |dy| >= J at an update; u = U - X0.  VALID: not jumped
 *                   and |u.x| < F and |u.y| < F.  Links are not read.
 *   kmc_pd_begin    is update 0: prev = U = X0 = (X, Y), flags = 0; the origin
 *                   is binned once.  The scratch (109 bytes per protein and 12
 *                   per cell) is allocated here and freed by kmc_pd_end /
 *                   kmc_destroy; a failed allocation is KMC_ERR_HIP with the
 *                   recorder off.
 *   kmc_pd_update   the per-protein step, legal only when kmc_current_step() ==
 *                   the step of the last update + every (else KMC_ERR_ARG,
 *                   nothing changes).
 *   kmc_pd_sample   the tables of the state as of the last update (species 0 =
 *                   receptor, 1 = ligand):
 *                   A. D = minimum image of (fold(U_j) - fold(X0_i)) per axis,
 *                      d2 binned.  gd[2 species(i) + species(j)][k] counts every
 *                      ORDERED pair i != j, gs[species(i)][k] counts i == j:
 *                      the folded self part, the bin of the true displacement
 *                      while |u| < box / 2.  No validity filter: a teleported
 *                      protein is still where it is.
 *                   B. over UNORDERED pairs i < j, D = minimum image of (X0_j -
 *                      X0_i), d2 binned; kind 0 = AA, 1 = AB, 2 = BB.  Per (kind,
 *                      k) a kmc_pd_cell: n_pairs (every pair), n_valid (both
 *                      proteins valid), and over the valid pairs dot += u_i.x
 *                      u_j.x + u_i.y u_j.y (|term| < 2^49) and sq += |u_i|^2 +
 *                      |u_j|^2 (term < 2^50).  C_u = 2 dot / sq is 1 for rigid
 *                      co-translation.
 *                   Each call computes the tables anew (nothing accumulates);
 *                   gd [4][nbins], gs [2][nbins], cu [3][nbins] may each be NULL,
 *                   and with all three NULL only out is filled.
 *   kmc_pd_arrays   U [N][2], X0 [N][2] and flags [N] (each may be NULL) by
 *                   reference index: diagnostics and tests.
 *   kmc_pd_end      drops the recorder and frees its memory; idempotent.
 * kmc_analysis_ms covers the last call.  The recorder is not checkpointed.
 * kmc_host_pd_*: the same from host state views, sequentially, no device, with
 * a cell list of their own; the caller owns the arrays of the kmc_pd_view and
 * the kmc_pd_out that carries the recorder between the calls.
 * KMC_ERR_ARG for a null / out-of-range argument, a handle without state, a
 * decomposed window, an update off the stride and a recorder that was not
 * begun; kmc_set_state, kmc_load_*, kmc_init_random and kmc_dd_set_state drop
 * the recorder. */
#define KMC_PD_MAX_BINS 256
#define KMC_PD_JUMPED 1
typedef struct kmc_pd_config {
  int32_t every, nbins;
  double r_max, max_jump, max_disp;
} kmc_pd_config;
typedef struct kmc_pd_info {
  int64_t n_updates; /* n of this update */
  int64_t n_jumped;  /* proteins whose flags hold KMC_PD_JUMPED after it */
} kmc_pd_info;
typedef struct kmc_pd_cell {
  int64_t n_pairs, n_valid;
  kmc_i128 dot, sq;
} kmc_pd_cell;
typedef struct kmc_pd_out {
  kmc_pd_config cfg; /* as in effect: max_jump and max_disp resolved */
  int64_t J, F, BX, BY;
  int64_t ncx, ncy;
  int64_t origin_step, last_step, n_updates;
} kmc_pd_out;
typedef struct kmc_pd_view {
  int64_t* prev;  /* [N][2] */
  int64_t* U;     /* [N][2] */
  int64_t* X0;    /* [N][2] */
  uint8_t* flags; /* [N] */
} kmc_pd_view;
int kmc_pd_begin(kmc_sim* s, const kmc_pd_config* cfg);
int kmc_pd_update(kmc_sim* s, kmc_pd_info* info);
int kmc_pd_sample(kmc_sim* s, kmc_pd_out* out, int64_t* gd /* [4][nbins] */, int64_t* gs /* [2][nbins] */,
                  kmc_pd_cell* cu /* [3][nbins] */);
int kmc_pd_arrays(kmc_sim* s, int64_t* U /* [N][2] */, int64_t* X0 /* [N][2] */, uint8_t* flags /* [N] */);
int kmc_pd_end(kmc_sim* s);
int kmc_host_pd_begin(const kmc_params* p, const kmc_state_view* v, const kmc_pd_config* cfg, const kmc_pd_view* view,
                      kmc_pd_out* acc);
int kmc_host_pd_update(const kmc_params* p, const kmc_state_view* v, const kmc_pd_view* view, kmc_pd_out* acc,
                       kmc_pd_info* info);
int kmc_host_pd_sample(const kmc_params* p, const kmc_pd_view* view, const kmc_pd_out* acc, kmc_pd_out* out,
                       int64_t* gd, int64_t* gs, kmc_pd_cell* cu);

/* Body dynamics: how a cluster of s proteins moves and how long
 * it keeps its identity, against the one origin of kmc_bd_begin.  A BODY is a
 * connected component of the bond graph at the begin (kmc_components' labels,
 * single proteins included); per body the sample reports the displacement of
 * its centre, its rigid rotation and its fate, filed by (holds a ligand, size).
 * Like the pair dynamics it reads the CURRENT state, launches nothing inside
 * kmc_step and leaves the state, the step counter and kmc_get_clusters'
 * validity untouched; arrays are indexed by reference index.  All results are
 * integers: the device, kmc_host_bd_* and the tests agree by equality, and the
 * tables of replicas (and of recorders sampled at the same lag) add.
 *
 * Definitions — the device, kmc_host_bd_* and the tests share them:
 *   integer coords  kmc_lag_*'s, with its minimum image, J and F (max_jump <= 0:
 *                   min(box) / 4, else at most min(box) / 2; max_disp <= 0:
 *                   16384 A, else at most 16384 A, so F <= 2^24).  KMC_ERR_ARG
 *                   for a box of 2^21 A or more.
 *   configuration   (kmc_bd_config) every >= 1; 2 <= max_size <= KMC_BD_MAX_SIZE.
 *   bodies          static for the recorder's life: the label (the smallest
 *                   reference index r, the ROOT), n_r, n_l, n = n_r + n_l, hl =
 *                   (n_l > 0), the spanning bits of kmc_unwrap, and per member
 *                   D0_i = X0_i + shift_i * B - X0_r with kmc_unwrap's image
 *                   shifts (zero in a spanning body, as it reports them).  WIDE
 *                   (KMC_BD_WIDE in the body's bits) when some |D0| component is
 *                   >= 2^24.
 *   per protein     prev, U, X0 (= U at the begin) and the three links as
 *                   kmc_lag_* stores them; flags, sticky: KMC_BD_JUMPED when
 *                   |d| >= J on an axis at an update, KMC_BD_CHANGED when a link
 *                   differed from the stored one at an update (the stored links
 *                   then become the current ones); u = U - X0.
 *   kmc_bd_begin    is update 0.  The scratch (189 bytes per protein) is
 *                   allocated here and freed by kmc_bd_end / kmc_destroy; a
 *                   failed allocation is KMC_ERR_HIP with the recorder off.
 *   kmc_bd_update   legal only when kmc_current_step() == the step of the last
 *                   update + every (else KMC_ERR_ARG, nothing changes).
 *   kmc_bd_sample   legal only at the step of the last update (else
 *                   KMC_ERR_ARG), so that the flags and the current components
 *                   describe one state.  With L_i the current kmc_components
 *                   label, a body is
 *                     BROKEN   its members carry more than one L;
 *                     INTACT   one L, and that component has n members now (the
 *                              membership is then the same);
 *                     GROWN    one L, and that component is larger;
 *                     PRISTINE no member has a flag (on a trajectory this
 *                              implies INTACT);
 *                     VALID    PRISTINE and |u| < F on both axes for every member.
 *                   Translation of a VALID body: Su = sum of u_i (n times the
 *                   displacement of its centre), T = Su.x^2 + Su.y^2 < 2^111.
 *                   Rotation of a VALID body with 2 <= n <= KMC_BD_ROT_MAX, no
 *                   spanning bit and not WIDE (every other VALID body of n >= 2
 *                   counts in n_rot_skipped): D_i = D0_i + u_i - u_r,
 *                     C = sum D0_i . D_i,  S = sum (D0x_i Dy_i - D0y_i Dx_i),
 *                   int64, |.| < 2^61 (|D0| < 2^24, |D| < 2^26: a term is below
 *                   2^51, at most 1023 of them).  C = S = 0 counts in n_rot_null;
 *                   otherwise phi = atan2((double) S, (double) C) in (-pi, pi]
 *                   and c1 = (int64) round_(cos(phi) 2^30), c2 = (int64)
 *                   round_(cos(2 phi) 2^30), p = (int64) round_(phi 2^24), p^2
 *                   summed (kmc_math.h's atan2, cos and round_).
 *   table           [2][max_size + 1] kmc_bd_cell by hl and k = min(n,
 *                   max_size); row 0 stays zero, the last row is the overflow
 *                   row.  n_bodies and sum_size are static; n_intact + n_grown +
 *                   n_broken = n_bodies; m2 = sum of T over VALID bodies.  Each
 *                   call computes the table anew; table may be NULL.
 *   kmc_bd_bodies   one kmc_bd_body per body of at least min_size >= 1 members,
 *                   sorted by label, kmc_cluster_list's capacity rule.  su is
 *                   zero unless VALID, C and S unless the rot bit is set;
 *                   cur_label is the smallest current label among the members,
 *                   cur_size that component's size.
 *   kmc_bd_arrays   U [N][2], X0 [N][2], flags [N], label [N] (1-based), D0
 *                   [N][2]; each may be NULL.
 *   kmc_bd_get      copies the per-protein state out: prev, U, links and flags
 *                   are needed, X0, label, D0 and bits are filled when given.
 *   kmc_bd_put      loads prev, U, links and flags into a recorder that was
 *                   begun on the current state and sets the step of the last
 *                   update to last_step <= kmc_current_step().  The bodies, X0
 *                   and D0 stay those of the begin.  A recorder's per-protein
 *                   state can be carried across a saved state this way, and a
 *                   test can set U and the flags by hand under a hand-built graph.
 *   kmc_bd_end      drops the recorder and frees its memory; idempotent.
 * kmc_analysis_ms covers the last call.  kmc_host_bd_*: the same from host
 * state views, sequentially, no device; the caller owns the eight arrays of
 * the kmc_bd_view and the kmc_bd_out that carries the recorder between calls.
 * KMC_ERR_ARG for a null / out-of-range argument, a handle without state, a
 * decomposed window, an update off the stride, a sample off the last update's
 * step and a recorder that was not begun; KMC_ERR_STATE and KMC_ERR_CAPACITY as
 * kmc_unwrap; kmc_set_state, kmc_load_*, kmc_init_random and kmc_dd_set_state
 * drop the recorder. */
#define KMC_BD_MAX_SIZE 255
#define KMC_BD_ROT_MAX 1023
#define KMC_BD_JUMPED 1
#define KMC_BD_CHANGED 2
#define KMC_BD_WIDE 4 /* beside KMC_SPAN_X and KMC_SPAN_Y in a body's bits */
#define KMC_BD_INTACT 0
#define KMC_BD_GROWN 1
#define KMC_BD_BROKEN 2
#define KMC_BD_IS_PRISTINE 1
#define KMC_BD_IS_VALID 2
#define KMC_BD_IS_ROT 4
typedef struct kmc_bd_config {
  int32_t every, max_size;
  double max_jump, max_disp;
} kmc_bd_config;
typedef struct kmc_bd_info {
  int64_t n_updates; /* n of this update */
  int64_t n_jumped;  /* proteins that this update flagged KMC_BD_JUMPED for the first time */
  int64_t n_changed; /* the same for KMC_BD_CHANGED */
} kmc_bd_info;
typedef struct kmc_bd_cell {
  int64_t n_bodies, sum_size, n_pristine, n_intact, n_grown, n_broken, n_valid, n_rot, n_rot_null, n_rot_skipped, c1, c2;
  kmc_i128 m2, phi2;
} kmc_bd_cell;
typedef struct kmc_bd_out {
  kmc_bd_config cfg; /* as in effect: max_jump and max_disp resolved */
  int64_t J, F, BX, BY;
  int64_t origin_step, last_step, n_updates;
  int64_t n_bodies; /* bodies of the origin, single proteins included */
} kmc_bd_out;
typedef struct kmc_bd_body {
  int32_t label, n_r, n_l;
  int32_t bits;   /* KMC_SPAN_X | KMC_SPAN_Y | KMC_BD_WIDE */
  int32_t status; /* KMC_BD_INTACT / GROWN / BROKEN */
  int32_t is;     /* KMC_BD_IS_PRISTINE | KMC_BD_IS_VALID | KMC_BD_IS_ROT */
  int32_t cur_label, cur_size;
  int64_t su[2], C, S;
} kmc_bd_body;
typedef struct kmc_bd_view {
  int64_t* prev;  /* [N][2] */
  int64_t* U;     /* [N][2] */
  int64_t* X0;    /* [N][2] */
  int32_t* links; /* [3][N] */
  uint8_t* flags; /* [N] */
  int32_t* label; /* [N] 1-based */
  int64_t* D0;    /* [N][2] */
  uint8_t* bits;  /* [N] the bits of the protein's body */
} kmc_bd_view;
int kmc_bd_begin(kmc_sim* s, const kmc_bd_config* cfg);
int kmc_bd_update(kmc_sim* s, kmc_bd_info* info);
int kmc_bd_sample(kmc_sim* s, kmc_bd_out* out, kmc_bd_cell* table /* [2][max_size + 1] */);
/* device milliseconds of the last kmc_bd_sample with a table: the current components, the reduction, the finish
 * (the memset of the table counts with the first) */
int kmc_bd_sample_ms(const kmc_sim* s, double ms[3]);
int kmc_bd_bodies(kmc_sim* s, int32_t min_size, int64_t cap, kmc_bd_body* rows, int64_t* n);
int kmc_bd_arrays(kmc_sim* s, int64_t* U, int64_t* X0, uint8_t* flags, int32_t* label, int64_t* D0);
int kmc_bd_get(kmc_sim* s, const kmc_bd_view* view);
int kmc_bd_put(kmc_sim* s, const kmc_bd_view* view, int64_t last_step);
int kmc_bd_end(kmc_sim* s);
int kmc_host_bd_begin(const kmc_params* p, const kmc_state_view* v, const kmc_bd_config* cfg, const kmc_bd_view* view,
                      kmc_bd_out* acc);
int kmc_host_bd_update(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, kmc_bd_out* acc,
                       kmc_bd_info* info);
int kmc_host_bd_sample(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, const kmc_bd_out* acc,
                       kmc_bd_out* out, kmc_bd_cell* table);
int kmc_host_bd_bodies(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, const kmc_bd_out* acc,
                       int32_t min_size, int64_t cap, kmc_bd_body* rows, int64_t* n);

/* Encounter statistics: what happens BEFORE the association
 * draw.  A bond forms when two sites diffuse into reach, pass the orientation
 * gates and win a draw (main.cpp:1877-2058); this layer evaluates the first two
 * conditions exactly on the committed state — what kmc_get_state returns — and
 * follows every R–L encounter from the update it opens to the one it ends in.
 * Nothing runs inside kmc_step; every output is an integer count, and the
 * device, kmc_host_reach_census / kmc_host_enc_* and the tests agree by
 * equality.
 *
 * Definitions (no minimum image anywhere, as in the engine's gates):
 *   in reach, R–L     the triple (receptor i, ligand b, site k in 2..4) with
 *                     protein_status[i][2] == 0, protein_status[b][k] == 0 and
 *                       d2 = dx*dx + dy*dy + dz*dz < T(bond_dist_cutoff),
 *                     (dx, dy, dz) = R[b][k][2] - R[i][3][2], T(c) the smallest
 *                     double with sqrt(T) >= c (sqrt(d2) < c <=> d2 < T), no
 *                     fused multiply-add.
 *   reactive, R–L     in reach, and |theta_pd| < bond_thetapd_cutoff and
 *                     |theta_ot - 180| < bond_thetaot_cutoff, the two angles
 *                     from the vectors of main.cpp:1889-1911 in gettheta's
 *                     expression order (main.cpp:2329-2366; conv = 180/3.14159).
 *   in reach, cis     the pair i < j of receptors with protein_status[.][3] == 0
 *                     on both and d2 of their [3][3] beads < T(cis_dist_cutoff);
 *                     its kind is MONO when protein_status[.][2] == 0 on both,
 *                     else CX; reactive when |theta_ot - 180| < cis_thetaot_cutoff
 *                     (main.cpp:1966-1981, the lower receptor first).
 *
 * kmc_reach_census (read-only, no recorder), channels KMC_REACH_RL / MONO / CX:
 *   out            n_reach, n_reactive per channel; for R–L the receptors with
 *                  protein_status[.][2] == 0 and the ligand sites with status 0,
 *                  those of them with at least one partner in reach, and the
 *                  largest number of partners of one receptor.
 *   hist_d         [3][2][nd] (may be NULL) in-reach pairs by channel, reactive
 *                  flag and distance bin k = #{m in 1..nd-1 : E2[m] <= d2},
 *                  E2[m] = e*e, e = cutoff*m/nd in double (the channel's cutoff).
 *   hist_a_rl      [na][na] (may be NULL) in-reach R–L triples over
 *                  (|theta_pd|, |theta_ot - 180|); hist_a_cis [2][na] (may be
 *                  NULL) the MONO and the CX pairs over |theta_ot - 180|.  An
 *                  angle x falls into bin min((int)(x * (na / 180.0)), na - 1).
 *   1 <= nd <= KMC_REACH_MAX_ND, 1 <= na <= KMC_REACH_MAX_NA, else KMC_ERR_ARG.
 *
 * The recorder, R–L channel.  Per receptor: the (lig, site) link seen at the
 * last update (lig: the ligand's reference index n_a + b, 0: none) and
 * KMC_ENC_SLOTS slots, each key = b << 2 | (k - 2) (b = 1..n_b; 0: empty),
 * since (the step it opened), nreact (the looks, the opening one included, at
 * which it was reactive) and flags (KMC_ENC_CENSORED: open at begin; GEMINATE;
 * REACTIVE: at the last look; WAS_REACTIVE: at some look).  The slots are
 * sorted by key, the empty ones last.  A receptor's current set is ALL its
 * in-reach triples cut to the KMC_ENC_SLOTS smallest keys — the result does
 * not depend on the order a scan meets the pairs in — and the cut entries add
 * to n_overflow (at begin and at every update).
 *   kmc_enc_begin   cfg->every >= 1.  The current sets become the slots, since
 *                   = the current step, flagged CENSORED; the links are stored.
 *                   A running recorder ends first.  The arrays are allocated
 *                   here and freed by kmc_enc_end / kmc_destroy.
 *   kmc_enc_update  due exactly `every` steps after the last one (KMC_ERR_ARG
 *                   otherwise); a second update at the same step moves only
 *                   n_updates.  At step t, D = t - last_step, per receptor:
 *                   1. exp_reach += D * open slots, exp_reactive += D * slots
 *                      with REACTIVE, exp_free_receptor += D * receptors whose
 *                      link was 0, all as of the last update;
 *                   2. R–L born (the link is non-zero and differs from the
 *                      stored one): if (lig, site) is an open slot,
 *                      on_from_encounter++ and t - since is filed in row BOUND,
 *                      or GEM_REBOUND if the slot is GEMINATE; else on_direct++;
 *                   3. every other open slot that is not in the current set has
 *                      ended: LOST_RECEPTOR if the receptor is bound now, else
 *                      LOST_SITE if protein_status[b][k] != 0 now, else
 *                      SEPARATED; a CENSORED slot files t - since in row
 *                      CENSORED_ENDED, a GEMINATE one in GEM_ESCAPED (separated)
 *                      or GEM_LOST, the others in the row of their outcome;
 *                      each slot that ended in 2. or 3. counts in n_ended and
 *                      files nreact in react_hist[bound ? 0 : 1];
 *                   4. every current triple that is not an open slot opens one
 *                      (n_opened++), since = t, GEMINATE if the stored link is
 *                      this very triple (the bond to it ended at this update);
 *                   5. the slots that continue refresh REACTIVE, and nreact += 1
 *                      when reactive;
 *                   6. the link is stored; occ_reach, occ_reactive,
 *                      occ_free_receptor are counted.
 *                   Every duration and nreact is binned by the kinetics rule
 *                   (KMC_KIN_BINS bins, §15).
 *   kmc_enc_sample  read-only over the recorder as of the last update: out, hist
 *                   (may be NULL) [KMC_ENC_HISTS][KMC_ENC_BINS] — rows 0-7 since
 *                   begin, row 8 (ALIVE) the ages last_step - since of the open
 *                   slots that are not CENSORED (those are counted in
 *                   n_censored_alive) — and react_hist (may be NULL) [2][KMC_ENC_BINS].
 *   kmc_enc_arrays  copies the per-receptor arrays out, by reference index
 *                   (each pointer of the view may be NULL).
 *   kmc_enc_end     drops the recorder and frees its arrays; idempotent.
 *   kmc_enc_phase_ms  device milliseconds of the last census / begin / update:
 *                   binning + the distance walk, the gates, the rest.
 * A new state drops the recorder; a call that fails on the device drops it too;
 * a decomposed window is refused (KMC_ERR_ARG); KMC_ERR_STATE when a slot or a
 * receptor's link leaves its range.  kmc_host_*: the same, sequentially (brute
 * force over all pairs), from host state views, no device: acc carries the
 * counters between the calls, hist10 [10][KMC_ENC_BINS] rows 0-7 and react_hist's
 * two.  KMC_DEBUG_ENC_SLOTS (1..4) lowers the slots kept, on both sides. */
#define KMC_ENC_SLOTS 4
#define KMC_ENC_BINS 256
#define KMC_ENC_HISTS 9
#define KMC_ENC_CENSORED 1
#define KMC_ENC_GEMINATE 2
#define KMC_ENC_REACTIVE 4
#define KMC_ENC_WAS_REACTIVE 8
#define KMC_REACH_RL 0
#define KMC_REACH_MONO 1
#define KMC_REACH_CX 2
#define KMC_REACH_MAX_ND 64
#define KMC_REACH_MAX_NA 36
typedef struct kmc_reach_out {
  int64_t n_reach[3], n_reactive[3]; /* per channel */
  int64_t rl_free_receptors, rl_free_sites, rl_receptors_in_reach, rl_sites_in_reach, rl_max_partners;
} kmc_reach_out;
typedef struct kmc_enc_config {
  int32_t every; /* steps between two updates */
  int32_t reserved;
} kmc_enc_config;
typedef struct kmc_enc_out {
  int64_t origin_step, last_step, n_updates;
  int64_t on_from_encounter, on_direct, n_opened, n_ended; /* since begin */
  int64_t exp_reach, exp_reactive, exp_free_receptor;      /* slot-steps, receptor-steps since begin */
  int64_t n_overflow;                                      /* in-reach triples beyond the slots, summed over the looks */
  int64_t occ_reach, occ_reactive, occ_free_receptor;      /* at the last look */
  int64_t n_censored_alive;                                /* kmc_enc_sample only */
  int64_t every, slots;                                    /* the configuration; the slots kept per receptor */
} kmc_enc_out;
typedef struct kmc_enc_view {
  int32_t *lig, *site; /* [n_a] */
  int32_t* key;        /* [n_a][KMC_ENC_SLOTS] */
  int64_t* since;      /* [n_a][KMC_ENC_SLOTS] */
  int32_t* nreact;     /* [n_a][KMC_ENC_SLOTS] */
  uint8_t* flags;      /* [n_a][KMC_ENC_SLOTS] */
} kmc_enc_view;
int kmc_reach_census(kmc_sim* s, int32_t nd, int32_t na, kmc_reach_out* out, int64_t* hist_d, int64_t* hist_a_rl,
                     int64_t* hist_a_cis);
int kmc_enc_begin(kmc_sim* s, const kmc_enc_config* cfg);
int kmc_enc_update(kmc_sim* s, kmc_enc_out* out);
int kmc_enc_sample(kmc_sim* s, kmc_enc_out* out, int64_t* hist, int64_t* react_hist);
int kmc_enc_arrays(kmc_sim* s, const kmc_enc_view* view);
int kmc_enc_end(kmc_sim* s);
int kmc_enc_phase_ms(const kmc_sim* s, double ms[3]);
int kmc_host_reach_census(const kmc_params* p, const kmc_state_view* v, int32_t nd, int32_t na, kmc_reach_out* out,
                          int64_t* hist_d, int64_t* hist_a_rl, int64_t* hist_a_cis);
int kmc_host_enc_begin(const kmc_params* p, const kmc_state_view* v, const kmc_enc_config* cfg,
                       const kmc_enc_view* view, kmc_enc_out* acc, int64_t* hist10);
int kmc_host_enc_update(const kmc_params* p, const kmc_state_view* v, const kmc_enc_view* view, kmc_enc_out* acc,
                        int64_t* hist10);
int kmc_host_enc_sample(const kmc_params* p, const kmc_enc_view* view, const kmc_enc_out* acc, const int64_t* hist10,
                        kmc_enc_out* out, int64_t* hist, int64_t* react_hist);

/* Proximity clusters: what localisation microscopy measures —
 * DBSCAN / friends-of-friends clusters at a search radius eps, local neighbour
 * counts and nearest-neighbour distances of the CURRENT state — and how well
 * those clusters recover the bonded oligomers, as exact integers.  Like the
 * other analyses the call reads the current state on the device (valid
 * straight after kmc_set_state / kmc_load_*), launches nothing inside kmc_step,
 * reads no step-internal table, leaves the state, the step counter, the
 * recorders, kmc_get_clusters' validity and the other analyses' scratch
 * untouched and is timed by kmc_analysis_ms; its scratch is its own (allocated
 * by the first call, freed by kmc_destroy).
 *
 * Definitions — the device, kmc_host_prox_clusters and the tests share them bit
 * for bit (doubles, no fused multiply-add; round = half away from zero):
 *   position        (x, y) of bead [1][1], as in kmc_pair_counts.
 *   integer coords  X = (int64) round(x * 1024.0), BX = (int64) round(box_x *
 *                   1024.0); the same in y (§12's 2^-10 A).  KMC_ERR_ARG
 *                   unless 1 <= BX, BY < 2^31.
 *   displacement    i -> j: DX = (X_j - X_i) mod BX in [0, BX) (the floor
 *                   modulus); if (2 DX >= BX) DX -= BX; the same in y;
 *                   D2 = DX*DX + DY*DY in int64.
 *   set             which = KMC_PX_A (receptors), KMC_PX_B (ligands) or
 *                   KMC_PX_AB (both species as one point set); select =
 *                   KMC_SK_ALL, or KMC_SK_BOUND: a receptor with nei2 != 0 or
 *                   nei3 != 0, a ligand with any of nei2..4 != 0; mask: NULL
 *                   keeps all, else n_a + n_b bytes by reference index (a
 *                   ligand b at n_a + b), non-zero keeps the protein — the
 *                   labelling efficiency.  The set is the intersection of the
 *                   three; centres and neighbours both come from it.
 *   neighbours      EPS = (int64) round(eps * 1024.0); every j != i of the set
 *                   with D2 <= EPS^2 — an integer test, inclusive and
 *                   symmetric.  Coincident points (D2 = 0) ARE neighbours here,
 *                   unlike §14.  Needs eps > 0, EPS >= 1, floor(BX / EPS) >= 3
 *                   and floor(BY / EPS) >= 3 (integer division), else
 *                   KMC_ERR_ARG.  N_i = the number of neighbours, int32.
 *   core            point i is a core iff N_i + 1 >= min_pts, 1 <= min_pts <=
 *                   2^30.  min_pts = 1 makes every point a core: friends of
 *                   friends.
 *   cluster         a connected component of the cores under "is a neighbour".
 *                   Its label is the smallest reference index among its cores,
 *                   1-based and global (ligand b is n_a + b).
 *   border          a non-core point with at least one core neighbour.  It
 *                   joins the cluster of its nearest core: smallest D2, ties to
 *                   the smaller reference index.  Textbook DBSCAN gives a border
 *                   point to whichever cluster visits it first, so its result
 *                   depends on the visiting order; this rule fixes the choice,
 *                   is local to the point and independent of any order.
 *   noise           any other selected point: label 0.
 *   kind            kind[i] = 0 not in the set, 1 noise, 2 border, 3 core.
 *   size histogram  size_hist[max_size + 1], 1 <= max_size <= 65535: clusters
 *                   by member count (cores plus borders), counts above max_size
 *                   clamped into the last bin; the bins sum to n_clusters.
 *   neighbour hist  nn_hist[KMC_PX_NN_ROWS]: the selected points by min(N_i, 63).
 *   nearest neighb. for every point with N_i > 0, M_i = min D2 over its
 *                   neighbours.  nnd_hist[nbins], 1 <= nbins <= 4096: dr = eps
 *                   / nbins, E_m = (int64) round(((double) m * dr) * 1024.0),
 *                   bin k = #{m in 1..nbins-1 : E_m^2 <= M_i}.  The points with
 *                   N_i = 0 are counted in n_alone instead.
 *   summary         kmc_prox_out: n_sel, n_core, n_border, n_noise, n_alone,
 *                   n_clusters; n_multi = clusters with >= 2 members; sum_nn =
 *                   sum N_i (twice the pairs within eps); n_core_edges = the
 *                   unordered core - core pairs within eps; max_size and
 *                   max_label of the largest cluster, ties to the smallest
 *                   label (0, 0 without a cluster).
 *   purity          against the bond graph: c(i) = kmc_components' label of
 *                   protein i over the WHOLE bond graph (ligands included even
 *                   when the set is receptors only).  n_pure = clusters with
 *                   >= 2 members whose members all have one c; n_whole = the
 *                   pure clusters whose size equals the number of selected
 *                   proteins carrying that c (the oligomers recovered exactly);
 *                   n_bond_multi = bond components with >= 2 selected members;
 *                   n_bond_kept = those whose selected members all carry the
 *                   same non-zero proximity label.
 *   per protein out label[N] (int32), nn[N] (int32), kind[N] (uint8) by
 *                   reference index, N = n_a + n_b, zero for unselected
 *                   proteins; a NULL pointer skips that copy, and each
 *                   histogram may be NULL too.
 * kmc_host_prox_clusters: the same from a host state view, sequentially on a
 * cell grid of its own, no device.  kmc_prox_phase_ms: device milliseconds of
 * the last call's four phases — select and bin; the count walk; the union walk
 * and the flatten; the border walk, the bond components and the reduces.
 * KMC_ERR_ARG for a null handle or out, an out-of-range argument, a handle
 * without state and a decomposed window; KMC_ERR_STATE from the component
 * labelling for a bond link that leaves the state.  Every device loop is
 * bounded, and the number of launches is fixed whatever the clusters look
 * like. */
#define KMC_PX_A 0
#define KMC_PX_B 1
#define KMC_PX_AB 2
#define KMC_PX_NN_ROWS 64
#define KMC_PX_MAX_SIZE 65535
#define KMC_PX_NND_BINS 4096
typedef struct kmc_prox_out {
  int64_t n_sel, n_core, n_border, n_noise, n_alone, n_clusters;
  int64_t n_multi, sum_nn, n_core_edges;
  int64_t n_pure, n_whole, n_bond_multi, n_bond_kept;
  int32_t max_size, max_label;
} kmc_prox_out;
int kmc_prox_clusters(kmc_sim* s, int32_t which, int32_t select, const uint8_t* mask, double eps, int32_t min_pts,
                      int32_t max_size, int32_t nbins, kmc_prox_out* out, int64_t* size_hist /* [max_size + 1] */,
                      int64_t* nn_hist /* [KMC_PX_NN_ROWS] */, int64_t* nnd_hist /* [nbins] */, int32_t* label,
                      int32_t* nn, uint8_t* kind);
int kmc_host_prox_clusters(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t select,
                           const uint8_t* mask, double eps, int32_t min_pts, int32_t max_size, int32_t nbins,
                           kmc_prox_out* out, int64_t* size_hist, int64_t* nn_hist, int64_t* nnd_hist, int32_t* label,
                           int32_t* nn, uint8_t* kind);
int kmc_prox_phase_ms(const kmc_sim* s, double ms[4]);

/* Formatting helpers shared by every host driver.  Each returns the number of
 * characters written (excluding NUL) or < 0. */
int kmc_format_bond_line(const kmc_params* p, const kmc_obs* o, char* buf, size_t n);   /* main.cpp:2251 */

/* FNV-1a-64 hash of a host state view in reference order (beads x,y,z as
 * IEEE bits, then the ints, then counters and step): the per-step parity
 * fingerprint shared by the oracle, the reference trace and the GPU tests. */
uint64_t kmc_state_hash(const kmc_params* p, const kmc_state_view* v);

/* Host-only helpers (no device needed): the same formats and generator as
 * above on caller-owned host buffers. */
const char* kmc_host_last_error(void);
int kmc_host_load_cpt(const kmc_params* p, const char* path, kmc_state_view* v);
int kmc_host_write_cpt(const kmc_params* p, const kmc_state_view* v, const char* path);
int kmc_host_init_random(const kmc_params* p, kmc_state_view* v);
int kmc_host_save_state(const kmc_params* p, const kmc_state_view* v, const char* path);
int kmc_host_load_state(const kmc_params* p, const char* path, kmc_state_view* v);
/* parameter.log (main.cpp:178-205), test.gro frame (2258-2287, appended),
 * cluster.log block (2291-2305, appended) */
int kmc_host_write_parameter_log(const kmc_params* p, const char* path);
int kmc_host_append_gro(const kmc_params* p, const kmc_state_view* v, const char* path);
int kmc_host_append_cluster_log(const kmc_params* p, int64_t step, const int32_t* row_len, const int32_t* members,
                                const char* path);
/* the parameter envelope (kmc_create above), then bond-link consistency +
 * rigid-body extent bound; KMC_OK or an error code */
int kmc_host_validate(const kmc_params* p, const kmc_state_view* v);
/* the parameter envelope alone, exactly what kmc_create accepts: KMC_OK or
 * KMC_ERR_ARG (kmc_host_last_error names the field) */
int kmc_host_check_params(const kmc_params* p);
/* the arguments kmc_dd_set_state checks first: gid[0..n) increasing and in
 * [0, INT32_MAX), own[i] 0 or 1; KMC_OK or KMC_ERR_ARG */
int kmc_host_dd_check(int32_t n, const int32_t* gid, const uint8_t* own);

/* Domain decomposition of ONE trajectory over several handles (SURVEY.md
 * §8(f).4; the host driver is slabs.py).  The reference has no
 * counterpart: its step is one sequential loop (main.cpp:577, 1877-2058).
 * A handle created for the n_a + n_b proteins of one slab's window (the
 * proteins its slab owns plus halo copies of its neighbours') simulates the
 * window with the trajectory's own random streams:
 *   kmc_dd_set_state  the window in local numbering (receptors, then ligands,
 *                     each increasing in the global index gid[]: every order
 *                     the step takes is then the global one), own[i] = 1 for
 *                     the proteins this slab owns (the observables count only
 *                     those; a cis pair at its lower-index member), ctl5 =
 *                     the counters' offsets (bond, rl, cis, mono_cis) and the
 *                     running largest complex of this slab's share.
 *   kmc_dd_export     the end-of-step state of local proteins ids[0..n):
 *                     beads[n][48] (kmc_state_view bead order; a ligand uses
 *                     the first 24) and ints[n][8] (receptor st2 st3 nei2
 *                     nei4 nei3, ligand st1..4 nei1..4; links = local index+1).
 *   kmc_dd_import     the owners' end-of-step state of halo proteins, same
 *                     layout; flags[i] |= 1 where a coordinate differed from
 *                     this handle's own result, 2 where a status / link did.
 *   kmc_dd_drift      the largest periodic x displacement of an owned
 *                     protein since kmc_dd_set_state.
 *   kmc_dd_jumpers    the owned proteins displaced more than S since then:
 *                     *n of them (may exceed cap), the first cap as (local
 *                     index, x of bead [1][1]).
 *   kmc_dd_counters   out[0] collisions of a moved unit's member with a protein
 *                     of the other ownership (owned against halo) whose unit
 *                     moves later in the step, i.e. at its old position — every
 *                     such pair, as the sequential loop would meet them;
 *                     out[1] bonds formed between an owned and a halo protein,
 *                     both since kmc_dd_set_state. */
int kmc_dd_set_state(kmc_sim* s, const kmc_state_view* v, const int32_t* gid, const uint8_t* own,
                     const int32_t* ctl5);
int kmc_dd_export(kmc_sim* s, int32_t n, const int32_t* ids, double* beads, int32_t* ints);
int kmc_dd_import(kmc_sim* s, int32_t n, const int32_t* ids, const double* beads, const int32_t* ints,
                  uint8_t* flags);
int kmc_dd_drift(kmc_sim* s, double* max_dx);
int kmc_dd_jumpers(kmc_sim* s, double S, int32_t cap, int32_t* ids, double* xs, int32_t* n);
int kmc_dd_counters(kmc_sim* s, int64_t* out);

/* The halo exchange on device memory (the per-step path of slabs.py; the
 * host-buffer export / import above stay for diagnostics).  One exchanged
 * row is KMC_DD_ROW bytes: 48 doubles (kmc_dd_export's bead order) then 8
 * int32 (kmc_dd_export's fields) whose links are GLOBAL reference index + 1
 * (0 = none), so a row means the same thing in every window.
 *   kmc_dd_plan    once per partition (and after an ownership change):
 *                  send_ids[n_send] the local ids whose rows this window
 *                  sends, grouped by destination; recv_ids[n_recv] the local
 *                  ids of the rows it receives, grouped by source, each group
 *                  in its source's send order; own[N] replaces the ownership
 *                  of kmc_dd_set_state; band[N] = 1 for the halo proteins
 *                  whose end-of-step state must equal their owner's.  Sent
 *                  proteins must be owned, received ones not.
 *   kmc_dd_step    one step of the window (kmc_step) that also packs the
 *                  end-of-step rows of send_ids into device memory dst
 *                  (n_send rows; NULL: the handle's own send buffer,
 *                  kmc_dd_send_buffer) and lists the owned proteins more
 *                  than S (periodic x) from their x at kmc_dd_set_state —
 *                  all before the step's one wait.
 *   kmc_dd_pack    the rows alone, likewise (returns after the stream drained).
 *   kmc_dd_unpack  rows [first, first + n) of the receive plan from device
 *                  memory src (another handle's send buffer on this device,
 *                  or a collective's receive buffer), enqueued on the
 *                  handle's stream: each row's links go through a binary
 *                  search of the window's global indices; a link to a
 *                  protein the window does not hold is cut with its status;
 *                  the row overwrites this handle's own result and the
 *                  differences are counted.
 *   kmc_dd_finish  waits for the unpacks and returns the step's report: band
 *                  rows that differed or had a link cut (bad; > 0 means the
 *                  step must be redone from a wider partition), rows that
 *                  differed, rows whose status / links differed; kmc_dd_step's
 *                  jumpers (n_jump, the first KMC_DD_JCAP listed as local id
 *                  + x); the bonds formed since the last finish between an
 *                  owned and a halo protein (n_xb, the first KMC_DD_XCAP as
 *                  local id pairs); kmc_dd_counters' values.
 *   kmc_dd_cut_count  how many of ids[n] had a link cut at the last unpack
 *                  (their unit is not held whole by this window).
 * A decomposed window takes no chunk snapshot (the slab driver keeps the
 * checkpoint): a kmc_step that raises a device error leaves the window's
 * state undefined and returns the error; after a list overflow
 * (KMC_ERR_CAPACITY) the lists have already been doubled —
 * kmc_list_growth / kmc_set_list_growth carry that size to the handle the
 * driver rebuilds. */
#define KMC_DD_ROW 416
#define KMC_DD_JCAP 256
#define KMC_DD_XCAP 64
typedef struct kmc_dd_report {
  int64_t xcol, xbond;
  int32_t bad, differed, links, n_jump, n_xb, reserved;
  int32_t jump_id[KMC_DD_JCAP];
  double jump_x[KMC_DD_JCAP];
  int32_t xb[KMC_DD_XCAP][2];
} kmc_dd_report;
int kmc_dd_plan(kmc_sim* s, int32_t n_send, const int32_t* send_ids, int32_t n_recv, const int32_t* recv_ids,
                const uint8_t* own, const uint8_t* band);
int kmc_dd_step(kmc_sim* s, void* dst, double S, kmc_obs* out);
int kmc_dd_pack(kmc_sim* s, void* dst);
void* kmc_dd_send_buffer(kmc_sim* s);
int kmc_dd_unpack(kmc_sim* s, const void* src, int32_t first, int32_t n);
int kmc_dd_finish(kmc_sim* s, kmc_dd_report* out);
int kmc_dd_cut_count(kmc_sim* s, int32_t n, const int32_t* ids, int32_t* count);

/* Output-list capacities as 2^level times their defaults (kmc_step doubles
 * them itself after an overflow, up to level 6). */
int kmc_list_growth(const kmc_sim* s);
int kmc_set_list_growth(kmc_sim* s, int32_t level);

/* Diagnostics: the portable math of kmc_math.h evaluated on the host and on
 * the device (op 0 sin, 1 cos, 2 atan2(x,y), 3 acos, 4 sqrt, 5 x/y, 6 round)
 * — the GPU numerics test compares the two bit for bit. */
int kmc_host_math(int op, const double* x, const double* y, double* out, int64_t n);
int kmc_device_math(int op, const double* x, const double* y, double* out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* KMC_H */
