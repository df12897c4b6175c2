// kmc_run.cpp — drop-in replacement for the reference executable.
//
// Reproduces main.cpp's process/file contract on top of libkmc (include/kmc.h):
//   * writes parameter.log (main.cpp:169-205);
//   * resumes from ./position.cpt when it exists, continuing at saved step + 1
//     (main.cpp:226-270); otherwise truncates test.gro, bond.dat, cluster.log
//     and position.cpt and draws a random configuration (main.cpp:273-456);
//   * runs the diffusion–reaction loop on the GPU up to simu_step
//     (main.cpp:461-2308);
//   * every out_interval steps (5000, main.cpp:2206) rewrites position.cpt and
//     appends bond.dat, test.gro and cluster.log (main.cpp:2206-2305).
// Parameters that are compile-time #defines / globals in the reference
// (main.cpp:39-99) are command-line options here:
//   kmc_run [--n-a 150] [--n-b 50] [--steps 20000000] [--box 5773 5773 1000]
//           [--out-interval 5000] [--seed 1] [--replica 0] [--device 0]
//           [--set name=value ...]   (any kmc_params field, e.g. ass_rate=0.04)
//           [--state FILE]   exact checkpoint (include/kmc.h, KMCSTAT1): resumed
//                            from when it exists (instead of position.cpt) and
//                            rewritten with position.cpt every out_interval
//           [--census FILE]  every out_interval, one line per non-empty bin of the
//                            oligomer census (kmc_oligomer_census): step n_r n_l count
//           [--rdf WHICH RMAX NBINS FILE]  every out_interval, the lateral pair counts
//                            (kmc_pair_counts; WHICH = AA, AB or BB): step k count
//                            (both appended; truncated on a fresh start, like bond.dat;
//                            census bins clamp at 63 receptors / 63 ligands)
//           [--geom MAXSIZE FILE]  every out_interval, the cluster geometry
//                            (kmc_cluster_geometry; 2 <= MAXSIZE <= 1023, larger clusters clamp
//                            into the last bin), appended like the census: per non-empty bin
//                              step size count sum_m_hi sum_m_lo      (Rg² = m / n² / 2^20 Å²)
//                            and one line
//                              step span n_spanning n_span_x n_span_y largest_size largest_span
//           [--sq HMAX KMAX FILE]  every out_interval, the structure factor sums of every
//                            protein (kmc_structure_factor, KMC_SK_ALL; 0 <= HMAX, KMAX <= 64),
//                            appended like the census: one line per wave vector
//                              step h k C_A S_A C_B S_B      (exact integers, terms in units of 2^-30)
//           [--psi WHICH FOLD RCUT NBINS FILE]  every out_interval, the bond-orientational order
//                            of species WHICH (A or B) over the neighbours within RCUT
//                            (kmc_bond_order, KMC_BO_WITHIN, KMC_BO_ALL; 1 <= FOLD <= 12,
//                            1 <= NBINS <= 1024), appended like the census: per non-empty bin
//                              step row bin count      (row = min(neighbours, 15), bin of |psi|)
//                            and one line
//                              step sum n_sel n_with sum_nn sum_pc sum_ps sum_m
//           [--prox WHICH EPS MINPTS MAXSIZE FILE]  every out_interval, the proximity clusters of the
//                            point set WHICH (A, B or AB) at the search radius EPS (kmc_prox_clusters,
//                            KMC_SK_ALL, no mask; MINPTS >= 1, 1 <= MAXSIZE <= 65535), appended like the
//                            census: per non-empty bin of the size histogram
//                              step size count
//                            and one line with kmc_prox_out's fields in their order
//                              step sum n_sel n_core n_border n_noise n_alone n_clusters n_multi sum_nn
//                                       n_core_edges n_pure n_whole n_bond_multi n_bond_kept max_size max_label
//           [--rings MAXLEN FILE]  every out_interval, the rings of the ligand network of up to
//                            MAXLEN bridges (kmc_rings; 1 <= MAXLEN <= 12), appended like the
//                            census: one line
//                              step len all chordless     (per length with a ring)
//                            and one line
//                              step net n_bridges n_loops n_half n_free_dimers n_vertices
//                                   n_net_components cycle_rank
//           [--dyn EVERY RMAX NBINS FILE]  displacement tracking (kmc_track_*): the origin is
//                            the state the process starts or resumes from (the tracker is
//                            not checkpointed: a resume starts a new origin, every line
//                            carries it); kmc_step runs in pieces of at most EVERY steps
//                            with an update after each; every out_interval FILE gets
//                              msd step origin class n n_clean sum_u2 sum_u2_clean
//                              surv step origin rl0 rl_now rl_kept cis0 cis_now cis_kept
//                              vh step class k count        (non-empty van Hove bins)
//           [--kin EVERY FILE]  bond kinetics (kmc_kin_*): the recorder begins at the state the
//                            process starts or resumes from (it is not checkpointed: a resume
//                            starts a new origin, every kin line carries it); kmc_step runs in
//                            pieces of at most EVERY steps with an update after each (EVERY = 1:
//                            exact lifetimes); every out_interval FILE gets one line
//                              kin step origin n_updates rl_on rl_off rl_swap cis_on cis_off_mono
//                                  cis_off_cx cis_swap exp_rl exp_mono exp_cx exp_free_receptor
//                                  exp_free_site occ_rl occ_mono occ_cx occ_free_receptor
//                                  occ_free_site n_rl_censored_alive n_cis_censored_alive
//                            and per non-empty bin of the histogram since that origin
//                              life step row bin count
//           [--reach FILE]   reach census (kmc_reach_census, 16 distance and 18 angle bins): every
//                            out_interval FILE gets per channel (0 R-L, 1 mono cis, 2 complex cis)
//                              reach step channel n_reach n_reactive
//                            then
//                              reachrl step free_receptors free_sites receptors_in_reach sites_in_reach
//                                      max_partners
//                            and per non-empty bin
//                              rd step channel reactive k count     (distance bins)
//                              ra step i j count                    (R-L: |theta_pd| bin, |theta_ot - 180| bin)
//                              rc step kind k count                 (cis, kind 0 mono 1 complex: |theta_ot - 180| bin)
//           [--enc EVERY FILE]  R-L encounter recorder (kmc_enc_*): it begins at the state the process starts
//                            or resumes from (not checkpointed: a resume starts a new origin, every enc line
//                            carries it); kmc_step runs in pieces that end where an update is due, EVERY steps
//                            after the last one, on across the intervals; every out_interval FILE gets one line
//                              enc step origin last_step n_updates on_from_encounter on_direct n_opened n_ended
//                                  exp_reach exp_reactive exp_free_receptor n_overflow occ_reach occ_reactive
//                                  occ_free_receptor n_censored_alive every slots
//                            and per non-empty bin of the histograms since that origin
//                              dwell step row bin count
//                              react step row bin count             (row 0: ended in the bond, 1: otherwise)
//           [--cf EVERY SMAX FILE]  cluster growth kinetics (kmc_cf_*, sizes clamped at SMAX): the
//                            recorder begins where the process starts or resumes (a new origin,
//                            as --kin's); an update after every piece of at most EVERY steps;
//                            every out_interval FILE gets, since that origin,
//                              cf step origin n_updates max_size formed_rl formed_cis broken_rl
//                                 broken_cis n_cores n_clusters cycles_closed cycles_opened max_cluster
//                              merge step a b count          (non-zero bins, a <= b)
//                              frag step a b count
//                              pieces step k mergers fragmentations       (non-zero rows)
//                              sizes step s n_s expo merge_product frag_parent (non-zero rows)
//           [--lag EVERY LEVELS SLOTS FILE]  multi-origin lag correlator (kmc_lag_*): the recorder
//                            begins where the process starts or resumes (it is not checkpointed: a
//                            new origin, every line carries it); kmc_step runs in pieces that end
//                            where an update is due, EVERY steps after the last one (the stride runs
//                            on across the output steps); every out_interval FILE gets, since that
//                            origin, one line
//                              lag step origin n_updates every levels slots J F BX BY
//                            and per non-empty cell (the 128-bit sums in decimal)
//                              cell step origin row lag class n_pairs n_all n_clean n_far m2_all
//                                   m2_clean m4_clean
//           [--rot EVERY LEVELS SLOTS FILE]  orientation recorder (kmc_rot_*), scheduled as --lag is and
//                            with an origin of its own; every out_interval FILE gets, since that origin,
//                              rot step origin n_updates every levels slots
//                            and per non-empty cell (the 128-bit sums in decimal; v: 0 heading / axis, 1 arm)
//                              cell step origin row lag class v n_pairs n_all n_clean s1_all s1_clean s2_clean
//           [--pd EVERY SAMPLE_EVERY RMAX NBINS FILE]  pair dynamics (kmc_pd_*): distinct van Hove and
//                            displacement correlation against the origin where the process starts or
//                            resumes (not checkpointed: a new origin, every line carries it); updates
//                            every EVERY steps as --lag's, and after every SAMPLE_EVERY-th update FILE gets
//                              pd step origin n_updates every nbins J F BX BY
//                            and per non-empty cell (the 128-bit sums in decimal)
//                              gd step origin kind k count             (kind = 2 species(i) + species(j))
//                              gs step origin species k count
//                              cu step origin kind k n_pairs n_valid dot sq   (kind: 0 AA, 1 AB, 2 BB)
//           [--bd EVERY SAMPLE_EVERY MAX_SIZE FILE]  body dynamics (kmc_bd_*): the clusters of the state where the
//                            process starts or resumes are the bodies (not checkpointed: a new origin, every
//                            line carries it); updates every EVERY steps as --lag's, and after every
//                            SAMPLE_EVERY-th update FILE gets
//                              bd step origin n_updates every max_size J F BX BY n_bodies
//                            and per non-empty cell (hl: holds a ligand; k = min(size, max_size); the 128-bit
//                            sums in decimal)
//                              body step origin hl k n_bodies sum_size n_pristine n_intact n_grown n_broken
//                                   n_valid n_rot n_rot_null n_rot_skipped c1 c2 m2 phi2
//           [--pose NZ NC FILE]  ligand pose census (kmc_ligand_pose) of every output step:
//                              pose step nz nc n_bad chi_pos[0..3] chi_neg[0..3]
//                              bin step k zbin tiltbin count          (non-zero bins)
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kmc.h"

namespace {

// a kmc_i128 in decimal
std::string dec128(kmc_i128 w) {
  unsigned __int128 u = (unsigned __int128)(uint64_t)w.hi << 64 | w.lo;
  const bool neg = w.hi < 0;
  if (neg) u = ~u + 1;
  std::string d;
  do {
    d.insert(d.begin(), (char)('0' + (int)(u % 10)));
    u /= 10;
  } while (u);
  return neg ? "-" + d : d;
}

// --pd: one sample's non-empty cells appended to path, every line with the current and the origin step
int pd_append(kmc_sim* s, const char* path) {
  kmc_pd_out k;
  int rc = kmc_pd_sample(s, &k, nullptr, nullptr, nullptr);
  if (rc) return rc;
  const int nb = k.cfg.nbins;
  std::vector<int64_t> gd((size_t)4 * nb), gs((size_t)2 * nb);
  std::vector<kmc_pd_cell> cu((size_t)3 * nb);
  rc = kmc_pd_sample(s, &k, gd.data(), gs.data(), cu.data());
  if (rc) return rc;
  FILE* f = fopen(path, "ab");
  if (!f) return KMC_ERR_IO;
  const long long step = (long long)k.last_step, o = (long long)k.origin_step;
  fprintf(f, "pd %lld %lld %lld %d %d %lld %lld %lld %lld\n", step, o, (long long)k.n_updates, k.cfg.every, nb,
          (long long)k.J, (long long)k.F, (long long)k.BX, (long long)k.BY);
  for (int t = 0; t < 4; ++t)
    for (int b = 0; b < nb; ++b)
      if (gd[(size_t)t * nb + b]) fprintf(f, "gd %lld %lld %d %d %lld\n", step, o, t, b, (long long)gd[(size_t)t * nb + b]);
  for (int t = 0; t < 2; ++t)
    for (int b = 0; b < nb; ++b)
      if (gs[(size_t)t * nb + b]) fprintf(f, "gs %lld %lld %d %d %lld\n", step, o, t, b, (long long)gs[(size_t)t * nb + b]);
  for (int t = 0; t < 3; ++t)
    for (int b = 0; b < nb; ++b) {
      const kmc_pd_cell& w = cu[(size_t)t * nb + b];
      if (w.n_pairs)
        fprintf(f, "cu %lld %lld %d %d %lld %lld %s %s\n", step, o, t, b, (long long)w.n_pairs, (long long)w.n_valid,
                dec128(w.dot).c_str(), dec128(w.sq).c_str());
    }
  fclose(f);
  return KMC_OK;
}

// --bd: one sample's non-empty cells appended to path, every line with the current and the origin step
int bd_append(kmc_sim* s, const char* path) {
  kmc_bd_out k;
  int rc = kmc_bd_sample(s, &k, nullptr);
  if (rc) return rc;
  const int ms = k.cfg.max_size;
  std::vector<kmc_bd_cell> table((size_t)2 * (ms + 1));
  rc = kmc_bd_sample(s, &k, table.data());
  if (rc) return rc;
  FILE* f = fopen(path, "ab");
  if (!f) return KMC_ERR_IO;
  const long long step = (long long)k.last_step, o = (long long)k.origin_step;
  fprintf(f, "bd %lld %lld %lld %d %d %lld %lld %lld %lld %lld\n", step, o, (long long)k.n_updates, k.cfg.every, ms,
          (long long)k.J, (long long)k.F, (long long)k.BX, (long long)k.BY, (long long)k.n_bodies);
  for (int hl = 0; hl < 2; ++hl)
    for (int b = 0; b <= ms; ++b) {
      const kmc_bd_cell& w = table[(size_t)hl * (ms + 1) + b];
      if (!w.n_bodies) continue;
      fprintf(f, "body %lld %lld %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %s %s\n", step, o, hl,
              b, (long long)w.n_bodies, (long long)w.sum_size, (long long)w.n_pristine, (long long)w.n_intact,
              (long long)w.n_grown, (long long)w.n_broken, (long long)w.n_valid, (long long)w.n_rot,
              (long long)w.n_rot_null, (long long)w.n_rot_skipped, (long long)w.c1, (long long)w.c2,
              dec128(w.m2).c_str(), dec128(w.phi2).c_str());
    }
  fclose(f);
  return KMC_OK;
}

bool set_field(kmc_params* p, const std::string& k, const std::string& v) {
  double d = strtod(v.c_str(), nullptr);
#define F(name)            \
  if (k == #name) {        \
    p->name = (decltype(p->name))d; \
    return true;           \
  }
  F(n_a) F(n_b) F(time_step) F(box_x) F(box_y) F(box_z) F(pai) F(ra_radius) F(ra_D) F(ra_rot_D) F(rb_radius)
  F(rb_D) F(rb_rot_D) F(mono_cis_ass_rate) F(mono_cis_diss_rate) F(cis_D) F(cis_rot_D) F(cis_ass_rate)
  F(cis_diss_rate) F(bond_D) F(bond_rot_D) F(ass_rate) F(diss_rate) F(bond_dist_cutoff) F(bond_thetapd_cutoff)
  F(bond_thetaot_cutoff) F(cis_thetaot_cutoff) F(cis_dist_cutoff) F(simu_step) F(out_interval) F(replica)
#undef F
  if (k == "seed") {
    p->seed = strtoull(v.c_str(), nullptr, 10);
    return true;
  }
  return false;
}

int die(kmc_sim* s, int rc, const char* what) {
  fprintf(stderr, "kmc_run: %s failed (%d): %s\n", what, rc, s ? kmc_last_error(s) : kmc_host_last_error());
  return 1;
}

bool exists(const char* path) {
  struct stat st;
  return stat(path, &st) == 0;
}

void truncate(const char* path) {
  FILE* f = fopen(path, "wb");
  if (f) fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  kmc_params p;
  kmc_params_default(&p);
  int device = 0;
  std::string state_path, census_path, rdf_path, dyn_path, geom_path, sq_path, psi_path, kin_path, cf_path, rings_path, lag_path;
  int rings_max = 0;
  int psi_which = -1, psi_fold = 0, psi_nbins = 0;
  std::string prox_path;
  int prox_which = -1, prox_min_pts = 0, prox_max_size = 0;
  double prox_eps = 0.0;
  double psi_rcut = 0.0;
  int rdf_which = -1, rdf_nbins = 0, dyn_nbins = 0, geom_max = 0, sq_hmax = 0, sq_kmax = 0;
  double rdf_rmax = 0.0, dyn_rmax = 0.0;
  int64_t dyn_every = 0, kin_every = 0, cf_every = 0;
  std::string reach_path, enc_path;
  kmc_enc_config enc_cfg = {0, 0};
  int cf_smax = 0;
  kmc_lag_config lag_cfg;
  std::memset(&lag_cfg, 0, sizeof lag_cfg);
  std::string rot_path, pose_path;
  kmc_rot_config rot_cfg = {0, 0, 0};
  std::string pd_path;
  kmc_pd_config pd_cfg = {0, 0, 0.0, 0.0, 0.0};
  int pd_sample_every = 0;
  std::string bd_path;
  kmc_bd_config bd_cfg = {0, 0, 0.0, 0.0};
  int bd_sample_every = 0;
  int pose_nz = 0, pose_nc = 0;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) {
        fprintf(stderr, "kmc_run: %s needs a value\n", a.c_str());
        exit(2);
      }
      return argv[++i];
    };
    if (a == "--n-a") p.n_a = atoi(next().c_str());
    else if (a == "--n-b") p.n_b = atoi(next().c_str());
    else if (a == "--steps") p.simu_step = atoll(next().c_str());
    else if (a == "--box") {
      p.box_x = atof(next().c_str());
      p.box_y = atof(next().c_str());
      p.box_z = atof(next().c_str());
    } else if (a == "--out-interval") p.out_interval = atoi(next().c_str());
    else if (a == "--seed") p.seed = strtoull(next().c_str(), nullptr, 10);
    else if (a == "--replica") p.replica = (uint32_t)atoi(next().c_str());
    else if (a == "--device") device = atoi(next().c_str());
    else if (a == "--state") state_path = next();
    else if (a == "--census") census_path = next();
    else if (a == "--rdf") {
      const std::string w = next();
      rdf_which = w == "AA" ? KMC_PAIR_AA : w == "AB" ? KMC_PAIR_AB : w == "BB" ? KMC_PAIR_BB : -1;
      rdf_rmax = atof(next().c_str());
      rdf_nbins = atoi(next().c_str());
      rdf_path = next();
      if (rdf_which < 0 || !(rdf_rmax > 0.0) || rdf_nbins < 1 || rdf_nbins > KMC_PAIR_MAX_BINS) {
        fprintf(stderr, "kmc_run: bad --rdf %s %g %d\n", w.c_str(), rdf_rmax, rdf_nbins);
        return 2;
      }
    }
    else if (a == "--geom") {
      geom_max = atoi(next().c_str());
      geom_path = next();
      if (geom_max < 2 || geom_max > KMC_GEOM_MAX_SIZE) {
        fprintf(stderr, "kmc_run: bad --geom %d\n", geom_max);
        return 2;
      }
    }
    else if (a == "--sq") {
      sq_hmax = atoi(next().c_str());
      sq_kmax = atoi(next().c_str());
      sq_path = next();
      if (sq_hmax < 0 || sq_hmax > KMC_SK_MAX || sq_kmax < 0 || sq_kmax > KMC_SK_MAX) {
        fprintf(stderr, "kmc_run: bad --sq %d %d\n", sq_hmax, sq_kmax);
        return 2;
      }
    }
    else if (a == "--psi") {
      const std::string w = next();
      psi_which = w == "A" ? KMC_BO_A : w == "B" ? KMC_BO_B : -1;
      psi_fold = atoi(next().c_str());
      psi_rcut = atof(next().c_str());
      psi_nbins = atoi(next().c_str());
      psi_path = next();
      if (psi_which < 0 || psi_fold < 1 || psi_fold > KMC_BO_MAX_FOLD || !(psi_rcut > 0.0) || psi_nbins < 1 ||
          psi_nbins > 1024) {
        fprintf(stderr, "kmc_run: bad --psi %s %d %g %d\n", w.c_str(), psi_fold, psi_rcut, psi_nbins);
        return 2;
      }
    }
    else if (a == "--rings") {
      rings_max = atoi(next().c_str());
      rings_path = next();
      if (rings_max < 1 || rings_max > KMC_RING_MAX) {
        fprintf(stderr, "kmc_run: bad --rings %d\n", rings_max);
        return 2;
      }
    }
    else if (a == "--dyn") {
      dyn_every = atoll(next().c_str());
      dyn_rmax = atof(next().c_str());
      dyn_nbins = atoi(next().c_str());
      dyn_path = next();
      if (dyn_every < 1 || !(dyn_rmax > 0.0) || dyn_nbins < 1 || dyn_nbins > KMC_TRACK_MAX_BINS) {
        fprintf(stderr, "kmc_run: bad --dyn %lld %g %d\n", (long long)dyn_every, dyn_rmax, dyn_nbins);
        return 2;
      }
    }
    else if (a == "--prox") {
      const std::string w = next();
      prox_which = w == "A" ? KMC_PX_A : w == "B" ? KMC_PX_B : w == "AB" ? KMC_PX_AB : -1;
      prox_eps = atof(next().c_str());
      prox_min_pts = atoi(next().c_str());
      prox_max_size = atoi(next().c_str());
      prox_path = next();
      if (prox_which < 0 || !(prox_eps > 0.0) || prox_min_pts < 1 || prox_max_size < 1 ||
          prox_max_size > KMC_PX_MAX_SIZE) {
        fprintf(stderr, "kmc_run: bad --prox %s %g %d %d\n", w.c_str(), prox_eps, prox_min_pts, prox_max_size);
        return 2;
      }
    }
    else if (a == "--reach") {
      reach_path = next();
    }
    else if (a == "--enc") {
      enc_cfg.every = atoi(next().c_str());
      enc_path = next();
      if (enc_cfg.every < 1) {
        fprintf(stderr, "kmc_run: bad --enc %d\n", enc_cfg.every);
        return 2;
      }
    }
    else if (a == "--kin") {
      kin_every = atoll(next().c_str());
      kin_path = next();
      if (kin_every < 1) {
        fprintf(stderr, "kmc_run: bad --kin %lld\n", (long long)kin_every);
        return 2;
      }
    }
    else if (a == "--cf") {
      cf_every = atoll(next().c_str());
      cf_smax = atoi(next().c_str());
      cf_path = next();
      if (cf_every < 1 || cf_smax < 2 || cf_smax > KMC_CF_MAX_SIZE) {
        fprintf(stderr, "kmc_run: bad --cf %lld %d\n", (long long)cf_every, cf_smax);
        return 2;
      }
    }
    else if (a == "--lag") {
      lag_cfg.every = atoi(next().c_str());
      lag_cfg.levels = atoi(next().c_str());
      lag_cfg.slots = atoi(next().c_str());
      lag_path = next();
      if (lag_cfg.every < 1 || lag_cfg.levels < 1 || lag_cfg.levels > KMC_LAG_MAX_LEVELS || lag_cfg.slots < 2 ||
          lag_cfg.slots > KMC_LAG_MAX_SLOTS || lag_cfg.slots % 2) {
        fprintf(stderr, "kmc_run: bad --lag %d %d %d\n", lag_cfg.every, lag_cfg.levels, lag_cfg.slots);
        return 2;
      }
    }
    else if (a == "--pd") {
      pd_cfg.every = atoi(next().c_str());
      pd_sample_every = atoi(next().c_str());
      pd_cfg.r_max = strtod(next().c_str(), nullptr);
      pd_cfg.nbins = atoi(next().c_str());
      pd_path = next();
      if (pd_cfg.every < 1 || pd_sample_every < 1 || !(pd_cfg.r_max > 0.0) || pd_cfg.nbins < 1 ||
          pd_cfg.nbins > KMC_PD_MAX_BINS) {
        fprintf(stderr, "kmc_run: bad --pd %d %d %g %d\n", pd_cfg.every, pd_sample_every, pd_cfg.r_max, pd_cfg.nbins);
        return 2;
      }
    }
    else if (a == "--bd") {
      bd_cfg.every = atoi(next().c_str());
      bd_sample_every = atoi(next().c_str());
      bd_cfg.max_size = atoi(next().c_str());
      bd_path = next();
      if (bd_cfg.every < 1 || bd_sample_every < 1 || bd_cfg.max_size < 2 || bd_cfg.max_size > KMC_BD_MAX_SIZE) {
        fprintf(stderr, "kmc_run: bad --bd %d %d %d\n", bd_cfg.every, bd_sample_every, bd_cfg.max_size);
        return 2;
      }
    }
    else if (a == "--rot") {
      rot_cfg.every = atoi(next().c_str());
      rot_cfg.levels = atoi(next().c_str());
      rot_cfg.slots = atoi(next().c_str());
      rot_path = next();
      if (rot_cfg.every < 1 || rot_cfg.levels < 1 || rot_cfg.levels > KMC_LAG_MAX_LEVELS || rot_cfg.slots < 2 ||
          rot_cfg.slots > KMC_LAG_MAX_SLOTS || rot_cfg.slots % 2) {
        fprintf(stderr, "kmc_run: bad --rot %d %d %d\n", rot_cfg.every, rot_cfg.levels, rot_cfg.slots);
        return 2;
      }
    }
    else if (a == "--pose") {
      pose_nz = atoi(next().c_str());
      pose_nc = atoi(next().c_str());
      pose_path = next();
      if (pose_nz < 1 || pose_nz > KMC_POSE_MAX_BINS || pose_nc < 1 || pose_nc > KMC_POSE_MAX_BINS) {
        fprintf(stderr, "kmc_run: bad --pose %d %d\n", pose_nz, pose_nc);
        return 2;
      }
    }
    else if (a == "--set") {
      std::string kv = next();
      size_t eq = kv.find('=');
      if (eq == std::string::npos || !set_field(&p, kv.substr(0, eq), kv.substr(eq + 1))) {
        fprintf(stderr, "kmc_run: bad --set %s\n", kv.c_str());
        return 2;
      }
    } else {
      fprintf(stderr, "kmc_run: unknown option %s\n", a.c_str());
      return 2;
    }
  }
  if (p.out_interval <= 0) p.out_interval = 5000;

  int rc = kmc_host_write_parameter_log(&p, "parameter.log");
  if (rc) return die(nullptr, rc, "parameter.log");
  kmc_sim* s = nullptr;
  rc = kmc_create(&p, device, &s);
  if (rc) return die(nullptr, rc, "kmc_create");
  if (!state_path.empty() && exists(state_path.c_str())) {
    printf("STATE file is exist\n");
    rc = kmc_load_state(s, state_path.c_str());
    if (rc) return die(s, rc, state_path.c_str());
  } else if (exists("position.cpt")) {
    printf("CPT file is exist\n");
    rc = kmc_load_cpt(s, "position.cpt");
    if (rc) return die(s, rc, "position.cpt");
  } else {
    printf("CPT file not exist\n");
    truncate("test.gro");
    truncate("bond.dat");
    truncate("cluster.log");
    truncate("position.cpt");
    if (!census_path.empty()) truncate(census_path.c_str());
    if (!rdf_path.empty()) truncate(rdf_path.c_str());
    if (!dyn_path.empty()) truncate(dyn_path.c_str());
    if (!geom_path.empty()) truncate(geom_path.c_str());
    if (!sq_path.empty()) truncate(sq_path.c_str());
    if (!psi_path.empty()) truncate(psi_path.c_str());
    if (!prox_path.empty()) truncate(prox_path.c_str());
    if (!rings_path.empty()) truncate(rings_path.c_str());
    if (!kin_path.empty()) truncate(kin_path.c_str());
    if (!cf_path.empty()) truncate(cf_path.c_str());
    if (!lag_path.empty()) truncate(lag_path.c_str());
    if (!rot_path.empty()) truncate(rot_path.c_str());
    if (!pd_path.empty()) truncate(pd_path.c_str());
    if (!bd_path.empty()) truncate(bd_path.c_str());
    if (!pose_path.empty()) truncate(pose_path.c_str());
    if (!reach_path.empty()) truncate(reach_path.c_str());
    if (!enc_path.empty()) truncate(enc_path.c_str());
    rc = kmc_init_random(s);
    if (rc) return die(s, rc, "random placement");
  }
  fflush(stdout);

  const int na = p.n_a, nb = p.n_b;
  std::vector<double> ra((size_t)48 * na + 1), rb((size_t)24 * nb + 1);
  std::vector<int32_t> ai((size_t)5 * na + 1), bi((size_t)8 * nb + 1), row((size_t)nb + 1),
      mem((size_t)na + nb + 1);
  kmc_state_view v{ra.data(), rb.data(), ai.data(), bi.data(), {0, 0, 0, 0, 0}, 0, 0};
  std::vector<kmc_obs> obs;
  const int census_max = 63;  // census rows / columns: 0..63 receptors / ligands, more clamp into the last
  std::vector<int64_t> hist((size_t)(census_max + 1) * (census_max + 1)), pairs((size_t)rdf_nbins + 1);
  std::vector<kmc_geom_bin> geom((size_t)geom_max + 1);
  const size_t sq_nq = (size_t)(sq_hmax + 1) * (2 * sq_kmax + 1);
  std::vector<int64_t> sq(sq_path.empty() ? 0 : 4 * sq_nq);
  std::vector<int64_t> psi((size_t)KMC_BO_NN_ROWS * psi_nbins + 1);
  std::vector<int64_t> vh((size_t)KMC_TRACK_CLASSES * dyn_nbins + 1);
  if (!dyn_path.empty()) {
    rc = kmc_track_begin(s, 0.0);
    if (rc) return die(s, rc, "track begin");
  }
  std::vector<int64_t> life(kin_path.empty() ? 0 : (size_t)KMC_KIN_HISTS * KMC_KIN_BINS);
  if (!kin_path.empty()) {
    rc = kmc_kin_begin(s);
    if (rc) return die(s, rc, "kinetics begin");
  }
  if (!cf_path.empty()) {
    rc = kmc_cf_begin(s, cf_smax);
    if (rc) return die(s, rc, "growth begin");
  }
  int64_t lag_left = lag_cfg.every;  // steps until the correlator's next update: its stride runs on across the intervals
  if (!lag_path.empty()) {
    rc = kmc_lag_begin(s, &lag_cfg);
    if (rc) return die(s, rc, "lag begin");
  }
  int64_t rot_left = rot_cfg.every;
  if (!rot_path.empty()) {
    rc = kmc_rot_begin(s, &rot_cfg);
    if (rc) return die(s, rc, "rot begin");
  }
  int64_t pd_left = pd_cfg.every;
  if (!pd_path.empty()) {
    rc = kmc_pd_begin(s, &pd_cfg);
    if (rc) return die(s, rc, "pd begin");
  }
  int64_t bd_left = bd_cfg.every;
  if (!bd_path.empty()) {
    rc = kmc_bd_begin(s, &bd_cfg);
    if (rc) return die(s, rc, "bd begin");
  }
  int64_t enc_left = enc_cfg.every;
  if (!enc_path.empty()) {
    rc = kmc_enc_begin(s, &enc_cfg);
    if (rc) return die(s, rc, "enc begin");
  }
  int64_t step = kmc_current_step(s);
  while (step < p.simu_step) {
    int64_t next_out = (step / p.out_interval + 1) * p.out_interval;
    int64_t end = next_out < p.simu_step ? next_out : p.simu_step;
    int64_t n = end - step;
    obs.resize((size_t)n);
    if (dyn_path.empty() && kin_path.empty() && cf_path.empty() && lag_path.empty() && rot_path.empty() &&
        pd_path.empty() && bd_path.empty() && enc_path.empty()) {
      rc = kmc_step(s, n, obs.data());
      if (rc) return die(s, rc, "kmc_step");
    } else {
      // pieces end where the tracker's or the recorder's next update is due (each counts from the interval's start)
      const int64_t far = n + 1;
      int64_t dyn_left = dyn_path.empty() ? far : dyn_every, kin_left = kin_path.empty() ? far : kin_every;
      int64_t cf_left = cf_path.empty() ? far : cf_every;
      for (int64_t done = 0; done < n;) {
        int64_t m = n - done;
        if (dyn_left < m) m = dyn_left;
        if (kin_left < m) m = kin_left;
        if (cf_left < m) m = cf_left;
        if (!lag_path.empty() && lag_left < m) m = lag_left;
        if (!rot_path.empty() && rot_left < m) m = rot_left;
        if (!pd_path.empty() && pd_left < m) m = pd_left;
        if (!bd_path.empty() && bd_left < m) m = bd_left;
        if (!enc_path.empty() && enc_left < m) m = enc_left;
        rc = kmc_step(s, m, obs.data() + done);
        if (rc) return die(s, rc, "kmc_step");
        done += m;
        dyn_left -= m;
        kin_left -= m;
        cf_left -= m;
        lag_left -= m;
        rot_left -= m;
        pd_left -= m;
        bd_left -= m;
        enc_left -= m;
        if (!enc_path.empty() && enc_left == 0) {
          rc = kmc_enc_update(s, nullptr);
          if (rc) return die(s, rc, "enc update");
          enc_left = enc_cfg.every;
        }
        if (!dyn_path.empty() && (dyn_left == 0 || done == n)) {
          rc = kmc_track_update(s, nullptr);
          if (rc) return die(s, rc, "track update");
          dyn_left = dyn_every;
        }
        if (!kin_path.empty() && (kin_left == 0 || done == n)) {
          rc = kmc_kin_update(s, nullptr);
          if (rc) return die(s, rc, "kinetics update");
          kin_left = kin_every;
        }
        if (!cf_path.empty() && (cf_left == 0 || done == n)) {
          rc = kmc_cf_update(s, nullptr);
          if (rc) return die(s, rc, "growth update");
          cf_left = cf_every;
        }
        if (!lag_path.empty() && lag_left == 0) {
          rc = kmc_lag_update(s, nullptr);
          if (rc) return die(s, rc, "lag update");
          lag_left = lag_cfg.every;
        }
        if (!rot_path.empty() && rot_left == 0) {
          rc = kmc_rot_update(s, nullptr);
          if (rc) return die(s, rc, "rot update");
          rot_left = rot_cfg.every;
        }
        if (!pd_path.empty() && pd_left == 0) {
          kmc_pd_info info;
          rc = kmc_pd_update(s, &info);
          if (rc) return die(s, rc, "pd update");
          pd_left = pd_cfg.every;
          if (info.n_updates % pd_sample_every == 0) {
            rc = pd_append(s, pd_path.c_str());
            if (rc) return die(s, rc, "pd sample");
          }
        }
        if (!bd_path.empty() && bd_left == 0) {
          kmc_bd_info info;
          rc = kmc_bd_update(s, &info);
          if (rc) return die(s, rc, "bd update");
          bd_left = bd_cfg.every;
          if (info.n_updates % bd_sample_every == 0) {
            rc = bd_append(s, bd_path.c_str());
            if (rc) return die(s, rc, "bd sample");
          }
        }
      }
    }
    step = end;
    if (step % p.out_interval == 0) {
      rc = kmc_write_cpt(s, "position.cpt");
      if (rc) return die(s, rc, "position.cpt");
      if (!state_path.empty()) {
        rc = kmc_save_state(s, state_path.c_str());
        if (rc) return die(s, rc, state_path.c_str());
      }
      char line[256];
      kmc_format_bond_line(&p, &obs.back(), line, sizeof line);
      FILE* f = fopen("bond.dat", "ab");
      if (!f) return die(s, KMC_ERR_IO, "bond.dat");
      fputs(line, f);
      fclose(f);
      rc = kmc_get_state(s, &v);
      if (rc) return die(s, rc, "state");
      rc = kmc_host_append_gro(&p, &v, "test.gro");
      if (rc) return die(s, rc, "test.gro");
      rc = kmc_get_clusters(s, row.data(), mem.data());
      if (rc) return die(s, rc, "clusters");
      rc = kmc_host_append_cluster_log(&p, step, row.data(), mem.data(), "cluster.log");
      if (rc) return die(s, rc, "cluster.log");
      if (!census_path.empty()) {
        kmc_census cs;
        rc = kmc_oligomer_census(s, census_max, census_max, hist.data(), &cs);
        if (rc) return die(s, rc, "census");
        f = fopen(census_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, census_path.c_str());
        for (int r = 0; r <= census_max; ++r)
          for (int l = 0; l <= census_max; ++l)
            if (hist[(size_t)r * (census_max + 1) + l])
              fprintf(f, "%lld %d %d %lld\n", (long long)step, r, l, (long long)hist[(size_t)r * (census_max + 1) + l]);
        fclose(f);
      }
      if (!rdf_path.empty()) {
        rc = kmc_pair_counts(s, rdf_which, rdf_rmax, rdf_nbins, pairs.data());
        if (rc) return die(s, rc, "pair counts");
        f = fopen(rdf_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, rdf_path.c_str());
        for (int k = 0; k < rdf_nbins; ++k) fprintf(f, "%lld %d %lld\n", (long long)step, k, (long long)pairs[k]);
        fclose(f);
      }
      if (!geom_path.empty()) {
        kmc_geom g;
        rc = kmc_cluster_geometry(s, geom_max, geom.data(), &g);
        if (rc) return die(s, rc, "cluster geometry");
        f = fopen(geom_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, geom_path.c_str());
        for (int k = 0; k <= geom_max; ++k)
          if (geom[k].count)
            fprintf(f, "%lld %d %lld %lld %llu\n", (long long)step, k, (long long)geom[k].count,
                    (long long)geom[k].sum_m.hi, (unsigned long long)geom[k].sum_m.lo);
        fprintf(f, "%lld span %lld %lld %lld %d %d\n", (long long)step, (long long)g.n_spanning, (long long)g.n_span_x,
                (long long)g.n_span_y, g.largest_size, g.largest_span);
        fclose(f);
      }
      if (!sq_path.empty()) {
        int64_t n_sel[2];
        rc = kmc_structure_factor(s, sq_hmax, sq_kmax, KMC_SK_ALL, sq.data(), n_sel);
        if (rc) return die(s, rc, "structure factor");
        f = fopen(sq_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, sq_path.c_str());
        for (size_t q = 0; q < sq_nq; ++q)
          fprintf(f, "%lld %d %d %lld %lld %lld %lld\n", (long long)step, (int)(q / (2 * sq_kmax + 1)),
                  (int)(q % (2 * sq_kmax + 1)) - sq_kmax, (long long)sq[q], (long long)sq[sq_nq + q],
                  (long long)sq[2 * sq_nq + q], (long long)sq[3 * sq_nq + q]);
        fclose(f);
      }
      if (!psi_path.empty()) {
        kmc_bond_order_out bo;
        rc = kmc_bond_order(s, psi_which, KMC_BO_WITHIN, psi_fold, psi_rcut, KMC_BO_ALL, psi_nbins, psi.data(), &bo,
                            nullptr, nullptr, nullptr);
        if (rc) return die(s, rc, "bond order");
        f = fopen(psi_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, psi_path.c_str());
        for (int r = 0; r < KMC_BO_NN_ROWS; ++r)
          for (int b = 0; b < psi_nbins; ++b)
            if (psi[(size_t)r * psi_nbins + b])
              fprintf(f, "%lld %d %d %lld\n", (long long)step, r, b, (long long)psi[(size_t)r * psi_nbins + b]);
        fprintf(f, "%lld sum %lld %lld %lld %lld %lld %lld\n", (long long)step, (long long)bo.n_sel,
                (long long)bo.n_with, (long long)bo.sum_nn, (long long)bo.sum_pc, (long long)bo.sum_ps,
                (long long)bo.sum_m);
        fclose(f);
      }
      if (!rings_path.empty()) {
        int64_t rc_counts[2][KMC_RING_MAX + 1];
        kmc_net_out net;
        rc = kmc_rings(s, rings_max, &rc_counts[0][0], nullptr, &net);
        if (rc) return die(s, rc, "rings");
        f = fopen(rings_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, rings_path.c_str());
        for (int len = 1; len <= rings_max; ++len)
          if (rc_counts[0][len])
            fprintf(f, "%lld %d %lld %lld\n", (long long)step, len, (long long)rc_counts[0][len],
                    (long long)rc_counts[1][len]);
        fprintf(f, "%lld net %lld %lld %lld %lld %lld %lld %lld\n", (long long)step, (long long)net.n_bridges,
                (long long)net.n_loops, (long long)net.n_half, (long long)net.n_free_dimers, (long long)net.n_vertices,
                (long long)net.n_net_components, (long long)net.cycle_rank);
        fclose(f);
      }
      if (!dyn_path.empty()) {
        kmc_track_sample_t ts;
        rc = kmc_track_sample(s, dyn_rmax, dyn_nbins, &ts, vh.data());
        if (rc) return die(s, rc, "track sample");
        f = fopen(dyn_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, dyn_path.c_str());
        const long long o = (long long)ts.origin_step;
        for (int c = 0; c < KMC_TRACK_CLASSES; ++c)
          fprintf(f, "msd %lld %lld %d %lld %lld %.17g %.17g\n", (long long)step, o, c, (long long)ts.n[c],
                  (long long)ts.n_clean[c], ts.sum_u2[c], ts.sum_u2_clean[c]);
        fprintf(f, "surv %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)step, o, (long long)ts.rl0,
                (long long)ts.rl_now, (long long)ts.rl_kept, (long long)ts.cis0, (long long)ts.cis_now,
                (long long)ts.cis_kept);
        for (int c = 0; c < KMC_TRACK_CLASSES; ++c)
          for (int k = 0; k < dyn_nbins; ++k)
            if (vh[(size_t)c * dyn_nbins + k])
              fprintf(f, "vh %lld %d %d %lld\n", (long long)step, c, k, (long long)vh[(size_t)c * dyn_nbins + k]);
        fclose(f);
      }
      if (!prox_path.empty()) {
        kmc_prox_out px;
        std::vector<int64_t> sizes((size_t)prox_max_size + 1);
        rc = kmc_prox_clusters(s, prox_which, KMC_SK_ALL, nullptr, prox_eps, prox_min_pts, prox_max_size, 1, &px,
                               sizes.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc) return die(s, rc, "prox clusters");
        f = fopen(prox_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, prox_path.c_str());
        for (int k = 0; k <= prox_max_size; ++k)
          if (sizes[(size_t)k]) fprintf(f, "%lld %d %lld\n", (long long)step, k, (long long)sizes[(size_t)k]);
        const int64_t fields[] = {px.n_sel, px.n_core, px.n_border, px.n_noise, px.n_alone, px.n_clusters, px.n_multi,
                                  px.sum_nn, px.n_core_edges, px.n_pure, px.n_whole, px.n_bond_multi, px.n_bond_kept,
                                  px.max_size, px.max_label};
        fprintf(f, "%lld sum", (long long)step);
        for (int64_t x : fields) fprintf(f, " %lld", (long long)x);
        fputc('\n', f);
        fclose(f);
      }
      if (!reach_path.empty()) {
        const int nd = 16, na = 18;
        kmc_reach_out r;
        std::vector<int64_t> hd((size_t)3 * 2 * nd), harl((size_t)na * na), hacis((size_t)2 * na);
        rc = kmc_reach_census(s, nd, na, &r, hd.data(), harl.data(), hacis.data());
        if (rc) return die(s, rc, "reach census");
        f = fopen(reach_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, reach_path.c_str());
        for (int c = 0; c < 3; ++c)
          fprintf(f, "reach %lld %d %lld %lld\n", (long long)step, c, (long long)r.n_reach[c], (long long)r.n_reactive[c]);
        fprintf(f, "reachrl %lld %lld %lld %lld %lld %lld\n", (long long)step, (long long)r.rl_free_receptors,
                (long long)r.rl_free_sites, (long long)r.rl_receptors_in_reach, (long long)r.rl_sites_in_reach,
                (long long)r.rl_max_partners);
        for (int c = 0; c < 3; ++c)
          for (int x = 0; x < 2; ++x)
            for (int k = 0; k < nd; ++k)
              if (hd[(size_t)(c * 2 + x) * nd + k])
                fprintf(f, "rd %lld %d %d %d %lld\n", (long long)step, c, x, k, (long long)hd[(size_t)(c * 2 + x) * nd + k]);
        for (int i = 0; i < na; ++i)
          for (int j = 0; j < na; ++j)
            if (harl[(size_t)i * na + j])
              fprintf(f, "ra %lld %d %d %lld\n", (long long)step, i, j, (long long)harl[(size_t)i * na + j]);
        for (int c = 0; c < 2; ++c)
          for (int k = 0; k < na; ++k)
            if (hacis[(size_t)c * na + k])
              fprintf(f, "rc %lld %d %d %lld\n", (long long)step, c, k, (long long)hacis[(size_t)c * na + k]);
        fclose(f);
      }
      if (!enc_path.empty()) {
        kmc_enc_out k;
        std::vector<int64_t> dwell((size_t)KMC_ENC_HISTS * KMC_ENC_BINS), react((size_t)2 * KMC_ENC_BINS);
        rc = kmc_enc_sample(s, &k, dwell.data(), react.data());
        if (rc) return die(s, rc, "enc sample");
        f = fopen(enc_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, enc_path.c_str());
        const int64_t fields[] = {k.origin_step, k.last_step, k.n_updates, k.on_from_encounter, k.on_direct, k.n_opened,
                                  k.n_ended, k.exp_reach, k.exp_reactive, k.exp_free_receptor, k.n_overflow,
                                  k.occ_reach, k.occ_reactive, k.occ_free_receptor, k.n_censored_alive, k.every,
                                  k.slots};
        fprintf(f, "enc %lld", (long long)step);
        for (int64_t x : fields) fprintf(f, " %lld", (long long)x);
        fputc('\n', f);
        for (int r = 0; r < KMC_ENC_HISTS; ++r)
          for (int b = 0; b < KMC_ENC_BINS; ++b)
            if (dwell[(size_t)r * KMC_ENC_BINS + b])
              fprintf(f, "dwell %lld %d %d %lld\n", (long long)step, r, b, (long long)dwell[(size_t)r * KMC_ENC_BINS + b]);
        for (int r = 0; r < 2; ++r)
          for (int b = 0; b < KMC_ENC_BINS; ++b)
            if (react[(size_t)r * KMC_ENC_BINS + b])
              fprintf(f, "react %lld %d %d %lld\n", (long long)step, r, b, (long long)react[(size_t)r * KMC_ENC_BINS + b]);
        fclose(f);
      }
      if (!kin_path.empty()) {
        kmc_kin_out k;
        rc = kmc_kin_sample(s, &k, life.data());
        if (rc) return die(s, rc, "kinetics sample");
        f = fopen(kin_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, kin_path.c_str());
        const int64_t fields[] = {k.origin_step, k.n_updates, k.rl_on, k.rl_off, k.rl_swap, k.cis_on, k.cis_off_mono,
                                  k.cis_off_cx, k.cis_swap, k.exp_rl, k.exp_mono, k.exp_cx, k.exp_free_receptor,
                                  k.exp_free_site, k.occ_rl, k.occ_mono, k.occ_cx, k.occ_free_receptor,
                                  k.occ_free_site, k.n_rl_censored_alive, k.n_cis_censored_alive};
        fprintf(f, "kin %lld", (long long)step);
        for (int64_t x : fields) fprintf(f, " %lld", (long long)x);
        fputc('\n', f);
        for (int r = 0; r < KMC_KIN_HISTS; ++r)
          for (int b = 0; b < KMC_KIN_BINS; ++b)
            if (life[(size_t)r * KMC_KIN_BINS + b])
              fprintf(f, "life %lld %d %d %lld\n", (long long)step, r, b, (long long)life[(size_t)r * KMC_KIN_BINS + b]);
        fclose(f);
      }
      if (!cf_path.empty()) {
        const size_t n1 = (size_t)cf_smax + 1;
        std::vector<int64_t> merge(n1 * n1), frag(n1 * n1), mp(KMC_CF_PIECES), fp(KMC_CF_PIECES), prod(n1), par(n1),
            ns(n1), expo(n1);
        kmc_cf_tables t;
        std::memset(&t, 0, sizeof t);
        t.merge = merge.data();
        t.frag = frag.data();
        t.merge_pieces = mp.data();
        t.frag_pieces = fp.data();
        t.merge_product = prod.data();
        t.frag_parent = par.data();
        t.n_s = ns.data();
        t.expo = expo.data();
        kmc_cf_out k;
        rc = kmc_cf_sample(s, &k, &t);
        if (rc) return die(s, rc, "growth sample");
        f = fopen(cf_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, cf_path.c_str());
        const int64_t fields[] = {k.origin_step, k.n_updates, k.max_size, k.formed_rl, k.formed_cis, k.broken_rl,
                                  k.broken_cis, k.n_cores, k.n_clusters, k.cycles_closed, k.cycles_opened,
                                  k.max_cluster};
        fprintf(f, "cf %lld", (long long)step);
        for (int64_t x : fields) fprintf(f, " %lld", (long long)x);
        fputc('\n', f);
        for (int pass = 0; pass < 2; ++pass) {
          const std::vector<int64_t>& tab = pass ? frag : merge;
          for (size_t a = 1; a < n1; ++a)
            for (size_t b = a; b < n1; ++b)
              if (tab[a * n1 + b])
                fprintf(f, "%s %lld %zu %zu %lld\n", pass ? "frag" : "merge", (long long)step, a, b,
                        (long long)tab[a * n1 + b]);
        }
        for (int q = 0; q < KMC_CF_PIECES; ++q)
          if (mp[(size_t)q] || fp[(size_t)q])
            fprintf(f, "pieces %lld %d %lld %lld\n", (long long)step, q, (long long)mp[(size_t)q], (long long)fp[(size_t)q]);
        for (size_t q = 1; q < n1; ++q)
          if (ns[q] || expo[q] || prod[q] || par[q])
            fprintf(f, "sizes %lld %zu %lld %lld %lld %lld\n", (long long)step, q, (long long)ns[q], (long long)expo[q],
                    (long long)prod[q], (long long)par[q]);
        fclose(f);
      }
      if (!lag_path.empty()) {
        kmc_lag_out k;
        std::vector<kmc_lag_cell> table((size_t)KMC_LAG_MAX_ROWS * KMC_LAG_CLASSES);
        int64_t n_pairs[KMC_LAG_MAX_ROWS];
        rc = kmc_lag_sample(s, &k, table.data(), n_pairs);
        if (rc) return die(s, rc, "lag sample");
        f = fopen(lag_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, lag_path.c_str());
        fprintf(f, "lag %lld %lld %lld %d %d %d %lld %lld %lld %lld\n", (long long)step, (long long)k.origin_step,
                (long long)k.n_updates, k.cfg.every, k.cfg.levels, k.cfg.slots, (long long)k.J, (long long)k.F,
                (long long)k.BX, (long long)k.BY);
        const int P = k.cfg.slots;
        for (int r = 0; r < (int)k.rows; ++r) {
          const int lv = r < P ? 0 : 1 + (r - P) / (P / 2);
          const int64_t lag = (int64_t)(r < P ? r + 1 : P / 2 + 1 + (r - P) % (P / 2)) << lv;
          for (int c = 0; c < KMC_LAG_CLASSES; ++c) {
            const kmc_lag_cell& w = table[(size_t)r * KMC_LAG_CLASSES + c];
            if (!(w.n_all || w.n_far)) continue;
            fprintf(f, "cell %lld %lld %d %lld %d %lld %lld %lld %lld %s %s %s\n", (long long)step,
                    (long long)k.origin_step, r, (long long)lag, c, (long long)n_pairs[r], (long long)w.n_all,
                    (long long)w.n_clean, (long long)w.n_far, dec128(w.m2_all).c_str(), dec128(w.m2_clean).c_str(),
                    dec128(w.m4_clean).c_str());
          }
        }
        fclose(f);
      }
      if (!rot_path.empty()) {
        kmc_rot_out k;
        std::vector<kmc_rot_cell> table((size_t)KMC_LAG_MAX_ROWS * KMC_LAG_CLASSES * KMC_ROT_VECS);
        int64_t n_pairs[KMC_LAG_MAX_ROWS];
        rc = kmc_rot_sample(s, &k, table.data(), n_pairs);
        if (rc) return die(s, rc, "rot sample");
        f = fopen(rot_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, rot_path.c_str());
        fprintf(f, "rot %lld %lld %lld %d %d %d\n", (long long)step, (long long)k.origin_step, (long long)k.n_updates,
                k.cfg.every, k.cfg.levels, k.cfg.slots);
        const int P = k.cfg.slots;
        for (int r = 0; r < (int)k.rows; ++r) {
          const int lv = r < P ? 0 : 1 + (r - P) / (P / 2);
          const int64_t lag = (int64_t)(r < P ? r + 1 : P / 2 + 1 + (r - P) % (P / 2)) << lv;
          for (int c = 0; c < KMC_LAG_CLASSES * KMC_ROT_VECS; ++c) {
            const kmc_rot_cell& w = table[(size_t)r * KMC_LAG_CLASSES * KMC_ROT_VECS + c];
            if (!w.n_all) continue;
            fprintf(f, "cell %lld %lld %d %lld %d %d %lld %lld %lld %s %s %s\n", (long long)step,
                    (long long)k.origin_step, r, (long long)lag, c / KMC_ROT_VECS, c % KMC_ROT_VECS,
                    (long long)n_pairs[r], (long long)w.n_all, (long long)w.n_clean, dec128(w.s1_all).c_str(),
                    dec128(w.s1_clean).c_str(), dec128(w.s2_clean).c_str());
          }
        }
        fclose(f);
      }
      if (!pose_path.empty()) {
        kmc_pose_out k;
        std::vector<int64_t> bins((size_t)KMC_POSE_CLASSES * pose_nz * pose_nc);
        rc = kmc_ligand_pose(s, pose_nz, pose_nc, bins.data(), &k);
        if (rc) return die(s, rc, "pose");
        f = fopen(pose_path.c_str(), "ab");
        if (!f) return die(s, KMC_ERR_IO, pose_path.c_str());
        fprintf(f, "pose %lld %d %d %lld", (long long)step, pose_nz, pose_nc, (long long)k.n_bad);
        for (int c = 0; c < KMC_POSE_CLASSES; ++c) fprintf(f, " %lld", (long long)k.chi_pos[c]);
        for (int c = 0; c < KMC_POSE_CLASSES; ++c) fprintf(f, " %lld", (long long)k.chi_neg[c]);
        fputc('\n', f);
        for (size_t b = 0; b < bins.size(); ++b)
          if (bins[b])
            fprintf(f, "bin %lld %zu %zu %zu %lld\n", (long long)step, b / ((size_t)pose_nz * pose_nc),
                    b / pose_nc % pose_nz, b % pose_nc, (long long)bins[b]);
        fclose(f);
      }
    }
  }
  kmc_destroy(s);
  return 0;
}
