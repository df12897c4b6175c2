// kmc_io.cpp — host-side formats and initial configurations of libkmc.
//
//  * position.cpt reader (main.cpp:226-270) and writer (main.cpp:2206-2244),
//    byte-compatible with the reference (pinned by tests against files the
//    reference itself wrote, tests/golden/*.cpt.gz);
//  * the bond.dat line (main.cpp:2247-2253);
//  * random placement with the reference's rules (main.cpp:281-447) drawn from
//    the keyed Philox stream, O(N) through a hash grid so 1e6-1e7-particle
//    boxes are reachable (the reference's goto sampler is O(N^2));
//  * state validation: bond-link consistency and the rigid-body extent bound
//    the device cell list relies on.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kmc.h"
#include "kmc_bodydyn.h"
#include "kmc_bondorder.h"
#include "kmc_coag.h"
#include "kmc_encounter.h"
#include "kmc_host.h"
#include "kmc_kinetics.h"
#include "kmc_lagcorr.h"
#include "kmc_orient.h"
#include "kmc_math.h"
#include "kmc_pairdyn.h"
#include "kmc_params_check.h"
#include "kmc_philox.h"
#include "kmc_proximity.h"
#include "kmc_rings.h"
#include "kmc_state_hash.h"
#include "kmc_structure.h"

namespace {

inline size_t RA(int na, int j, int k, int c, int i) { return (size_t)((((j - 1) * 4 + (k - 1)) * 3) + c) * na + i; }
inline size_t RB(int nb, int j, int k, int c, int i) { return (size_t)((((j - 1) * 2 + (k - 1)) * 3) + c) * nb + i; }

struct Tok {
  FILE* f;
  char buf[128];
  bool next(std::string* err) {
    int c;
    do {
      c = fgetc(f);
    } while (c == ' ' || c == '\n' || c == '\t' || c == '\r');
    if (c == EOF) {
      *err = "unexpected end of file";
      return false;
    }
    int n = 0;
    while (c != EOF && c != ' ' && c != '\n' && c != '\t' && c != '\r') {
      if (n < 127) buf[n++] = (char)c;
      c = fgetc(f);
    }
    buf[n] = 0;
    return true;
  }
  bool f64(double* out, std::string* err) {
    if (!next(err)) return false;
    char* e = nullptr;
    errno = 0;
    *out = strtod(buf, &e);  // istream >> double: strtod in the C locale
    if (e == buf || *e) {
      *err = std::string("bad number '") + buf + "'";
      return false;
    }
    return true;
  }
  bool i32(int32_t* out, std::string* err) {
    if (!next(err)) return false;
    char* e = nullptr;
    long v = strtol(buf, &e, 10);
    if (e == buf || *e) {
      *err = std::string("bad integer '") + buf + "'";
      return false;
    }
    *out = (int32_t)v;
    return true;
  }
};

}  // namespace

namespace kmch_host {

int load_cpt(const kmc_params* p, const char* path, kmc_state_view* v, std::string* err) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    *err = std::string("cannot open ") + path;
    return KMC_ERR_IO;
  }
  Tok t{f, {0}};
  const int na = p->n_a, nb = p->n_b;
  int rc = KMC_OK;
  for (int i = 0; i < na && rc == KMC_OK; ++i) {
    for (int j = 1; j <= 4 && rc == KMC_OK; ++j)
      for (int k = 1; k <= 4 && rc == KMC_OK; ++k)
        for (int c = 0; c < 3; ++c)
          if (!t.f64(&v->ra[RA(na, j, k, c, i)], err)) {
            rc = KMC_ERR_FORMAT;
            break;
          }
    for (int q = 0; q < 5 && rc == KMC_OK; ++q)  // status2 status3 nei2 nei4 nei3
      if (!t.i32(&v->a_int[(size_t)q * na + i], err)) rc = KMC_ERR_FORMAT;
  }
  for (int i = 0; i < nb && rc == KMC_OK; ++i)
    for (int j = 1; j <= 4 && rc == KMC_OK; ++j) {
      for (int k = 1; k <= 2 && rc == KMC_OK; ++k)
        for (int c = 0; c < 3; ++c)
          if (!t.f64(&v->rb[RB(nb, j, k, c, i)], err)) {
            rc = KMC_ERR_FORMAT;
            break;
          }
      if (rc == KMC_OK && !t.i32(&v->b_int[(size_t)(j - 1) * nb + i], err)) rc = KMC_ERR_FORMAT;
      if (rc == KMC_OK && !t.i32(&v->b_int[(size_t)(4 + j - 1) * nb + i], err)) rc = KMC_ERR_FORMAT;
    }
  for (int q = 0; q < 5 && rc == KMC_OK; ++q)
    if (!t.i32(&v->counters[q], err)) rc = KMC_ERR_FORMAT;
  int32_t step = 0;
  if (rc == KMC_OK && !t.i32(&step, err)) rc = KMC_ERR_FORMAT;
  fclose(f);
  if (rc == KMC_OK) v->step = step;  // the run continues at step+1 (main.cpp:267)
  return rc;
}

int write_cpt(const kmc_params* p, const kmc_state_view* v, const char* path, std::string* err) {
  FILE* f = fopen(path, "wb");
  if (!f) {
    *err = std::string("cannot open ") + path;
    return KMC_ERR_IO;
  }
  const int na = p->n_a, nb = p->n_b;
  // fixed, setprecision(3), setw(10) per coordinate; setw(8) per int
  for (int i = 0; i < na; ++i) {
    for (int j = 1; j <= 4; ++j)
      for (int k = 1; k <= 4; ++k)
        fprintf(f, "%10.3f%10.3f%10.3f\n", v->ra[RA(na, j, k, 0, i)], v->ra[RA(na, j, k, 1, i)], v->ra[RA(na, j, k, 2, i)]);
    fprintf(f, "%8d%8d%8d%8d%8d\n", v->a_int[0 * (size_t)na + i], v->a_int[1 * (size_t)na + i],
            v->a_int[2 * (size_t)na + i], v->a_int[3 * (size_t)na + i], v->a_int[4 * (size_t)na + i]);
  }
  for (int i = 0; i < nb; ++i)
    for (int j = 1; j <= 4; ++j) {
      for (int k = 1; k <= 2; ++k)
        fprintf(f, "%10.3f%10.3f%10.3f\n", v->rb[RB(nb, j, k, 0, i)], v->rb[RB(nb, j, k, 1, i)], v->rb[RB(nb, j, k, 2, i)]);
      fprintf(f, "%8d%8d\n", v->b_int[(size_t)(j - 1) * nb + i], v->b_int[(size_t)(4 + j - 1) * nb + i]);
    }
  for (int q = 0; q < 5; ++q) fprintf(f, "%d\n", v->counters[q]);
  fprintf(f, "%lld\n", (long long)v->step);
  if (fclose(f) != 0) {
    *err = "write failed";
    return KMC_ERR_IO;
  }
  return KMC_OK;
}

// bond-link consistency (what every reference step maintains) and the
// extent bound of the 130 Å cell list (kmc_kernels.hip)
int validate(const kmc_params* p, const kmc_state_view* v, std::string* err) {
  if (const char* bad = kmcp::check_params(p)) {
    *err = std::string("parameter outside the accepted envelope: ") + bad;
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, nb = p->n_b, n = na + nb;
  char msg[256];
  for (int i = 0; i < na; ++i) {
    int st2 = v->a_int[0 * (size_t)na + i], st3 = v->a_int[1 * (size_t)na + i];
    int n2 = v->a_int[2 * (size_t)na + i], n4 = v->a_int[3 * (size_t)na + i], n3 = v->a_int[4 * (size_t)na + i];
    bool ok = (st2 == 0 || st2 == 1) && (st3 == 0 || st3 == 1) && (st2 == (n2 != 0)) && (st3 == (n3 != 0));
    if (ok && n2) {
      ok = n2 > na && n2 <= n && n4 >= 2 && n4 <= 4;
      if (ok) {
        int b = n2 - 1 - na;
        ok = v->b_int[(size_t)(4 + n4 - 1) * nb + b] == i + 1 && v->b_int[(size_t)(n4 - 1) * nb + b] == 1;
      }
    } else if (ok) {
      ok = n4 == 0;
    }
    if (ok && n3) ok = n3 >= 1 && n3 <= na && n3 != i + 1 && v->a_int[4 * (size_t)na + (n3 - 1)] == i + 1;
    if (!ok) {
      snprintf(msg, sizeof msg, "inconsistent bond state at receptor %d", i + 1);
      *err = msg;
      return KMC_ERR_STATE;
    }
  }
  for (int b = 0; b < nb; ++b) {
    if (v->b_int[0 * (size_t)nb + b] != 0 || v->b_int[4 * (size_t)nb + b] != 0) {
      snprintf(msg, sizeof msg, "ligand %d: site 1 is the virtual centre and cannot bind", na + b + 1);
      *err = msg;
      return KMC_ERR_STATE;
    }
    for (int j = 2; j <= 4; ++j) {
      int st = v->b_int[(size_t)(j - 1) * nb + b], ne = v->b_int[(size_t)(4 + j - 1) * nb + b];
      bool ok = (st == (ne != 0)) && (st == 0 || st == 1);
      if (ok && ne) ok = ne >= 1 && ne <= na && v->a_int[2 * (size_t)na + (ne - 1)] == na + b + 1 &&
                         v->a_int[3 * (size_t)na + (ne - 1)] == j;
      if (!ok) {
        snprintf(msg, sizeof msg, "inconsistent bond state at ligand %d site %d", na + b + 1, j);
        *err = msg;
        return KMC_ERR_STATE;
      }
    }
  }
  // extents: receptor beads within 0.3 Å (domain axis) / 20.3 Å (sites) of
  // [1][1] in xy; ligand [1][2] ≤ 30.3, subunit centres ≤ 35, sites ≤ 65 Å
  for (int i = 0; i < na; ++i) {
    double x0 = v->ra[RA(na, 1, 1, 0, i)], y0 = v->ra[RA(na, 1, 1, 1, i)];
    for (int j = 1; j <= 4; ++j)
      for (int k = 1; k <= 4; ++k) {
        double dx = v->ra[RA(na, j, k, 0, i)] - x0, dy = v->ra[RA(na, j, k, 1, i)] - y0;
        double lim = (k == 1 || k == 4) ? 0.3 : 20.3;
        if (!(dx * dx + dy * dy <= lim * lim)) {
          snprintf(msg, sizeof msg, "receptor %d bead [%d][%d] outside the rigid-body extent bound", i + 1, j, k);
          *err = msg;
          return KMC_ERR_GEOMETRY;
        }
      }
  }
  for (int b = 0; b < nb; ++b) {
    double x0 = v->rb[RB(nb, 1, 1, 0, b)], y0 = v->rb[RB(nb, 1, 1, 1, b)];
    for (int j = 1; j <= 4; ++j)
      for (int k = 1; k <= 2; ++k) {
        double dx = v->rb[RB(nb, j, k, 0, b)] - x0, dy = v->rb[RB(nb, j, k, 1, b)] - y0;
        double lim = j == 1 ? (k == 1 ? 0.3 : 30.3) : (k == 1 ? 35.0 : 65.0);
        if (!(dx * dx + dy * dy <= lim * lim)) {
          snprintf(msg, sizeof msg, "ligand %d bead [%d][%d] outside the rigid-body extent bound", na + b + 1, j, k);
          *err = msg;
          return KMC_ERR_GEOMETRY;
        }
      }
  }
  return KMC_OK;
}

// derived bond counters of a state: rl, mono-cis pairs, complex-cis pairs
void derived_counts(const kmc_params* p, const kmc_state_view* v, int* rl, int* mono, int* cis) {
  const int na = p->n_a;
  *rl = *mono = *cis = 0;
  for (int i = 0; i < na; ++i) {
    *rl += v->a_int[0 * (size_t)na + i];
    if (v->a_int[1 * (size_t)na + i] == 1) {
      int q = v->a_int[4 * (size_t)na + i] - 1;
      if (i < q) {
        if (v->a_int[0 * (size_t)na + i] == 0 && v->a_int[0 * (size_t)na + q] == 0) ++*mono;
        else ++*cis;
      }
    }
  }
}

// ------------------------------------------------------------------ placement
// main.cpp:281-447 with keyed draws: identical to the oracle's keyed
// placement (a hash grid only prunes pairs that cannot reject).
struct Grid {
  double cs, x0, y0;
  int nx, ny;
  std::vector<int> head, next;  // linked lists of item indices
  Grid(double box_x, double box_y, double cell, int cap) {
    cs = cell;
    x0 = -box_x / 2 - 2 * cell;
    y0 = -box_y / 2 - std::max(box_x, box_y) / 2 - 2 * cell;  // ligand y range uses box_x (sic)
    nx = (int)((box_x + 4 * cell) / cell) + 1;
    ny = (int)((box_y + std::max(box_x, box_y) + 4 * cell) / cell) + 1;
    head.assign((size_t)nx * ny, -1);
    next.assign(cap, -1);
  }
  int cx(double x) const { return std::min(std::max((int)std::floor((x - x0) / cs), 0), nx - 1); }
  int cy(double y) const { return std::min(std::max((int)std::floor((y - y0) / cs), 0), ny - 1); }
  void add(int item, double x, double y) {
    size_t c = (size_t)cy(y) * nx + cx(x);
    next[item] = head[c];
    head[c] = item;
  }
  template <typename F>
  bool any_near(double x, double y, F f) const {
    int X = cx(x), Y = cy(y);
    for (int yy = Y - 1; yy <= Y + 1; ++yy)
      for (int xx = X - 1; xx <= X + 1; ++xx) {
        if (xx < 0 || yy < 0 || xx >= nx || yy >= ny) continue;
        for (int it = head[(size_t)yy * nx + xx]; it >= 0; it = next[it])
          if (f(it)) return true;
      }
    return false;
  }
};

static void euler(double theta, double phi, double psai, double t[3][3]) {
  double cth = kmcm::cos(theta), sth = kmcm::sin(theta);
  double cph = kmcm::cos(phi), sph = kmcm::sin(phi);
  double cps = kmcm::cos(psai), sps = kmcm::sin(psai);
  t[0][0] = cps * cph - cth * sph * sps;
  t[0][1] = -sps * cph - cth * sph * cps;
  t[0][2] = sth * sph;
  t[1][0] = cps * sph + cth * cph * sps;
  t[1][1] = -sps * sph + cth * cph * cps;
  t[1][2] = -sth * cph;
  t[2][0] = sps * sth;
  t[2][1] = cps * sth;
  t[2][2] = cth;
}

int init_random(const kmc_params* p, kmc_state_view* v, std::string* err) {
  const int na = p->n_a, nb = p->n_b;
  const double RAd = p->ra_radius, RBd = p->rb_radius, pai = p->pai;
  const kmcr::Key key = kmcr::make_key(p->seed, p->replica);
  const int64_t MAXATT = 100000000;
  auto draw = [&](int prot1, uint32_t att, int slot) {
    double u0, u1;
    kmcr::uniform2(key, kmcr::DOM_INIT, (uint32_t)(prot1 - 1), att, 0, (uint32_t)(slot >> 1), &u0, &u1);
    return (slot & 1) ? u1 : u0;
  };
  const uint32_t ORIENT = 0xffffffffu;
  const double S3 = kmcm::sqrt_(3.0);
  // receptors: 2-D rejection vs earlier receptors (dist <= 2 R_A)
  Grid ga(p->box_x, p->box_y, 130.0, std::max(na, 1));
  std::vector<double> ax(na), ay(na);
  for (int i = 0; i < na; ++i) {
    double ti = 0, tj = 0;
    for (uint32_t att = 0;; ++att) {
      if (att >= MAXATT) {
        *err = "receptor placement failed";
        return KMC_ERR_PLACEMENT;
      }
      ti = draw(i + 1, att, 0) * p->box_x - p->box_x / 2;
      tj = draw(i + 1, att, 1) * p->box_y - p->box_y / 2;
      bool bad = ga.any_near(ti, tj, [&](int j) {
        double d = kmcm::sqrt_((ti - ax[j]) * (ti - ax[j]) + (tj - ay[j]) * (tj - ay[j]));
        return d <= RAd + RAd;
      });
      if (!bad) break;
    }
    ax[i] = ti;
    ay[i] = tj;
    ga.add(i, ti, tj);
    double tk = 0;
    double t[3][3];
    euler(0, 0, (2 * draw(i + 1, ORIENT, 0) - 1) * pai, t);
    for (int j = 1; j <= 4; ++j) {
      double cx = ti, cy = tj, cz = tk + (j * 2 - 2) * RAd;
      v->ra[RA(na, j, 1, 0, i)] = cx;
      v->ra[RA(na, j, 1, 1, i)] = cy;
      v->ra[RA(na, j, 1, 2, i)] = cz;
      double ox[5] = {0, 0, ti + RAd, ti - RAd, ti};
      double oy[5] = {0, 0, tj, tj, tj};
      double oz[5] = {0, 0, tk + (j * 2 - 2) * RAd, tk + (j * 2 - 2) * RAd, tk + (j * 2 - 1) * RAd};
      for (int k = 2; k <= 4; ++k) {
        v->ra[RA(na, j, k, 0, i)] = t[0][0] * (ox[k] - cx) + t[0][1] * (oy[k] - cy) + t[0][2] * (oz[k] - cz) + cx;
        v->ra[RA(na, j, k, 1, i)] = t[1][0] * (ox[k] - cx) + t[1][1] * (oy[k] - cy) + t[1][2] * (oz[k] - cz) + cy;
        v->ra[RA(na, j, k, 2, i)] = t[2][0] * (ox[k] - cx) + t[2][1] * (oy[k] - cy) + t[2][2] * (oz[k] - cz) + cz;
      }
    }
    for (int q = 0; q < 5; ++q) v->a_int[(size_t)q * na + i] = 0;
  }
  // ligands: 3-D rejection vs receptor domain centres and earlier ligands
  Grid gb(p->box_x, p->box_y, 130.0, std::max(nb, 1));
  std::vector<double> bx(nb), by(nb), bz(nb);
  for (int b = 0; b < nb; ++b) {
    int prot = na + b + 1;
    double ti = 0, tj = 0, tk = 0;
    for (uint32_t att = 0;; ++att) {
      if (att >= MAXATT) {
        *err = "ligand placement failed";
        return KMC_ERR_PLACEMENT;
      }
      ti = draw(prot, att, 0) * p->box_x - p->box_x / 2;
      tj = draw(prot, att, 1) * p->box_y - p->box_x / 2;  // sic: cell_range_x (main.cpp:358)
      tk = draw(prot, att, 2) * p->box_z;
      bool bad = ga.any_near(ti, tj, [&](int j) {
        for (int k = 1; k <= 4; ++k) {
          double X = v->ra[RA(na, k, 1, 0, j)], Y = v->ra[RA(na, k, 1, 1, j)], Z = v->ra[RA(na, k, 1, 2, j)];
          double d = kmcm::sqrt_((ti - X) * (ti - X) + (tj - Y) * (tj - Y) + (tk - Z) * (tk - Z));
          if (d <= RAd + RBd * 2 / S3 + RBd) return true;
        }
        return false;
      });
      if (!bad)
        bad = gb.any_near(ti, tj, [&](int j) {
          double d = kmcm::sqrt_((ti - bx[j]) * (ti - bx[j]) + (tj - by[j]) * (tj - by[j]) + (tk - bz[j]) * (tk - bz[j]));
          return d <= RBd * 2 / S3 + RBd * 2 / S3 + 2 * RBd;
        });
      if (!bad) break;
    }
    bx[b] = ti;
    by[b] = tj;
    bz[b] = tk;
    gb.add(b, ti, tj);
    // template R_x_0 (main.cpp:390-412), index [j][k]
    double ox[5][3] = {{0}}, oy[5][3] = {{0}}, oz[5][3] = {{0}};
    ox[1][2] = ti; oy[1][2] = tj; oz[1][2] = tk + RBd;
    ox[2][1] = ti; oy[2][1] = tj + RBd * 2 / S3; oz[2][1] = tk;
    ox[3][1] = ti - RBd; oy[3][1] = tj - RBd / S3; oz[3][1] = tk;
    ox[4][1] = ti + RBd; oy[4][1] = tj - RBd / S3; oz[4][1] = tk;
    ox[2][2] = ti; oy[2][2] = tj + RBd * (2 / S3 + 1); oz[2][2] = tk;
    ox[3][2] = ti - RBd * (S3 / 2 + 1); oy[3][2] = tj - RBd / S3 - RBd / 2; oz[3][2] = tk;
    ox[4][2] = ti + RBd * (S3 / 2 + 1); oy[4][2] = tj - RBd / S3 - RBd / 2; oz[4][2] = tk;
    double th = (2 * draw(prot, ORIENT, 0) - 1) * pai;
    double ph = (2 * draw(prot, ORIENT, 1) - 1) * pai;
    double ps = (2 * draw(prot, ORIENT, 2) - 1) * pai;
    double t[3][3];
    euler(th, ph, ps, t);
    v->rb[RB(nb, 1, 1, 0, b)] = ti;
    v->rb[RB(nb, 1, 1, 1, b)] = tj;
    v->rb[RB(nb, 1, 1, 2, b)] = tk;
    for (int j = 1; j <= 4; ++j)
      for (int k = 1; k <= 2; ++k) {
        if (j == 1 && k == 1) continue;
        v->rb[RB(nb, j, k, 0, b)] = t[0][0] * (ox[j][k] - ti) + t[0][1] * (oy[j][k] - tj) + t[0][2] * (oz[j][k] - tk) + ti;
        v->rb[RB(nb, j, k, 1, b)] = t[1][0] * (ox[j][k] - ti) + t[1][1] * (oy[j][k] - tj) + t[1][2] * (oz[j][k] - tk) + tj;
        v->rb[RB(nb, j, k, 2, b)] = t[2][0] * (ox[j][k] - ti) + t[2][1] * (oy[j][k] - tj) + t[2][2] * (oz[j][k] - tk) + tk;
      }
    for (int q = 0; q < 8; ++q) v->b_int[(size_t)q * nb + b] = 0;
  }
  for (int q = 0; q < 5; ++q) v->counters[q] = 0;
  v->step = 0;
  return KMC_OK;
}

// ---------------------------------------------------------------- exact checkpoint
// Layout (little-endian): "KMCSTAT1", u32 version, i32 n_a, i32 n_b,
// u32 replica, u64 seed, i64 step, i32 counters[5], i32 reserved, then the
// view's arrays in their SoA layout (ra, rb as f64; a_int, b_int as i32), then
// an FNV-1a-64 of every preceding byte.
namespace {
const char kStateMagic[8] = {'K', 'M', 'C', 'S', 'T', 'A', 'T', '1'};
struct StateHeader {
  char magic[8];
  uint32_t version;
  int32_t n_a, n_b;
  uint32_t replica;
  uint64_t seed;
  int64_t step;
  int32_t counters[5];
  int32_t reserved;
};
static_assert(sizeof(StateHeader) == 64, "state header layout");

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void add(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
};
}  // namespace

int save_state(const kmc_params* p, const kmc_state_view* v, const char* path, std::string* err) {
  const size_t NA = (size_t)p->n_a, NB = (size_t)p->n_b;
  StateHeader hd;
  std::memset(&hd, 0, sizeof hd);
  std::memcpy(hd.magic, kStateMagic, 8);
  hd.version = 1;
  hd.n_a = p->n_a;
  hd.n_b = p->n_b;
  hd.replica = p->replica;
  hd.seed = p->seed;
  hd.step = v->step;
  for (int k = 0; k < 5; ++k) hd.counters[k] = v->counters[k];
  FILE* f = fopen(path, "wb");
  if (!f) {
    *err = std::string("cannot write ") + path;
    return KMC_ERR_IO;
  }
  Fnv h;
  auto put = [&](const void* d, size_t n) {
    h.add(d, n);
    return fwrite(d, 1, n, f) == n;
  };
  bool ok = put(&hd, sizeof hd) && put(v->ra, sizeof(double) * 48 * NA) && put(v->rb, sizeof(double) * 24 * NB) &&
            put(v->a_int, sizeof(int32_t) * 5 * NA) && put(v->b_int, sizeof(int32_t) * 8 * NB);
  uint64_t tr = h.h;
  ok = ok && fwrite(&tr, 1, sizeof tr, f) == sizeof tr;
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    *err = std::string("write failed: ") + path;
    return KMC_ERR_IO;
  }
  return KMC_OK;
}

int load_state(const kmc_params* p, const char* path, kmc_state_view* v, std::string* err) {
  const size_t NA = (size_t)p->n_a, NB = (size_t)p->n_b;
  FILE* f = fopen(path, "rb");
  if (!f) {
    *err = std::string("cannot open ") + path;
    return KMC_ERR_IO;
  }
  Fnv h;
  auto get = [&](void* d, size_t n) {
    if (fread(d, 1, n, f) != n) return false;
    h.add(d, n);
    return true;
  };
  StateHeader hd;
  int rc = KMC_OK;
  if (!get(&hd, sizeof hd) || std::memcmp(hd.magic, kStateMagic, 8) != 0 || hd.version != 1) {
    *err = std::string("not a KMCSTAT1 file: ") + path;
    rc = KMC_ERR_FORMAT;
  } else if (hd.n_a != p->n_a || hd.n_b != p->n_b || hd.seed != p->seed || hd.replica != p->replica) {
    *err = "state file is of another trajectory (n_a, n_b, seed or replica differ)";
    rc = KMC_ERR_ARG;
  } else if (!get(v->ra, sizeof(double) * 48 * NA) || !get(v->rb, sizeof(double) * 24 * NB) ||
             !get(v->a_int, sizeof(int32_t) * 5 * NA) || !get(v->b_int, sizeof(int32_t) * 8 * NB)) {
    *err = std::string("truncated state file: ") + path;
    rc = KMC_ERR_FORMAT;
  } else {
    uint64_t tr = 0, want = h.h;
    if (fread(&tr, 1, sizeof tr, f) != sizeof tr || tr != want) {
      *err = std::string("state file checksum mismatch: ") + path;
      rc = KMC_ERR_FORMAT;
    }
  }
  fclose(f);
  if (rc != KMC_OK) return rc;
  v->step = hd.step;
  for (int k = 0; k < 5; ++k) v->counters[k] = hd.counters[k];
  v->reserved = 0;
  return validate(p, v, err);
}

// The window of a decomposed trajectory (kmc_dd_set_state): its local
// numbering is monotone in the global one (receptors, then ligands: every
// order the step takes — unit keys, BFS roots, the greedy reactions — is then
// the global order restricted to the window), a global index fits an
// exchanged link (global index + 1 in an int32), and ownership is 0 or 1.
int dd_check(int32_t n, const int32_t* gid, const uint8_t* own, std::string* err) {
  if (n < 0 || (n > 0 && (!gid || !own))) return KMC_ERR_ARG;
  for (int32_t i = 0; i < n; ++i) {
    if (gid[i] < 0 || gid[i] >= INT32_MAX) {
      if (err) *err = "dd: global index out of range";
      return KMC_ERR_ARG;
    }
    if (i > 0 && gid[i] <= gid[i - 1]) {
      if (err) *err = "dd: global indices not increasing";
      return KMC_ERR_ARG;
    }
    if (own[i] > 1) {
      if (err) *err = "dd: ownership flag not 0 or 1";
      return KMC_ERR_ARG;
    }
  }
  return KMC_OK;
}

}  // namespace kmch_host

// ------------------------------------------------------------------ C ABI (host-only part)
extern "C" {

void kmc_params_default(kmc_params* p) {
  memset(p, 0, sizeof *p);
  p->n_a = 150;
  p->n_b = 50;
  p->time_step = 10;
  p->box_x = 5773;
  p->box_y = 5773;
  p->box_z = 1000;
  p->pai = 3.1415926;
  p->ra_radius = 20;
  p->ra_D = 1;
  p->ra_rot_D = 0.0174;
  p->rb_radius = 30;
  p->rb_D = 7.2614;
  p->rb_rot_D = 0.0061209;
  p->mono_cis_ass_rate = 0.000047;
  p->mono_cis_diss_rate = 0.000000000000112;
  p->cis_D = 0.5;
  p->cis_rot_D = 0.005;
  p->cis_ass_rate = 0.00096;
  p->cis_diss_rate = 0.000000000000112;
  p->bond_D = 0.5;
  p->bond_rot_D = 0.005;
  p->ass_rate = 0.04;
  p->diss_rate = 0.000000000000348;
  p->bond_dist_cutoff = 18;
  p->bond_thetapd_cutoff = 45;
  p->bond_thetaot_cutoff = 90;
  p->cis_thetaot_cutoff = 10;
  p->cis_dist_cutoff = 15;
  p->simu_step = 20000000;
  p->out_interval = 5000;
  p->seed = 1;
  p->replica = 0;
}

int kmc_format_bond_line(const kmc_params* p, const kmc_obs* o, char* buf, size_t n) {
  // setw(15) t, setw(5) rl, setw(5) mono, setw(10) cis, setw(10) bond,
  // setw(10) cluster_size (fixed, 3 decimals), setw(10) max complex
  (void)p;
  return snprintf(buf, n, "%15.3f%5d%5d%10d%10d%10.3f%10d\n", o->t, o->bond_num_rl, o->bond_num_mono_cis,
                  o->bond_num_cis, o->bond_num, o->cluster_size, o->protein_num_in_max_complex);
}

uint64_t kmc_state_hash(const kmc_params* p, const kmc_state_view* v) { return kmch::state_hash(p->n_a, p->n_b, v); }

// parameter.log, main.cpp:178-205 (default ostream float format = %g)
int kmc_host_write_parameter_log(const kmc_params* p, const char* path) {
  FILE* f = fopen(path, "wb");
  if (!f) return KMC_ERR_IO;
  auto L = [&](const char* k, double v) { fprintf(f, "%25s%15g\n", k, v); };
  fprintf(f, "%25s%15g%7g%7g\n\n", "box size: x y z", p->box_x, p->box_y, p->box_z);
  fprintf(f, "%25s%15d\n", "protein_A_tot_num", p->n_a);
  fprintf(f, "%25s%15d\n", "RB_A_tot_num", p->n_a * 4);
  fprintf(f, "%25s%15d\n", "protein_B_tot_num", p->n_b);
  fprintf(f, "%25s%15d\n\n", "RB_B_tot_num", p->n_b * 4);
  L("RB_A_D", p->ra_D);
  L("RB_A_rot_D", p->ra_rot_D);
  L("RB_B_D", p->rb_D);
  fprintf(f, "%25s%15g\n\n", "RB_B_rot_D", p->rb_rot_D);
  fprintf(f, "%25s\n", "R-L interaction:");
  L("bond_D", p->bond_D);
  L("bond_rot_D", p->bond_rot_D);
  L("Ass_Rate", p->ass_rate);
  fprintf(f, "%25s%15g\n\n", "Diss_Rate", p->diss_rate);
  fprintf(f, "%25s\n", "Cis interaction:");
  L("cis_D", p->cis_D);
  L("cis_rot_D", p->cis_rot_D);
  L("mono_cis_Ass_Rate", p->mono_cis_ass_rate);
  fprintf(f, "%25s%15g\n\n", "mono_cis_Diss_Rate", p->mono_cis_diss_rate);
  L("cis_Ass_Rate", p->cis_ass_rate);
  fprintf(f, "%25s%15g\n\n", "cis_Diss_Rate", p->cis_diss_rate);
  return fclose(f) == 0 ? KMC_OK : KMC_ERR_IO;
}

// test.gro frame, main.cpp:2258-2287 (appended): receptor domain centres and
// ligand subunit centres in nm, fixed with 3 decimals
int kmc_host_append_gro(const kmc_params* p, const kmc_state_view* v, const char* path) {
  FILE* f = fopen(path, "ab");
  if (!f) return KMC_ERR_IO;
  const int na = p->n_a, nb = p->n_b;
  fprintf(f, "Hello Gro!, t=%.3f\n", (double)(int)v->step * p->time_step);
  fprintf(f, "%d\n", na * 4 + nb * 3);
  for (int i = 0; i < na; ++i)
    for (int j = 1; j <= 4; ++j)
      fprintf(f, "%5dALA%7s%5d%8.3f%8.3f%8.3f\n", i + 1, "CA", i + 1, v->ra[RA(na, j, 1, 0, i)] / 10,
              v->ra[RA(na, j, 1, 1, i)] / 10, v->ra[RA(na, j, 1, 2, i)] / 10);
  for (int b = 0; b < nb; ++b)
    for (int j = 2; j <= 4; ++j)
      fprintf(f, "%5dLEU%7s%5d%8.3f%8.3f%8.3f\n", na + b + 1, "CA", na + b + 1, v->rb[RB(nb, j, 1, 0, b)] / 10,
              v->rb[RB(nb, j, 1, 1, b)] / 10, v->rb[RB(nb, j, 1, 2, b)] / 10);
  fprintf(f, "%8.3f%12.3f%12.3f\n", p->box_x / 10, p->box_y / 10, p->box_z / 10);
  return fclose(f) == 0 ? KMC_OK : KMC_ERR_IO;
}

// cluster.log block, main.cpp:2291-2305 (appended): for every ligand its BFS
// row (members in results[i][.] order, "  "-separated; empty for non-roots)
int kmc_host_append_cluster_log(const kmc_params* p, int64_t step, const int32_t* row_len, const int32_t* members,
                                const char* path) {
  FILE* f = fopen(path, "ab");
  if (!f) return KMC_ERR_IO;
  fprintf(f, "Hello Cluster!, t=%g\n", (double)(int)step * p->time_step);
  int64_t o = 0;
  for (int b = 0; b < p->n_b; ++b) {
    for (int t = 0; t < row_len[b]; ++t) fprintf(f, "%d  ", members[o++]);
    fputc('\n', f);
  }
  return fclose(f) == 0 ? KMC_OK : KMC_ERR_IO;
}

static thread_local std::string g_host_err;
const char* kmc_host_last_error(void) { return g_host_err.c_str(); }

int kmc_host_load_cpt(const kmc_params* p, const char* path, kmc_state_view* v) {
  return kmch_host::load_cpt(p, path, v, &g_host_err);
}
int kmc_host_write_cpt(const kmc_params* p, const kmc_state_view* v, const char* path) {
  return kmch_host::write_cpt(p, v, path, &g_host_err);
}
int kmc_host_init_random(const kmc_params* p, kmc_state_view* v) { return kmch_host::init_random(p, v, &g_host_err); }
int kmc_host_save_state(const kmc_params* p, const kmc_state_view* v, const char* path) {
  return kmch_host::save_state(p, v, path, &g_host_err);
}
int kmc_host_load_state(const kmc_params* p, const char* path, kmc_state_view* v) {
  return kmch_host::load_state(p, path, v, &g_host_err);
}
int kmc_host_validate(const kmc_params* p, const kmc_state_view* v) { return kmch_host::validate(p, v, &g_host_err); }
int kmc_host_check_params(const kmc_params* p) {
  const char* bad = kmcp::check_params(p);
  if (!bad) return KMC_OK;
  g_host_err = std::string("parameter outside the accepted envelope: ") + bad;
  return KMC_ERR_ARG;
}
int kmc_host_dd_check(int32_t n, const int32_t* gid, const uint8_t* own) {
  return kmch_host::dd_check(n, gid, own, &g_host_err);
}

// Components of the bond graph and their census (include/kmc.h), sequential:
// a breadth-first walk from every protein not yet labelled, in index order,
// so the walk's start is the component's smallest index — its label.
int kmc_host_census(const kmc_params* p, const kmc_state_view* v, int32_t* label, int32_t max_r, int32_t max_l,
                    int64_t* hist, kmc_census* out) {
  if (!p || !v || !out || !v->a_int || !v->b_int || p->n_a < 0 || p->n_b < 0 || max_r < 0 || max_l < 0) {
    g_host_err = "census: params, state and out are needed, max_r and max_l >= 0";
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, nb = p->n_b, n = na + nb;
  std::vector<int32_t> lab((size_t)n, 0), queue;
  queue.reserve((size_t)n);
  std::memset(out, 0, sizeof *out);
  if (hist) std::fill(hist, hist + ((size_t)max_r + 1) * ((size_t)max_l + 1), (int64_t)0);
  for (int r = 0; r < n; ++r) {
    if (lab[r]) continue;
    queue.clear();
    queue.push_back(r);
    lab[r] = r + 1;
    int nr = 0, nl = 0;
    for (size_t h = 0; h < queue.size(); ++h) {
      const int q = queue[h];
      int nei[3], m = 0;
      if (q < na) {
        ++nr;
        nei[m++] = v->a_int[2 * (size_t)na + q];
        nei[m++] = v->a_int[4 * (size_t)na + q];
      } else {
        ++nl;
        for (int j = 2; j <= 4; ++j) nei[m++] = v->b_int[(size_t)(4 + j - 1) * nb + (q - na)];
      }
      for (int e = 0; e < m; ++e) {
        if (nei[e] == 0) continue;
        if (nei[e] < 1 || nei[e] > n) {
          g_host_err = "census: a bond link of protein " + std::to_string(q + 1) + " leaves the state";
          return KMC_ERR_STATE;
        }
        if (!lab[nei[e] - 1]) {
          lab[nei[e] - 1] = r + 1;
          queue.push_back(nei[e] - 1);
        }
      }
    }
    const int size = nr + nl;
    out->n_components += 1;
    if (nl >= 1 && size > 1) {
      out->n_complexes += 1;
      out->proteins_in_complexes += size;
    }
    if (nl == 0 && nr == 2) out->n_cis_dimers += 1;
    if (size > out->max_size) {  // (components come in label order: the first of a size keeps the tie)
      out->max_size = size;
      out->max_receptors = nr;
      out->max_ligands = nl;
      out->max_label = r + 1;
    }
    if (hist) hist[(size_t)std::min(nr, (int)max_r) * ((size_t)max_l + 1) + std::min(nl, (int)max_l)] += 1;
  }
  if (label) std::copy(lab.begin(), lab.end(), label);
  return KMC_OK;
}

// Cluster geometry (include/kmc.h), sequential: a breadth-first walk from every
// protein not yet labelled, in index order — the start is the label, its image
// shift (0, 0), and a member takes its shift from the member that reached it;
// then every edge of the component is compared with the shifts (the spanning
// bits), and the moments are summed in 128-bit integers.
int kmc_host_cluster_geometry(const kmc_params* p, const kmc_state_view* v, int32_t* label, int32_t* shift,
                              uint8_t* span, int32_t max_size, kmc_geom_bin* table, kmc_geom* out) {
  if (!p || !v || !out || !v->a_int || !v->b_int || !v->ra || !v->rb || p->n_a < 0 || p->n_b < 0 || max_size < 2) {
    g_host_err = "cluster geometry: params, state and out are needed, max_size >= 2";
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, nb = p->n_b, n = na + nb;
  const double box[2] = {p->box_x, p->box_y};
  const long long B[2] = {(long long)kmcm::round_(p->box_x * 1024.0), (long long)kmcm::round_(p->box_y * 1024.0)};
  auto pos = [&](int q, int c) { return q < na ? v->ra[RA(na, 1, 1, c, q)] : v->rb[RB(nb, 1, 1, c, q - na)]; };
  auto edge = [&](int i, int j, int c) { return -(int)kmcm::round_((pos(j, c) - pos(i, c)) / box[c]); };
  auto links = [&](int q, int* nei) {
    int m = 0;
    if (q < na) {
      nei[m++] = v->a_int[2 * (size_t)na + q];
      nei[m++] = v->a_int[4 * (size_t)na + q];
    } else {
      for (int j = 2; j <= 4; ++j) nei[m++] = v->b_int[(size_t)(4 + j - 1) * nb + (q - na)];
    }
    return m;
  };
  typedef __int128 i128;
  auto put = [](kmc_i128* w, i128 x) {
    w->lo = (uint64_t)(unsigned __int128)x;
    w->hi = (int64_t)(x >> 64);
  };
  std::vector<int32_t> lab((size_t)n, 0), sx((size_t)n, 0), sy((size_t)n, 0), queue;
  std::vector<uint8_t> sp((size_t)n, 0);
  std::vector<i128> sum_m(table ? (size_t)max_size + 1 : 0, 0);
  queue.reserve((size_t)n);
  std::memset(out, 0, sizeof *out);
  if (table) std::memset(table, 0, sizeof(kmc_geom_bin) * ((size_t)max_size + 1));
  for (int r = 0; r < n; ++r) {
    if (lab[r]) continue;
    queue.clear();
    queue.push_back(r);
    lab[r] = r + 1;
    for (size_t h = 0; h < queue.size(); ++h) {
      const int q = queue[h];
      int nei[3];
      const int m = links(q, nei);
      for (int e = 0; e < m; ++e) {
        if (nei[e] == 0) continue;
        if (nei[e] < 1 || nei[e] > n) {
          g_host_err = "cluster geometry: a bond link of protein " + std::to_string(q + 1) + " leaves the state";
          return KMC_ERR_STATE;
        }
        const int j = nei[e] - 1;
        if (lab[j]) continue;
        lab[j] = r + 1;
        sx[j] = sx[q] + edge(q, j, 0);
        sy[j] = sy[q] + edge(q, j, 1);
        queue.push_back(j);
      }
    }
    int bits = 0;
    for (int q : queue) {
      int nei[3];
      const int m = links(q, nei);
      for (int e = 0; e < m; ++e) {
        if (nei[e] == 0) continue;
        const int j = nei[e] - 1;
        if (sx[j] - sx[q] != edge(q, j, 0)) bits |= KMC_SPAN_X;
        if (sy[j] - sy[q] != edge(q, j, 1)) bits |= KMC_SPAN_Y;
      }
    }
    const int size = (int)queue.size();
    if (size > out->largest_size) {  // (components come in label order: the first of a size keeps the tie)
      out->largest_size = size;
      out->largest_label = r + 1;
      out->largest_span = bits;
    }
    if (bits) {
      out->n_spanning += 1;
      out->n_span_x += (bits & KMC_SPAN_X) != 0;
      out->n_span_y += (bits & KMC_SPAN_Y) != 0;
      out->proteins_in_spanning += size;
      for (int q : queue) {
        sp[q] = (uint8_t)bits;
        sx[q] = sy[q] = 0;
      }
      continue;
    }
    if (size < 2) continue;
    out->n_measured += 1;
    if (!table) continue;
    long long s1[2] = {0, 0};
    i128 s2 = 0;
    for (int q : queue)
      for (int c = 0; c < 2; ++c) {
        const long long d = ((long long)kmcm::round_(pos(q, c) * 1024.0) + (long long)(c ? sy[q] : sx[q]) * B[c]) -
                            (long long)kmcm::round_(pos(r, c) * 1024.0);
        s1[c] += d;
        s2 += (i128)d * d;
      }
    const int k = std::min(size, (int)max_size);
    table[k].count += 1;
    table[k].sum_size += size;
    sum_m[k] += (i128)size * s2 - ((i128)s1[0] * s1[0] + (i128)s1[1] * s1[1]);
  }
  for (size_t k = 0; k < sum_m.size(); ++k) put(&table[k].sum_m, sum_m[k]);
  if (label) std::copy(lab.begin(), lab.end(), label);
  if (shift) {
    std::copy(sx.begin(), sx.end(), shift);
    std::copy(sy.begin(), sy.end(), shift + n);
  }
  if (span) std::copy(sp.begin(), sp.end(), span);
  return KMC_OK;
}

// Structure factor (include/kmc.h), sequential: per selected protein the axis
// tables of h = 0..hmax and |k| = 0..kmax, then one term per wave vector added
// to its species' sums.
int kmc_host_structure_factor(const kmc_params* p, const kmc_state_view* v, int32_t hmax, int32_t kmax,
                              int32_t select, int64_t* sums, int64_t n_sel[2]) {
  if (!p || !v || !sums || !n_sel || !v->a_int || !v->b_int || !v->ra || !v->rb || p->n_a < 0 || p->n_b < 0 ||
      hmax < 0 || hmax > KMC_SK_MAX || kmax < 0 || kmax > KMC_SK_MAX ||
      (select != KMC_SK_ALL && select != KMC_SK_BOUND)) {
    g_host_err = "structure factor: params, state, sums and n_sel are needed, 0 <= hmax, kmax <= 64, select 0 or 1";
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, nb = p->n_b, n = na + nb;
  const int64_t B[2] = {(int64_t)kmcm::round_(p->box_x * 1024.0), (int64_t)kmcm::round_(p->box_y * 1024.0)};
  if (B[0] < 1 || B[1] < 1) {
    g_host_err = "structure factor: the box is below 2^-10 A";
    return KMC_ERR_ARG;
  }
  const int W = 2 * kmax + 1;
  const size_t nq = (size_t)(hmax + 1) * W;
  std::memset(sums, 0, sizeof(int64_t) * 4 * nq);
  n_sel[0] = n_sel[1] = 0;
  double cx[KMC_SK_MAX + 1], sx[KMC_SK_MAX + 1], cy[KMC_SK_MAX + 1], sy[KMC_SK_MAX + 1];
  for (int q = 0; q < n; ++q) {
    const int sp = q < na ? 0 : 1;
    if (select == KMC_SK_BOUND) {
      bool bound;
      if (q < na) bound = v->a_int[2 * (size_t)na + q] != 0 || v->a_int[4 * (size_t)na + q] != 0;
      else {
        bound = false;
        for (int j = 2; j <= 4; ++j) bound = bound || v->b_int[(size_t)(4 + j - 1) * nb + (q - na)] != 0;
      }
      if (!bound) continue;
    }
    n_sel[sp] += 1;
    const double x = q < na ? v->ra[RA(na, 1, 1, 0, q)] : v->rb[RB(nb, 1, 1, 0, q - na)];
    const double y = q < na ? v->ra[RA(na, 1, 1, 1, q)] : v->rb[RB(nb, 1, 1, 1, q - na)];
    const int64_t X = (int64_t)kmcm::round_(x * 1024.0), Y = (int64_t)kmcm::round_(y * 1024.0);
    for (int h = 0; h <= hmax; ++h) kmcs::axis_phase(h, X, B[0], &cx[h], &sx[h]);
    for (int k = 0; k <= kmax; ++k) kmcs::axis_phase(k, Y, B[1], &cy[k], &sy[k]);
    int64_t* C = sums + (size_t)(2 * sp) * nq;
    int64_t* S = sums + (size_t)(2 * sp + 1) * nq;
    for (int h = 0; h <= hmax; ++h)
      for (int k = -kmax; k <= kmax; ++k) {
        const int ak = k < 0 ? -k : k;
        int64_t tc, ts;
        kmcs::term(cx[h], sx[h], cy[ak], sy[ak], k < 0, &tc, &ts);
        C[(size_t)h * W + (k + kmax)] += tc;
        S[(size_t)h * W + (k + kmax)] += ts;
      }
  }
  return KMC_OK;
}

// Bond-orientational order (include/kmc.h), sequential.  The local pass leaves
// the set, its integer coordinates and every protein's (C, S, N) by the
// species' reference index; neighbours within the cutoff come from a
// counting-sorted periodic cell grid (the 3 x 3 cells around a centre), so the
// cost is linear in the set whatever its size.
extern "C++" {
namespace {

struct BoHost {
  int n = 0;          // proteins of the species
  int64_t B[2] = {0, 0};
  std::vector<uint8_t> sel;
  std::vector<int64_t> X, Y, C, S;
  std::vector<int32_t> nn;
};

struct BoCells {
  int ncx = 0, ncy = 0;
  std::vector<int32_t> start, item;  // cell c holds item[start[c] .. start[c + 1])
  void build(const BoHost& h, const std::vector<int32_t>& who, int ncx_, int ncy_) {
    ncx = ncx_;
    ncy = ncy_;
    start.assign((size_t)ncx * ncy + 1, 0);
    item.resize(who.size());
    std::vector<int32_t> cell(who.size());
    for (size_t t = 0; t < who.size(); ++t) {
      const int i = who[t];
      cell[t] = kmcb::cell_of(kmcb::wrap(h.Y[i], h.B[1]), ncy, h.B[1]) * ncx +
                kmcb::cell_of(kmcb::wrap(h.X[i], h.B[0]), ncx, h.B[0]);
      start[(size_t)cell[t] + 1] += 1;
    }
    for (size_t c = 0; c + 1 < start.size(); ++c) start[c + 1] += start[c];
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (size_t t = 0; t < who.size(); ++t) item[(size_t)fill[cell[t]]++] = who[t];
  }
  // f(j) for every item of the 3 x 3 cells around point i's cell (distinct cells: ncx, ncy >= 3)
  template <typename F>
  void around(const BoHost& h, int i, F f) const {
    const int cx = kmcb::cell_of(kmcb::wrap(h.X[i], h.B[0]), ncx, h.B[0]);
    const int cy = kmcb::cell_of(kmcb::wrap(h.Y[i], h.B[1]), ncy, h.B[1]);
    for (int oy = -1; oy <= 1; ++oy)
      for (int ox = -1; ox <= 1; ++ox) {
        const size_t c = (size_t)((cy + oy + ncy) % ncy) * ncx + (cx + ox + ncx) % ncx;
        for (int32_t t = start[c]; t < start[c + 1]; ++t) f(item[(size_t)t]);
      }
  }
};

int bo_host_local(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t mode, int32_t fold,
                  double r_cut, int32_t select, BoHost* h, std::string* err) {
  if (!p || !v || !v->a_int || !v->b_int || !v->ra || !v->rb || p->n_a < 0 || p->n_b < 0 ||
      (which != KMC_BO_A && which != KMC_BO_B) || (mode != KMC_BO_WITHIN && mode != KMC_BO_LINKED) || fold < 1 ||
      fold > KMC_BO_MAX_FOLD || (select != KMC_BO_ALL && select != KMC_BO_BOUND) ||
      (mode == KMC_BO_LINKED && which != KMC_BO_B)) {
    *err = "bond order: params and state are needed, which 0 or 1, mode 0 or 1 (linked: ligands only), 1 <= fold <= 12, select 0 or 1";
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, nb = p->n_b, n = which == KMC_BO_A ? na : nb;
  const double bx = kmcm::round_(p->box_x * 1024.0), by = kmcm::round_(p->box_y * 1024.0);
  if (!(bx >= 1.0) || !(by >= 1.0) || !(bx < (double)BO_BOX_MAX) || !(by < (double)BO_BOX_MAX)) {
    *err = "bond order: the box is below 2^-10 A or not below 2^21 A";
    return KMC_ERR_ARG;
  }
  h->n = n;
  h->B[0] = (int64_t)bx;
  h->B[1] = (int64_t)by;
  int64_t RC = 0;
  if (mode == KMC_BO_WITHIN) {
    const double rc = r_cut > 0.0 && r_cut * 1024.0 < (double)BO_BOX_MAX ? kmcm::round_(r_cut * 1024.0) : 0.0;
    RC = (int64_t)rc;
    if (RC < 1 || h->B[0] / RC < 3 || h->B[1] / RC < 3) {
      *err = "bond order: r_cut must be positive and at most a third of the box (3 cells along an axis)";
      return KMC_ERR_ARG;
    }
  }
  h->sel.assign((size_t)n, 1);
  h->X.resize((size_t)n);
  h->Y.resize((size_t)n);
  h->C.assign((size_t)n, 0);
  h->S.assign((size_t)n, 0);
  h->nn.assign((size_t)n, 0);
  std::vector<int32_t> who;
  for (int i = 0; i < n; ++i) {
    if (which == KMC_BO_A) {
      h->X[i] = (int64_t)kmcm::round_(v->ra[RA(na, 1, 1, 0, i)] * 1024.0);
      h->Y[i] = (int64_t)kmcm::round_(v->ra[RA(na, 1, 1, 1, i)] * 1024.0);
      if (select == KMC_BO_BOUND) h->sel[i] = v->a_int[2 * (size_t)na + i] != 0 || v->a_int[4 * (size_t)na + i] != 0;
    } else {
      h->X[i] = (int64_t)kmcm::round_(v->rb[RB(nb, 1, 1, 0, i)] * 1024.0);
      h->Y[i] = (int64_t)kmcm::round_(v->rb[RB(nb, 1, 1, 1, i)] * 1024.0);
      if (select == KMC_BO_BOUND) {
        bool bound = false;
        for (int j = 2; j <= 4; ++j) bound = bound || v->b_int[(size_t)(4 + j - 1) * nb + i] != 0;
        h->sel[i] = bound;
      }
    }
    if (h->sel[i]) who.push_back(i);
  }
  auto add = [&](int i, int j) {
    const int64_t DX = kmcb::fold(h->X[j] - h->X[i], h->B[0]), DY = kmcb::fold(h->Y[j] - h->Y[i], h->B[1]);
    if (DX == 0 && DY == 0) return;
    int64_t tc, ts;
    kmcb::term(fold, DX, DY, &tc, &ts);
    h->C[i] += tc;
    h->S[i] += ts;
    h->nn[i] += 1;
  };
  if (mode == KMC_BO_WITHIN) {
    BoCells g;
    g.build(*h, who, (int)std::min<int64_t>(h->B[0] / RC, BO_NC_MAX), (int)std::min<int64_t>(h->B[1] / RC, BO_NC_MAX));
    const int64_t RC2 = RC * RC;
    for (int i : who) {
      int64_t cnt = 0;
      g.around(*h, i, [&](int j) {
        const int64_t DX = kmcb::fold(h->X[j] - h->X[i], h->B[0]), DY = kmcb::fold(h->Y[j] - h->Y[i], h->B[1]);
        const int64_t D2 = DX * DX + DY * DY;
        if (D2 <= 0 || D2 > RC2) return;
        if (++cnt <= BO_NN_MAX) add(i, j);
      });
      if (cnt > BO_NN_MAX) {
        *err = "bond order: a protein with more than 65535 neighbours";
        return KMC_ERR_CAPACITY;
      }
    }
  } else {
    for (int b : who) {
      for (int j = 2; j <= 4; ++j) {
        const int r = v->b_int[(size_t)(4 + j - 1) * nb + b];
        if (r == 0) continue;
        int r2 = 0, l = 0;
        bool ok = r >= 1 && r <= na;
        if (ok) {
          r2 = v->a_int[4 * (size_t)na + (r - 1)];
          ok = r2 >= 0 && r2 <= na;
        }
        if (ok && r2 != 0) {
          l = v->a_int[2 * (size_t)na + (r2 - 1)];
          ok = l == 0 || (l > na && l <= na + nb);
        }
        if (!ok) {
          *err = "bond order: a link followed from ligand " + std::to_string(b + 1) + " leaves the state";
          return KMC_ERR_STATE;
        }
        if (r2 == 0 || l == 0) continue;
        const int b2 = l - 1 - na;
        if (b2 == b || !h->sel[b2]) continue;
        add(b, b2);
      }
    }
  }
  return KMC_OK;
}

}  // namespace
}  // extern "C++"

int kmc_host_bond_order(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t mode, int32_t fold,
                        double r_cut, int32_t select, int32_t nbins, int64_t* hist, kmc_bond_order_out* out,
                        int64_t* C, int64_t* S, int32_t* nn) {
  if (!out || nbins < 1 || nbins > BO_HIST_BINS) {
    g_host_err = "bond order: out is needed, 1 <= nbins <= 1024";
    return KMC_ERR_ARG;
  }
  BoHost h;
  const int rc = bo_host_local(p, v, which, mode, fold, r_cut, select, &h, &g_host_err);
  if (rc != KMC_OK) return rc;
  std::memset(out, 0, sizeof *out);
  if (hist) std::fill(hist, hist + (size_t)KMC_BO_NN_ROWS * nbins, (int64_t)0);
  for (int i = 0; i < h.n; ++i) {
    if (!h.sel[i]) continue;
    const int64_t N = h.nn[i];
    const int64_t pc = N ? kmcb::normalise(h.C[i], N) : 0, ps = N ? kmcb::normalise(h.S[i], N) : 0;
    const int64_t m = pc * pc + ps * ps;
    out->n_sel += 1;
    out->n_with += N > 0;
    out->sum_nn += N;
    out->sum_pc += pc;
    out->sum_ps += ps;
    out->sum_m += m;
    if (hist) hist[(size_t)std::min<int64_t>(N, KMC_BO_NN_ROWS - 1) * nbins + kmcb::mag_bin(m, nbins)] += 1;
  }
  if (C) std::copy(h.C.begin(), h.C.end(), C);
  if (S) std::copy(h.S.begin(), h.S.end(), S);
  if (nn) std::copy(h.nn.begin(), h.nn.end(), nn);
  return KMC_OK;
}

int kmc_host_bond_order_corr(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t mode,
                             int32_t fold, double r_cut, int32_t select, double r_max, int32_t nbins,
                             int64_t* corr) {
  if (!corr || nbins < 1 || nbins > BO_CORR_BINS || !(r_max > 0.0) || !std::isfinite(r_max)) {
    g_host_err = "bond order: corr is needed, r_max > 0, 1 <= nbins <= 4096";
    return KMC_ERR_ARG;
  }
  BoHost h;
  const int rc = bo_host_local(p, v, which, mode, fold, r_cut, select, &h, &g_host_err);
  if (rc != KMC_OK) return rc;
  const double dr = r_max / nbins;
  std::vector<int64_t> E2((size_t)nbins + 1);
  const int64_t EN = r_max * 1024.0 < (double)BO_BOX_MAX ? kmcb::corr_edge(nbins, dr) : 0;
  if (EN < 1 || !(std::floor(p->box_x / r_max) >= 3.0) || !(std::floor(p->box_y / r_max) >= 3.0) || h.B[0] / EN < 3 ||
      h.B[1] / EN < 3) {
    g_host_err = "bond order: r_max must be at least 2^-10 A and at most a third of the box (3 cells along an axis)";
    return KMC_ERR_ARG;
  }
  for (int m = 0; m <= nbins; ++m) {
    const int64_t e = kmcb::corr_edge(m, dr);
    E2[m] = e * e;
  }
  std::vector<int32_t> who;
  std::vector<int64_t> pc((size_t)h.n, 0), ps((size_t)h.n, 0);
  for (int i = 0; i < h.n; ++i) {
    if (!h.sel[i] || h.nn[i] == 0) continue;
    pc[i] = kmcb::normalise(h.C[i], h.nn[i]);
    ps[i] = kmcb::normalise(h.S[i], h.nn[i]);
    who.push_back(i);
  }
  std::fill(corr, corr + 2 * (size_t)nbins, (int64_t)0);
  BoCells g;
  g.build(h, who, (int)std::min<int64_t>(h.B[0] / EN, BO_NC_MAX), (int)std::min<int64_t>(h.B[1] / EN, BO_NC_MAX));
  const double inv = 1.0 / (dr * 1024.0);
  for (int i : who)
    g.around(h, i, [&](int j) {
      if (j <= i) return;
      const int64_t DX = kmcb::fold(h.X[j] - h.X[i], h.B[0]), DY = kmcb::fold(h.Y[j] - h.Y[i], h.B[1]);
      const int64_t D2 = DX * DX + DY * DY;
      if (D2 >= E2[nbins]) return;
      const int k = kmcb::corr_bin(E2.data(), nbins, D2, (int)(std::sqrt((double)D2) * inv));
      if (k >= nbins) return;
      corr[k] += pc[i] * pc[j] + ps[i] * ps[j];
      corr[(size_t)nbins + k] += 1;
    });
  return KMC_OK;
}

// Proximity clusters (include/kmc.h), sequential on the bond
// order's cell grid (BoHost holds all n_a + n_b proteins by reference index):
// the neighbour counts, a union-find over the core pairs in index order, the
// border rule from each non-core's side, then the counts; c(i) is
// kmc_host_census' label.  The expressions are kmc_proximity.h's.
int kmc_host_prox_clusters(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t select,
                           const uint8_t* mask, double eps, int32_t min_pts, int32_t max_size, int32_t nbins,
                           kmc_prox_out* out, int64_t* size_hist, int64_t* nn_hist, int64_t* nnd_hist, int32_t* label,
                           int32_t* nn, uint8_t* kind) {
  if (!p || !v || !out || !v->a_int || !v->b_int || !v->ra || !v->rb || p->n_a < 0 || p->n_b < 0 || which < KMC_PX_A ||
      which > KMC_PX_AB || (select != KMC_SK_ALL && select != KMC_SK_BOUND) || min_pts < 1 ||
      min_pts > PX_MIN_PTS_MAX || max_size < 1 || max_size > PX_MAX_SIZE || nbins < 1 || nbins > PX_NND_BINS) {
    g_host_err = "prox: params, state and out are needed, which 0..2, select 0 or 1, 1 <= min_pts <= 2^30, 1 <= max_size <= 65535, 1 <= nbins <= 4096";
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, nb = p->n_b, n = na + nb;
  const double bx = kmcm::round_(p->box_x * 1024.0), by = kmcm::round_(p->box_y * 1024.0);
  if (!(bx >= 1.0) || !(by >= 1.0) || !(bx < (double)BO_BOX_MAX) || !(by < (double)BO_BOX_MAX)) {
    g_host_err = "prox: the box is below 2^-10 A or not below 2^21 A";
    return KMC_ERR_ARG;
  }
  BoHost h;
  h.n = n;
  h.B[0] = (int64_t)bx;
  h.B[1] = (int64_t)by;
  const int64_t EPS = eps > 0.0 && eps * 1024.0 < (double)BO_BOX_MAX ? (int64_t)kmcm::round_(eps * 1024.0) : 0;
  if (EPS < 1 || h.B[0] / EPS < 3 || h.B[1] / EPS < 3) {
    g_host_err = "prox: eps must be at least 2^-10 A and at most a third of the box (3 cells along an axis)";
    return KMC_ERR_ARG;
  }
  std::vector<int32_t> c((size_t)n, 0);
  kmc_census census;
  const int rc = kmc_host_census(p, v, c.data(), 0, 0, nullptr, &census);
  if (rc != KMC_OK) return rc;
  h.sel.assign((size_t)n, 0);
  h.X.resize((size_t)n);
  h.Y.resize((size_t)n);
  std::vector<int32_t> who;
  for (int i = 0; i < n; ++i) {
    bool sel;
    if (i < na) {
      h.X[i] = (int64_t)kmcm::round_(v->ra[RA(na, 1, 1, 0, i)] * 1024.0);
      h.Y[i] = (int64_t)kmcm::round_(v->ra[RA(na, 1, 1, 1, i)] * 1024.0);
      sel = which != KMC_PX_B &&
            (select == KMC_SK_ALL || v->a_int[2 * (size_t)na + i] != 0 || v->a_int[4 * (size_t)na + i] != 0);
    } else {
      const int b = i - na;
      h.X[i] = (int64_t)kmcm::round_(v->rb[RB(nb, 1, 1, 0, b)] * 1024.0);
      h.Y[i] = (int64_t)kmcm::round_(v->rb[RB(nb, 1, 1, 1, b)] * 1024.0);
      bool bound = false;
      for (int j = 2; j <= 4; ++j) bound = bound || v->b_int[(size_t)(4 + j - 1) * nb + b] != 0;
      sel = which != KMC_PX_A && (select == KMC_SK_ALL || bound);
    }
    if (sel && mask) sel = mask[i] != 0;
    h.sel[i] = sel;
    if (sel) who.push_back(i);
  }
  BoCells g;
  g.build(h, who, (int)std::min<int64_t>(h.B[0] / EPS, BO_NC_MAX), (int)std::min<int64_t>(h.B[1] / EPS, BO_NC_MAX));
  const int64_t EPS2 = EPS * EPS;
  auto dist2 = [&](int i, int j) {
    const int64_t DX = kmcb::fold(h.X[j] - h.X[i], h.B[0]), DY = kmcb::fold(h.Y[j] - h.Y[i], h.B[1]);
    return DX * DX + DY * DY;
  };
  std::vector<int32_t> N((size_t)n, 0), lab((size_t)n, 0), parent((size_t)n);
  std::vector<int64_t> M((size_t)n, 0);
  std::vector<uint8_t> kd((size_t)n, 0);
  for (int i : who) {
    int64_t best = INT64_MAX;
    g.around(h, i, [&](int j) {
      if (j == i) return;
      const int64_t D2 = dist2(i, j);
      if (D2 > EPS2) return;
      N[i] += 1;
      best = std::min(best, D2);
    });
    M[i] = N[i] ? best : 0;
    kd[i] = kmcx::is_core(N[i], min_pts) ? 3 : 1;
  }
  for (int i = 0; i < n; ++i) parent[i] = i;
  auto find = [&](int x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  std::memset(out, 0, sizeof *out);
  for (int i : who) {
    if (kd[i] != 3) continue;
    g.around(h, i, [&](int j) {
      if (j >= i || kd[j] != 3 || dist2(i, j) > EPS2) return;
      out->n_core_edges += 1;
      const int a = find(i), b = find(j);
      if (a != b) parent[std::max(a, b)] = std::min(a, b);
    });
  }
  for (int i : who)
    if (kd[i] == 3) lab[i] = find(i) + 1;
  for (int i : who) {
    if (kd[i] == 3 || N[i] == 0) continue;
    int64_t bestD = 0;
    int32_t bestR = -1;
    g.around(h, i, [&](int j) {
      if (j == i || kd[j] != 3) return;
      const int64_t D2 = dist2(i, j);
      if (D2 > EPS2 || !kmcx::nearer(D2, j, bestD, bestR)) return;
      bestD = D2;
      bestR = j;
    });
    if (bestR >= 0) {
      kd[i] = 2;
      lab[i] = lab[bestR];
    }
  }
  const double dr = eps / nbins;
  std::vector<int64_t> E2((size_t)nbins);
  for (int m = 0; m < nbins; ++m) {
    const int64_t e = kmcb::corr_edge(m, dr);
    E2[m] = e * e;
  }
  const double inv = 1.0 / (dr * 1024.0);
  if (size_hist) std::fill(size_hist, size_hist + (size_t)max_size + 1, (int64_t)0);
  if (nn_hist) std::fill(nn_hist, nn_hist + KMC_PX_NN_ROWS, (int64_t)0);
  if (nnd_hist) std::fill(nnd_hist, nnd_hist + nbins, (int64_t)0);
  // by root (a cluster's label - 1, a component's c - 1): members and the ranges purity is read from
  std::vector<int32_t> cnt((size_t)n, 0), cmin((size_t)n, INT32_MAX), cmax((size_t)n, -1), pmin((size_t)n, INT32_MAX),
      pmax((size_t)n, -1), bsel((size_t)n, 0);
  for (int i : who) {
    out->n_sel += 1;
    (kd[i] == 3 ? out->n_core : kd[i] == 2 ? out->n_border : out->n_noise) += 1;
    out->sum_nn += N[i];
    if (nn_hist) nn_hist[std::min<int32_t>(N[i], KMC_PX_NN_ROWS - 1)] += 1;
    if (N[i] == 0) out->n_alone += 1;
    else if (nnd_hist) nnd_hist[kmcx::nnd_bin(E2.data(), nbins, M[i], (int)(std::sqrt((double)M[i]) * inv))] += 1;
    const int ci = c[i] - 1, L = lab[i];
    bsel[ci] += 1;
    pmin[ci] = std::min(pmin[ci], L);
    pmax[ci] = std::max(pmax[ci], L);
    if (L > 0) {
      cnt[L - 1] += 1;
      cmin[L - 1] = std::min(cmin[L - 1], ci);
      cmax[L - 1] = std::max(cmax[L - 1], ci);
    }
  }
  for (int i = 0; i < n; ++i) {
    if (kd[i] == 3 && lab[i] == i + 1) {
      const int size = cnt[i];
      if (size_hist) size_hist[std::min(size, (int)max_size)] += 1;
      out->n_clusters += 1;
      if (size > out->max_size) {  // (roots come in label order: the first of a size keeps the tie)
        out->max_size = size;
        out->max_label = i + 1;
      }
      if (size >= 2) {
        out->n_multi += 1;
        if (cmin[i] == cmax[i]) {
          out->n_pure += 1;
          if (bsel[cmin[i]] == size) out->n_whole += 1;
        }
      }
    }
    if (bsel[i] >= 2) {
      out->n_bond_multi += 1;
      if (pmin[i] == pmax[i] && pmin[i] > 0) out->n_bond_kept += 1;
    }
  }
  if (label) std::copy(lab.begin(), lab.end(), label);
  if (nn) std::copy(N.begin(), N.end(), nn);
  if (kind) std::copy(kd.begin(), kd.end(), kind);
  return KMC_OK;
}

// Bond kinetics (include/kmc.h): kmc_kin_*'s definitions on host
// state views, one receptor after the other; the transition and the bin rule
// are kmc_kinetics.h's, the ones the device evaluates.
extern "C++" {
namespace {

bool kin_view_ok(const kmc_kin_view* w) {
  return w && w->rl_lig && w->rl_site && w->rl_since && w->cis_with && w->cis_since && w->last_lig && w->free_since &&
         w->bits;
}

// receptor i's (0-based) current links, checked as the device checks them
bool kin_host_cur(const kmc_params* p, const kmc_state_view* v, int i, kmck::Cur* c) {
  const int na = p->n_a, n = p->n_a + p->n_b;
  const int32_t n2 = v->a_int[2 * (size_t)na + i], n4 = v->a_int[3 * (size_t)na + i], n3 = v->a_int[4 * (size_t)na + i];
  c->lig = c->site = c->cis = 0;
  c->cx = false;
  if (n2 != 0 && (n2 <= na || n2 > n)) return false;
  if (n3 != 0 && (n3 < 1 || n3 > na || n3 == i + 1)) return false;
  if (n4 < 0 || n4 > 4) return false;
  c->lig = n2;
  c->site = n4;
  c->cis = n3;
  c->cx = n3 != 0 && (n2 != 0 || v->a_int[2 * (size_t)na + (n3 - 1)] != 0);
  return true;
}

kmck::Rec kin_load(const kmc_kin_view* w, int i) {
  kmck::Rec r;
  r.rl_lig = w->rl_lig[i];
  r.rl_site = w->rl_site[i];
  r.cis_with = w->cis_with[i];
  r.last_lig = w->last_lig[i];
  r.rl_since = w->rl_since[i];
  r.cis_since = w->cis_since[i];
  r.free_since = w->free_since[i];
  r.bits = w->bits[i];
  return r;
}

void kin_store(const kmc_kin_view* w, int i, const kmck::Rec& r) {
  w->rl_lig[i] = r.rl_lig;
  w->rl_site[i] = r.rl_site;
  w->cis_with[i] = r.cis_with;
  w->last_lig[i] = r.last_lig;
  w->rl_since[i] = r.rl_since;
  w->cis_since[i] = r.cis_since;
  w->free_since[i] = r.free_since;
  w->bits[i] = r.bits;
}

void kin_set_occ(const kmc_params* p, kmc_kin_out* acc, const int64_t cnt[kmck::KIN_NCNT]) {
  acc->occ_rl = cnt[kmck::KIN_OCC_RL];
  acc->occ_mono = cnt[kmck::KIN_OCC_MONO];
  acc->occ_cx = cnt[kmck::KIN_OCC_CX];
  acc->occ_free_receptor = (int64_t)p->n_a - acc->occ_rl;
  acc->occ_free_site = 3 * (int64_t)p->n_b - acc->occ_rl;
}

}  // namespace
}  // extern "C++"

int kmc_host_kin_begin(const kmc_params* p, const kmc_state_view* v, const kmc_kin_view* view, kmc_kin_out* acc,
                       int64_t* hist7) {
  if (!p || !v || !v->a_int || !kin_view_ok(view) || !acc || !hist7) {
    g_host_err = "kinetics: params, state, the view's eight arrays, acc and hist are needed";
    return KMC_ERR_ARG;
  }
  int64_t cnt[kmck::KIN_NCNT] = {0};
  for (int i = 0; i < p->n_a; ++i) {
    kmck::Cur c;
    if (!kin_host_cur(p, v, i, &c)) {
      g_host_err = "kinetics: a receptor's bond link leaves its range";
      return KMC_ERR_STATE;
    }
    kmck::Rec r;
    const uint32_t m = kmck::begin(i + 1, v->step, c, r);
    kin_store(view, i, r);
    for (int b = 0; b < kmck::KIN_NCNT; ++b) cnt[b] += m >> b & 1u;
  }
  std::memset(acc, 0, sizeof *acc);
  std::fill(hist7, hist7 + (size_t)KIN_ROWS_UPD * KIN_BINS, (int64_t)0);
  acc->origin_step = acc->last_step = v->step;
  kin_set_occ(p, acc, cnt);
  return KMC_OK;
}

int kmc_host_kin_update(const kmc_params* p, const kmc_state_view* v, const kmc_kin_view* view, kmc_kin_out* acc,
                        int64_t* hist7) {
  if (!p || !v || !v->a_int || !kin_view_ok(view) || !acc || !hist7) {
    g_host_err = "kinetics: params, state, the view's eight arrays, acc and hist are needed";
    return KMC_ERR_ARG;
  }
  for (int i = 0; i < p->n_a; ++i) {  // checked first: a failed call leaves the recorder as it was
    kmck::Cur c;
    if (!kin_host_cur(p, v, i, &c)) {
      g_host_err = "kinetics: a receptor's bond link leaves its range";
      return KMC_ERR_STATE;
    }
  }
  const int64_t t = v->step, dt = t - acc->last_step;
  acc->exp_rl += dt * acc->occ_rl;
  acc->exp_mono += dt * acc->occ_mono;
  acc->exp_cx += dt * acc->occ_cx;
  acc->exp_free_receptor += dt * acc->occ_free_receptor;
  acc->exp_free_site += dt * acc->occ_free_site;
  int64_t cnt[kmck::KIN_NCNT] = {0};
  for (int i = 0; i < p->n_a; ++i) {
    kmck::Cur c;
    kin_host_cur(p, v, i, &c);
    kmck::Rec r = kin_load(view, i);
    int row[3], nh;
    int64_t val[3];
    const uint32_t m = kmck::transition(i + 1, t, c, r, row, val, &nh);
    for (int k = 0; k < nh; ++k) hist7[(size_t)row[k] * KIN_BINS + kmck::bin(val[k])] += 1;
    kin_store(view, i, r);
    for (int b = 0; b < kmck::KIN_NCNT; ++b) cnt[b] += m >> b & 1u;
  }
  acc->rl_on += cnt[kmck::KIN_EV_RL_ON];
  acc->rl_off += cnt[kmck::KIN_EV_RL_OFF];
  acc->rl_swap += cnt[kmck::KIN_EV_RL_SWAP];
  acc->cis_on += cnt[kmck::KIN_EV_CIS_ON];
  acc->cis_off_mono += cnt[kmck::KIN_EV_CIS_OFF_MONO];
  acc->cis_off_cx += cnt[kmck::KIN_EV_CIS_OFF_CX];
  acc->cis_swap += cnt[kmck::KIN_EV_CIS_SWAP];
  kin_set_occ(p, acc, cnt);
  acc->last_step = t;
  acc->n_updates += 1;
  return KMC_OK;
}

int kmc_host_kin_sample(const kmc_params* p, const kmc_kin_view* view, const kmc_kin_out* acc, const int64_t* hist7,
                        kmc_kin_out* out, int64_t* hist9) {
  if (!p || !kin_view_ok(view) || !acc || !hist7 || !out) {
    g_host_err = "kinetics sample: params, the view's eight arrays, acc, hist and out are needed";
    return KMC_ERR_ARG;
  }
  const kmc_kin_out a = *acc;  // (out may be acc itself)
  *out = a;
  out->n_rl_censored_alive = out->n_cis_censored_alive = 0;
  if (hist9) {
    std::copy(hist7, hist7 + (size_t)KIN_ROWS_UPD * KIN_BINS, hist9);
    std::fill(hist9 + (size_t)KIN_ROWS_UPD * KIN_BINS, hist9 + (size_t)KIN_HISTS * KIN_BINS, (int64_t)0);
  }
  for (int i = 0; i < p->n_a; ++i) {
    const kmck::Rec r = kin_load(view, i);
    const uint32_t m = kmck::alive(i + 1, r);
    if (hist9 && (m & 1u)) hist9[(size_t)kmck::KIN_ROW_RL_ALIVE * KIN_BINS + kmck::bin(a.last_step - r.rl_since)] += 1;
    if (hist9 && (m & 2u)) hist9[(size_t)kmck::KIN_ROW_CIS_ALIVE * KIN_BINS + kmck::bin(a.last_step - r.cis_since)] += 1;
    out->n_rl_censored_alive += m >> 2 & 1u;
    out->n_cis_censored_alive += m >> 3 & 1u;
  }
  return KMC_OK;
}

// Cluster growth kinetics (include/kmc.h): kmc_cf_*'s
// definitions on host state views.  Where the device runs two lock-free
// union-finds, the partitions here come from breadth-first walks over an
// adjacency list (the walk's start, in index order, is the label); the filing
// rule is kmc_coag.h's, the one the device evaluates.
extern "C++" {
namespace {

typedef std::pair<int32_t, int32_t> CfEdge;

bool cf_view_ok(const kmc_cf_view* w) { return w && w->rl_lig && w->cis_with && w->prev_label; }

bool cf_tables_ok(const kmc_cf_tables* t) {
  return t && t->merge && t->frag && t->merge_kind && t->frag_kind && t->merge_pieces && t->frag_pieces &&
         t->merge_product && t->frag_parent && t->n_s && t->expo && t->expo2;
}

// receptor i's (0-based) current bonds, checked as the device checks them
bool cf_host_cur(const kmc_params* p, const kmc_state_view* v, int i, int32_t* lig, int32_t* cis) {
  const int na = p->n_a, n = p->n_a + p->n_b;
  const int32_t n2 = v->a_int[2 * (size_t)na + i], n3 = v->a_int[4 * (size_t)na + i];
  *lig = *cis = 0;
  if (n2 != 0 && (n2 <= na || n2 > n)) return false;
  if (n3 != 0 && (n3 < 1 || n3 > na || n3 == i + 1)) return false;
  *lig = n2;
  *cis = n3;
  return true;
}

// components of n vertices under `edges` (0-based ends): label[i] = the
// smallest member (0-based), cnt[label] = the packed (receptors, ligands)
void cf_walk(int n, int na, const std::vector<CfEdge>& edges, std::vector<int32_t>& label,
             std::vector<uint64_t>& cnt) {
  std::vector<int32_t> start((size_t)n + 1, 0), adj(2 * edges.size()), queue;
  for (const CfEdge& e : edges) {
    start[(size_t)e.first + 1] += 1;
    start[(size_t)e.second + 1] += 1;
  }
  for (int i = 0; i < n; ++i) start[(size_t)i + 1] += start[(size_t)i];
  std::vector<int32_t> fill(start.begin(), start.end() - 1);
  for (const CfEdge& e : edges) {
    adj[(size_t)fill[(size_t)e.first]++] = e.second;
    adj[(size_t)fill[(size_t)e.second]++] = e.first;
  }
  label.assign((size_t)n, -1);
  cnt.assign((size_t)n, 0);
  queue.reserve((size_t)n);
  for (int r = 0; r < n; ++r) {
    if (label[(size_t)r] >= 0) continue;
    queue.clear();
    queue.push_back(r);
    label[(size_t)r] = r;
    for (size_t h = 0; h < queue.size(); ++h) {
      const int q = queue[h];
      cnt[(size_t)r] += q < na ? 1ull : 1ull << 32;
      for (int32_t k = start[(size_t)q]; k < start[(size_t)q + 1]; ++k)
        if (label[(size_t)adj[(size_t)k]] < 0) {
          label[(size_t)adj[(size_t)k]] = r;
          queue.push_back(adj[(size_t)k]);
        }
    }
  }
}

// the look at `label` / `cnt` becomes the last one: n_s, n_clusters, max_cluster
void cf_host_look(int n, int S, const std::vector<int32_t>& label, const std::vector<uint64_t>& cnt, kmc_cf_out* acc,
                  int64_t* n_s) {
  std::fill(n_s, n_s + S + 1, (int64_t)0);
  acc->n_clusters = acc->max_cluster = 0;
  for (int i = 0; i < n; ++i) {
    if (label[(size_t)i] != i) continue;
    const int size = kmcc::size_of(cnt[(size_t)i]);
    n_s[kmcc::clamp_size(size, S)] += 1;
    acc->n_clusters += 1;
    if (size > acc->max_cluster) acc->max_cluster = size;
  }
}

}  // namespace
}  // extern "C++"

int kmc_host_cf_begin(const kmc_params* p, const kmc_state_view* v, int32_t max_size, const kmc_cf_view* view,
                      kmc_cf_out* acc, const kmc_cf_tables* t) {
  if (!p || !v || !v->a_int || !cf_view_ok(view) || !acc || !cf_tables_ok(t) || max_size < CF_MIN_SIZE ||
      max_size > CF_MAX_SIZE) {
    g_host_err = "growth: params, state, the view's three arrays, acc and every table are needed, 2 <= max_size <= 63";
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, n = p->n_a + p->n_b, S = max_size;
  std::vector<CfEdge> e1;
  for (int i = 0; i < na; ++i) {
    int32_t lig, cis;
    if (!cf_host_cur(p, v, i, &lig, &cis)) {
      g_host_err = "growth: a receptor's bond link leaves its range";
      return KMC_ERR_STATE;
    }
    if (lig) e1.push_back(CfEdge(i, lig - 1));
    if (cis && i + 1 < cis) e1.push_back(CfEdge(i, cis - 1));
  }
  for (int i = 0; i < na; ++i) cf_host_cur(p, v, i, &view->rl_lig[i], &view->cis_with[i]);
  std::vector<int32_t> label;
  std::vector<uint64_t> cnt;
  cf_walk(n, na, e1, label, cnt);
  for (int i = 0; i < n; ++i) view->prev_label[i] = label[(size_t)i] + 1;
  const size_t n1 = (size_t)S + 1, n2 = n1 * n1;
  std::memset(acc, 0, sizeof *acc);
  std::fill(t->merge, t->merge + n2, (int64_t)0);
  std::fill(t->frag, t->frag + n2, (int64_t)0);
  std::fill(t->merge_kind, t->merge_kind + CF_KINDS * CF_KINDS, (int64_t)0);
  std::fill(t->frag_kind, t->frag_kind + CF_KINDS * CF_KINDS, (int64_t)0);
  std::fill(t->merge_pieces, t->merge_pieces + CF_PIECES, (int64_t)0);
  std::fill(t->frag_pieces, t->frag_pieces + CF_PIECES, (int64_t)0);
  std::fill(t->merge_product, t->merge_product + n1, (int64_t)0);
  std::fill(t->frag_parent, t->frag_parent + n1, (int64_t)0);
  std::fill(t->expo, t->expo + n1, (int64_t)0);
  std::memset(t->expo2, 0, sizeof(kmc_i128) * n2);
  acc->origin_step = acc->last_step = v->step;
  acc->max_size = S;
  cf_host_look(n, S, label, cnt, acc, t->n_s);
  return KMC_OK;
}

int kmc_host_cf_update(const kmc_params* p, const kmc_state_view* v, const kmc_cf_view* view, kmc_cf_out* acc,
                       const kmc_cf_tables* t) {
  if (!p || !v || !v->a_int || !cf_view_ok(view) || !acc || !cf_tables_ok(t) || acc->max_size < CF_MIN_SIZE ||
      acc->max_size > CF_MAX_SIZE) {
    g_host_err = "growth: params, state, the view's three arrays, a begun acc and every table are needed";
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, n = p->n_a + p->n_b, S = (int)acc->max_size;
  if (v->step == acc->last_step) {  // the state of the last look: nothing to file
    acc->n_updates += 1;
    return KMC_OK;
  }
  // the current bonds E1 and the kept bonds K, with the bond counters of this update
  std::vector<CfEdge> e1, kept;
  int64_t ev[4] = {0, 0, 0, 0};  // formed_rl, formed_cis, broken_rl, broken_cis
  for (int i = 0; i < na; ++i) {  // checked first: a failed call leaves the recorder as it was
    int32_t lig, cis;
    if (!cf_host_cur(p, v, i, &lig, &cis)) {
      g_host_err = "growth: a receptor's bond link leaves its range";
      return KMC_ERR_STATE;
    }
  }
  for (int i = 0; i < n; ++i) {
    const int32_t l = view->prev_label[i];
    if (l < 1 || l > i + 1 || view->prev_label[l - 1] != l) {
      g_host_err = "growth: the recorder's label of protein " + std::to_string(i + 1) + " is not its class' smallest member";
      return KMC_ERR_STATE;
    }
  }
  for (int i = 0; i < na; ++i) {
    int32_t lig, cis;
    cf_host_cur(p, v, i, &lig, &cis);
    const int32_t old_lig = view->rl_lig[i], old_cis = view->cis_with[i], me = i + 1;
    if (lig) e1.push_back(CfEdge(i, lig - 1));
    if (cis && me < cis) e1.push_back(CfEdge(i, cis - 1));
    if (lig != old_lig) {
      ev[0] += lig != 0;
      ev[2] += old_lig != 0;
    } else if (lig) {
      kept.push_back(CfEdge(i, lig - 1));
    }
    if (cis != old_cis) {
      ev[1] += cis != 0 && me < cis;
      ev[3] += old_cis != 0 && me < old_cis;
    } else if (cis && me < cis) {
      kept.push_back(CfEdge(i, cis - 1));
    }
    view->rl_lig[i] = lig;
    view->cis_with[i] = cis;
  }
  std::vector<int32_t> cur, core, prev((size_t)n);
  std::vector<uint64_t> cur_cnt, core_cnt, prev_cnt((size_t)n, 0);
  cf_walk(n, na, e1, cur, cur_cnt);
  cf_walk(n, na, kept, core, core_cnt);
  for (int i = 0; i < n; ++i) {
    prev[(size_t)i] = view->prev_label[i] - 1;
    prev_cnt[(size_t)prev[(size_t)i]] += i < na ? 1ull : 1ull << 32;
  }
  // cores per previous and per current cluster
  std::vector<int32_t> k0((size_t)n, 0), k1((size_t)n, 0);
  int64_t n_cores = 0;
  for (int i = 0; i < n; ++i)
    if (core[(size_t)i] == i) {
      k0[(size_t)prev[(size_t)i]] += 1;
      k1[(size_t)cur[(size_t)i]] += 1;
      n_cores += 1;
    }
  for (int i = 0; i < n; ++i) {
    if (core[(size_t)i] != i) continue;
    const int32_t pl = prev[(size_t)i], cl = cur[(size_t)i];
    kmcc::Filing f = kmcc::file(i, core_cnt[(size_t)i], pl, prev_cnt[(size_t)pl], k0[(size_t)pl], S);
    if (f.pieces >= 0) t->frag_pieces[f.pieces] += 1;
    if (f.whole >= 0) t->frag_parent[f.whole] += 1;
    if (f.pair >= 0) t->frag[f.pair] += 1;
    if (f.kinds >= 0) t->frag_kind[f.kinds] += 1;
    f = kmcc::file(i, core_cnt[(size_t)i], cl, cur_cnt[(size_t)cl], k1[(size_t)cl], S);
    if (f.pieces >= 0) t->merge_pieces[f.pieces] += 1;
    if (f.whole >= 0) t->merge_product[f.whole] += 1;
    if (f.pair >= 0) t->merge[f.pair] += 1;
    if (f.kinds >= 0) t->merge_kind[f.kinds] += 1;
  }
  // exposures of the interval that ended, from the previous look's n_s
  typedef __int128 i128;
  const int64_t dt = v->step - acc->last_step;
  for (int x = 1; x <= S; ++x) {
    const int64_t nx = t->n_s[x];
    t->expo[x] += dt * nx;
    for (int y = x; y <= S; ++y) {
      kmc_i128* w = &t->expo2[(size_t)x * (S + 1) + y];
      i128 e = ((i128)w->hi << 64) + (i128)w->lo;
      e += y == x ? (i128)dt * nx * (nx - 1) / 2 : (i128)dt * nx * t->n_s[y];
      w->lo = (uint64_t)(unsigned __int128)e;
      w->hi = (int64_t)(e >> 64);
    }
  }
  const int64_t clusters_prev = acc->n_clusters;
  for (int i = 0; i < n; ++i) view->prev_label[i] = cur[(size_t)i] + 1;
  cf_host_look(n, S, cur, cur_cnt, acc, t->n_s);
  acc->formed_rl += ev[0];
  acc->formed_cis += ev[1];
  acc->broken_rl += ev[2];
  acc->broken_cis += ev[3];
  acc->n_cores = n_cores;
  acc->cycles_closed += ev[0] + ev[1] - (n_cores - acc->n_clusters);
  acc->cycles_opened += ev[2] + ev[3] - (n_cores - clusters_prev);
  acc->last_step = v->step;
  acc->n_updates += 1;
  return KMC_OK;
}

int kmc_host_cf_sample(const kmc_params* p, const kmc_cf_view* view, const kmc_cf_out* acc, const kmc_cf_tables* t,
                       kmc_cf_out* out, const kmc_cf_tables* to) {
  if (!p || !cf_view_ok(view) || !acc || !cf_tables_ok(t) || !out || acc->max_size < CF_MIN_SIZE ||
      acc->max_size > CF_MAX_SIZE) {
    g_host_err = "growth sample: params, the view's three arrays, a begun acc, every table and out are needed";
    return KMC_ERR_ARG;
  }
  const kmc_cf_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (!to) return KMC_OK;
  const size_t n1 = (size_t)a.max_size + 1, n2 = n1 * n1;
  auto copy = [](int64_t* dst, const int64_t* src, size_t n) {
    if (dst && dst != src) std::copy(src, src + n, dst);
  };
  copy(to->merge, t->merge, n2);
  copy(to->frag, t->frag, n2);
  copy(to->merge_kind, t->merge_kind, CF_KINDS * CF_KINDS);
  copy(to->frag_kind, t->frag_kind, CF_KINDS * CF_KINDS);
  copy(to->merge_pieces, t->merge_pieces, CF_PIECES);
  copy(to->frag_pieces, t->frag_pieces, CF_PIECES);
  copy(to->merge_product, t->merge_product, n1);
  copy(to->frag_parent, t->frag_parent, n1);
  copy(to->n_s, t->n_s, n1);
  copy(to->expo, t->expo, n1);
  if (to->expo2 && to->expo2 != t->expo2) std::copy(t->expo2, t->expo2 + n2, to->expo2);
  return KMC_OK;
}

// Ligand network and rings (include/kmc.h), sequential: the
// hops, their checks and the chord rule are kmc_rings.h's, the ones the device
// evaluates; the adjacency is by reference index, and a ring is counted from
// its smallest ligand by a recursive walk.
extern "C++" {
namespace {

struct RgHost {
  std::vector<int32_t> lig, site;  // [nb][3]: the hop's 1-based ligand number and site, 0: none
  int64_t hist[16];
  kmc_net_out out;
};

int rg_host_network(const kmc_params* p, const kmc_state_view* v, RgHost* g, std::string* err) {
  if (!p || !v || !v->a_int || !v->b_int || p->n_a < 0 || p->n_b < 0) {
    *err = "rings: params and state are needed";
    return KMC_ERR_ARG;
  }
  const int na = p->n_a, nb = p->n_b, n = na + nb;
  const size_t NA = (size_t)na;
  g->lig.assign(3 * (size_t)nb, 0);
  g->site.assign(3 * (size_t)nb, 0);
  std::fill(g->hist, g->hist + 16, (int64_t)0);
  std::memset(&g->out, 0, sizeof g->out);
  for (int i = 0; i < na; ++i) {
    const int32_t v2 = v->a_int[2 * NA + i], v3 = v->a_int[4 * NA + i];
    bool ok = kmcr::receptor_links_ok(v2, v3, i + 1, na, nb);
    if (ok && v3 != 0) {
      const int32_t p2 = v->a_int[2 * NA + (v3 - 1)], p3 = v->a_int[4 * NA + (v3 - 1)];
      ok = p3 == i + 1;
      if (ok && v2 == 0 && p2 == 0 && i + 1 < v3) g->out.n_free_dimers += 1;
    }
    if (!ok) {
      *err = "rings: a bond link of receptor " + std::to_string(i + 1) + " is of the wrong kind or not returned";
      return KMC_ERR_STATE;
    }
    g->out.rec[kmcr::rec_bin(v2, v3)] += 1;
  }
  std::vector<uint8_t> vertex((size_t)nb, 0);
  for (int b = 0; b < nb; ++b) {
    kmcr::Hops h;
    kmcr::hops(v->a_int, v->b_int, na, nb, b, h);
    if (h.bad) {
      *err = "rings: a link followed from ligand " + std::to_string(b + 1) + " is of the wrong kind or the bridge is asymmetric";
      return KMC_ERR_STATE;
    }
    int occ = 0, ends = 0;
    for (int e = 0; e < 3; ++e) {
      occ += h.r[e] != 0;
      if (h.r2[e] != 0 && h.l[e] == 0) g->out.n_half += 1;
      if (h.l[e] == 0) continue;
      ++ends;
      g->lig[3 * (size_t)b + e] = h.l[e];
      g->site[3 * (size_t)b + e] = h.s2[e];
      if (kmcr::first_end(b + 1, e + 2, h.l[e], h.s2[e])) {
        g->out.n_bridges += 1;
        g->out.n_loops += h.l[e] == b + 1;
      }
    }
    g->hist[occ * 4 + ends] += 1;
    vertex[b] = ends >= 1;
    g->out.n_vertices += ends >= 1;
  }
  // the components of the whole bond graph (kmc_host_census' walk; every link was checked above) that hold a bridge
  std::vector<uint8_t> seen((size_t)n, 0);
  std::vector<int32_t> queue;
  for (int r = 0; r < n; ++r) {
    if (seen[r]) continue;
    queue.assign(1, r);
    seen[r] = 1;
    bool holds = false;
    for (size_t q = 0; q < queue.size(); ++q) {
      const int x = queue[q];
      int32_t nei[3] = {0, 0, 0};
      if (x < na) {
        nei[0] = v->a_int[2 * NA + x];
        nei[1] = v->a_int[4 * NA + x];
      } else {
        holds = holds || vertex[x - na];
        for (int j = 2; j <= 4; ++j) nei[j - 2] = v->b_int[(size_t)(4 + j - 1) * nb + (x - na)];
      }
      for (int e = 0; e < 3; ++e)
        if (nei[e] != 0 && !seen[nei[e] - 1]) {
          seen[nei[e] - 1] = 1;
          queue.push_back(nei[e] - 1);
        }
    }
    g->out.n_net_components += holds;
  }
  g->out.cycle_rank = g->out.n_bridges - g->out.n_vertices + g->out.n_net_components;
  return KMC_OK;
}

// the walk of one (root, s_first < s_last): simple paths over ligands above the root, closed through s_last
struct RgWalk {
  const RgHost& g;
  int nb, max_len;
  int64_t* counts;   // [2][RG_MAX + 1]
  uint32_t* member;  // [2][nb] or null
  int root = 0, sb = 0;
  int32_t path[RG_MAX];
  int in[RG_MAX], out[RG_MAX];

  void close(int L) {
    auto vert = [&](int j) { return path[j]; };
    auto off = [&](int i) { return g.lig[3 * (size_t)(path[i] - 1) + kmcr::off_site(in[i], out[i]) - 2]; };
    const bool chordless = kmcr::chordless(L, vert, off);
    counts[L] += 1;
    if (chordless) counts[RG_MAX + 1 + L] += 1;
    if (!member) return;
    for (int i = 0; i < L; ++i) {
      member[path[i] - 1] |= 1u << L;
      if (chordless) member[(size_t)nb + path[i] - 1] |= 1u << L;
    }
  }
  // ligand v entered by site s at depth k < max_len (at most max_len - 1 levels of recursion)
  void visit(int32_t v, int s, int k) {
    path[k] = v;
    in[k] = s;
    for (int c = 2; c <= 4; ++c) {
      if (c == s) continue;
      const int32_t w = g.lig[3 * (size_t)(v - 1) + c - 2];
      const int ws = g.site[3 * (size_t)(v - 1) + c - 2];
      if (w == 0) continue;
      out[k] = c;
      if (w == root) {
        if (ws == sb) close(k + 1);
        continue;
      }
      if (w < root || k + 1 >= max_len) continue;
      bool seen = false;
      for (int j = 1; j <= k; ++j) seen = seen || path[j] == w;
      if (!seen) visit(w, ws, k + 1);
    }
  }
  void from(int32_t r, int sa, int sb_) {
    root = r;
    sb = sb_;
    path[0] = r;
    in[0] = sb_;
    out[0] = sa;
    const int32_t w = g.lig[3 * (size_t)(r - 1) + sa - 2];
    const int ws = g.site[3 * (size_t)(r - 1) + sa - 2];
    if (w == 0) return;
    if (w == r) {
      if (ws == sb) close(1);
      return;
    }
    if (w > r && max_len >= 2) visit(w, ws, 1);
  }
};

}  // namespace
}  // extern "C++"

int kmc_host_network(const kmc_params* p, const kmc_state_view* v, kmc_net_out* out, int64_t* lig_hist,
                     int32_t* adj_lig, int32_t* adj_site) {
  RgHost g;
  const int rc = rg_host_network(p, v, &g, &g_host_err);
  if (rc != KMC_OK) return rc;
  if (out) *out = g.out;
  if (lig_hist) std::copy(g.hist, g.hist + 16, lig_hist);
  if (adj_lig) std::copy(g.lig.begin(), g.lig.end(), adj_lig);
  if (adj_site) std::copy(g.site.begin(), g.site.end(), adj_site);
  return KMC_OK;
}

int kmc_host_rings(const kmc_params* p, const kmc_state_view* v, int32_t max_len, int64_t* counts, uint32_t* member,
                   kmc_net_out* out) {
  if (!counts || max_len < 1 || max_len > RG_MAX) {
    g_host_err = "rings: counts is needed, 1 <= max_len <= 12";
    return KMC_ERR_ARG;
  }
  RgHost g;
  const int rc = rg_host_network(p, v, &g, &g_host_err);
  if (rc != KMC_OK) return rc;
  const int nb = p->n_b;
  std::fill(counts, counts + 2 * (RG_MAX + 1), (int64_t)0);
  if (member) std::fill(member, member + 2 * (size_t)nb, 0u);
  RgWalk w{g, nb, max_len, counts, member};
  for (int r = 1; r <= nb; ++r) {
    w.from(r, 2, 3);
    w.from(r, 2, 4);
    w.from(r, 3, 4);
  }
  if (out) *out = g.out;
  return KMC_OK;
}

// Lag correlator (include/kmc.h): kmc_lag_*'s definitions on
// host state views, one protein after the other and one task after the other;
// the schedule and the pair term are kmc_lagcorr.h's, the ones the device
// evaluates.  Every sum is taken whole, in __int128.
extern "C++" {
namespace {

bool lag_view_ok(const kmc_lag_view* w) {
  return w && w->prev && w->U && w->links && w->last_event && w->ring && w->table && w->n_pairs;
}

// protein i's (0-based reference index) integer position and links as the tracker names them
void lag_host_cur(const kmc_params* p, const kmc_state_view* v, int i, int64_t X[2], int32_t l[3]) {
  const int na = p->n_a, nb = p->n_b, n = na + nb;
  auto ref = [&](int32_t x) { return x >= 1 && x <= n ? x : 0; };
  if (i < na) {
    for (int c = 0; c < 2; ++c) X[c] = (int64_t)kmcm::round_(v->ra[RA(na, 1, 1, c, i)] * 1024.0);
    l[0] = ref(v->a_int[2 * (size_t)na + i]);
    l[1] = v->a_int[3 * (size_t)na + i];
    l[2] = ref(v->a_int[4 * (size_t)na + i]);
  } else {
    const int b = i - na;
    for (int c = 0; c < 2; ++c) X[c] = (int64_t)kmcm::round_(v->rb[RB(nb, 1, 1, c, b)] * 1024.0);
    for (int j = 2; j <= 4; ++j) l[j - 2] = ref(v->b_int[(size_t)(4 + j - 1) * nb + b]);
  }
}

void lag_add(kmc_i128* w, __int128 x) {
  const unsigned __int128 u = ((unsigned __int128)(uint64_t)w->hi << 64 | w->lo) + (unsigned __int128)x;
  w->lo = (uint64_t)u;
  w->hi = (int64_t)(uint64_t)(u >> 64);
}

}  // namespace
}  // extern "C++"

int kmc_host_lag_begin(const kmc_params* p, const kmc_state_view* v, const kmc_lag_config* cfg,
                       const kmc_lag_view* view, kmc_lag_out* acc) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !cfg || !lag_view_ok(view) || !acc) {
    g_host_err = "lag: params, state, the configuration, the view's seven arrays and acc are needed";
    return KMC_ERR_ARG;
  }
  kmc_lag_config c = *cfg;
  for (int k = std::max(0, std::min(c.nq, LAG_MAX_Q)); k < LAG_MAX_Q; ++k) c.h[k] = 0;
  int64_t J, F, BX, BY;
  const char* bad =
      kmcl::check(c.every, c.levels, c.slots, c.nq, c.h, p->box_x, p->box_y, &c.max_jump, &c.max_disp, &J, &F, &BX, &BY);
  if (bad) {
    g_host_err = bad;
    return KMC_ERR_ARG;
  }
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  const int L = c.levels, P = c.slots, rows = kmcl::rows(L, P);
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    lag_host_cur(p, v, (int)i, X, l);
    for (int k = 0; k < 2; ++k) view->prev[2 * i + k] = view->U[2 * i + k] = X[k];
    for (int k = 0; k < 3; ++k) view->links[(size_t)k * N + i] = l[k];
    view->last_event[i] = 0;
    for (int lv = 0; lv < L; ++lv)
      for (int k = 0; k < 2; ++k) view->ring[((size_t)(lv * P) * N + i) * 2 + k] = X[k];
  }
  std::memset(view->table, 0, sizeof(kmc_lag_cell) * (size_t)rows * LAG_CLASSES);
  std::fill(view->n_pairs, view->n_pairs + rows, (int64_t)0);
  std::memset(acc, 0, sizeof *acc);
  acc->cfg = c;
  acc->J = J;
  acc->F = F;
  acc->BX = BX;
  acc->BY = BY;
  acc->origin_step = acc->last_step = v->step;
  acc->rows = rows;
  return KMC_OK;
}

int kmc_host_lag_update(const kmc_params* p, const kmc_state_view* v, const kmc_lag_view* view, kmc_lag_out* acc,
                        kmc_lag_info* info) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !lag_view_ok(view) || !acc) {
    g_host_err = "lag: params, state, the view's seven arrays and acc are needed";
    return KMC_ERR_ARG;
  }
  if (v->step != acc->last_step + acc->cfg.every || acc->n_updates >= INT32_MAX) {
    g_host_err = "lag: an update is due " + std::to_string(acc->cfg.every) + " steps after the last one";
    return KMC_ERR_ARG;
  }
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  const int L = acc->cfg.levels, P = acc->cfg.slots, nq = acc->cfg.nq;
  const int64_t n = acc->n_updates + 1;
  kmcl::Task tasks[LAG_MAX_ROWS];
  const int nt = kmcl::tasks(n, L, P, tasks);
  int64_t n_events = 0;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2], d[2];
    int32_t l[3];
    lag_host_cur(p, v, (int)i, X, l);
    d[0] = kmcl::min_image(X[0] - view->prev[2 * i], acc->BX);
    d[1] = kmcl::min_image(X[1] - view->prev[2 * i + 1], acc->BY);
    int64_t U[2];
    for (int k = 0; k < 2; ++k) {
      U[k] = view->U[2 * i + k] += d[k];
      view->prev[2 * i + k] = X[k];
    }
    bool ev = std::llabs(d[0]) >= acc->J || std::llabs(d[1]) >= acc->J;
    for (int k = 0; k < 3; ++k) {
      int32_t* q = &view->links[(size_t)k * N + i];
      ev = ev || *q != l[k];
      *q = l[k];
    }
    if (ev) {
      view->last_event[i] = (int32_t)n;
      ++n_events;
    }
    const int c = kmcl::cls(i < (size_t)p->n_a, l);
    for (int t = 0; t < nt; ++t) {
      const int64_t* O = &view->ring[((size_t)tasks[t].ring * N + i) * 2];
      const int64_t Dx = U[0] - O[0], Dy = U[1] - O[1];
      kmc_lag_cell* cell = &view->table[(size_t)tasks[t].row * LAG_CLASSES + c];
      if (kmcl::far(Dx, Dy, acc->F)) {
        cell->n_far += 1;
        continue;
      }
      const uint64_t q = kmcl::sq(Dx, Dy);
      cell->n_all += 1;
      lag_add(&cell->m2_all, (__int128)q);
      if (view->last_event[i] > tasks[t].nk) continue;
      cell->n_clean += 1;
      lag_add(&cell->m2_clean, (__int128)q);
      uint64_t a2, ab, b2;
      kmcl::split(q, &a2, &ab, &b2);
      lag_add(&cell->m4_clean, (__int128)kmcl::m4(a2, ab, b2));
      for (int k = 0; k < nq; ++k)
        lag_add(&cell->fs[k], (__int128)kmcl::fs_term(acc->cfg.h[k], Dx, Dy, acc->BX, acc->BY));
    }
    for (int lv = 0; lv < L && kmcl::fires(n, lv); ++lv)
      for (int k = 0; k < 2; ++k) view->ring[((size_t)kmcl::store_ring(n, lv, P) * N + i) * 2 + k] = U[k];
  }
  for (int t = 0; t < nt; ++t) view->n_pairs[tasks[t].row] += 1;
  acc->last_step = v->step;
  acc->n_updates = n;
  if (info) {
    info->n_updates = n;
    info->n_tasks = nt;
    info->n_events = n_events;
  }
  return KMC_OK;
}

int kmc_host_lag_sample(const kmc_params* p, const kmc_lag_view* view, const kmc_lag_out* acc, kmc_lag_out* out,
                        kmc_lag_cell* table, int64_t* n_pairs) {
  if (!p || !lag_view_ok(view) || !acc || !out) {
    g_host_err = "lag sample: params, the view's seven arrays, acc and out are needed";
    return KMC_ERR_ARG;
  }
  const kmc_lag_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (table && table != view->table) std::copy(view->table, view->table + (size_t)a.rows * LAG_CLASSES, table);
  if (n_pairs && n_pairs != view->n_pairs) std::copy(view->n_pairs, view->n_pairs + a.rows, n_pairs);
  return KMC_OK;
}

// Orientation layer (include/kmc.h): kmc_rot_*'s and
// kmc_ligand_pose's definitions on host state views, one protein after the
// other; the vectors, the packing, the pair term and the bins are
// kmc_orient.h's, the ones the device evaluates.  Every sum is taken whole.
extern "C++" {
namespace {

bool rot_view_ok(const kmc_rot_view* w) {
  return w && w->vec && w->links && w->last_event && w->chi && w->ring && w->table && w->n_pairs;
}

// protein i's packed words, handedness and links; false for a bad protein.  Z, Nz as rot_vectors' (kmc_orient.hip)
bool rot_host_cur(const kmc_params* p, const kmc_state_view* v, int i, uint64_t w[2], int* chi, int32_t l[3], int64_t* Z,
                  int64_t* Nz) {
  const int na = p->n_a, nb = p->n_b;
  int64_t X[2];
  lag_host_cur(p, v, i, X, l);
  *chi = 0;
  *Z = *Nz = 0;
  if (i < na) {
    const double b31[2] = {v->ra[RA(na, 3, 1, 0, i)], v->ra[RA(na, 3, 1, 1, i)]};
    const double b32[2] = {v->ra[RA(na, 3, 2, 0, i)], v->ra[RA(na, 3, 2, 1, i)]};
    const kmco::V3 h = kmco::heading(b31, b32);
    const bool ok = kmco::fits(h);
    w[0] = ok ? kmco::pack(h) : ROT_BAD;
    w[1] = 0;
    return ok;
  }
  const int b = i - na;
  double bead[4][3];
  const int jk[4][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 1}};
  for (int m = 0; m < 4; ++m)
    for (int c = 0; c < 3; ++c) bead[m][c] = v->rb[RB(nb, jk[m][0], jk[m][1], c, b)];
  const kmco::Lig g = kmco::ligand(bead[0], bead[1], bead[2], bead[3]);
  const bool ok = kmco::fits(g);
  w[0] = ok ? kmco::pack(g.n) : ROT_BAD;
  w[1] = ok ? kmco::pack(g.a) : ROT_BAD;
  if (ok) *chi = kmco::chi(g.n, g.a, g.c);
  *Z = kmco::q(bead[0][2]);
  *Nz = g.n.z;
  return ok;
}

size_t rot_at(size_t i, int v, size_t na, size_t nb) { return i < na ? i : na + (size_t)v * nb + (i - na); }

}  // namespace
}  // extern "C++"

int kmc_host_rot_begin(const kmc_params* p, const kmc_state_view* v, const kmc_rot_config* cfg,
                       const kmc_rot_view* view, kmc_rot_out* acc) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !cfg || !rot_view_ok(view) || !acc) {
    g_host_err = "rot: params, state, the configuration, the view's seven arrays and acc are needed";
    return KMC_ERR_ARG;
  }
  const kmc_rot_config c = *cfg;
  const char* bad = kmco::check(c.every, c.levels, c.slots);
  if (bad) {
    g_host_err = bad;
    return KMC_ERR_ARG;
  }
  const size_t na = (size_t)p->n_a, nb = (size_t)p->n_b, N = na + nb, W = na + 2 * nb;
  const int L = c.levels, P = c.slots, rows = kmcl::rows(L, P);
  for (size_t i = 0; i < N; ++i) {
    uint64_t w[2];
    int chi;
    int32_t l[3];
    int64_t Z, Nz;
    rot_host_cur(p, v, (int)i, w, &chi, l, &Z, &Nz);
    for (int k = 0; k < (i < na ? 1 : 2); ++k) {
      const size_t at = rot_at(i, k, na, nb);
      view->vec[at] = w[k];
      for (int lv = 0; lv < L; ++lv) view->ring[(size_t)(lv * P) * W + at] = w[k];
    }
    for (int k = 0; k < 3; ++k) view->links[(size_t)k * N + i] = l[k];
    view->last_event[i] = 0;
    view->chi[i] = (int8_t)chi;
  }
  std::memset(view->table, 0, sizeof(kmc_rot_cell) * (size_t)rows * LAG_CLASSES * ROT_VECS);
  std::fill(view->n_pairs, view->n_pairs + rows, (int64_t)0);
  std::memset(acc, 0, sizeof *acc);
  acc->cfg = c;
  acc->origin_step = acc->last_step = v->step;
  acc->rows = rows;
  return KMC_OK;
}

int kmc_host_rot_update(const kmc_params* p, const kmc_state_view* v, const kmc_rot_view* view, kmc_rot_out* acc,
                        kmc_rot_info* info) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !rot_view_ok(view) || !acc) {
    g_host_err = "rot: params, state, the view's seven arrays and acc are needed";
    return KMC_ERR_ARG;
  }
  if (v->step != acc->last_step + acc->cfg.every || acc->n_updates >= INT32_MAX) {
    g_host_err = "rot: an update is due " + std::to_string(acc->cfg.every) + " steps after the last one";
    return KMC_ERR_ARG;
  }
  const size_t na = (size_t)p->n_a, nb = (size_t)p->n_b, N = na + nb, W = na + 2 * nb;
  const int L = acc->cfg.levels, P = acc->cfg.slots;
  const int64_t n = acc->n_updates + 1;
  kmcl::Task tasks[LAG_MAX_ROWS];
  const int nt = kmcl::tasks(n, L, P, tasks);
  int64_t n_events = 0, n_flips = 0, n_bad = 0;
  for (size_t i = 0; i < N; ++i) {
    uint64_t w[2];
    int chi;
    int32_t l[3];
    int64_t Z, Nz;
    const bool ok = rot_host_cur(p, v, (int)i, w, &chi, l, &Z, &Nz);
    const int nv = i < na ? 1 : 2;
    if (!ok) ++n_bad;
    const bool flip = view->chi[i] != (int8_t)chi;
    view->chi[i] = (int8_t)chi;
    bool ev = flip;
    for (int k = 0; k < 3; ++k) {
      int32_t* q = &view->links[(size_t)k * N + i];
      ev = ev || *q != l[k];
      *q = l[k];
    }
    if (flip) ++n_flips;
    if (ev) {
      view->last_event[i] = (int32_t)n;
      ++n_events;
    }
    const int c = kmcl::cls(i < na, l);
    for (int k = 0; k < nv; ++k) {
      const size_t at = rot_at(i, k, na, nb);
      view->vec[at] = w[k];
      const kmco::V3 u = kmco::unpack(w[k]);
      for (int t = 0; ok && t < nt; ++t) {
        const uint64_t o = view->ring[(size_t)tasks[t].ring * W + at];
        if (o & ROT_BAD) continue;
        const int64_t d = kmco::dot(u, kmco::unpack(o));
        kmc_rot_cell* cell = &view->table[((size_t)tasks[t].row * LAG_CLASSES + c) * ROT_VECS + k];
        cell->n_all += 1;
        lag_add(&cell->s1_all, (__int128)d);
        if (view->last_event[i] > tasks[t].nk) continue;
        cell->n_clean += 1;
        lag_add(&cell->s1_clean, (__int128)d);
        uint64_t a2, ab, b2;
        kmco::split(d, &a2, &ab, &b2);
        lag_add(&cell->s2_clean, (__int128)kmco::sq(a2, ab, b2));
      }
      for (int lv = 0; lv < L && kmcl::fires(n, lv); ++lv) view->ring[(size_t)kmcl::store_ring(n, lv, P) * W + at] = w[k];
    }
  }
  for (int t = 0; t < nt; ++t) view->n_pairs[tasks[t].row] += 1;
  acc->last_step = v->step;
  acc->n_updates = n;
  if (info) {
    info->n_updates = n;
    info->n_tasks = nt;
    info->n_events = n_events;
    info->n_flips = n_flips;
    info->n_bad = n_bad;
  }
  return KMC_OK;
}

int kmc_host_rot_sample(const kmc_params* p, const kmc_rot_view* view, const kmc_rot_out* acc, kmc_rot_out* out,
                        kmc_rot_cell* table, int64_t* n_pairs) {
  if (!p || !rot_view_ok(view) || !acc || !out) {
    g_host_err = "rot sample: params, the view's seven arrays, acc and out are needed";
    return KMC_ERR_ARG;
  }
  const kmc_rot_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (table && table != view->table)
    std::copy(view->table, view->table + (size_t)a.rows * LAG_CLASSES * ROT_VECS, table);
  if (n_pairs && n_pairs != view->n_pairs) std::copy(view->n_pairs, view->n_pairs + a.rows, n_pairs);
  return KMC_OK;
}

int kmc_host_ligand_pose(const kmc_params* p, const kmc_state_view* v, int32_t nz, int32_t nc, int64_t* hist,
                         kmc_pose_out* out) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !out) {
    g_host_err = "pose: params, state and out are needed";
    return KMC_ERR_ARG;
  }
  int64_t BZ, Lq;
  const char* bad = kmco::pose_check(nz, nc, p->box_z, p->rb_radius, &BZ, &Lq);
  if (bad) {
    g_host_err = bad;
    return KMC_ERR_ARG;
  }
  if (hist) std::fill(hist, hist + (size_t)POSE_CLASSES * nz * nc, (int64_t)0);
  std::memset(out, 0, sizeof *out);
  for (int b = 0; b < p->n_b; ++b) {
    uint64_t w[2];
    int chi;
    int32_t l[3];
    int64_t Z, Nz;
    const bool ok = rot_host_cur(p, v, p->n_a + b, w, &chi, l, &Z, &Nz);
    const int k = (l[0] != 0) + (l[1] != 0) + (l[2] != 0);
    if (!ok) {
      out->n_bad += 1;
      continue;
    }
    if (chi > 0) out->chi_pos[k] += 1;
    if (chi < 0) out->chi_neg[k] += 1;
    if (hist) hist[((size_t)k * nz + kmco::pose_zbin(Z, BZ, nz)) * nc + kmco::pose_tbin(Nz, Lq, nc)] += 1;
  }
  return KMC_OK;
}

// Pair dynamics (include/kmc.h): kmc_pd_*'s definitions on host
// state views, one protein and one pair after the other; the fold, the cell,
// the bin, the validity and the terms are kmc_pairdyn.h's, the ones the device
// evaluates.  The sample sorts both point sets by cell (a counting sort of its
// own) and walks the 3 x 3 block for part A and the half shell for part B.
extern "C++" {
namespace {

bool pd_view_ok(const kmc_pd_view* w) { return w && w->prev && w->U && w->X0 && w->flags; }

// the configuration in acc resolved again: the grid and the edges (they were checked at begin)
const char* pd_grid(const kmc_params* p, const kmc_pd_out* acc, kmcp::Grid* G, int64_t* E) {
  double mj = acc->cfg.max_jump, md = acc->cfg.max_disp;
  return kmcp::check(acc->cfg.every, acc->cfg.nbins, acc->cfg.r_max, p->box_x, p->box_y, &mj, &md, G, E);
}

// points sorted by cell: start[ncell + 1], order[N] (the point indices of cell c are order[start[c] .. start[c + 1]))
struct PdCells {
  std::vector<int32_t> start, order, cx, cy;
  std::vector<int64_t> fx, fy;
  void build(const int64_t* X, size_t N, const kmcp::Grid& G) {
    const size_t ncell = (size_t)G.ncx * G.ncy;
    start.assign(ncell + 1, 0);
    order.resize(N);
    cx.resize(N);
    cy.resize(N);
    fx.resize(N);
    fy.resize(N);
    for (size_t i = 0; i < N; ++i) {
      fx[i] = kmcp::fold(X[2 * i], G.BX);
      fy[i] = kmcp::fold(X[2 * i + 1], G.BY);
      cx[i] = kmcp::cell(fx[i], G.ncx, G.BX);
      cy[i] = kmcp::cell(fy[i], G.ncy, G.BY);
      start[(size_t)cy[i] * G.ncx + cx[i] + 1] += 1;
    }
    for (size_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
    std::vector<int32_t> at(start.begin(), start.end() - 1);
    for (size_t i = 0; i < N; ++i) order[at[(size_t)cy[i] * G.ncx + cx[i]]++] = (int32_t)i;
  }
};

}  // namespace
}  // extern "C++"

int kmc_host_pd_begin(const kmc_params* p, const kmc_state_view* v, const kmc_pd_config* cfg, const kmc_pd_view* view,
                      kmc_pd_out* acc) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !cfg || !pd_view_ok(view) || !acc) {
    g_host_err = "pd: params, state, the configuration, the view's four arrays and acc are needed";
    return KMC_ERR_ARG;
  }
  kmc_pd_config c = *cfg;
  kmcp::Grid G;
  int64_t E[PD_MAX_BINS + 1];
  const char* bad = kmcp::check(c.every, c.nbins, c.r_max, p->box_x, p->box_y, &c.max_jump, &c.max_disp, &G, E);
  if (bad) {
    g_host_err = bad;
    return KMC_ERR_ARG;
  }
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    lag_host_cur(p, v, (int)i, X, l);
    for (int k = 0; k < 2; ++k) view->prev[2 * i + k] = view->U[2 * i + k] = view->X0[2 * i + k] = X[k];
    view->flags[i] = 0;
  }
  std::memset(acc, 0, sizeof *acc);
  acc->cfg = c;
  acc->J = G.J;
  acc->F = G.F;
  acc->BX = G.BX;
  acc->BY = G.BY;
  acc->ncx = G.ncx;
  acc->ncy = G.ncy;
  acc->origin_step = acc->last_step = v->step;
  return KMC_OK;
}

int kmc_host_pd_update(const kmc_params* p, const kmc_state_view* v, const kmc_pd_view* view, kmc_pd_out* acc,
                       kmc_pd_info* info) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !pd_view_ok(view) || !acc) {
    g_host_err = "pd: params, state, the view's four arrays and acc are needed";
    return KMC_ERR_ARG;
  }
  if (v->step != acc->last_step + acc->cfg.every) {
    g_host_err = "pd: an update is due " + std::to_string(acc->cfg.every) + " steps after the last one";
    return KMC_ERR_ARG;
  }
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  int64_t n_jumped = 0;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    lag_host_cur(p, v, (int)i, X, l);
    const int64_t B[2] = {acc->BX, acc->BY};
    for (int k = 0; k < 2; ++k) {
      const int64_t d = kmcl::min_image(X[k] - view->prev[2 * i + k], B[k]);
      view->U[2 * i + k] += d;
      view->prev[2 * i + k] = X[k];
      if (std::llabs(d) >= acc->J) view->flags[i] |= PD_JUMPED;
    }
    n_jumped += view->flags[i] & PD_JUMPED;
  }
  acc->last_step = v->step;
  acc->n_updates += 1;
  if (info) {
    info->n_updates = acc->n_updates;
    info->n_jumped = n_jumped;
  }
  return KMC_OK;
}

int kmc_host_pd_sample(const kmc_params* p, const kmc_pd_view* view, const kmc_pd_out* acc, kmc_pd_out* out, int64_t* gd,
                       int64_t* gs, kmc_pd_cell* cu) {
  if (!p || !pd_view_ok(view) || !acc || !out) {
    g_host_err = "pd sample: params, the view's four arrays, acc and out are needed";
    return KMC_ERR_ARG;
  }
  kmcp::Grid G;
  int64_t E[PD_MAX_BINS + 1];
  const char* bad = pd_grid(p, acc, &G, E);
  if (bad) {
    g_host_err = bad;
    return KMC_ERR_ARG;
  }
  const kmc_pd_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (!gd && !gs && !cu) return KMC_OK;
  const int nb = G.nbins, na = p->n_a;
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  uint64_t E2[PD_MAX_BINS + 1];
  for (int m = 0; m <= nb; ++m) E2[m] = (uint64_t)E[m] * (uint64_t)E[m];
  if (gd) std::fill(gd, gd + 4 * (size_t)nb, (int64_t)0);
  if (gs) std::fill(gs, gs + 2 * (size_t)nb, (int64_t)0);
  if (cu) std::memset(cu, 0, sizeof(kmc_pd_cell) * 3 * (size_t)nb);
  PdCells o, w;
  o.build(view->X0, N, G);
  if (gd || gs) {
    w.build(view->U, N, G);
    for (size_t i = 0; i < N; ++i) {
      const int si = (int)i >= na;
      for (int q = 0; q < 9; ++q) {
        const int jx = (o.cx[i] + q % 3 - 1 + G.ncx) % G.ncx, jy = (o.cy[i] + q / 3 - 1 + G.ncy) % G.ncy;
        const size_t jc = (size_t)jy * G.ncx + jx;
        for (int32_t t = w.start[jc]; t < w.start[jc + 1]; ++t) {
          const size_t j = (size_t)w.order[t];
          const int k = kmcp::bin(E2, nb, kmcp::d2(kmcl::min_image(w.fx[j] - o.fx[i], G.BX),
                                                   kmcl::min_image(w.fy[j] - o.fy[i], G.BY)));
          if (k >= nb) continue;
          if (i == j) {
            if (gs) gs[(size_t)si * nb + k] += 1;
          } else if (gd) {
            gd[(size_t)kmcp::kind_a(si, (int)j >= na) * nb + k] += 1;
          }
        }
      }
    }
  }
  if (cu) {
    for (int cy = 0; cy < G.ncy; ++cy)
      for (int cx = 0; cx < G.ncx; ++cx) {
        const size_t c = (size_t)cy * G.ncx + cx;
        for (int q = 0; q < 5; ++q) {
          int ox, oy;
          kmcp::half_shell(q, &ox, &oy);
          const size_t jc = (size_t)((cy + oy + G.ncy) % G.ncy) * G.ncx + (cx + ox + G.ncx) % G.ncx;
          for (int32_t ta = o.start[c]; ta < o.start[c + 1]; ++ta)
            for (int32_t tb = q == 0 ? ta + 1 : o.start[jc]; tb < o.start[jc + 1]; ++tb) {
              const size_t i = (size_t)o.order[ta], j = (size_t)o.order[tb];
              const int k = kmcp::bin(E2, nb, kmcp::d2(kmcl::min_image(o.fx[j] - o.fx[i], G.BX),
                                                       kmcl::min_image(o.fy[j] - o.fy[i], G.BY)));
              if (k >= nb) continue;
              kmc_pd_cell* cell = &cu[(size_t)kmcp::kind_b((int)i >= na, (int)j >= na) * nb + k];
              cell->n_pairs += 1;
              const int64_t uix = view->U[2 * i] - view->X0[2 * i], uiy = view->U[2 * i + 1] - view->X0[2 * i + 1];
              const int64_t ujx = view->U[2 * j] - view->X0[2 * j], ujy = view->U[2 * j + 1] - view->X0[2 * j + 1];
              if (!kmcp::valid(view->flags[i], uix, uiy, G.F) || !kmcp::valid(view->flags[j], ujx, ujy, G.F)) continue;
              cell->n_valid += 1;
              lag_add(&cell->dot, (__int128)kmcp::dot(uix, uiy, ujx, ujy));
              lag_add(&cell->sq, (__int128)kmcp::sq(uix, uiy, ujx, ujy));
            }
        }
      }
  }
  return KMC_OK;
}

// Body dynamics (include/kmc.h), sequential: the bodies are the components of
// kmc_host_cluster_geometry at the begin, with its image shifts; the
// per-protein step is the lag correlator's; the sample labels the current
// components (kmc_host_census) and walks each body's members in index order.
// C and S are summed as include/kmc.h defines them, member by member with D =
// D0 + u - u_r — not through the device's rearrangement; the verdict's bounds
// and the rotation terms are kmc_bodydyn.h's.
extern "C++" {
namespace {

bool bd_view_ok(const kmc_bd_view* w) {
  return w && w->prev && w->U && w->X0 && w->links && w->flags && w->label && w->D0 && w->bits;
}

// one row per body, in label order, from the view and the current state
int bd_host_rows(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* w, const kmc_bd_out* acc,
                 std::vector<kmc_bd_body>* rows) {
  const int na = p->n_a, n = p->n_a + p->n_b;
  std::vector<int32_t> cur((size_t)n), size((size_t)n + 1, 0);
  kmc_census census;
  const int rc = kmc_host_census(p, v, cur.data(), 0, 0, nullptr, &census);
  if (rc != KMC_OK) return rc;
  for (int i = 0; i < n; ++i) size[(size_t)cur[i]] += 1;
  // the members of every body, in index order: a counting sort by label
  std::vector<int32_t> start((size_t)n + 2, 0), order((size_t)n);
  for (int i = 0; i < n; ++i) start[(size_t)w->label[i] + 1] += 1;
  for (int r = 1; r <= n; ++r) start[(size_t)r + 1] += start[r];
  std::vector<int32_t> at(start.begin(), start.end() - 1);
  for (int i = 0; i < n; ++i) order[(size_t)at[(size_t)w->label[i]]++] = i;
  rows->clear();
  for (int r = 1; r <= n; ++r) {
    const int m = start[(size_t)r + 1] - start[r];
    if (!m) continue;
    const int32_t* mem = &order[(size_t)start[r]];
    kmc_bd_body b;
    std::memset(&b, 0, sizeof b);
    b.label = r;
    b.bits = w->bits[r - 1];
    int orbits = 0, lmin = n + 1, lmax = 0;
    for (int t = 0; t < m; ++t) {
      const size_t i = (size_t)mem[t];
      ((int)i < na ? b.n_r : b.n_l) += 1;
      orbits |= kmcb::member_bits(w->flags[i], w->U[2 * i] - w->X0[2 * i], w->U[2 * i + 1] - w->X0[2 * i + 1], acc->F);
      lmin = std::min(lmin, (int)cur[i]);
      lmax = std::max(lmax, (int)cur[i]);
    }
    b.cur_label = lmin;
    b.cur_size = size[(size_t)lmin];
    b.status = lmin != lmax ? KMC_BD_BROKEN : b.cur_size == m ? KMC_BD_INTACT : KMC_BD_GROWN;
    if (!(orbits & (BD_JUMPED | BD_CHANGED))) b.is |= KMC_BD_IS_PRISTINE;
    if (!orbits) {
      b.is |= KMC_BD_IS_VALID;
      const size_t q = (size_t)r - 1;
      const int64_t ur[2] = {w->U[2 * q] - w->X0[2 * q], w->U[2 * q + 1] - w->X0[2 * q + 1]};
      const bool rot = m >= 2 && m <= KMC_BD_ROT_MAX && !b.bits;
      for (int t = 0; t < m; ++t) {
        const size_t i = (size_t)mem[t];
        const int64_t u[2] = {w->U[2 * i] - w->X0[2 * i], w->U[2 * i + 1] - w->X0[2 * i + 1]};
        b.su[0] += u[0];
        b.su[1] += u[1];
        if (!rot) continue;
        const int64_t d0[2] = {w->D0[2 * i], w->D0[2 * i + 1]};
        const int64_t d[2] = {d0[0] + u[0] - ur[0], d0[1] + u[1] - ur[1]};
        b.C += d0[0] * d[0] + d0[1] * d[1];
        b.S += d0[0] * d[1] - d0[1] * d[0];
      }
      if (rot) b.is |= KMC_BD_IS_ROT;
    }
    rows->push_back(b);
  }
  return KMC_OK;
}

}  // namespace
}  // extern "C++"

int kmc_host_bd_begin(const kmc_params* p, const kmc_state_view* v, const kmc_bd_config* cfg, const kmc_bd_view* view,
                      kmc_bd_out* acc) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !cfg || !bd_view_ok(view) || !acc) {
    g_host_err = "bd: params, state, the configuration, the view's eight arrays and acc are needed";
    return KMC_ERR_ARG;
  }
  kmc_bd_config c = *cfg;
  int64_t J, F, BX, BY;
  const char* bad = kmcb::check(c.every, c.max_size, p->box_x, p->box_y, &c.max_jump, &c.max_disp, &J, &F, &BX, &BY);
  if (bad) {
    g_host_err = bad;
    return KMC_ERR_ARG;
  }
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  std::vector<int32_t> shift(2 * N + 1);
  kmc_geom geom;
  const int rc = kmc_host_cluster_geometry(p, v, view->label, shift.data(), view->bits, 2, nullptr, &geom);
  if (rc != KMC_OK) return rc;
  int64_t n_bodies = 0;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    lag_host_cur(p, v, (int)i, X, l);
    for (int k = 0; k < 2; ++k) view->prev[2 * i + k] = view->U[2 * i + k] = view->X0[2 * i + k] = X[k];
    for (int k = 0; k < 3; ++k) view->links[(size_t)k * N + i] = l[k];
    view->flags[i] = 0;
    n_bodies += view->label[i] == (int32_t)i + 1;
  }
  for (size_t i = 0; i < N; ++i) {
    const size_t r = (size_t)view->label[i] - 1;
    view->D0[2 * i] = view->X0[2 * i] + (int64_t)shift[i] * BX - view->X0[2 * r];
    view->D0[2 * i + 1] = view->X0[2 * i + 1] + (int64_t)shift[N + i] * BY - view->X0[2 * r + 1];
  }
  // a body is WIDE by any of its members: the bit goes to all of them
  std::vector<uint8_t> wide(N, 0);
  for (size_t i = 0; i < N; ++i)
    if (kmcb::wide(view->D0[2 * i], view->D0[2 * i + 1])) wide[(size_t)view->label[i] - 1] = 1;
  for (size_t i = 0; i < N; ++i)
    if (wide[(size_t)view->label[i] - 1]) view->bits[i] |= KMC_BD_WIDE;
  std::memset(acc, 0, sizeof *acc);
  acc->cfg = c;
  acc->J = J;
  acc->F = F;
  acc->BX = BX;
  acc->BY = BY;
  acc->origin_step = acc->last_step = v->step;
  acc->n_bodies = n_bodies;
  return KMC_OK;
}

int kmc_host_bd_update(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, kmc_bd_out* acc,
                       kmc_bd_info* info) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || !bd_view_ok(view) || !acc) {
    g_host_err = "bd: params, state, the view's eight arrays and acc are needed";
    return KMC_ERR_ARG;
  }
  if (v->step != acc->last_step + acc->cfg.every) {
    g_host_err = "bd: an update is due " + std::to_string(acc->cfg.every) + " steps after the last one";
    return KMC_ERR_ARG;
  }
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  const int64_t B[2] = {acc->BX, acc->BY};
  int64_t n_jumped = 0, n_changed = 0;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    lag_host_cur(p, v, (int)i, X, l);
    int f = 0;
    for (int k = 0; k < 2; ++k) {
      const int64_t d = kmcl::min_image(X[k] - view->prev[2 * i + k], B[k]);
      view->U[2 * i + k] += d;
      view->prev[2 * i + k] = X[k];
      if (std::llabs(d) >= acc->J) f |= BD_JUMPED;
    }
    for (int k = 0; k < 3; ++k) {
      int32_t* q = &view->links[(size_t)k * N + i];
      if (*q != l[k]) f |= BD_CHANGED;
      *q = l[k];
    }
    const int fresh = f & ~view->flags[i];
    n_jumped += (fresh & BD_JUMPED) != 0;
    n_changed += (fresh & BD_CHANGED) != 0;
    view->flags[i] |= (uint8_t)f;
  }
  acc->last_step = v->step;
  acc->n_updates += 1;
  if (info) {
    info->n_updates = acc->n_updates;
    info->n_jumped = n_jumped;
    info->n_changed = n_changed;
  }
  return KMC_OK;
}

int kmc_host_bd_sample(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, const kmc_bd_out* acc,
                       kmc_bd_out* out, kmc_bd_cell* table) {
  if (!p || !v || !v->a_int || !v->b_int || !bd_view_ok(view) || !acc || !out) {
    g_host_err = "bd sample: params, state, the view's eight arrays, acc and out are needed";
    return KMC_ERR_ARG;
  }
  if (v->step != acc->last_step) {
    g_host_err = "bd sample: the state has moved on since the last update (an update is due first)";
    return KMC_ERR_ARG;
  }
  const kmc_bd_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (!table) return KMC_OK;
  std::vector<kmc_bd_body> rows;
  const int rc = bd_host_rows(p, v, view, &a, &rows);
  if (rc != KMC_OK) return rc;
  const int ms = a.cfg.max_size;
  std::memset(table, 0, sizeof(kmc_bd_cell) * 2 * ((size_t)ms + 1));
  for (const kmc_bd_body& b : rows) {
    const int n = b.n_r + b.n_l;
    kmc_bd_cell* c = &table[(size_t)(b.n_l > 0) * (ms + 1) + std::min(n, ms)];
    c->n_bodies += 1;
    c->sum_size += n;
    (b.status == KMC_BD_INTACT ? c->n_intact : b.status == KMC_BD_GROWN ? c->n_grown : c->n_broken) += 1;
    if (b.is & KMC_BD_IS_PRISTINE) c->n_pristine += 1;
    if (!(b.is & KMC_BD_IS_VALID)) continue;
    c->n_valid += 1;
    lag_add(&c->m2, (__int128)kmcb::trans_term(b.su[0], b.su[1]));
    if (!(b.is & KMC_BD_IS_ROT)) {
      if (n >= 2) c->n_rot_skipped += 1;
      continue;
    }
    if (b.C == 0 && b.S == 0) {
      c->n_rot_null += 1;
      continue;
    }
    int64_t c1, c2, ph;
    kmcb::rot_terms(b.C, b.S, &c1, &c2, &ph);
    c->n_rot += 1;
    c->c1 += c1;
    c->c2 += c2;
    lag_add(&c->phi2, (__int128)(ph * ph));
  }
  return KMC_OK;
}

int kmc_host_bd_bodies(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, const kmc_bd_out* acc,
                       int32_t min_size, int64_t cap, kmc_bd_body* rows, int64_t* n) {
  if (!p || !v || !v->a_int || !v->b_int || !bd_view_ok(view) || !acc || !n || min_size < 1 || cap < 0 ||
      (cap > 0 && !rows)) {
    g_host_err = "bd bodies: params, state, the view, acc and n are needed, min_size >= 1, cap >= 0, rows for cap > 0";
    return KMC_ERR_ARG;
  }
  if (v->step != acc->last_step) {
    g_host_err = "bd bodies: the state has moved on since the last update (an update is due first)";
    return KMC_ERR_ARG;
  }
  std::vector<kmc_bd_body> all;
  const int rc = bd_host_rows(p, v, view, acc, &all);
  if (rc != KMC_OK) return rc;
  *n = 0;
  for (const kmc_bd_body& b : all)
    if (b.n_r + b.n_l >= min_size) {
      if (*n < cap) rows[*n] = b;
      *n += 1;
    }
  if (*n > cap) {
    g_host_err = "bd bodies: " + std::to_string(*n) + " bodies qualify, cap is " + std::to_string(cap);
    return KMC_ERR_CAPACITY;
  }
  return KMC_OK;
}

// Encounter statistics (include/kmc.h): kmc_reach_census' and
// kmc_enc_*'s definitions on host state views by brute force over all pairs;
// the gates, the bin rules and the slot transition are kmc_encounter.h's, the
// ones the device evaluates.
extern "C++" {
namespace {

struct EncHost {
  const kmc_params* p;
  const kmc_state_view* v;
  int na, nb;
  double T_bond, T_cis;
  kmce::V3 a(int i, int j, int k) const {
    const size_t o = (size_t)((j - 1) * 4 + (k - 1)) * 3;
    return kmce::V3{v->ra[(o + 0) * na + i], v->ra[(o + 1) * na + i], v->ra[(o + 2) * na + i]};
  }
  kmce::V3 b(int q, int j, int k) const {
    const size_t o = (size_t)((j - 1) * 2 + (k - 1)) * 3;
    return kmce::V3{v->rb[(o + 0) * nb + q], v->rb[(o + 1) * nb + q], v->rb[(o + 2) * nb + q]};
  }
  int st2(int i) const { return v->a_int[0 * (size_t)na + i]; }
  int st3(int i) const { return v->a_int[1 * (size_t)na + i]; }
  int stb(int q, int k) const { return v->b_int[(size_t)(k - 1) * nb + q]; }
};

bool enc_host_open(const kmc_params* p, const kmc_state_view* v, EncHost* h) {
  if (!p || !v || !v->ra || !v->rb || !v->a_int || !v->b_int || p->n_a < 0 || p->n_b < 0) return false;
  h->p = p;
  h->v = v;
  h->na = p->n_a;
  h->nb = p->n_b;
  h->T_bond = kmce::sqrt_threshold(p->bond_dist_cutoff);
  h->T_cis = kmce::sqrt_threshold(p->cis_dist_cutoff);
  return true;
}

// the R–L triple (i, q, k), all 0-based but k: in reach (then *q2, *pd, *ot are set)
bool enc_host_rl(const EncHost& h, int i, int q, int k, double* q2, double* pd, double* ot) {
  const kmce::V3 s = h.a(i, 3, 2), t = h.b(q, k, 2);
  *q2 = kmce::d2(t.x - s.x, t.y - s.y, t.z - s.z);
  if (!(*q2 < h.T_bond)) return false;
  kmce::rl_angles(h.a(i, 3, 1), s, h.a(i, 3, 4), h.b(q, k, 1), t, h.b(q, 1, 1), h.b(q, 1, 2), pd, ot);
  return true;
}

bool enc_view_ok(const kmc_enc_view* w) { return w && w->lig && w->site && w->key && w->since && w->nreact && w->flags; }

// receptor i's (0-based) current look, checked as the device checks it
bool enc_host_cur(const EncHost& h, int i, int slots, kmce::Cur* c) {
  kmck::Cur l;
  bool ok = kin_host_cur(h.p, h.v, i, &l);
  if (ok && l.lig != 0 && (l.site < 2 || l.site > 4)) ok = false;
  kmce::cur_clear(*c, ok ? l.lig : 0, ok && l.lig != 0 ? l.site : 0);
  if (!ok) return false;
  if (h.st2(i) != 0) return true;
  for (int q = 0; q < h.nb; ++q)
    for (int k = 2; k <= 4; ++k) {
      if (h.stb(q, k) != 0) continue;
      double q2, pd, ot;
      if (!enc_host_rl(h, i, q, k, &q2, &pd, &ot)) continue;
      kmce::cur_add(*c, slots, kmce::key_of(q + 1, k), pd < h.p->bond_thetapd_cutoff && ot < h.p->bond_thetaot_cutoff);
    }
  return true;
}

kmce::Slots enc_load(const kmc_enc_view* w, int i) {
  kmce::Slots r;
  r.lig = w->lig[i];
  r.site = w->site[i];
  for (int s = 0; s < ENC_SLOTS; ++s) {
    r.key[s] = w->key[(size_t)i * ENC_SLOTS + s];
    r.since[s] = w->since[(size_t)i * ENC_SLOTS + s];
    r.nreact[s] = w->nreact[(size_t)i * ENC_SLOTS + s];
    r.flags[s] = w->flags[(size_t)i * ENC_SLOTS + s];
  }
  return r;
}

void enc_store(const kmc_enc_view* w, int i, const kmce::Slots& r) {
  w->lig[i] = r.lig;
  w->site[i] = r.site;
  for (int s = 0; s < ENC_SLOTS; ++s) {
    w->key[(size_t)i * ENC_SLOTS + s] = r.key[s];
    w->since[(size_t)i * ENC_SLOTS + s] = r.since[s];
    w->nreact[(size_t)i * ENC_SLOTS + s] = r.nreact[s];
    w->flags[(size_t)i * ENC_SLOTS + s] = r.flags[s];
  }
}

void enc_set_occ(kmc_enc_out* acc, const int64_t cnt[kmce::ENC_NCNT]) {
  acc->occ_reach = cnt[kmce::C_OCC_REACH];
  acc->occ_reactive = cnt[kmce::C_OCC_REACTIVE];
  acc->occ_free_receptor = cnt[kmce::C_OCC_FREE];
}

}  // namespace
}  // extern "C++"

int kmc_host_reach_census(const kmc_params* p, const kmc_state_view* v, int32_t nd, int32_t na, kmc_reach_out* out,
                          int64_t* hist_d, int64_t* hist_a_rl, int64_t* hist_a_cis) {
  EncHost h;
  if (!enc_host_open(p, v, &h) || !out) {
    g_host_err = "reach census: params, the state's four arrays and out are needed";
    return KMC_ERR_ARG;
  }
  if (nd < 1 || nd > ENC_MAX_ND || na < 1 || na > ENC_MAX_NA) {
    g_host_err = "reach census: 1 <= nd <= 64 and 1 <= na <= 36";
    return KMC_ERR_ARG;
  }
  double E2[ENC_CHANNELS][ENC_MAX_ND];
  kmce::edges(p->bond_dist_cutoff, nd, E2[kmce::CH_RL]);
  kmce::edges(p->cis_dist_cutoff, nd, E2[kmce::CH_MONO]);
  kmce::edges(p->cis_dist_cutoff, nd, E2[kmce::CH_CX]);
  std::memset(out, 0, sizeof *out);
  if (hist_d) std::fill(hist_d, hist_d + (size_t)ENC_CHANNELS * 2 * nd, (int64_t)0);
  if (hist_a_rl) std::fill(hist_a_rl, hist_a_rl + (size_t)na * na, (int64_t)0);
  if (hist_a_cis) std::fill(hist_a_cis, hist_a_cis + (size_t)2 * na, (int64_t)0);
  auto file = [&](int ch, bool react, double q2) {
    out->n_reach[ch] += 1;
    out->n_reactive[ch] += react ? 1 : 0;
    if (hist_d) hist_d[(size_t)(ch * 2 + (react ? 1 : 0)) * nd + kmce::dist_bin(E2[ch], nd, q2)] += 1;
  };
  std::vector<uint8_t> site_hit((size_t)3 * h.nb, 0);
  for (int q = 0; q < h.nb; ++q)
    for (int k = 2; k <= 4; ++k) out->rl_free_sites += h.stb(q, k) == 0 ? 1 : 0;
  for (int i = 0; i < h.na; ++i) {
    if (h.st2(i) != 0) continue;
    out->rl_free_receptors += 1;
    int64_t partners = 0;
    for (int q = 0; q < h.nb; ++q)
      for (int k = 2; k <= 4; ++k) {
        if (h.stb(q, k) != 0) continue;
        double q2, pd, ot;
        if (!enc_host_rl(h, i, q, k, &q2, &pd, &ot)) continue;
        file(kmce::CH_RL, pd < p->bond_thetapd_cutoff && ot < p->bond_thetaot_cutoff, q2);
        if (hist_a_rl) hist_a_rl[(size_t)kmce::ang_bin(pd, na) * na + kmce::ang_bin(ot, na)] += 1;
        site_hit[(size_t)3 * q + (k - 2)] = 1;
        partners += 1;
      }
    out->rl_receptors_in_reach += partners > 0 ? 1 : 0;
    out->rl_max_partners = std::max(out->rl_max_partners, partners);
  }
  for (uint8_t f : site_hit) out->rl_sites_in_reach += f;
  for (int i = 0; i < h.na; ++i) {
    if (h.st3(i) != 0) continue;
    for (int j = i + 1; j < h.na; ++j) {
      if (h.st3(j) != 0) continue;
      const kmce::V3 si = h.a(i, 3, 3), sj = h.a(j, 3, 3);
      const double q2 = kmce::d2(sj.x - si.x, sj.y - si.y, sj.z - si.z);
      if (!(q2 < h.T_cis)) continue;
      const double ot = kmce::cis_angle(h.a(i, 3, 1), si, h.a(j, 3, 1), sj);
      const int ch = h.st2(i) != 0 || h.st2(j) != 0 ? kmce::CH_CX : kmce::CH_MONO;
      file(ch, ot < p->cis_thetaot_cutoff, q2);
      if (hist_a_cis) hist_a_cis[(size_t)(ch - kmce::CH_MONO) * na + kmce::ang_bin(ot, na)] += 1;
    }
  }
  return KMC_OK;
}

int kmc_host_enc_begin(const kmc_params* p, const kmc_state_view* v, const kmc_enc_config* cfg,
                       const kmc_enc_view* view, kmc_enc_out* acc, int64_t* hist10) {
  EncHost h;
  if (!enc_host_open(p, v, &h) || !cfg || !enc_view_ok(view) || !acc || !hist10) {
    g_host_err = "enc: params, state, the configuration, the view's six arrays, acc and hist are needed";
    return KMC_ERR_ARG;
  }
  if (cfg->every < 1) {
    g_host_err = "enc: every >= 1";
    return KMC_ERR_ARG;
  }
  // debug: fewer slots are kept per receptor
  const char* e = getenv("KMC_DEBUG_ENC_SLOTS");
  const int slots = e && *e ? std::max(1, std::min(ENC_SLOTS, atoi(e))) : ENC_SLOTS;
  int64_t cnt[kmce::ENC_NCNT] = {0};
  std::vector<kmce::Slots> recs((size_t)h.na);
  for (int i = 0; i < h.na; ++i) {
    kmce::Cur c;
    if (!enc_host_cur(h, i, slots, &c)) {
      g_host_err = "enc: a receptor's bond link leaves its range";
      return KMC_ERR_STATE;
    }
    int32_t m[kmce::ENC_NCNT] = {0};
    kmce::begin(v->step, c, recs[(size_t)i], m);
    for (int k = 0; k < kmce::ENC_NCNT; ++k) cnt[k] += m[k];
  }
  for (int i = 0; i < h.na; ++i) enc_store(view, i, recs[(size_t)i]);
  std::memset(acc, 0, sizeof *acc);
  std::fill(hist10, hist10 + (size_t)ENC_ACC_ROWS * ENC_BINS, (int64_t)0);
  acc->origin_step = acc->last_step = v->step;
  acc->n_overflow = cnt[kmce::C_OVERFLOW];
  acc->every = cfg->every;
  acc->slots = slots;
  enc_set_occ(acc, cnt);
  return KMC_OK;
}

int kmc_host_enc_update(const kmc_params* p, const kmc_state_view* v, const kmc_enc_view* view, kmc_enc_out* acc,
                        int64_t* hist10) {
  EncHost h;
  if (!enc_host_open(p, v, &h) || !enc_view_ok(view) || !acc || !hist10) {
    g_host_err = "enc: params, state, the view's six arrays, acc and hist are needed";
    return KMC_ERR_ARG;
  }
  const int64_t t = v->step, dt = t - acc->last_step;
  if (dt == 0) {  // a second update at the same step moves only the count
    acc->n_updates += 1;
    return KMC_OK;
  }
  if (dt != acc->every) {
    g_host_err = "enc: an update is due " + std::to_string(acc->every) + " steps after the last one";
    return KMC_ERR_ARG;
  }
  const int slots = (int)acc->slots;
  std::vector<kmce::Cur> cur((size_t)h.na);
  for (int i = 0; i < h.na; ++i)  // checked first: a failed call leaves the recorder as it was
    if (!enc_host_cur(h, i, slots, &cur[(size_t)i])) {
      g_host_err = "enc: a receptor's bond link leaves its range";
      return KMC_ERR_STATE;
    }
  acc->exp_reach += dt * acc->occ_reach;
  acc->exp_reactive += dt * acc->occ_reactive;
  acc->exp_free_receptor += dt * acc->occ_free_receptor;
  int64_t cnt[kmce::ENC_NCNT] = {0};
  for (int i = 0; i < h.na; ++i) {
    kmce::Slots r = enc_load(view, i);
    bool occ[ENC_SLOTS];
    for (int s = 0; s < ENC_SLOTS; ++s) {
      const int32_t k = r.key[s];
      const int q = (k >> 2) - 1;
      occ[s] = k != 0 && q >= 0 && q < h.nb && h.stb(q, 2 + (k & 3)) != 0;
    }
    kmce::Events ev;
    int32_t m[kmce::ENC_NCNT] = {0};
    kmce::transition(t, h.na, cur[(size_t)i], occ, r, ev, m);
    for (int k = 0; k < ev.n; ++k) {
      hist10[(size_t)ev.row[k] * ENC_BINS + kmck::bin(ev.val[k])] += 1;
      hist10[(size_t)(ENC_ROWS_UPD + ev.rrow[k]) * ENC_BINS + kmck::bin(ev.rval[k])] += 1;
    }
    enc_store(view, i, r);
    for (int k = 0; k < kmce::ENC_NCNT; ++k) cnt[k] += m[k];
  }
  acc->on_from_encounter += cnt[kmce::C_FROM_ENCOUNTER];
  acc->on_direct += cnt[kmce::C_DIRECT];
  acc->n_opened += cnt[kmce::C_OPENED];
  acc->n_ended += cnt[kmce::C_ENDED];
  acc->n_overflow += cnt[kmce::C_OVERFLOW];
  enc_set_occ(acc, cnt);
  acc->last_step = t;
  acc->n_updates += 1;
  return KMC_OK;
}

int kmc_host_enc_sample(const kmc_params* p, const kmc_enc_view* view, const kmc_enc_out* acc, const int64_t* hist10,
                        kmc_enc_out* out, int64_t* hist, int64_t* react_hist) {
  if (!p || !enc_view_ok(view) || !acc || !hist10 || !out) {
    g_host_err = "enc sample: params, the view's six arrays, acc, hist10 and out are needed";
    return KMC_ERR_ARG;
  }
  const kmc_enc_out a = *acc;  // (out may be acc itself)
  *out = a;
  out->n_censored_alive = 0;
  if (hist) {
    std::copy(hist10, hist10 + (size_t)ENC_ROWS_UPD * ENC_BINS, hist);
    std::fill(hist + (size_t)ENC_ROWS_UPD * ENC_BINS, hist + (size_t)ENC_HISTS * ENC_BINS, (int64_t)0);
  }
  if (react_hist)
    std::copy(hist10 + (size_t)ENC_ROWS_UPD * ENC_BINS, hist10 + (size_t)ENC_ACC_ROWS * ENC_BINS, react_hist);
  for (int i = 0; i < p->n_a; ++i) {
    const kmce::Slots r = enc_load(view, i);
    for (int s = 0; s < ENC_SLOTS; ++s) {
      if (r.key[s] == 0) continue;
      if (r.flags[s] & kmce::F_CENSORED) out->n_censored_alive += 1;
      else if (hist) hist[(size_t)kmce::ROW_ALIVE * ENC_BINS + kmck::bin(a.last_step - r.since[s])] += 1;
    }
  }
  return KMC_OK;
}

int kmc_host_math(int op, const double* x, const double* y, double* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    double a = x[i], b = y[i], r = 0;
    switch (op) {
      case 0: r = kmcm::sin(a); break;
      case 1: r = kmcm::cos(a); break;
      case 2: r = kmcm::atan2(a, b); break;
      case 3: r = kmcm::acos(a); break;
      case 4: r = kmcm::sqrt_(a); break;
      case 5: r = a / b; break;
      default: r = kmcm::round_(a); break;
    }
    out[i] = r;
  }
  return KMC_OK;
}

}  // extern "C"
