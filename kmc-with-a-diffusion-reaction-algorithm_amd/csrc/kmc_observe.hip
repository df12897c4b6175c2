// kmc_observe.hip — the host side of the read-only layers over the committed
// state: their C-ABI calls, one section a layer, over the
// kernels and the state structs of kmc_analysis.hip ... kmc_proximity.hip.  Nothing
// here writes a buffer a step reads, so the trajectory, the step counter and
// clusters_valid stay as they are.
//
// Included by kmc_engine.hip after its helpers (fail, HIPCHK, dalloc, dfree):
// one translation unit, the library's flags.  What the layers share comes
// first; the engine uses the knob helpers and bins_scan too.

namespace {

// ---------------------------------------------------------------- environment knobs
// the three idioms: on by '1'; on unless '0'; an integer clamped into [lo, hi]
// (dflt when unset or empty).  The knob's literal name comes first:
// tests/test_knob_docs.py finds the knobs by it.
bool flag_getenv(const char* name) {
  const char* v = getenv(name);
  return v && *v == '1';
}
bool unless_getenv(const char* name) {
  const char* v = getenv(name);
  return !(v && *v == '0');
}
int64_t int_getenv(const char* name, int64_t dflt, int64_t lo, int64_t hi) {
  const char* v = getenv(name);
  return v && *v ? std::max(lo, std::min(hi, (int64_t)atoll(v))) : dflt;
}

void observe_knobs(kmc_sim* s) {
  // debug: kmc_pair_counts stages fewer points at a time
  s->an.chunk = (int)int_getenv("KMC_DEBUG_PAIR_CHUNK", AN_CHUNK, 1, AN_CHUNK);
  // debug: kmc_bond_order_corr stages fewer points at a time
  s->bo.chunk = (int)int_getenv("KMC_DEBUG_BO_CHUNK", BO_CHUNK, 1, BO_CHUNK);
}

// ---------------------------------------------------------------- cell binning
// Exclusive scan of n counts (in may be out) on the handle's stream: tile sums
// into part, their scan, the tiles.
void bins_scan(kmc_sim* s, const int32_t* in, int32_t* out, int n, int32_t* part) {
  const int nb = (n + SCAN_TILE - 1) / SCAN_TILE;
  k_scan_part<<<nb, 256, 0, s->stream>>>(in, n, part);
  k_scan_top<<<1, 256, 0, s->stream>>>(part, nb);
  k_scan_down<<<nb, 256, 0, s->stream>>>(in, out, n, part);
}

// room for ncnt counts (the cells and the scan's last entry); `what` names the layer in the failure
int bins_reserve(kmc_sim* s, CellBins& b, size_t ncnt, const char* what) {
  if (ncnt <= b.cap) return KMC_OK;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  dfree(s, b.ccnt);
  dfree(s, b.cstart);
  dfree(s, b.part);
  b.cap = 0;
  int rc = KMC_OK;
  rc |= dalloc(s, &b.ccnt, ncnt);
  rc |= dalloc(s, &b.cstart, ncnt);
  rc |= dalloc(s, &b.part, (ncnt + SCAN_TILE - 1) / SCAN_TILE);
  if (rc != KMC_OK) return fail(s, KMC_ERR_HIP, std::string(what) + ": scratch allocation failed");
  b.cap = ncnt;
  return KMC_OK;
}

// squared bin edges: bin k holds e[k] <= d2 < e[k + 1], e[m] the product (m dr)(m dr) in double
std::vector<double> sq_edges(double r_max, int nbins) {
  const double dr = r_max / nbins;
  std::vector<double> edges2((size_t)nbins + 1);
  for (int m = 0; m <= nbins; ++m) edges2[m] = (m * dr) * (m * dr);
  return edges2;
}

// ---------------------------------------------------------------- scratch groups
// dalloc, recorded in the layer's group
template <typename T>
int salloc(kmc_sim* s, Scratch& g, T** p, size_t n) {
  const int rc = dalloc(s, p, n);
  if (rc == KMC_OK) g.ptrs.push_back(*p);
  return rc;
}

// frees what the group holds (dfree: the handle's list forgets the buffers too)
void scratch_free(kmc_sim* s, Scratch& g) {
  for (void*& v : g.ptrs) dfree(s, v);
  g.ptrs.clear();
}

// ---------------------------------------------------------------- calls and recorders
int an_check(kmc_sim* s) {
  if (!s->have_state) return fail(s, KMC_ERR_ARG, "analysis: no state");
  if (s->K.dd) return fail(s, KMC_ERR_ARG, "analysis: a decomposed window is not analysed");
  return KMC_OK;
}

// HIP events around one call's device work on the handle's stream
int an_begin(kmc_sim* s) {
  for (auto& e : s->an_ev)
    if (!e) HIPCHK(s, hipEventCreate(&e));
  HIPCHK(s, hipEventRecord(s->an_ev[0], s->stream));
  return KMC_OK;
}
int an_end(kmc_sim* s) {
  HIPCHK(s, hipEventRecord(s->an_ev[1], s->stream));
  HIPCHK(s, hipStreamSynchronize(s->stream));
  float ms = 0;
  HIPCHK(s, hipEventElapsedTime(&ms, s->an_ev[0], s->an_ev[1]));
  s->an_ms = ms;
  return KMC_OK;
}

// a recorder's call other than its begin: `off` is the layer's "not begun" message
int rec_check(kmc_sim* s, const Recorder& r, const char* off) {
  const int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  if (!r.on) return fail(s, KMC_ERR_ARG, off);
  return KMC_OK;
}

// the layer's scratch is freed and its state starts over: a begin's way out
// when an allocation failed, and, after the stream's work, a recorder's end
template <typename State>
void scratch_drop(kmc_sim* s, State& st) {
  scratch_free(s, st.scratch);
  st = State{};
}
template <typename State>
int rec_end(kmc_sim* s, State& st) {
  if (s->stream) HIPCHK(s, hipStreamSynchronize(s->stream));
  scratch_drop(s, st);
  return KMC_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- analysis
// kmc_analysis.hip: components with the census, pair counts.

// labels (0-based roots, reference order) and the roots' member counts, left
// on the device; the stream is not waited for
static int an_components(kmc_sim* s) {
  const int N = s->K.N, NA = s->K.NA;
  if (!s->an.out) {
    int rc = KMC_OK;
    rc |= dalloc(s, &s->an.parent, (size_t)N);
    rc |= dalloc(s, &s->an.label, (size_t)N);
    rc |= dalloc(s, &s->an.cnt, (size_t)N);
    if (!s->an.hist) rc |= dalloc(s, &s->an.hist, (size_t)AN_HIST_MAX);
    rc |= dalloc(s, &s->an.out, 1);
    if (rc != KMC_OK) return fail(s, KMC_ERR_HIP, "analysis: scratch allocation failed");
  }
  hipStream_t st = s->stream;
  const unsigned g = (unsigned)((N + AN_T - 1) / AN_T);
  HIPCHK(s, hipMemsetAsync(s->an.out, 0, sizeof(AnOut), st));
  if (g) {
    k_an_init<<<g, AN_T, 0, st>>>(s->an.parent, s->an.cnt, N);
    k_an_hook<<<g, AN_T, 0, st>>>(s->K, s->d, s->an.parent, s->an.out);
    k_an_flatten<<<g, AN_T, 0, st>>>(s->an.parent, s->an.label, N, s->an.out);
    k_an_count<<<g, AN_T, 0, st>>>(s->an.label, s->an.cnt, NA, N);
  }
  HIPCHK(s, hipGetLastError());
  return KMC_OK;
}

int kmc_components(kmc_sim* s, int32_t* label) {
  if (!s) return KMC_ERR_ARG;
  int rc = an_check(s);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = an_components(s);
  if (rc == KMC_OK) rc = an_end(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N;
  AnOut o;
  HIPCHK(s, hipMemcpy(&o, s->an.out, sizeof o, hipMemcpyDeviceToHost));
  if (o.err) return fail(s, KMC_ERR_STATE, "analysis: a bond link leaves the state or the link chains do not end");
  if (label) {
    HIPCHK(s, hipMemcpy(label, s->an.label, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i) label[i] += 1;
  }
  return KMC_OK;
}

int kmc_oligomer_census(kmc_sim* s, int32_t max_r, int32_t max_l, int64_t* hist, kmc_census* out) {
  if (!s) return KMC_ERR_ARG;
  if (!out || max_r < 0 || max_l < 0) return fail(s, KMC_ERR_ARG, "census: out is needed, max_r and max_l >= 0");
  const int64_t nbin = hist ? ((int64_t)max_r + 1) * ((int64_t)max_l + 1) : 0;
  if (nbin > AN_HIST_MAX)
    return fail(s, KMC_ERR_ARG, "census: more than " + std::to_string(AN_HIST_MAX) + " bins (larger counts clamp into the last row / column)");
  int rc = an_check(s);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = an_components(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N;
  hipStream_t st = s->stream;
  if (nbin) HIPCHK(s, hipMemsetAsync(s->an.hist, 0, sizeof(unsigned long long) * (size_t)nbin, st));
  const unsigned g = (unsigned)std::min<int64_t>(AN_WG_MAX, ((int64_t)N + AN_T - 1) / AN_T);
  if (g)
    k_an_census<<<g, AN_T, sizeof(unsigned long long) * (size_t)(nbin + 5), st>>>(
        s->an.label, s->an.cnt, N, max_r, max_l, nbin ? s->an.hist : nullptr, s->an.out);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  AnOut o;
  HIPCHK(s, hipMemcpy(&o, s->an.out, sizeof o, hipMemcpyDeviceToHost));
  if (o.err) return fail(s, KMC_ERR_STATE, "analysis: a bond link leaves the state or the link chains do not end");
  std::memset(out, 0, sizeof *out);
  out->n_components = (int64_t)o.n_components;
  out->n_complexes = (int64_t)o.n_complexes;
  out->proteins_in_complexes = (int64_t)o.proteins_in_complexes;
  out->n_cis_dimers = (int64_t)o.n_cis_dimers;
  if (o.n_components) {
    const uint32_t root = 0xffffffffu - (uint32_t)o.best;
    unsigned long long c = 0;
    HIPCHK(s, hipMemcpy(&c, s->an.cnt + root, sizeof c, hipMemcpyDeviceToHost));
    out->max_size = (int32_t)(o.best >> 32);
    out->max_receptors = (int32_t)(uint32_t)c;
    out->max_ligands = (int32_t)(c >> 32);
    out->max_label = (int32_t)root + 1;
  }
  if (nbin) HIPCHK(s, hipMemcpy(hist, s->an.hist, sizeof(int64_t) * (size_t)nbin, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_pair_counts(kmc_sim* s, int32_t which, double r_max, int32_t nbins, int64_t* counts) {
  if (!s) return KMC_ERR_ARG;
  if (!counts || which < KMC_PAIR_AA || which > KMC_PAIR_BB || !(r_max > 0.0) || !std::isfinite(r_max) || nbins < 1 ||
      nbins > AN_HIST_MAX)
    return fail(s, KMC_ERR_ARG, "pair counts: which 0..2, r_max > 0, 1 <= nbins <= " + std::to_string(AN_HIST_MAX));
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  const KParams& K = s->K;
  const double fx = std::floor(K.box_x / r_max), fy = std::floor(K.box_y / r_max);
  if (!(fx >= 3.0) || !(fy >= 3.0))
    return fail(s, KMC_ERR_ARG, "pair counts: r_max above a third of the box (fewer than 3 cells along an axis)");
  AnGrid G;
  G.ncx = (int)std::min<double>(fx, AN_NC_MAX);
  G.ncy = (int)std::min<double>(fy, AN_NC_MAX);
  G.box_x = K.box_x;
  G.box_y = K.box_y;
  G.nsets = which == KMC_PAIR_AB ? 2 : 1;
  G.lo[0] = which == KMC_PAIR_BB ? K.NA : 0;
  G.hi[0] = which == KMC_PAIR_BB ? K.N : K.NA;
  G.lo[1] = K.NA;
  G.hi[1] = K.N;
  const int N = K.N, ncell = G.ncx * G.ncy, npts = (G.hi[0] - G.lo[0]) + (G.nsets > 1 ? G.hi[1] - G.lo[1] : 0);
  const size_t ncnt = (size_t)G.nsets * ncell + 1;  // the scan's last entry is the number of points
  if (!s->an.pts) {
    rc = KMC_OK;
    rc |= dalloc(s, &s->an.cell, (size_t)N);
    rc |= dalloc(s, &s->an.rank, (size_t)N);
    rc |= dalloc(s, &s->an.pts, (size_t)N);
    rc |= dalloc(s, &s->an.edges, (size_t)AN_HIST_MAX + 1);
    if (!s->an.hist) rc |= dalloc(s, &s->an.hist, (size_t)AN_HIST_MAX);
    if (rc != KMC_OK) return fail(s, KMC_ERR_HIP, "analysis: scratch allocation failed");
  }
  rc = bins_reserve(s, s->an.bins, ncnt, "analysis");
  if (rc != KMC_OK) return rc;
  const double dr = r_max / nbins;
  const std::vector<double> edges2 = sq_edges(r_max, nbins);
  hipStream_t st = s->stream;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpyAsync(s->an.edges, edges2.data(), sizeof(double) * edges2.size(), hipMemcpyHostToDevice, st));
  HIPCHK(s, hipMemsetAsync(s->an.hist, 0, sizeof(unsigned long long) * (size_t)nbins, st));
  HIPCHK(s, hipMemsetAsync(s->an.bins.ccnt, 0, sizeof(int32_t) * ncnt, st));
  if (npts > 0) {
    const unsigned g = (unsigned)((npts + AN_T - 1) / AN_T);
    k_an_cell_count<<<g, AN_T, 0, st>>>(s->K, s->d, G, s->an.bins.ccnt, s->an.cell, s->an.rank);
    bins_scan(s, s->an.bins.ccnt, s->an.bins.cstart, (int)ncnt, s->an.bins.part);
    k_an_cell_scatter<<<g, AN_T, 0, st>>>(s->K, s->d, G, s->an.bins.cstart, s->an.cell, s->an.rank, s->an.pts);
    const size_t lds = sizeof(unsigned long long) * (size_t)nbins + 2 * sizeof(double2) * (size_t)s->an.chunk;
    k_an_pairs<<<(unsigned)std::min(ncell, AN_WG_MAX), AN_T, lds, st>>>(
        G, s->an.bins.cstart, s->an.pts, s->an.edges, nbins, (float)(1.0 / dr), s->an.chunk, s->an.hist);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);  // (waits: edges2 is read by the copy until here)
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpy(counts, s->an.hist, sizeof(int64_t) * (size_t)nbins, hipMemcpyDeviceToHost));
  return KMC_OK;
}

double kmc_analysis_ms(const kmc_sim* s) { return s ? s->an_ms : 0.0; }

// ---------------------------------------------------------------- cluster geometry
// kmc_geometry.hip: read-only like the analysis above, on scratch of its own.

static_assert(sizeof(kmc_geom_bin) == sizeof(unsigned long long) * GEO_BIN, "a table bin is GEO_BIN words");
static_assert(sizeof(kmc_cluster) == 80, "kmc_cluster layout");
static_assert(KMC_GEOM_MAX_SIZE == GEO_MAX_SIZE, "kmc.h and kmc_geometry.hip agree on the table limit");

// labels, image shifts, spanning bits, member counts and moments by root, left
// on the device (five launches); the stream is not waited for
static int geo_run(kmc_sim* s) {
  const int N = s->K.N, NA = s->K.NA;
  if (!s->geo.out) {
    int rc = KMC_OK;
    rc |= dalloc(s, &s->geo.word, (size_t)N);
    rc |= dalloc(s, &s->geo.cnt, (size_t)N);
    rc |= dalloc(s, &s->geo.acc, (size_t)N * GEO_ACC);
    rc |= dalloc(s, &s->geo.table, (size_t)(GEO_MAX_SIZE + 1) * GEO_BIN);
    rc |= dalloc(s, &s->geo.X, (size_t)N);
    rc |= dalloc(s, &s->geo.label, (size_t)N);
    rc |= dalloc(s, &s->geo.off, (size_t)N);
    rc |= dalloc(s, &s->geo.span, (size_t)N);
    rc |= dalloc(s, &s->geo.out, 1);
    if (rc != KMC_OK) return fail(s, KMC_ERR_HIP, "geometry: scratch allocation failed");
  }
  hipStream_t st = s->stream;
  const unsigned g = (unsigned)((N + AN_T - 1) / AN_T);
  const long long BX = (long long)kmcm::round_(s->K.box_x * 1024.0), BY = (long long)kmcm::round_(s->K.box_y * 1024.0);
  HIPCHK(s, hipMemsetAsync(s->geo.out, 0, sizeof(GeoOut), st));
  if (g) {
    k_geo_init<<<g, AN_T, 0, st>>>(s->K, s->d, s->geo.word, s->geo.X, s->geo.cnt, s->geo.span, s->geo.acc);
    k_geo_hook<<<g, AN_T, 0, st>>>(s->K, s->d, s->geo.word, s->geo.out);
    k_geo_flatten<<<g, AN_T, 0, st>>>(s->geo.word, s->geo.label, s->geo.off, s->geo.cnt, NA, N, s->geo.out);
    k_geo_check<<<g, AN_T, 0, st>>>(s->K, s->d, s->geo.label, s->geo.off, s->geo.span, s->geo.out);
    k_geo_moments<<<g, AN_T, 0, st>>>(s->geo.label, s->geo.off, s->geo.X, s->geo.span, BX, BY, N, s->geo.acc);
  }
  HIPCHK(s, hipGetLastError());
  return KMC_OK;
}

// the device's verdict of the last geometry call
static int geo_result(kmc_sim* s, GeoOut* o) {
  HIPCHK(s, hipMemcpy(o, s->geo.out, sizeof *o, hipMemcpyDeviceToHost));
  if (o->err & 1u)
    return fail(s, KMC_ERR_STATE, "geometry: a bond link leaves the state or the link chains do not end");
  if (o->err & 2u) return fail(s, KMC_ERR_CAPACITY, "geometry: an image shift leaves [-32767, 32767]");
  return KMC_OK;
}

int kmc_unwrap(kmc_sim* s, int32_t* label, int32_t* shift, uint8_t* span) {
  if (!s) return KMC_ERR_ARG;
  int rc = an_check(s);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = geo_run(s);
  if (rc == KMC_OK) rc = an_end(s);
  if (rc != KMC_OK) return rc;
  GeoOut o;
  rc = geo_result(s, &o);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N;
  std::vector<int32_t> lab(N);
  std::vector<uint32_t> sp(N);
  HIPCHK(s, hipMemcpy(lab.data(), s->geo.label, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(sp.data(), s->geo.span, sizeof(uint32_t) * N, hipMemcpyDeviceToHost));
  if (shift) {
    std::vector<int2> off(N);
    HIPCHK(s, hipMemcpy(off.data(), s->geo.off, sizeof(int2) * N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) {
      const bool wraps = sp[lab[i]] != 0;  // (its offsets depend on the tree: not reported)
      shift[i] = wraps ? 0 : off[i].x;
      shift[N + i] = wraps ? 0 : off[i].y;
    }
  }
  if (span)
    for (size_t i = 0; i < N; ++i) span[i] = (uint8_t)sp[lab[i]];
  if (label)
    for (size_t i = 0; i < N; ++i) label[i] = lab[i] + 1;
  return KMC_OK;
}

int kmc_cluster_geometry(kmc_sim* s, int32_t max_size, kmc_geom_bin* table, kmc_geom* out) {
  if (!s) return KMC_ERR_ARG;
  if (!out || max_size < 2 || max_size > GEO_MAX_SIZE)
    return fail(s, KMC_ERR_ARG, "cluster geometry: out is needed, 2 <= max_size <= " + std::to_string(GEO_MAX_SIZE) +
                                    " (larger clusters clamp into the last bin)");
  int rc = an_check(s);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = geo_run(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N;
  const size_t nbin = table ? (size_t)max_size + 1 : 0;
  hipStream_t st = s->stream;
  if (nbin) HIPCHK(s, hipMemsetAsync(s->geo.table, 0, sizeof(kmc_geom_bin) * nbin, st));
  const unsigned g = (unsigned)std::min<int64_t>(GEO_TABLE_WG, ((int64_t)N + AN_T - 1) / AN_T);
  if (g)
    k_geo_table<<<g, AN_T, sizeof(unsigned long long) * (nbin * GEO_BIN + 6), st>>>(
        s->geo.label, s->geo.cnt, s->geo.span, s->geo.acc, N, max_size, nbin ? s->geo.table : nullptr, s->geo.out);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  GeoOut o;
  rc = geo_result(s, &o);
  if (rc != KMC_OK) return rc;
  std::memset(out, 0, sizeof *out);
  out->n_measured = (int64_t)o.n_measured;
  out->n_spanning = (int64_t)o.n_spanning;
  out->n_span_x = (int64_t)o.n_span_x;
  out->n_span_y = (int64_t)o.n_span_y;
  out->proteins_in_spanning = (int64_t)o.proteins_in_spanning;
  if (o.best) {
    const uint32_t root = 0xffffffffu - (uint32_t)o.best;
    uint32_t sp = 0;
    HIPCHK(s, hipMemcpy(&sp, s->geo.span + root, sizeof sp, hipMemcpyDeviceToHost));
    out->largest_label = (int32_t)root + 1;
    out->largest_size = (int32_t)(o.best >> 32);
    out->largest_span = (int32_t)sp;
  }
  if (nbin) HIPCHK(s, hipMemcpy(table, s->geo.table, sizeof(kmc_geom_bin) * nbin, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_cluster_list(kmc_sim* s, int32_t min_size, int64_t cap, kmc_cluster* rows, int64_t* n) {
  if (!s) return KMC_ERR_ARG;
  if (!n || min_size < 2 || cap < 0 || (cap > 0 && !rows))
    return fail(s, KMC_ERR_ARG, "cluster list: n is needed, min_size >= 2, cap >= 0, rows for cap > 0");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N;
  // no more than N / min_size roots can qualify: a larger cap needs no larger buffer
  const size_t dcap = (size_t)std::min<int64_t>(cap, N / min_size);
  if (dcap > s->geo.rows_cap) {
    HIPCHK(s, hipStreamSynchronize(s->stream));
    dfree(s, s->geo.rows);
    s->geo.rows_cap = 0;
    if (dalloc(s, &s->geo.rows, dcap) != KMC_OK) return fail(s, KMC_ERR_HIP, "geometry: scratch allocation failed");
    s->geo.rows_cap = dcap;
  }
  rc = an_begin(s);
  if (rc == KMC_OK) rc = geo_run(s);
  if (rc != KMC_OK) return rc;
  const unsigned g = (unsigned)((N + AN_T - 1) / AN_T);
  if (g)
    k_geo_list<<<g, AN_T, 0, s->stream>>>(s->geo.label, s->geo.cnt, s->geo.span, s->geo.acc, N, min_size,
                                          (long long)dcap, s->geo.rows, s->geo.out);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  GeoOut o;
  rc = geo_result(s, &o);
  if (rc != KMC_OK) return rc;
  *n = (int64_t)o.n_rows;
  if (*n > cap)
    return fail(s, KMC_ERR_CAPACITY, "cluster list: " + std::to_string(*n) + " components qualify, cap is " +
                                         std::to_string(cap));
  if (*n) {
    HIPCHK(s, hipMemcpy(rows, s->geo.rows, sizeof(kmc_cluster) * (size_t)*n, hipMemcpyDeviceToHost));
    std::sort(rows, rows + *n, [](const kmc_cluster& a, const kmc_cluster& b) { return a.label < b.label; });
  }
  return KMC_OK;
}

// ---------------------------------------------------------------- structure factor
// kmc_structure.hip: read-only like the analysis above, one launch on scratch of its own.

static_assert(KMC_SK_MAX == SK_MAX, "kmc.h and kmc_structure.h agree on the grid limit");
#define SK_NQ_MAX ((SK_MAX + 1) * (2 * SK_MAX + 1))

int kmc_structure_factor(kmc_sim* s, int32_t hmax, int32_t kmax, int32_t select, int64_t* sums, int64_t n_sel[2]) {
  if (!s) return KMC_ERR_ARG;
  if (!sums || !n_sel || hmax < 0 || hmax > SK_MAX || kmax < 0 || kmax > SK_MAX ||
      (select != KMC_SK_ALL && select != KMC_SK_BOUND))
    return fail(s, KMC_ERR_ARG, "structure factor: sums and n_sel are needed, 0 <= hmax, kmax <= " +
                                    std::to_string(SK_MAX) + ", select is KMC_SK_ALL or KMC_SK_BOUND");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  SkArgs a;
  a.hmax = hmax;
  a.kmax = kmax;
  a.select = select;
  a.W = 2 * kmax + 1;
  a.nq = (hmax + 1) * a.W;
  const int nqb = (a.nq + SK_QB - 1) / SK_QB;
  a.qb = (a.nq + nqb - 1) / nqb;
  a.nh_max = std::min(hmax + 1, (a.qb - 1) / a.W + 2);
  a.E = a.nh_max + kmax + 1;
  a.BX = (long long)kmcm::round_(s->K.box_x * 1024.0);
  a.BY = (long long)kmcm::round_(s->K.box_y * 1024.0);
  if (a.BX < 1 || a.BY < 1) return fail(s, KMC_ERR_ARG, "structure factor: the box is below 2^-10 A");
  if (a.E > SK_E_MAX) return fail(s, KMC_ERR_CAPACITY, "structure factor: axis tables beyond SK_E_MAX");
  if (!s->sk.sums && dalloc(s, &s->sk.sums, (size_t)4 * SK_NQ_MAX + 2) != KMC_OK)
    return fail(s, KMC_ERR_HIP, "structure factor: scratch allocation failed");
  const size_t nw = (size_t)4 * a.nq;
  unsigned long long* d_nsel = s->sk.sums + (size_t)4 * SK_NQ_MAX;
  const int ntile = (std::max(s->K.NA, s->K.NB) + SK_TILE - 1) / SK_TILE;
  const dim3 grid((unsigned)std::max(1, std::min(ntile, SK_WG / nqb)), (unsigned)nqb);
  const size_t lds = (sizeof(double2) * (size_t)SK_TILE * a.E + sizeof(longlong2) * SK_TILE + sizeof(int) * (SK_TILE + 1) + 15) / 16 * 16;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  hipStream_t st = s->stream;
  HIPCHK(s, hipMemsetAsync(s->sk.sums, 0, sizeof(unsigned long long) * nw, st));
  HIPCHK(s, hipMemsetAsync(d_nsel, 0, sizeof(unsigned long long) * 2, st));
  k_sk_sums<<<grid, SK_T, lds, st>>>(s->K, s->d, a, s->sk.sums, d_nsel);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpy(sums, s->sk.sums, sizeof(int64_t) * nw, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(n_sel, d_nsel, sizeof(int64_t) * 2, hipMemcpyDeviceToHost));
  return KMC_OK;
}

// ---------------------------------------------------------------- bond-orientational order
// kmc_bondorder.hip: read-only like the analysis above, on scratch of its own.

static_assert(KMC_BO_MAX_FOLD == BO_MAX_FOLD && KMC_BO_NN_ROWS == BO_NN_ROWS, "kmc.h and kmc_bondorder.h agree");
static_assert(sizeof(kmc_bond_order_out) == 6 * sizeof(unsigned long long), "kmc_bond_order_out is BoOut's six sums");

// a workgroup's dynamic LDS beyond the 64 KiB every launch may ask for (the CU has 160 KiB)
static void bo_lds_limit(const void* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    (void)hipGetLastError();  // the launch itself reports what it cannot have
}

// the arguments both calls share, checked and turned into the kernels'; the scratch of the first call
static int bo_setup(kmc_sim* s, int32_t which, int32_t mode, int32_t fold, double r_cut, int32_t select, BoArgs* a) {
  if ((which != KMC_BO_A && which != KMC_BO_B) || (mode != KMC_BO_WITHIN && mode != KMC_BO_LINKED) || fold < 1 ||
      fold > BO_MAX_FOLD || (select != KMC_BO_ALL && select != KMC_BO_BOUND) ||
      (mode == KMC_BO_LINKED && which != KMC_BO_B))
    return fail(s, KMC_ERR_ARG, "bond order: which 0 or 1, mode 0 or 1 (linked: ligands only), 1 <= fold <= " +
                                    std::to_string(BO_MAX_FOLD) + ", select 0 or 1");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  const KParams& K = s->K;
  const double bx = kmcm::round_(K.box_x * 1024.0), by = kmcm::round_(K.box_y * 1024.0);
  if (!(bx >= 1.0) || !(by >= 1.0) || !(bx < (double)BO_BOX_MAX) || !(by < (double)BO_BOX_MAX))
    return fail(s, KMC_ERR_ARG, "bond order: the box is below 2^-10 A or not below 2^21 A");
  a->which = which;
  a->mode = mode;
  a->fold = fold;
  a->select = select;
  a->base = which == KMC_BO_A ? 0 : K.NA;
  a->n = which == KMC_BO_A ? K.NA : K.NB;
  a->BX = (long long)bx;
  a->BY = (long long)by;
  a->RC2 = 0;
  a->ncx = a->ncy = 0;
  if (mode == KMC_BO_WITHIN) {
    const long long RC =
        r_cut > 0.0 && r_cut * 1024.0 < (double)BO_BOX_MAX ? (long long)kmcm::round_(r_cut * 1024.0) : 0;
    if (RC < 1 || a->BX / RC < 3 || a->BY / RC < 3)
      return fail(s, KMC_ERR_ARG, "bond order: r_cut must be positive and at most a third of the box (3 cells along an axis)");
    a->RC2 = RC * RC;
    a->ncx = (int)std::min<long long>(a->BX / RC, BO_NC_MAX);
    a->ncy = (int)std::min<long long>(a->BY / RC, BO_NC_MAX);
  }
  if (!s->bo.out) {
    const size_t n = (size_t)std::max(K.NA, K.NB);
    rc = KMC_OK;
    rc |= dalloc(s, &s->bo.cell, n);
    rc |= dalloc(s, &s->bo.rank, n);
    rc |= dalloc(s, &s->bo.ref, n);
    rc |= dalloc(s, &s->bo.nn, n);
    rc |= dalloc(s, &s->bo.pts, n);
    rc |= dalloc(s, &s->bo.pcs, n);
    rc |= dalloc(s, &s->bo.pcs_sorted, n);
    rc |= dalloc(s, &s->bo.C, n);
    rc |= dalloc(s, &s->bo.S, n);
    rc |= dalloc(s, &s->bo.hist, (size_t)BO_NN_ROWS * BO_HIST_BINS);
    rc |= dalloc(s, &s->bo.corr, (size_t)2 * BO_CORR_BINS);
    rc |= dalloc(s, &s->bo.E2, (size_t)BO_CORR_BINS + 1);
    rc |= dalloc(s, &s->bo.out, 1);
    if (rc != KMC_OK) return fail(s, KMC_ERR_HIP, "bond order: scratch allocation failed");
  }
  return KMC_OK;
}

// the set binned on the grid a->ncx x a->ncy (nn_filter: only the proteins with neighbours, with their (pc, ps))
static int bo_grid(kmc_sim* s, const BoArgs& a, bool corr_grid) {
  const size_t ncnt = (size_t)a.ncx * a.ncy + 1;  // the scan's last entry is the number of binned points
  const int rc = bins_reserve(s, s->bo.bins, ncnt, "bond order");
  if (rc != KMC_OK) return rc;
  hipStream_t st = s->stream;
  HIPCHK(s, hipMemsetAsync(s->bo.bins.ccnt, 0, sizeof(int32_t) * ncnt, st));
  const unsigned g = (unsigned)((a.n + BO_T - 1) / BO_T);
  if (g)
    k_bo_cell_count<<<g, BO_T, 0, st>>>(s->K, s->d, a, corr_grid ? s->bo.nn : nullptr, s->bo.bins.ccnt, s->bo.cell,
                                        s->bo.rank, s->bo.out);
  bins_scan(s, s->bo.bins.ccnt, s->bo.bins.cstart, (int)ncnt, s->bo.bins.part);
  if (g)
    k_bo_cell_scatter<<<g, BO_T, 0, st>>>(s->K, s->d, a, s->bo.bins.cstart, s->bo.cell, s->bo.rank, s->bo.pts,
                                          s->bo.ref, corr_grid ? s->bo.pcs : nullptr, s->bo.pcs_sorted);
  HIPCHK(s, hipGetLastError());
  return KMC_OK;
}

// the local pass and the reduce, left on the device: (C, S, N) and (pc, ps) by reference index, the six sums and,
// for nbins > 0, the histogram.  The stream is not waited for.
static int bo_local(kmc_sim* s, const BoArgs& a, int nbins) {
  hipStream_t st = s->stream;
  const size_t n = (size_t)a.n;
  HIPCHK(s, hipMemsetAsync(s->bo.out, 0, sizeof(BoOut), st));
  HIPCHK(s, hipMemsetAsync(s->bo.C, 0, sizeof(unsigned long long) * n, st));
  HIPCHK(s, hipMemsetAsync(s->bo.S, 0, sizeof(unsigned long long) * n, st));
  HIPCHK(s, hipMemsetAsync(s->bo.nn, 0xff, sizeof(int32_t) * n, st));  // -1: outside the set until a centre writes its count
  if (nbins) HIPCHK(s, hipMemsetAsync(s->bo.hist, 0, sizeof(unsigned long long) * (size_t)BO_NN_ROWS * nbins, st));
  if (a.n == 0) return KMC_OK;
  if (a.mode == KMC_BO_WITHIN) {
    const int rc = bo_grid(s, a, false);
    if (rc != KMC_OK) return rc;
    const unsigned g = (unsigned)std::min<int64_t>(4 * BO_WG_MAX, ((int64_t)a.n + BO_T - 1) / BO_T);
    k_bo_local_queue<<<g, BO_T, 0, st>>>(a, s->bo.bins.cstart, s->bo.pts, s->bo.ref, s->bo.C, s->bo.S, s->bo.nn);
  } else {
    k_bo_local_linked<<<(unsigned)((a.n + BO_T - 1) / BO_T), BO_T, 0, st>>>(s->K, s->d, a, s->bo.C, s->bo.S, s->bo.nn,
                                                                            s->bo.out);
  }
  const size_t lds = sizeof(unsigned long long) * (6 + (size_t)BO_NN_ROWS * nbins);
  bo_lds_limit((const void*)k_bo_reduce, lds);
  const unsigned g = (unsigned)std::min<int64_t>(nbins > 64 ? 256 : BO_WG_MAX, ((int64_t)a.n + BO_T - 1) / BO_T);
  k_bo_reduce<<<g, BO_T, lds, st>>>(a.n, nbins, s->bo.C, s->bo.S, s->bo.nn, s->bo.pcs, nbins ? s->bo.hist : nullptr,
                                    s->bo.out);
  HIPCHK(s, hipGetLastError());
  return KMC_OK;
}

static int bo_result(kmc_sim* s, BoOut* o) {
  HIPCHK(s, hipMemcpy(o, s->bo.out, sizeof *o, hipMemcpyDeviceToHost));
  if (o->err & 1u) return fail(s, KMC_ERR_STATE, "bond order: a bond link leaves the state");
  if (o->err & 2u) return fail(s, KMC_ERR_CAPACITY, "bond order: a protein with more than 65535 neighbours");
  return KMC_OK;
}

int kmc_bond_order(kmc_sim* s, int32_t which, int32_t mode, int32_t fold, double r_cut, int32_t select, int32_t nbins,
                   int64_t* hist, kmc_bond_order_out* out, int64_t* C, int64_t* S, int32_t* nn) {
  if (!s) return KMC_ERR_ARG;
  if (!out || nbins < 1 || nbins > BO_HIST_BINS)
    return fail(s, KMC_ERR_ARG, "bond order: out is needed, 1 <= nbins <= " + std::to_string(BO_HIST_BINS));
  BoArgs a;
  int rc = bo_setup(s, which, mode, fold, r_cut, select, &a);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = bo_local(s, a, hist ? nbins : 0);
  if (rc == KMC_OK) rc = an_end(s);
  if (rc != KMC_OK) return rc;
  BoOut o;
  rc = bo_result(s, &o);
  if (rc != KMC_OK) return rc;
  std::memcpy(out, o.sum, sizeof *out);
  const size_t n = (size_t)a.n;
  if (hist) HIPCHK(s, hipMemcpy(hist, s->bo.hist, sizeof(int64_t) * (size_t)BO_NN_ROWS * nbins, hipMemcpyDeviceToHost));
  if (C && n) HIPCHK(s, hipMemcpy(C, s->bo.C, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
  if (S && n) HIPCHK(s, hipMemcpy(S, s->bo.S, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
  if (nn && n) {
    HIPCHK(s, hipMemcpy(nn, s->bo.nn, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
      if (nn[i] < 0) nn[i] = 0;  // outside the set
  }
  return KMC_OK;
}

int kmc_bond_order_corr(kmc_sim* s, int32_t which, int32_t mode, int32_t fold, double r_cut, int32_t select,
                        double r_max, int32_t nbins, int64_t* corr) {
  if (!s) return KMC_ERR_ARG;
  if (!corr || nbins < 1 || nbins > BO_CORR_BINS || !(r_max > 0.0) || !std::isfinite(r_max))
    return fail(s, KMC_ERR_ARG, "bond order: corr is needed, r_max > 0, 1 <= nbins <= " + std::to_string(BO_CORR_BINS));
  BoArgs a;
  int rc = bo_setup(s, which, mode, fold, r_cut, select, &a);
  if (rc != KMC_OK) return rc;
  const double dr = r_max / nbins;
  const int64_t EN = r_max * 1024.0 < (double)BO_BOX_MAX ? kmcb::corr_edge(nbins, dr) : 0;
  if (EN < 1 || !(std::floor(s->K.box_x / r_max) >= 3.0) || !(std::floor(s->K.box_y / r_max) >= 3.0) ||
      a.BX / EN < 3 || a.BY / EN < 3)
    return fail(s, KMC_ERR_ARG, "bond order: r_max must be at least 2^-10 A and at most a third of the box (3 cells along an axis)");
  std::vector<int64_t> E2((size_t)nbins + 1);
  for (int m = 0; m <= nbins; ++m) {
    const int64_t e = kmcb::corr_edge(m, dr);
    E2[m] = e * e;
  }
  hipStream_t st = s->stream;
  rc = an_begin(s);
  if (rc == KMC_OK) rc = bo_local(s, a, 0);
  if (rc != KMC_OK) return rc;
  BoOut o;
  HIPCHK(s, hipStreamSynchronize(st));
  rc = bo_result(s, &o);  // a local pass that failed ends the call before the pair walk
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpyAsync(s->bo.E2, E2.data(), sizeof(int64_t) * E2.size(), hipMemcpyHostToDevice, st));
  HIPCHK(s, hipMemsetAsync(s->bo.corr, 0, sizeof(unsigned long long) * 2 * (size_t)nbins, st));
  if (a.n > 0) {
    BoArgs g = a;  // the second grid: cells no narrower than the last edge
    g.ncx = (int)std::min<int64_t>(a.BX / EN, BO_NC_MAX);
    g.ncy = (int)std::min<int64_t>(a.BY / EN, BO_NC_MAX);
    rc = bo_grid(s, g, true);
    if (rc != KMC_OK) return rc;
    const size_t lds = 48 * (size_t)s->bo.chunk + sizeof(unsigned long long) * 2 * (size_t)nbins;
    bo_lds_limit((const void*)k_bo_corr, lds);
    k_bo_corr<<<(unsigned)std::min(g.ncx * g.ncy, BO_WG_MAX), BO_T, lds, st>>>(
        g, s->bo.bins.cstart, s->bo.pts, s->bo.pcs_sorted, s->bo.E2, nbins, (float)(1.0 / (dr * 1024.0)), s->bo.chunk,
        s->bo.corr);
    HIPCHK(s, hipGetLastError());
  }
  rc = an_end(s);  // (waits: E2 is read by the copy until here)
  if (rc == KMC_OK) rc = bo_result(s, &o);  // the second grid's index check
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpy(corr, s->bo.corr, sizeof(int64_t) * 2 * (size_t)nbins, hipMemcpyDeviceToHost));
  return KMC_OK;
}

// ---------------------------------------------------------------- displacement tracking
// kmc_dynamics.hip: the tracker is a layer of its own over the committed
// state; its calls write only TrkState's buffers.

static const char* const TRK_OFF = "track: no origin (kmc_track_begin; a new state drops the tracker)";

int kmc_track_begin(kmc_sim* s, double max_jump) {
  if (!s) return KMC_ERR_ARG;
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  const double half = 0.5 * std::min(s->K.box_x, s->K.box_y);
  if (!(max_jump <= 0.0) && !(max_jump <= half))  // (a NaN fails both)
    return fail(s, KMC_ERR_ARG, "track: max_jump above half the box (or not a number)");
  const int N = s->K.N;
  if (!s->trk.acc) {
    const size_t nblk = ((size_t)N + TRK_T - 1) / TRK_T;
    Scratch& g = s->trk.scratch;
    rc = KMC_OK;
    rc |= salloc(s, g, &s->trk.dev.prev, (size_t)N);
    rc |= salloc(s, g, &s->trk.dev.u, (size_t)N);
    rc |= salloc(s, g, &s->trk.dev.flags, (size_t)N);
    rc |= salloc(s, g, &s->trk.dev.cls, (size_t)N);
    rc |= salloc(s, g, &s->trk.dev.link0, 3 * (size_t)N);
    rc |= salloc(s, g, &s->trk.out, 1);
    rc |= salloc(s, g, &s->trk.part[0], TRK_NSUM * nblk);
    rc |= salloc(s, g, &s->trk.part[1], TRK_NSUM * ((nblk + TRK_T - 1) / TRK_T));
    rc |= salloc(s, g, &s->trk.edges, (size_t)TRK_BINS_MAX + 1);
    rc |= salloc(s, g, &s->trk.vh, (size_t)TRK_CLASSES * TRK_BINS_MAX);
    rc |= salloc(s, g, &s->trk.acc, 1);
    if (rc != KMC_OK) {
      scratch_drop(s, s->trk);
      return fail(s, KMC_ERR_HIP, "track: scratch allocation failed");
    }
  }
  s->trk.rec.on = false;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemsetAsync(s->trk.acc, 0, sizeof(TrkAcc), s->stream));
  if (N > 0) k_trk_begin<<<(unsigned)((N + TRK_T - 1) / TRK_T), TRK_T, 0, s->stream>>>(s->K, s->d, s->trk.dev);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  s->trk.max_jump = max_jump <= 0.0 ? 0.5 * half : max_jump;
  s->trk.rec = Recorder{true, s->step_done, s->step_done, 0};
  return KMC_OK;
}

int kmc_track_update(kmc_sim* s, kmc_track_info* info) {
  if (!s) return KMC_ERR_ARG;
  int rc = rec_check(s, s->trk.rec, TRK_OFF);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N;
  // the maxima persist since begin; the flag counts are of this update
  HIPCHK(s, hipMemsetAsync(&s->trk.acc->n_jumped, 0, 2 * sizeof(unsigned long long), s->stream));
  if (N > 0)
    k_trk_update<<<(unsigned)((N + TRK_T - 1) / TRK_T), TRK_T, 0, s->stream>>>(s->K, s->d, s->trk.dev, s->trk.max_jump,
                                                                             s->trk.acc);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  s->trk.rec.last = s->step_done;
  s->trk.rec.updates += 1;
  if (info) {
    TrkAcc a;
    HIPCHK(s, hipMemcpy(&a, s->trk.acc, sizeof a, hipMemcpyDeviceToHost));
    info->origin_step = s->trk.rec.origin;
    info->last_step = s->trk.rec.last;
    info->n_updates = s->trk.rec.updates;
    std::memcpy(&info->max_dx, &a.max_dx, sizeof(double));
    std::memcpy(&info->max_dy, &a.max_dy, sizeof(double));
    info->n_jumped = (int64_t)a.n_jumped;
    info->n_changed = (int64_t)a.n_changed;
  }
  return KMC_OK;
}

int kmc_track_sample(kmc_sim* s, double r_max, int32_t nbins, kmc_track_sample_t* out, int64_t* vanhove) {
  if (!s) return KMC_ERR_ARG;
  if (!out || !(r_max > 0.0) || !std::isfinite(r_max) || nbins < 1 || nbins > TRK_BINS_MAX)
    return fail(s, KMC_ERR_ARG, "track sample: out is needed, r_max > 0, 1 <= nbins <= " + std::to_string(TRK_BINS_MAX));
  int rc = rec_check(s, s->trk.rec, TRK_OFF);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N;
  const double dr = r_max / nbins;
  const std::vector<double> edges2 = sq_edges(r_max, nbins);
  hipStream_t st = s->stream;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpyAsync(s->trk.edges, edges2.data(), sizeof(double) * edges2.size(), hipMemcpyHostToDevice, st));
  HIPCHK(s, hipMemsetAsync(s->trk.out, 0, sizeof(TrkOut), st));
  if (vanhove) HIPCHK(s, hipMemsetAsync(s->trk.vh, 0, sizeof(unsigned long long) * TRK_CLASSES * (size_t)nbins, st));
  // level 1: blocks of 256 proteins -> part[0][s][nblk]; then the tree's next levels until one value per sum
  int n = (N + TRK_T - 1) / TRK_T, cur = 0;
  if (n > 0) {
    const size_t lds = sizeof(unsigned long long) * (size_t)(TRK_NSUM * TRK_T + TRK_NCNT + (vanhove ? TRK_CLASSES * nbins : 0));
    k_trk_sample<<<(unsigned)std::min(n, AN_WG_MAX), TRK_T, lds, st>>>(s->K, s->d, s->trk.dev, s->trk.edges, nbins,
                                                                      (float)(1.0 / dr), vanhove ? s->trk.vh : nullptr, n,
                                                                      s->trk.part[0], s->trk.out);
    while (n > 1) {
      const int nout = (n + TRK_T - 1) / TRK_T;
      k_trk_tree<<<dim3((unsigned)nout, TRK_NSUM), TRK_T, 0, st>>>(s->trk.part[cur], n, s->trk.part[cur ^ 1], nout);
      n = nout;
      cur ^= 1;
    }
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);  // (waits: edges2 is read by the copy until here)
  if (rc != KMC_OK) return rc;
  TrkOut o;
  double sums[TRK_NSUM] = {0};
  HIPCHK(s, hipMemcpy(&o, s->trk.out, sizeof o, hipMemcpyDeviceToHost));
  if (n == 1) HIPCHK(s, hipMemcpy(sums, s->trk.part[cur], sizeof sums, hipMemcpyDeviceToHost));
  std::memset(out, 0, sizeof *out);
  out->origin_step = s->trk.rec.origin;
  out->last_step = s->trk.rec.last;
  for (int c = 0; c < TRK_CLASSES; ++c) {
    out->n[c] = (int64_t)o.cnt[c];
    out->n_clean[c] = (int64_t)o.cnt[TRK_CLASSES + c];
    out->sum_u2[c] = sums[c];
    out->sum_u2_clean[c] = sums[TRK_CLASSES + c];
  }
  out->rl0 = (int64_t)o.cnt[10];
  out->rl_now = (int64_t)o.cnt[11];
  out->rl_kept = (int64_t)o.cnt[12];
  out->cis0 = (int64_t)o.cnt[13];
  out->cis_now = (int64_t)o.cnt[14];
  out->cis_kept = (int64_t)o.cnt[15];
  if (vanhove)
    HIPCHK(s, hipMemcpy(vanhove, s->trk.vh, sizeof(int64_t) * TRK_CLASSES * (size_t)nbins, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_track_displacements(kmc_sim* s, double* u, uint8_t* flags) {
  if (!s) return KMC_ERR_ARG;
  if (!u) return fail(s, KMC_ERR_ARG, "track displacements: u is needed");
  const int rc = rec_check(s, s->trk.rec, TRK_OFF);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N;
  std::vector<double2> h(N);
  HIPCHK(s, hipStreamSynchronize(s->stream));
  HIPCHK(s, hipMemcpy(h.data(), s->trk.dev.u, sizeof(double2) * N, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < N; ++i) {
    u[i] = h[i].x;
    u[N + i] = h[i].y;
  }
  if (flags) {
    HIPCHK(s, hipMemcpy(flags, s->trk.dev.flags, N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) flags[i] &= (uint8_t)(KMC_TRACK_CHANGED | KMC_TRACK_JUMPED);
  }
  return KMC_OK;
}

int kmc_track_end(kmc_sim* s) {
  return s ? rec_end(s, s->trk) : KMC_ERR_ARG;
}

// ---------------------------------------------------------------- bond kinetics
// kmc_kinetics.hip: the recorder is a layer of its own over the committed
// state, independent of the tracker; its calls write only KinState's buffers.

static const char* const KIN_OFF = "kinetics: not begun (kmc_kin_begin; a new state drops the recorder)";

// the counters of the call that just ran; a link out of range drops the recorder
static int kin_result(kmc_sim* s, KinAcc* a) {
  HIPCHK(s, hipMemcpy(a, s->kin.acc, sizeof *a, hipMemcpyDeviceToHost));
  if (a->err) {
    s->kin.rec.on = false;
    return fail(s, KMC_ERR_STATE, "kinetics: a receptor's bond link leaves its range");
  }
  return KMC_OK;
}

static void kin_fill(const kmc_sim* s, const KinAcc& a, kmc_kin_out* out) {
  std::memset(out, 0, sizeof *out);
  out->origin_step = s->kin.rec.origin;
  out->last_step = s->kin.rec.last;
  out->n_updates = s->kin.rec.updates;
  out->rl_on = (int64_t)a.ev[kmck::KIN_EV_RL_ON];
  out->rl_off = (int64_t)a.ev[kmck::KIN_EV_RL_OFF];
  out->rl_swap = (int64_t)a.ev[kmck::KIN_EV_RL_SWAP];
  out->cis_on = (int64_t)a.ev[kmck::KIN_EV_CIS_ON];
  out->cis_off_mono = (int64_t)a.ev[kmck::KIN_EV_CIS_OFF_MONO];
  out->cis_off_cx = (int64_t)a.ev[kmck::KIN_EV_CIS_OFF_CX];
  out->cis_swap = (int64_t)a.ev[kmck::KIN_EV_CIS_SWAP];
  out->exp_rl = s->kin.exp[0];
  out->exp_mono = s->kin.exp[1];
  out->exp_cx = s->kin.exp[2];
  out->exp_free_receptor = s->kin.exp[3];
  out->exp_free_site = s->kin.exp[4];
  out->occ_rl = s->kin.occ[0];
  out->occ_mono = s->kin.occ[1];
  out->occ_cx = s->kin.occ[2];
  out->occ_free_receptor = (int64_t)s->p.n_a - s->kin.occ[0];
  out->occ_free_site = 3 * (int64_t)s->p.n_b - s->kin.occ[0];
}

int kmc_kin_begin(kmc_sim* s) {
  if (!s) return KMC_ERR_ARG;
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  const int NA = s->K.NA;
  if (!s->kin.acc) {
    Scratch& g = s->kin.scratch;
    rc = KMC_OK;
    rc |= salloc(s, g, &s->kin.dev.rl_lig, (size_t)NA);
    rc |= salloc(s, g, &s->kin.dev.rl_site, (size_t)NA);
    rc |= salloc(s, g, &s->kin.dev.cis_with, (size_t)NA);
    rc |= salloc(s, g, &s->kin.dev.last_lig, (size_t)NA);
    rc |= salloc(s, g, &s->kin.dev.rl_since, (size_t)NA);
    rc |= salloc(s, g, &s->kin.dev.cis_since, (size_t)NA);
    rc |= salloc(s, g, &s->kin.dev.free_since, (size_t)NA);
    rc |= salloc(s, g, &s->kin.dev.bits, (size_t)NA);
    rc |= salloc(s, g, &s->kin.hist, (size_t)KIN_HISTS * KIN_BINS);
    rc |= salloc(s, g, &s->kin.acc, 1);
    if (rc != KMC_OK) {
      scratch_drop(s, s->kin);
      return fail(s, KMC_ERR_HIP, "kinetics: scratch allocation failed");
    }
  }
  s->kin.rec.on = false;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemsetAsync(s->kin.acc, 0, sizeof(KinAcc), s->stream));
  HIPCHK(s, hipMemsetAsync(s->kin.hist, 0, sizeof(unsigned long long) * KIN_HISTS * KIN_BINS, s->stream));
  if (NA > 0)
    k_kin_begin<<<(unsigned)((NA + KIN_T - 1) / KIN_T), KIN_T, 0, s->stream>>>(s->K, s->d, s->kin.dev,
                                                                              (long long)s->step_done, s->kin.acc);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  KinAcc a;
  rc = kin_result(s, &a);
  if (rc != KMC_OK) return rc;
  s->kin.rec = Recorder{true, s->step_done, s->step_done, 0};
  for (int k = 0; k < 3; ++k) s->kin.occ[k] = (int64_t)a.occ[k];
  for (auto& e : s->kin.exp) e = 0;
  return KMC_OK;
}

int kmc_kin_update(kmc_sim* s, kmc_kin_out* out) {
  if (!s) return KMC_ERR_ARG;
  int rc = rec_check(s, s->kin.rec, KIN_OFF);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  const int NA = s->K.NA;
  // the events persist since begin; the occupancy and the error flag are of this update
  HIPCHK(s, hipMemsetAsync(s->kin.acc->occ, 0, sizeof(KinAcc) - offsetof(KinAcc, occ), s->stream));
  if (NA > 0)
    k_kin_update<<<(unsigned)((NA + KIN_T - 1) / KIN_T), KIN_T, 0, s->stream>>>(
        s->K, s->d, s->kin.dev, (long long)s->step_done, s->kin.hist, s->kin.acc);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  // the occupancy is the next update's exposure: read back at every update
  KinAcc a;
  rc = kin_result(s, &a);
  if (rc != KMC_OK) return rc;
  const int64_t dt = s->step_done - s->kin.rec.last;
  const int64_t prev[5] = {s->kin.occ[0], s->kin.occ[1], s->kin.occ[2], (int64_t)s->p.n_a - s->kin.occ[0],
                           3 * (int64_t)s->p.n_b - s->kin.occ[0]};
  for (int k = 0; k < 5; ++k) s->kin.exp[k] += dt * prev[k];
  for (int k = 0; k < 3; ++k) s->kin.occ[k] = (int64_t)a.occ[k];
  s->kin.rec.last = s->step_done;
  s->kin.rec.updates += 1;
  if (out) kin_fill(s, a, out);
  return KMC_OK;
}

int kmc_kin_sample(kmc_sim* s, kmc_kin_out* out, int64_t* hist) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "kinetics sample: out is needed");
  int rc = rec_check(s, s->kin.rec, KIN_OFF);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  const int NA = s->K.NA;
  unsigned long long* rows = s->kin.hist + (size_t)KIN_ROWS_UPD * KIN_BINS;
  HIPCHK(s, hipMemsetAsync(rows, 0, sizeof(unsigned long long) * 2 * KIN_BINS, s->stream));
  HIPCHK(s, hipMemsetAsync(s->kin.acc->alive, 0, sizeof(KinAcc) - offsetof(KinAcc, alive), s->stream));
  const int nblk = (NA + KIN_T - 1) / KIN_T;
  if (nblk > 0)
    k_kin_sample<<<(unsigned)std::min(nblk, AN_WG_MAX), KIN_T, 0, s->stream>>>(
        NA, s->kin.dev, (long long)s->kin.rec.last, nblk, rows, s->kin.acc);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  KinAcc a;
  rc = kin_result(s, &a);
  if (rc != KMC_OK) return rc;
  kin_fill(s, a, out);
  out->n_rl_censored_alive = (int64_t)a.alive[0];
  out->n_cis_censored_alive = (int64_t)a.alive[1];
  if (hist)
    HIPCHK(s, hipMemcpy(hist, s->kin.hist, sizeof(int64_t) * KIN_HISTS * KIN_BINS, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_kin_get(kmc_sim* s, const kmc_kin_view* v) {
  if (!s) return KMC_ERR_ARG;
  if (!v || !v->rl_lig || !v->rl_site || !v->rl_since || !v->cis_with || !v->cis_since || !v->last_lig ||
      !v->free_since || !v->bits)
    return fail(s, KMC_ERR_ARG, "kinetics get: the view and its eight arrays are needed");
  const int rc = rec_check(s, s->kin.rec, KIN_OFF);
  if (rc != KMC_OK) return rc;
  const size_t NA = (size_t)s->K.NA;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  HIPCHK(s, hipMemcpy(v->rl_lig, s->kin.dev.rl_lig, sizeof(int32_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->rl_site, s->kin.dev.rl_site, sizeof(int32_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->rl_since, s->kin.dev.rl_since, sizeof(int64_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->cis_with, s->kin.dev.cis_with, sizeof(int32_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->cis_since, s->kin.dev.cis_since, sizeof(int64_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->last_lig, s->kin.dev.last_lig, sizeof(int32_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->free_since, s->kin.dev.free_since, sizeof(int64_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->bits, s->kin.dev.bits, NA, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_kin_end(kmc_sim* s) {
  return s ? rec_end(s, s->kin) : KMC_ERR_ARG;
}

// ---------------------------------------------------------------- cluster growth kinetics
// kmc_coag.hip: a layer of its own over the committed state, independent of
// the tracker and of the kinetics recorder; its calls write only CfState's
// buffers and the analysis scratch an_components fills.

static const char* const CF_OFF = "growth: not begun (kmc_cf_begin; a new state drops the recorder)";

// the counters of the call that just ran (the components' flag included); an
// error drops the recorder
static int cf_result(kmc_sim* s, bool components, CfAcc* a) {
  HIPCHK(s, hipMemcpy(a, s->cf.acc, sizeof *a, hipMemcpyDeviceToHost));
  AnOut o;
  o.err = 0;
  if (components) HIPCHK(s, hipMemcpy(&o, s->an.out, sizeof o, hipMemcpyDeviceToHost));
  if (a->err || o.err) {
    s->cf.rec.on = false;
    return fail(s, KMC_ERR_STATE, "growth: a bond link leaves its range or the link chains do not end");
  }
  return KMC_OK;
}

// the look that a begin, an update or a put just took becomes the last one
static void cf_look(kmc_sim* s, const CfAcc& a) {
  s->cf.clusters = (int64_t)a.n_clusters;
  s->cf.max = (int64_t)a.max_cluster;
  for (int k = 0; k <= CF_MAX_SIZE; ++k) s->cf.ns[k] = (int64_t)a.n_s[k];
}

// every table and counter since begin starts again at `origin`
static int cf_reset(kmc_sim* s, int64_t origin) {
  HIPCHK(s, hipMemsetAsync(s->cf.tab, 0, sizeof(CfTab), s->stream));
  HIPCHK(s, hipMemsetAsync(s->cf.acc, 0, sizeof(CfAcc), s->stream));
  s->cf.rec.origin = s->cf.rec.last = origin;
  s->cf.rec.updates = 0;
  for (auto& e : s->cf.ev) e = 0;
  s->cf.cores = s->cf.closed = s->cf.opened = 0;
  for (auto& e : s->cf.expo) e = 0;
  s->cf.expo2.assign((size_t)(s->cf.S + 1) * (s->cf.S + 1), (__int128)0);
  return KMC_OK;
}

static void cf_fill(const kmc_sim* s, kmc_cf_out* out) {
  std::memset(out, 0, sizeof *out);
  out->origin_step = s->cf.rec.origin;
  out->last_step = s->cf.rec.last;
  out->n_updates = s->cf.rec.updates;
  out->max_size = s->cf.S;
  out->formed_rl = s->cf.ev[CF_EV_FORMED_RL];
  out->formed_cis = s->cf.ev[CF_EV_FORMED_CIS];
  out->broken_rl = s->cf.ev[CF_EV_BROKEN_RL];
  out->broken_cis = s->cf.ev[CF_EV_BROKEN_CIS];
  out->n_cores = s->cf.cores;
  out->n_clusters = s->cf.clusters;
  out->cycles_closed = s->cf.closed;
  out->cycles_opened = s->cf.opened;
  out->max_cluster = s->cf.max;
}

// the components of the current state into the other label / count set, which
// becomes the last look's
static int cf_take_components(kmc_sim* s) {
  const int rc = an_components(s);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N;
  s->cf.cur ^= 1;
  HIPCHK(s, hipMemcpyAsync(s->cf.dev.label[s->cf.cur], s->an.label, sizeof(int32_t) * N, hipMemcpyDeviceToDevice,
                           s->stream));
  HIPCHK(s, hipMemcpyAsync(s->cf.dev.cnt[s->cf.cur], s->an.cnt, sizeof(unsigned long long) * N, hipMemcpyDeviceToDevice,
                           s->stream));
  return KMC_OK;
}

int kmc_cf_begin(kmc_sim* s, int32_t max_size) {
  if (!s) return KMC_ERR_ARG;
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  if (max_size < CF_MIN_SIZE || max_size > CF_MAX_SIZE)
    return fail(s, KMC_ERR_ARG, "growth begin: 2 <= max_size <= " + std::to_string(CF_MAX_SIZE));
  const int NA = s->K.NA, N = s->K.N;
  if (!s->cf.acc) {
    Scratch& g = s->cf.scratch;
    rc = KMC_OK;
    rc |= salloc(s, g, &s->cf.dev.rl_lig, (size_t)NA);
    rc |= salloc(s, g, &s->cf.dev.cis_with, (size_t)NA);
    for (int k = 0; k < 2; ++k) {
      rc |= salloc(s, g, &s->cf.dev.label[k], (size_t)N);
      rc |= salloc(s, g, &s->cf.dev.cnt[k], (size_t)N);
    }
    rc |= salloc(s, g, &s->cf.dev.parent, (size_t)N);
    rc |= salloc(s, g, &s->cf.dev.core, (size_t)N);
    rc |= salloc(s, g, &s->cf.dev.core_cnt, (size_t)N);
    rc |= salloc(s, g, &s->cf.dev.pieces_prev, (size_t)N);
    rc |= salloc(s, g, &s->cf.dev.pieces_cur, (size_t)N);
    rc |= salloc(s, g, &s->cf.tab, 1);
    rc |= salloc(s, g, &s->cf.acc, 1);
    if (rc != KMC_OK) {
      scratch_drop(s, s->cf);
      return fail(s, KMC_ERR_HIP, "growth: scratch allocation failed");
    }
  }
  s->cf.rec.on = false;
  s->cf.S = max_size;
  rc = an_begin(s);
  if (rc == KMC_OK) rc = cf_reset(s, s->step_done);
  if (rc == KMC_OK) rc = cf_take_components(s);
  if (rc != KMC_OK) return rc;
  if (NA > 0) k_cf_begin<<<(unsigned)((NA + CF_T - 1) / CF_T), CF_T, 0, s->stream>>>(s->K, s->d, s->cf.dev, s->cf.acc);
  if (N > 0)
    k_cf_sizes<<<(unsigned)((N + CF_T - 1) / CF_T), CF_T, 0, s->stream>>>(
        s->cf.dev.label[s->cf.cur], s->cf.dev.cnt[s->cf.cur], N, s->cf.S, s->cf.acc);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  CfAcc a;
  rc = cf_result(s, true, &a);
  if (rc != KMC_OK) return rc;
  cf_look(s, a);
  s->cf.rec.on = true;
  return KMC_OK;
}

int kmc_cf_update(kmc_sim* s, kmc_cf_out* out) {
  if (!s) return KMC_ERR_ARG;
  int rc = rec_check(s, s->cf.rec, CF_OFF);
  if (rc != KMC_OK) return rc;
  if (s->step_done == s->cf.rec.last) {  // the state of the last look: nothing to file
    s->cf.rec.updates += 1;
    if (out) cf_fill(s, out);
    return KMC_OK;
  }
  rc = an_begin(s);
  if (rc == KMC_OK) rc = cf_take_components(s);
  if (rc != KMC_OK) return rc;
  const int NA = s->K.NA, N = s->K.N, cur = s->cf.cur, prev = cur ^ 1;
  // the bond counters persist since begin; the rest is of this update
  HIPCHK(s, hipMemsetAsync(&s->cf.acc->n_cores, 0, sizeof(CfAcc) - offsetof(CfAcc, n_cores), s->stream));
  const unsigned g = (unsigned)((N + CF_T - 1) / CF_T);
  if (g) {
    k_cf_init<<<g, CF_T, 0, s->stream>>>(s->cf.dev, N);
    if (NA > 0) k_cf_hook<<<(unsigned)((NA + CF_T - 1) / CF_T), CF_T, 0, s->stream>>>(s->K, s->d, s->cf.dev, s->cf.acc);
    k_cf_flatten<<<g, CF_T, 0, s->stream>>>(s->cf.dev, s->cf.dev.label[prev], s->cf.dev.label[cur], NA, N, s->cf.acc);
    k_cf_events<<<g, CF_T, 0, s->stream>>>(s->cf.dev, s->cf.dev.label[prev], s->cf.dev.cnt[prev], s->cf.dev.label[cur],
                                           s->cf.dev.cnt[cur], N, s->cf.S, s->cf.tab, s->cf.acc);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  CfAcc a;
  rc = cf_result(s, true, &a);
  if (rc != KMC_OK) return rc;
  // exposures of the interval that ended, from the previous look's n_s
  const int S = s->cf.S;
  const int64_t dt = s->step_done - s->cf.rec.last;
  for (int x = 1; x <= S; ++x) {
    const int64_t nx = s->cf.ns[x];
    s->cf.expo[x] += dt * nx;
    s->cf.expo2[(size_t)x * (S + 1) + x] += (__int128)dt * nx * (nx - 1) / 2;
    for (int y = x + 1; y <= S; ++y) s->cf.expo2[(size_t)x * (S + 1) + y] += (__int128)dt * nx * s->cf.ns[y];
  }
  // the change of the cycle rank, from this update's bonds
  int64_t ev[CF_NEV];
  for (int k = 0; k < CF_NEV; ++k) ev[k] = (int64_t)a.ev[k] - s->cf.ev[k];
  const int64_t formed = ev[CF_EV_FORMED_RL] + ev[CF_EV_FORMED_CIS], broken = ev[CF_EV_BROKEN_RL] + ev[CF_EV_BROKEN_CIS];
  const int64_t cores = (int64_t)a.n_cores;
  s->cf.closed += formed - (cores - (int64_t)a.n_clusters);
  s->cf.opened += broken - (cores - s->cf.clusters);
  for (int k = 0; k < CF_NEV; ++k) s->cf.ev[k] = (int64_t)a.ev[k];
  s->cf.cores = cores;
  cf_look(s, a);
  s->cf.rec.last = s->step_done;
  s->cf.rec.updates += 1;
  if (out) cf_fill(s, out);
  return KMC_OK;
}

int kmc_cf_sample(kmc_sim* s, kmc_cf_out* out, const kmc_cf_tables* t) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "growth sample: out is needed");
  const int rc = rec_check(s, s->cf.rec, CF_OFF);
  if (rc != KMC_OK) return rc;
  cf_fill(s, out);
  if (!t) return KMC_OK;
  const int S = s->cf.S;
  const size_t n1 = (size_t)S + 1, n2 = n1 * n1;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  auto pull = [&](int64_t* dst, const unsigned long long* src, size_t n) -> hipError_t {
    return dst ? hipMemcpy(dst, src, sizeof(int64_t) * n, hipMemcpyDeviceToHost) : hipSuccess;
  };
  HIPCHK(s, pull(t->merge, s->cf.tab->merge, n2));
  HIPCHK(s, pull(t->frag, s->cf.tab->frag, n2));
  HIPCHK(s, pull(t->merge_kind, s->cf.tab->merge_kind, CF_KINDS * CF_KINDS));
  HIPCHK(s, pull(t->frag_kind, s->cf.tab->frag_kind, CF_KINDS * CF_KINDS));
  HIPCHK(s, pull(t->merge_pieces, s->cf.tab->merge_pieces, CF_PIECES));
  HIPCHK(s, pull(t->frag_pieces, s->cf.tab->frag_pieces, CF_PIECES));
  HIPCHK(s, pull(t->merge_product, s->cf.tab->merge_product, n1));
  HIPCHK(s, pull(t->frag_parent, s->cf.tab->frag_parent, n1));
  if (t->n_s) std::copy(s->cf.ns, s->cf.ns + n1, t->n_s);
  if (t->expo) std::copy(s->cf.expo, s->cf.expo + n1, t->expo);
  if (t->expo2)
    for (size_t b = 0; b < n2; ++b) {
      t->expo2[b].lo = (uint64_t)(unsigned __int128)s->cf.expo2[b];
      t->expo2[b].hi = (int64_t)(s->cf.expo2[b] >> 64);
    }
  return KMC_OK;
}

int kmc_cf_get(kmc_sim* s, const kmc_cf_view* v) {
  if (!s) return KMC_ERR_ARG;
  if (!v || !v->rl_lig || !v->cis_with || !v->prev_label)
    return fail(s, KMC_ERR_ARG, "growth get: the view and its three arrays are needed");
  const int rc = rec_check(s, s->cf.rec, CF_OFF);
  if (rc != KMC_OK) return rc;
  const size_t NA = (size_t)s->K.NA, N = (size_t)s->K.N;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  HIPCHK(s, hipMemcpy(v->rl_lig, s->cf.dev.rl_lig, sizeof(int32_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->cis_with, s->cf.dev.cis_with, sizeof(int32_t) * NA, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(v->prev_label, s->cf.dev.label[s->cf.cur], sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < N; ++i) v->prev_label[i] += 1;
  return KMC_OK;
}

int kmc_cf_put(kmc_sim* s, const kmc_cf_view* v, int64_t last_step) {
  if (!s) return KMC_ERR_ARG;
  if (!v || !v->rl_lig || !v->cis_with || !v->prev_label)
    return fail(s, KMC_ERR_ARG, "growth put: the view and its three arrays are needed");
  int rc = rec_check(s, s->cf.rec, CF_OFF);
  if (rc != KMC_OK) return rc;
  if (last_step > s->step_done) return fail(s, KMC_ERR_ARG, "growth put: last_step lies after the current step");
  const int NA = s->K.NA, N = s->K.N;
  for (int i = 0; i < NA; ++i) {
    const int32_t l = v->rl_lig[i], c = v->cis_with[i];
    if ((l != 0 && (l <= NA || l > N)) || (c != 0 && (c < 1 || c > NA || c == i + 1)))
      return fail(s, KMC_ERR_STATE, "growth put: a stored bond of receptor " + std::to_string(i + 1) + " leaves its range");
  }
  std::vector<int32_t> lab((size_t)N);
  for (int i = 0; i < N; ++i) {
    const int32_t l = v->prev_label[i];
    // a class' label is one of its members, labelled by itself, and no member lies below it
    if (l < 1 || l > i + 1 || v->prev_label[l - 1] != l)
      return fail(s, KMC_ERR_STATE, "growth put: the label of protein " + std::to_string(i + 1) +
                                        " is out of range or not the smallest member of its class");
    lab[(size_t)i] = l - 1;
  }
  rc = an_begin(s);
  if (rc == KMC_OK) rc = cf_reset(s, last_step);
  if (rc != KMC_OK) return rc;
  const int cur = s->cf.cur;
  hipStream_t st = s->stream;
  HIPCHK(s, hipMemcpyAsync(s->cf.dev.rl_lig, v->rl_lig, sizeof(int32_t) * (size_t)NA, hipMemcpyHostToDevice, st));
  HIPCHK(s, hipMemcpyAsync(s->cf.dev.cis_with, v->cis_with, sizeof(int32_t) * (size_t)NA, hipMemcpyHostToDevice, st));
  HIPCHK(s, hipMemcpyAsync(s->cf.dev.label[cur], lab.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, st));
  HIPCHK(s, hipMemsetAsync(s->cf.dev.cnt[cur], 0, sizeof(unsigned long long) * (size_t)N, st));
  const unsigned g = (unsigned)((N + CF_T - 1) / CF_T);
  if (g) {
    k_an_count<<<g, AN_T, 0, st>>>(s->cf.dev.label[cur], s->cf.dev.cnt[cur], NA, N);
    k_cf_sizes<<<g, CF_T, 0, st>>>(s->cf.dev.label[cur], s->cf.dev.cnt[cur], N, s->cf.S, s->cf.acc);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);  // (waits: lab is read by the copy until here)
  if (rc != KMC_OK) return rc;
  CfAcc a;
  rc = cf_result(s, false, &a);
  if (rc != KMC_OK) return rc;
  cf_look(s, a);
  return KMC_OK;
}

int kmc_cf_end(kmc_sim* s) {
  return s ? rec_end(s, s->cf) : KMC_ERR_ARG;
}

// ---------------------------------------------------------------- ligand network and rings
// kmc_rings.hip: read-only like the analysis above, on scratch of its own.

static_assert(KMC_RING_MAX == RG_MAX, "kmc.h and kmc_rings.h agree on the longest ring");
static_assert(sizeof(kmc_net_out) == 11 * sizeof(int64_t), "kmc_net_out layout");

// The component labels (on the layer's own buffers), the adjacency with its
// bins, counters and worklist and, for max_len > 0, the rings, left on the
// device: five launches, or six.  The stream is not waited for.
static int rg_run(kmc_sim* s, int max_len, bool members) {
  const int N = s->K.N, NA = s->K.NA, NB = s->K.NB;
  RgState& r = s->rg;
  if (!r.out) {
    int rc = KMC_OK;
    rc |= dalloc(s, &r.parent, (size_t)N);
    rc |= dalloc(s, &r.label, (size_t)N);
    rc |= dalloc(s, &r.cnt, (size_t)N);
    rc |= dalloc(s, &r.flag, (size_t)N);
    rc |= dalloc(s, &r.an_out, 1);
    rc |= dalloc(s, &r.rows, (size_t)NB);
    rc |= dalloc(s, &r.work, (size_t)NB);
    rc |= dalloc(s, &r.member, 2 * (size_t)NB);
    rc |= dalloc(s, &r.out, 1);
    if (rc != KMC_OK) return fail(s, KMC_ERR_HIP, "rings: scratch allocation failed");
  }
  hipStream_t st = s->stream;
  HIPCHK(s, hipMemsetAsync(r.an_out, 0, sizeof(AnOut), st));
  HIPCHK(s, hipMemsetAsync(r.out, 0, sizeof(RgOut), st));
  HIPCHK(s, hipMemsetAsync(r.flag, 0, sizeof(int32_t) * (size_t)N, st));
  if (members && NB > 0) HIPCHK(s, hipMemsetAsync(r.member, 0, sizeof(uint32_t) * 2 * (size_t)NB, st));
  const unsigned g = (unsigned)((N + AN_T - 1) / AN_T);
  if (g) {
    k_an_init<<<g, AN_T, 0, st>>>(r.parent, r.cnt, N);
    k_an_hook<<<g, AN_T, 0, st>>>(s->K, s->d, r.parent, r.an_out);
    k_an_flatten<<<g, AN_T, 0, st>>>(r.parent, r.label, N, r.an_out);
    k_rg_adj<<<(unsigned)((std::max(NA, NB) + RG_T - 1) / RG_T), RG_T, 0, st>>>(s->K, s->d, r.label, r.flag, r.rows,
                                                                                r.work, r.out);
  }
  if (max_len > 0 && NB > 0) {
    // a task a lane, three tasks a worklist entry; the worklist's length is known on the device only
    const unsigned gr = (unsigned)std::min<int64_t>(RG_WG_MAX, (3 * (int64_t)NB + RG_T - 1) / RG_T);
    k_rg_rings<<<gr, RG_T, 0, st>>>(NB, max_len, r.rows, r.work, members ? r.member : nullptr, r.out);
  }
  HIPCHK(s, hipGetLastError());
  return KMC_OK;
}

// the device's verdict of the last call and its counters
static int rg_result(kmc_sim* s, RgOut* o, kmc_net_out* out) {
  AnOut a;
  HIPCHK(s, hipMemcpy(&a, s->rg.an_out, sizeof a, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(o, s->rg.out, sizeof *o, hipMemcpyDeviceToHost));
  if (a.err || o->err)
    return fail(s, KMC_ERR_STATE, "rings: a bond link of the wrong kind, an asymmetric bridge or a link that leaves the state");
  if (out) {
    const unsigned long long* c = o->bins + 20;
    out->n_bridges = (int64_t)c[RG_BRIDGES];
    out->n_loops = (int64_t)c[RG_LOOPS];
    out->n_half = (int64_t)c[RG_HALF];
    out->n_free_dimers = (int64_t)c[RG_FREE_DIMERS];
    out->n_vertices = (int64_t)c[RG_VERTICES];
    out->n_net_components = (int64_t)c[RG_COMPONENTS];
    out->cycle_rank = out->n_bridges - out->n_vertices + out->n_net_components;
    for (int k = 0; k < 4; ++k) out->rec[k] = (int64_t)o->bins[16 + k];
  }
  return KMC_OK;
}

int kmc_network(kmc_sim* s, kmc_net_out* out, int64_t* lig_hist, int32_t* adj_lig, int32_t* adj_site) {
  if (!s) return KMC_ERR_ARG;
  int rc = an_check(s);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = rg_run(s, 0, false);
  if (rc == KMC_OK) rc = an_end(s);
  if (rc != KMC_OK) return rc;
  RgOut o;
  rc = rg_result(s, &o, out);
  if (rc != KMC_OK) return rc;
  if (lig_hist)
    for (int k = 0; k < 16; ++k) lig_hist[k] = (int64_t)o.bins[k];
  const size_t NB = (size_t)s->K.NB;
  if ((adj_lig || adj_site) && NB) {
    std::vector<int4> rows(NB);
    HIPCHK(s, hipMemcpy(rows.data(), s->rg.rows, sizeof(int4) * NB, hipMemcpyDeviceToHost));
    auto ref = [&](size_t slot) { return (size_t)((uint32_t)rows[slot].w >> 8); };  // checked by the kernel: < NB
    for (size_t b = 0; b < NB; ++b) {
      const int32_t l[3] = {rows[b].x, rows[b].y, rows[b].z};  // slots + 1 in [0, NB]
      for (int e = 0; e < 3; ++e) {
        if (adj_lig) adj_lig[3 * ref(b) + e] = l[e] ? (int32_t)ref((size_t)l[e] - 1) + 1 : 0;
        if (adj_site) adj_site[3 * ref(b) + e] = l[e] ? (int32_t)(((uint32_t)rows[b].w >> (2 * e)) & 3u) + 2 : 0;
      }
    }
  }
  return KMC_OK;
}

int64_t kmc_rings_hops(const kmc_sim* s) { return s ? s->rg.hops : 0; }

int kmc_rings(kmc_sim* s, int32_t max_len, int64_t* counts, uint32_t* member, kmc_net_out* out) {
  if (!s) return KMC_ERR_ARG;
  if (!counts || max_len < 1 || max_len > RG_MAX)
    return fail(s, KMC_ERR_ARG, "rings: counts is needed, 1 <= max_len <= " + std::to_string(RG_MAX));
  int rc = an_check(s);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = rg_run(s, max_len, member != nullptr);
  if (rc == KMC_OK) rc = an_end(s);
  if (rc != KMC_OK) return rc;
  RgOut o;
  rc = rg_result(s, &o, out);
  if (rc != KMC_OK) return rc;
  for (int k = 0; k < 2 * (RG_MAX + 1); ++k) counts[k] = (int64_t)(&o.counts[0][0])[k];
  s->rg.hops = (int64_t)o.hops;
  const size_t NB = (size_t)s->K.NB;
  if (member && NB) HIPCHK(s, hipMemcpy(member, s->rg.member, sizeof(uint32_t) * 2 * NB, hipMemcpyDeviceToHost));
  return KMC_OK;
}

// ---------------------------------------------------------------- lag correlator
// kmc_lagcorr.hip: a recorder of its own over the committed state, independent
// of the tracker; its calls write only LagState's buffers.  Unlike the other
// recorders its memory depends on the configuration (the rings): begin
// allocates it, end frees it.

static_assert(KMC_LAG_MAX_LEVELS == LAG_MAX_LEVELS && KMC_LAG_MAX_SLOTS == LAG_MAX_SLOTS && KMC_LAG_MAX_Q == LAG_MAX_Q &&
                  KMC_LAG_CLASSES == LAG_CLASSES && KMC_LAG_MAX_ROWS == LAG_MAX_ROWS,
              "kmc.h and kmc_lagcorr.h agree");
static_assert(sizeof(kmc_lag_cell) == sizeof(lag_u64) * LAG_CELL, "a table cell is LAG_CELL words");
static_assert(offsetof(kmc_lag_cell, m2_all) == 24 && offsetof(kmc_lag_cell, m4_clean) == 56 &&
                  offsetof(kmc_lag_cell, fs) == 72,
              "kmc_lag_cell is the layout lag_flush adds into");

static const char* const LAG_OFF = "lag: not begun (kmc_lag_begin; a new state drops the recorder)";

int kmc_lag_begin(kmc_sim* s, const kmc_lag_config* cfg) {
  if (!s) return KMC_ERR_ARG;
  if (!cfg) return fail(s, KMC_ERR_ARG, "lag: the configuration is needed");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  kmc_lag_config c = *cfg;
  for (int k = std::max(0, std::min(c.nq, LAG_MAX_Q)); k < LAG_MAX_Q; ++k) c.h[k] = 0;
  int64_t J, F, BX, BY;
  const char* bad = kmcl::check(c.every, c.levels, c.slots, c.nq, c.h, s->K.box_x, s->K.box_y, &c.max_jump, &c.max_disp,
                                &J, &F, &BX, &BY);
  if (bad) return fail(s, KMC_ERR_ARG, bad);
  // a recorder that was on ends here, whatever becomes of this call
  rc = rec_end(s, s->lag);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N;
  const int L = c.levels, P = c.slots, rows = kmcl::rows(L, P);
  Scratch& g = s->lag.scratch;
  rc = KMC_OK;
  rc |= salloc(s, g, &s->lag.dev.prev, N);
  rc |= salloc(s, g, &s->lag.dev.U, N);
  rc |= salloc(s, g, &s->lag.dev.links, 3 * N);
  rc |= salloc(s, g, &s->lag.dev.last_event, N);
  rc |= salloc(s, g, &s->lag.dev.cls, N);
  rc |= salloc(s, g, &s->lag.tasks, (size_t)LAG_MAX_ROWS);
  rc |= salloc(s, g, &s->lag.table, (size_t)rows * LAG_CLASSES * LAG_CELL);
  rc |= salloc(s, g, &s->lag.n_events, 1);
  if (rc == KMC_OK) rc |= salloc(s, g, &s->lag.dev.ring, (size_t)L * P * N);
  if (rc != KMC_OK) {
    scratch_drop(s, s->lag);
    return fail(s, KMC_ERR_HIP, "lag: allocation failed (the rings take levels * slots * 16 bytes per protein)");
  }
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  if (N > 0) k_lag_begin<<<(unsigned)((N + LAG_T - 1) / LAG_T), LAG_T, 0, s->stream>>>(s->K, s->d, s->lag.dev, L, P);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  s->lag.cfg = c;
  LagArgs& a = s->lag.a;
  a.BX = BX;
  a.BY = BY;
  a.J = J;
  a.F = F;
  a.L = L;
  a.P = P;
  a.nq = c.nq;
  for (int k = 0; k < LAG_MAX_Q; ++k) a.h[k] = c.h[k];
  s->lag.rec = Recorder{true, s->step_done, s->step_done, 0};
  return KMC_OK;
}

int kmc_lag_update(kmc_sim* s, kmc_lag_info* info) {
  if (!s) return KMC_ERR_ARG;
  int rc = rec_check(s, s->lag.rec, LAG_OFF);
  if (rc != KMC_OK) return rc;
  LagState& g = s->lag;
  if (s->step_done != g.rec.last + g.cfg.every)
    return fail(s, KMC_ERR_ARG, "lag: an update is due " + std::to_string(g.cfg.every) + " steps after the last one");
  if (g.rec.updates >= INT32_MAX) return fail(s, KMC_ERR_ARG, "lag: the update counter is full");
  const int64_t n = g.rec.updates + 1;
  kmcl::Task tasks[LAG_MAX_ROWS];
  const int nt = kmcl::tasks(n, g.a.L, g.a.P, tasks);
  g.a.n = (int)n;
  g.a.ntasks = nt;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N;
  const int nblk = (N + LAG_T - 1) / LAG_T;
  HIPCHK(s, hipMemcpyAsync(g.tasks, tasks, sizeof(kmcl::Task) * (size_t)nt, hipMemcpyHostToDevice, s->stream));
  HIPCHK(s, hipMemsetAsync(g.n_events, 0, sizeof(lag_u64), s->stream));
  if (nblk > 0) {
    const size_t lds = sizeof(lag_u64) * (size_t)(std::min(nt, LAG_CHUNK) * LAG_CLASSES * LAG_W);
    k_lag_update<<<(unsigned)std::min(nblk, AN_WG_MAX), LAG_T, lds, s->stream>>>(s->K, s->d, g.dev, g.a, g.tasks, nblk,
                                                                                g.table, g.n_events);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);  // (waits: tasks is read by the copy until here)
  if (rc != KMC_OK) {
    g.rec.on = false;  // the per-protein state may be half advanced
    return rc;
  }
  for (int t = 0; t < nt; ++t) g.n_pairs[tasks[t].row] += 1;
  g.rec.last = s->step_done;
  g.rec.updates = n;
  if (info) {
    lag_u64 ne = 0;
    HIPCHK(s, hipMemcpy(&ne, g.n_events, sizeof ne, hipMemcpyDeviceToHost));
    info->n_updates = n;
    info->n_tasks = nt;
    info->n_events = (int64_t)ne;
  }
  return KMC_OK;
}

int kmc_lag_sample(kmc_sim* s, kmc_lag_out* out, kmc_lag_cell* table, int64_t* n_pairs) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "lag sample: out is needed");
  int rc = rec_check(s, s->lag.rec, LAG_OFF);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = an_end(s);  // (no device work: the time of this call is that of its copy's wait)
  if (rc != KMC_OK) return rc;
  const LagState& g = s->lag;
  const int rows = kmcl::rows(g.a.L, g.a.P);
  std::memset(out, 0, sizeof *out);
  out->cfg = g.cfg;
  out->J = g.a.J;
  out->F = g.a.F;
  out->BX = g.a.BX;
  out->BY = g.a.BY;
  out->origin_step = g.rec.origin;
  out->last_step = g.rec.last;
  out->n_updates = g.rec.updates;
  out->rows = rows;
  if (table)
    HIPCHK(s, hipMemcpy(table, g.table, sizeof(kmc_lag_cell) * (size_t)rows * LAG_CLASSES, hipMemcpyDeviceToHost));
  if (n_pairs) std::copy(g.n_pairs, g.n_pairs + rows, n_pairs);
  return KMC_OK;
}

int kmc_lag_arrays(kmc_sim* s, int64_t* U, int32_t* last_event) {
  if (!s) return KMC_ERR_ARG;
  const int rc = rec_check(s, s->lag.rec, LAG_OFF);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  static_assert(sizeof(longlong2) == 2 * sizeof(int64_t), "U [N][2] is the device's longlong2 [N]");
  if (U && N) HIPCHK(s, hipMemcpy(U, s->lag.dev.U, sizeof(longlong2) * N, hipMemcpyDeviceToHost));
  if (last_event && N) HIPCHK(s, hipMemcpy(last_event, s->lag.dev.last_event, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_lag_end(kmc_sim* s) {
  return s ? rec_end(s, s->lag) : KMC_ERR_ARG;
}

// ---------------------------------------------------------------- pair dynamics
// kmc_pairdyn.hip: a recorder with one origin, on the lag correlator's life
// cycle (begin allocates, end frees).  Its update advances the per-protein
// state only; the sample does the device work: it bins the current positions
// and runs the two pair walks into tables it zeroed.

static_assert(KMC_PD_MAX_BINS == PD_MAX_BINS && KMC_PD_JUMPED == PD_JUMPED, "kmc.h and kmc_pairdyn.h agree");
static_assert(sizeof(kmc_pd_cell) == sizeof(pd_u64) * PD_CU_WORDS && offsetof(kmc_pd_cell, dot) == 16 &&
                  offsetof(kmc_pd_cell, sq) == 32,
              "kmc_pd_cell is the layout k_pd_walk adds into");

static const char* const PD_OFF = "pd: not begun (kmc_pd_begin; a new state drops the recorder)";

int kmc_pd_begin(kmc_sim* s, const kmc_pd_config* cfg) {
  if (!s) return KMC_ERR_ARG;
  if (!cfg) return fail(s, KMC_ERR_ARG, "pd: the configuration is needed");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  kmc_pd_config c = *cfg;
  kmcp::Grid G;
  int64_t E[PD_MAX_BINS + 1];
  const char* bad = kmcp::check(c.every, c.nbins, c.r_max, s->K.box_x, s->K.box_y, &c.max_jump, &c.max_disp, &G, E);
  if (bad) return fail(s, KMC_ERR_ARG, bad);
  // a recorder that was on ends here, whatever becomes of this call
  rc = rec_end(s, s->pd);
  if (rc != KMC_OK) return rc;
  // debug: the pair walks stage fewer points at a time
  s->pd.chunk = (int)int_getenv("KMC_DEBUG_PD_CHUNK", PD_CHUNK, 1, PD_CHUNK);
  const size_t N = (size_t)s->K.N, ncnt = (size_t)G.ncx * G.ncy + 1;
  const int nb = G.nbins;
  Scratch& g = s->pd.scratch;
  Pd& D = s->pd.dev;
  rc = KMC_OK;
  rc |= salloc(s, g, &D.prev, N);
  rc |= salloc(s, g, &D.U, N);
  rc |= salloc(s, g, &D.X0, N);
  rc |= salloc(s, g, &D.flags, N);
  rc |= salloc(s, g, &D.opos, N);
  rc |= salloc(s, g, &D.opt, N);
  rc |= salloc(s, g, &D.npt, N);
  rc |= salloc(s, g, &D.upl, N);
  rc |= salloc(s, g, &D.cell, N);
  rc |= salloc(s, g, &D.rank, N);
  rc |= salloc(s, g, &D.ccnt, ncnt);
  rc |= salloc(s, g, &D.ocstart, ncnt);
  rc |= salloc(s, g, &D.ncstart, ncnt);
  rc |= salloc(s, g, &D.part, (ncnt + SCAN_TILE - 1) / SCAN_TILE);
  rc |= salloc(s, g, &D.E2, (size_t)nb + 1);
  rc |= salloc(s, g, &D.out, (size_t)(PD_A_BINS + PD_B_KINDS * PD_CU_WORDS) * nb + 1);
  if (rc != KMC_OK) {
    scratch_drop(s, s->pd);
    return fail(s, KMC_ERR_HIP, "pd: allocation failed (109 bytes per protein and 12 per cell of the search grid)");
  }
  pd_u64 E2[PD_MAX_BINS + 1];
  for (int m = 0; m <= nb; ++m) E2[m] = (pd_u64)E[m] * (pd_u64)E[m];
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpyAsync(D.E2, E2, sizeof(pd_u64) * (size_t)(nb + 1), hipMemcpyHostToDevice, s->stream));
  if (N > 0) {
    const unsigned gr = (unsigned)((N + PD_T - 1) / PD_T);
    k_pd_begin<<<gr, PD_T, 0, s->stream>>>(s->K, s->d, D, G);  // (ccnt is zero: salloc)
    bins_scan(s, D.ccnt, D.ocstart, (int)ncnt, D.part);
    k_pd_origin_scatter<<<gr, PD_T, 0, s->stream>>>((int)N, D, G);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);  // (waits: E2 is read by the copy until here)
  if (rc != KMC_OK) {
    scratch_drop(s, s->pd);
    return rc;
  }
  s->pd.cfg = c;
  s->pd.G = G;
  s->pd.inv_dr = (float)((double)nb / (double)E[nb]);
  s->pd.rec = Recorder{true, s->step_done, s->step_done, 0};
  return KMC_OK;
}

int kmc_pd_update(kmc_sim* s, kmc_pd_info* info) {
  if (!s) return KMC_ERR_ARG;
  int rc = rec_check(s, s->pd.rec, PD_OFF);
  if (rc != KMC_OK) return rc;
  PdState& g = s->pd;
  if (s->step_done != g.rec.last + g.cfg.every)
    return fail(s, KMC_ERR_ARG, "pd: an update is due " + std::to_string(g.cfg.every) + " steps after the last one");
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N, nblk = (N + PD_T - 1) / PD_T;
  pd_u64* n_jumped = g.dev.out + (size_t)(PD_A_BINS + PD_B_KINDS * PD_CU_WORDS) * g.G.nbins;
  HIPCHK(s, hipMemsetAsync(n_jumped, 0, sizeof(pd_u64), s->stream));
  if (nblk > 0)
    k_pd_update<<<(unsigned)std::min(nblk, AN_WG_MAX), PD_T, 0, s->stream>>>(s->K, s->d, g.dev, g.G, nblk, n_jumped);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) {
    g.rec.on = false;  // the per-protein state may be half advanced
    return rc;
  }
  g.rec.last = s->step_done;
  g.rec.updates += 1;
  if (info) {
    pd_u64 nj = 0;
    HIPCHK(s, hipMemcpy(&nj, n_jumped, sizeof nj, hipMemcpyDeviceToHost));
    info->n_updates = g.rec.updates;
    info->n_jumped = (int64_t)nj;
  }
  return KMC_OK;
}

int kmc_pd_sample(kmc_sim* s, kmc_pd_out* out, int64_t* gd, int64_t* gs, kmc_pd_cell* cu) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "pd sample: out is needed");
  int rc = rec_check(s, s->pd.rec, PD_OFF);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  PdState& g = s->pd;
  const kmcp::Grid& G = g.G;
  const int N = s->K.N, nb = G.nbins, ncell = G.ncx * G.ncy;
  const size_t nout = (size_t)(PD_A_BINS + PD_B_KINDS * PD_CU_WORDS) * nb;
  const bool part_a = gd || gs, part_b = cu != nullptr;
  hipStream_t st = s->stream;
  if (part_a || part_b) HIPCHK(s, hipMemsetAsync(g.dev.out, 0, sizeof(pd_u64) * nout, st));
  if ((part_a || part_b) && N > 0) {
    const Pd& D = g.dev;
    const unsigned gr = (unsigned)((N + PD_T - 1) / PD_T);
    const unsigned gw = (unsigned)std::min((ncell + PD_WAVES - 1) / PD_WAVES, AN_WG_MAX);
    HIPCHK(s, hipMemsetAsync(D.ccnt, 0, sizeof(int32_t) * (size_t)(ncell + 1), st));
    k_pd_now<<<gr, PD_T, 0, st>>>(N, D, G);
    bins_scan(s, D.ccnt, D.ncstart, ncell + 1, D.part);
    k_pd_now_scatter<<<gr, PD_T, 0, st>>>(N, D, G);
    const size_t fixed = sizeof(pd_u64) * (size_t)(nb + 1);
    if (part_a)
      k_pd_walk<false><<<gw, PD_T, sizeof(int4) * 2 * PD_WAVES * (size_t)g.chunk + fixed + sizeof(pd_u64) * PD_A_BINS * nb,
                         st>>>(D, G, s->K.NA, g.chunk, g.inv_dr);
    if (part_b)
      k_pd_walk<true><<<gw, PD_T,
                        sizeof(int4) * 4 * PD_WAVES * (size_t)g.chunk + fixed +
                            sizeof(pd_u64) * PD_B_KINDS * PD_CU_WORDS * nb,
                        st>>>(D, G, s->K.NA, g.chunk, g.inv_dr);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  std::memset(out, 0, sizeof *out);
  out->cfg = g.cfg;
  out->J = G.J;
  out->F = G.F;
  out->BX = G.BX;
  out->BY = G.BY;
  out->ncx = G.ncx;
  out->ncy = G.ncy;
  out->origin_step = g.rec.origin;
  out->last_step = g.rec.last;
  out->n_updates = g.rec.updates;
  static_assert(sizeof(pd_u64) == sizeof(int64_t), "the bins are copied out as they are");
  if (gd) HIPCHK(s, hipMemcpy(gd, g.dev.out, sizeof(pd_u64) * 4 * (size_t)nb, hipMemcpyDeviceToHost));
  if (gs) HIPCHK(s, hipMemcpy(gs, g.dev.out + 4 * (size_t)nb, sizeof(pd_u64) * 2 * (size_t)nb, hipMemcpyDeviceToHost));
  if (cu)
    HIPCHK(s, hipMemcpy(cu, g.dev.out + (size_t)PD_A_BINS * nb, sizeof(kmc_pd_cell) * PD_B_KINDS * (size_t)nb,
                        hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_pd_arrays(kmc_sim* s, int64_t* U, int64_t* X0, uint8_t* flags) {
  if (!s) return KMC_ERR_ARG;
  const int rc = rec_check(s, s->pd.rec, PD_OFF);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  if (U && N) HIPCHK(s, hipMemcpy(U, s->pd.dev.U, sizeof(longlong2) * N, hipMemcpyDeviceToHost));
  if (X0 && N) HIPCHK(s, hipMemcpy(X0, s->pd.dev.X0, sizeof(longlong2) * N, hipMemcpyDeviceToHost));
  if (flags && N) HIPCHK(s, hipMemcpy(flags, s->pd.dev.flags, N, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_pd_end(kmc_sim* s) {
  return s ? rec_end(s, s->pd) : KMC_ERR_ARG;
}

// ---------------------------------------------------------------- body dynamics
// kmc_bodydyn.hip: a recorder with one origin, on the pair dynamics' life cycle
// (begin allocates, end frees).  The begin runs the geometry layer's unwrap
// once and sorts the members by body; the update advances the per-protein
// state; the sample labels the current components and runs the segmented
// reduction and the finish into a table it zeroed.

static_assert(KMC_BD_MAX_SIZE == BD_MAX_SIZE && KMC_BD_ROT_MAX == BD_ROT_MAX && KMC_BD_JUMPED == BD_JUMPED &&
                  KMC_BD_CHANGED == BD_CHANGED && KMC_BD_WIDE == BD_WIDE && KMC_BD_INTACT == BD_INTACT &&
                  KMC_BD_GROWN == BD_GROWN && KMC_BD_BROKEN == BD_BROKEN &&
                  KMC_BD_IS_PRISTINE == BD_IS_PRISTINE && KMC_BD_IS_VALID == BD_IS_VALID &&
                  KMC_BD_IS_ROT == BD_IS_ROT,
              "kmc.h and kmc_bodydyn.h agree");
static_assert(sizeof(kmc_bd_cell) == sizeof(bd_u64) * BD_CELL_WORDS &&
                  offsetof(kmc_bd_cell, n_intact) == 8 * BD_W_INTACT &&
                  offsetof(kmc_bd_cell, n_broken) == 8 * BD_W_BROKEN && offsetof(kmc_bd_cell, c1) == 8 * BD_W_C1 &&
                  offsetof(kmc_bd_cell, m2) == 8 * BD_W_M2 && offsetof(kmc_bd_cell, phi2) == 8 * BD_W_PHI2,
              "kmc_bd_cell is the layout k_bd_finish adds into");
static_assert(sizeof(kmc_bd_body) == 64, "kmc_bd_body layout");

static const char* const BD_OFF = "bd: not begun (kmc_bd_begin; a new state drops the recorder)";

int kmc_bd_begin(kmc_sim* s, const kmc_bd_config* cfg) {
  if (!s) return KMC_ERR_ARG;
  if (!cfg) return fail(s, KMC_ERR_ARG, "bd: the configuration is needed");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  kmc_bd_config c = *cfg;
  int64_t J, F, BX, BY;
  const char* bad = kmcb::check(c.every, c.max_size, s->K.box_x, s->K.box_y, &c.max_jump, &c.max_disp, &J, &F, &BX, &BY);
  if (bad) return fail(s, KMC_ERR_ARG, bad);
  // a recorder that was on ends here, whatever becomes of this call
  rc = rec_end(s, s->bd);
  if (rc != KMC_OK) return rc;
  // debug: the segmented reduction takes shorter spans of the member list
  s->bd.span = (int)int_getenv("KMC_DEBUG_BD_SPAN", BD_SPAN, 1, BD_SPAN);
  const size_t N = (size_t)s->K.N;
  Scratch& g = s->bd.scratch;
  Bd& D = s->bd.dev;
  rc = KMC_OK;
  rc |= salloc(s, g, &D.prev, N);
  rc |= salloc(s, g, &D.U, N);
  rc |= salloc(s, g, &D.X0, N);
  rc |= salloc(s, g, &D.D0, N);
  rc |= salloc(s, g, &D.links, 3 * N);
  rc |= salloc(s, g, &D.flags, N);
  rc |= salloc(s, g, &D.label, N);
  rc |= salloc(s, g, &D.list, N);
  rc |= salloc(s, g, &D.rank, N);
  rc |= salloc(s, g, &D.ccnt, N + 1);
  rc |= salloc(s, g, &D.start, N + 1);
  rc |= salloc(s, g, &D.part, (N + 1 + SCAN_TILE - 1) / SCAN_TILE);
  rc |= salloc(s, g, &D.sd0, 2 * N);
  rc |= salloc(s, g, &D.sd2, N);
  rc |= salloc(s, g, &D.cnt, N);
  rc |= salloc(s, g, &D.bits, N);
  rc |= salloc(s, g, &D.acc, N * BD_ACC);
  rc |= salloc(s, g, &D.table, (size_t)2 * (BD_MAX_SIZE + 1) * BD_CELL_WORDS);
  rc |= salloc(s, g, &D.out, BD_OUT);
  if (rc != KMC_OK) {
    scratch_drop(s, s->bd);
    return fail(s, KMC_ERR_HIP, "bd: allocation failed (189 bytes per protein)");
  }
  rc = an_begin(s);
  if (rc == KMC_OK) rc = geo_run(s);
  if (rc != KMC_OK) {
    scratch_drop(s, s->bd);
    return rc;
  }
  if (N > 0) {
    const unsigned gr = (unsigned)((N + BD_T - 1) / BD_T);
    // (ccnt, the bodies' sums and bits, acc and out are zero: salloc)
    k_bd_begin<<<gr, BD_T, 0, s->stream>>>(s->K, s->d, D, s->geo.label, s->geo.off, s->geo.span, s->geo.cnt, BX, BY);
    bins_scan(s, D.ccnt, D.start, (int)N + 1, D.part);
    k_bd_scatter<<<gr, BD_T, 0, s->stream>>>((int)N, D);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  GeoOut o;
  if (rc == KMC_OK) rc = geo_result(s, &o);
  bd_u64 out[BD_OUT] = {0, 0, 0, 0};
  if (rc == KMC_OK && hipMemcpy(out, D.out, sizeof out, hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(s, KMC_ERR_HIP, "bd: the begin's counts could not be read");
  if (rc != KMC_OK) {
    scratch_drop(s, s->bd);
    return rc;
  }
  s->bd.cfg = c;
  s->bd.J = J;
  s->bd.F = F;
  s->bd.BX = BX;
  s->bd.BY = BY;
  s->bd.n_bodies = (int64_t)out[3];
  s->bd.rec = Recorder{true, s->step_done, s->step_done, 0};
  return KMC_OK;
}

int kmc_bd_update(kmc_sim* s, kmc_bd_info* info) {
  if (!s) return KMC_ERR_ARG;
  int rc = rec_check(s, s->bd.rec, BD_OFF);
  if (rc != KMC_OK) return rc;
  BdState& g = s->bd;
  if (s->step_done != g.rec.last + g.cfg.every)
    return fail(s, KMC_ERR_ARG, "bd: an update is due " + std::to_string(g.cfg.every) + " steps after the last one");
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N, nblk = (N + BD_T - 1) / BD_T;
  HIPCHK(s, hipMemsetAsync(g.dev.out, 0, sizeof(bd_u64) * 2, s->stream));
  if (nblk > 0)
    k_bd_update<<<(unsigned)std::min(nblk, AN_WG_MAX), BD_T, 0, s->stream>>>(s->K, s->d, g.dev, g.BX, g.BY, g.J, nblk);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) {
    g.rec.on = false;  // the per-protein state may be half advanced
    return rc;
  }
  g.rec.last = s->step_done;
  g.rec.updates += 1;
  if (info) {
    bd_u64 n[2] = {0, 0};
    HIPCHK(s, hipMemcpy(n, g.dev.out, sizeof n, hipMemcpyDeviceToHost));
    info->n_updates = g.rec.updates;
    info->n_jumped = (int64_t)n[0];
    info->n_changed = (int64_t)n[1];
  }
  return KMC_OK;
}

// the current components and the segmented reduction over the member list,
// left on the device for k_bd_finish or k_bd_rows; the stream is not waited
// for.  timed: an event after either part (kmc_bd_sample_ms).
static int bd_reduce(kmc_sim* s, bool timed) {
  const int rc = an_components(s);
  if (rc != KMC_OK) return rc;
  if (timed) {
    for (auto& e : s->bd_ev)
      if (!e) HIPCHK(s, hipEventCreate(&e));
    HIPCHK(s, hipEventRecord(s->bd_ev[0], s->stream));
  }
  const BdState& g = s->bd;
  const int N = s->K.N, nspans = (N + g.span - 1) / g.span, nwg = (nspans + BD_T / 64 - 1) / (BD_T / 64);
  if (nwg > 0)
    k_bd_reduce<<<(unsigned)std::min(nwg, AN_WG_MAX), BD_T, 0, s->stream>>>(g.dev, s->an.label, N, g.span, g.F, nspans);
  if (timed) HIPCHK(s, hipEventRecord(s->bd_ev[1], s->stream));
  return KMC_OK;
}

static int bd_ready(kmc_sim* s, const char* what) {
  const int rc = rec_check(s, s->bd.rec, BD_OFF);
  if (rc != KMC_OK) return rc;
  if (s->step_done != s->bd.rec.last)
    return fail(s, KMC_ERR_ARG, std::string(what) + ": the state has moved on since the last update (an update is due first)");
  return KMC_OK;
}

static int bd_components_ok(kmc_sim* s) {
  AnOut o;
  HIPCHK(s, hipMemcpy(&o, s->an.out, sizeof o, hipMemcpyDeviceToHost));
  if (o.err) return fail(s, KMC_ERR_STATE, "analysis: a bond link leaves the state or the link chains do not end");
  return KMC_OK;
}

int kmc_bd_sample(kmc_sim* s, kmc_bd_out* out, kmc_bd_cell* table) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "bd sample: out is needed");
  int rc = bd_ready(s, "bd sample");
  if (rc != KMC_OK) return rc;
  BdState& g = s->bd;
  const int N = s->K.N, ms = g.cfg.max_size;
  const size_t nword = (size_t)2 * (ms + 1) * BD_CELL_WORDS;
  if (table) {
    rc = an_begin(s);
    if (rc != KMC_OK) return rc;
    HIPCHK(s, hipMemsetAsync(g.dev.table, 0, sizeof(bd_u64) * nword, s->stream));
    if (N > 0) {
      rc = bd_reduce(s, true);
      if (rc != KMC_OK) return rc;
      const int nblk = (N + BD_T - 1) / BD_T;
      // (at most 2 x 256 cells of 128 bytes: the 64 KiB every launch may ask for)
      k_bd_finish<<<(unsigned)std::min(nblk, AN_WG_MAX), BD_T, sizeof(bd_u64) * nword, s->stream>>>(g.dev, s->an.cnt, N, ms,
                                                                                                   g.span);
    }
    HIPCHK(s, hipGetLastError());
    rc = an_end(s);
    if (rc == KMC_OK && N > 0) rc = bd_components_ok(s);
    if (rc != KMC_OK) {
      g.rec.on = false;  // the accumulators may be half served
      return rc;
    }
    float ms[3] = {0.0f, 0.0f, 0.0f};
    if (N > 0) {
      HIPCHK(s, hipEventElapsedTime(&ms[0], s->an_ev[0], s->bd_ev[0]));
      HIPCHK(s, hipEventElapsedTime(&ms[1], s->bd_ev[0], s->bd_ev[1]));
      HIPCHK(s, hipEventElapsedTime(&ms[2], s->bd_ev[1], s->an_ev[1]));
    }
    for (int k = 0; k < 3; ++k) s->bd_ms[k] = ms[k];
  }
  std::memset(out, 0, sizeof *out);
  out->cfg = g.cfg;
  out->J = g.J;
  out->F = g.F;
  out->BX = g.BX;
  out->BY = g.BY;
  out->origin_step = g.rec.origin;
  out->last_step = g.rec.last;
  out->n_updates = g.rec.updates;
  out->n_bodies = g.n_bodies;
  if (table) HIPCHK(s, hipMemcpy(table, g.dev.table, sizeof(bd_u64) * nword, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_bd_sample_ms(const kmc_sim* s, double ms[3]) {
  if (!s || !ms) return KMC_ERR_ARG;
  for (int k = 0; k < 3; ++k) ms[k] = s->bd_ms[k];
  return KMC_OK;
}

int kmc_bd_bodies(kmc_sim* s, int32_t min_size, int64_t cap, kmc_bd_body* rows, int64_t* n) {
  if (!s) return KMC_ERR_ARG;
  if (!n || min_size < 1 || cap < 0 || (cap > 0 && !rows))
    return fail(s, KMC_ERR_ARG, "bd bodies: n is needed, min_size >= 1, cap >= 0, rows for cap > 0");
  int rc = bd_ready(s, "bd bodies");
  if (rc != KMC_OK) return rc;
  BdState& g = s->bd;
  const int N = s->K.N;
  // no more than N / min_size bodies can qualify: a larger cap needs no larger buffer
  const size_t dcap = (size_t)std::min<int64_t>(cap, N / min_size);
  if (dcap > g.rows_cap) {
    HIPCHK(s, hipStreamSynchronize(s->stream));
    if (g.rows) {
      g.scratch.ptrs.erase(std::find(g.scratch.ptrs.begin(), g.scratch.ptrs.end(), (void*)g.rows));
      dfree(s, g.rows);
    }
    g.rows_cap = 0;
    if (salloc(s, g.scratch, &g.rows, dcap) != KMC_OK) return fail(s, KMC_ERR_HIP, "bd bodies: scratch allocation failed");
    g.rows_cap = dcap;
  }
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemsetAsync(g.dev.out + 2, 0, sizeof(bd_u64), s->stream));
  if (N > 0) {
    rc = bd_reduce(s, false);
    if (rc != KMC_OK) return rc;
    k_bd_rows<<<(unsigned)((N + BD_T - 1) / BD_T), BD_T, 0, s->stream>>>(g.dev, s->an.cnt, N, g.span, min_size,
                                                                         (long long)dcap, g.rows);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc == KMC_OK && N > 0) rc = bd_components_ok(s);
  if (rc != KMC_OK) {
    g.rec.on = false;
    return rc;
  }
  bd_u64 cnt = 0;
  HIPCHK(s, hipMemcpy(&cnt, g.dev.out + 2, sizeof cnt, hipMemcpyDeviceToHost));
  *n = (int64_t)cnt;
  if (*n > cap)
    return fail(s, KMC_ERR_CAPACITY, "bd bodies: " + std::to_string(*n) + " bodies qualify, cap is " + std::to_string(cap));
  if (*n) {
    HIPCHK(s, hipMemcpy(rows, g.rows, sizeof(kmc_bd_body) * (size_t)*n, hipMemcpyDeviceToHost));
    std::sort(rows, rows + *n, [](const kmc_bd_body& a, const kmc_bd_body& b) { return a.label < b.label; });
  }
  return KMC_OK;
}

int kmc_bd_arrays(kmc_sim* s, int64_t* U, int64_t* X0, uint8_t* flags, int32_t* label, int64_t* D0) {
  if (!s) return KMC_ERR_ARG;
  const int rc = rec_check(s, s->bd.rec, BD_OFF);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N;
  const Bd& D = s->bd.dev;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  if (U && N) HIPCHK(s, hipMemcpy(U, D.U, sizeof(longlong2) * N, hipMemcpyDeviceToHost));
  if (X0 && N) HIPCHK(s, hipMemcpy(X0, D.X0, sizeof(longlong2) * N, hipMemcpyDeviceToHost));
  if (flags && N) HIPCHK(s, hipMemcpy(flags, D.flags, N, hipMemcpyDeviceToHost));
  if (D0 && N) HIPCHK(s, hipMemcpy(D0, D.D0, sizeof(longlong2) * N, hipMemcpyDeviceToHost));
  if (label && N) {
    HIPCHK(s, hipMemcpy(label, D.label, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) label[i] += 1;
  }
  return KMC_OK;
}

int kmc_bd_get(kmc_sim* s, const kmc_bd_view* v) {
  if (!s) return KMC_ERR_ARG;
  if (!v || !v->prev || !v->U || !v->links || !v->flags)
    return fail(s, KMC_ERR_ARG, "bd get: the view with prev, U, links and flags is needed");
  int rc = kmc_bd_arrays(s, v->U, v->X0, v->flags, v->label, v->D0);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N;
  const Bd& D = s->bd.dev;
  if (N) HIPCHK(s, hipMemcpy(v->prev, D.prev, sizeof(longlong2) * N, hipMemcpyDeviceToHost));
  if (N) HIPCHK(s, hipMemcpy(v->links, D.links, sizeof(int32_t) * 3 * N, hipMemcpyDeviceToHost));
  if (v->bits && N) {
    std::vector<uint32_t> b(N);
    std::vector<int32_t> lab(N);
    HIPCHK(s, hipMemcpy(b.data(), D.bits, sizeof(uint32_t) * N, hipMemcpyDeviceToHost));
    HIPCHK(s, hipMemcpy(lab.data(), D.label, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) v->bits[i] = (uint8_t)b[(size_t)lab[i]];
  }
  return KMC_OK;
}

int kmc_bd_put(kmc_sim* s, const kmc_bd_view* v, int64_t last_step) {
  if (!s) return KMC_ERR_ARG;
  if (!v || !v->prev || !v->U || !v->links || !v->flags)
    return fail(s, KMC_ERR_ARG, "bd put: the view with prev, U, links and flags is needed");
  const int rc = rec_check(s, s->bd.rec, BD_OFF);
  if (rc != KMC_OK) return rc;
  if (last_step > s->step_done) return fail(s, KMC_ERR_ARG, "bd put: last_step lies after the current step");
  const size_t N = (size_t)s->K.N;
  for (size_t i = 0; i < N; ++i)
    if (v->flags[i] & ~(BD_JUMPED | BD_CHANGED))
      return fail(s, KMC_ERR_ARG, "bd put: the flags of protein " + std::to_string(i + 1) + " hold an unknown bit");
  const Bd& D = s->bd.dev;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  if (N) {
    HIPCHK(s, hipMemcpy(D.prev, v->prev, sizeof(longlong2) * N, hipMemcpyHostToDevice));
    HIPCHK(s, hipMemcpy(D.U, v->U, sizeof(longlong2) * N, hipMemcpyHostToDevice));
    HIPCHK(s, hipMemcpy(D.links, v->links, sizeof(int32_t) * 3 * N, hipMemcpyHostToDevice));
    HIPCHK(s, hipMemcpy(D.flags, v->flags, N, hipMemcpyHostToDevice));
  }
  s->bd.rec.last = last_step;
  return KMC_OK;
}

int kmc_bd_end(kmc_sim* s) {
  return s ? rec_end(s, s->bd) : KMC_ERR_ARG;
}

// ---------------------------------------------------------------- orientation
// kmc_orient.hip: the rotational recorder, on the lag correlator's schedule and
// with its life cycle (begin allocates the rings, end frees them), and the
// one-shot pose census, whose buffer stays with the handle.

static_assert(KMC_ROT_VECS == ROT_VECS && KMC_ROT_BAD == ROT_BAD && KMC_POSE_MAX_BINS == POSE_MAX_BINS &&
                  KMC_POSE_CLASSES == POSE_CLASSES,
              "kmc.h and kmc_orient.h agree");
static_assert(sizeof(kmc_rot_cell) == sizeof(lag_u64) * ROT_CELL, "a table cell is ROT_CELL words");
static_assert(offsetof(kmc_rot_cell, s1_all) == 16 && offsetof(kmc_rot_cell, s1_clean) == 32 &&
                  offsetof(kmc_rot_cell, s2_clean) == 48,
              "kmc_rot_cell is the layout rot_flush adds into");
static_assert(sizeof(kmc_pose_out) == sizeof(lag_u64) * (2 * POSE_CLASSES + 1), "kmc_pose_out is k_pose's nine counters");

static const char* const ROT_OFF = "rot: not begun (kmc_rot_begin; a new state drops the recorder)";

int kmc_rot_begin(kmc_sim* s, const kmc_rot_config* cfg) {
  if (!s) return KMC_ERR_ARG;
  if (!cfg) return fail(s, KMC_ERR_ARG, "rot: the configuration is needed");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  const kmc_rot_config c = *cfg;
  const char* bad = kmco::check(c.every, c.levels, c.slots);
  if (bad) return fail(s, KMC_ERR_ARG, bad);
  // a recorder that was on ends here, whatever becomes of this call
  rc = rec_end(s, s->rot);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N, W = (size_t)s->K.NA + 2 * (size_t)s->K.NB;
  const int L = c.levels, P = c.slots, rows = kmcl::rows(L, P);
  Scratch& g = s->rot.scratch;
  rc = KMC_OK;
  rc |= salloc(s, g, &s->rot.dev.vec, W);
  rc |= salloc(s, g, &s->rot.dev.links, 3 * N);
  rc |= salloc(s, g, &s->rot.dev.last_event, N);
  rc |= salloc(s, g, &s->rot.dev.chi, N);
  rc |= salloc(s, g, &s->rot.dev.cls, N);
  rc |= salloc(s, g, &s->rot.tasks, (size_t)LAG_MAX_ROWS);
  rc |= salloc(s, g, &s->rot.table, (size_t)rows * LAG_CLASSES * ROT_VECS * ROT_CELL);
  rc |= salloc(s, g, &s->rot.counts, 3);
  if (rc == KMC_OK) rc |= salloc(s, g, &s->rot.dev.ring, (size_t)L * P * W);
  if (rc != KMC_OK) {
    scratch_drop(s, s->rot);
    return fail(s, KMC_ERR_HIP, "rot: allocation failed (the rings take levels * slots * (8 n_a + 16 n_b) bytes)");
  }
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  if (N > 0) k_rot_begin<<<(unsigned)((N + ROT_T - 1) / ROT_T), ROT_T, 0, s->stream>>>(s->K, s->d, s->rot.dev, L, P);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  s->rot.cfg = c;
  s->rot.a.L = L;
  s->rot.a.P = P;
  s->rot.rec = Recorder{true, s->step_done, s->step_done, 0};
  return KMC_OK;
}

int kmc_rot_update(kmc_sim* s, kmc_rot_info* info) {
  if (!s) return KMC_ERR_ARG;
  int rc = rec_check(s, s->rot.rec, ROT_OFF);
  if (rc != KMC_OK) return rc;
  RotState& g = s->rot;
  if (s->step_done != g.rec.last + g.cfg.every)
    return fail(s, KMC_ERR_ARG, "rot: an update is due " + std::to_string(g.cfg.every) + " steps after the last one");
  if (g.rec.updates >= INT32_MAX) return fail(s, KMC_ERR_ARG, "rot: the update counter is full");
  const int64_t n = g.rec.updates + 1;
  kmcl::Task tasks[LAG_MAX_ROWS];
  const int nt = kmcl::tasks(n, g.a.L, g.a.P, tasks);
  g.a.n = (int)n;
  g.a.ntasks = nt;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  const int N = s->K.N;
  const int nblk = (N + ROT_T - 1) / ROT_T;
  HIPCHK(s, hipMemcpyAsync(g.tasks, tasks, sizeof(kmcl::Task) * (size_t)nt, hipMemcpyHostToDevice, s->stream));
  HIPCHK(s, hipMemsetAsync(g.counts, 0, sizeof(lag_u64) * 3, s->stream));
  if (nblk > 0) {
    const size_t lds = sizeof(lag_u64) * (size_t)(std::min(nt, ROT_CHUNK) * ROT_TASK_W);
    k_rot_update<<<(unsigned)std::min(nblk, AN_WG_MAX), ROT_T, lds, s->stream>>>(s->K, s->d, g.dev, g.a, g.tasks, nblk,
                                                                                g.table, g.counts);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);  // (waits: tasks is read by the copy until here)
  if (rc != KMC_OK) {
    g.rec.on = false;  // the per-protein state may be half advanced
    return rc;
  }
  for (int t = 0; t < nt; ++t) g.n_pairs[tasks[t].row] += 1;
  g.rec.last = s->step_done;
  g.rec.updates = n;
  if (info) {
    lag_u64 c[3] = {0, 0, 0};
    HIPCHK(s, hipMemcpy(c, g.counts, sizeof c, hipMemcpyDeviceToHost));
    info->n_updates = n;
    info->n_tasks = nt;
    info->n_events = (int64_t)c[0];
    info->n_flips = (int64_t)c[1];
    info->n_bad = (int64_t)c[2];
  }
  return KMC_OK;
}

int kmc_rot_sample(kmc_sim* s, kmc_rot_out* out, kmc_rot_cell* table, int64_t* n_pairs) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "rot sample: out is needed");
  int rc = rec_check(s, s->rot.rec, ROT_OFF);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc == KMC_OK) rc = an_end(s);  // (no device work: the time of this call is that of its copy's wait)
  if (rc != KMC_OK) return rc;
  const RotState& g = s->rot;
  const int rows = kmcl::rows(g.a.L, g.a.P);
  std::memset(out, 0, sizeof *out);
  out->cfg = g.cfg;
  out->origin_step = g.rec.origin;
  out->last_step = g.rec.last;
  out->n_updates = g.rec.updates;
  out->rows = rows;
  if (table)
    HIPCHK(s, hipMemcpy(table, g.table, sizeof(kmc_rot_cell) * (size_t)rows * LAG_CLASSES * ROT_VECS, hipMemcpyDeviceToHost));
  if (n_pairs) std::copy(g.n_pairs, g.n_pairs + rows, n_pairs);
  return KMC_OK;
}

int kmc_rot_arrays(kmc_sim* s, uint64_t* vec, int32_t* last_event, int8_t* chi) {
  if (!s) return KMC_ERR_ARG;
  const int rc = rec_check(s, s->rot.rec, ROT_OFF);
  if (rc != KMC_OK) return rc;
  const size_t N = (size_t)s->K.N, W = (size_t)s->K.NA + 2 * (size_t)s->K.NB;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  if (vec && W) HIPCHK(s, hipMemcpy(vec, s->rot.dev.vec, sizeof(lag_u64) * W, hipMemcpyDeviceToHost));
  if (last_event && N) HIPCHK(s, hipMemcpy(last_event, s->rot.dev.last_event, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  if (chi && N) HIPCHK(s, hipMemcpy(chi, s->rot.dev.chi, N, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_rot_end(kmc_sim* s) {
  return s ? rec_end(s, s->rot) : KMC_ERR_ARG;
}

int kmc_ligand_pose(kmc_sim* s, int32_t nz, int32_t nc, int64_t* hist, kmc_pose_out* out) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "pose: out is needed");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  int64_t BZ, Lq;
  const char* bad = kmco::pose_check(nz, nc, s->K.box_z, s->p.rb_radius, &BZ, &Lq);
  if (bad) return fail(s, KMC_ERR_ARG, bad);
  if (!s->pose.hist && dalloc(s, &s->pose.hist, (size_t)POSE_HIST_MAX + 2 * POSE_CLASSES + 1) != KMC_OK)
    return fail(s, KMC_ERR_HIP, "pose: scratch allocation failed");
  const size_t nbin = (size_t)POSE_CLASSES * nz * nc;
  lag_u64* counts = s->pose.hist + POSE_HIST_MAX;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemsetAsync(s->pose.hist, 0, sizeof(lag_u64) * nbin, s->stream));
  HIPCHK(s, hipMemsetAsync(counts, 0, sizeof(lag_u64) * (2 * POSE_CLASSES + 1), s->stream));
  const int NB = s->K.NB, nblk = (NB + ROT_T - 1) / ROT_T;
  if (nblk > 0)
    k_pose<<<(unsigned)std::min(nblk, POSE_WG_MAX), ROT_T, sizeof(uint32_t) * nbin, s->stream>>>(
        s->K, s->d, nz, nc, BZ, Lq, nblk, s->pose.hist, counts);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  static_assert(sizeof(lag_u64) == sizeof(int64_t), "the bins are copied out as they are");
  if (hist) HIPCHK(s, hipMemcpy(hist, s->pose.hist, sizeof(lag_u64) * nbin, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(out, counts, sizeof *out, hipMemcpyDeviceToHost));
  return KMC_OK;
}

// ---------------------------------------------------------------- encounters
// kmc_encounter.hip: a read-only census and a recorder on the kinetics
// recorder's life cycle (begin allocates its arrays, end frees them).  Both run
// the same walk: binning, phase A into the hit list (read back once: a list
// that was too short is grown and the walk replayed), the per-receptor scan,
// phase B.  The walk's scratch is the handle's, allocated at the first call.

static_assert(KMC_ENC_SLOTS == ENC_SLOTS && KMC_ENC_BINS == ENC_BINS && KMC_ENC_HISTS == ENC_HISTS &&
                  KMC_REACH_MAX_ND == ENC_MAX_ND && KMC_REACH_MAX_NA == ENC_MAX_NA &&
                  KMC_ENC_CENSORED == kmce::F_CENSORED && KMC_ENC_GEMINATE == kmce::F_GEMINATE &&
                  KMC_ENC_REACTIVE == kmce::F_REACTIVE && KMC_ENC_WAS_REACTIVE == kmce::F_WAS_REACTIVE,
              "kmc.h and kmc_encounter.h agree");

static const char* const ENC_OFF = "enc: not begun (kmc_enc_begin; a new state drops the recorder)";

// the walk's scratch: 48 bytes per receptor, 123 per ligand, 16 per cell of the search grid, 28 per hit
static int enc_reserve(kmc_sim* s) {
  EncWalk& E = s->ew;
  EncW& W = E.w;
  if (W.acc) return KMC_OK;
  const size_t NA = (size_t)s->K.NA, NS = 3 * (size_t)s->K.NB;
  // cell side: the larger cutoff (and a margin for the division's rounding), but about 8 proteins a cell at least
  const double cut = std::max(s->p.bond_dist_cutoff, s->p.cis_dist_cutoff) * (1.0 + 1.0 / 1024.0);
  EncGrid G;
  G.cs = std::max(cut, std::sqrt(8.0 * s->p.box_x * s->p.box_y / (double)std::max(1, s->K.N)));
  G.x0 = -s->p.box_x / 2;
  G.y0 = -s->p.box_y / 2;
  G.ncx = (int)std::max(1.0, std::min(32768.0, std::ceil(s->p.box_x / G.cs)));
  G.ncy = (int)std::max(1.0, std::min(32768.0, std::ceil(s->p.box_y / G.cs)));
  const size_t ncnt = (size_t)G.ncx * G.ncy + 1;
  // debug: the walk stages fewer points at a time
  E.chunk = (int)int_getenv("KMC_DEBUG_ENC_CHUNK", ENC_CHUNK, 1, ENC_CHUNK);
  // debug: a shorter first hit list (the growth and the replay at test size)
  const int64_t hits0 = std::max<int64_t>(1024, s->K.N);
  const unsigned int cap = (unsigned int)int_getenv("KMC_DEBUG_ENC_HITS", hits0, 1, hits0);
  for (auto& e : E.ev)
    if (!e) HIPCHK(s, hipEventCreate(&e));
  int rc = KMC_OK;
  rc |= dalloc(s, &W.probe, NA);
  rc |= dalloc(s, &W.point, NS);
  rc |= dalloc(s, &W.pcell, NA);
  rc |= dalloc(s, &W.prank, NA);
  rc |= dalloc(s, &W.tcell, NS);
  rc |= dalloc(s, &W.trank, NS);
  rc |= dalloc(s, &W.pcnt, ncnt);
  rc |= dalloc(s, &W.pstart, ncnt);
  rc |= dalloc(s, &W.tcnt, ncnt);
  rc |= dalloc(s, &W.tstart, ncnt);
  rc |= dalloc(s, &W.part, (ncnt + SCAN_TILE - 1) / SCAN_TILE);
  rc |= dalloc(s, &W.rcnt, NA + 1);
  rc |= dalloc(s, &W.rstart, NA + 1);
  rc |= dalloc(s, &W.rpart, (NA + 1 + SCAN_TILE - 1) / SCAN_TILE);
  rc |= dalloc(s, &W.hits, (size_t)cap);
  rc |= dalloc(s, &W.rhit, (size_t)cap);
  rc |= dalloc(s, &W.site_flag, NS);
  rc |= dalloc(s, &W.E2, (size_t)ENC_CHANNELS * ENC_MAX_ND);
  rc |= dalloc(s, &W.tab, (size_t)ENC_TAB_WORDS);
  if (rc == KMC_OK) rc = dalloc(s, &W.acc, 1);  // (the last: set when all the others are)
  if (rc != KMC_OK) {
    dfree(s, W.probe), dfree(s, W.point), dfree(s, W.pcell), dfree(s, W.prank), dfree(s, W.tcell), dfree(s, W.trank);
    dfree(s, W.pcnt), dfree(s, W.pstart), dfree(s, W.tcnt), dfree(s, W.tstart), dfree(s, W.part), dfree(s, W.rcnt);
    dfree(s, W.rstart), dfree(s, W.rpart), dfree(s, W.hits), dfree(s, W.rhit), dfree(s, W.site_flag), dfree(s, W.E2);
    dfree(s, W.tab);
    return fail(s, KMC_ERR_HIP, "enc: scratch allocation failed");
  }
  W.hit_cap = cap;
  W.G = G;
  return KMC_OK;
}

// one walk (walk 0 or 1 of the call: its two events) on the handle's stream; the stream is waited for once,
// after phase A
static int enc_walk(kmc_sim* s, bool cis, int walk, int nd, int na, int hist) {
  EncWalk& E = s->ew;
  EncW& W = E.w;
  hipStream_t st = s->stream;
  const int NA = s->K.NA, NS = 3 * s->K.NB, ncell = W.G.ncx * W.G.ncy;
  const int nthr = std::max(NA, cis ? 0 : NS);
  unsigned int nhits = 0;
  HIPCHK(s, hipMemsetAsync(W.pcnt, 0, sizeof(int32_t) * (size_t)(ncell + 1), st));
  if (!cis) {
    HIPCHK(s, hipMemsetAsync(W.tcnt, 0, sizeof(int32_t) * (size_t)(ncell + 1), st));
    HIPCHK(s, hipMemsetAsync(W.site_flag, 0, (size_t)std::max(NS, 1), st));
  }
  HIPCHK(s, hipMemsetAsync(W.rcnt, 0, sizeof(int32_t) * (size_t)(NA + 1), st));
  HIPCHK(s, hipMemsetAsync(&W.acc->nhits, 0, sizeof(unsigned int), st));
  if (NA > 0) {
    const unsigned gr = (unsigned)((nthr + ENC_T - 1) / ENC_T);
    const unsigned gw = (unsigned)std::min((ncell + ENC_WAVES - 1) / ENC_WAVES, AN_WG_MAX);
    const size_t lds = sizeof(EncPt) * 2 * ENC_WAVES * (size_t)E.chunk;
    const double T2 = cis ? s->K.T_cis : s->K.T_bond;
    if (cis) k_enc_count<true><<<gr, ENC_T, 0, st>>>(s->K, s->d, W);
    else k_enc_count<false><<<gr, ENC_T, 0, st>>>(s->K, s->d, W);
    bins_scan(s, W.pcnt, W.pstart, ncell + 1, W.part);
    if (!cis) bins_scan(s, W.tcnt, W.tstart, ncell + 1, W.part);
    if (cis) k_enc_scatter<true><<<gr, ENC_T, 0, st>>>(s->K, s->d, W);
    else k_enc_scatter<false><<<gr, ENC_T, 0, st>>>(s->K, s->d, W);
    for (int attempt = 0;; ++attempt) {
      if (cis) k_enc_walk<true><<<gw, ENC_T, lds, st>>>(W, T2, E.chunk);
      else k_enc_walk<false><<<gw, ENC_T, lds, st>>>(W, T2, E.chunk);
      HIPCHK(s, hipGetLastError());
      HIPCHK(s, hipMemcpyAsync(&nhits, &W.acc->nhits, sizeof nhits, hipMemcpyDeviceToHost, st));
      HIPCHK(s, hipStreamSynchronize(st));
      if (nhits <= W.hit_cap) break;
      if (attempt > 0) return fail(s, KMC_ERR_CAPACITY, "enc: the hit list overflowed after it was grown");
      // the list was too short: grown to what the walk counted, and the walk replayed
      dfree(s, W.hits);
      dfree(s, W.rhit);
      W.hit_cap = 0;
      int rc = dalloc(s, &W.hits, (size_t)nhits);
      if (rc == KMC_OK) rc = dalloc(s, &W.rhit, (size_t)nhits);
      if (rc != KMC_OK) return fail(s, KMC_ERR_HIP, "enc: the hit list could not be grown");
      W.hit_cap = nhits;
      HIPCHK(s, hipMemsetAsync(W.rcnt, 0, sizeof(int32_t) * (size_t)(NA + 1), st));
      HIPCHK(s, hipMemsetAsync(&W.acc->nhits, 0, sizeof(unsigned int), st));
    }
  }
  HIPCHK(s, hipEventRecord(E.ev[2 * walk], st));
  if (NA > 0) {
    if (!cis) bins_scan(s, W.rcnt, W.rstart, NA + 1, W.rpart);
    const unsigned gb = (unsigned)std::min<size_t>(std::max<size_t>(((size_t)nhits + ENC_T - 1) / ENC_T, 1), AN_WG_MAX);
    if (cis) k_enc_gates<true><<<gb, ENC_T, 0, st>>>(s->K, s->d, W, nd, na, hist);
    else k_enc_gates<false><<<gb, ENC_T, 0, st>>>(s->K, s->d, W, nd, na, hist);
  }
  HIPCHK(s, hipEventRecord(E.ev[2 * walk + 1], st));
  HIPCHK(s, hipGetLastError());
  return KMC_OK;
}

// the phases' times of a call of `walks` walks, after an_end
static int enc_times(kmc_sim* s, int walks) {
  EncWalk& E = s->ew;
  float a = 0, b = 0, c = 0, t = 0;
  HIPCHK(s, hipEventElapsedTime(&a, s->an_ev[0], E.ev[0]));
  HIPCHK(s, hipEventElapsedTime(&b, E.ev[0], E.ev[1]));
  if (walks == 2) {
    HIPCHK(s, hipEventElapsedTime(&t, E.ev[1], E.ev[2]));
    a += t;
    HIPCHK(s, hipEventElapsedTime(&t, E.ev[2], E.ev[3]));
    b += t;
  }
  HIPCHK(s, hipEventElapsedTime(&c, E.ev[2 * walks - 1], s->an_ev[1]));
  E.ms[0] = a;
  E.ms[1] = b;
  E.ms[2] = c;
  return KMC_OK;
}

int kmc_enc_phase_ms(const kmc_sim* s, double ms[3]) {
  if (!s || !ms) return KMC_ERR_ARG;
  for (int k = 0; k < 3; ++k) ms[k] = s->ew.ms[k];
  return KMC_OK;
}

int kmc_reach_census(kmc_sim* s, int32_t nd, int32_t na, kmc_reach_out* out, int64_t* hist_d, int64_t* hist_a_rl,
                     int64_t* hist_a_cis) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "reach census: out is needed");
  if (nd < 1 || nd > ENC_MAX_ND || na < 1 || na > ENC_MAX_NA)
    return fail(s, KMC_ERR_ARG, "reach census: 1 <= nd <= 64 and 1 <= na <= 36");
  int rc = an_check(s);
  if (rc == KMC_OK) rc = enc_reserve(s);
  if (rc != KMC_OK) return rc;
  EncW& W = s->ew.w;
  double E2[ENC_CHANNELS * ENC_MAX_ND] = {0.0};
  kmce::edges(s->p.bond_dist_cutoff, nd, E2 + kmce::CH_RL * ENC_MAX_ND);
  kmce::edges(s->p.cis_dist_cutoff, nd, E2 + kmce::CH_MONO * ENC_MAX_ND);
  kmce::edges(s->p.cis_dist_cutoff, nd, E2 + kmce::CH_CX * ENC_MAX_ND);
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  hipStream_t st = s->stream;
  HIPCHK(s, hipMemcpyAsync(W.E2, E2, sizeof E2, hipMemcpyHostToDevice, st));  // (waited for in the first walk)
  HIPCHK(s, hipMemsetAsync(W.acc, 0, sizeof(EncAcc), st));
  HIPCHK(s, hipMemsetAsync(W.tab, 0, sizeof(enc_u64) * ENC_TAB_WORDS, st));
  rc = enc_walk(s, false, 0, nd, na, 1);
  if (rc != KMC_OK) return rc;
  const int nthr = std::max(s->K.NA, 3 * s->K.NB);
  if (s->K.NA > 0) k_enc_census_fin<<<(unsigned)((nthr + ENC_T - 1) / ENC_T), ENC_T, 0, st>>>(s->K, W);
  rc = enc_walk(s, true, 1, nd, na, 1);
  if (rc == KMC_OK) rc = an_end(s);
  if (rc == KMC_OK) rc = enc_times(s, 2);
  if (rc != KMC_OK) return rc;
  EncAcc a;
  std::vector<enc_u64> tab(ENC_TAB_WORDS);
  HIPCHK(s, hipMemcpy(&a, W.acc, sizeof a, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(tab.data(), W.tab, sizeof(enc_u64) * ENC_TAB_WORDS, hipMemcpyDeviceToHost));
  if (a.err) return fail(s, KMC_ERR_STATE, "reach census: a slot leaves its range");
  std::memset(out, 0, sizeof *out);
  for (int c = 0; c < ENC_CHANNELS; ++c) {
    out->n_reach[c] = (int64_t)tab[ENC_TAB_N + c];
    out->n_reactive[c] = (int64_t)tab[ENC_TAB_N + 3 + c];
  }
  out->rl_free_receptors = (int64_t)tab[ENC_TAB_RL + 0];
  out->rl_free_sites = (int64_t)tab[ENC_TAB_RL + 1];
  out->rl_receptors_in_reach = (int64_t)tab[ENC_TAB_RL + 2];
  out->rl_sites_in_reach = (int64_t)tab[ENC_TAB_RL + 3];
  out->rl_max_partners = (int64_t)a.max_partners;
  auto put = [](int64_t* to, const enc_u64* from, size_t n) {
    if (to)
      for (size_t k = 0; k < n; ++k) to[k] = (int64_t)from[k];
  };
  put(hist_d, tab.data() + ENC_TAB_D, (size_t)ENC_CHANNELS * 2 * nd);
  put(hist_a_rl, tab.data() + ENC_TAB_ARL, (size_t)na * na);
  put(hist_a_cis, tab.data() + ENC_TAB_ACIS, (size_t)2 * na);
  return KMC_OK;
}

static void enc_fill(const kmc_sim* s, int64_t alive, kmc_enc_out* out) {
  const EncState& g = s->enc;
  std::memset(out, 0, sizeof *out);
  out->origin_step = g.rec.origin;
  out->last_step = g.rec.last;
  out->n_updates = g.rec.updates;
  out->on_from_encounter = g.ev[kmce::C_FROM_ENCOUNTER];
  out->on_direct = g.ev[kmce::C_DIRECT];
  out->n_opened = g.ev[kmce::C_OPENED];
  out->n_ended = g.ev[kmce::C_ENDED];
  out->n_overflow = g.ev[kmce::C_OVERFLOW];
  out->exp_reach = g.exp[0];
  out->exp_reactive = g.exp[1];
  out->exp_free_receptor = g.exp[2];
  out->occ_reach = g.occ[0];
  out->occ_reactive = g.occ[1];
  out->occ_free_receptor = g.occ[2];
  out->n_censored_alive = alive;
  out->every = g.every;
  out->slots = g.slots;
}

// the device work of a begin (t: its step) or an update: the R–L walk, then the slot kernel; the counters come back
static int enc_look(kmc_sim* s, bool begin, EncAcc* a) {
  EncState& g = s->enc;
  EncW& W = s->ew.w;
  hipStream_t st = s->stream;
  int rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemsetAsync(W.acc, 0, sizeof(EncAcc), st));
  rc = enc_walk(s, false, 0, 0, 0, 0);
  if (rc != KMC_OK) return rc;
  const int NA = s->K.NA;
  if (NA > 0) {
    const unsigned gr = (unsigned)((NA + ENC_T - 1) / ENC_T);
    if (begin) k_enc_slots<true><<<gr, ENC_T, 0, st>>>(s->K, s->d, W, g.dev, g.slots, (long long)s->step_done, g.hist);
    else k_enc_slots<false><<<gr, ENC_T, 0, st>>>(s->K, s->d, W, g.dev, g.slots, (long long)s->step_done, g.hist);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc == KMC_OK) rc = enc_times(s, 1);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpy(a, W.acc, sizeof *a, hipMemcpyDeviceToHost));
  if (a->err) return fail(s, KMC_ERR_STATE, "enc: a slot or a receptor's bond link leaves its range");
  return KMC_OK;
}

int kmc_enc_begin(kmc_sim* s, const kmc_enc_config* cfg) {
  if (!s) return KMC_ERR_ARG;
  if (!cfg) return fail(s, KMC_ERR_ARG, "enc: the configuration is needed");
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  if (cfg->every < 1) return fail(s, KMC_ERR_ARG, "enc: every >= 1");
  // a recorder that was on ends here, whatever becomes of this call
  rc = rec_end(s, s->enc);
  if (rc == KMC_OK) rc = enc_reserve(s);
  if (rc != KMC_OK) return rc;
  EncState& g = s->enc;
  const size_t NA = (size_t)s->K.NA;
  rc = KMC_OK;
  rc |= salloc(s, g.scratch, &g.dev.lig, NA);
  rc |= salloc(s, g.scratch, &g.dev.site, NA);
  rc |= salloc(s, g.scratch, &g.dev.key, NA);
  rc |= salloc(s, g.scratch, &g.dev.since, NA);
  rc |= salloc(s, g.scratch, &g.dev.nreact, NA);
  rc |= salloc(s, g.scratch, &g.dev.flags, NA);
  rc |= salloc(s, g.scratch, &g.hist, (size_t)(ENC_ACC_ROWS + 1) * ENC_BINS);  // (zero: salloc)
  if (rc != KMC_OK) {
    scratch_drop(s, s->enc);
    return fail(s, KMC_ERR_HIP, "enc: allocation failed (76 bytes per receptor)");
  }
  g.every = cfg->every;
  // debug: fewer slots are kept per receptor
  g.slots = (int)int_getenv("KMC_DEBUG_ENC_SLOTS", ENC_SLOTS, 1, ENC_SLOTS);
  EncAcc a;
  rc = enc_look(s, true, &a);
  if (rc != KMC_OK) {
    scratch_drop(s, s->enc);
    return rc;
  }
  g.ev[kmce::C_OVERFLOW] = (int64_t)a.cnt[kmce::C_OVERFLOW];
  for (int k = 0; k < 3; ++k) g.occ[k] = (int64_t)a.cnt[kmce::C_OCC_REACH + k];
  g.rec = Recorder{true, s->step_done, s->step_done, 0};
  return KMC_OK;
}

int kmc_enc_update(kmc_sim* s, kmc_enc_out* out) {
  if (!s) return KMC_ERR_ARG;
  int rc = rec_check(s, s->enc.rec, ENC_OFF);
  if (rc != KMC_OK) return rc;
  EncState& g = s->enc;
  if (s->step_done == g.rec.last) {  // a second update at the same step moves only the count
    g.rec.updates += 1;
    if (out) enc_fill(s, 0, out);
    return KMC_OK;
  }
  if (s->step_done != g.rec.last + g.every)
    return fail(s, KMC_ERR_ARG, "enc: an update is due " + std::to_string(g.every) + " steps after the last one");
  EncAcc a;
  rc = enc_look(s, false, &a);
  if (rc != KMC_OK) {
    g.rec.on = false;  // the slots may be half advanced
    return rc;
  }
  const int64_t dt = s->step_done - g.rec.last;
  for (int k = 0; k < 3; ++k) {
    g.exp[k] += dt * g.occ[k];
    g.occ[k] = (int64_t)a.cnt[kmce::C_OCC_REACH + k];
  }
  for (int k = 0; k < ENC_NEV; ++k) g.ev[k] += (int64_t)a.cnt[k];
  g.rec.last = s->step_done;
  g.rec.updates += 1;
  if (out) enc_fill(s, 0, out);
  return KMC_OK;
}

int kmc_enc_sample(kmc_sim* s, kmc_enc_out* out, int64_t* hist, int64_t* react_hist) {
  if (!s) return KMC_ERR_ARG;
  if (!out) return fail(s, KMC_ERR_ARG, "enc sample: out is needed");
  int rc = rec_check(s, s->enc.rec, ENC_OFF);
  if (rc == KMC_OK) rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  EncState& g = s->enc;
  EncW& W = s->ew.w;
  enc_u64* row = g.hist + (size_t)ENC_ACC_ROWS * ENC_BINS;
  HIPCHK(s, hipMemsetAsync(row, 0, sizeof(enc_u64) * ENC_BINS, s->stream));
  HIPCHK(s, hipMemsetAsync(&W.acc->alive, 0, sizeof(enc_u64), s->stream));
  const int NA = s->K.NA, nblk = (NA + ENC_T - 1) / ENC_T;
  if (nblk > 0)
    k_enc_sample<<<(unsigned)std::min(nblk, AN_WG_MAX), ENC_T, 0, s->stream>>>(NA, g.dev, (long long)g.rec.last, nblk,
                                                                             row, W.acc);
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);
  if (rc != KMC_OK) return rc;
  enc_u64 alive = 0;
  HIPCHK(s, hipMemcpy(&alive, &W.acc->alive, sizeof alive, hipMemcpyDeviceToHost));
  enc_fill(s, (int64_t)alive, out);
  static_assert(sizeof(enc_u64) == sizeof(int64_t), "the bins are copied out as they are");
  if (hist) {
    HIPCHK(s, hipMemcpy(hist, g.hist, sizeof(enc_u64) * ENC_ROWS_UPD * ENC_BINS, hipMemcpyDeviceToHost));
    HIPCHK(s, hipMemcpy(hist + (size_t)ENC_ROWS_UPD * ENC_BINS, row, sizeof(enc_u64) * ENC_BINS, hipMemcpyDeviceToHost));
  }
  if (react_hist)
    HIPCHK(s, hipMemcpy(react_hist, g.hist + (size_t)ENC_ROWS_UPD * ENC_BINS, sizeof(enc_u64) * ENC_REACT * ENC_BINS,
                        hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_enc_arrays(kmc_sim* s, const kmc_enc_view* v) {
  if (!s) return KMC_ERR_ARG;
  if (!v) return fail(s, KMC_ERR_ARG, "enc arrays: the view is needed (each of its arrays may be NULL)");
  const int rc = rec_check(s, s->enc.rec, ENC_OFF);
  if (rc != KMC_OK) return rc;
  const size_t NA = (size_t)s->K.NA;
  const Enc& D = s->enc.dev;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  if (NA == 0) return KMC_OK;
  if (v->lig) HIPCHK(s, hipMemcpy(v->lig, D.lig, sizeof(int32_t) * NA, hipMemcpyDeviceToHost));
  if (v->site) HIPCHK(s, hipMemcpy(v->site, D.site, sizeof(int32_t) * NA, hipMemcpyDeviceToHost));
  if (v->key) HIPCHK(s, hipMemcpy(v->key, D.key, sizeof(int4) * NA, hipMemcpyDeviceToHost));
  if (v->since) HIPCHK(s, hipMemcpy(v->since, D.since, sizeof(longlong4) * NA, hipMemcpyDeviceToHost));
  if (v->nreact) HIPCHK(s, hipMemcpy(v->nreact, D.nreact, sizeof(int4) * NA, hipMemcpyDeviceToHost));
  if (v->flags) HIPCHK(s, hipMemcpy(v->flags, D.flags, sizeof(uchar4) * NA, hipMemcpyDeviceToHost));
  return KMC_OK;
}

int kmc_enc_end(kmc_sim* s) {
  return s ? rec_end(s, s->enc) : KMC_ERR_ARG;
}

// ---------------------------------------------------------------- proximity clusters
// kmc_proximity.hip: read-only like the bond order above, on scratch of its own.
// A fixed sequence of launches whatever the clusters look like: init, the bond
// components, the binning, the count walk, the union walk, the flatten, the
// border walk, the two reduces; the stream is waited for once, at the end.

static_assert(KMC_PX_NN_ROWS == PX_NN_ROWS && KMC_PX_MAX_SIZE == PX_MAX_SIZE && KMC_PX_NND_BINS == PX_NND_BINS,
              "kmc.h and kmc_proximity.h agree");
static_assert(sizeof(kmc_prox_out) == 13 * sizeof(int64_t) + 2 * sizeof(int32_t), "kmc_prox_out layout");

// the scratch of the first call: 91 bytes per protein, 12 per cell of the grid in use, 0.5 MiB of bins
static int px_reserve(kmc_sim* s) {
  PxState& X = s->px;
  if (X.out) return KMC_OK;
  const size_t N = (size_t)s->K.N;
  // debug: the union walk flushes its queue at fewer pairs
  X.q = (int)int_getenv("KMC_DEBUG_PX_QUEUE", 64, 1, 64);
  for (auto& e : X.ev)
    if (!e) HIPCHK(s, hipEventCreate(&e));
  int rc = KMC_OK;
  rc |= dalloc(s, &X.cell, N);
  rc |= dalloc(s, &X.rank, N);
  rc |= dalloc(s, &X.pts, N);
  rc |= dalloc(s, &X.ref, N);
  rc |= dalloc(s, &X.clist, N);
  rc |= dalloc(s, &X.blist, N);
  rc |= dalloc(s, &X.core_s, N);
  rc |= dalloc(s, &X.kind, N);
  rc |= dalloc(s, &X.mask, N);
  rc |= dalloc(s, &X.nn, N);
  rc |= dalloc(s, &X.parent, N);
  rc |= dalloc(s, &X.label, N);
  rc |= dalloc(s, &X.cnt, N);
  rc |= dalloc(s, &X.M, N);
  rc |= dalloc(s, &X.cparent, N);
  rc |= dalloc(s, &X.clab, N);
  rc |= dalloc(s, &X.cmin, N);
  rc |= dalloc(s, &X.cmax, N);
  rc |= dalloc(s, &X.pmin, N);
  rc |= dalloc(s, &X.pmax, N);
  rc |= dalloc(s, &X.bsel, N);
  rc |= dalloc(s, &X.size_hist, (size_t)PX_MAX_SIZE + 1);
  rc |= dalloc(s, &X.nn_hist, (size_t)PX_NN_ROWS);
  rc |= dalloc(s, &X.nnd_hist, (size_t)PX_NND_BINS);
  rc |= dalloc(s, &X.E2, (size_t)PX_NND_BINS);
  rc |= dalloc(s, &X.an_out, 1);
  if (rc == KMC_OK) rc = dalloc(s, &X.out, 1);  // (the last: set when all the others are)
  if (rc != KMC_OK) {
    dfree(s, X.cell), dfree(s, X.rank), dfree(s, X.pts), dfree(s, X.ref), dfree(s, X.clist), dfree(s, X.blist);
    dfree(s, X.core_s), dfree(s, X.kind), dfree(s, X.mask), dfree(s, X.nn), dfree(s, X.parent), dfree(s, X.label);
    dfree(s, X.cnt), dfree(s, X.M), dfree(s, X.cparent), dfree(s, X.clab), dfree(s, X.cmin), dfree(s, X.cmax);
    dfree(s, X.pmin), dfree(s, X.pmax), dfree(s, X.bsel), dfree(s, X.size_hist), dfree(s, X.nn_hist);
    dfree(s, X.nnd_hist), dfree(s, X.E2), dfree(s, X.an_out);
    return fail(s, KMC_ERR_HIP, "prox: scratch allocation failed");
  }
  return KMC_OK;
}

int kmc_prox_phase_ms(const kmc_sim* s, double ms[4]) {
  if (!s || !ms) return KMC_ERR_ARG;
  for (int k = 0; k < 4; ++k) ms[k] = s->px.ms[k];
  return KMC_OK;
}

int kmc_prox_clusters(kmc_sim* s, int32_t which, int32_t select, const uint8_t* mask, double eps, int32_t min_pts,
                      int32_t max_size, int32_t nbins, kmc_prox_out* out, int64_t* size_hist, int64_t* nn_hist,
                      int64_t* nnd_hist, int32_t* label, int32_t* nn, uint8_t* kind) {
  if (!s) return KMC_ERR_ARG;
  if (!out || which < KMC_PX_A || which > KMC_PX_AB || (select != KMC_SK_ALL && select != KMC_SK_BOUND) ||
      min_pts < 1 || min_pts > PX_MIN_PTS_MAX || max_size < 1 || max_size > PX_MAX_SIZE || nbins < 1 ||
      nbins > PX_NND_BINS)
    return fail(s, KMC_ERR_ARG, "prox: out is needed, which 0..2, select 0 or 1, 1 <= min_pts <= 2^30, 1 <= max_size <= " +
                                    std::to_string(PX_MAX_SIZE) + ", 1 <= nbins <= " + std::to_string(PX_NND_BINS));
  int rc = an_check(s);
  if (rc != KMC_OK) return rc;
  const KParams& K = s->K;
  const double bx = kmcm::round_(K.box_x * 1024.0), by = kmcm::round_(K.box_y * 1024.0);
  if (!(bx >= 1.0) || !(by >= 1.0) || !(bx < (double)BO_BOX_MAX) || !(by < (double)BO_BOX_MAX))
    return fail(s, KMC_ERR_ARG, "prox: the box is below 2^-10 A or not below 2^21 A");
  BoArgs a;
  a.which = which;
  a.mode = a.fold = 0;
  a.select = select;
  a.base = which == KMC_PX_B ? K.NA : 0;
  a.n = which == KMC_PX_A ? K.NA : which == KMC_PX_B ? K.NB : K.N;
  a.BX = (long long)bx;
  a.BY = (long long)by;
  const long long EPS = eps > 0.0 && eps * 1024.0 < (double)BO_BOX_MAX ? (long long)kmcm::round_(eps * 1024.0) : 0;
  if (EPS < 1 || a.BX / EPS < 3 || a.BY / EPS < 3)
    return fail(s, KMC_ERR_ARG, "prox: eps must be at least 2^-10 A and at most a third of the box (3 cells along an axis)");
  a.RC2 = EPS * EPS;
  a.ncx = (int)std::min<long long>(a.BX / EPS, BO_NC_MAX);
  a.ncy = (int)std::min<long long>(a.BY / EPS, BO_NC_MAX);
  rc = px_reserve(s);
  if (rc != KMC_OK) return rc;
  PxState& X = s->px;
  const size_t ncnt = (size_t)a.ncx * a.ncy + 1;  // the scan's last entry is the number of binned points
  rc = bins_reserve(s, X.bins, ncnt, "prox");
  if (rc != KMC_OK) return rc;
  const int N = K.N;
  const double dr = eps / nbins;
  PxArgs x;
  x.min_pts = min_pts;
  x.max_size = max_size;
  x.nbins = nbins;
  x.N = N;
  x.inv_dr = (float)(1.0 / (dr * 1024.0));
  std::vector<int64_t> E2((size_t)nbins);
  for (int m = 0; m < nbins; ++m) {
    const int64_t e = kmcb::corr_edge(m, dr);
    E2[m] = e * e;
  }
  hipStream_t st = s->stream;
  rc = an_begin(s);
  if (rc != KMC_OK) return rc;
  HIPCHK(s, hipMemcpyAsync(X.E2, E2.data(), sizeof(int64_t) * E2.size(), hipMemcpyHostToDevice, st));
  if (mask && N) HIPCHK(s, hipMemcpyAsync(X.mask, mask, (size_t)N, hipMemcpyHostToDevice, st));
  HIPCHK(s, hipMemsetAsync(X.out, 0, sizeof(PxOut), st));
  HIPCHK(s, hipMemsetAsync(X.an_out, 0, sizeof(AnOut), st));
  HIPCHK(s, hipMemsetAsync(X.size_hist, 0, sizeof(unsigned long long) * ((size_t)max_size + 1), st));
  HIPCHK(s, hipMemsetAsync(X.nn_hist, 0, sizeof(unsigned long long) * PX_NN_ROWS, st));
  HIPCHK(s, hipMemsetAsync(X.nnd_hist, 0, sizeof(unsigned long long) * (size_t)nbins, st));
  HIPCHK(s, hipMemsetAsync(X.bins.ccnt, 0, sizeof(int32_t) * ncnt, st));
  const unsigned gN = (unsigned)((N + PX_T - 1) / PX_T), gn = (unsigned)((a.n + PX_T - 1) / PX_T);
  const unsigned gw = (unsigned)std::min<int64_t>(4 * PX_WG_MAX, ((int64_t)a.n + PX_T - 1) / PX_T);
  const unsigned gr = (unsigned)std::min<int64_t>(PX_WG_MAX, ((int64_t)N + PX_T - 1) / PX_T);
  // bin
  if (gN) k_px_init<<<gN, PX_T, 0, st>>>(N, X.parent, X.cparent, X.nn, X.kind, X.label, X.cnt, X.cmin, X.cmax, X.pmin,
                                         X.pmax, X.bsel);
  if (gn) k_px_cell_count<<<gn, PX_T, 0, st>>>(s->K, s->d, a, mask ? X.mask : nullptr, X.bins.ccnt, X.cell, X.rank, X.out);
  bins_scan(s, X.bins.ccnt, X.bins.cstart, (int)ncnt, X.bins.part);
  if (gn) k_px_cell_scatter<<<gn, PX_T, 0, st>>>(s->K, s->d, a, X.bins.cstart, X.cell, X.rank, X.pts, X.ref);
  HIPCHK(s, hipEventRecord(X.ev[0], st));
  // count walk
  if (gn)
    k_px_count<<<gw, PX_T, 0, st>>>(a, x, X.bins.cstart, X.pts, X.ref, X.nn, X.M, X.kind, X.core_s, X.clist, X.blist,
                                    X.out);
  HIPCHK(s, hipEventRecord(X.ev[1], st));
  // union + flatten
  if (gn) {
    k_px_union<<<gw, PX_T, 0, st>>>(a, x, X.q, X.bins.cstart, X.pts, X.ref, X.core_s, X.clist, X.parent, X.out);
    k_px_flatten<<<gN, PX_T, 0, st>>>(N, X.kind, X.parent, X.label, X.out);
  }
  HIPCHK(s, hipEventRecord(X.ev[2], st));
  // border + reduce (the bond components feed the reduce alone)
  if (gN) {
    k_an_hook<<<gN, AN_T, 0, st>>>(s->K, s->d, X.cparent, X.an_out);
    k_an_flatten<<<gN, AN_T, 0, st>>>(X.cparent, X.clab, N, X.an_out);
  }
  if (gn) {
    k_px_border<<<gw, PX_T, 0, st>>>(a, X.bins.cstart, X.pts, X.ref, X.core_s, X.blist, X.kind, X.label, X.out);
    const size_t lds = sizeof(unsigned long long) * (size_t)(PX_NSUM + PX_NN_ROWS + nbins);
    k_px_points<<<gr, PX_T, lds, st>>>(x, X.kind, X.nn, X.M, X.label, X.clab, X.E2, X.cnt, X.cmin, X.cmax, X.pmin, X.pmax,
                                       X.bsel, X.nn_hist, X.nnd_hist, X.out);
    k_px_roots<<<gr, PX_T, 0, st>>>(x, X.kind, X.label, X.cnt, X.cmin, X.cmax, X.pmin, X.pmax, X.bsel, X.size_hist, X.out);
  }
  HIPCHK(s, hipGetLastError());
  rc = an_end(s);  // (waits: E2 and the mask are read by the copies until here)
  if (rc != KMC_OK) return rc;
  float t[4] = {0, 0, 0, 0};
  HIPCHK(s, hipEventElapsedTime(&t[0], s->an_ev[0], X.ev[0]));
  HIPCHK(s, hipEventElapsedTime(&t[1], X.ev[0], X.ev[1]));
  HIPCHK(s, hipEventElapsedTime(&t[2], X.ev[1], X.ev[2]));
  HIPCHK(s, hipEventElapsedTime(&t[3], X.ev[2], s->an_ev[1]));
  for (int k = 0; k < 4; ++k) X.ms[k] = t[k];
  PxOut o;
  AnOut ao;
  HIPCHK(s, hipMemcpy(&o, X.out, sizeof o, hipMemcpyDeviceToHost));
  HIPCHK(s, hipMemcpy(&ao, X.an_out, sizeof ao, hipMemcpyDeviceToHost));
  if (ao.err) return fail(s, KMC_ERR_STATE, "prox: a bond link leaves the state or the link chains do not end");
  if (o.err) return fail(s, KMC_ERR_STATE, "prox: a reference index or a union-find chain left its range");
  std::memset(out, 0, sizeof *out);
  out->n_sel = (int64_t)o.sum[PX_N_SEL];
  out->n_core = (int64_t)o.sum[PX_N_CORE];
  out->n_border = (int64_t)o.sum[PX_N_BORDER];
  out->n_noise = (int64_t)o.sum[PX_N_NOISE];
  out->n_alone = (int64_t)o.sum[PX_N_ALONE];
  out->n_clusters = (int64_t)o.sum[PX_N_CLUSTERS];
  out->n_multi = (int64_t)o.sum[PX_N_MULTI];
  out->sum_nn = (int64_t)o.sum[PX_SUM_NN];
  out->n_core_edges = (int64_t)o.sum[PX_N_EDGES];
  out->n_pure = (int64_t)o.sum[PX_N_PURE];
  out->n_whole = (int64_t)o.sum[PX_N_WHOLE];
  out->n_bond_multi = (int64_t)o.sum[PX_N_BMULTI];
  out->n_bond_kept = (int64_t)o.sum[PX_N_BKEPT];
  if (o.best) {
    out->max_size = (int32_t)(o.best >> 32);
    out->max_label = (int32_t)(0xffffffffu - (uint32_t)o.best) + 1;
  }
  const size_t n = (size_t)N;
  if (size_hist)
    HIPCHK(s, hipMemcpy(size_hist, X.size_hist, sizeof(int64_t) * ((size_t)max_size + 1), hipMemcpyDeviceToHost));
  if (nn_hist) HIPCHK(s, hipMemcpy(nn_hist, X.nn_hist, sizeof(int64_t) * PX_NN_ROWS, hipMemcpyDeviceToHost));
  if (nnd_hist) HIPCHK(s, hipMemcpy(nnd_hist, X.nnd_hist, sizeof(int64_t) * (size_t)nbins, hipMemcpyDeviceToHost));
  if (label && n) HIPCHK(s, hipMemcpy(label, X.label, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (nn && n) HIPCHK(s, hipMemcpy(nn, X.nn, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (kind && n) HIPCHK(s, hipMemcpy(kind, X.kind, n, hipMemcpyDeviceToHost));
  return KMC_OK;
}

}  // extern "C"
