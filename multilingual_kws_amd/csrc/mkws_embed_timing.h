// mkws_embed_timing.h -- development-build reporting for the launchers of mkws_embed.hip (`make timing`: -DMKWS_FRONT_TIMING).
//
// Not a stand-alone header: mkws_embed.hip includes it once, inside its anonymous namespace, behind the kernels and their argument
// structs.  The kernels of a timing build leave wall_clock64 / shader-clock stamps in the buffers armed here; the report functions
// synchronise the stream, copy the stamps back and print one line per launch to stderr (never for benchmarks).  A launcher reads
//   fill args; timing_arm(args, ...); launch; timing_report_<kernel>(...);
// and in the product build every function below is an empty inline stub: no buffer, no synchronisation, no argument field.
#pragma once

#ifndef MKWS_FRONT_TIMING

template <class... A> inline void timing_arm(A&&...) {}
template <class... A> inline void timing_report_gemm(A&&...) {}
template <class... A> inline void timing_report_front(A&&...) {}
template <class... A> inline void timing_report_block(A&&...) {}
template <class... A> inline void timing_report_chain(A&&...) {}
template <class... A> inline void timing_report_cluster(A&&...) {}
template <class... A> inline void timing_report_cluster_chain(A&&...) {}
template <class... A> inline void timing_report_mid(A&&...) {}
inline void wg_trace_arm() {}
template <class... A> inline void wg_trace_report(A&&...) {}
template <class... A> inline void wg_phase_report(A&&...) {}

#else

// ---- stamp buffers (allocated on first use, never freed: a development build) ---------------------------------------------------
inline unsigned long long* timing_buffer(unsigned long long** slot, size_t words) {
  if (!*slot) (void)hipMalloc(slot, sizeof(unsigned long long) * words);
  return *slot;
}
inline unsigned long long* gemm_timing_buffer() { static unsigned long long* d = nullptr; return timing_buffer(&d, 2 * 65536); }
inline unsigned long long* front_timing_buffer() { static unsigned long long* d = nullptr; return timing_buffer(&d, 4 * 65536); }
constexpr size_t kMidStampWords = 8 * 65536;
inline unsigned long long* mid_timing_buffer() { static unsigned long long* d = nullptr; return timing_buffer(&d, kMidStampWords); }
// the whole-block kernels (block, pair, cluster, cluster chain): 8 stamps per workgroup
inline unsigned long long* block_timing_buffer() { static unsigned long long* d = nullptr; return timing_buffer(&d, 8 * 4096); }
inline unsigned long long* chain_timing_buffer() { static unsigned long long* d = nullptr; return timing_buffer(&d, 4096 * kChainMax * 8 + 4096); }
inline std::vector<unsigned long long> timing_fetch(hipStream_t s, const unsigned long long* d, size_t words) {
  (void)hipStreamSynchronize(s);
  std::vector<unsigned long long> h(words);
  (void)hipMemcpy(h.data(), d, words * 8, hipMemcpyDeviceToHost);
  return h;
}

// ---- arming: point the launch's argument struct at its stamp buffer -------------------------------------------------------------
inline void timing_arm(GemmArgs& a, const dim3& grid) { a.dbg_clk = (grid.x * grid.y <= 65536 && a.splitk == 1) ? gemm_timing_buffer() : nullptr; }
inline void timing_arm(FrontArgs& a) { a.dbg_t = front_timing_buffer(); }
inline void timing_arm(MidArgs& a, unsigned nwg) { a.dbg_t = ((size_t)nwg * kMidStamps <= kMidStampWords) ? mid_timing_buffer() : nullptr; }
inline void timing_arm(BlockArgs& a) { a.dbg_t = block_timing_buffer(); }
// (cluster kernels: padding workgroups leave before the first stamp, so the report tells live members by a nonzero stamp)
inline void timing_arm(BlockArgs& a, hipStream_t s) { a.dbg_t = block_timing_buffer(); (void)hipMemsetAsync(a.dbg_t, 0, sizeof(unsigned long long) * 8 * 4096, s); }
inline void timing_arm(ClusterChainArgs& cc, hipStream_t s) { cc.dbg_t = block_timing_buffer(); (void)hipMemsetAsync(cc.dbg_t, 0, sizeof(unsigned long long) * 8 * 4096, s); }
inline void timing_arm(ChainArgs& ca, unsigned nwg) { ca.dbg_t = (nwg <= 4096) ? chain_timing_buffer() : nullptr; }

// ---- per-CU timeline of the last launch from the (start, end, CU) triples the workgroups left (wg_trace_begin / _end) -----------
inline unsigned long long* wg_trace_buffer() {
  static unsigned long long* d = nullptr;
  if (!d) {
    (void)hipMalloc(&d, sizeof(unsigned long long) * (3 + 8) * 131072);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wgtrace), &d, sizeof(d));
    const char* ab = getenv("MKWS_ABLATE");
    const int abv = ab ? atoi(ab) : 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_ablate), &abv, sizeof(abv));
  }
  return d;
}
inline void wg_trace_arm() { (void)wg_trace_buffer(); }
inline void wg_trace_report(hipStream_t s, const char* stage, const char* kernel, size_t nblk) {
  const std::vector<unsigned long long> h = timing_fetch(s, wg_trace_buffer(), nblk * 3);
  std::map<unsigned, std::vector<std::pair<unsigned long long, unsigned long long>>> cu;
  unsigned long long t0 = ~0ull, t1 = 0; double dur = 0;
  for (size_t i = 0; i < nblk; ++i) {
    cu[(unsigned)h[3 * i + 2]].push_back({h[3 * i], h[3 * i + 1]});
    if (h[3 * i] < t0) t0 = h[3 * i];
    if (h[3 * i + 1] > t1) t1 = h[3 * i + 1];
    dur += (double)(h[3 * i + 1] - h[3 * i]);
  }
  // per CU: peak number of resident workgroups, time with >= 1 resident, slot time = peak x (last end - first start)
  size_t wmin = ~(size_t)0, wmax = 0; int peak_all = 0; double busy1 = 0, first = 0, last = 0, gap = 0; size_t ngap = 0;
  for (auto& kv : cu) {
    auto& v = kv.second;
    if (v.size() < wmin) wmin = v.size();
    if (v.size() > wmax) wmax = v.size();
    std::vector<std::pair<unsigned long long, int>> ev;
    for (auto& w : v) { ev.push_back({w.first, +1}); ev.push_back({w.second, -1}); }
    std::sort(ev.begin(), ev.end());
    int cur = 0, peak = 0; unsigned long long prev = ev[0].first; double b1 = 0;
    for (auto& e : ev) { if (cur > 0) b1 += (double)(e.first - prev); prev = e.first; cur += e.second; if (cur > peak) peak = cur; }
    if (peak > peak_all) peak_all = peak;
    busy1 += b1;
    first += (double)(ev.front().first - t0); last += (double)(t1 - ev.back().first);
    // gap between a workgroup's end and the next start on the same CU (slots paired greedily in time order)
    std::sort(v.begin(), v.end());
    std::vector<unsigned long long> ends;
    for (auto& w : v) {
      size_t best = ends.size();
      for (size_t k = 0; k < ends.size(); ++k) if (ends[k] <= w.first && (best == ends.size() || ends[k] > ends[best])) best = k;
      if (best == ends.size()) ends.push_back(w.second);
      else { gap += (double)(w.first - ends[best]); ++ngap; ends[best] = w.second; }
    }
  }
  const double span = (double)(t1 - t0), ncu = (double)cu.size();
  fprintf(stderr, "[wg-trace] %s %s: %zu workgroups on %zu CUs (%zu-%zu per CU, peak %d resident); mean workgroup %.2f us; span %.2f us; "
                  "mean residency %.2f; CU busy (>=1 resident) %.2f of span; first start +%.2f us, last end -%.2f us; slot gap %.2f us (n %zu)\n",
          stage, kernel, nblk, cu.size(), wmin, wmax, peak_all, dur / nblk / 100.0, span / 100.0, dur / (ncu * span), busy1 / (ncu * span),
          first / ncu / 100.0, last / ncu / 100.0, ngap ? gap / ngap / 100.0 : 0.0, ngap);
}
inline void wg_phase_report(const char* stage, size_t nblk, int nph) {
  std::vector<unsigned long long> h(nblk * 8);
  (void)hipMemcpy(h.data(), wg_trace_buffer() + 3 * 131072, h.size() * 8, hipMemcpyDeviceToHost);
  fprintf(stderr, "[wg-phase] %s: shader-clock cycles per workgroup (mean):", stage);
  for (int k = 0; k < nph; ++k) { double t = 0; for (size_t i = 0; i < nblk; ++i) t += (double)h[8 * i + k]; fprintf(stderr, " %d: %.0f", k, t / nblk); }
  fprintf(stderr, "\n");
}

// ---- one printer per kernel family (wall_clock64 ticks at 100 MHz) --------------------------------------------------------------
inline void timing_report_gemm(hipStream_t s, const char* stage, int MT, int NT, const dim3& grid, const GemmArgs& a) {
  if (!a.dbg_clk) return;
  const size_t nb = (size_t)grid.x * grid.y;
  const std::vector<unsigned long long> h = timing_fetch(s, a.dbg_clk, 2 * nb);
  double mhz = 0, us = 0;
  for (size_t i = 0; i < nb; ++i) { mhz += (double)h[2 * i] / ((double)h[2 * i + 1] / 100.0); us += (double)h[2 * i + 1] / 100.0; }
  fprintf(stderr, "[gemm-timing] %s <%d,%d>: %zu workgroups, K loop of wave 0: %.2f us mean, shader clock %.0f MHz\n", stage, MT, NT, nb, us / nb, mhz / nb);
}

inline void timing_report_front(hipStream_t s, const char* stage, int ks, int st, size_t nblk) {
  const std::vector<unsigned long long> h = timing_fetch(s, front_timing_buffer(), nblk * 4);
  double p1 = 0, bar = 0, p2 = 0; unsigned long long t0 = ~0ull, t1 = 0;
  for (size_t i = 0; i < nblk; ++i) {
    p1 += (double)(h[4 * i + 1] - h[4 * i]); bar += (double)(h[4 * i + 2] - h[4 * i + 1]); p2 += (double)(h[4 * i + 3] - h[4 * i + 2]);
    if (h[4 * i] < t0) t0 = h[4 * i];
    if (h[4 * i + 3] > t1) t1 = h[4 * i + 3];
  }
  fprintf(stderr, "[front-timing] %s ks%d s%d blocks %zu: phase1 %.2f us  barrier %.2f us  phase2 %.2f us  kernel span %.2f us\n", stage, ks, st, nblk,
          p1 / nblk / 100.0, bar / nblk / 100.0, p2 / nblk / 100.0, (double)(t1 - t0) / 100.0);
}

// per-phase means of the stamps mbconv_block_kernel / mbconv_pair_kernel leave
inline void timing_report_block(hipStream_t s, const char* stage, unsigned nblk) {
  const std::vector<unsigned long long> h = timing_fetch(s, block_timing_buffer(), (size_t)nblk * 8);
  double ph[6] = {0, 0, 0, 0, 0, 0}; unsigned long long t0 = ~0ull, t1 = 0;
  for (size_t i = 0; i < nblk; ++i) {
    for (int k = 0; k < 6; ++k) ph[k] += (double)(h[8 * i + k + 1] - h[8 * i + k]);
    if (h[8 * i] < t0) t0 = h[8 * i];
    if (h[8 * i + 6] > t1) t1 = h[8 * i + 6];
  }
  double clk = 0; for (size_t i = 0; i < nblk; ++i) clk += (double)h[8 * i + 7] / ((double)(h[8 * i + 6] - h[8 * i]) / 100.0);
  fprintf(stderr, "[block-timing] shader clock %.0f MHz\n", clk / nblk);
  fprintf(stderr, "[block-timing] %s blocks %u: stage %.2f  A %.2f  B %.2f  C1 %.2f  C2 %.2f  D %.2f us; span %.2f us\n", stage, nblk,
          ph[0] / nblk / 100.0, ph[1] / nblk / 100.0, ph[2] / nblk / 100.0, ph[3] / nblk / 100.0, ph[4] / nblk / 100.0,
          ph[5] / nblk / 100.0, (double)(t1 - t0) / 100.0);
}

// mbconv_chain_kernel: blocks[0 .. n - 1] are the chain's blocks, `names` their comma-separated names
inline void timing_report_chain(hipStream_t s, const BlockPlan* blocks, int n, const std::string& names, unsigned nwg, const ChainArgs& ca) {
  if (!ca.dbg_t) return;
  const std::vector<unsigned long long> h = timing_fetch(s, ca.dbg_t, (size_t)nwg * kChainMax * 8 + nwg);
  unsigned long long t0 = ~0ull, t1 = 0;
  for (unsigned w = 0; w < nwg; ++w) {
    t0 = std::min(t0, h[(size_t)nwg * kChainMax * 8 + w]);
    t1 = std::max(t1, h[((size_t)w * kChainMax + (n - 1)) * 8 + 6]);
  }
  double pro = 0;
  for (unsigned w = 0; w < nwg; ++w) pro += (double)(h[((size_t)w * kChainMax) * 8 + 7] - h[(size_t)nwg * kChainMax * 8 + w]);
  fprintf(stderr, "[chain-timing] %s: %u workgroups, span %.2f us, prologue %.2f us\n", names.c_str(), nwg, (double)(t1 - t0) / 100.0, pro / nwg / 100.0);
  for (int k = 0; k < n; ++k) {
    double ph[7] = {0, 0, 0, 0, 0, 0, 0};
    unsigned long long e_min = ~0ull, e_max = 0;
    for (unsigned w = 0; w < nwg; ++w) {
      const unsigned long long* q = &h[((size_t)w * kChainMax + k) * 8];
      ph[0] += (double)(q[0] - q[7]);
      for (int j = 0; j < 6; ++j) ph[j + 1] += (double)(q[j + 1] - q[j]);
      e_min = std::min(e_min, q[6]); e_max = std::max(e_max, q[6]);
    }
    fprintf(stderr, "[chain-timing]   %s: args %.2f  A %.2f  B %.2f  C1 %.2f  C2 %.2f  gate %.2f  D %.2f us; end skew %.2f us\n", blocks[k].spec.name,
            ph[0] / nwg / 100.0, ph[1] / nwg / 100.0, ph[2] / nwg / 100.0, ph[3] / nwg / 100.0, ph[4] / nwg / 100.0, ph[5] / nwg / 100.0,
            ph[6] / nwg / 100.0, (double)(e_max - e_min) / 100.0);
  }
}

// mbconv_cluster_kernel, members of live clusters only.  MKWS_CLUSTER_TWICE in the environment: `relaunch` repeats the launch and the
// second one, whose weights are hot in the XCD's L2, is reported too (dev aid).
template <class Relaunch>
inline void timing_report_cluster(hipStream_t s, const char* stage, unsigned nwg, Relaunch relaunch) {
  static const bool twice = getenv("MKWS_CLUSTER_TWICE") != nullptr;
  for (int rep = 0; rep < (twice ? 2 : 1); ++rep) {
    if (rep == 1) {
      (void)hipMemsetAsync(block_timing_buffer(), 0, sizeof(unsigned long long) * 8 * 4096, s);
      relaunch();
    }
    const std::vector<unsigned long long> h = timing_fetch(s, block_timing_buffer(), (size_t)nwg * 8);
    double ph[6] = {0, 0, 0, 0, 0, 0}; int n = 0; unsigned long long t0 = ~0ull, t1 = 0; double clk = 0;
    for (size_t i = 0; i < nwg; ++i) {
      if (h[8 * i + 6] == 0) continue;
      clk += (double)h[8 * i + 7] / ((double)(h[8 * i + 6] - h[8 * i]) / 100.0);      // shader-clock ticks per us of wall clock = MHz
      for (int k = 0; k < 6; ++k) ph[k] += (double)(h[8 * i + k + 1] - h[8 * i + k]);
      if (h[8 * i] < t0) t0 = h[8 * i];
      if (h[8 * i + 6] > t1) t1 = h[8 * i + 6];
      ++n;
    }
    if (n) fprintf(stderr, "[cluster-timing] %s%s members %d: stage %.2f  A %.2f  B %.2f  C1+x1 %.2f  C2 %.2f  D+x2 %.2f us; span %.2f us; shader clock %.0f MHz\n", stage, rep ? " (again: L2-hot)" : "", n,
                   ph[0] / n / 100.0, ph[1] / n / 100.0, ph[2] / n / 100.0, ph[3] / n / 100.0, ph[4] / n / 100.0, ph[5] / n / 100.0, (double)(t1 - t0) / 100.0, clk / n);
  }
}

// mbconv_cluster_chain_kernel: per block, over its members (workgroups cc.base[k] .. cc.base[k + 1] - 1): latest start, latest end of
// the wait, then the phases from there
inline void timing_report_cluster_chain(hipStream_t s, const BlockPlan* blocks, const ClusterChainArgs& cc) {
  const int nwg = cc.base[cc.n];
  const std::vector<unsigned long long> h = timing_fetch(s, cc.dbg_t, (size_t)nwg * 8);
  unsigned long long t0 = ~0ull;
  for (int i = 0; i < nwg; ++i) if (h[8 * (size_t)i + 6] != 0 && h[8 * (size_t)i] < t0) t0 = h[8 * (size_t)i];
  for (int k = 0; k < cc.n; ++k) {
    double st[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int nm = 0;
    for (int i = cc.base[k]; i < cc.base[k + 1]; ++i) {
      if (h[8 * (size_t)i + 6] == 0) continue;
      for (int q = 0; q < 8; ++q) st[q] = std::max(st[q], (double)(h[8 * (size_t)i + q] - t0) / 100.0);
      ++nm;
    }
    fprintf(stderr, "[cluster-chain] %-3s members %2d: started %6.2f  wait over %6.2f | input staged %6.2f  A %6.2f  B %6.2f  C1+x1 %6.2f  C2 %6.2f  D+x2+publish %6.2f us (latest member, since the launch's first stamp)\n",
            blocks[k].spec.name, nm, st[0], st[7], st[1], st[2], st[3], st[4], st[5], st[6]);
  }
}

// mbconv_mid_kernel: means over the workgroups of the durations thread 0 stamped (the slot table stands at MID_STAMP)
inline void timing_report_mid(hipStream_t s, const char* stage, int CC, int G, int nch, unsigned nwg, int nthr, size_t lds) {
  if ((size_t)nwg * kMidStamps > kMidStampWords) return;           // not armed
  const std::vector<unsigned long long> h = timing_fetch(s, mid_timing_buffer(), (size_t)nwg * kMidStamps);
  double m[kMidStamps] = {}; unsigned long long t0 = ~0ull, t1 = 0;
  for (size_t i = 0; i < nwg; ++i) {
    const unsigned long long* q = &h[i * kMidStamps];
    for (int k = 1; k < kMidStampProj + 3; ++k) m[k] += (double)q[k] / nwg / 100.0;
    m[0] += (double)(q[kMidStampProj + 3] - q[0]) / nwg / 100.0;
    t0 = std::min(t0, q[0]); t1 = std::max(t1, q[kMidStampProj + 3]);
  }
  double p1 = 0, p2 = 0, se = 0;
  for (int c = 0; c < nch; ++c) { p1 += m[2 + 4 * c] + m[3 + 4 * c]; p2 += m[4 + 4 * c] + m[5 + 4 * c]; }
  for (int k = kMidStampSE; k < kMidStampProj; ++k) se += m[k];
  fprintf(stderr, "[mid-timing] %s CC %d G %d: %u workgroups x %d thr, lds %zu: prologue %.2f  expand %.2f  depthwise %.2f  SE %.2f  project %.2f  total %.2f us per workgroup; span %.2f us\n",
          stage, CC, G, nwg, nthr, lds, m[1], p1, p2, se, m[kMidStampProj] + m[kMidStampProj + 1] + m[kMidStampProj + 2], m[0], (double)(t1 - t0) / 100.0);
  fprintf(stderr, "[mid-phases] %s: chunks (P1 tasks of wave 0, +constants stored +barrier, P2 items, +constants stored +barrier):", stage);
  for (int c = 0; c < nch; ++c) fprintf(stderr, " [%.2f %.2f %.2f %.2f]", m[2 + 4 * c], m[3 + 4 * c], m[4 + 4 * c], m[5 + 4 * c]);
  fprintf(stderr, "; SE per barrier:");
  for (int k = kMidStampSE; k < kMidStampProj; ++k) fprintf(stderr, " %.2f", m[k]);
  fprintf(stderr, "; projection: ring wait %.2f  MFMA loop of wave 0 %.2f  last wave %.2f us\n", m[kMidStampProj], m[kMidStampProj + 1], m[kMidStampProj + 2]);
}

#endif  // MKWS_FRONT_TIMING
