// The slot Gram sums behind the error bars of a reweighted histogram (me_mbar_histogram_gram and its engine-less twin in the
// public header): what the asymptotic covariance of MBAR (me_mbar_cov.hip; Shirts & Chodera 2008, eq. D8) needs for the
// weight matrix [K ladder columns | state column of target t | one indicator column per slot], WITHOUT forming that matrix.
//
// Definition.  Notation of me_mbar_cov.hip and me_mbar_hist.hip: a sample is USED when its energy is finite, d_n is the log
// denominator, slot_n in [0, n_bins + 3) the slot of its value (half-open bins, then below, above, NaN),
//     W_nj = exp(min(f_j - E_n / T_j - d_n, 0))              ladder column j, the expression of k_mbar_gram's fill
//     w_nt = exp(min(-E_n / T_t - d_n - ln_z_t, 0))          state column of target t, the weight k_mbar_hist forms
// and the indicator column of (t, s) is w_nt 1[slot_n = s] / p_ts with p_ts the histogram's mass.  The indicator columns of
// one target are disjoint, so every entry of the Gram matrix that involves them follows from
//     H[t][j][s] = sum_{n used, slot_n = s} W_nj w_nt   (j < K),       H[t][K][s] = sum_{n used, slot_n = s} w_nt^2:
// ladder_j x slot_s = H[t][j][s] / p_ts, state x slot_s = H[t][K][s] / p_ts, slot_s x slot_s' = delta_ss' H[t][K][s] / p_ts^2,
// ladder_j x state = sum_s H[t][j][s], state x state = sum_s H[t][K][s]; the ladder x ladder block is mbar_gram's with no
// targets.  The host never assembles the matrix: the state and slot columns have no samples of their own, so the covariance of
// the log masses reduces to one K x K pseudo-inverse and O(S K^2) products (statistics.py, _SlotLogCovariance, which the
// joint unit's cells share).
//
// Host.  slot_gram_passes is the driver of both Gram units (this one and me_mbar_hist2d_cov.hip), as histogram_slots is of the
// mass units, and histogram_gram_stages the body of their entry points behind the argument checks; a unit keeps its kernel, its
// choice of R and its launch (SlotGramTable, me_mbar.h).
//
// Kernels.  The masses, counts, ln_z_t and d_n are those of histogram() (me_mbar_hist.hip), called first: the same code, the
// same bits.  k_mbar_hist_cov<R> is slot_pass (me_mbar_slots.h, which describes the scheme and the summation order) with
// k_mbar_hist's Slots1d and GramRows<R>: a chunk of R rows j of ONE temperature, one pass per (t, chunk), n ceil((K + 1) / R)
// passes, each reading 24 bytes per sample, finding the slot and forming w_nt (state_weight, as k_mbar_hist does) once and
// one more exponential per ladder row.  It keeps no counts.  k_mbar_hist_sum adds the block partials of every (row, slot) in
// a fixed order.  H[t][j][s] depends neither on t, nor on j, nor on R, nor on which chunk a row falls into.
// Rows per pass: R is a pure cost choice, passes against LDS (occupancy): the widest of 16, 8, 4 whose table leaves
// kMinBlocksPerCu = 4 workgroups on a CU (rows_per_pass): 16 up to 75 bins, 8 up to 152, 4 beyond.  Measured at 2^25 samples,
// 8 targets, K = 32, R = 4 / 8 / 16 forced (profiles/mbar_profile_uncertainty.txt), milliseconds for all passes: 64 bins, every
// value in one bin 39.8 / 34.5 / 34.9, 64 different bins per wavefront 97.0 / 58.4 / 47.1 (a wide R shares the match loop, the
// slot search and w_nt among its rows); 256 bins 46.5 / 57.5 / 86.6 and 109.8 / 103.4 / 129.1 (R = 16 leaves ONE workgroup per
// CU, one wavefront per SIMD, and nothing hides the LDS round trips of the table).  LDS per workgroup: (n_bins + 1) 8 + 4 R
// (n_bins + 3) 8 bytes: 34 824 at 64 bins with R = 16, 35 208 at 256 bins with R = 4.  Registers (hipcc -O3, gfx950):
// profiles/mbar_slot_skeleton.txt; no AGPRs, no kernel uses scratch.
#include "me_launch.h"
#include "me_mbar_slots.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {
namespace {

#ifndef ME_HIST_COV_ROWS
#define ME_HIST_COV_ROWS 0
#endif
// 0: the rule of rows_per_pass; 4, 8, 16: that R at every bin count (to be measured against: profiles/mbar_profile_uncertainty.txt)
constexpr int kForcedRows = ME_HIST_COV_ROWS;
constexpr int kMaxRows = 16;
constexpr int kMinBlocksPerCu = 4;              // 4 wavefronts per SIMD, k_mbar_hist's own occupancy at 256 bins

static_assert(slot_pass_lds(16, 64 + 3, 64 + 1, false) == 34824 && slot_pass_lds(4, 256 + 3, 256 + 1, false) == 35208,
              "the LDS of the header comment");

// R of a launch: the widest of 16, 8, 4 with which kMinBlocksPerCu workgroups fit a CU's LDS (R = 4 always does), by the EXACT
// bytes of the n_bins + 1 edges.  The joint units' rule (joint_rule_rows, me_mbar_slots.h) bounds the edges by 2 bytes per cell
// and would put the thresholds at 76 and 155 bins, not at the measured 75 and 152: this rule stays its own.
// tools/bench_mbar.py (gram_rows) restates this rule to print its pass counts: change both together.
constexpr int rule_rows(int n_bins) {
  for (int rows = kMaxRows; rows > 4; rows /= 2)
    if (kMinBlocksPerCu * slot_pass_lds(rows, n_bins + 3, n_bins + 1, false) <= kCuLds) return rows;
  return 4;
}
static_assert(rule_rows(75) == 16 && rule_rows(76) == 8 && rule_rows(152) == 8 && rule_rows(153) == 4,
              "the thresholds of the header comment");
int rows_per_pass(int n_bins) { return kForcedRows ? kForcedRows : rule_rows(n_bins); }

// One pass: rows j0 .. j0 + n_rows (n_rows <= kRows, j0 + n_rows <= n_rungs + 1) of target *inv_temp, *ln_z (GramRows).
// Samples and values are addressed as in k_mbar_hist.
template <int kRows>
__global__ void __launch_bounds__(kThreads) k_mbar_hist_cov(const double *__restrict__ energies, const double *__restrict__ d,
                                                            const double *__restrict__ values, long long n_chains,
                                                            long long record_stride, const double *__restrict__ edges, int n_bins,
                                                            int top, const double *__restrict__ table, int n_rungs,
                                                            const double *__restrict__ inv_temp, const double *__restrict__ ln_z,
                                                            int j0, int n_rows, long long n_tiles, double *partials) {
  const Slots1d where{values, n_bins, top};
  const GramRows<kRows> rows(table, n_rungs, inv_temp, ln_z, j0, n_rows);
  slot_pass<kRows, false>(energies, d, n_chains, record_stride, edges, where, rows, 0, n_tiles, partials, nullptr);
}

// enqueues rows j0 .. j0 + n_rows of target t of a problem whose histogram() left `keep`
template <int kRows>
hipError_t launch_pass(const Problem &p, const ObsColumns &values, const HistogramScratch &keep, int n_bins, int t, int j0,
                       int n_rows, double *partials) {
  constexpr size_t most = slot_pass_lds(kRows, ME_MAX_HISTOGRAM_BINS + 3, ME_MAX_HISTOGRAM_BINS + 1, false);
  if (most > 64 * 1024) ME_MBAR_HIP(raise_lds_limit<k_mbar_hist_cov<kRows>>(most));
  hipLaunchKernelGGL(k_mbar_hist_cov<kRows>, dim3(blocks_of(p.sm.n_samples)), dim3(kThreads),
                     slot_pass_lds(kRows, n_bins + 3, n_bins + 1, false), p.stream, p.sm.energies, keep.d.get<const double>(),
                     values.data, values.n_chains, values.record_stride, keep.edges.get<const double>(), n_bins, keep.top,
                     p.w.table.get<const double>(), p.n_rungs, p.w.inv_temps.get<const double>() + t,
                     p.w.out.get<const double>() + 4 * (size_t)t, j0, n_rows, tiles_of(p.sm.n_samples), partials);
  return hipSuccess;
}

// the Gram table of a problem whose histogram() left `keep`: R and its kernel from the bin count
SlotGramTable slot_gram_table(const Problem &p, const ObsColumns &values, const HistogramScratch &keep, int n_bins, double *slot_gram) {
  const int rows = rows_per_pass(n_bins);
  return SlotGramTable{n_bins + 3, rows, slot_gram, [=, &p, &keep](int t, int j0, int n_rows, double *partials) {
                         return rows == 16  ? launch_pass<16>(p, values, keep, n_bins, t, j0, n_rows, partials)
                                : rows == 8 ? launch_pass<8>(p, values, keep, n_bins, t, j0, n_rows, partials)
                                            : launch_pass<4>(p, values, keep, n_bins, t, j0, n_rows, partials);
                       }};
}

struct HistogramGram {
  Histogram h;
  double *slot_gram;
  LadderGram ladder;
};

// the two forms of me_mbar_histogram_gram behind their Source; the checks and their order are histogram_common's
int histogram_gram_common(const Source &src, const ObsColumns &values, const double *f, const double *temps, int n,
                          const HistogramGram &hg) {
  int rc = check_edges(src.e, hg.h.edges, hg.h.n_bins);
  if (rc) return rc;
  rc = check_f_and_targets(src.e, f, src.n_rungs, temps, n, 1);
  if (rc) return rc;
  return histogram_gram_stages(
      src, f, n, [&](Problem &p, HistogramScratch &keep) { return histogram(p, src, values, f, temps, n, hg.h, keep); },
      [&](const Problem &p, const HistogramScratch &keep) { return slot_gram_table(p, values, keep, hg.h.n_bins, hg.slot_gram); },
      hg.ladder);
}

}  // namespace

hipError_t slot_gram_passes(Problem &p, const SlotGramTable &table, int n_temps) {
  const int n_slots = table.n_slots, rows = table.rows, n_blocks = blocks_of(p.sm.n_samples), n_cols = p.n_rungs + 1;
  const size_t entries = (size_t)n_temps * n_cols * n_slots;
  DeviceBuffer partials, sums;
  ME_MBAR_HIP(partials.resize((size_t)n_blocks * rows * n_slots * sizeof(double)));
  ME_MBAR_HIP(sums.resize(entries * sizeof(double)));
  for (int t = 0; t < n_temps; ++t)
    for (int j0 = 0; j0 < n_cols; j0 += rows) {
      const int n_rows = std::min(rows, n_cols - j0);
      ME_MBAR_HIP(table.launch(t, j0, n_rows, partials.get<double>()));
      hipLaunchKernelGGL(k_mbar_hist_sum, dim3(n_slots, n_rows), dim3(kThreads), 0, p.stream, partials.get<const double>(),
                         (const unsigned long long *)nullptr, n_blocks, rows, n_slots,
                         sums.get<double>() + ((size_t)t * n_cols + j0) * n_slots, (long long *)nullptr);
    }
  ME_MBAR_HIP(hipGetLastError());
  ME_MBAR_HIP(hipMemcpyAsync(table.gram, sums.get(), entries * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  return hipStreamSynchronize(p.stream);
}

int histogram_gram_stages(const Source &src, const double *f, int n_temps,
                          const std::function<hipError_t(Problem &, HistogramScratch &)> &histogram,
                          const std::function<SlotGramTable(const Problem &, const HistogramScratch &)> &gram_table,
                          const LadderGram &out) {
  int rc;
  long long n_used = 0;
  {
    Problem p;
    HistogramScratch keep;
    rc = mbar_check_common(src.e, p, histogram(p, keep));
    if (rc) return rc;
    const SlotGramTable table = gram_table(p, keep);
    if (table.gram) {
      rc = mbar_check_common(src.e, p, slot_gram_passes(p, table, n_temps));
      if (rc) return rc;
    }
    n_used = p.n_used_ll;
  }                                                                // (the problem's device scratch and d_n go before the next pass)
  if (out.ladder_gram || out.column_counts) {
    // The Gram pass with no targets (me_mbar_cov.hip), reused whole: it prepares a problem of its own (a second counting pass
    // over the samples) because it packs the used samples before anything else.
    Problem ladder;
    std::vector<double> gram((size_t)src.n_rungs * src.n_rungs), column_counts((size_t)src.n_rungs);
    rc = mbar_check_common(src.e, ladder, mbar_gram(ladder, src, f, nullptr, 0, gram.data(), column_counts.data(), nullptr, nullptr));
    if (rc) return rc;
    if (out.ladder_gram) std::copy(gram.begin(), gram.end(), out.ladder_gram);
    if (out.column_counts) std::copy(column_counts.begin(), column_counts.end(), out.column_counts);
  }
  if (out.n_used) *out.n_used = n_used;
  return ME_OK;
}

}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_mbar_histogram_gram(me_engine *e, const double *f, const double *temps, int32_t n, int32_t column, const double *edges,
                           int32_t n_bins, double *slot_gram, double *ladder_gram, double *column_counts, double *mass,
                           int64_t *counts, double *neff_fraction, int64_t *n_used) {
  Source src;
  int rc = src.from_engine(e);
  if (rc) return rc;
  ObsColumns values{};
  rc = histogram_column(src, column, values);
  if (rc) return rc;
  return histogram_gram_common(src, values, f, temps, n,
                               HistogramGram{Histogram{edges, n_bins, mass, counts, neff_fraction}, slot_gram,
                                             LadderGram{ladder_gram, column_counts, n_used}});
}

int me_mbar_histogram_gram_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                   const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                                   const double *values, const double *edges, int32_t n_bins, double *slot_gram,
                                   double *ladder_gram, double *column_counts, double *mass, int64_t *counts,
                                   double *neff_fraction, int64_t *n_used) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs, values, 1);
  return rc ? rc
            : src.finish(histogram_gram_common(src, src.columns, f, temps, n,
                                               HistogramGram{Histogram{edges, n_bins, mass, counts, neff_fraction}, slot_gram,
                                                             LadderGram{ladder_gram, column_counts, n_used}}));
}

}  // extern "C"
