// The cell Gram sums behind the error bars of a joint reweighted histogram (me_mbar_histogram_joint_gram and its engine-less
// twin in the public header): me_mbar_hist_cov.hip for the cells of me_mbar_hist2d.hip's grid.  What the asymptotic covariance
// of MBAR needs for the weight matrix [K ladder columns | state column of target t | one indicator column per cell], WITHOUT
// forming that matrix.
//
// Definition.  Notation of me_mbar_hist_cov.hip with "cell" for "slot": the cell of a used sample is Slots2d's cell_n = slot_x
// (By + 3) + slot_y in [0, S), S = (Bx + 3)(By + 3) <= ME_MAX_HISTOGRAM2D_SLOTS,
//     H[t][j][c] = sum_{n used, cell_n = c} W_nj w_nt   (j < K),       H[t][K][c] = sum_{n used, cell_n = c} w_nt^2
// with W_nj k_mbar_gram's fill and w_nt state_weight (me_mbar_slots.h).  The indicator columns of one target are disjoint, so
// every entry of the Gram matrix that involves them follows from H, the masses and the ladder block exactly as in the 1-D
// unit.  The host never assembles the (K + 1 + S)-column matrix: the state and cell columns have no samples of their own, so
// the covariance of the log masses reduces to a K x K problem (statistics.py, _SlotLogCovariance, for bins and cells alike).
// The host driver and the stages of the entry points are the 1-D unit's (slot_gram_passes, histogram_gram_stages, me_mbar.h):
// this file keeps its kernel, its choice of R and its launch.
//
// Kernels.  The masses, counts, ln_z_t and d_n are those of histogram2d() (me_mbar_hist2d.hip), called first: the same code,
// the same bits.  k_mbar_hist2d_cov<R> is slot_pass (me_mbar_slots.h, which describes the scheme and the summation order) with
// k_mbar_hist2d's Slots2d and k_mbar_hist_cov's GramRows<R>: a chunk of R rows j of ONE temperature, one pass per (t, chunk),
// n ceil((K + 1) / R) passes, each reading E_n, d_n and the two values (32 bytes per sample; an axis that IS the energy reads
// nothing more), finding the cell and forming w_nt once and one more exponential per ladder row.  It keeps no counts.
// k_mbar_hist_sum adds the block partials of every (row, cell) in a fixed order.  H[t][j][c] depends neither on t's position
// in the request, nor on the chunk that row j falls into, nor on R.
//
// Rows per pass.  R is a pure cost choice, passes against LDS (occupancy), made from S ALONE as in me_mbar_hist2d.hip.  A
// workgroup holds (Bx + By + 2) 8 bytes of edges, at most 2 S, and 4 R S 8 bytes of tables (no counts): at most S (32 R + 2)
// bytes.  R is the widest of 16, 8, 4, 2, 1 with which kMinBlocksPerCu = 3 workgroups fit the 160 KiB of a CU (54 613 bytes
// each):
//     R = 16   S <= 106     (up to 7 x 7 bins)          at most 54 484 bytes
//     R = 8    S <= 211     (up to 11 x 11 bins)        at most 54 438 bytes
//     R = 4    S <= 420     (up to 17 x 17 bins)        at most 54 600 bytes
//     R = 2    S <= 827     (up to 25 x 25 bins)        at most 54 582 bytes
//     R = 1    S <= 1296    (up to 33 x 33 bins)        at most 44 064 bytes
// so every table stays under 64 KiB (no dynamic-LDS attribute).  Three workgroups is the value me_mbar_hist2d.hip measured for
// its own table; what was measured for THIS kernel (R forced one step up and down around each threshold, 2^25 samples) is in
// profiles/mbar_surface_uncertainty.txt, and keeps it: above each threshold the narrower R is 14 to 37 % faster when a
// wavefront's samples share a cell (two workgroups per CU do not hide the table's LDS round trips), below it the wider R is up
// to 27 % faster when its 64 lanes fall in 64 cells and within 2 % otherwise, except at 196 cells (R = 4 15 % faster on the
// first input, 4 % slower on the second).  -DME_HIST2D_COV_ROWS=16 / 8 / 4 / 2 / 1 forces that R wherever its table fits 64 KiB
// (to be measured against).  Registers, LDS and scratch (hipcc -O3, gfx950): profiles/mbar_surface_uncertainty.txt.
#include "me_mbar_slots.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {
namespace {

#ifndef ME_HIST2D_COV_ROWS
#define ME_HIST2D_COV_ROWS 0
#endif
// 0: the rule of rows_per_pass; 16, 8, 4, 2, 1: that R wherever its table fits 64 KiB (to be measured against)
constexpr int kForcedRows = ME_HIST2D_COV_ROWS;
constexpr int kMaxRows = 16;
constexpr int kMinBlocksPerCu = 3;              // 3 wavefronts per SIMD: me_mbar_hist2d.hip's measured choice (the header comment)
static_assert(kForcedRows == 0 || kForcedRows == 1 || kForcedRows == 2 || kForcedRows == 4 || kForcedRows == 8 || kForcedRows == 16,
              "ME_HIST2D_COV_ROWS must be one of the kernel's instantiations");

// The joint rule (me_mbar_slots.h) for tables WITHOUT counts: R of a launch, from the number of cells alone.
// tools/bench_mbar.py (surface_gram_rows) restates this rule to print its pass counts: change both together.
constexpr size_t lds_bound(int rows, int n_cells) { return joint_lds_bound(rows, n_cells, false); }
constexpr int cells_at(int rows) { return joint_cells_at(rows, false, kMinBlocksPerCu); }
constexpr int rule_rows(int n_cells) { return joint_rule_rows(n_cells, kMaxRows, false, kMinBlocksPerCu); }
static_assert(lds_bound(16, 1) == 514 && lds_bound(1, 1) == 34, "32 R S + 2 S bytes");
static_assert(cells_at(16) == 106 && cells_at(8) == 211 && cells_at(4) == 420 && cells_at(2) == 827,
              "the thresholds of the header comment");
static_assert(lds_bound(16, cells_at(16)) <= 64 * 1024 && lds_bound(8, cells_at(8)) <= 64 * 1024 &&
                  lds_bound(4, cells_at(4)) <= 64 * 1024 && lds_bound(2, cells_at(2)) <= 64 * 1024 &&
                  lds_bound(1, ME_MAX_HISTOGRAM2D_SLOTS) <= 64 * 1024,
              "no table of the rule needs the dynamic-LDS attribute");
static_assert(rule_rows(106) == 16 && rule_rows(107) == 8 && rule_rows(212) == 4 && rule_rows(421) == 2 && rule_rows(828) == 1 &&
                  rule_rows(ME_MAX_HISTOGRAM2D_SLOTS) == 1,
              "the thresholds of the header comment");
int rows_per_pass(int n_cells) { return joint_rows_per_pass(n_cells, kMaxRows, false, kMinBlocksPerCu, kForcedRows); }

// One pass: rows j0 .. j0 + n_rows (n_rows <= kRows, j0 + n_rows <= n_rungs + 1) of target *inv_temp, *ln_z (GramRows).
// Samples and values are addressed as in k_mbar_hist2d.
template <int kRows>
__global__ void __launch_bounds__(kThreads)
    k_mbar_hist2d_cov(const double *__restrict__ energies, const double *__restrict__ d, const double *__restrict__ values_x,
                      const double *__restrict__ values_y, long long n_chains, long long record_stride,
                      const double *__restrict__ edges, int n_bins_x, int n_bins_y, int top_x, int top_y,
                      const double *__restrict__ table, int n_rungs, const double *__restrict__ inv_temp,
                      const double *__restrict__ ln_z, int j0, int n_rows, long long n_tiles, double *partials) {
  const Slots2d where{values_x, values_y, n_bins_x, n_bins_y, top_x, top_y};
  const GramRows<kRows> rows(table, n_rungs, inv_temp, ln_z, j0, n_rows);
  slot_pass<kRows, false>(energies, d, n_chains, record_stride, edges, where, rows, 0, n_tiles, partials, nullptr);
}

// enqueues rows j0 .. j0 + n_rows of target t of a problem whose histogram2d() left `keep`
template <int kRows>
void launch_pass(const Problem &p, const ValuePair &values, const HistogramScratch &keep, const Histogram2d &h, int t, int j0,
                 int n_rows, double *partials) {
  const int n_cells = (h.n_bins_x + 3) * (h.n_bins_y + 3);
  hipLaunchKernelGGL(k_mbar_hist2d_cov<kRows>, dim3(blocks_of(p.sm.n_samples)), dim3(kThreads),
                     slot_pass_lds(kRows, n_cells, h.n_bins_x + h.n_bins_y + 2, false), p.stream, p.sm.energies,
                     keep.d.get<const double>(), values.x, values.y, values.n_chains, values.record_stride,
                     keep.edges.get<const double>(), h.n_bins_x, h.n_bins_y, keep.top, keep.top_y, p.w.table.get<const double>(),
                     p.n_rungs, p.w.inv_temps.get<const double>() + t, p.w.out.get<const double>() + 4 * (size_t)t, j0, n_rows,
                     tiles_of(p.sm.n_samples), partials);
}

// the Gram table of a problem whose histogram2d() left `keep`: R and its kernel from the number of cells
SlotGramTable cell_gram_table(const Problem &p, const ValuePair &values, const HistogramScratch &keep, const Histogram2d &h,
                              double *cell_gram) {
  const int n_cells = (h.n_bins_x + 3) * (h.n_bins_y + 3), rows = rows_per_pass(n_cells);
  return SlotGramTable{n_cells, rows, cell_gram, [=, &p, &keep, &h](int t, int j0, int n_rows, double *partials) {
                         switch (rows) {
                           case 16: launch_pass<16>(p, values, keep, h, t, j0, n_rows, partials); break;
                           case 8: launch_pass<8>(p, values, keep, h, t, j0, n_rows, partials); break;
                           case 4: launch_pass<4>(p, values, keep, h, t, j0, n_rows, partials); break;
                           case 2: launch_pass<2>(p, values, keep, h, t, j0, n_rows, partials); break;
                           default: launch_pass<1>(p, values, keep, h, t, j0, n_rows, partials); break;
                         }
                         return hipSuccess;
                       }};
}

struct Histogram2dGram {
  Histogram2d h;
  double *cell_gram;
  LadderGram ladder;
};

// the two forms of me_mbar_histogram_joint_gram behind their Source; the checks and their order are histogram2d_common's
int histogram2d_gram_common(const Source &src, const ValuePair &values, const double *f, const double *temps, int n,
                            const Histogram2dGram &hg) {
  const int rc = check_histogram2d(src, f, temps, n, hg.h);
  if (rc) return rc;
  return histogram_gram_stages(
      src, f, n, [&](Problem &p, HistogramScratch &keep) { return histogram2d(p, src, values, f, temps, n, hg.h, keep); },
      [&](const Problem &p, const HistogramScratch &keep) { return cell_gram_table(p, values, keep, hg.h, hg.cell_gram); },
      hg.ladder);
}

}  // namespace
}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_mbar_histogram_joint_gram(me_engine *e, const double *f, const double *temps, int32_t n, int32_t column_x,
                                 const double *edges_x, int32_t n_bins_x, int32_t column_y, const double *edges_y,
                                 int32_t n_bins_y, double *cell_gram, double *ladder_gram, double *column_counts, double *mass,
                                 int64_t *counts, double *neff_fraction, int64_t *n_used) {
  Source src;
  int rc = src.from_engine(e);
  if (rc) return rc;
  ValuePair values{};
  rc = joint_columns(src, column_x, column_y, values);
  if (rc) return rc;
  return histogram2d_gram_common(src, values, f, temps, n,
                                 Histogram2dGram{Histogram2d{edges_x, n_bins_x, edges_y, n_bins_y, mass, counts, neff_fraction},
                                                 cell_gram, LadderGram{ladder_gram, column_counts, n_used}});
}

int me_mbar_histogram_joint_gram_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                         const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps,
                                         int32_t n, const double *values_x, const double *values_y, const double *edges_x,
                                         int32_t n_bins_x, const double *edges_y, int32_t n_bins_y, double *cell_gram,
                                         double *ladder_gram, double *column_counts, double *mass, int64_t *counts,
                                         double *neff_fraction, int64_t *n_used) {
  if (!values_x || !values_y) return fail(nullptr, ME_ERR_INVALID, "null pointer");
  Source src;
  int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs);
  if (rc) return rc;
  ValuePair values{};
  rc = joint_upload(src, values_x, values_y, n_samples, values);
  if (rc) return rc;
  return src.finish(histogram2d_gram_common(
      src, values, f, temps, n,
      Histogram2dGram{Histogram2d{edges_x, n_bins_x, edges_y, n_bins_y, mass, counts, neff_fraction}, cell_gram,
                      LadderGram{ladder_gram, column_counts, n_used}}));
}

}  // extern "C"
