// Joint reweighted histograms of a ladder's samples along TWO quantities (me_mbar_histogram_joint and its engine-less twin in the
// public header): the distribution p(A, B; T) at any temperature, from which the free-energy surface F(A, B; T) = -T ln p(A, B;
// T) follows.
//
// Definition.  The weights are me_mbar_hist.hip's: d_n = m_n + ln s_n, l_nt = -E_n / T_t - d_n, w_nt = exp(min(l_nt - ln_z_t,
// 0)); a sample is USED when its ENERGY is finite.  Each axis has its own n_bins + 1 edges (finite, strictly increasing, any
// spacing) and the slot rule of me_mbar_hist.hip (slot_of, me_mbar_slots.h): slot_x in [0, Bx + 3), slot_y in [0, By + 3) -- the
// bins, then below, above (a value ON the last edge is above) and not a number.  A used sample falls into exactly one of the
// S = (Bx + 3)(By + 3) cells, cell = slot_x (By + 3) + slot_y, and
//     mass[t][cell] = sum_{n in cell} w_nt / sum_n w_nt,      counts[cell] = #{n in cell},
// the total taken over ALL cells in a fixed order, so that a temperature's masses sum to 1 by construction.  ln_z_t and
// neff_fraction are reweight_enqueue's, d_n is log_denominator_enqueue's, as in the 1-D unit.
//
// Kernels.
//   k_mbar_hist2d<R>     slot_pass (me_mbar_slots.h, which describes the scheme and the summation order, with "cell" for
//                        "slot") with Slots2d and the TemperatureRows<R> of k_mbar_hist: one pass per chunk of R temperatures
//                        reads E_n, d_n and the two values (32 bytes per sample; an axis that IS the energy reads nothing
//                        more), ONE exponential per (sample, temperature), both edge arrays in LDS, two branch-free binary
//                        searches.  The counts are added in the first pass only (with_counts).
//   k_mbar_hist_sum, k_mbar_hist_normalise (me_mbar_slots.h)   the block partials of every (temperature, cell) in a fixed order;
//                        the total over the S cells in a fixed order, then the division.
// R is chosen from S alone (below), so a mass is bit for bit the same alone or among any number of temperatures.  (Exchanging
// the axes transposes the counts exactly; the masses then agree to rounding only, because the normalising total runs over the
// cells in another order.)
//
// LDS and the temperatures per pass.  A workgroup holds (Bx + By + 2) 8 bytes of edges and 4 S (8 R + 4) bytes of tables; the
// edges are at most 2 S bytes (one axis of a single bin), so a workgroup needs at most S (32 R + 18) bytes.  R is the widest of
// 4, 2, 1 with which THREE workgroups fit the 160 KiB of a CU (54 613 bytes each), from S ALONE:
//     R = 4   S <= 374    (up to 16 x 16 bins)         at most 54 604 bytes    4 workgroups per CU up to S = 280, then 3
//     R = 2   S <= 666    (up to 22 x 22 bins)         at most 54 612 bytes    4 up to S = 499, then 3
//     R = 1   S <= 1296   (up to 33 x 33 bins)         at most 64 280 bytes    4 up to S = 819, 3 up to 1092, then 2
// so the small grids keep the four workgroups per CU (4 wavefronts per SIMD) of the 1-D kernel at 256 bins.  Three is the
// measured choice (profiles/mbar_surface.txt: 2^25 samples, 8 temperatures, R forced): giving up the fourth workgroup for half
// the passes wins by 10 to 25 % (361 cells: 3.7 / 6.0 ms at R = 4 against 4.1 / 7.6 at R = 2; 625 cells: 4.9 / 10.1 ms at R = 2
// against 5.7 / 12.6 at R = 1), giving up the third does not (400 and 441 cells at R = 4, 784 at R = 2: within 15 % either way).
// ME_MAX_HISTOGRAM2D_SLOTS = 1296 keeps the whole table under 64 KiB of LDS (no dynamic-LDS attribute) and two workgroups, 2
// wavefronts per SIMD, on a CU.  -DME_HIST2D_ROWS=4 / 2 / 1 forces that R wherever its table fits 64 KiB (to be measured
// against).
// histogram2d(), the argument checks and the two ways to a ValuePair are declared in me_mbar.h: me_mbar_hist2d_cov.hip runs them
// first and takes its d_n and edges from the HistogramScratch they leave.
// Registers (hipcc -O3, gfx950): profiles/mbar_slot_skeleton.txt; no AGPRs, no scratch, and the registers allow more
// wavefronts per SIMD than the LDS (4 to 2 workgroups of 4 wavefronts), which is what limits the occupancy.
#include "me_mbar_slots.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {
namespace {

#ifndef ME_HIST2D_ROWS
#define ME_HIST2D_ROWS 0
#endif
// 0: the rule of rows_per_pass; 4, 2, 1: that R wherever its table fits 64 KiB (to be measured against)
constexpr int kForcedRows = ME_HIST2D_ROWS;
constexpr int kMaxRows = 4;
constexpr int kMinBlocksPerCu = 3;              // 3 wavefronts per SIMD: the measured choice (the header comment)

// the joint rule (me_mbar_slots.h) for tables WITH counts: S (32 R + 18) bytes at most
constexpr int cells_at(int rows) { return joint_cells_at(rows, true, kMinBlocksPerCu); }
static_assert(cells_at(4) == 374 && cells_at(2) == 666, "the thresholds of the header comment");
static_assert(joint_lds_bound(1, ME_MAX_HISTOGRAM2D_SLOTS, true) <= 64 * 1024, "the largest table needs no dynamic-LDS attribute");

// R of a launch, from the number of cells alone.  tools/bench_mbar.py (surface_rows) restates this rule to print its pass
// counts: change both together.
int rows_per_pass(int n_cells) { return joint_rows_per_pass(n_cells, kMaxRows, true, kMinBlocksPerCu, kForcedRows); }

// values_x / values_y: the two value columns (Slots2d; nullptr: the axis is the energy itself); edges = [edges_x | edges_y];
// ln_z has stride 4 (reweight_enqueue's out); with_counts: this pass also counts
template <int kRows>
__global__ void __launch_bounds__(kThreads) k_mbar_hist2d(const double *__restrict__ energies, const double *__restrict__ d,
                                                          const double *__restrict__ values_x, const double *__restrict__ values_y,
                                                          long long n_chains, long long record_stride,
                                                          const double *__restrict__ edges, int n_bins_x, int n_bins_y, int top_x,
                                                          int top_y, const double *__restrict__ inv_temps,
                                                          const double *__restrict__ ln_z, int n_targets, int with_counts,
                                                          long long n_tiles, double *partials, unsigned long long *count_partials) {
  const Slots2d where{values_x, values_y, n_bins_x, n_bins_y, top_x, top_y};
  const TemperatureRows<kRows> rows(inv_temps, ln_z, n_targets);
  slot_pass<kRows, true>(energies, d, n_chains, record_stride, edges, where, rows, with_counts, n_tiles, partials, count_partials);
}

}  // namespace

// histogram_slots (me_mbar_hist.hip) for the S cells of the grid and the concatenated edges (me_mbar.h)
hipError_t histogram2d(Problem &p, const Source &src, const ValuePair &values, const double *f, const double *temps, int n_temps,
                       const Histogram2d &h, HistogramScratch &keep) {
  const int n_edges_x = h.n_bins_x + 1, n_edges_y = h.n_bins_y + 1, n_cells = (h.n_bins_x + 3) * (h.n_bins_y + 3);
  const int rows = rows_per_pass(n_cells);
  std::vector<double> edges(h.edges_x, h.edges_x + n_edges_x);
  edges.insert(edges.end(), h.edges_y, h.edges_y + n_edges_y);
  keep.top = top_of(n_edges_x);
  keep.top_y = top_of(n_edges_y);
  const size_t lds = slot_pass_lds(rows, n_cells, n_edges_x + n_edges_y, true);
  const auto launch = [&](int t0, int nt, double *partials, unsigned long long *count_partials) {
    const auto kernel = rows == 4 ? k_mbar_hist2d<4> : rows == 2 ? k_mbar_hist2d<2> : k_mbar_hist2d<1>;
    hipLaunchKernelGGL(kernel, dim3(blocks_of(p.sm.n_samples)), dim3(kThreads), lds, p.stream, p.sm.energies,
                       keep.d.get<const double>(), values.x, values.y, values.n_chains, values.record_stride,
                       keep.edges.get<const double>(), h.n_bins_x, h.n_bins_y, keep.top, keep.top_y,
                       p.w.inv_temps.get<const double>() + t0, p.w.out.get<const double>() + 4 * (size_t)t0, nt, t0 == 0,
                       tiles_of(p.sm.n_samples), partials, count_partials);
  };
  return histogram_slots(p, src, f, temps, n_temps,
                         SlotTable{edges.data(), n_edges_x + n_edges_y, n_cells, rows, h.mass, h.counts, h.neff, launch}, keep);
}

int check_histogram2d(const Source &src, const double *f, const double *temps, int n, const Histogram2d &h) {
  int rc = check_edges(src.e, h.edges_x, h.n_bins_x);
  if (rc) return rc;
  rc = check_edges(src.e, h.edges_y, h.n_bins_y);
  if (rc) return rc;
  if ((h.n_bins_x + 3) * (h.n_bins_y + 3) > ME_MAX_HISTOGRAM2D_SLOTS)
    return fail(src.e, ME_ERR_INVALID, "(n_bins_x + 3) (n_bins_y + 3) must not exceed " + std::to_string(ME_MAX_HISTOGRAM2D_SLOTS));
  return check_f_and_targets(src.e, f, src.n_rungs, temps, n, 1);
}

int joint_columns(const Source &src, int column_x, int column_y, ValuePair &values) {
  ObsColumns x{}, y{};
  int rc = histogram_column(src, column_x, x);
  if (rc) return rc;
  rc = histogram_column(src, column_y, y);
  if (rc) return rc;
  // recorded columns share the store's strides; the energy is read as the energy (nullptr), whatever the other axis is
  const ObsColumns &strides = column_x >= 0 ? x : y;
  values = ValuePair{column_x >= 0 ? x.data : nullptr, column_y >= 0 ? y.data : nullptr, strides.n_chains, strides.record_stride};
  return ME_OK;
}

int joint_upload(Source &src, const double *values_x, const double *values_y, int64_t n_samples, ValuePair &values) {
  const size_t column_bytes = sizeof(double) * (size_t)n_samples;
  ME_HIP(nullptr, src.columns_dev.resize(2 * column_bytes));
  double *columns = src.columns_dev.get<double>();
  ME_HIP(nullptr, hipMemcpy(columns, values_x, column_bytes, hipMemcpyHostToDevice));
  ME_HIP(nullptr, hipMemcpy(columns + n_samples, values_y, column_bytes, hipMemcpyHostToDevice));
  values = ValuePair{columns, columns + n_samples, n_samples, 0};
  return ME_OK;
}

namespace {

// the two forms of me_mbar_histogram_joint behind their Source
int histogram2d_common(const Source &src, const ValuePair &values, const double *f, const double *temps, int n, const Histogram2d &h) {
  const int rc = check_histogram2d(src, f, temps, n, h);
  if (rc) return rc;
  Problem p;
  HistogramScratch keep;
  return mbar_check_common(src.e, p, histogram2d(p, src, values, f, temps, n, h, keep));
}

}  // namespace
}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_mbar_histogram_joint(me_engine *e, const double *f, const double *temps, int32_t n, int32_t column_x, const double *edges_x,
                        int32_t n_bins_x, int32_t column_y, const double *edges_y, int32_t n_bins_y, double *mass, int64_t *counts,
                        double *neff_fraction) {
  Source src;
  int rc = src.from_engine(e);
  if (rc) return rc;
  ValuePair values{};
  rc = joint_columns(src, column_x, column_y, values);
  if (rc) return rc;
  return histogram2d_common(src, values, f, temps, n, Histogram2d{edges_x, n_bins_x, edges_y, n_bins_y, mass, counts, neff_fraction});
}

int me_mbar_histogram_joint_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                                const double *values_x, const double *values_y, const double *edges_x, int32_t n_bins_x,
                                const double *edges_y, int32_t n_bins_y, double *mass, int64_t *counts, double *neff_fraction) {
  if (!values_x || !values_y) return fail(nullptr, ME_ERR_INVALID, "null pointer");
  Source src;
  int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs);
  if (rc) return rc;
  ValuePair values{};
  rc = joint_upload(src, values_x, values_y, n_samples, values);
  if (rc) return rc;
  return src.finish(
      histogram2d_common(src, values, f, temps, n, Histogram2d{edges_x, n_bins_x, edges_y, n_bins_y, mass, counts, neff_fraction}));
}

}  // extern "C"
