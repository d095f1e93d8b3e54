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
//   k_mbar_hist2d<R>     one pass per chunk of R temperatures: reads E_n, d_n and the two values (32 bytes per sample; an axis
//                        that IS the energy reads nothing more), ONE exponential per (sample, temperature), both edge arrays in
//                        LDS, two branch-free binary searches.  Each wavefront owns a private LDS table [R][S] of doubles and
//                        [S] counts (integer LDS atomics, added in the first pass only); the weights go into the table through
//                        slot_accumulate (me_mbar_slots.h) with the cell as its slot: NO atomic touches a floating-point number
//                        and no cross-lane operation runs under a partial lane mask.
//   k_mbar_hist_sum, k_mbar_hist_normalise (me_mbar_slots.h)   the block partials of every (temperature, cell) in a fixed order;
//                        the total over the S cells in a fixed order, then the division.
// Summation order of one mass: that of me_mbar_hist.hip's header with "cell" for "slot"; it is fixed by the samples' cells and
// order alone.  Neither depends on the temperature or on R, R is chosen from S alone (below), and a temperature's weights are
// formed by the same instructions at every position of a chunk (`fp contract(off)`, the fused multiply-add spelled out): a mass
// is bit for bit the same run to run, alone or among any number of temperatures, and through the engine's store or host arrays
// of the same samples in the same order.  (Exchanging the axes transposes the counts exactly; the masses then agree to
// rounding only, because the normalising total runs over the cells in another order.)
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
// Registers (hipcc -O3, gfx950; profiles/mbar_surface.txt): 57 / 52 / 46 VGPRs for R = 4 / 2 / 1, no AGPRs, no scratch: the
// registers allow 7 / 8 / 8 wavefronts per SIMD, so LDS (4 to 2 workgroups of 4 wavefronts) is what limits the occupancy.
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
constexpr size_t kCuLds = 160 * 1024;           // LDS of a CU
constexpr int kMinBlocksPerCu = 3;              // 3 wavefronts per SIMD: the measured choice (the header comment)

// the most LDS a workgroup needs for S cells at R temperatures per pass, whatever the two bin counts
constexpr size_t lds_bound(int rows, int n_cells) { return (size_t)n_cells * (kWaves * (rows * sizeof(double) + sizeof(unsigned int)) + 2); }
constexpr int cells_at(int rows) { return (int)(kCuLds / kMinBlocksPerCu / lds_bound(rows, 1)); }
constexpr int kCells4 = cells_at(4), kCells2 = cells_at(2);
static_assert(kCells4 == 374 && kCells2 == 666, "the thresholds of the header comment");
static_assert(lds_bound(1, ME_MAX_HISTOGRAM2D_SLOTS) <= 64 * 1024, "the largest table needs no dynamic-LDS attribute");

// R of a launch, from the number of cells alone.  tools/bench_mbar.py (time_surface) restates this rule to print its pass
// counts: change both together.
int rows_per_pass(int n_cells) {
  if (kForcedRows && lds_bound(kForcedRows, n_cells) <= 64 * 1024) return kForcedRows;
  return n_cells <= kCells4 ? 4 : n_cells <= kCells2 ? 2 : 1;
}

size_t lds_bytes(int rows, int n_bins_x, int n_bins_y) {
  return (size_t)(n_bins_x + n_bins_y + 2) * sizeof(double) +
         (size_t)kWaves * (n_bins_x + 3) * (n_bins_y + 3) * (rows * sizeof(double) + sizeof(unsigned int));
}

// values_x / values_y: sample i = record * n_chains + chain sits at values[record * record_stride + chain] (two columns of the
// engine's store: n_chains, Q n_chains; host arrays: n, 0); nullptr: the axis is the energy itself.  `d` is padded to whole
// tiles.  edges = [edges_x | edges_y].  ln_z has stride 4 (reweight_enqueue's out).  with_counts: this pass also counts.
// Dynamic LDS: [edges_x | edges_y | mass[kWaves][kRows][n_cells] | count[kWaves][n_cells]].
template <int kRows>
__global__ void __launch_bounds__(kThreads) k_mbar_hist2d(const double *__restrict__ energies, const double *__restrict__ d,
                                                          const double *__restrict__ values_x, const double *__restrict__ values_y,
                                                          long long n_chains, long long record_stride,
                                                          const double *__restrict__ edges, int n_bins_x, int n_bins_y, int top_x,
                                                          int top_y, const double *__restrict__ inv_temps,
                                                          const double *__restrict__ ln_z, int n_targets, int with_counts,
                                                          long long n_tiles, double *partials, unsigned long long *count_partials) {
  extern __shared__ double lds[];
  const int n_edges_x = n_bins_x + 1, n_edges_y = n_bins_y + 1, n_slots_y = n_bins_y + 3, n_cells = (n_bins_x + 3) * n_slots_y;
  double *s_edges_x = lds, *s_edges_y = lds + n_edges_x, *s_mass = s_edges_y + n_edges_y;
  unsigned int *s_count = reinterpret_cast<unsigned int *>(s_mass + kWaves * kRows * n_cells);
  for (int i = threadIdx.x; i < n_edges_x + n_edges_y; i += kThreads) lds[i] = edges[i];
  for (int i = threadIdx.x; i < kWaves * kRows * n_cells; i += kThreads) s_mass[i] = 0.0;
  for (int i = threadIdx.x; i < kWaves * n_cells; i += kThreads) s_count[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double *my_mass = s_mass + wave * kRows * n_cells;
  unsigned int *my_count = s_count + wave * n_cells;
  const unsigned long long below_me = (1ull << lane) - 1ull;
  double inv[kRows], lz[kRows];
#pragma unroll
  for (int t = 0; t < kRows; ++t) {
    inv[t] = t < n_targets ? inv_temps[t] : 0.0;
    lz[t] = t < n_targets ? ln_z[4 * t] : 0.0;
  }
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long base = tile * kTile + threadIdx.x;
    long long record = base / n_chains, chain = base - record * n_chains;
#pragma unroll 1
    for (int r = 0; r < kItems; ++r) {
      const long long i = base + (long long)r * kThreads;
      const double dn = d[i];                   // (padded: in bounds; NaN beyond n and for an unused sample)
      int cell = -1;
      double w[kRows];
#pragma unroll
      for (int t = 0; t < kRows; ++t) w[t] = 0.0;
      if (dn == dn) {
        const double e = energies[i];
        const long long at = record * record_stride + chain;
        const double a = values_x ? values_x[at] : e, b = values_y ? values_y[at] : e;
        cell = slot_of(s_edges_x, n_edges_x, top_x, a) * n_slots_y + slot_of(s_edges_y, n_edges_y, top_y, b);
#pragma unroll
        for (int t = 0; t < kRows; ++t)
          if (t < n_targets) w[t] = math64::exp_nonpos(fmin(__builtin_fma(-e, inv[t], -dn) - lz[t], 0.0));
      }
      chain += kThreads;
      while (chain >= n_chains) {
        chain -= n_chains;
        record += 1;
      }
      if (with_counts && cell >= 0) atomicAdd(&my_count[cell], 1u);       // (integers: exact in any order)
      // every lane is active from here on (me_mbar_slots.h)
      slot_accumulate<kRows>(my_mass, n_cells, n_targets, cell, w, lane, below_me);
    }
  }
  __syncthreads();
  slot_tables_store(s_mass, kRows, n_targets, n_cells, partials);
  if (!with_counts) return;
  for (int c = threadIdx.x; c < n_cells; c += kThreads) {
    unsigned long long sum = 0;
    for (int k = 0; k < kWaves; ++k) sum += s_count[k * n_cells + c];
    count_partials[(size_t)blockIdx.x * n_cells + c] = sum;
  }
}

// A joint histogram request: the edges of both axes and the host outputs mass[n_temps][Bx + 3][By + 3], counts[Bx + 3][By + 3],
// neff[n_temps] (each may be nullptr)
struct Histogram2d {
  const double *edges_x;
  int n_bins_x;
  const double *edges_y;
  int n_bins_y;
  double *mass;
  int64_t *counts;
  double *neff;
};

// The two value columns that go with the problem's samples: x and y share n_chains and record_stride; nullptr = the energy
struct ValuePair {
  const double *x, *y;
  long long n_chains, record_stride;
};

struct PassArgs {
  const MbarSamples *sm;
  const ValuePair *values;
  const double *d, *edges, *inv_temps, *ln_z;
  int n_bins_x, n_bins_y, top_x, top_y, n_targets, with_counts, n_blocks;
  long long n_tiles;
  double *partials;
  unsigned long long *count_partials;
};

template <int kRows>
void launch_pass(const PassArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(k_mbar_hist2d<kRows>, dim3(a.n_blocks), dim3(kThreads), lds_bytes(kRows, a.n_bins_x, a.n_bins_y), stream,
                     a.sm->energies, a.d, a.values->x, a.values->y, a.values->n_chains, a.values->record_stride, a.edges, a.n_bins_x,
                     a.n_bins_y, a.top_x, a.top_y, a.inv_temps, a.ln_z, a.n_targets, a.with_counts, a.n_tiles, a.partials,
                     a.count_partials);
}

int top_of(int n_edges) {                       // `top` of slot_of
  int top = 1;
  while (2 * top <= n_edges) top *= 2;
  return top;
}

// Prepares `p`, reweights to temps[0 .. n_temps), fills the joint histogram and waits for the stream.  With an empty rung
// nothing else is computed.
hipError_t histogram2d(Problem &p, const Source &src, const ValuePair &values, const double *f, const double *temps, int n_temps,
                       const Histogram2d &h) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const int n_edges_x = h.n_bins_x + 1, n_edges_y = h.n_bins_y + 1, n_cells = (h.n_bins_x + 3) * (h.n_bins_y + 3);
  const int n_blocks = blocks_of(p.sm.n_samples), rows = rows_per_pass(n_cells);
  std::vector<double> inv, edges_host(h.edges_x, h.edges_x + n_edges_x);
  edges_host.insert(edges_host.end(), h.edges_y, h.edges_y + n_edges_y);
  DeviceBuffer d, edges, partials, count_partials, mass, counts;
  ME_MBAR_HIP(reweight_enqueue(p, p.sm, temps, n_temps, inv));      // ln_z and neff_fraction of every target into w.out
  ME_MBAR_HIP(log_denominator_enqueue(p, p.sm, d));
  ME_MBAR_HIP(edges.resize(edges_host.size() * sizeof(double)));
  ME_MBAR_HIP(partials.resize((size_t)n_blocks * rows * n_cells * sizeof(double)));
  ME_MBAR_HIP(count_partials.resize((size_t)n_blocks * n_cells * sizeof(unsigned long long)));
  ME_MBAR_HIP(mass.resize((size_t)n_temps * n_cells * sizeof(double)));
  ME_MBAR_HIP(counts.resize((size_t)n_cells * sizeof(long long)));
  ME_MBAR_HIP(hipMemcpyAsync(edges.get(), edges_host.data(), edges.bytes(), hipMemcpyHostToDevice, p.stream));
  PassArgs a{&p.sm, &values, d.get<const double>(), edges.get<const double>(), nullptr, nullptr, h.n_bins_x, h.n_bins_y,
             top_of(n_edges_x), top_of(n_edges_y), 0, 0, n_blocks, tiles_of(p.sm.n_samples), partials.get<double>(),
             count_partials.get<unsigned long long>()};
  for (int t0 = 0; t0 < n_temps; t0 += rows) {
    double *sums = mass.get<double>() + (size_t)t0 * n_cells;
    a.inv_temps = w.inv_temps.get<const double>() + t0;
    a.ln_z = w.out.get<const double>() + 4 * (size_t)t0;
    a.n_targets = std::min(rows, n_temps - t0);
    a.with_counts = t0 == 0;
    if (rows == 4) launch_pass<4>(a, p.stream);
    else if (rows == 2) launch_pass<2>(a, p.stream);
    else launch_pass<1>(a, p.stream);
    hipLaunchKernelGGL(k_mbar_hist_sum, dim3(n_cells, a.n_targets), dim3(kThreads), 0, p.stream, partials.get<const double>(),
                       count_partials.get<const unsigned long long>(), n_blocks, rows, n_cells, sums,
                       t0 == 0 ? counts.get<long long>() : nullptr);
    hipLaunchKernelGGL(k_mbar_hist_normalise, dim3(a.n_targets), dim3(kThreads), 0, p.stream, n_cells, sums);
  }
  ME_MBAR_HIP(hipGetLastError());
  std::vector<double> out(4 * (size_t)n_temps), mass_host((size_t)n_temps * n_cells);
  std::vector<long long> counts_host((size_t)n_cells);
  ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipMemcpyAsync(mass_host.data(), mass.get(), mass.bytes(), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipMemcpyAsync(counts_host.data(), counts.get(), counts.bytes(), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipStreamSynchronize(p.stream));    // (also: `inv`, the edges and the scratch buffers leave scope)
  unpack_targets(out, n_temps, nullptr, nullptr, nullptr, h.neff);
  if (h.mass) std::copy(mass_host.begin(), mass_host.end(), h.mass);
  if (h.counts) std::copy(counts_host.begin(), counts_host.end(), h.counts);
  return hipSuccess;
}

// the two forms of me_mbar_histogram_joint behind their Source
int histogram2d_common(const Source &src, const ValuePair &values, const double *f, const double *temps, int n, const Histogram2d &h) {
  int rc = check_edges(src.e, h.edges_x, h.n_bins_x);
  if (rc) return rc;
  rc = check_edges(src.e, h.edges_y, h.n_bins_y);
  if (rc) return rc;
  if ((h.n_bins_x + 3) * (h.n_bins_y + 3) > ME_MAX_HISTOGRAM2D_SLOTS)
    return fail(src.e, ME_ERR_INVALID, "(n_bins_x + 3) (n_bins_y + 3) must not exceed " + std::to_string(ME_MAX_HISTOGRAM2D_SLOTS));
  rc = check_f_and_targets(src.e, f, src.n_rungs, temps, n, 1);
  if (rc) return rc;
  Problem p;
  return mbar_check_common(src.e, p, histogram2d(p, src, values, f, temps, n, h));
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
  ObsColumns x{}, y{};
  rc = histogram_column(src, column_x, x);
  if (rc) return rc;
  rc = histogram_column(src, column_y, y);
  if (rc) return rc;
  // recorded columns share the store's strides; the energy is read as the energy (nullptr), whatever the other axis is
  const ObsColumns &strides = column_x >= 0 ? x : y;
  const ValuePair values{column_x >= 0 ? x.data : nullptr, column_y >= 0 ? y.data : nullptr, strides.n_chains, strides.record_stride};
  return histogram2d_common(src, values, f, temps, n, Histogram2d{edges_x, n_bins_x, edges_y, n_bins_y, mass, counts, neff_fraction});
}

int me_mbar_histogram_joint_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                                const double *values_x, const double *values_y, const double *edges_x, int32_t n_bins_x,
                                const double *edges_y, int32_t n_bins_y, double *mass, int64_t *counts, double *neff_fraction) {
  if (!values_x || !values_y) return fail(nullptr, ME_ERR_INVALID, "null pointer");
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs);
  if (rc) return rc;
  const size_t column_bytes = sizeof(double) * (size_t)n_samples;
  ME_HIP(nullptr, src.columns_dev.resize(2 * column_bytes));
  double *columns = src.columns_dev.get<double>();
  ME_HIP(nullptr, hipMemcpy(columns, values_x, column_bytes, hipMemcpyHostToDevice));
  ME_HIP(nullptr, hipMemcpy(columns + n_samples, values_y, column_bytes, hipMemcpyHostToDevice));
  const ValuePair values{columns, columns + n_samples, n_samples, 0};
  return src.finish(
      histogram2d_common(src, values, f, temps, n, Histogram2d{edges_x, n_bins_x, edges_y, n_bins_y, mass, counts, neff_fraction}));
}

}  // extern "C"
