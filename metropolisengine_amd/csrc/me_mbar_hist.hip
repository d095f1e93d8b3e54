// Reweighted histograms of a ladder's samples along one observable (me_mbar_histogram and its engine-less twin in the public
// header): the distribution p(A; T) at any temperature, from which the free-energy profile F(A; T) = -T ln p(A; T) follows.
//
// Definition.  With the weights of me_mbar_reweight (me_mbar.hip: d_n = m_n + ln s_n, l_nt = -E_n / T_t - d_n; a sample is USED
// when its ENERGY is finite) every used sample falls into exactly one of n_bins + 3 slots by its value A_n and the n_bins + 1
// edges (finite, strictly increasing, any spacing):
//     bin b < n_bins        edges[b] <= A_n < edges[b + 1]            (half-open everywhere)
//     below = n_bins        A_n < edges[0], -inf included
//     above = n_bins + 1    A_n >= edges[n_bins], +inf included       (a value ON the last edge is above)
//     nan   = n_bins + 2    A_n is not a number
// i.e. searchsorted(edges, A, side = "right") - 1, and
//     mass[t][slot] = sum_{n in slot} w_nt / sum_n w_nt,   w_nt = exp(min(l_nt - ln_z_t, 0)),   counts[slot] = #{n in slot}.
// ln_z_t is me_mbar_reweight's (reweight_enqueue runs first, which also gives neff_fraction): ln_z_t = M + ln sum exp(l - M) is
// at least the largest l_nt up to rounding, so every exponent is <= 0 after the clamp and the weights already sum to 1 up to
// rounding; the division by the total over ALL slots makes the masses sum to 1 by construction.
//
// Kernels.  d_n comes from me_mbar_obs.hip's scratch pass (log_denominator_enqueue: 8 bytes per sample, NaN when unused).
//   k_mbar_hist          one pass per chunk of kHistTargets = 4 temperatures: reads E_n, d_n, A_n (24 bytes per sample), ONE
//                        exponential per (sample, temperature).  The edges sit in LDS; a lane finds its slot by a branch-free
//                        binary search (at most 9 steps for 257 edges).  Each wavefront owns a private LDS table
//                        [4][n_bins + 3] of doubles and [n_bins + 3] counts; nothing is shared between wavefronts before the
//                        end, and NO atomic touches a floating-point number.
//   k_mbar_hist_sum      block (slot, t): the block partials of one cell in a fixed order; the integer counts.
//   k_mbar_hist_normalise  block t: the total over the slots in a fixed order, then the division.
// (slot_of, steps 1 to 3 below as slot_accumulate, k_mbar_hist_sum and k_mbar_hist_normalise live in me_mbar_slots.h:
// me_mbar_hist_cov.hip and me_mbar_hist2d.hip fill their tables by the same code.)
// How a wavefront adds the 64 weights of one item of the tile into its table, all lanes active throughout (the loop condition
// is a ballot, wave-uniform; no cross-lane operation ever runs under a partial lane mask):
//   0. every lane adds 1 to its slot's count with an integer LDS atomic (integers: exact in any order);
//   1. the groups of lanes that share a slot are found one by one: the lowest lane not yet matched names the slot (readlane
//      with a wave-uniform lane number), a ballot gives the group and its popcount the group's size;
//   2. a group of more than kDense = 8 lanes is summed at once: wave_sum over the wavefront with +0.0 from the other lanes
//      (exact), lane 0 adds the four sums to the table.  At most 7 such groups exist among 64 lanes;
//   3. a lane of a smaller group keeps its rank r inside the group (popcount of the group's lower lanes).  After the match loop
//      round r = 1 .. (largest such group) lets the lanes of rank r add their own weights to the table themselves: they all
//      hold DIFFERENT slots, so the plain read-add-write of a round touches every address at most once.
// The worst cases are bounded: 64 lanes in one bin cost one match round and four wave_sums; 64 lanes in 64 bins cost 64 match
// rounds (readlane, compare, ballot, popcount, two selects) and ONE round of step 3, not 64 x 4 wave_sums.  Measured at 2^25
// samples, 8 temperatures, 64 bins (profiles/mbar_profile.txt): 3.2 ms with every value in one bin and 4.2 ms with 64
// different bins per wavefront; summing EVERY group by wave_sum (kDense = 0) takes 3.3 and 40.3 ms, letting every lane add for
// itself (kDense = 64) 7.2 and 3.6 ms.
// Summation order, fixed by the samples' values and order alone: per item the large groups in order of their lowest lane, then
// the small groups' lanes by rank (lane order inside a group); the items and tiles of a block in order; the block's wavefront
// tables in wavefront order -> partials[block][t][slot] -> k_mbar_hist_sum, in which lane l adds blocks l, l + 256, ... in
// order, then the butterfly and the wavefronts in order.  Neither the slots nor the order depend on the temperature, and a
// temperature's weights are formed by the same instructions at every position of a chunk (`fp contract(off)`, the fused
// multiply-add spelled out): mass[t][slot] is bit for bit the same run to run, alone or among any number of temperatures, and
// through the engine's store or host arrays of the same samples in the same order (the values are addressed through strides).
// Registers and LDS (hipcc -O3, gfx950): see profiles/mbar_profile.txt; no kernel uses scratch.  LDS per workgroup: (n_bins +
// 1) 8 + 4 (n_bins + 3)(4 x 8 + 4) bytes, 39 352 at 256 bins.
#include "me_mbar_slots.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {
namespace {

constexpr int kHistTargets = 4;                 // temperatures per pass

// values: sample i = record * n_chains + chain sits at values[record * record_stride + chain] (a column of the engine's store:
// n_chains, Q n_chains; a host array or the energies themselves: n, 0).  `d` is padded to whole tiles.  ln_z has stride 4
// (reweight_enqueue's out).  Dynamic LDS: [edges | mass[kWaves][kHistTargets][n_slots] | count[kWaves][n_slots]].
__global__ void __launch_bounds__(kThreads) k_mbar_hist(const double *__restrict__ energies, const double *__restrict__ d,
                                                        const double *__restrict__ values, long long n_chains,
                                                        long long record_stride, const double *__restrict__ edges, int n_bins,
                                                        int top, const double *__restrict__ inv_temps,
                                                        const double *__restrict__ ln_z, int n_targets, long long n_tiles,
                                                        double *partials, unsigned long long *count_partials) {
  extern __shared__ double lds[];
  const int n_edges = n_bins + 1, n_slots = n_bins + 3;
  double *s_edges = lds, *s_mass = lds + n_edges;
  unsigned int *s_count = reinterpret_cast<unsigned int *>(s_mass + kWaves * kHistTargets * n_slots);
  for (int i = threadIdx.x; i < n_edges; i += kThreads) s_edges[i] = edges[i];
  for (int i = threadIdx.x; i < kWaves * kHistTargets * n_slots; i += kThreads) s_mass[i] = 0.0;
  for (int i = threadIdx.x; i < kWaves * n_slots; i += kThreads) s_count[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double *my_mass = s_mass + wave * kHistTargets * n_slots;
  unsigned int *my_count = s_count + wave * n_slots;
  const unsigned long long below_me = (1ull << lane) - 1ull;
  double inv[kHistTargets], lz[kHistTargets];
#pragma unroll
  for (int t = 0; t < kHistTargets; ++t) {
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
      int slot = -1;
      double w[kHistTargets];
#pragma unroll
      for (int t = 0; t < kHistTargets; ++t) w[t] = 0.0;
      if (dn == dn) {
        const double e = energies[i];
        slot = slot_of(s_edges, n_edges, top, values[record * record_stride + chain]);
#pragma unroll
        for (int t = 0; t < kHistTargets; ++t)
          if (t < n_targets) w[t] = math64::exp_nonpos(fmin(__builtin_fma(-e, inv[t], -dn) - lz[t], 0.0));
      }
      chain += kThreads;
      while (chain >= n_chains) {
        chain -= n_chains;
        record += 1;
      }
      if (slot >= 0) atomicAdd(&my_count[slot], 1u);          // (integers: exact in any order)
      // every lane is active from here on (me_mbar_slots.h)
      slot_accumulate<kHistTargets>(my_mass, n_slots, n_targets, slot, w, lane, below_me);
    }
  }
  __syncthreads();
  slot_tables_store(s_mass, kHistTargets, n_targets, n_slots, partials);
  for (int c = threadIdx.x; c < n_slots; c += kThreads) {
    unsigned long long sum = 0;
    for (int k = 0; k < kWaves; ++k) sum += s_count[k * n_slots + c];
    count_partials[(size_t)blockIdx.x * n_slots + c] = sum;
  }
}

}  // namespace

// `values`: one column (n_columns = 1) that goes with the problem's samples
hipError_t histogram(Problem &p, const Source &src, const ObsColumns &values, const double *f, const double *temps, int n_temps,
                     const Histogram &h, HistogramScratch &keep) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const int n_edges = h.n_bins + 1, n_slots = h.n_bins + 3, n_blocks = blocks_of(p.sm.n_samples);
  const long long n_tiles = tiles_of(p.sm.n_samples);
  int top = 1;
  while (2 * top <= n_edges) top *= 2;
  keep.top = top;
  std::vector<double> inv;
  DeviceBuffer &d = keep.d, &edges = keep.edges;
  DeviceBuffer partials, count_partials, mass, counts;
  ME_MBAR_HIP(reweight_enqueue(p, p.sm, temps, n_temps, inv));      // ln_z and neff_fraction of every target into w.out
  ME_MBAR_HIP(log_denominator_enqueue(p, p.sm, d));
  ME_MBAR_HIP(edges.resize((size_t)n_edges * sizeof(double)));
  ME_MBAR_HIP(partials.resize((size_t)n_blocks * kHistTargets * n_slots * sizeof(double)));
  ME_MBAR_HIP(count_partials.resize((size_t)n_blocks * n_slots * sizeof(unsigned long long)));
  ME_MBAR_HIP(mass.resize((size_t)n_temps * n_slots * sizeof(double)));
  ME_MBAR_HIP(counts.resize((size_t)n_slots * sizeof(long long)));
  ME_MBAR_HIP(hipMemcpyAsync(edges.get(), h.edges, edges.bytes(), hipMemcpyHostToDevice, p.stream));
  const size_t lds = (size_t)n_edges * sizeof(double) + (size_t)kWaves * n_slots * (kHistTargets * sizeof(double) + sizeof(unsigned int));
  for (int t0 = 0; t0 < n_temps; t0 += kHistTargets) {
    const int nt = std::min(kHistTargets, n_temps - t0);
    double *sums = mass.get<double>() + (size_t)t0 * n_slots;
    hipLaunchKernelGGL(k_mbar_hist, dim3(n_blocks), dim3(kThreads), lds, p.stream, p.sm.energies, d.get<const double>(), values.data,
                       values.n_chains, values.record_stride, edges.get<const double>(), h.n_bins, top,
                       w.inv_temps.get<const double>() + t0, w.out.get<const double>() + 4 * (size_t)t0, nt, n_tiles,
                       partials.get<double>(), count_partials.get<unsigned long long>());
    hipLaunchKernelGGL(k_mbar_hist_sum, dim3(n_slots, nt), dim3(kThreads), 0, p.stream, partials.get<const double>(),
                       count_partials.get<const unsigned long long>(), n_blocks, kHistTargets, n_slots, sums,
                       t0 == 0 ? counts.get<long long>() : nullptr);
    hipLaunchKernelGGL(k_mbar_hist_normalise, dim3(nt), dim3(kThreads), 0, p.stream, n_slots, sums);
  }
  ME_MBAR_HIP(hipGetLastError());
  std::vector<double> out(4 * (size_t)n_temps), mass_host((size_t)n_temps * n_slots);
  std::vector<long long> counts_host((size_t)n_slots);
  ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipMemcpyAsync(mass_host.data(), mass.get(), mass.bytes(), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipMemcpyAsync(counts_host.data(), counts.get(), counts.bytes(), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipStreamSynchronize(p.stream));    // (also: `inv` and the scratch buffers but `keep` leave scope)
  unpack_targets(out, n_temps, nullptr, nullptr, nullptr, h.neff);
  if (h.mass) std::copy(mass_host.begin(), mass_host.end(), h.mass);
  if (h.counts) std::copy(counts_host.begin(), counts_host.end(), h.counts);
  return hipSuccess;
}

int check_edges(me_engine *e, const double *edges, int n_bins) {
  if (n_bins < 1 || n_bins > ME_MAX_HISTOGRAM_BINS)
    return fail(e, ME_ERR_INVALID, "n_bins must lie in [1, " + std::to_string(ME_MAX_HISTOGRAM_BINS) + "]");
  if (!edges) return fail(e, ME_ERR_INVALID, "edges missing");
  for (int b = 0; b <= n_bins; ++b)
    if (!std::isfinite(edges[b]) || (b > 0 && !(edges[b] > edges[b - 1])))
      return fail(e, ME_ERR_INVALID, "edges must be finite and strictly increasing");
  return ME_OK;
}

// column >= 0: that recorded column of an engine's store; -1: the energies themselves
int histogram_column(const Source &src, int column, ObsColumns &values) {
  me_engine *e = src.e;
  values = ObsColumns{src.sm.energies, 1, src.sm.n_samples, 0, src.sm.n_samples};
  if (column >= 0) {
    if (src.columns.n_columns == 0)
      return fail(e, ME_ERR_STATE, "no recorded observables: me_observable_samples_enable, then me_energy_samples_record");
    if (column >= src.columns.n_columns)
      return fail(e, ME_ERR_INVALID, "column " + std::to_string(column) + " outside the " + std::to_string(src.columns.n_columns) +
                                         " recorded columns");
    values = ObsColumns{src.columns.data + (size_t)column * (size_t)src.columns.column_stride, 1, src.columns.n_chains,
                        src.columns.record_stride, src.columns.column_stride};
  } else if (column != -1) {
    return fail(e, ME_ERR_INVALID, "column must be a recorded column or -1 (the energy)");
  }
  return ME_OK;
}

namespace {

// the two forms of me_mbar_histogram behind their Source
int histogram_common(const Source &src, const ObsColumns &values, const double *f, const double *temps, int n, const Histogram &h) {
  int rc = check_edges(src.e, h.edges, h.n_bins);
  if (rc) return rc;
  rc = check_f_and_targets(src.e, f, src.n_rungs, temps, n, 1);
  if (rc) return rc;
  Problem p;
  HistogramScratch keep;
  return mbar_check_common(src.e, p, histogram(p, src, values, f, temps, n, h, keep));
}

}  // namespace
}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_mbar_histogram(me_engine *e, const double *f, const double *temps, int32_t n, int32_t column, const double *edges,
                      int32_t n_bins, double *mass, int64_t *counts, double *neff_fraction) {
  Source src;
  int rc = src.from_engine(e);
  if (rc) return rc;
  ObsColumns values{};
  rc = histogram_column(src, column, values);
  if (rc) return rc;
  return histogram_common(src, values, f, temps, n, Histogram{edges, n_bins, mass, counts, neff_fraction});
}

int me_mbar_histogram_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                              const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                              const double *values, const double *edges, int32_t n_bins, double *mass, int64_t *counts,
                              double *neff_fraction) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs, values, 1);
  return rc ? rc : src.finish(histogram_common(src, src.columns, f, temps, n, Histogram{edges, n_bins, mass, counts, neff_fraction}));
}

}  // extern "C"
