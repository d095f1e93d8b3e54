// Reweighted histograms of a ladder's samples along one observable (me_mbar_histogram and its engine-less twin in the public
// header): the distribution p(A; T) at any temperature, from which the free-energy profile F(A; T) = -T ln p(A; T) follows.
// Also the host driver that the three histogram units share (histogram_slots).
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
//   k_mbar_hist          slot_pass (me_mbar_slots.h, which describes the scheme and the summation order) with Slots1d and
//                        TemperatureRows<kHistTargets = 4>: one pass per chunk of 4 temperatures reads E_n, d_n, A_n (24 bytes
//                        per sample), ONE exponential per (sample, temperature).  It counts in every pass (the kernel has no
//                        switch; k_mbar_hist_sum reads the counts of the first chunk only).
//   k_mbar_hist_sum      block (slot, t): the block partials of one cell in a fixed order; the integer counts.
//   k_mbar_hist_normalise  block t: the total over the slots in a fixed order, then the division.
// Registers and LDS (hipcc -O3, gfx950): see profiles/mbar_profile.txt and profiles/mbar_slot_skeleton.txt; no kernel uses
// scratch.  LDS per workgroup: (n_bins + 1) 8 + 4 (n_bins + 3)(4 x 8 + 4) bytes, 39 352 at 256 bins.
#include "me_mbar_slots.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {
namespace {

constexpr int kHistTargets = 4;                 // temperatures per pass
static_assert(slot_pass_lds(kHistTargets, 256 + 3, 256 + 1, true) == 39352, "the LDS of the header comment");

// values: the one value column (slot_pass); ln_z has stride 4 (reweight_enqueue's out)
__global__ void __launch_bounds__(kThreads) k_mbar_hist(const double *__restrict__ energies, const double *__restrict__ d,
                                                        const double *__restrict__ values, long long n_chains,
                                                        long long record_stride, const double *__restrict__ edges, int n_bins,
                                                        int top, const double *__restrict__ inv_temps,
                                                        const double *__restrict__ ln_z, int n_targets, long long n_tiles,
                                                        double *partials, unsigned long long *count_partials) {
  const Slots1d where{values, n_bins, top};
  const TemperatureRows<kHistTargets> rows(inv_temps, ln_z, n_targets);
  slot_pass<kHistTargets, true>(energies, d, n_chains, record_stride, edges, where, rows, 1, n_tiles, partials, count_partials);
}

}  // namespace

hipError_t histogram_slots(Problem &p, const Source &src, const double *f, const double *temps, int n_temps, const SlotTable &table,
                           HistogramScratch &keep) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const int n_slots = table.n_slots, rows = table.rows, n_blocks = blocks_of(p.sm.n_samples);
  std::vector<double> inv;
  DeviceBuffer partials, count_partials, mass, counts;
  ME_MBAR_HIP(reweight_enqueue(p, p.sm, temps, n_temps, inv));      // ln_z and neff_fraction of every target into w.out
  ME_MBAR_HIP(log_denominator_enqueue(p, p.sm, keep.d));
  ME_MBAR_HIP(keep.edges.resize((size_t)table.n_edges * sizeof(double)));
  ME_MBAR_HIP(partials.resize((size_t)n_blocks * rows * n_slots * sizeof(double)));
  ME_MBAR_HIP(count_partials.resize((size_t)n_blocks * n_slots * sizeof(unsigned long long)));
  ME_MBAR_HIP(mass.resize((size_t)n_temps * n_slots * sizeof(double)));
  ME_MBAR_HIP(counts.resize((size_t)n_slots * sizeof(long long)));
  ME_MBAR_HIP(hipMemcpyAsync(keep.edges.get(), table.edges, keep.edges.bytes(), hipMemcpyHostToDevice, p.stream));
  for (int t0 = 0; t0 < n_temps; t0 += rows) {
    const int nt = std::min(rows, n_temps - t0);
    double *sums = mass.get<double>() + (size_t)t0 * n_slots;
    table.launch(t0, nt, partials.get<double>(), count_partials.get<unsigned long long>());
    hipLaunchKernelGGL(k_mbar_hist_sum, dim3(n_slots, nt), dim3(kThreads), 0, p.stream, partials.get<const double>(),
                       count_partials.get<const unsigned long long>(), n_blocks, rows, n_slots, sums,
                       t0 == 0 ? counts.get<long long>() : nullptr);
    hipLaunchKernelGGL(k_mbar_hist_normalise, dim3(nt), dim3(kThreads), 0, p.stream, n_slots, sums);
  }
  ME_MBAR_HIP(hipGetLastError());
  std::vector<double> out(4 * (size_t)n_temps), mass_host((size_t)n_temps * n_slots);
  std::vector<long long> counts_host((size_t)n_slots);
  ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipMemcpyAsync(mass_host.data(), mass.get(), mass.bytes(), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipMemcpyAsync(counts_host.data(), counts.get(), counts.bytes(), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipStreamSynchronize(p.stream));    // (also: `inv`, the host edges and the scratch buffers but `keep` leave scope)
  unpack_targets(out, n_temps, nullptr, nullptr, nullptr, table.neff);
  if (table.mass) std::copy(mass_host.begin(), mass_host.end(), table.mass);
  if (table.counts) std::copy(counts_host.begin(), counts_host.end(), table.counts);
  return hipSuccess;
}

// `values`: one column (n_columns = 1) that goes with the problem's samples
hipError_t histogram(Problem &p, const Source &src, const ObsColumns &values, const double *f, const double *temps, int n_temps,
                     const Histogram &h, HistogramScratch &keep) {
  const int n_edges = h.n_bins + 1, n_slots = h.n_bins + 3;
  keep.top = top_of(n_edges);
  const size_t lds = slot_pass_lds(kHistTargets, n_slots, n_edges, true);
  const auto launch = [&](int t0, int nt, double *partials, unsigned long long *count_partials) {     // (counts in every pass)
    hipLaunchKernelGGL(k_mbar_hist, dim3(blocks_of(p.sm.n_samples)), dim3(kThreads), lds, p.stream, p.sm.energies,
                       keep.d.get<const double>(), values.data, values.n_chains, values.record_stride,
                       keep.edges.get<const double>(), h.n_bins, keep.top, p.w.inv_temps.get<const double>() + t0,
                       p.w.out.get<const double>() + 4 * (size_t)t0, nt, tiles_of(p.sm.n_samples), partials, count_partials);
  };
  return histogram_slots(p, src, f, temps, n_temps,
                         SlotTable{h.edges, n_edges, n_slots, kHistTargets, h.mass, h.counts, h.neff, launch}, keep);
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
