// Statistical inefficiencies of the recorded series, pooled over the chains of a rung (include/metropolis_engine.h has the
// formulas): the number every MBAR error bar of this library asks for as `inefficiency`.  The stores stay on the device.
//
//   k_series_sums    pass 1: one lane owns one chain; it adds the R records of one column (less the pivot, see pivot_of) in record
//                    order and tests them for finiteness.  A chain is used for a column when all of them are finite: bit `column` of used_mask[chain]
//                    (integer or: the order does not matter).  wave_sum gives one partial and one count per wavefront.
//   k_series_means   one thread per (column, rung) adds the wavefront partials of the rung in wavefront order: the mean and M_u.
//   k_series_lags    pass 2, the hot kernel: grid (wavefronts of chains) x (lag tiles) x (columns).  A lane walks its chain's
//                    records once and forms sum_n d[n] d[n + t] for the kLagTile lags of its tile, then wave_sum: per-wavefront
//                    partials [column][wavefront][lag of the batch].
//   k_series_reduce  one thread per (column, rung, lag) adds them in wavefront order.
// A rung is a run of whole wavefronts (M is a multiple of 64), so a wavefront never straddles rungs, while a block of four
// does: partials are per wavefront.  No floating-point atomics; the order of every sum depends on (R, M) alone: a lane adds in
// record order, the butterfly adds the lanes, one thread adds the wavefronts of a rung in wavefront order.  The sum of one lag
// does not depend on the tile or the batch it was computed in.
//
// The host side of the entry point asks for the lags in batches of kBatch, copies the (1 + Q) K kBatch sums back and walks the
// stop rule of every (column, rung); it ends with the batch in which the last walk stops.
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "me_engine.h"
#include "me_mbar.h"
#include "me_wave.h"

#ifndef ME_SERIES_LAG_TILE
#define ME_SERIES_LAG_TILE 16     // experiments: 32 halves the passes over the records for 64 more VGPRs
#endif

namespace me {
namespace series {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLagTile = ME_SERIES_LAG_TILE;
constexpr int kBatch = 64;                       // lags per round trip to the host
static_assert(kBatch % kLagTile == 0, "a batch is whole tiles");

// The columns of one call: column 0 is energy[record][chain]; column 1 + q is column q of `obs` (me_mbar.h).
struct Columns {
  const double *energy;
  mbar::ObsColumns obs;
  long long n_chains;
};
// the values of `column`, record r of chain c at base[r * stride + c]
__device__ __forceinline__ const double *column_base(const Columns &cols, int column, long long &stride) {
  if (column == 0) {
    stride = cols.n_chains;
    return cols.energy;
  }
  stride = cols.obs.record_stride;
  return cols.obs.data + (long long)(column - 1) * cols.obs.column_stride;
}

// The pivot of a (column, rung): the first record of the rung's first chain, 0 when that is not finite.  Every value is taken
// relative to it before anything is added, so that a large common offset (energies of -1e6 +- 1) costs the centred values no
// digits: the mean is kept as the pair (pivot, mean - pivot), and d = (a - pivot) - (mean - pivot).
__device__ __forceinline__ double pivot_of(const double *column, long long first_chain) {
  const double v = column[first_chain];
  return isfinite(v) ? v : 0.0;
}

__global__ void __launch_bounds__(kThreads) k_series_sums(Columns cols, long long n_records, long long n_waves, long long rung_chains,
                                                          unsigned int *used_mask, double *wave_sums, unsigned int *wave_used) {
  const int column = blockIdx.y;
  const long long c = (long long)blockIdx.x * kThreads + threadIdx.x, wave = c >> 6;
  if (wave >= n_waves) return;                                            // (wave-uniform)
  const bool live = c < cols.n_chains;
  long long stride;
  const double *base = column_base(cols, column, stride), *a = base + (live ? c : 0);
  const double pivot = pivot_of(base, (live ? c : 0) / rung_chains * rung_chains);
  double sum = 0.0;
  bool finite = true;
  long long r = 0;
  for (; r + 8 <= n_records; r += 8) {                                    // eight loads in flight, added in record order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = a[(r + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      sum = sum + (v[u] - pivot);
      finite = finite && isfinite(v[u]);
    }
  }
  for (; r < n_records; ++r) {
    const double v = a[r * stride];
    sum = sum + (v - pivot);
    finite = finite && isfinite(v);
  }
  const bool used = live && finite;
  if (used) atomicOr(used_mask + c, 1u << column);
  const double total = wave_sum(used ? sum : 0.0);
  const unsigned int count = (unsigned int)__popcll(__ballot(used));
  if ((threadIdx.x & 63) == 0) {
    wave_sums[(long long)column * n_waves + wave] = total;
    wave_used[(long long)column * n_waves + wave] = count;
  }
}

// rung k of the K rungs is the wavefronts [k waves_per_rung, (k + 1) waves_per_rung)
// centre[task] = (pivot, mean - pivot, mean)
__global__ void __launch_bounds__(kThreads) k_series_means(Columns cols, const double *wave_sums, const unsigned int *wave_used,
                                                           long long n_waves, long long waves_per_rung, long long rung_chains,
                                                           int n_columns, int n_rungs, long long n_records, double *centre,
                                                           long long *chains_used) {
  const int task = blockIdx.x * kThreads + threadIdx.x;
  if (task >= n_columns * n_rungs) return;
  const int column = task / n_rungs, rung = task - column * n_rungs;
  const long long first = (long long)column * n_waves + (long long)rung * waves_per_rung;
  double sum = 0.0;
  long long used = 0;
  for (long long w = 0; w < waves_per_rung; ++w) {
    sum = sum + wave_sums[first + w];
    used += wave_used[first + w];
  }
  long long stride;
  const double pivot = pivot_of(column_base(cols, column, stride), (long long)rung * rung_chains);
  const double delta = used ? sum / ((double)used * (double)n_records) : std::numeric_limits<double>::quiet_NaN();
  centre[3 * task] = pivot;
  centre[3 * task + 1] = delta;
  centre[3 * task + 2] = pivot + delta;
  chains_used[task] = used;
}

// kLagTile records of the walk, from record `base` (a multiple of L).  The ring `win` holds the centred values t0 records
// behind the walk: win[p] that of the last step m with m % L == p, so the value i steps back sits at the compile-time index (u -
// i) mod L after unrolling (a runtime-indexed ring would live in scratch memory).  FIRST: t0 == 0, where the ring takes the
// walk's own value.  GUARD: the last, partial block.
template <int L, bool FIRST, bool GUARD>
__device__ __forceinline__ void lag_block(const double *a, long long stride, bool used, double pivot, double delta, long long base, long long n_records,
                                          long long t0, double (&win)[L], double (&acc)[L]) {
#pragma unroll
  for (int u = 0; u < L; ++u) {
    const long long m = base + u;
    if (GUARD && m >= n_records) break;
    const double lead = used ? (a[m * stride] - pivot) - delta : 0.0;
    double trail = lead;
    if constexpr (!FIRST) {
      const long long back = m - t0;                                      // (uniform)
      const double v = a[(back >= 0 ? back : 0) * stride];
      trail = used && back >= 0 ? (v - pivot) - delta : 0.0;
    }
    win[u] = trail;
#pragma unroll
    for (int i = 0; i < L; ++i) acc[i] = __builtin_fma(win[(u - i + L) % L], lead, acc[i]);
  }
}

template <int L, bool FIRST>
__device__ __forceinline__ void lag_walk(const double *a, long long stride, bool used, double pivot, double delta, long long n_records, long long t0,
                                         double (&acc)[L]) {
  double win[L];
#pragma unroll
  for (int i = 0; i < L; ++i) win[i] = 0.0;
  long long base = 0;
  for (; base + L <= n_records; base += L) lag_block<L, FIRST, false>(a, stride, used, pivot, delta, base, n_records, t0, win, acc);
  if (base < n_records) lag_block<L, FIRST, true>(a, stride, used, pivot, delta, base, n_records, t0, win, acc);
}

// Lags lag_begin + L blockIdx.y + [0, L) of column blockIdx.z.  A pair (n, n + t) contributes at step m = n + t of the walk; lags
// beyond the series meet no pair and give exact zeros, and so does an unused chain.
template <int L>
__global__ void __launch_bounds__(kThreads) k_series_lags(Columns cols, long long n_records, long long n_waves, int n_rungs,
                                                          long long rung_chains, const unsigned int *used_mask, const double *centre,
                                                          int lag_begin, double *partials) {
  const int column = blockIdx.z;
  const long long c = (long long)blockIdx.x * kThreads + threadIdx.x, wave = c >> 6;
  if (wave >= n_waves) return;                                            // (wave-uniform)
  const bool live = c < cols.n_chains;
  const long long chain = live ? c : 0;
  const bool used = live && ((used_mask[chain] >> column) & 1u);
  const double *mine = centre + 3 * (column * n_rungs + (int)(chain / rung_chains));
  const double pivot = mine[0], delta = used ? mine[1] : 0.0;
  long long stride;
  const double *a = column_base(cols, column, stride) + chain;
  const long long t0 = (long long)lag_begin + (long long)blockIdx.y * L;
  double acc[L];
#pragma unroll
  for (int i = 0; i < L; ++i) acc[i] = 0.0;
  if (t0 == 0) lag_walk<L, true>(a, stride, used, pivot, delta, n_records, t0, acc);
  else lag_walk<L, false>(a, stride, used, pivot, delta, n_records, t0, acc);
  double *out = partials + ((long long)column * n_waves + wave) * kBatch + (long long)blockIdx.y * L;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const double s = wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) out[i] = s;
  }
}

// sums[(column, rung)][lag of the batch] = the wavefront partials of the rung, added in wavefront order
__global__ void __launch_bounds__(kThreads) k_series_reduce(const double *partials, long long n_waves, long long waves_per_rung,
                                                            int n_columns, int n_rungs, double *sums) {
  const int task = blockIdx.x * kThreads + threadIdx.x;
  if (task >= n_columns * n_rungs * kBatch) return;
  const int lag = task % kBatch, pair = task / kBatch;
  const int column = pair / n_rungs, rung = pair - column * n_rungs;
  const double *p = partials + ((long long)column * n_waves + (long long)rung * waves_per_rung) * kBatch + lag;
  double sum = 0.0;
  for (long long w = 0; w < waves_per_rung; ++w) sum = sum + p[w * kBatch];
  sums[task] = sum;
}

// host outputs of a call, each may be nullptr: [n_columns][n_rungs], acf [n_columns][n_rungs][max_lag + 1]
struct Outputs {
  double *g, *mean, *var;
  int32_t *stop_lag;
  int64_t *chains_used;
  double *acf;
};

// The whole computation for `cols` (device memory) on `stream`; waits for it.  n_rungs groups of rung_chains chains each:
// whole wavefronts, unless there is one group only.  The arguments have been checked.
int inefficiency(me_engine *e, hipStream_t stream, const Columns &cols, int n_columns, long long n_records, int n_rungs,
                 long long rung_chains, int mintime, int max_lag, const Outputs &out) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const long long n_waves = (cols.n_chains + 63) / 64, waves_per_rung = n_waves / n_rungs;
  const int n_pairs = n_columns * n_rungs;
  const long long blocks_x = (n_waves + kWaves - 1) / kWaves;
  if (blocks_x > 0x7fffffffLL) return fail(e, ME_ERR_INVALID, "too many chains for one launch");
  DeviceBuffer used_mask, wave_sums, wave_used, centre_dev, used_dev, partials, sums_dev;
  ME_HIP(e, used_mask.resize(sizeof(unsigned int) * (size_t)cols.n_chains));
  ME_HIP(e, wave_sums.resize(sizeof(double) * (size_t)n_columns * (size_t)n_waves));
  ME_HIP(e, wave_used.resize(sizeof(unsigned int) * (size_t)n_columns * (size_t)n_waves));
  ME_HIP(e, centre_dev.resize(sizeof(double) * 3 * (size_t)n_pairs));
  ME_HIP(e, used_dev.resize(sizeof(long long) * (size_t)n_pairs));
  ME_HIP(e, partials.resize(sizeof(double) * (size_t)n_columns * (size_t)n_waves * kBatch));
  ME_HIP(e, sums_dev.resize(sizeof(double) * (size_t)n_pairs * kBatch));
  ME_HIP(e, hipMemsetAsync(used_mask.get(), 0, used_mask.bytes(), stream));
  ME_HIP(e, hipMemsetAsync(partials.get(), 0, partials.bytes(), stream));   // (tiles beyond max_lag are not launched)

  hipLaunchKernelGGL(k_series_sums, dim3((unsigned)blocks_x, (unsigned)n_columns), dim3(kThreads), 0, stream, cols, n_records, n_waves,
                     rung_chains, used_mask.get<unsigned int>(), wave_sums.get<double>(), wave_used.get<unsigned int>());
  hipLaunchKernelGGL(k_series_means, dim3((unsigned)((n_pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, cols,
                     wave_sums.get<const double>(), wave_used.get<const unsigned int>(), n_waves, waves_per_rung, rung_chains, n_columns,
                     n_rungs, n_records, centre_dev.get<double>(), used_dev.get<long long>());
  ME_HIP(e, hipGetLastError());
  std::vector<double> centre(3 * (size_t)n_pairs), sums((size_t)n_pairs * kBatch);
  std::vector<long long> used((size_t)n_pairs);
  ME_HIP(e, hipMemcpyAsync(centre.data(), centre_dev.get(), centre_dev.bytes(), hipMemcpyDeviceToHost, stream));
  ME_HIP(e, hipMemcpyAsync(used.data(), used_dev.get(), used_dev.bytes(), hipMemcpyDeviceToHost, stream));

  // the walk of every (column, rung): statistics.statistical_inefficiency with fast=False on the pooled sums
  struct Walk {
    double p0 = 0.0, g = 1.0;
    int stop = 0;
    bool walking = false;
  };
  std::vector<Walk> walks((size_t)n_pairs);
  const size_t acf_row = (size_t)max_lag + 1;
  if (out.acf)
    for (size_t i = 0; i < (size_t)n_pairs * acf_row; ++i) out.acf[i] = nan;
  const double big_r = (double)n_records;
  int n_walking = n_pairs;
  for (int lag_begin = 0; lag_begin <= max_lag && n_walking > 0; lag_begin += kBatch) {
    const int lag_end = std::min(lag_begin + kBatch - 1, max_lag);      // (inclusive)
    const int tiles = (lag_end - lag_begin) / kLagTile + 1;
    hipLaunchKernelGGL((k_series_lags<kLagTile>), dim3((unsigned)blocks_x, (unsigned)tiles, (unsigned)n_columns), dim3(kThreads), 0,
                       stream, cols, n_records, n_waves, n_rungs, rung_chains, used_mask.get<const unsigned int>(),
                       centre_dev.get<const double>(), lag_begin, partials.get<double>());
    hipLaunchKernelGGL(k_series_reduce, dim3((unsigned)((n_pairs * kBatch + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                       partials.get<const double>(), n_waves, waves_per_rung, n_columns, n_rungs, sums_dev.get<double>());
    ME_HIP(e, hipGetLastError());
    ME_HIP(e, hipMemcpyAsync(sums.data(), sums_dev.get(), sums_dev.bytes(), hipMemcpyDeviceToHost, stream));
    ME_HIP(e, hipStreamSynchronize(stream));
    for (int i = 0; i < n_pairs; ++i) {
      Walk &w = walks[(size_t)i];
      const double *p = sums.data() + (size_t)i * kBatch;
      int t = lag_begin;
      if (lag_begin == 0) {
        w.p0 = p[0];
        w.walking = used[(size_t)i] > 0 && w.p0 > 0.0;                   // (a NaN fails the comparison too)
        if (!w.walking) --n_walking;
        else if (out.acf) out.acf[(size_t)i * acf_row] = 1.0;
        t = 1;
      }
      for (; w.walking && t <= lag_end; ++t) {
        const double c = p[t - lag_begin] * big_r / (w.p0 * (big_r - (double)t));
        if (out.acf) out.acf[(size_t)i * acf_row + (size_t)t] = c;
        if (c <= 0.0 && t > mintime) {
          w.stop = t;
          w.walking = false;
          --n_walking;
        } else {
          w.g += 2.0 * c * (1.0 - (double)t / big_r);
        }
      }
      if (w.walking && lag_end == max_lag) {
        w.stop = max_lag + 1;
        w.walking = false;
        --n_walking;
      }
    }
  }
  ME_HIP(e, hipStreamSynchronize(stream));
  for (int i = 0; i < n_pairs; ++i) {
    const Walk &w = walks[(size_t)i];
    const bool any = used[(size_t)i] > 0;
    if (out.g) out.g[i] = w.stop > 0 ? std::max(w.g, 1.0) : nan;
    if (out.mean) out.mean[i] = centre[3 * (size_t)i + 2];
    if (out.var) out.var[i] = any ? w.p0 / ((double)used[(size_t)i] * big_r) : nan;
    if (out.stop_lag) out.stop_lag[i] = w.stop;
    if (out.chains_used) out.chains_used[i] = used[(size_t)i];
  }
  return ME_OK;
}

// mintime >= 0 and max_lag in [1, R - 2] (0: R - 2), for R >= 3 records
int check_lags(me_engine *e, long long n_records, int mintime, int &max_lag) {
  if (mintime < 0) return fail(e, ME_ERR_INVALID, "mintime must be >= 0");
  if (max_lag == 0) max_lag = (int)std::min<long long>(n_records - 2, 0x7fffffbfLL);
  if (max_lag < 1 || max_lag > n_records - 2)
    return fail(e, ME_ERR_INVALID, "max_lag must lie in [1, records - 2 = " + std::to_string(n_records - 2) + "] (0: records - 2)");
  return ME_OK;
}

}  // namespace
}  // namespace series
}  // namespace me

using namespace me;
using namespace me::series;

extern "C" {

int me_recorded_inefficiency(me_engine *e, int32_t mintime, int32_t max_lag, double *g, double *mean, double *var, int32_t *stop_lag,
                             int64_t *chains_used, double *acf) {
  if (!e) return ME_ERR_INVALID;
  const me_engine::Samples &s = e->samples;
  if (!s.data) return fail(e, ME_ERR_STATE, "no recorded energy samples: me_energy_samples_enable, then me_energy_samples_record");
  if (s.rows < 3) return fail(e, ME_ERR_STATE, "a statistical inefficiency needs at least 3 records, the store holds " + std::to_string(s.rows));
  const int rc = check_lags(e, s.rows, mintime, max_lag);
  if (rc) return rc;
  // without a ladder the engine is one group at its scalar temperature (MBAR's front end, mbar::Source, refuses such engines)
  const int n_rungs = e->ladder.n_rungs > 0 ? e->ladder.n_rungs : 1;
  ME_HIP(e, hipSetDevice(e->device));
  const Columns cols{s.data.get<const double>(),
                     mbar::ObsColumns{s.obs.get<const double>(), s.n_obs, e->n, (long long)s.n_obs * e->n, e->n}, e->n};
  return inefficiency(e, e->stream, cols, 1 + s.n_obs, s.rows, n_rungs, e->n / n_rungs, mintime, max_lag,
                      Outputs{g, mean, var, stop_lag, chains_used, acf});
}

int me_series_inefficiency_samples(int32_t device_id, const double *series, int64_t n_records, int64_t n_series, int64_t group_chains,
                                   int32_t mintime, int32_t max_lag, double *g, double *mean, double *var, int32_t *stop_lag,
                                   int64_t *chains_used, double *acf) {
  if (!series) return fail(nullptr, ME_ERR_INVALID, "null pointer");
  if (n_records < 3 || n_series < 1) return fail(nullptr, ME_ERR_INVALID, "need n_records >= 3 and n_series >= 1");
  if (group_chains < 64 || group_chains % 64 != 0 || n_series % group_chains != 0)
    return fail(nullptr, ME_ERR_INVALID, "group_chains must be a multiple of 64 that divides n_series");
  if (n_series / group_chains > 0x7fffffLL) return fail(nullptr, ME_ERR_INVALID, "too many groups");
  const int rc = check_lags(nullptr, n_records, mintime, max_lag);
  if (rc) return rc;
  ME_HIP(nullptr, hipSetDevice(device_id));
  DeviceBuffer dev;
  ME_HIP(nullptr, dev.resize(sizeof(double) * (size_t)n_records * (size_t)n_series));
  ME_HIP(nullptr, hipMemcpy(dev.get(), series, dev.bytes(), hipMemcpyHostToDevice));
  const Columns cols{dev.get<const double>(), mbar::ObsColumns{nullptr, 0, n_series, 0, 0}, n_series};
  const int status = inefficiency(nullptr, nullptr, cols, 1, n_records, (int)(n_series / group_chains), group_chains, mintime, max_lag,
                                  Outputs{g, mean, var, stop_lag, chains_used, acf});
  (void)hipDeviceSynchronize();                   // (an error path may leave a launch in flight: the buffers go after it)
  return status;
}

}  // extern "C"
