// Energy samples of a temperature ladder, their MBAR free energies and temperature reweighting (me_energy_samples_record,
// me_mbar_solve, me_mbar_reweight and the engine-less twins in the public header).
//
// The multistate Bennett acceptance ratio (Shirts & Chodera, J. Chem. Phys. 129:124105, 2008) for states that differ by
// their temperature only: the reduced potential of sample n in state k is beta_k E_n, beta_k = 1 / T_k, so one number per
// sample is all there is.  A sample is USED when its energy is finite; N_k = the used samples of rung k; f starts at 0.
// One iteration, which tests/mbar_reference.py restates:
//     a_nj = (ln N_j + f_j) - beta_j E_n                      (all j; one fused multiply-add on the device)
//     m_n  = max_j a_nj,  e_nj = exp(a_nj - m_n),  s_n = sum_j e_nj     (j in rung order)
//     w_nk = e_nk / s_n                                       in (0, 1], sum_k w_nk = 1
//     S_k  = sum_n w_nk                                       (= N_k at the fixed point)
//     f_k <- f_k - ln(S_k / N_k);  then f <- f - f_0;  residual = max_k |change of f_k|
// until residual <= tolerance or max_iterations.  f_k = -ln Z(T_k) / Z(T_0).  Every weight is <= 1, so S_k is a plain sum;
// every exponential has an argument <= 0 (me_math64.h: exp_nonpos); the iteration takes no logarithm per sample.
//
// Reweighting to a temperature T from f: d_n = m_n + ln s_n, l_n = -E_n / T - d_n, M = max_n l_n, w_n = exp(l_n - M),
//     ln_z = M + ln sum w  (= ln Z(T) / Z(T_0); -f_k at T = T_k),   mean_e = sum w E / sum w,
//     var_e = sum w (E - mean_e)^2 / sum w,   neff_fraction = (sum w)^2 / (N sum w^2),  N = all used samples.
// M is not known in advance: every lane keeps (M, W = sum w, mean, M2 = sum w (E - mean)^2, Q = sum w^2) relative to its own
// running maximum and two such states merge by rescaling to the larger maximum (the weighted form of Chan's update for the
// mean and M2: no difference of large sums anywhere).
//
// Kernels.  k_mbar_weights: one lane per sample, each sample read once per iteration (8 bytes); a block walks tiles of
// kTile samples grid-stride.  The ladder table (beta_j, ln N_j + f_j) is read with wave-uniform indices from a const
// __restrict__ kernel argument: scalar loads into scalar registers, no per-lane loads.  Up to kChunk = 16 rungs the e_nj
// stay in registers between the sum and the division: ONE exponential per (sample, rung) and one division per sample, the
// per-lane partial S_k live in registers for the whole launch.  Beyond 16 rungs the rungs go in chunks of 16: m_n and
// 1 / s_n of the tile's samples are kept (in LDS), the e_nj are recomputed chunk by chunk (two exponentials per (sample, rung)) and
// the chunk's partials are reduced after every tile.  No kernel is instantiated per K.
// Summation order, fixed: per-lane partial -> butterfly in the wavefront -> the block's wavefronts in order -> the block's
// tiles in order -> partials[block][k] in global memory -> k_mbar_update adds them per rung (lane l takes the blocks l, l +
// 64, ... in order, then the same butterfly), updates f and the table, and raises `done` once residual <= tolerance: the
// launches of a batch that follow see it and return at once, so f stays the iterate that met the tolerance.  The host reads
// 16 bytes per batch of kBatch iterations; no per-sample data leaves the device and there are no floating-point atomics.
// k_mbar_count counts N_k (integer atomics); k_mbar_reweight / k_mbar_reweight_finish follow the same order for the merged
// states, kTargets temperatures per pass.
#include <algorithm>
#include <cmath>
#include <vector>

#include "me_device.h"
#include "me_math64.h"

namespace me {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;                       // samples per thread and tile
constexpr int kTile = kThreads * kItems;        // 2048 samples
constexpr int kChunk = 16;                      // rungs whose per-lane partial sums are in registers at a time
constexpr int kMaxBlocks = 2048;                // about 8 blocks per CU; the grid depends on the sample count only
constexpr int kUpdateThreads = 1024;
constexpr int kBatch = 16;                      // iterations enqueued between two looks at the residual
constexpr int kTargets = 8;                     // reweighting temperatures per pass over the samples
constexpr int kK = kMbarMaxRungs;

// device-side state of a solve: doubles [beta | c = ln N + f | ln N | N | f], then the control words
constexpr int kBeta = 0, kC = kK, kLnN = 2 * kK, kN = 3 * kK, kF = 4 * kK, kTableDoubles = 5 * kK;
struct MbarControl {
  double residual;
  int iterations, done;
};

template <typename R>
__global__ void __launch_bounds__(kThreads) k_energy_record(const R *energy, long long n, int n_terms, double *dst) {
  const long long c = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (c >= n) return;
  const Field<R> fe(energy, n, n_terms);
  dst[c] = (double)chain_energy(fe, (unsigned int)c * (unsigned int)sizeof(R), n_terms);
}

// N_k: the finite samples of every rung
__global__ void __launch_bounds__(kThreads) k_mbar_count(const double *__restrict__ energies, const int *__restrict__ rungs,
                                                         long long n, long long n_chains, long long rung_chains, int n_rungs,
                                                         unsigned long long *counts) {
  __shared__ unsigned int local[kK];
  if (threadIdx.x < kK) local[threadIdx.x] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    if (!isfinite(energies[i])) continue;
    const long long k = rungs ? (long long)rungs[i] : (i % n_chains) / rung_chains;
    if (k >= 0 && k < n_rungs) atomicAdd(&local[k], 1u);      // (the host has checked the range of `rungs`)
  }
  __syncthreads();
  if (threadIdx.x < n_rungs && local[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)local[threadIdx.x]);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
  return v;
}

// the block's sum of every lane's acc[0 .. kChunk) added to total[c0 ..): wavefront butterfly, then the wavefronts in order
__device__ __forceinline__ void flush_chunk(double (&acc)[kChunk], int c0, int n_rungs, double (*red)[kChunk], double *total) {
#pragma unroll
  for (int j = 0; j < kChunk; ++j) {
    if (c0 + j < n_rungs) {
      const double s = wave_sum(acc[j]);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s;
    }
    acc[j] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < kChunk && c0 + (int)threadIdx.x < n_rungs) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < kWaves; ++w) s = s + red[w][threadIdx.x];
    total[c0 + threadIdx.x] = total[c0 + threadIdx.x] + s;
  }
  __syncthreads();
}

// m_n and s_n of one sample over all rungs (table indices are wave-uniform)
__device__ __forceinline__ void sample_max_sum(const double *__restrict__ table, int n_rungs, double e, double &m, double &s) {
  m = -INFINITY;
  for (int j = 0; j < n_rungs; ++j) m = fmax(m, __builtin_fma(-table[kBeta + j], e, table[kC + j]));
  s = 0.0;
  for (int j = 0; j < n_rungs; ++j) s = s + math64::exp_nonpos(__builtin_fma(-table[kBeta + j], e, table[kC + j]) - m);
}

// one sample of a tile: its energy (0 when it does not count) and whether it counts
__device__ __forceinline__ double load_sample(const double *__restrict__ energies, long long i, long long n, bool &ok) {
  const double v = i < n ? energies[i] : NAN;
  ok = isfinite(v);
  return ok ? v : 0.0;
}

__global__ void __launch_bounds__(kThreads) k_mbar_weights(const double *__restrict__ energies, long long n, int n_rungs,
                                                           const double *__restrict__ table,
                                                           const MbarControl *__restrict__ control, long long n_tiles,
                                                           double *partials) {
  if (control->done) return;
  __shared__ double red[kWaves][kChunk], total[kK];
  __shared__ double kept_m[kItems][kThreads], kept_inv[kItems][kThreads];     // beyond kChunk rungs: a thread's own samples
  if (threadIdx.x < kK) total[threadIdx.x] = 0.0;
  __syncthreads();
  double acc[kChunk];
#pragma unroll
  for (int j = 0; j < kChunk; ++j) acc[j] = 0.0;
  const bool single = n_rungs <= kChunk;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long base = tile * kTile + threadIdx.x;
    // (the sample loops stay rolled: sixteen exponentials in flight per lane are enough, and eight samples' worth of them
    // took 407 registers)
    if (single) {
#pragma unroll 1
      for (int r = 0; r < kItems; ++r) {
        bool ok;
        const double e = load_sample(energies, base + (long long)r * kThreads, n, ok);
        double a[kChunk], m = -INFINITY, s = 0.0;
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
          if (j < n_rungs) {
            a[j] = __builtin_fma(-table[kBeta + j], e, table[kC + j]);
            m = fmax(m, a[j]);
          }
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
          if (j < n_rungs) {
            a[j] = math64::exp_nonpos(a[j] - m);
            s = s + a[j];
          }
        const double inv = ok ? 1.0 / s : 0.0;
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
          if (j < n_rungs) acc[j] = __builtin_fma(a[j], inv, acc[j]);
      }
    } else {
#pragma unroll 1
      for (int r = 0; r < kItems; ++r) {
        bool ok;
        const double e = load_sample(energies, base + (long long)r * kThreads, n, ok);
        double m, s;
        sample_max_sum(table, n_rungs, e, m, s);
        kept_m[r][threadIdx.x] = m;
        kept_inv[r][threadIdx.x] = ok ? 1.0 / s : 0.0;
      }
      for (int c0 = 0; c0 < n_rungs; c0 += kChunk) {
#pragma unroll 1
        for (int r = 0; r < kItems; ++r) {
          bool ok;
          const double e = load_sample(energies, base + (long long)r * kThreads, n, ok);
          const double m = kept_m[r][threadIdx.x], inv = kept_inv[r][threadIdx.x];
#pragma unroll
          for (int j = 0; j < kChunk; ++j)
            if (c0 + j < n_rungs) {
              const double a = __builtin_fma(-table[kBeta + c0 + j], e, table[kC + c0 + j]);
              acc[j] = __builtin_fma(math64::exp_nonpos(a - m), inv, acc[j]);
            }
        }
        flush_chunk(acc, c0, n_rungs, red, total);
      }
    }
  }
  if (single) flush_chunk(acc, 0, n_rungs, red, total);
  if ((int)threadIdx.x < n_rungs) partials[(size_t)blockIdx.x * n_rungs + threadIdx.x] = total[threadIdx.x];
}

// S_k from the block partials, the update of f and of the table, the residual and the stop flag (one block)
__global__ void __launch_bounds__(kUpdateThreads) k_mbar_update(const double *partials, int n_blocks, int n_rungs, double tolerance,
                                                                double *table, MbarControl *control) {
  if (control->done) return;
  __shared__ double sums[kK], f_new[kK], change[kK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < n_rungs; k += kUpdateThreads / 64) {
    double s = 0.0;
    for (int b = lane; b < n_blocks; b += 64) s = s + partials[(size_t)b * n_rungs + k];
    s = wave_sum(s);
    if (lane == 0) sums[k] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < n_rungs) f_new[k] = table[kF + k] - log(sums[k] / table[kN + k]);
  __syncthreads();
  if (k < n_rungs) {
    const double f = f_new[k] - f_new[0];
    change[k] = fabs(f - table[kF + k]);
    table[kF + k] = f;
    table[kC + k] = table[kLnN + k] + f;
  }
  __syncthreads();
  if (k == 0) {
    double r = change[0];
    for (int j = 1; j < n_rungs; ++j) r = (change[j] > r || change[j] != change[j]) ? change[j] : r;   // (a NaN shows)
    control->residual = r;
    control->iterations += 1;
    if (r <= tolerance) control->done = 1;
  }
}

// ---- reweighting ------------------------------------------------------------------------------------------------------
// weights w_n = exp(l_n - M) of some samples: W = sum w, the weighted mean of E, M2 = sum w (E - mean)^2, Q = sum w^2
struct Moments {
  double M, W, mean, M2, Q;
};

__device__ __forceinline__ Moments empty_moments() { return Moments{-INFINITY, 0.0, 0.0, 0.0, 0.0}; }

// one more sample (l, e); one exponential, no branch
__device__ __forceinline__ void add_sample(Moments &s, double l, double e) {
  const bool higher = l > s.M;
  const double x = math64::exp_nonpos(higher ? s.M - l : l - s.M);
  const double scale = higher ? x : 1.0, w = higher ? 1.0 : x;
  const double W_old = s.W * scale, W = W_old + w;
  const double delta = e - s.mean;
  s.mean = s.mean + delta * (w / W);
  s.M2 = s.M2 * scale + w * delta * (e - s.mean);
  s.Q = s.Q * (scale * scale) + w * w;
  s.W = W;
  s.M = higher ? l : s.M;
}

// a (earlier in the fixed order) and b joined
__device__ __forceinline__ Moments merge(const Moments &a, const Moments &b) {
  if (!(b.W > 0.0)) return a;
  if (!(a.W > 0.0)) return b;
  Moments r;
  r.M = fmax(a.M, b.M);
  const double sa = math64::exp_nonpos(a.M - r.M), sb = math64::exp_nonpos(b.M - r.M);
  const double Wa = a.W * sa, Wb = b.W * sb;
  r.W = Wa + Wb;
  const double delta = b.mean - a.mean;
  r.mean = a.mean + delta * (Wb / r.W);
  r.M2 = (a.M2 * sa + b.M2 * sb) + (delta * delta) * (Wa * (Wb / r.W));
  r.Q = a.Q * (sa * sa) + b.Q * (sb * sb);
  return r;
}

__device__ __forceinline__ Moments shuffle_xor(const Moments &s, int d) {
  return Moments{__shfl_xor(s.M, d), __shfl_xor(s.W, d), __shfl_xor(s.mean, d), __shfl_xor(s.M2, d), __shfl_xor(s.Q, d)};
}

// butterfly over the wavefront; the lower lane's state is always the first operand, so every lane holds the same result
__device__ __forceinline__ Moments wave_merge(Moments s) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Moments o = shuffle_xor(s, d);
    s = (lane & d) ? merge(o, s) : merge(s, o);
  }
  return s;
}

// block `b`'s merged states of n_targets temperatures (inv_temps[t] = 1 / T_t) into partials[b][t]
__global__ void __launch_bounds__(kThreads) k_mbar_reweight(const double *__restrict__ energies, long long n, int n_rungs,
                                                            const double *__restrict__ table,
                                                            const double *__restrict__ inv_temps, int n_targets,
                                                            long long n_tiles, Moments *partials) {
  __shared__ Moments waves[kWaves];
  Moments st[kTargets];
#pragma unroll
  for (int t = 0; t < kTargets; ++t) st[t] = empty_moments();
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long base = tile * kTile + threadIdx.x;
    for (int r = 0; r < kItems; ++r) {
      const long long i = base + (long long)r * kThreads;
      const double e = i < n ? energies[i] : NAN;
      if (!isfinite(e)) continue;
      double m, s;
      sample_max_sum(table, n_rungs, e, m, s);
      const double d = m + log(s);
#pragma unroll
      for (int t = 0; t < kTargets; ++t)
        if (t < n_targets) add_sample(st[t], __builtin_fma(-e, inv_temps[t], -d), e);
    }
  }
#pragma unroll
  for (int t = 0; t < kTargets; ++t) {
    if (t >= n_targets) break;
    const Moments w = wave_merge(st[t]);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      Moments b = waves[0];
      for (int k = 1; k < kWaves; ++k) b = merge(b, waves[k]);
      partials[(size_t)blockIdx.x * kTargets + t] = b;
    }
    __syncthreads();
  }
}

// block t: the block partials of temperature t joined in a fixed order; out[t] = (ln_z, mean_e, var_e, neff_fraction)
__global__ void __launch_bounds__(kThreads) k_mbar_reweight_finish(const Moments *partials, int n_blocks, double n_used,
                                                                   double *out) {
  __shared__ Moments waves[kWaves];
  const int t = blockIdx.x;
  Moments s = empty_moments();
  for (int b = threadIdx.x; b < n_blocks; b += kThreads) s = merge(s, partials[(size_t)b * kTargets + t]);
  s = wave_merge(s);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  Moments b = waves[0];
  for (int k = 1; k < kWaves; ++k) b = merge(b, waves[k]);
  out[4 * t] = b.M + log(b.W);
  out[4 * t + 1] = b.mean;
  out[4 * t + 2] = b.M2 / b.W;
  out[4 * t + 3] = (b.W * b.W) / (n_used * b.Q);
}

// ---- host side --------------------------------------------------------------------------------------------------------
struct Work {
  double *table = nullptr, *partials = nullptr, *inv_temps = nullptr, *out = nullptr;
  Moments *moments = nullptr;
  unsigned long long *counts = nullptr;
  MbarControl *control = nullptr;
  ~Work() {
    for (void *p : {(void *)table, (void *)partials, (void *)inv_temps, (void *)out, (void *)moments, (void *)counts, (void *)control})
      if (p) (void)hipFree(p);
  }
};

#define ME_MBAR_HIP(call)                 \
  do {                                    \
    hipError_t err__ = (call);            \
    if (err__ != hipSuccess) return err__; \
  } while (0)

long long tiles_of(long long n) { return (n + kTile - 1) / kTile; }
int blocks_of(long long n) { return (int)std::min<long long>(tiles_of(n), kMaxBlocks); }

// N_k into host `counts`; *empty_rung = the first rung without a finite sample or -1
hipError_t count_used(const MbarSamples &sm, int n_rungs, Work &w, std::vector<unsigned long long> &counts, int *empty_rung,
                      hipStream_t stream) {
  ME_MBAR_HIP(hipMalloc((void **)&w.counts, kK * sizeof(unsigned long long)));
  ME_MBAR_HIP(hipMemsetAsync(w.counts, 0, kK * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_mbar_count, dim3(blocks_of(sm.n_samples)), dim3(kThreads), 0, stream, sm.energies, sm.rungs, sm.n_samples,
                     sm.n_chains, sm.rung_chains, n_rungs, w.counts);
  ME_MBAR_HIP(hipGetLastError());
  counts.assign(kK, 0);
  ME_MBAR_HIP(hipMemcpyAsync(counts.data(), w.counts, kK * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  ME_MBAR_HIP(hipStreamSynchronize(stream));
  *empty_rung = -1;
  for (int k = n_rungs - 1; k >= 0; --k)
    if (counts[k] == 0) *empty_rung = k;
  return hipSuccess;
}

// the device table for free energies f
hipError_t upload_table(Work &w, const double *ladder_temps, int n_rungs, const std::vector<unsigned long long> &counts,
                        const double *f, hipStream_t stream) {
  std::vector<double> table(kTableDoubles, 0.0);
  for (int k = 0; k < n_rungs; ++k) {
    table[kBeta + k] = 1.0 / ladder_temps[k];
    table[kN + k] = (double)counts[k];
    table[kLnN + k] = std::log((double)counts[k]);
    table[kF + k] = f ? f[k] : 0.0;
    table[kC + k] = table[kLnN + k] + table[kF + k];
  }
  ME_MBAR_HIP(hipMalloc((void **)&w.table, kTableDoubles * sizeof(double)));
  ME_MBAR_HIP(hipMemcpyAsync(w.table, table.data(), kTableDoubles * sizeof(double), hipMemcpyHostToDevice, stream));
  ME_MBAR_HIP(hipStreamSynchronize(stream));      // `table` leaves scope
  return hipSuccess;
}

}  // namespace

hipError_t launch_energy_record(const void *energy, long long n, int n_terms, int dtype, double *dst, hipStream_t stream) {
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
  if (dtype == ME_F32) hipLaunchKernelGGL(k_energy_record<float>, grid, dim3(kThreads), 0, stream, (const float *)energy, n, n_terms, dst);
  else hipLaunchKernelGGL(k_energy_record<double>, grid, dim3(kThreads), 0, stream, (const double *)energy, n, n_terms, dst);
  return hipGetLastError();
}

hipError_t mbar_solve(const MbarSamples &sm, const double *ladder_temps, int n_rungs, double tolerance, int max_iterations,
                      double *f, int *iterations, double *residual, long long *n_used, int *empty_rung, hipStream_t stream) {
  if (n_rungs < 1 || n_rungs > kK || sm.n_samples < 1) return hipErrorInvalidValue;
  Work w;
  std::vector<unsigned long long> counts;
  ME_MBAR_HIP(count_used(sm, n_rungs, w, counts, empty_rung, stream));
  for (int k = 0; k < n_rungs; ++k) n_used[k] = (long long)counts[k];
  if (*empty_rung >= 0) return hipSuccess;
  ME_MBAR_HIP(upload_table(w, ladder_temps, n_rungs, counts, nullptr, stream));
  const int n_blocks = blocks_of(sm.n_samples);
  const long long n_tiles = tiles_of(sm.n_samples);
  ME_MBAR_HIP(hipMalloc((void **)&w.partials, (size_t)n_blocks * n_rungs * sizeof(double)));
  ME_MBAR_HIP(hipMalloc((void **)&w.control, sizeof(MbarControl)));
  ME_MBAR_HIP(hipMemsetAsync(w.control, 0, sizeof(MbarControl), stream));
  MbarControl c{0.0, 0, 0};
  while (c.iterations < max_iterations && !c.done) {
    const int batch = std::min(kBatch, max_iterations - c.iterations);
    for (int it = 0; it < batch; ++it) {
      hipLaunchKernelGGL(k_mbar_weights, dim3(n_blocks), dim3(kThreads), 0, stream, sm.energies, sm.n_samples, n_rungs,
                         (const double *)w.table, (const MbarControl *)w.control, n_tiles, w.partials);
      hipLaunchKernelGGL(k_mbar_update, dim3(1), dim3(kUpdateThreads), 0, stream, (const double *)w.partials, n_blocks, n_rungs,
                         tolerance, w.table, w.control);
    }
    ME_MBAR_HIP(hipGetLastError());
    ME_MBAR_HIP(hipMemcpyAsync(&c, w.control, sizeof(MbarControl), hipMemcpyDeviceToHost, stream));
    ME_MBAR_HIP(hipStreamSynchronize(stream));
  }
  ME_MBAR_HIP(hipMemcpyAsync(f, w.table + kF, (size_t)n_rungs * sizeof(double), hipMemcpyDeviceToHost, stream));
  ME_MBAR_HIP(hipStreamSynchronize(stream));
  *iterations = c.iterations;
  *residual = c.residual;
  return hipSuccess;
}

hipError_t mbar_reweight(const MbarSamples &sm, const double *ladder_temps, int n_rungs, const double *f, const double *temps,
                         int n_temps, double *ln_z, double *mean_e, double *var_e, double *neff_fraction, int *empty_rung,
                         hipStream_t stream) {
  if (n_rungs < 1 || n_rungs > kK || sm.n_samples < 1 || n_temps < 1) return hipErrorInvalidValue;
  Work w;
  std::vector<unsigned long long> counts;
  ME_MBAR_HIP(count_used(sm, n_rungs, w, counts, empty_rung, stream));
  if (*empty_rung >= 0) return hipSuccess;
  double n_used = 0.0;
  for (int k = 0; k < n_rungs; ++k) n_used += (double)counts[k];
  ME_MBAR_HIP(upload_table(w, ladder_temps, n_rungs, counts, f, stream));
  const int n_blocks = blocks_of(sm.n_samples);
  const long long n_tiles = tiles_of(sm.n_samples);
  std::vector<double> inv((size_t)n_temps), out(4 * (size_t)n_temps);
  for (int t = 0; t < n_temps; ++t) inv[t] = 1.0 / temps[t];
  ME_MBAR_HIP(hipMalloc((void **)&w.inv_temps, inv.size() * sizeof(double)));
  ME_MBAR_HIP(hipMalloc((void **)&w.out, out.size() * sizeof(double)));
  ME_MBAR_HIP(hipMalloc((void **)&w.moments, (size_t)n_blocks * kTargets * sizeof(Moments)));
  ME_MBAR_HIP(hipMemcpyAsync(w.inv_temps, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  for (int t0 = 0; t0 < n_temps; t0 += kTargets) {
    const int nt = std::min(kTargets, n_temps - t0);
    hipLaunchKernelGGL(k_mbar_reweight, dim3(n_blocks), dim3(kThreads), 0, stream, sm.energies, sm.n_samples, n_rungs,
                       (const double *)w.table, (const double *)(w.inv_temps + t0), nt, n_tiles, w.moments);
    hipLaunchKernelGGL(k_mbar_reweight_finish, dim3(nt), dim3(kThreads), 0, stream, (const Moments *)w.moments, n_blocks, n_used,
                       w.out + 4 * (size_t)t0);
  }
  ME_MBAR_HIP(hipGetLastError());
  ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out, out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  ME_MBAR_HIP(hipStreamSynchronize(stream));
  for (int t = 0; t < n_temps; ++t) {
    if (ln_z) ln_z[t] = out[4 * (size_t)t];
    if (mean_e) mean_e[t] = out[4 * (size_t)t + 1];
    if (var_e) var_e[t] = out[4 * (size_t)t + 2];
    if (neff_fraction) neff_fraction[t] = out[4 * (size_t)t + 3];
  }
  return hipSuccess;
}

}  // namespace me
