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
#include "me_mbar.h"

namespace me {
namespace mbar {
namespace {

constexpr int kChunk = 16;                      // rungs whose per-lane partial sums are in registers at a time
constexpr int kUpdateThreads = 1024;
constexpr int kBatch = 16;                      // iterations enqueued between two looks at the residual

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

}  // namespace


// ---- host side --------------------------------------------------------------------------------------------------------
hipError_t prepare(Problem &p, const Source &src, const double *f) {
  p.sm = src.sm;
  p.n_rungs = src.n_rungs;
  p.stream = src.stream;
  Work &w = p.w;
  const int n_rungs = p.n_rungs;
  if (n_rungs < 1 || n_rungs > kK || p.sm.n_samples < 1) return hipErrorInvalidValue;
  // N_k: the finite samples of every rung
  ME_MBAR_HIP(w.counts.resize(kK * sizeof(unsigned long long)));
  ME_MBAR_HIP(hipMemsetAsync(w.counts.get(), 0, w.counts.bytes(), p.stream));
  hipLaunchKernelGGL(k_mbar_count, dim3(blocks_of(p.sm.n_samples)), dim3(kThreads), 0, p.stream, p.sm.energies, p.sm.rungs,
                     p.sm.n_samples, p.sm.n_chains, p.sm.rung_chains, n_rungs, w.counts.get<unsigned long long>());
  ME_MBAR_HIP(hipGetLastError());
  ME_MBAR_HIP(hipMemcpyAsync(p.counts, w.counts.get(), kK * sizeof(unsigned long long), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipStreamSynchronize(p.stream));
  p.empty_rung = -1;
  for (int k = n_rungs - 1; k >= 0; --k)
    if (p.counts[k] == 0) p.empty_rung = k;
  if (p.empty_rung >= 0) return hipSuccess;
  for (int k = 0; k < n_rungs; ++k) {
    p.n_used += (double)p.counts[k];
    p.n_used_ll += (long long)p.counts[k];
  }
  // the device table for the free energies f
  std::vector<double> table(kTableDoubles, 0.0);
  for (int k = 0; k < n_rungs; ++k) {
    table[kBeta + k] = 1.0 / src.ladder_temps[k];
    table[kN + k] = (double)p.counts[k];
    table[kLnN + k] = std::log((double)p.counts[k]);
    table[kF + k] = f ? f[k] : 0.0;
    table[kC + k] = table[kLnN + k] + table[kF + k];
  }
  ME_MBAR_HIP(w.table.resize(kTableDoubles * sizeof(double)));
  ME_MBAR_HIP(hipMemcpyAsync(w.table.get(), table.data(), kTableDoubles * sizeof(double), hipMemcpyHostToDevice, p.stream));
  return hipStreamSynchronize(p.stream);          // `table` leaves scope
}

hipError_t upload_targets(Problem &p, const double *temps, int n, size_t out_doubles, std::vector<double> &inv) {
  inv.resize((size_t)n);
  for (int t = 0; t < n; ++t) inv[t] = 1.0 / temps[t];
  ME_MBAR_HIP(p.w.inv_temps.resize(inv.size() * sizeof(double)));
  ME_MBAR_HIP(p.w.out.resize(out_doubles * sizeof(double)));
  return hipMemcpyAsync(p.w.inv_temps.get(), inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice, p.stream);
}

hipError_t reweight_enqueue(Problem &p, const MbarSamples &sm, const double *temps, int n_temps, std::vector<double> &inv) {
  Work &w = p.w;
  const int n_blocks = blocks_of(sm.n_samples);
  const long long n_tiles = tiles_of(sm.n_samples);
  ME_MBAR_HIP(w.moments.resize((size_t)n_blocks * kTargets * sizeof(Moments)));
  ME_MBAR_HIP(upload_targets(p, temps, n_temps, 4 * (size_t)n_temps, inv));
  for (int t0 = 0; t0 < n_temps; t0 += kTargets) {
    const int nt = std::min(kTargets, n_temps - t0);
    hipLaunchKernelGGL(k_mbar_reweight, dim3(n_blocks), dim3(kThreads), 0, p.stream, sm.energies, sm.n_samples, p.n_rungs,
                       w.table.get<const double>(), w.inv_temps.get<const double>() + t0, nt, n_tiles, w.moments.get<Moments>());
    hipLaunchKernelGGL(k_mbar_reweight_finish, dim3(nt), dim3(kThreads), 0, p.stream, w.moments.get<const Moments>(), n_blocks,
                       p.n_used, w.out.get<double>() + 4 * (size_t)t0);
  }
  return hipGetLastError();
}

void unpack_targets(const std::vector<double> &out, int n_temps, double *ln_z, double *mean_e, double *var_e, double *neff_fraction) {
  double *const dst[4] = {ln_z, mean_e, var_e, neff_fraction};
  for (int j = 0; j < 4; ++j)
    for (int t = 0; dst[j] && t < n_temps; ++t) dst[j][t] = out[4 * (size_t)t + j];
}

// ---- what the entry points share ----------------------------------------------------------------------------------------
int mbar_check_common(me_engine *e, const Problem &p, hipError_t err) {
  if (err == hipErrorInvalidValue)
    return fail(e, ME_ERR_UNSUPPORTED, "MBAR supports 1 to " + std::to_string(kK) + " rungs and at least one sample");
  ME_HIP(e, err);
  if (p.empty_rung >= 0)
    return fail(e, ME_ERR_STATE, "rung " + std::to_string(p.empty_rung) + " of " + std::to_string(p.n_rungs) +
                                     " has no sample with a finite energy: MBAR needs every rung sampled");
  return ME_OK;
}
int mbar_check_temps(me_engine *e, const double *temps, int n, const char *what) {
  for (int k = 0; k < n; ++k)
    if (!(std::isfinite(temps[k]) && temps[k] > 0)) return fail(e, ME_ERR_INVALID, std::string(what) + " must be finite and > 0");
  return ME_OK;
}
int check_f_and_targets(me_engine *e, const double *f, int n_rungs, const double *temps, int n, int min_targets) {
  if (!f || n < min_targets || (n > 0 && !temps))
    return fail(e, ME_ERR_INVALID, min_targets > 0 ? "f and at least one target temperature are needed"
                                                   : "f and n_targets >= 0 temperatures are needed");
  const int rc = mbar_check_temps(e, temps, n, "target temperatures");
  if (rc) return rc;
  for (int k = 0; k < n_rungs; ++k)
    if (!std::isfinite(f[k])) return fail(e, ME_ERR_INVALID, "f must be finite");
  return ME_OK;
}

int Source::from_engine(me_engine *engine) {
  if (!engine) return ME_ERR_INVALID;
  e = engine;
  if (e->ladder.n_rungs == 0) return fail(e, ME_ERR_STATE, "no temperature ladder: MBAR combines the rungs of me_set_temperature_ladder");
  if (!e->samples.data || e->samples.rows == 0)
    return fail(e, ME_ERR_STATE, "no recorded energy samples: me_energy_samples_enable, then me_energy_samples_record");
  sm = MbarSamples{e->samples.data.get<double>(), nullptr, e->samples.rows * e->n, e->n, e->n / e->ladder.n_rungs};
  ladder_temps = e->ladder.temps.data();
  n_rungs = e->ladder.n_rungs;
  stream = e->stream;
  columns = ObsColumns{e->samples.obs.get<const double>(), e->samples.n_obs, e->n, (long long)e->samples.n_obs * e->n, e->n};
  ME_HIP(e, hipSetDevice(e->device));
  return ME_OK;
}
int Source::from_host(int device_id, const double *energies, const int32_t *rungs, int64_t n_samples, const double *temps, int n) {
  if (!energies || !rungs || !temps) return fail(nullptr, ME_ERR_INVALID, "null pointer");
  if (n_samples < 1 || n < 1) return fail(nullptr, ME_ERR_INVALID, "need n_samples >= 1 and n_rungs >= 1");
  const int rc = mbar_check_temps(nullptr, temps, n, "ladder temperatures");
  if (rc) return rc;
  for (int64_t i = 0; i < n_samples; ++i)
    if (rungs[i] < 0 || rungs[i] >= n) return fail(nullptr, ME_ERR_INVALID, "rungs must lie in [0, n_rungs)");
  ME_HIP(nullptr, hipSetDevice(device_id));
  ME_HIP(nullptr, energies_dev.resize(sizeof(double) * (size_t)n_samples));
  ME_HIP(nullptr, rungs_dev.resize(sizeof(int) * (size_t)n_samples));
  ME_HIP(nullptr, hipMemcpy(energies_dev.get(), energies, energies_dev.bytes(), hipMemcpyHostToDevice));
  ME_HIP(nullptr, hipMemcpy(rungs_dev.get(), rungs, rungs_dev.bytes(), hipMemcpyHostToDevice));
  sm = MbarSamples{energies_dev.get<double>(), rungs_dev.get<int>(), n_samples, 1, 1};
  ladder_temps = temps;
  n_rungs = n;
  return ME_OK;
}
int Source::from_host(int device_id, const double *energies, const int32_t *rungs, int64_t n_samples, const double *temps, int n,
                      const double *observables, int n_columns) {
  if (!observables) return fail(nullptr, ME_ERR_INVALID, "null pointer");
  if (n_columns < 1 || n_columns > ME_MAX_RECORDED_OBSERVABLES)
    return fail(nullptr, ME_ERR_INVALID, "n_observables must lie in [1, " + std::to_string(ME_MAX_RECORDED_OBSERVABLES) + "]");
  const int rc = from_host(device_id, energies, rungs, n_samples, temps, n);
  if (rc) return rc;
  ME_HIP(nullptr, columns_dev.resize(sizeof(double) * (size_t)n_samples * (size_t)n_columns));
  ME_HIP(nullptr, hipMemcpy(columns_dev.get(), observables, columns_dev.bytes(), hipMemcpyHostToDevice));
  columns = ObsColumns{columns_dev.get<const double>(), n_columns, n_samples, 0, n_samples};
  return ME_OK;
}
int Source::finish(int rc) const {
  (void)hipDeviceSynchronize();
  return rc;
}

namespace {

// Both wait for the stream and write host arrays; with an empty rung (p.empty_rung) nothing else is computed.
// mbar_solve: f[K].  mbar_reweight: any of the four outputs may be nullptr.
hipError_t mbar_solve(Problem &p, const Source &src, double tolerance, int max_iterations, double *f, int *iterations, double *residual) {
  ME_MBAR_HIP(prepare(p, src, nullptr));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const int n_rungs = p.n_rungs, n_blocks = blocks_of(p.sm.n_samples);
  const long long n_tiles = tiles_of(p.sm.n_samples);
  ME_MBAR_HIP(w.partials.resize((size_t)n_blocks * n_rungs * sizeof(double)));
  ME_MBAR_HIP(w.control.resize(sizeof(MbarControl)));
  ME_MBAR_HIP(hipMemsetAsync(w.control.get(), 0, sizeof(MbarControl), p.stream));
  MbarControl c{0.0, 0, 0};
  while (c.iterations < max_iterations && !c.done) {
    const int batch = std::min(kBatch, max_iterations - c.iterations);
    for (int it = 0; it < batch; ++it) {
      hipLaunchKernelGGL(k_mbar_weights, dim3(n_blocks), dim3(kThreads), 0, p.stream, p.sm.energies, p.sm.n_samples, n_rungs,
                         w.table.get<const double>(), w.control.get<const MbarControl>(), n_tiles, w.partials.get<double>());
      hipLaunchKernelGGL(k_mbar_update, dim3(1), dim3(kUpdateThreads), 0, p.stream, w.partials.get<const double>(), n_blocks, n_rungs,
                         tolerance, w.table.get<double>(), w.control.get<MbarControl>());
    }
    ME_MBAR_HIP(hipGetLastError());
    ME_MBAR_HIP(hipMemcpyAsync(&c, w.control.get(), sizeof(MbarControl), hipMemcpyDeviceToHost, p.stream));
    ME_MBAR_HIP(hipStreamSynchronize(p.stream));
  }
  ME_MBAR_HIP(hipMemcpyAsync(f, w.table.get<double>() + kF, (size_t)n_rungs * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipStreamSynchronize(p.stream));
  *iterations = c.iterations;
  *residual = c.residual;
  return hipSuccess;
}

hipError_t mbar_reweight(Problem &p, const Source &src, const double *f, const double *temps, int n_temps, double *ln_z, double *mean_e,
                         double *var_e, double *neff_fraction) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  std::vector<double> inv, out(4 * (size_t)n_temps);
  ME_MBAR_HIP(reweight_enqueue(p, p.sm, temps, n_temps, inv));
  ME_MBAR_HIP(hipMemcpyAsync(out.data(), p.w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipStreamSynchronize(p.stream));
  unpack_targets(out, n_temps, ln_z, mean_e, var_e, neff_fraction);
  return hipSuccess;
}

// the two forms of me_mbar_solve and of me_mbar_reweight behind their Source
int solve_common(const Source &src, double tolerance, int max_iterations, double *f_out, int32_t *iterations, double *residual,
                 int64_t *n_used_out) {
  if (!f_out) return fail(src.e, ME_ERR_INVALID, "f_out missing");
  if (!(tolerance > 0) || max_iterations < 1) return fail(src.e, ME_ERR_INVALID, "need tolerance > 0 and max_iterations >= 1");
  Problem p;
  int its = 0;
  double res = 0.0;
  const hipError_t err = mbar_solve(p, src, tolerance, max_iterations, f_out, &its, &res);
  if (err == hipSuccess && n_used_out)            // (also when a rung is empty: the message names one, these show all)
    for (int k = 0; k < p.n_rungs; ++k) n_used_out[k] = (int64_t)p.counts[k];
  const int rc = mbar_check_common(src.e, p, err);
  if (rc) return rc;
  if (iterations) *iterations = its;
  if (residual) *residual = res;
  return ME_OK;
}

int reweight_common(const Source &src, const double *f, const double *temps, int n, double *ln_z, double *mean_e, double *var_e,
                    double *neff_fraction) {
  const int rc = check_f_and_targets(src.e, f, src.n_rungs, temps, n, 1);
  if (rc) return rc;
  Problem p;
  return mbar_check_common(src.e, p, mbar_reweight(p, src, f, temps, n, ln_z, mean_e, var_e, neff_fraction));
}

}  // namespace
}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_energy_samples_enable(me_engine *e, int64_t capacity_records) {
  if (!e) return ME_ERR_INVALID;
  if (capacity_records < 0) return fail(e, ME_ERR_INVALID, "capacity_records must be >= 0");
  const int rc = refuse_stale_total(e, "energy samples are");
  if (rc != ME_OK) return rc;
  ME_HIP(e, hipSetDevice(e->device));
  ME_HIP(e, hipStreamSynchronize(e->stream));       // a record in flight writes the field
  e->samples = me_engine::Samples();
  ME_HIP(e, e->samples.data.resize((size_t)capacity_records * (size_t)e->n * sizeof(double)));
  e->samples.capacity = capacity_records;
  return ME_OK;
}

int me_energy_samples_record(me_engine *e) {
  if (!e) return ME_ERR_INVALID;
  if (!e->samples.data) return fail(e, ME_ERR_STATE, "energy samples are not enabled: call me_energy_samples_enable first");
  if (e->samples.rows >= e->samples.capacity)
    return fail(e, ME_ERR_STATE, "the energy sample store is full (" + std::to_string(e->samples.capacity) + " records)");
  ME_HIP(e, hipSetDevice(e->device));
  // dst[c] = (double)(sum of chain c's ledger rows in row order in the device dtype), c < n
  double *dst = e->samples.data.get<double>() + (size_t)e->samples.rows * (size_t)e->n;
  const dim3 grid((unsigned)((e->n + kThreads - 1) / kThreads));
  if (e->dtype == ME_F32)
    hipLaunchKernelGGL(k_energy_record<float>, grid, dim3(kThreads), 0, e->stream, e->energy.get<const float>(), e->n, e->n_terms, dst);
  else hipLaunchKernelGGL(k_energy_record<double>, grid, dim3(kThreads), 0, e->stream, e->energy.get<const double>(), e->n, e->n_terms, dst);
  ME_HIP(e, hipGetLastError());
  if (e->samples.n_obs) ME_HIP(e, observable_record_enqueue(e, e->samples.rows));     // the same moment, the same row
  e->samples.rows += 1;
  return ME_OK;
}

int me_energy_samples_count(me_engine *e, int64_t *records, int64_t *capacity) {
  if (!e) return ME_ERR_INVALID;
  if (records) *records = e->samples.rows;
  if (capacity) *capacity = e->samples.capacity;
  return ME_OK;
}

int me_energy_samples_get(me_engine *e, int64_t record_begin, int64_t n_records, double *dst) {
  if (!e || (!dst && n_records > 0)) return ME_ERR_INVALID;
  if (record_begin < 0 || n_records < 0 || record_begin + n_records > e->samples.rows)
    return fail(e, ME_ERR_INVALID, "record range outside the recorded samples");
  if (n_records == 0) return ME_OK;
  ME_HIP(e, hipSetDevice(e->device));
  ME_HIP(e, hipMemcpyAsync(dst, e->samples.data.get<double>() + (size_t)record_begin * (size_t)e->n, (size_t)n_records * (size_t)e->n * sizeof(double),
                           hipMemcpyDeviceToHost, e->stream));
  ME_HIP(e, hipStreamSynchronize(e->stream));
  return ME_OK;
}

int me_energy_samples_set(me_engine *e, int64_t n_records, const double *src) {
  if (!e || (!src && n_records > 0)) return ME_ERR_INVALID;
  if (!e->samples.data) return fail(e, ME_ERR_STATE, "energy samples are not enabled: call me_energy_samples_enable first");
  if (n_records < 0 || n_records > e->samples.capacity) return fail(e, ME_ERR_INVALID, "n_records must lie in [0, capacity]");
  ME_HIP(e, hipSetDevice(e->device));
  if (n_records > 0) {
    ME_HIP(e, hipMemcpyAsync(e->samples.data.get(), src, (size_t)n_records * (size_t)e->n * sizeof(double), hipMemcpyHostToDevice, e->stream));
    ME_HIP(e, hipStreamSynchronize(e->stream));
  }
  e->samples.rows = n_records;
  return ME_OK;
}

int me_mbar_solve(me_engine *e, double tolerance, int32_t max_iterations, double *f_out, int32_t *iterations, double *residual,
                  int64_t *n_used_out) {
  Source src;
  const int rc = src.from_engine(e);
  return rc ? rc : solve_common(src, tolerance, max_iterations, f_out, iterations, residual, n_used_out);
}

int me_mbar_reweight(me_engine *e, const double *f, const double *temps, int32_t n, double *ln_z, double *mean_e, double *var_e,
                     double *neff_fraction) {
  Source src;
  const int rc = src.from_engine(e);
  return rc ? rc : reweight_common(src, f, temps, n, ln_z, mean_e, var_e, neff_fraction);
}

int me_mbar_solve_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                          const double *ladder_temps, int32_t n_rungs, double tolerance, int32_t max_iterations, double *f_out,
                          int32_t *iterations, double *residual, int64_t *n_used_out) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs);
  return rc ? rc : src.finish(solve_common(src, tolerance, max_iterations, f_out, iterations, residual, n_used_out));
}

int me_mbar_reweight_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                             const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                             double *ln_z, double *mean_e, double *var_e, double *neff_fraction) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs);
  return rc ? rc : src.finish(reweight_common(src, f, temps, n, ln_z, mean_e, var_e, neff_fraction));
}

}  // extern "C"
