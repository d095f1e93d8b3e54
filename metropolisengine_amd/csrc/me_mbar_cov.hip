// The Gram matrix of the MBAR weight matrix, from which the host forms the asymptotic covariance of the free energies and of
// reweighted energies (me_mbar_gram and its engine-less twin in the public header; Shirts & Chodera, J. Chem. Phys.
// 129:124105, 2008, eqs. 8, 12-15, D8).  Notation as in me_mbar.hip: samples n are USED when E_n is finite, K rungs, beta_k =
// 1 / T_k, N_k used samples of rung k, f from a converged solve, d_n = ln sum_j N_j exp(f_j - beta_j E_n) = m_n + ln s_n
// exactly as the reweighting kernel evaluates it (sample_max_sum, then the device log).
//
// The columns of W (N_used x C, C = K + 2 n_targets), every entry >= 0 and every column summing to 1:
//     ladder column k            W_nk = exp(f_k - beta_k E_n - d_n)                        column k,          count N_k
//     state column of target t   W_na = exp(-E_n / T_t - d_n - ln_z_t)                     column K + 2 t,     count 0
//     energy column of target t  W_nA = W_na (E_n - E_shift) / mean_t                      column K + 2 t + 1, count 0
// ln_z_t is what the reweighting kernels return for T_t, E_shift = (min over the used samples of E_n) - 1 so that every
// factor is >= 1, and mean_t = sum_n W_na (E_n - E_shift) = mean_e(T_t) - E_shift with the reweighting kernels' mean_e.  The
// device produces G = W^T W; the C x C algebra (eigendecomposition, pseudo-inverse) is the host's, in float64.
//
// Kernels.  When some energy is not finite the used samples are first packed, in their order, into a buffer of their own
// (k_mbar_used_tiles counts them per tile of 2048, k_mbar_scan turns the counts into offsets, k_mbar_compact writes them:
// ballots and integer sums only), and everything below runs on the packed samples: the result is bit for bit the result on
// the array with the other samples removed.  k_mbar_min: the block minima of the finite energies.  k_mbar_gram_columns (one
// block): E_shift from them (me_mbar_energy_shift hands the same value to the host, which needs it for mean_t) and the
// per-column constants (b, g, mean) with W_n,col = exp(g - b E_n - d_n) [(E_n - E_shift) / mean], read from the ladder table and from the reweighting kernels' output on the device -- no host round trip per target.  k_mbar_gram: one pass over the
// samples with the grid policy of k_mbar_weights (tiles of 2048 samples walked grid-stride, the grid depends on the sample
// count only).  Per 256 samples of a tile every lane computes d_n of its sample (K exponentials, exp_nonpos) and parks (E_n,
// d_n) in LDS.  They are consumed in sub-tiles of 16 samples: thread (h, j) = (t >> 4, t & 15) writes row h of the sub-tile's
// W, columns j, j + 16, ... (one exponential each; argument clamped at 0, unused samples and the padding columns give 0), as
// float64 into LDS [16][Cp]; Cp = C padded to a multiple of 16 (Cpad), plus 16 when that is a multiple of 32, so that the
// rows a half-wavefront reads lie in different banks.  The sub-tile buffers alternate, so one barrier per sub-tile is enough.
// The block accumulates W^T W with v_mfma_f64_16x16x4_f64: for the 16 x 16 tile (I, J) of G, I >= J, lane l feeds
// A[i = l & 15][k = l >> 4] = W[n0 + k][16 I + i] and B[k = l >> 4][j = l & 15] = W[n0 + k][16 J + j] and receives rows (l >> 4)
// + 4 r (r < 4) of column l & 15.  Only the lower-triangle tiles are computed: pair p = I (I + 1) / 2 + J belongs to wavefront
// p % 4, slot p / 4 -- at C = 128 that is 36 tiles, 9 per wavefront, 9 x 8 = 72 accumulator registers which stay in registers
// for the whole launch.  C <= 128 per launch; more targets go in chunks that each carry the K ladder columns (host side).
// Summation order, fixed (no floating-point atomics, bitwise reproducible): the MFMA's own accumulation over the 4 samples of
// a k-step -> the k-steps in sample order -> the block's tiles in order -> partials[block][C (C + 1) / 2] (packed lower
// triangle) in global memory -> k_mbar_gram_finish adds the blocks in ascending order, one thread per entry, and writes G[i][j]
// and G[j][i] from the same sum, so G is symmetric bit for bit.
// Registers (hipcc -O3, gfx950): k_mbar_gram 93 VGPRs + 72 AGPRs (the accumulators), 3 wavefronts per SIMD, no scratch.
#include "me_mbar.h"

namespace me {
namespace mbar {
namespace {

constexpr int kMaxCols = 128;                   // columns of W per launch
constexpr int kSub = 16;                        // samples per sub-tile in LDS
constexpr int kSlots = 9;                       // 16 x 16 tiles of G per wavefront: 36 lower-triangle tiles / 4
constexpr int kColB = 0, kColG = kMaxCols, kColMean = 2 * kMaxCols, kColShift = 3 * kMaxCols, kColDoubles = 3 * kMaxCols + 1;

typedef double f64x4 __attribute__((ext_vector_type(4)));

// counts[tile] = the finite energies of the tile
__global__ void __launch_bounds__(kThreads) k_mbar_used_tiles(const double *__restrict__ energies, long long n, unsigned int *counts) {
  __shared__ unsigned int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  unsigned int mine = 0;
  for (int r = 0; r < kItems; ++r) {
    const long long i = (long long)blockIdx.x * kTile + (long long)r * kThreads + threadIdx.x;
    mine += (i < n && isfinite(energies[i])) ? 1u : 0u;
  }
  atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// offsets[tile] = the finite energies before the tile (one block; thread t takes tiles [t chunk, (t + 1) chunk))
__global__ void __launch_bounds__(kThreads) k_mbar_scan(const unsigned int *__restrict__ counts, long long n_tiles, long long *offsets) {
  __shared__ long long sums[kThreads];
  const long long chunk = (n_tiles + kThreads - 1) / kThreads, begin = threadIdx.x * chunk, end = min(begin + chunk, n_tiles);
  long long s = 0;
  for (long long i = begin; i < end; ++i) s += counts[i];
  sums[threadIdx.x] = s;
  __syncthreads();
  long long before = 0;
  for (int k = 0; k < (int)threadIdx.x; ++k) before += sums[k];
  for (long long i = begin; i < end; ++i) {
    offsets[i] = before;
    before += counts[i];
  }
}

// the finite energies of tile blockIdx.x, in their order, to packed[offsets[tile] ..)
__global__ void __launch_bounds__(kThreads) k_mbar_compact(const double *__restrict__ energies, long long n,
                                                           const long long *__restrict__ offsets, double *packed) {
  __shared__ unsigned int waves[kItems][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double e[kItems];
  unsigned int rank[kItems];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const long long i = (long long)blockIdx.x * kTile + (long long)r * kThreads + threadIdx.x;
    e[r] = i < n ? energies[i] : NAN;
    const unsigned long long ballot = __ballot(isfinite(e[r]));
    rank[r] = (unsigned int)__popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) waves[r][wave] = (unsigned int)__popcll(ballot);
  }
  __syncthreads();
  long long at = offsets[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    unsigned int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      before += w < wave ? waves[r][w] : 0u;
      all += waves[r][w];
    }
    if (isfinite(e[r])) packed[at + before + rank[r]] = e[r];
    at += all;
  }
}

// minima[block] = the least finite energy of the block's tiles (+inf when it has none)
__global__ void __launch_bounds__(kThreads) k_mbar_min(const double *__restrict__ energies, long long n, long long n_tiles,
                                                       double *minima) {
  __shared__ double waves[kWaves];
  double v = INFINITY;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    for (int r = 0; r < kItems; ++r) {
      const long long i = tile * kTile + (long long)r * kThreads + threadIdx.x;
      const double e = i < n ? energies[i] : NAN;
      if (isfinite(e)) v = fmin(v, e);
    }
  v = wave_min(v);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) minima[blockIdx.x] = fmin(fmin(waves[0], waves[1]), fmin(waves[2], waves[3]));
}

// cols = [b | g | mean | E_shift] of the K ladder columns and of the two columns of each of n_targets temperatures, whose
// (ln_z, mean_e, ., .) the reweighting kernels left in `out`
__global__ void __launch_bounds__(kMaxCols) k_mbar_gram_columns(const double *__restrict__ table, int n_rungs,
                                                                const double *__restrict__ inv_temps,
                                                                const double *__restrict__ out, int n_targets,
                                                                const double *__restrict__ minima, int n_blocks, double *cols) {
  __shared__ double part[kMaxCols];
  double v = INFINITY;
  for (int b = threadIdx.x; b < n_blocks; b += kMaxCols) v = fmin(v, minima[b]);
  part[threadIdx.x] = v;
  __syncthreads();
  v = part[0];
  for (int k = 1; k < kMaxCols; ++k) v = fmin(v, part[k]);
  const double shift = v - 1.0;
  const int c = threadIdx.x;
  double b = 0.0, g = 0.0, mean = 0.0;
  if (c < n_rungs) {
    b = table[kBeta + c];
    g = table[kF + c];
  } else if (c < n_rungs + 2 * n_targets) {
    const int t = (c - n_rungs) >> 1;
    b = inv_temps[t];
    g = -out[4 * t];
    if ((c - n_rungs) & 1) mean = out[4 * t + 1] - shift;       // >= 1: 0 marks the columns without the energy factor
  }
  cols[kColB + c] = b;
  cols[kColG + c] = g;
  cols[kColMean + c] = mean;
  if (c == 0) cols[kColShift] = shift;
}

// partials[block] = the packed lower triangle of the block's part of W^T W, n_cols = K + 2 n_targets <= kMaxCols columns.
// Dynamic LDS: 2 * kSub * cp doubles, cp the padded row length (see the header of this file).
__global__ void __launch_bounds__(kThreads) k_mbar_gram(const double *__restrict__ energies, long long n, int n_rungs,
                                                        const double *__restrict__ table, const double *__restrict__ cols,
                                                        int n_cols, int cp, long long n_tiles, double *partials) {
  extern __shared__ double w_lds[];                              // [2][kSub][cp]
  __shared__ double s_e[kThreads], s_d[kThreads], c_b[kMaxCols], c_g[kMaxCols], c_mean[kMaxCols];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int h4 = lane >> 4, j16 = lane & 15;                     // the MFMA's (k, i / j) of this lane
  const int tn = (n_cols + 15) >> 4, n_pairs = tn * (tn + 1) / 2;
  if (t < kMaxCols) {
    c_b[t] = cols[kColB + t];
    c_g[t] = cols[kColG + t];
    c_mean[t] = cols[kColMean + t];
  }
  const double shift = cols[kColShift];
  // this wavefront's tiles: pair p = wave + 4 s = I (I + 1) / 2 + J, column offsets 16 I and 16 J
  int off_i[kSlots], off_j[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int p = wave + kWaves * s;
    int I = 0;
#pragma unroll
    for (int q = 1; q < kMaxCols / 16; ++q) I = p >= q * (q + 1) / 2 ? q : I;
    off_i[s] = 16 * I;
    off_j[s] = 16 * (p - I * (I + 1) / 2);
  }
  f64x4 acc[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int row = t >> 4;                                        // the sub-tile row this thread fills
  int parity = 0;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
    for (int r = 0; r < kItems; ++r) {
      const long long i = tile * kTile + (long long)r * kThreads + t;
      const double e = i < n ? energies[i] : NAN;
      const bool ok = isfinite(e);
      double m, s;
      sample_max_sum(table, n_rungs, ok ? e : 0.0, m, s);
      // (every thread has passed the last barrier of the step before, so its fills have read s_e and s_d)
      s_e[t] = ok ? e : 0.0;
      s_d[t] = ok ? m + log(s) : INFINITY;
      __syncthreads();
#pragma unroll 1
      for (int q = 0; q < kThreads / kSub; ++q) {
        double *buf = w_lds + parity * (kSub * cp);
        {
          const double es = s_e[q * kSub + row], ds = s_d[q * kSub + row];
          const bool used = ds < INFINITY;
#pragma unroll 1
          for (int col = j16; col < 16 * tn; col += 16) {
            double w = 0.0;
            if (used && col < n_cols) {
              w = math64::exp_nonpos(fmin(__builtin_fma(-c_b[col], es, c_g[col]) - ds, 0.0));
              const double mean = c_mean[col];
              if (mean != 0.0) w = w * (es - shift) / mean;
            }
            buf[row * cp + col] = w;
          }
        }
        __syncthreads();
#pragma unroll 2
        for (int ks = 0; ks < kSub / 4; ++ks) {
          const double *src = buf + (4 * ks + h4) * cp + j16;
#pragma unroll
          for (int s = 0; s < kSlots; ++s)
            if (wave + kWaves * s < n_pairs)                      // (wave-uniform)
              acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(src[off_i[s]], src[off_j[s]], acc[s], 0, 0, 0);
        }
        parity ^= 1;                                             // the next fill goes to the other buffer: no second barrier
      }
    }
  }
  double *dst = partials + (size_t)blockIdx.x * (size_t)(n_cols * (n_cols + 1) / 2);
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    if (wave + kWaves * s >= n_pairs) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = off_i[s] + h4 + 4 * r, gj = off_j[s] + j16;
      if (gi < n_cols && gj <= gi) dst[gi * (gi + 1) / 2 + gj] = acc[s][r];
    }
  }
}

// block i: row i of G (and column i) = the blocks' partials added in ascending block order; gram is [n_cols][n_cols]
__global__ void __launch_bounds__(kMaxCols) k_mbar_gram_finish(const double *__restrict__ partials, int n_blocks, int n_cols,
                                                               double *gram) {
  const int i = blockIdx.x, j = threadIdx.x;
  if (j > i) return;
  const size_t stride = (size_t)(n_cols * (n_cols + 1) / 2);
  const double *src = partials + (size_t)(i * (i + 1) / 2 + j);
  double s = 0.0;
  for (int b = 0; b < n_blocks; ++b) s = s + src[(size_t)b * stride];
  gram[i * n_cols + j] = s;
  gram[j * n_cols + i] = s;
}

// ---- host side --------------------------------------------------------------------------------------------------------
int padded_row(int n_cols) {
  const int cpad = (n_cols + 15) / 16 * 16;
  return cpad % 32 == 0 ? cpad + 16 : cpad;
}

// Waits for the stream and writes host arrays: gram[C][C] (C = n_rungs + 2 n_targets; the target-target blocks of targets
// from different chunks are NaN), column_counts[C], ln_z / mean_e[n_targets] (may be nullptr).  With an empty rung
// (p.empty_rung) nothing else is computed.
hipError_t mbar_gram(Problem &p, const Source &src, const double *f, const double *temps, int n_targets, double *gram,
                     double *column_counts, double *ln_z, double *mean_e) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const MbarSamples &sm = p.sm;
  const int n_rungs = p.n_rungs;
  hipStream_t stream = p.stream;
  // the used samples alone, in their order (the rungs are in the counts already)
  MbarSamples packed_samples{sm.energies, nullptr, p.n_used_ll, 1, 1};
  DeviceBuffer packed, tile_counts, tile_offsets;
  if (p.n_used_ll != sm.n_samples) {
    const long long all_tiles = tiles_of(sm.n_samples);
    ME_MBAR_HIP(packed.resize((size_t)p.n_used_ll * sizeof(double)));
    ME_MBAR_HIP(tile_counts.resize((size_t)all_tiles * sizeof(unsigned int)));
    ME_MBAR_HIP(tile_offsets.resize((size_t)all_tiles * sizeof(long long)));
    hipLaunchKernelGGL(k_mbar_used_tiles, dim3((unsigned)all_tiles), dim3(kThreads), 0, stream, sm.energies, sm.n_samples,
                       tile_counts.get<unsigned int>());
    hipLaunchKernelGGL(k_mbar_scan, dim3(1), dim3(kThreads), 0, stream, tile_counts.get<const unsigned int>(), all_tiles,
                       tile_offsets.get<long long>());
    hipLaunchKernelGGL(k_mbar_compact, dim3((unsigned)all_tiles), dim3(kThreads), 0, stream, sm.energies, sm.n_samples,
                       tile_offsets.get<const long long>(), packed.get<double>());
    ME_MBAR_HIP(hipGetLastError());
    packed_samples.energies = packed.get<double>();
  }
  const MbarSamples &ps = packed_samples;
  std::vector<double> inv;                                        // (on its way to the device until the wait below)
  if (n_targets > 0) ME_MBAR_HIP(reweight_enqueue(p, ps, temps, n_targets, inv));
  const int n_blocks = blocks_of(ps.n_samples);
  const long long n_tiles = tiles_of(ps.n_samples);
  const int per_chunk = (kMaxCols - n_rungs) / 2;                 // targets of one pass: K + 2 per_chunk <= kMaxCols
  const int n_chunks = std::max(1, (n_targets + per_chunk - 1) / per_chunk);
  const int max_cols = n_rungs + 2 * std::min(n_targets, per_chunk);
  DeviceBuffer minima, cols, chunk_partials, dense;
  ME_MBAR_HIP(minima.resize((size_t)n_blocks * sizeof(double)));
  ME_MBAR_HIP(cols.resize(kColDoubles * sizeof(double)));
  ME_MBAR_HIP(chunk_partials.resize((size_t)n_blocks * (size_t)(max_cols * (max_cols + 1) / 2) * sizeof(double)));
  ME_MBAR_HIP(dense.resize((size_t)n_chunks * kMaxCols * kMaxCols * sizeof(double)));
  hipLaunchKernelGGL(k_mbar_min, dim3(n_blocks), dim3(kThreads), 0, stream, ps.energies, ps.n_samples, n_tiles, minima.get<double>());
  for (int c = 0; c < n_chunks; ++c) {
    const int t0 = c * per_chunk, nt = std::min(per_chunk, n_targets - t0), n_cols = n_rungs + 2 * nt, cp = padded_row(n_cols);
    hipLaunchKernelGGL(k_mbar_gram_columns, dim3(1), dim3(kMaxCols), 0, stream, w.table.get<const double>(), n_rungs,
                       n_targets > 0 ? w.inv_temps.get<const double>() + t0 : nullptr,
                       n_targets > 0 ? w.out.get<const double>() + 4 * (size_t)t0 : nullptr, nt, minima.get<const double>(), n_blocks,
                       cols.get<double>());
    hipLaunchKernelGGL(k_mbar_gram, dim3(n_blocks), dim3(kThreads), 2 * kSub * cp * sizeof(double), stream, ps.energies, ps.n_samples,
                       n_rungs, w.table.get<const double>(), cols.get<const double>(), n_cols, cp, n_tiles, chunk_partials.get<double>());
    hipLaunchKernelGGL(k_mbar_gram_finish, dim3(n_cols), dim3(kMaxCols), 0, stream, chunk_partials.get<const double>(), n_blocks, n_cols,
                       dense.get<double>() + (size_t)c * kMaxCols * kMaxCols);
  }
  ME_MBAR_HIP(hipGetLastError());
  std::vector<double> host((size_t)n_chunks * kMaxCols * kMaxCols), out(4 * (size_t)n_targets);
  ME_MBAR_HIP(hipMemcpyAsync(host.data(), dense.get(), host.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (n_targets > 0) ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  ME_MBAR_HIP(hipStreamSynchronize(stream));
  const int n_all = n_rungs + 2 * n_targets;
  std::fill(gram, gram + (size_t)n_all * n_all, (double)NAN);
  for (int c = 0; c < n_chunks; ++c) {
    const int t0 = c * per_chunk, nt = std::min(per_chunk, n_targets - t0), n_cols = n_rungs + 2 * nt;
    const double *chunk = host.data() + (size_t)c * kMaxCols * kMaxCols;
    auto global = [&](int l) { return l < n_rungs ? l : l + 2 * t0; };
    for (int i = 0; i < n_cols; ++i)
      for (int j = 0; j < n_cols; ++j) gram[(size_t)global(i) * n_all + global(j)] = chunk[i * n_cols + j];
  }
  for (int k = 0; k < n_all; ++k) column_counts[k] = k < n_rungs ? (double)p.counts[k] : 0.0;
  unpack_targets(out, n_targets, ln_z, mean_e, nullptr, nullptr);
  return hipSuccess;
}

// *shift = E_shift of the samples: the block minima, then the one-block kernel that the Gram pass itself takes it from
hipError_t energy_shift(const MbarSamples &sm, double *shift, hipStream_t stream) {
  const int n_blocks = blocks_of(sm.n_samples);
  DeviceBuffer minima, cols;
  ME_MBAR_HIP(minima.resize((size_t)n_blocks * sizeof(double)));
  ME_MBAR_HIP(cols.resize(kColDoubles * sizeof(double)));
  hipLaunchKernelGGL(k_mbar_min, dim3(n_blocks), dim3(kThreads), 0, stream, sm.energies, sm.n_samples, tiles_of(sm.n_samples),
                     minima.get<double>());
  hipLaunchKernelGGL(k_mbar_gram_columns, dim3(1), dim3(kMaxCols), 0, stream, (const double *)nullptr, 0, (const double *)nullptr,
                     (const double *)nullptr, 0, minima.get<const double>(), n_blocks, cols.get<double>());
  ME_MBAR_HIP(hipGetLastError());
  ME_MBAR_HIP(hipMemcpyAsync(shift, cols.get<double>() + kColShift, sizeof(double), hipMemcpyDeviceToHost, stream));
  return hipStreamSynchronize(stream);
}

// the two forms of me_mbar_gram behind their Source
int gram_common(const Source &src, const double *f, const double *temps, int n_targets, double *gram, double *column_counts,
                double *ln_z, double *mean_e, int64_t *n_used) {
  if (!gram || !column_counts) return fail(src.e, ME_ERR_INVALID, "gram and column_counts are needed");
  // (only the first kK entries of f are looked at before the number of rungs is refused)
  int rc = check_f_and_targets(src.e, f, std::min(src.n_rungs, kK), temps, n_targets, 0);
  if (rc) return rc;
  Problem p;
  rc = mbar_check_common(src.e, p, mbar_gram(p, src, f, temps, n_targets, gram, column_counts, ln_z, mean_e));
  if (rc) return rc;
  if (n_used) *n_used = p.n_used_ll;
  return ME_OK;
}

}  // namespace
}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_mbar_gram(me_engine *e, const double *f, const double *temps, int32_t n_targets, double *gram, double *column_counts,
                 double *ln_z, double *mean_e, int64_t *n_used) {
  Source src;
  const int rc = src.from_engine(e);
  return rc ? rc : gram_common(src, f, temps, n_targets, gram, column_counts, ln_z, mean_e, n_used);
}

int me_mbar_energy_shift(me_engine *e, double *shift) {
  if (!e) return ME_ERR_INVALID;
  if (!shift) return fail(e, ME_ERR_INVALID, "shift missing");
  Source src;
  const int rc = src.from_engine(e);
  if (rc) return rc;
  ME_HIP(e, energy_shift(src.sm, shift, src.stream));
  if (!std::isfinite(*shift)) return fail(e, ME_ERR_STATE, "no recorded sample has a finite energy");
  return ME_OK;
}

int me_mbar_gram_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                         const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n_targets,
                         double *gram, double *column_counts, double *ln_z, double *mean_e, int64_t *n_used) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs);
  return rc ? rc : src.finish(gram_common(src, f, temps, n_targets, gram, column_counts, ln_z, mean_e, n_used));
}

}  // extern "C"
