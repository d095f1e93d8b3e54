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
//
// The observable form (me_mbar_gram_observables and its engine-less twin): error bars for the reweighted means of the Q <= 16
// recorded columns A_q (ObsColumns: an engine's store or host columns).  C = K + n_targets (1 + Q):
//     state column of target t         W_na as above                                          column K + t (1 + Q),         count 0
//     observable column q of target t  W_nA = W_na (A_qn - S_q) / (mean_tq - S_q)               column K + t (1 + Q) + 1 + q, count 0
// S_q = (the least finite value of column q over the used samples) - 1, so that every factor is >= 1 (a zero-mean observable
// is no special case), and mean_tq is what the observable reweighting kernels (me_mbar_obs.hip) leave on the device.  A column
// whose mean_tq is not finite (a non-finite A_q in a used sample) gets a NaN normaliser: its row and column of G are NaN and
// no other entry changes.  Targets go in chunks of (128 - K) / (1 + Q), at least 3, every chunk with the ladder columns.
// Kernels: k_mbar_compact also packs the columns of the used samples ([Q][n_used]); k_mbar_min_columns (grid (blocks, Q)) is
// k_mbar_min per column; k_mbar_gram_obs_columns (one block) is k_mbar_gram_columns with, per column of W, the observable it
// carries (-1: none), its shift and its normaliser; k_mbar_gram<Form::kObs> is k_mbar_gram<Form::kEnergy> (the energy form's)
// with two additions: per 256 samples every lane parks the Q values of its sample in LDS beside (E_n, d_n), as [Q][257]
// doubles -- the fill threads of a half-wavefront read 2 rows x 16 columns, that is observables q .. q + 15 of samples s, s + 1;
// with the odd stride 257 value (q, s) lies in bank 2 (q + s) mod 64 for the 8-byte reads, so only pairs with equal q + s
// collide (two-way), where the stride 256 would put all sixteen observables of a sample on one bank -- and the fill multiplies
// the exponential by (A_qn - S_q) / (mean_tq - S_q).  The MFMA loop, the tile assignment and the summation order are the same
// code, so an entry that pairs ladder and state columns has the bits the energy form gives it, and an observable column has the
// same bits alone as among 16.
//
// The fluctuation form (me_mbar_gram_fluctuations and its engine-less twin): error bars for the reweighted SECOND moments, the
// energy variance (heat capacity) and the variance and energy covariance (d<A_q>/dT) of the Q <= 16 recorded columns; Q = 0 is
// the heat capacity alone from the energy store alone.  With E' = E_n - E_shift and A'_q = A_qn - S_q, the shifts of the two
// forms above (every E', A'_q >= 1, so every product is >= 1 and every entry of W >= 0), C = K + n_targets (3 + 3 Q):
//     state column of target t   W_na                                                 column K + t (3 + 3 Q)
//     E1, E2                     W_na E' / m_E,  W_na E' E' / (var_e + m_E^2)            the next two; m_E = mean_e - E_shift
//     A1_q, A2_q, AE_q           W_na A'_q / m_q,  W_na A'_q A'_q / (var_tq + m_q^2),  W_na A'_q E' / (cov_energy_tq + m_q m_E)
//                                                                                     columns K + t (3 + 3 Q) + 3 + 3 q ...; m_q = mean_tq - S_q
// The normalisers are the reweighted moments of the factors, formed in k_mbar_gram_fluct_columns (one block) from what the
// reweighting kernels (me_mbar.hip, me_mbar_obs.hip) leave on the device, and returned as `moments`; an observable with a
// non-finite mean, variance or covariance gets NaN for all three (its rows and columns of G are NaN, no other entry changes).
// The host's delta method on Theta is in statistics.py.  Targets go in chunks of (128 - K) / (3 + 3 Q), at least 1.  The products
// are formed in registers in the fill: Form::kFluct of k_mbar_gram is the observable form's kernel (the same parking of the Q
// values, skipped when Q = 0) whose column constants also carry a kind (state, E1, E2, A1, A2, AE) and E_shift, and whose fill
// multiplies the exponential by w * x / norm with x = E' (the energy form's expression), A' (the observable form's), E' * E',
// A' * A' or A' * E'.  The MFMA loop, the tile assignment, the summation order, the packing and k_mbar_gram_finish are shared, so
// the entries among ladder, state and E1 columns have the energy form's bits and those among ladder, state and A1 columns the
// observable form's.  The machine code of the two other instantiations is the one they had before this form existed.
// LDS per block: [2][16][Cp] sub-tile buffers (36 KiB at C = 128), 4 KiB (E_n, d_n), 3 KiB column constants; the observable form
// adds Q x 257 x 8 bytes (32.1 KiB at Q = 16) and 1.5 KiB of column constants: 76.6 KiB at C = 128, Q = 16, which needs the
// raised dynamic-LDS limit and lets two blocks share a CU's 160 KiB (2 wavefronts per SIMD); 46.5 KiB at Q = 1 (3 blocks).  The
// fluctuation form adds 0.5 KiB of kinds to that: 77.1 KiB at C = 128, Q = 16 (still two blocks per CU), 45 KiB at Q = 0.
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_mbar_gram<Form::kEnergy> 93 VGPRs + 72 AGPRs (the
// accumulators), 3 wavefronts per SIMD, no scratch; k_mbar_gram<Form::kObs> 95 VGPRs + 72 AGPRs, 3 wavefronts per SIMD by
// registers (2 where the LDS of 16 observables decides), no scratch; k_mbar_gram<Form::kFluct> 95 VGPRs + 72 AGPRs, 106 SGPRs,
// 9 216 bytes of static LDS, 3 wavefronts per SIMD by registers, no scratch; no other kernel of this file uses scratch.
#include "me_launch.h"
#include "me_mbar.h"
#include "me_mbar_gram_tiles.h"

namespace me {
namespace mbar {
namespace {

constexpr int kMaxCols = 128;                   // columns of W per launch
constexpr int kSlots = 9;                       // 16 x 16 tiles of G per wavefront: 36 lower-triangle tiles / 4
constexpr int kColB = 0, kColG = kMaxCols, kColMean = 2 * kMaxCols, kColShift = 3 * kMaxCols, kColDoubles = 3 * kMaxCols + 1;
// the observable form's column constants: [b | g | normaliser | shift of the column | observable of the column, -1: none], then S_q
constexpr int kColOwnShift = 3 * kMaxCols, kColWhich = 4 * kMaxCols, kColShifts = 5 * kMaxCols;
constexpr int kObsColDoubles = 5 * kMaxCols + ME_MAX_RECORDED_OBSERVABLES;
constexpr int kObsStride = kThreads + 1;        // doubles between two observables of the parked samples (odd: see the header)
// the fluctuation form's column constants: the observable form's five arrays, then the kind of the column, then S_q and E_shift
constexpr int kColKind = 5 * kMaxCols, kFluctShifts = 6 * kMaxCols, kFluctEnergyShift = 6 * kMaxCols + ME_MAX_RECORDED_OBSERVABLES;
constexpr int kFluctColDoubles = kFluctEnergyShift + 1;
// the factor a column of the fluctuation form puts on the state weight: none, E', E'^2, A', A'^2, A' E'
enum Kind : int { kState = 0, kE1, kE2, kA1, kA2, kAE };
// the three forms of k_mbar_gram
enum class Form { kEnergy, kObs, kFluct };

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

// the finite energies of tile blockIdx.x, in their order, to packed[offsets[tile] ..), and the columns `oc` of those samples
// (oc.n_columns = 0: none) to packed_columns[column][n_used]
__global__ void __launch_bounds__(kThreads) k_mbar_compact(const double *__restrict__ energies, long long n,
                                                           const long long *__restrict__ offsets, double *packed, ObsColumns oc,
                                                           double *packed_columns, long long n_used) {
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
    if (isfinite(e[r])) {
      const long long to = at + before + rank[r];
      packed[to] = e[r];
      if (oc.n_columns > 0) {
        const double *from = oc.data + obs_offset(oc, (long long)blockIdx.x * kTile + (long long)r * kThreads + threadIdx.x);
        for (int q = 0; q < oc.n_columns; ++q) packed_columns[(long long)q * n_used + to] = from[(long long)q * oc.column_stride];
      }
    }
    at += all;
  }
}

// *dst = the least of the block's v
__device__ __forceinline__ void block_min_store(double v, double *dst) {
  __shared__ double waves[kWaves];
  v = wave_min(v);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *dst = fmin(fmin(waves[0], waves[1]), fmin(waves[2], waves[3]));
}

// minima[block] = the least finite energy of the block's tiles (+inf when it has none)
__global__ void __launch_bounds__(kThreads) k_mbar_min(const double *__restrict__ energies, long long n, long long n_tiles,
                                                       double *minima) {
  double v = INFINITY;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    for (int r = 0; r < kItems; ++r) {
      const long long i = tile * kTile + (long long)r * kThreads + threadIdx.x;
      const double e = i < n ? energies[i] : NAN;
      if (isfinite(e)) v = fmin(v, e);
    }
  block_min_store(v, minima + blockIdx.x);
}

// minima[column][block] = the least finite value of column blockIdx.y over the block's tiles; grid (blocks, columns)
__global__ void __launch_bounds__(kThreads) k_mbar_min_columns(ObsColumns oc, long long n, long long n_tiles, double *minima) {
  const double *column = oc.data + (long long)blockIdx.y * oc.column_stride;
  double v = INFINITY;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    for (int r = 0; r < kItems; ++r) {
      const long long i = tile * kTile + (long long)r * kThreads + threadIdx.x;
      const double a = i < n ? column[obs_offset(oc, i)] : NAN;
      if (isfinite(a)) v = fmin(v, a);
    }
  block_min_store(v, minima + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// the least of minima[0 .. n_blocks), in every thread of a block of kMaxCols
__device__ __forceinline__ double least_of_blocks(const double *__restrict__ minima, int n_blocks, double *part) {
  double v = INFINITY;
  for (int b = threadIdx.x; b < n_blocks; b += kMaxCols) v = fmin(v, minima[b]);
  part[threadIdx.x] = v;
  __syncthreads();
  v = part[0];
  for (int k = 1; k < kMaxCols; ++k) v = fmin(v, part[k]);
  return v;
}

// cols = [b | g | mean | E_shift] of the K ladder columns and of the two columns of each of n_targets temperatures, whose
// (ln_z, mean_e, ., .) the reweighting kernels left in `out`
__global__ void __launch_bounds__(kMaxCols) k_mbar_gram_columns(const double *__restrict__ table, int n_rungs,
                                                                const double *__restrict__ inv_temps,
                                                                const double *__restrict__ out, int n_targets,
                                                                const double *__restrict__ minima, int n_blocks, double *cols) {
  __shared__ double part[kMaxCols];
  const double shift = least_of_blocks(minima, n_blocks, part) - 1.0;
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

// The observable form's cols = [b | g | normaliser | shift | observable] of the K ladder columns and of the 1 + nq columns of
// each of n_targets temperatures, then S_q: (ln_z, ., ., .) of the targets in `out`, the reweighted means [n_targets][nq] in
// `means`, both as the reweighting kernels left them; minima is [nq][n_blocks]
__global__ void __launch_bounds__(kMaxCols) k_mbar_gram_obs_columns(const double *__restrict__ table, int n_rungs,
                                                                    const double *__restrict__ inv_temps,
                                                                    const double *__restrict__ out, const double *__restrict__ means,
                                                                    int nq, int n_targets, const double *__restrict__ minima,
                                                                    int n_blocks, double *cols) {
  __shared__ double part[kMaxCols], shifts[ME_MAX_RECORDED_OBSERVABLES];
  for (int q = 0; q < nq; ++q) {
    const double least = least_of_blocks(minima + (size_t)q * n_blocks, n_blocks, part);
    if (threadIdx.x == 0) shifts[q] = least - 1.0;
    __syncthreads();                                             // (`part` is written again)
  }
  const int c = threadIdx.x;
  double b = 0.0, g = 0.0, mean = 0.0, shift = 0.0, which = -1.0;
  if (c < n_rungs) {
    b = table[kBeta + c];
    g = table[kF + c];
  } else if (c < n_rungs + (1 + nq) * n_targets) {
    const int t = (c - n_rungs) / (1 + nq), j = (c - n_rungs) - t * (1 + nq);
    b = inv_temps[t];
    g = -out[4 * t];
    if (j > 0) {
      const double m = means[t * nq + j - 1];
      which = (double)(j - 1);
      shift = shifts[j - 1];
      mean = isfinite(m) ? m - shift : NAN;                      // (NaN: the whole column of W, and its row and column of G)
    }
  }
  cols[kColB + c] = b;
  cols[kColG + c] = g;
  cols[kColMean + c] = mean;
  cols[kColOwnShift + c] = shift;
  cols[kColWhich + c] = which;
  if (c < nq) cols[kColShifts + c] = shifts[c];
}

// The fluctuation form's cols = [b | g | normaliser | shift | observable | kind] of the K ladder columns and of the 3 + 3 nq
// columns (state, E1, E2, then A1, A2, AE of each observable) of each of n_targets temperatures, then S_q and E_shift.  (ln_z,
// mean_e, var_e, .) of the targets in `out`; obs = [mean | var | cov_energy], each [.][nq] from these targets on and obs_part
// doubles after the one before, all as the reweighting kernels left them (nq = 0: never read); e_minima is [n_blocks], a_minima
// [nq][n_blocks].  moments[n_targets][2 + 3 nq] = the normalisers in column order.  A non-finite mean, variance or covariance
// of observable q gives its three columns a NaN normaliser.
__global__ void __launch_bounds__(kMaxCols) k_mbar_gram_fluct_columns(const double *__restrict__ table, int n_rungs,
                                                                      const double *__restrict__ inv_temps,
                                                                      const double *__restrict__ out, const double *__restrict__ obs,
                                                                      long long obs_part, int nq, int n_targets,
                                                                      const double *__restrict__ e_minima,
                                                                      const double *__restrict__ a_minima, int n_blocks,
                                                                      double *cols, double *moments) {
  __shared__ double part[kMaxCols], shifts[ME_MAX_RECORDED_OBSERVABLES];
  const double e_shift = least_of_blocks(e_minima, n_blocks, part) - 1.0;
  __syncthreads();                                               // (`part` is written again)
  for (int q = 0; q < nq; ++q) {
    const double least = least_of_blocks(a_minima + (size_t)q * n_blocks, n_blocks, part);
    if (threadIdx.x == 0) shifts[q] = least - 1.0;
    __syncthreads();
  }
  const int c = threadIdx.x, per = 3 + 3 * nq;
  double b = 0.0, g = 0.0, norm = 0.0, shift = 0.0, which = -1.0;
  int kind = kState;
  if (c < n_rungs) {
    b = table[kBeta + c];
    g = table[kF + c];
  } else if (c < n_rungs + per * n_targets) {
    const int t = (c - n_rungs) / per, j = (c - n_rungs) - t * per;
    b = inv_temps[t];
    g = -out[4 * t];
    const double m_e = out[4 * t + 1] - e_shift;                 // >= 1
    if (j == 1 || j == 2) {
      kind = j == 1 ? kE1 : kE2;
      norm = j == 1 ? m_e : __builtin_fma(m_e, m_e, out[4 * t + 2]);
    } else if (j >= 3) {
      const int q = (j - 3) / 3;
      const double mean = obs[t * nq + q], var = obs[obs_part + t * nq + q], cov = obs[2 * obs_part + t * nq + q];
      kind = kA1 + (j - 3) - 3 * q;
      which = (double)q;
      shift = shifts[q];
      const double m_q = mean - shift;
      norm = kind == kA1 ? m_q : kind == kA2 ? __builtin_fma(m_q, m_q, var) : __builtin_fma(m_q, m_e, cov);
      if (!(isfinite(mean) && isfinite(var) && isfinite(cov))) norm = NAN;   // (the three columns of W, their rows and columns of G)
    }
    if (j >= 1) moments[t * (per - 1) + j - 1] = norm;
  }
  cols[kColB + c] = b;
  cols[kColG + c] = g;
  cols[kColMean + c] = norm;
  cols[kColOwnShift + c] = shift;
  cols[kColWhich + c] = which;
  cols[kColKind + c] = (double)kind;
  if (c < nq) cols[kFluctShifts + c] = shifts[c];
  if (c == 0) cols[kFluctEnergyShift] = e_shift;
}

// partials[block] = the packed lower triangle of the block's part of W^T W, n_cols <= kMaxCols columns.  Form::kEnergy: n_cols =
// K + 2 n_targets, `oc` unused; Form::kObs: the observable form, n_cols = K + (1 + Q) n_targets, `cols` of
// k_mbar_gram_obs_columns; Form::kFluct: the fluctuation form, n_cols = K + (3 + 3 Q) n_targets, `cols` of
// k_mbar_gram_fluct_columns, Q = oc.n_columns may be 0 (`oc` and the observables' LDS are then never touched).  Dynamic LDS: 2 *
// kSub * cp doubles, cp the padded row length (see the header of this file), and in the forms with observables oc.n_columns *
// kObsStride more.
template <Form kForm>
__global__ void __launch_bounds__(kThreads) k_mbar_gram(const double *__restrict__ energies, long long n, int n_rungs,
                                                        const double *__restrict__ table, const double *__restrict__ cols,
                                                        int n_cols, int cp, long long n_tiles, double *partials, ObsColumns oc) {
  constexpr bool kObs = kForm == Form::kObs, kFluct = kForm == Form::kFluct;
  extern __shared__ double w_lds[];                              // [2][kSub][cp], then s_a [Q][kObsStride]
  __shared__ double s_e[kThreads], s_d[kThreads], c_b[kMaxCols], c_g[kMaxCols], c_mean[kMaxCols];
  __shared__ double c_shift[kObs || kFluct ? kMaxCols : 1];
  __shared__ int c_which[kObs || kFluct ? kMaxCols : 1];
  __shared__ int c_kind[kFluct ? kMaxCols : 1];
  double *const s_a = w_lds + 2 * kSub * cp;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const Fragment fr = fragment_of(lane);                         // the MFMA's (k, i / j) of this lane
  const int j16 = fr.j16;
  const int tn = (n_cols + 15) >> 4, n_pairs = tn * (tn + 1) / 2;
  if (t < kMaxCols) {
    c_b[t] = cols[kColB + t];
    c_g[t] = cols[kColG + t];
    c_mean[t] = cols[kColMean + t];
    if constexpr (kObs || kFluct) {
      c_shift[t] = cols[kColOwnShift + t];
      c_which[t] = (int)cols[kColWhich + t];
    }
    if constexpr (kFluct) c_kind[t] = (int)cols[kColKind + t];
  }
  const double shift = kObs ? 0.0 : cols[kFluct ? kFluctEnergyShift : kColShift];
  // this wavefront's tiles: pair p = wave + 4 s = I (I + 1) / 2 + J, column offsets 16 I and 16 J
  int off_i[kSlots], off_j[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    pair_offsets(wave + kWaves * s, kMaxCols / 16, off_i[s], off_j[s]);
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
      if constexpr (kObs || kFluct) {
        if (i < n && (kObs || oc.n_columns > 0)) {               // (the fluctuation form without observables: nothing to park)
          // (the record of the step's first sample is wave-uniform: the division stays off the vector registers)
          long long record = (i - t) / oc.n_chains, chain = (i - t) - record * oc.n_chains + t;
          while (chain >= oc.n_chains) {
            chain -= oc.n_chains;
            record += 1;
          }
          const double *a = oc.data + record * oc.record_stride + chain;
          for (int c = 0; c < oc.n_columns; ++c) s_a[c * kObsStride + t] = a[(long long)c * oc.column_stride];
        }
      }
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
              if constexpr (kObs) {
                const int which = c_which[col];
                if (which >= 0) w = w * (s_a[which * kObsStride + q * kSub + row] - c_shift[col]) / c_mean[col];
              } else if constexpr (kFluct) {
                const int kind = c_kind[col];
                if (kind != kState) {
                  const int which = c_which[col];
                  const double e1 = es - shift;
                  const double a1 = which >= 0 ? s_a[which * kObsStride + q * kSub + row] - c_shift[col] : 0.0;
                  // E1 and A1 are the energy form's and the observable form's expressions; the others w * (x * y) / norm
                  const double factor = kind == kE1 ? e1 : kind == kE2 ? e1 * e1 : kind == kA1 ? a1 : kind == kA2 ? a1 * a1 : a1 * e1;
                  w = w * factor / c_mean[col];
                }
              } else {
                const double mean = c_mean[col];
                if (mean != 0.0) w = w * (es - shift) / mean;
              }
            }
            buf[row * cp + col] = w;
          }
        }
        __syncthreads();
#pragma unroll 2
        for (int ks = 0; ks < kSub / 4; ++ks) {
          const double *src = fragment_source(buf, ks, cp, fr);
#pragma unroll
          for (int s = 0; s < kSlots; ++s)
            if (wave + kWaves * s < n_pairs)                      // (wave-uniform)
              acc[s] = gram_mfma(src[off_i[s]], src[off_j[s]], acc[s]);
        }
        parity ^= 1;                                             // the next fill goes to the other buffer: no second barrier
      }
    }
  }
  double *dst = partials + (size_t)blockIdx.x * (size_t)(n_cols * (n_cols + 1) / 2);
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    if (wave + kWaves * s >= n_pairs) continue;
    store_lower_tile(dst, off_i[s], off_j[s], fr, n_cols, acc[s]);
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
// The used samples of a problem alone, in their order, with their observable columns (the rungs are in the counts already):
// the problem's own arrays when every energy is finite, a packed copy otherwise.
struct UsedSamples {
  MbarSamples sm{};
  ObsColumns oc{};
  DeviceBuffer energies, columns, tile_counts, tile_offsets;
};
hipError_t pack_used(const Problem &p, const ObsColumns &oc, UsedSamples &u) {
  const MbarSamples &sm = p.sm;
  u.sm = MbarSamples{sm.energies, nullptr, p.n_used_ll, 1, 1};
  u.oc = oc;
  if (p.n_used_ll == sm.n_samples) return hipSuccess;
  const long long all_tiles = tiles_of(sm.n_samples);
  ME_MBAR_HIP(u.energies.resize((size_t)p.n_used_ll * sizeof(double)));
  ME_MBAR_HIP(u.columns.resize((size_t)p.n_used_ll * (size_t)oc.n_columns * sizeof(double)));
  ME_MBAR_HIP(u.tile_counts.resize((size_t)all_tiles * sizeof(unsigned int)));
  ME_MBAR_HIP(u.tile_offsets.resize((size_t)all_tiles * sizeof(long long)));
  hipLaunchKernelGGL(k_mbar_used_tiles, dim3((unsigned)all_tiles), dim3(kThreads), 0, p.stream, sm.energies, sm.n_samples,
                     u.tile_counts.get<unsigned int>());
  hipLaunchKernelGGL(k_mbar_scan, dim3(1), dim3(kThreads), 0, p.stream, u.tile_counts.get<const unsigned int>(), all_tiles,
                     u.tile_offsets.get<long long>());
  hipLaunchKernelGGL(k_mbar_compact, dim3((unsigned)all_tiles), dim3(kThreads), 0, p.stream, sm.energies, sm.n_samples,
                     u.tile_offsets.get<const long long>(), u.energies.get<double>(), oc, u.columns.get<double>(), p.n_used_ll);
  ME_MBAR_HIP(hipGetLastError());
  u.sm.energies = u.energies.get<double>();
  if (oc.n_columns > 0) u.oc = ObsColumns{u.columns.get<const double>(), oc.n_columns, p.n_used_ll, 0, p.n_used_ll};
  return hipSuccess;
}

// The Gram matrix of a weight matrix of n_rungs + per_target n_targets columns over n_samples samples, in chunks of targets
// that each carry the ladder columns.  launch(t0, nt, n_cols, cp, partials) enqueues the column constants and the Gram kernel
// of the nt targets from t0 (n_cols = n_rungs + per_target nt columns, padded row cp); copy_results() enqueues the copies of
// whatever else the caller returns.  Waits for the stream and writes gram[C][C] (the target-target blocks of targets from
// different chunks are NaN) and column_counts[C].
template <class Launch, class Copy>
hipError_t gram_chunks(Problem &p, long long n_samples, int per_target, int n_targets, double *gram, double *column_counts,
                       Launch launch, Copy copy_results) {
  const int n_rungs = p.n_rungs, n_blocks = blocks_of(n_samples);
  hipStream_t stream = p.stream;
  const int per_chunk = (kMaxCols - n_rungs) / per_target;        // targets of one pass: K + per_target per_chunk <= kMaxCols
  const int n_chunks = std::max(1, (n_targets + per_chunk - 1) / per_chunk);
  const int max_cols = n_rungs + per_target * std::min(n_targets, per_chunk);
  DeviceBuffer chunk_partials, dense;
  ME_MBAR_HIP(chunk_partials.resize((size_t)n_blocks * (size_t)(max_cols * (max_cols + 1) / 2) * sizeof(double)));
  ME_MBAR_HIP(dense.resize((size_t)n_chunks * kMaxCols * kMaxCols * sizeof(double)));
  for (int c = 0; c < n_chunks; ++c) {
    const int t0 = c * per_chunk, nt = std::min(per_chunk, n_targets - t0), n_cols = n_rungs + per_target * nt;
    ME_MBAR_HIP(launch(t0, nt, n_cols, padded_row(n_cols), chunk_partials.get<double>()));
    hipLaunchKernelGGL(k_mbar_gram_finish, dim3(n_cols), dim3(kMaxCols), 0, stream, chunk_partials.get<const double>(), n_blocks, n_cols,
                       dense.get<double>() + (size_t)c * kMaxCols * kMaxCols);
  }
  ME_MBAR_HIP(hipGetLastError());
  std::vector<double> host((size_t)n_chunks * kMaxCols * kMaxCols);
  ME_MBAR_HIP(hipMemcpyAsync(host.data(), dense.get(), host.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  ME_MBAR_HIP(copy_results());
  ME_MBAR_HIP(hipStreamSynchronize(stream));
  const int n_all = n_rungs + per_target * n_targets;
  std::fill(gram, gram + (size_t)n_all * n_all, (double)NAN);
  for (int c = 0; c < n_chunks; ++c) {
    const int t0 = c * per_chunk, nt = std::min(per_chunk, n_targets - t0), n_cols = n_rungs + per_target * nt;
    const double *chunk = host.data() + (size_t)c * kMaxCols * kMaxCols;
    auto global = [&](int l) { return l < n_rungs ? l : l + per_target * t0; };
    for (int i = 0; i < n_cols; ++i)
      for (int j = 0; j < n_cols; ++j) gram[(size_t)global(i) * n_all + global(j)] = chunk[i * n_cols + j];
  }
  for (int k = 0; k < n_all; ++k) column_counts[k] = k < n_rungs ? (double)p.counts[k] : 0.0;
  return hipSuccess;
}

}  // namespace

// Waits for the stream and writes host arrays: gram[C][C] (C = n_rungs + 2 n_targets), column_counts[C], ln_z /
// mean_e[n_targets] (may be nullptr).  With an empty rung (p.empty_rung) nothing else is computed.  (Declared in me_mbar.h:
// me_mbar_hist_cov.hip takes its ladder block from here.)
hipError_t mbar_gram(Problem &p, const Source &src, const double *f, const double *temps, int n_targets, double *gram,
                     double *column_counts, double *ln_z, double *mean_e) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const int n_rungs = p.n_rungs;
  hipStream_t stream = p.stream;
  UsedSamples used;
  ME_MBAR_HIP(pack_used(p, ObsColumns{}, used));
  const MbarSamples &ps = used.sm;
  std::vector<double> inv;                                        // (on its way to the device until the wait in gram_chunks)
  if (n_targets > 0) ME_MBAR_HIP(reweight_enqueue(p, ps, temps, n_targets, inv));
  const int n_blocks = blocks_of(ps.n_samples);
  const long long n_tiles = tiles_of(ps.n_samples);
  DeviceBuffer minima, cols;
  ME_MBAR_HIP(minima.resize((size_t)n_blocks * sizeof(double)));
  ME_MBAR_HIP(cols.resize(kColDoubles * sizeof(double)));
  hipLaunchKernelGGL(k_mbar_min, dim3(n_blocks), dim3(kThreads), 0, stream, ps.energies, ps.n_samples, n_tiles, minima.get<double>());
  std::vector<double> out(4 * (size_t)n_targets);
  ME_MBAR_HIP(gram_chunks(
      p, ps.n_samples, 2, n_targets, gram, column_counts,
      [&](int t0, int nt, int n_cols, int cp, double *partials) {
        hipLaunchKernelGGL(k_mbar_gram_columns, dim3(1), dim3(kMaxCols), 0, stream, w.table.get<const double>(), n_rungs,
                           n_targets > 0 ? w.inv_temps.get<const double>() + t0 : nullptr,
                           n_targets > 0 ? w.out.get<const double>() + 4 * (size_t)t0 : nullptr, nt, minima.get<const double>(),
                           n_blocks, cols.get<double>());
        hipLaunchKernelGGL(k_mbar_gram<Form::kEnergy>, dim3(n_blocks), dim3(kThreads), 2 * kSub * cp * sizeof(double), stream, ps.energies,
                           ps.n_samples, n_rungs, w.table.get<const double>(), cols.get<const double>(), n_cols, cp, n_tiles, partials,
                           ObsColumns{});
        return hipSuccess;
      },
      [&] {
        if (n_targets == 0) return hipSuccess;
        return hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, stream);
      }));
  unpack_targets(out, n_targets, ln_z, mean_e, nullptr, nullptr);
  return hipSuccess;
}

namespace {

// The observable form: gram[C][C] and column_counts[C] with C = n_rungs + n_targets (1 + Q), ln_z[n_targets], mean[n_targets][Q]
// and shifts[Q] (the last three may be nullptr).  n_targets >= 1 and src has columns.
hipError_t mbar_gram_observables(Problem &p, const Source &src, const double *f, const double *temps, int n_targets, double *gram,
                                 double *column_counts, double *ln_z, double *mean, double *shifts) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const int n_rungs = p.n_rungs, nq = src.columns.n_columns;
  hipStream_t stream = p.stream;
  UsedSamples used;
  ME_MBAR_HIP(pack_used(p, src.columns, used));
  const MbarSamples &ps = used.sm;
  const size_t cells = (size_t)n_targets * nq;
  std::vector<double> inv;
  ObsScratch scratch;
  DeviceBuffer obs_out, minima, cols;
  ME_MBAR_HIP(reweight_enqueue(p, ps, temps, n_targets, inv));
  ME_MBAR_HIP(obs_out.resize((3 * cells + (size_t)n_targets) * sizeof(double)));
  ME_MBAR_HIP(reweight_observables_enqueue(p, ps, used.oc, w.inv_temps.get<const double>(), n_targets, scratch, obs_out.get<double>()));
  const int n_blocks = blocks_of(ps.n_samples);
  const long long n_tiles = tiles_of(ps.n_samples);
  ME_MBAR_HIP(minima.resize((size_t)nq * n_blocks * sizeof(double)));
  ME_MBAR_HIP(cols.resize(kObsColDoubles * sizeof(double)));
  ME_MBAR_HIP(raise_lds_limit<k_mbar_gram<Form::kObs>>((2 * kSub * padded_row(kMaxCols) + ME_MAX_RECORDED_OBSERVABLES * kObsStride) * sizeof(double)));
  hipLaunchKernelGGL(k_mbar_min_columns, dim3(n_blocks, nq), dim3(kThreads), 0, stream, used.oc, ps.n_samples, n_tiles, minima.get<double>());
  std::vector<double> out(4 * (size_t)n_targets), means(cells), own_shifts((size_t)nq);
  ME_MBAR_HIP(gram_chunks(
      p, ps.n_samples, 1 + nq, n_targets, gram, column_counts,
      [&](int t0, int nt, int n_cols, int cp, double *partials) {
        hipLaunchKernelGGL(k_mbar_gram_obs_columns, dim3(1), dim3(kMaxCols), 0, stream, w.table.get<const double>(), n_rungs,
                           w.inv_temps.get<const double>() + t0, w.out.get<const double>() + 4 * (size_t)t0,
                           obs_out.get<const double>() + (size_t)t0 * nq, nq, nt, minima.get<const double>(), n_blocks, cols.get<double>());
        hipLaunchKernelGGL(k_mbar_gram<Form::kObs>, dim3(n_blocks), dim3(kThreads), (2 * kSub * cp + nq * kObsStride) * sizeof(double), stream,
                           ps.energies, ps.n_samples, n_rungs, w.table.get<const double>(), cols.get<const double>(), n_cols, cp, n_tiles,
                           partials, used.oc);
        return hipSuccess;
      },
      [&] {
        ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        ME_MBAR_HIP(hipMemcpyAsync(means.data(), obs_out.get(), cells * sizeof(double), hipMemcpyDeviceToHost, stream));
        return hipMemcpyAsync(own_shifts.data(), cols.get<double>() + kColShifts, own_shifts.size() * sizeof(double), hipMemcpyDeviceToHost,
                              stream);
      }));
  unpack_targets(out, n_targets, ln_z, nullptr, nullptr, nullptr);
  if (mean) std::copy(means.begin(), means.end(), mean);
  if (shifts) std::copy(own_shifts.begin(), own_shifts.end(), shifts);
  return hipSuccess;
}

// The host outputs of the fluctuation form beside gram and column_counts, each may be nullptr: ln_z, mean_e, var_e [n_targets],
// moments [n_targets][2 + 3 Q], *energy_shift, shifts [Q], mean, var, cov_energy [n_targets][Q]
struct FluctuationOutputs {
  double *ln_z, *moments, *energy_shift, *shifts, *mean_e, *var_e, *mean, *var, *cov_energy;
};

// The fluctuation form: gram[C][C] and column_counts[C] with C = n_rungs + n_targets (3 + 3 Q), Q = the columns of src (0: the
// energy columns alone), and `o`.  n_targets >= 1.
hipError_t mbar_gram_fluctuations(Problem &p, const Source &src, const double *f, const double *temps, int n_targets, double *gram,
                                  double *column_counts, const FluctuationOutputs &o) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const int n_rungs = p.n_rungs, nq = src.columns.n_columns, per = 3 + 3 * nq;
  hipStream_t stream = p.stream;
  UsedSamples used;
  ME_MBAR_HIP(pack_used(p, src.columns, used));
  const MbarSamples &ps = used.sm;
  const size_t cells = (size_t)n_targets * nq;
  std::vector<double> inv;
  ObsScratch scratch;
  DeviceBuffer obs_out, e_minima, a_minima, cols, moments_dev;
  ME_MBAR_HIP(reweight_enqueue(p, ps, temps, n_targets, inv));
  const int n_blocks = blocks_of(ps.n_samples);
  const long long n_tiles = tiles_of(ps.n_samples);
  ME_MBAR_HIP(e_minima.resize((size_t)n_blocks * sizeof(double)));
  ME_MBAR_HIP(cols.resize(kFluctColDoubles * sizeof(double)));
  ME_MBAR_HIP(moments_dev.resize((size_t)n_targets * (per - 1) * sizeof(double)));
  hipLaunchKernelGGL(k_mbar_min, dim3(n_blocks), dim3(kThreads), 0, stream, ps.energies, ps.n_samples, n_tiles, e_minima.get<double>());
  if (nq > 0) {
    ME_MBAR_HIP(obs_out.resize((3 * cells + (size_t)n_targets) * sizeof(double)));
    ME_MBAR_HIP(reweight_observables_enqueue(p, ps, used.oc, w.inv_temps.get<const double>(), n_targets, scratch, obs_out.get<double>()));
    ME_MBAR_HIP(a_minima.resize((size_t)nq * n_blocks * sizeof(double)));
    hipLaunchKernelGGL(k_mbar_min_columns, dim3(n_blocks, nq), dim3(kThreads), 0, stream, used.oc, ps.n_samples, n_tiles,
                       a_minima.get<double>());
  }
  ME_MBAR_HIP(raise_lds_limit<k_mbar_gram<Form::kFluct>>((2 * kSub * padded_row(kMaxCols) + ME_MAX_RECORDED_OBSERVABLES * kObsStride) * sizeof(double)));
  std::vector<double> out(4 * (size_t)n_targets), obs(3 * cells), moments((size_t)n_targets * (per - 1)), own_shifts((size_t)nq + 1);
  ME_MBAR_HIP(gram_chunks(
      p, ps.n_samples, per, n_targets, gram, column_counts,
      [&](int t0, int nt, int n_cols, int cp, double *partials) {
        hipLaunchKernelGGL(k_mbar_gram_fluct_columns, dim3(1), dim3(kMaxCols), 0, stream, w.table.get<const double>(), n_rungs,
                           w.inv_temps.get<const double>() + t0, w.out.get<const double>() + 4 * (size_t)t0,
                           nq > 0 ? obs_out.get<const double>() + (size_t)t0 * nq : nullptr, (long long)cells, nq, nt,
                           e_minima.get<const double>(), nq > 0 ? a_minima.get<const double>() : nullptr, n_blocks, cols.get<double>(),
                           moments_dev.get<double>() + (size_t)t0 * (per - 1));
        hipLaunchKernelGGL(k_mbar_gram<Form::kFluct>, dim3(n_blocks), dim3(kThreads), (2 * kSub * cp + nq * kObsStride) * sizeof(double),
                           stream, ps.energies, ps.n_samples, n_rungs, w.table.get<const double>(), cols.get<const double>(), n_cols, cp,
                           n_tiles, partials, used.oc);
        return hipSuccess;
      },
      [&] {
        ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        ME_MBAR_HIP(hipMemcpyAsync(moments.data(), moments_dev.get(), moments.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (nq > 0) ME_MBAR_HIP(hipMemcpyAsync(obs.data(), obs_out.get(), obs.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        // (S_q and E_shift lie one after the other when Q = 16; they are fetched separately so that any Q reads its own)
        if (nq > 0)
          ME_MBAR_HIP(hipMemcpyAsync(own_shifts.data(), cols.get<double>() + kFluctShifts, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost,
                                     stream));
        return hipMemcpyAsync(own_shifts.data() + nq, cols.get<double>() + kFluctEnergyShift, sizeof(double), hipMemcpyDeviceToHost, stream);
      }));
  unpack_targets(out, n_targets, o.ln_z, o.mean_e, o.var_e, nullptr);
  if (o.moments) std::copy(moments.begin(), moments.end(), o.moments);
  if (o.energy_shift) *o.energy_shift = own_shifts[(size_t)nq];
  if (o.shifts) std::copy(own_shifts.begin(), own_shifts.begin() + nq, o.shifts);
  if (o.mean) std::copy(obs.begin(), obs.begin() + cells, o.mean);
  if (o.var) std::copy(obs.begin() + cells, obs.begin() + 2 * cells, o.var);
  if (o.cov_energy) std::copy(obs.begin() + 2 * cells, obs.end(), o.cov_energy);
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

// the two forms of me_mbar_gram_observables behind their Source
int gram_observables_common(const Source &src, const double *f, const double *temps, int n_targets, double *gram, double *column_counts,
                            double *ln_z, double *mean, double *shifts, int64_t *n_used) {
  if (!gram || !column_counts) return fail(src.e, ME_ERR_INVALID, "gram and column_counts are needed");
  int rc = check_f_and_targets(src.e, f, std::min(src.n_rungs, kK), temps, n_targets, 1);
  if (rc) return rc;
  Problem p;
  rc = mbar_check_common(src.e, p, mbar_gram_observables(p, src, f, temps, n_targets, gram, column_counts, ln_z, mean, shifts));
  if (rc) return rc;
  if (n_used) *n_used = p.n_used_ll;
  return ME_OK;
}

// the two forms of me_mbar_gram_fluctuations behind their Source
int gram_fluctuations_common(const Source &src, const double *f, const double *temps, int n_targets, double *gram, double *column_counts,
                             const FluctuationOutputs &o, int64_t *n_used) {
  if (!gram || !column_counts) return fail(src.e, ME_ERR_INVALID, "gram and column_counts are needed");
  int rc = check_f_and_targets(src.e, f, std::min(src.n_rungs, kK), temps, n_targets, 1);
  if (rc) return rc;
  Problem p;
  rc = mbar_check_common(src.e, p, mbar_gram_fluctuations(p, src, f, temps, n_targets, gram, column_counts, o));
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

int me_mbar_gram_observables(me_engine *e, const double *f, const double *temps, int32_t n_targets, double *gram, double *column_counts,
                             double *ln_z, double *mean, double *shifts, int64_t *n_used) {
  Source src;
  const int rc = src.from_engine(e);
  if (rc) return rc;
  if (src.columns.n_columns == 0)
    return fail(e, ME_ERR_STATE, "no recorded observables: me_observable_samples_enable, then me_energy_samples_record");
  return gram_observables_common(src, f, temps, n_targets, gram, column_counts, ln_z, mean, shifts, n_used);
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

int me_mbar_gram_observables_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                     const double *ladder_temps, int32_t n_rungs, const double *observables, int32_t n_columns,
                                     const double *f, const double *temps, int32_t n_targets, double *gram, double *column_counts,
                                     double *ln_z, double *mean, double *shifts, int64_t *n_used) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs, observables, n_columns);
  return rc ? rc : src.finish(gram_observables_common(src, f, temps, n_targets, gram, column_counts, ln_z, mean, shifts, n_used));
}

int me_mbar_gram_fluctuations(me_engine *e, const double *f, const double *temps, int32_t n_targets, double *gram, double *column_counts,
                              double *ln_z, double *moments, double *energy_shift, double *shifts, double *mean_e, double *var_e,
                              double *mean, double *var, double *cov_energy, int64_t *n_used) {
  Source src;
  const int rc = src.from_engine(e);      // (no observable store: src.columns.n_columns = 0, the energy columns alone)
  if (rc) return rc;
  return gram_fluctuations_common(src, f, temps, n_targets, gram, column_counts,
                                  FluctuationOutputs{ln_z, moments, energy_shift, shifts, mean_e, var_e, mean, var, cov_energy}, n_used);
}

int me_mbar_gram_fluctuations_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                      const double *ladder_temps, int32_t n_rungs, const double *observables, int32_t n_columns,
                                      const double *f, const double *temps, int32_t n_targets, double *gram, double *column_counts,
                                      double *ln_z, double *moments, double *energy_shift, double *shifts, double *mean_e,
                                      double *var_e, double *mean, double *var, double *cov_energy, int64_t *n_used) {
  Source src;
  const int rc = n_columns == 0 ? src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs)
                                : src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs, observables, n_columns);
  if (rc) return rc;
  return src.finish(gram_fluctuations_common(src, f, temps, n_targets, gram, column_counts,
                                             FluctuationOutputs{ln_z, moments, energy_shift, shifts, mean_e, var_e, mean, var, cov_energy},
                                             n_used));
}

}  // extern "C"
