// A Newton solver for the MBAR free energies of a temperature ladder (me_mbar_solve_newton and its engine-less twin in the
// public header).  Notation as in me_mbar.hip: samples n are USED when E_n is finite, K rungs, beta_k = 1 / T_k, N_k used
// samples of rung k, f starts at 0.  One pass over the samples from f, which tests/mbar_newton_reference.py restates:
//     a_nj = (ln N_j + f_j) - beta_j E_n,  m_n = max_j a_nj,  e_nj = exp(a_nj - m_n),  s_n = sum_j e_nj,  W_nj = e_nj / s_n
//     S_j = sum_n W_nj  (= N_j at the solution),  G = W^T W  (K x K),  gamma = max_j |S_j / N_j - 1|
// and then one step, of which there are two:
//     self-consistent   f_j <- f_j - ln(S_j / N_j), then f <- f - f_0                      (me_mbar.hip's update)
//     Newton            H = diag(S) - G  (= dS / df, positive semi-definite, H 1 = 0);  H[1:, 1:] delta[1:] = (N - S)[1:] by
//                       Cholesky, delta_0 = 0;  f <- f + delta
// Passes 1 and 2 take the self-consistent step and every later pass the Newton step.  When the step before a pass was a Newton
// step and gamma did not come out <= its value at the pass before, that step is withdrawn: f and S from before it are
// restored and the self-consistent step is taken from there.  A Cholesky pivot that is <= 0 or not finite makes the pass take
// the self-consistent step.  Both count as fallback_steps.  residual = max_k |change of f_k| of the step taken; the solve stops
// once residual <= tolerance or after max_iterations passes.  K = 1: f = [0], one iteration.
//
// Kernels.  k_mbar_newton_pass<kTN> (kTN = 1, 2, 4 tile rows of G: K <= 16, 32, 64): one pass over the energies with the grid
// policy of k_mbar_weights (tiles of 2048 samples walked grid-stride; a wavefront's lanes load 64 consecutive energies per
// step).  A wavefront works through its 64 samples in four sub-tiles of 16: lane l = (g, s) = (l >> 4, l & 15) takes sample s of
// the sub-tile (its energy comes by a shuffle) and the rungs j = g, g + 4, ..., so the four lanes of a sample share its K
// exponentials evenly whatever K is: the maximum and the sum cross the four lanes by two shuffles each (a symmetric butterfly:
// the four hold the same bits; beta_j and ln N_j + f_j come from a copy of the table in LDS), every lane takes the one reciprocal, and the weights -- each computed ONCE, by exp_nonpos,
// exactly 0 for a sample that does not count and for the columns from K to the tile edge -- go to the wavefront's own sub-tile
// in LDS, float64 [16][cp] (me_mbar_gram_tiles.h: lane_row).  From there the wavefront feeds v_mfma_f64_16x16x4_f64 with the
// fragment layout and the tile walk of k_mbar_gram (the same header), both operands from the one sub-tile: 1, 3 or 10 lower-
// triangle tiles, ALL held by every wavefront (4, 12 or 40 accumulator doubles per lane), so no barrier of the block is
// needed while the samples are walked -- a wavefront's LDS operations complete in order.  S needs no pass of its own: the operand
// a lane reads for tile column I is W[n][16 I + (l & 15)], and the lane adds what it reads (kTN additions per instruction group).
// Summation order, fixed (no floating-point atomics, bitwise reproducible): G: the instruction's own accumulation over its 4
// samples -> the k-steps in sample order -> the wavefront's steps and tiles in order; S: the samples n = l >> 4 (mod 4) of a lane
// in order -> the four lanes by butterfly (distances 16, 32); then for both: the block's wavefronts in order (in LDS, over the
// staging area) -> partials[block][K + K (K + 1) / 2] = [S | packed lower triangle of G] in global memory -> k_mbar_newton_sum
// adds the blocks in ascending order, one thread per entry (blocks of 64 threads, so that 35 MB of partials at K = 64 are read
// by 34 compute units and not by one) -> k_mbar_newton_update (ONE wavefront; lane k is rung k): gamma, the withdrawal rule, H
// in LDS ([K][65]: a lane's row is an odd number of doubles from its neighbours'), the right-looking Cholesky factorisation (lane
// i scales and updates row i; the pivot is one address read by all), the two triangular solves (the right-hand side stays in
// registers, x_j crosses by a shuffle), the step, the table (f, c = ln N + f), the control words, and f and S from before the
// step for the withdrawal rule.  Every kernel returns at once when control->done is set, as in me_mbar.hip, so within a batch
// of kBatch passes f stays the first iterate that met the tolerance; the host reads the control words once per batch.
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage) and the timings: profiles/mbar_newton.txt.
#include "me_mbar.h"
#include "me_mbar_gram_tiles.h"

namespace me {
namespace mbar {
namespace {

constexpr int kBatch = 16;                      // passes enqueued between two looks at the control words
constexpr int kSumThreads = 64;
constexpr int kLd = kK + 1;                     // doubles between two rows of H in LDS

struct NewtonControl {
  MbarControl base;                             // residual, iterations (= passes), done
  double gradient;                              // gamma of the last pass
  double gradient_kept;                         // gamma that belongs to the kept f and S
  int newton_steps, fallback_steps, last_newton, unused;
};

__device__ __forceinline__ void wave_sync() {
  // a wavefront's LDS operations issue and complete in program order; this keeps the compiler from moving them across
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the largest of v over the wavefront, NaN when any is NaN
__device__ __forceinline__ double wave_max_nan(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double o = __shfl_xor(v, d);
    v = (v != v || o != o) ? (double)NAN : fmax(v, o);
  }
  return v;
}

// partials[block] = [S | packed lower triangle of W^T W] of the block's tiles; n_rungs <= 16 kTN
template <int kTN>
__global__ void __launch_bounds__(kThreads) k_mbar_newton_pass(const double *__restrict__ energies, long long n, int n_rungs,
                                                               const double *__restrict__ table,
                                                               const NewtonControl *__restrict__ control, long long n_tiles,
                                                               double *partials) {
  if (control->base.done) return;
  constexpr int kCols = 16 * kTN, kMine = 4 * kTN, kPairs = kTN * (kTN + 1) / 2, kRow = lane_row(kCols);
  static_assert(kWaves * kSub * kRow >= kCols + kCols * (kCols + 1) / 2, "the block's sums reuse the staging area");
  __shared__ double stage[kWaves * kSub * kRow];
  __shared__ double t_beta[kCols], t_c[kCols];                   // (in LDS: sixteen rungs' worth in registers cost an occupancy step)
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const Fragment fr = fragment_of(lane);
  const int g = fr.h4, s16 = fr.j16;              // in the fill: the rungs g + 4 c of sample s16 of the sub-tile
  const int n_pairs = ((n_rungs + 15) >> 4) * (((n_rungs + 15) >> 4) + 1) / 2;
  if (t < kCols) {
    t_beta[t] = t < n_rungs ? table[kBeta + t] : 0.0;
    t_c[t] = t < n_rungs ? table[kC + t] : 0.0;
  }
  __syncthreads();
  f64x4 acc[kPairs];
#pragma unroll
  for (int p = 0; p < kPairs; ++p) acc[p] = f64x4{0.0, 0.0, 0.0, 0.0};
  double col_sum[kTN];
#pragma unroll
  for (int I = 0; I < kTN; ++I) col_sum[I] = 0.0;
  double *buf = stage + wave * (kSub * kRow);
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
    for (int r = 0; r < kItems; ++r) {
      const long long i = tile * kTile + (long long)r * kThreads + t;
      const double v = i < n ? energies[i] : NAN;
      const int ok = isfinite(v) ? 1 : 0;
      const double e = ok ? v : 0.0;
#pragma unroll 1
      for (int q = 0; q < 64 / kSub; ++q) {
        const double es = __shfl(e, kSub * q + s16);
        const int oks = __shfl(ok, kSub * q + s16);
        double a[kMine], m = -INFINITY, s = 0.0;
#pragma unroll
        for (int k = 0; k < kMine; ++k)
          if (4 * k < n_rungs) {                                  // (wave-uniform)
            a[k] = __builtin_fma(-t_beta[g + 4 * k], es, t_c[g + 4 * k]);
            m = g + 4 * k < n_rungs ? fmax(m, a[k]) : m;
          }
        m = fmax(m, __shfl_xor(m, 16));
        m = fmax(m, __shfl_xor(m, 32));
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
          if (4 * k < n_rungs) {
            const bool valid = g + 4 * k < n_rungs;
            const double x = math64::exp_nonpos(valid ? a[k] - m : 0.0);
            a[k] = valid ? x : 0.0;
            s = s + a[k];
          } else {
            a[k] = 0.0;
          }
        }
        s = s + __shfl_xor(s, 16);
        s = s + __shfl_xor(s, 32);
        const double inv = oks ? 1.0 / s : 0.0;
        wave_sync();                                              // (the fragments of the sub-tile before have been read)
#pragma unroll
        for (int k = 0; k < kMine; ++k) buf[s16 * kRow + g + 4 * k] = a[k] * inv;
        wave_sync();
#pragma unroll
        for (int ks = 0; ks < kSub / 4; ++ks) {
          const double *src = fragment_source(buf, ks, kRow, fr);
          double w[kTN];
#pragma unroll
          for (int I = 0; I < kTN; ++I) {
            w[I] = src[16 * I];
            col_sum[I] = col_sum[I] + w[I];
          }
#pragma unroll
          for (int p = 0; p < kPairs; ++p) {
            const int I = pair_row(p, kTN), J = p - I * (I + 1) / 2;
            if (p < n_pairs) acc[p] = gram_mfma(w[I], w[J], acc[p]);     // (wave-uniform)
          }
        }
      }
    }
  }
  // the block's wavefronts in order, over the staging area: [S | packed lower triangle]
  const int stride = n_rungs + n_rungs * (n_rungs + 1) / 2;
  __syncthreads();
  for (int k = t; k < stride; k += kThreads) stage[k] = 0.0;
  __syncthreads();
#pragma unroll
  for (int I = 0; I < kTN; ++I) {
    col_sum[I] = col_sum[I] + __shfl_xor(col_sum[I], 16);
    col_sum[I] = col_sum[I] + __shfl_xor(col_sum[I], 32);
  }
  for (int w = 0; w < kWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int p = 0; p < kPairs; ++p) {
        const int I = pair_row(p, kTN), J = p - I * (I + 1) / 2;
        if (p < n_pairs) store_lower_tile<true>(stage + n_rungs, 16 * I, 16 * J, fr, n_rungs, acc[p]);
      }
      if (fr.h4 == 0) {
#pragma unroll
        for (int I = 0; I < kTN; ++I)
          if (16 * I + fr.j16 < n_rungs) stage[16 * I + fr.j16] = stage[16 * I + fr.j16] + col_sum[I];
      }
    }
    __syncthreads();
  }
  for (int k = t; k < stride; k += kThreads) partials[(size_t)blockIdx.x * stride + k] = stage[k];
}

// sums[k] = the blocks' partials[block][k] added in ascending block order, k < stride
__global__ void __launch_bounds__(kSumThreads) k_mbar_newton_sum(const double *__restrict__ partials, int n_blocks, int stride,
                                                                 const NewtonControl *__restrict__ control, double *sums) {
  if (control->base.done) return;
  const int k = blockIdx.x * kSumThreads + threadIdx.x;
  if (k >= stride) return;
  double s = 0.0;
  for (int b = 0; b < n_blocks; ++b) s = s + partials[(size_t)b * stride + k];
  sums[k] = s;
}

// One step from sums = [S | packed lower triangle of G] (one wavefront; lane k is rung k): the policy of this file's header,
// the table, the control words, and kept = [f | S] from before the step
__global__ void __launch_bounds__(64) k_mbar_newton_update(const double *__restrict__ sums, int n_rungs, double tolerance, double *table,
                                                           NewtonControl *control, double *kept) {
  if (control->base.done) return;
  __shared__ double h[kK * kLd];
  const int lane = threadIdx.x;
  const bool mine = lane < n_rungs;
  const double count = mine ? table[kN + lane] : 1.0;
  double f = mine ? table[kF + lane] : 0.0, big_s = mine ? sums[lane] : 1.0;
  const double gamma = wave_max_nan(mine ? fabs(big_s / count - 1.0) : 0.0);
  const int passes = control->base.iterations;
  const bool withdraw = control->last_newton != 0 && !(gamma <= control->gradient_kept);
  double kept_gamma = gamma;
  int fallback = 0;
  if (withdraw) {
    f = mine ? kept[lane] : 0.0;
    big_s = mine ? kept[kK + lane] : 1.0;
    kept_gamma = control->gradient_kept;
    fallback = 1;
  }
  bool newton = !withdraw && passes >= 2;
  double f_new = f;
  if (newton) {
    // H[i][j] = (i == j ? S_i : 0) - G[i][j], 1 <= j <= i < K; lane i fills, scales and updates row i
    const double *gram = sums + n_rungs;
    const bool row = mine && lane >= 1;
    if (row)
      for (int j = 1; j <= lane; ++j) h[lane * kLd + j] = (j == lane ? big_s : 0.0) - gram[packed_index(lane, j)];
    for (int j = 1; j < n_rungs; ++j) {
      wave_sync();
      const double d = h[j * kLd + j];                             // (one address: the same in every lane)
      if (!(d > 0.0) || !isfinite(d)) {
        newton = false;
        fallback = 1;
        break;
      }
      const double l = sqrt(d);
      const bool below = mine && lane > j;
      double lij = 0.0;
      if (below) {
        lij = h[lane * kLd + j] / l;
        h[lane * kLd + j] = lij;
      }
      wave_sync();                                                // (every lane has read the pivot)
      if (lane == j) h[j * kLd + j] = l;
      if (below)
        for (int k = j + 1; k <= lane; ++k) h[lane * kLd + k] = h[lane * kLd + k] - lij * h[k * kLd + j];
    }
    wave_sync();
    if (newton) {
      double b = row ? count - big_s : 0.0;
      for (int j = 1; j < n_rungs; ++j) {                          // L y = b
        const double y = __shfl(b, j) / h[j * kLd + j];
        if (lane == j) b = y;
        else if (mine && lane > j) b = b - h[lane * kLd + j] * y;
      }
      for (int j = n_rungs - 1; j >= 1; --j) {                     // L^T x = y
        const double x = __shfl(b, j) / h[j * kLd + j];
        if (lane == j) b = x;
        else if (row && lane < j) b = b - h[j * kLd + lane] * x;
      }
      f_new = f + (row ? b : 0.0);
    }
  }
  if (!newton) {
    f_new = f - log(big_s / count);
    f_new = f_new - __shfl(f_new, 0);
  }
  const double r = wave_max_nan(mine ? fabs(f_new - f) : 0.0);
  if (mine) {
    kept[lane] = f;
    kept[kK + lane] = big_s;
    table[kF + lane] = f_new;
    table[kC + lane] = table[kLnN + lane] + f_new;
  }
  if (lane == 0) {
    control->base.residual = r;
    control->base.iterations = passes + 1;
    control->gradient = gamma;
    control->gradient_kept = kept_gamma;
    control->newton_steps += newton ? 1 : 0;
    control->fallback_steps += fallback;
    control->last_newton = newton ? 1 : 0;
    if (r <= tolerance) control->base.done = 1;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
template <int kTN>
void launch_pass(const Problem &p, int n_blocks, long long n_tiles, const NewtonControl *control, double *partials) {
  hipLaunchKernelGGL(k_mbar_newton_pass<kTN>, dim3(n_blocks), dim3(kThreads), 0, p.stream, p.sm.energies, p.sm.n_samples, p.n_rungs,
                     p.w.table.get<const double>(), control, n_tiles, partials);
}

// Waits for the stream and writes f[K] and the control words; with an empty rung (p.empty_rung) nothing else is computed.
hipError_t mbar_solve_newton(Problem &p, const Source &src, double tolerance, int max_iterations, double *f, NewtonControl &c) {
  ME_MBAR_HIP(prepare(p, src, nullptr));
  c = NewtonControl{};
  if (p.empty_rung >= 0) return hipSuccess;
  const int n_rungs = p.n_rungs, n_blocks = blocks_of(p.sm.n_samples);
  if (n_rungs == 1) {                             // nothing to solve: f_0 = 0 by definition
    f[0] = 0.0;
    c.base.iterations = 1;
    c.base.done = 1;
    return hipSuccess;
  }
  const long long n_tiles = tiles_of(p.sm.n_samples);
  const int stride = n_rungs + n_rungs * (n_rungs + 1) / 2;
  Work &w = p.w;
  DeviceBuffer sums, kept;
  ME_MBAR_HIP(w.partials.resize((size_t)n_blocks * stride * sizeof(double)));
  ME_MBAR_HIP(sums.resize((size_t)stride * sizeof(double)));
  ME_MBAR_HIP(kept.resize(2 * kK * sizeof(double)));
  ME_MBAR_HIP(w.control.resize(sizeof(NewtonControl)));
  ME_MBAR_HIP(hipMemsetAsync(w.control.get(), 0, sizeof(NewtonControl), p.stream));
  ME_MBAR_HIP(hipMemsetAsync(kept.get(), 0, kept.bytes(), p.stream));
  NewtonControl *control = w.control.get<NewtonControl>();
  while (c.base.iterations < max_iterations && !c.base.done) {
    const int batch = std::min(kBatch, max_iterations - c.base.iterations);
    for (int it = 0; it < batch; ++it) {
      if (n_rungs <= 16) launch_pass<1>(p, n_blocks, n_tiles, control, w.partials.get<double>());
      else if (n_rungs <= 32) launch_pass<2>(p, n_blocks, n_tiles, control, w.partials.get<double>());
      else launch_pass<4>(p, n_blocks, n_tiles, control, w.partials.get<double>());
      hipLaunchKernelGGL(k_mbar_newton_sum, dim3((stride + kSumThreads - 1) / kSumThreads), dim3(kSumThreads), 0, p.stream,
                         w.partials.get<const double>(), n_blocks, stride, control, sums.get<double>());
      hipLaunchKernelGGL(k_mbar_newton_update, dim3(1), dim3(64), 0, p.stream, sums.get<const double>(), n_rungs, tolerance,
                         w.table.get<double>(), control, kept.get<double>());
    }
    ME_MBAR_HIP(hipGetLastError());
    ME_MBAR_HIP(hipMemcpyAsync(&c, control, sizeof(NewtonControl), hipMemcpyDeviceToHost, p.stream));
    ME_MBAR_HIP(hipStreamSynchronize(p.stream));
  }
  ME_MBAR_HIP(hipMemcpyAsync(f, w.table.get<double>() + kF, (size_t)n_rungs * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  return hipStreamSynchronize(p.stream);
}

// the two forms of me_mbar_solve_newton behind their Source
int solve_newton_common(const Source &src, double tolerance, int max_iterations, double *f_out, int32_t *iterations, double *residual,
                        double *gradient, int32_t *newton_steps, int32_t *fallback_steps, int64_t *n_used_out) {
  if (!f_out) return fail(src.e, ME_ERR_INVALID, "f_out missing");
  if (!(tolerance > 0) || max_iterations < 1) return fail(src.e, ME_ERR_INVALID, "need tolerance > 0 and max_iterations >= 1");
  Problem p;
  NewtonControl c{};
  const hipError_t err = mbar_solve_newton(p, src, tolerance, max_iterations, f_out, c);
  if (err == hipSuccess && n_used_out)            // (also when a rung is empty: the message names one, these show all)
    for (int k = 0; k < p.n_rungs; ++k) n_used_out[k] = (int64_t)p.counts[k];
  const int rc = mbar_check_common(src.e, p, err);
  if (rc) return rc;
  if (iterations) *iterations = c.base.iterations;
  if (residual) *residual = c.base.residual;
  if (gradient) *gradient = c.gradient;
  if (newton_steps) *newton_steps = c.newton_steps;
  if (fallback_steps) *fallback_steps = c.fallback_steps;
  return ME_OK;
}

}  // namespace
}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_mbar_solve_newton(me_engine *e, double tolerance, int32_t max_iterations, double *f_out, int32_t *iterations, double *residual,
                         double *gradient, int32_t *newton_steps, int32_t *fallback_steps, int64_t *n_used_out) {
  Source src;
  const int rc = src.from_engine(e);
  return rc ? rc
            : solve_newton_common(src, tolerance, max_iterations, f_out, iterations, residual, gradient, newton_steps, fallback_steps,
                                  n_used_out);
}

int me_mbar_solve_newton_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                 const double *ladder_temps, int32_t n_rungs, double tolerance, int32_t max_iterations, double *f_out,
                                 int32_t *iterations, double *residual, double *gradient, int32_t *newton_steps,
                                 int32_t *fallback_steps, int64_t *n_used_out) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs);
  return rc ? rc
            : src.finish(solve_newton_common(src, tolerance, max_iterations, f_out, iterations, residual, gradient, newton_steps,
                                             fallback_steps, n_used_out));
}

}  // extern "C"
