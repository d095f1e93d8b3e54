// Population annealing: one Boltzmann resampling stage of the engine's chains (me_population_resample in the public header).
//
// A stage from T_old = temp to T_new reweights chain i by w_i = exp(l_i - M), l_i = -(1/T_new - 1/T_old) E_i in float64,
// E_i = the sum of the chain's energy-ledger rows in row order in the device dtype (k_replica_swap's quantity); a chain with
// a non-finite l_i has weight 0.  It records log_weight = M + ln(W / N) (the estimate of ln Z(T_new) / Z(T_old)),
// neff_fraction = W^2 / (N S2) and n_finite, then resamples systematically with ONE uniform u (word 0 of Philox block
// 0xfffe at counter (chain_offset, stage)): slot j takes the chain a_j = min{ i : N C_i / W > j + u }, C_i the inclusive
// prefix sum of the weights.  Slot j receives chain a_j's x, every energy-ledger row and its family id; everything adapted
// or measured (widths, running means, covariances, factors, traces, counters) stays with the slot -- the swap's rule.
//
// The arithmetic, which tests/population_reference.py restates step for step:
//   * The chains are cut into blocks of kPopChunk consecutive chains (block b: chains [b kPopChunk, (b+1) kPopChunk)).
//     m_b = max of the block's finite l_i, v_i = exp(l_i - m_b) (0 for a non-finite l_i), Q_i = the running sum of v
//     inside the block in chain order, s_b = the block's last Q, q_b = the block's sum of v_i^2.  k_pop_weights computes
//     these; k_pop_scan_ancestors recomputes v_i and Q_i with the SAME code, so its last Q_i is s_b bit for bit.
//   * k_pop_finalize: M = max_b m_b, f_b = exp(m_b - M), and, sequentially over b, O_{b+1} = O_b + f_b s_b (O_0 = 0) and
//     S2 = S2 + (f_b f_b) q_b.  W = O_B.
//   * C_i = O_b + f_b Q_i.  The last chain of block b has C = O_{b+1} exactly, so C is non-decreasing across blocks and
//     C_{N-1} = W; a chain of weight 0 has C_i = C_{i-1} and no offspring.  (C_i agrees with the textbook inclusive sum of
//     exp(l_i - M) to a few ulps; f_b v_i is the weight that is actually resampled.)
//   * Slot boundary of chain i: B_i = ceil(N C_i / W - u) clamped to [0, N] (evaluated as ((N C_i) / W) - u; the unit is
//     built with -ffp-contract=off so that no product is fused into the sum it feeds).  Chain i owns the slots
//     [B_{i-1}, B_i) (B_{-1} = 0), which are exactly the j with N C_{i-1} / W <= j + u < N C_i / W.  Every slot below
//     hi = B_{N-1} is written once.  Slots j >= hi, left undefined by rounding, take the ancestor of slot hi - 1: the last
//     chain with a positive weight.
//   * n_finite = 0: the population is left unchanged (a_j = j), log_weight = -inf, neff_fraction = 0.
// Identity (T_new = T_old): l_i = 0, v_i = f_b = 1, C_i = i + 1, N C_i / W = i + 1 exactly, a_j = j, log_weight = 0.
//
// Kernels (one instantiation per dtype, all on the engine stream): k_pop_weights (reads the ledger once: the block's
// kPopItems energies per thread stay in registers between the max and the sum), k_pop_finalize (one block), k_pop_scan_
// ancestors (scatters a_j into the engine-owned ancestor array; a chain's run of more than kSerialSlots slots is written by
// its whole wavefront), k_pop_gather (one lane per slot: x, the ledger rows and
// the family id of a_j into engine-owned scratch, eight rows in flight).  me_population_resample then copies the scratch back into x,
// the ledger and the family array: the x / energy pointers themselves never change (a captured graph holds them).
#include <algorithm>
#include <cmath>
#include <vector>

#include "me_device.h"
#include "me_engine.h"

namespace me {
namespace {

constexpr int kPopThreads = 256;
constexpr int kPopWaves = kPopThreads / 64;
constexpr int kPopItems = 8;                                  // chains per thread and block
constexpr int kPopChunk = kPopThreads * kPopItems;            // 2048 chains per block
constexpr int kFinalThreads = 256;
constexpr long long kSerialSlots = 8;                         // longer runs of slots are written by the whole wavefront

// device-side results of one stage that the later kernels read
struct PopParams {
  double M, W, u;
  long long hi;        // B_{N-1}: slots >= hi take the ancestor of slot hi - 1
  long long n_finite;
};

// l_i of chain c (block-local round r of thread t) and whether it counts
template <typename R>
__device__ __forceinline__ double chain_log_weight(const Field<R> &fe, long long c, long long n, int n_terms, double neg_dbeta,
                                                   bool &valid) {
  valid = false;
  if (c >= n) return 0.0;
  const unsigned int off = (unsigned int)c * (unsigned int)sizeof(R);
  const R e = chain_energy(fe, off, n_terms);
  const double l = neg_dbeta * (double)e;
  valid = isfinite(l);
  return l;
}

// The running sum of v over one round of kPopThreads consecutive chains, in a fixed association order (Hillis-Steele
// inside each wavefront, the wavefronts' totals added in order): returns carry + (the round's inclusive sum up to this
// thread) and sets `prev` to the same quantity of the chain before (carry for thread 0).  `carry` becomes the round's
// last value.  Identical in k_pop_weights and k_pop_scan_ancestors, so both see the same sums bit for bit.
__device__ __forceinline__ double round_running_sum(double v, double &carry, double &prev, double *wave_tot, double *wave_last) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double y = __shfl_up(x, d);
    if (lane >= d) x = y + x;
  }
  if (lane == 63) wave_tot[w] = x;
  __syncthreads();
  double off = 0.0;
  for (int k = 0; k < w; ++k) off = off + wave_tot[k];
  const double q = carry + (off + x);
  if (lane == 63) wave_last[w] = q;
  __syncthreads();
  const double up = __shfl_up(q, 1);
  prev = lane ? up : (w ? wave_last[w - 1] : carry);
  carry = wave_last[kPopWaves - 1];
  return q;
}

__device__ __forceinline__ double block_max(double v, double *scratch) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double m = scratch[0];
  for (int k = 1; k < kPopWaves; ++k) m = fmax(m, scratch[k]);
  __syncthreads();
  return m;
}

// sum over the block in a fixed order (butterfly in each wavefront, then the wavefronts in order)
__device__ __forceinline__ double block_sum(double v, double *scratch) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = scratch[0];
  for (int k = 1; k < kPopWaves; ++k) s = s + scratch[k];
  __syncthreads();
  return s;
}

// ---- stage 1: per block (m_b, s_b, q_b, n_finite_b) -------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kPopThreads) k_pop_weights(const R *energy, long long n, int n_terms, double neg_dbeta,
                                                            double *partials) {
  __shared__ double red[kPopWaves], wave_tot[kPopWaves], wave_last[kPopWaves];
  const Field<R> fe(energy, n, n_terms);
  const long long base = (long long)blockIdx.x * kPopChunk;
  double l[kPopItems];
  bool ok[kPopItems];
  double m = -INFINITY;
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < kPopItems; ++r) {
    l[r] = chain_log_weight(fe, base + r * kPopThreads + threadIdx.x, n, n_terms, neg_dbeta, ok[r]);
    if (ok[r]) {
      m = fmax(m, l[r]);
      ++cnt;
    }
  }
  m = block_max(m, red);
  const double n_fin = block_sum((double)cnt, red);
  double carry = 0.0, prev, sq = 0.0;
#pragma unroll
  for (int r = 0; r < kPopItems; ++r) {
    const double v = ok[r] ? exp(l[r] - m) : 0.0;
    round_running_sum(v, carry, prev, wave_tot, wave_last);
    sq = sq + v * v;
  }
  sq = block_sum(sq, red);
  if (threadIdx.x == 0) {
    double *p = partials + 4 * (size_t)blockIdx.x;
    p[0] = m;
    p[1] = carry;
    p[2] = sq;
    p[3] = n_fin;
  }
}

// ---- finalize: M, the block factors and offsets, W, S2, the stage record, u and hi (one block) --------------------------
__global__ void __launch_bounds__(kFinalThreads) k_pop_finalize(const double *partials, int n_blocks, long long n,
                                                               unsigned long long chain_offset, unsigned long long stage,
                                                               uint32_t seed_lo, uint32_t seed_hi, double *factors,
                                                               double *offsets, PopParams *params, double *record) {
  __shared__ double red[kFinalThreads / 64];
  __shared__ long long fin[kFinalThreads / 64];
  double m = -INFINITY;
  long long cnt = 0;
  for (int b = threadIdx.x; b < n_blocks; b += kFinalThreads) {
    m = fmax(m, partials[4 * (size_t)b]);
    cnt += (long long)partials[4 * (size_t)b + 3];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    m = fmax(m, __shfl_xor(m, d));
    cnt += __shfl_xor(cnt, d);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = m;
    fin[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  double M = red[0];
  long long n_finite = fin[0];
  for (int k = 1; k < kFinalThreads / 64; ++k) {
    M = fmax(M, red[k]);
    n_finite += fin[k];
  }
  for (int b = threadIdx.x; b < n_blocks; b += kFinalThreads) {
    const double mb = partials[4 * (size_t)b];
    factors[b] = (n_finite > 0 && mb > -INFINITY) ? exp(mb - M) : 0.0;
  }
  __syncthreads();
  if (n_finite == 0) {                           // nothing to reweight: the population stays as it is
    if (threadIdx.x == 0) {
      PopParams p;
      p.M = -INFINITY;
      p.W = 0.0;
      p.u = 0.5;
      p.hi = n;
      p.n_finite = 0;
      *params = p;
      record[0] = -INFINITY;
      record[1] = 0.0;
      record[2] = 0.0;
    }
    return;
  }
  // The sequential sums in block order, kFinalThreads blocks at a time: the terms are formed in parallel into LDS, one
  // thread adds them up and the offsets go out in parallel: 13.7 us at 512 blocks.  (Read from and written to global
  // memory in the loop, where the compiler cannot move the loads past the offset stores, the sums took 75 us; batches of
  // eight LDS loads ahead of their adds, predicated for the tail, took 50 us.)
  __shared__ double term[kFinalThreads], term2[kFinalThreads], run[kFinalThreads], total[2];
  if (threadIdx.x == 0) {
    total[0] = 0.0;
    total[1] = 0.0;
    offsets[0] = 0.0;
  }
  for (int b0 = 0; b0 < n_blocks; b0 += kFinalThreads) {
    const int b = b0 + (int)threadIdx.x;
    if (b < n_blocks) {
      const double f = factors[b];
      term[threadIdx.x] = f * partials[4 * (size_t)b + 1];
      term2[threadIdx.x] = (f * f) * partials[4 * (size_t)b + 2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int k_end = std::min(kFinalThreads, n_blocks - b0);
      double o = total[0], s2 = total[1];
      for (int k = 0; k < k_end; ++k) {
        o = o + term[k];
        s2 = s2 + term2[k];
        run[k] = o;
      }
      total[0] = o;
      total[1] = s2;
    }
    __syncthreads();
    if (b < n_blocks) offsets[b + 1] = run[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double W = total[0], s2 = total[1], N = (double)n;
  // word 0 of Philox block 0xfffe at counter (chain_offset, stage)
  U4 ctr;
  ctr.x = (uint32_t)chain_offset;
  ctr.y = (uint32_t)(chain_offset >> 32);
  ctr.z = (uint32_t)stage;
  ctr.w = ((uint32_t)(stage >> 32) << 16) | 0xfffeu;
  const double u = ((double)philox4x32_10(ctr, seed_lo, seed_hi).x + 0.5) * (1.0 / 4294967296.0);
  PopParams p;
  p.u = u;
  p.n_finite = n_finite;
  p.M = M;
  p.W = W;
  const double t = ceil((N * W) / W - u);
  p.hi = t <= 0.0 ? 0 : (t >= N ? n : (long long)t);
  *params = p;
  record[0] = M + log(W / N);
  record[1] = (W * W) / (N * s2);
  record[2] = (double)n_finite;
}

// ---- stage 2: each chain scatters its index into the slots it owns ------------------------------------------------------
__device__ __forceinline__ long long slot_bound(double c, double N, double W, double u, long long hi) {
  const double t = ceil((N * c) / W - u);
  return t <= 0.0 ? 0 : (t >= (double)hi ? hi : (long long)t);
}

template <typename R>
__global__ void __launch_bounds__(kPopThreads) k_pop_scan_ancestors(const R *energy, long long n, int n_terms, double neg_dbeta,
                                                                   const double *partials, const double *factors,
                                                                   const double *offsets, const PopParams *params,
                                                                   unsigned int *ancestors) {
  __shared__ double wave_tot[kPopWaves], wave_last[kPopWaves];
  const PopParams p = *params;
  const long long base = (long long)blockIdx.x * kPopChunk;
  if (p.n_finite == 0) {                         // identity
    for (int r = 0; r < kPopItems; ++r) {
      const long long c = base + r * kPopThreads + threadIdx.x;
      if (c < n) ancestors[c] = (unsigned int)c;
    }
    return;
  }
  const Field<R> fe(energy, n, n_terms);
  const double m = partials[4 * (size_t)blockIdx.x], f = factors[blockIdx.x], o = offsets[blockIdx.x];
  const double N = (double)n;
  double l[kPopItems];
  bool ok[kPopItems];
#pragma unroll
  for (int r = 0; r < kPopItems; ++r) l[r] = chain_log_weight(fe, base + r * kPopThreads + threadIdx.x, n, n_terms, neg_dbeta, ok[r]);
  double carry = 0.0, prev;
#pragma unroll
  for (int r = 0; r < kPopItems; ++r) {
    const double v = ok[r] ? exp(l[r] - m) : 0.0;
    const double q = round_running_sum(v, carry, prev, wave_tot, wave_last);
    const long long c = base + r * kPopThreads + threadIdx.x;
    long long lo = 0, up = 0;
    if (q > prev) {                              // (weight 0, or lost to rounding: no offspring)
      lo = slot_bound(o + f * prev, N, p.W, p.u, p.hi);
      up = slot_bound(o + f * q, N, p.W, p.u, p.hi);
    }
    // A chain owns about N w_i / W slots: a few for most, but all N when the weights collapse onto one chain.  Short runs
    // are written by their own lane; a long run by the whole wavefront, 64 consecutive slots per store instruction, one
    // long run after the other (the lanes of the wavefront are converged here: round_running_sum ends in a barrier).
    const bool long_run = up - lo > kSerialSlots;
    if (!long_run)
      for (long long j = lo; j < up; ++j) ancestors[j] = (unsigned int)c;
    unsigned long long runs = __ballot(long_run);
    while (runs) {
      const int src = __ffsll((long long)runs) - 1;
      runs &= runs - 1;
      const long long run_lo = __shfl(lo, src), run_up = __shfl(up, src);
      const unsigned int run_c = (unsigned int)__shfl(c, src);
      for (long long j = run_lo + (threadIdx.x & 63); j < run_up; j += 64) ancestors[j] = run_c;
    }
  }
}

// ---- stage 3: gather x, the ledger rows and the family ids of the ancestors into scratch --------------------------------
template <class F>
__device__ __forceinline__ void copy_rows(const F &src, const F &dst, unsigned int src_off, unsigned int dst_off, int rows) {
  constexpr int B = 8;
  for (int r0 = 0; r0 < rows; r0 += B) {
    decltype(src.load(0, 0u)) v[B];
#pragma unroll
    for (int k = 0; k < B; ++k)
      if (r0 + k < rows) v[k] = src.load(r0 + k, src_off);
#pragma unroll
    for (int k = 0; k < B; ++k)
      if (r0 + k < rows) dst.store(r0 + k, dst_off, v[k]);
  }
}

template <typename R>
__global__ void __launch_bounds__(kPopThreads) k_pop_gather(const R *x, const R *energy, const long long *fam, R *x_out,
                                                           R *energy_out, long long *fam_out, long long n, int d, int n_terms,
                                                           int tiled, const unsigned int *ancestors, const PopParams *params) {
  const long long j = (long long)blockIdx.x * kPopThreads + threadIdx.x;
  if (j >= n) return;
  const long long hi = params->hi;
  const long long a = (long long)ancestors[j < hi ? j : hi - 1];
  const unsigned int a_off = (unsigned int)a * (unsigned int)sizeof(R), j_off = (unsigned int)j * (unsigned int)sizeof(R);
  if (tiled) copy_rows(TiledField<R>(x, n, d), TiledField<R>(x_out, n, d), tiled_offset<R>(a, d), tiled_offset<R>(j, d), d);
  else copy_rows(Field<R>(x, n, d), Field<R>(x_out, n, d), a_off, j_off, d);
  copy_rows(Field<R>(energy, n, n_terms), Field<R>(energy_out, n, n_terms), a_off, j_off, n_terms);
  fam_out[j] = fam[a];
}

__global__ void __launch_bounds__(kPopThreads) k_pop_init_families(long long *fam, long long n, unsigned long long chain_offset) {
  const long long j = (long long)blockIdx.x * kPopThreads + threadIdx.x;
  if (j < n) fam[j] = (long long)(chain_offset + (unsigned long long)j);
}

// One stage on the engine's stream: weights, scan, ancestors, and the gather of x, the ledger rows and the family ids of
// the ancestors into the engine's scratch (the caller copies them back).  neg_dbeta = -(1/T_new - 1/T_old).
template <typename R>
hipError_t launch(me_engine *e, double neg_dbeta) {
  me_engine::Population &pop = e->population;
  const long long n = e->n;
  hipStream_t stream = e->stream;
  const int n_blocks = (int)((n + kPopChunk - 1) / kPopChunk);
  const unsigned slot_blocks = (unsigned)((n + kPopThreads - 1) / kPopThreads);
  double *partials = pop.scratch.get<double>(), *factors = partials + 4 * (size_t)n_blocks, *offsets = factors + n_blocks;
  PopParams *params = (PopParams *)(offsets + n_blocks + 1);
  double *record = pop.records.get<double>() + 3 * (size_t)pop.stages;     // this stage's (log_weight, neff_fraction, n_finite)
  hipLaunchKernelGGL(k_pop_weights<R>, dim3(n_blocks), dim3(kPopThreads), 0, stream, e->energy.get<const R>(), n, e->n_terms,
                     neg_dbeta, partials);
  hipLaunchKernelGGL(k_pop_finalize, dim3(1), dim3(kFinalThreads), 0, stream, (const double *)partials, n_blocks, n,
                     e->chain_offset, pop.stages, (uint32_t)e->seed, (uint32_t)(e->seed >> 32), factors, offsets, params, record);
  hipLaunchKernelGGL(k_pop_scan_ancestors<R>, dim3(n_blocks), dim3(kPopThreads), 0, stream, e->energy.get<const R>(), n,
                     e->n_terms, neg_dbeta, (const double *)partials, (const double *)factors, (const double *)offsets,
                     (const PopParams *)params, pop.anc.get<unsigned int>());
  hipLaunchKernelGGL(k_pop_gather<R>, dim3(slot_blocks), dim3(kPopThreads), 0, stream, e->x.get<const R>(), e->energy.get<const R>(),
                     pop.fam.get<const long long>(), pop.x.get<R>(), pop.energy.get<R>(), pop.fam_out.get<long long>(), n, e->d,
                     e->n_terms, e->x_tiled ? 1 : 0, pop.anc.get<const unsigned int>(), (const PopParams *)params);
  return hipGetLastError();
}

size_t population_scratch_doubles(long long n) {
  const long long n_blocks = (n + kPopChunk - 1) / kPopChunk;
  return (size_t)(4 * n_blocks + n_blocks + n_blocks + 1) + (sizeof(PopParams) + sizeof(double) - 1) / sizeof(double);
}

// ---- entry points: the scalar temperature and population annealing -------------------------------------------------------
int ensure_families(me_engine *e) {
  me_engine::Population &pop = e->population;
  if (pop.fam) return ME_OK;
  ME_HIP(e, pop.fam.resize((size_t)e->n * sizeof(long long)));
  hipLaunchKernelGGL(k_pop_init_families, dim3((unsigned)((e->n + kPopThreads - 1) / kPopThreads)), dim3(kPopThreads), 0, e->stream,
                     pop.fam.get<long long>(), e->n, e->chain_offset);
  ME_HIP(e, hipGetLastError());
  return ME_OK;
}
// everything a stage writes besides x, the ledger and the families; the ledger scratch follows me_set_energy's row count
int ensure_population_scratch(me_engine *e) {
  me_engine::Population &pop = e->population;
  const size_t energy_bytes = (size_t)e->n * (size_t)e->n_terms * e->esize;
  if (pop.energy.bytes() < energy_bytes) {
    if (pop.energy) ME_HIP(e, hipStreamSynchronize(e->stream));
    ME_HIP(e, pop.energy.reserve(energy_bytes));
  }
  if (!pop.x) {
    // same extent as x (tile-major: whole 64-chain tiles); it starts as a copy so that the padding lanes of a partial tile,
    // which no gather writes, never carry uninitialised memory back into x
    ME_HIP(e, pop.x.resize(e->x.bytes()));
    ME_HIP(e, hipMemcpyAsync(pop.x.get(), e->x.get(), pop.x.bytes(), hipMemcpyDeviceToDevice, e->stream));
  }
  ME_HIP(e, pop.fam_out.resize((size_t)e->n * sizeof(long long)));
  ME_HIP(e, pop.anc.resize((size_t)e->n * sizeof(unsigned int)));
  ME_HIP(e, pop.scratch.resize(population_scratch_doubles(e->n) * sizeof(double)));
  return ME_OK;
}
// room for `stages` stage records on the device (grown by doubling; a growth waits for the stream once)
int ensure_records(me_engine *e, unsigned long long stages) {
  me_engine::Population &pop = e->population;
  if (stages <= pop.capacity) return ME_OK;
  unsigned long long cap = std::max<unsigned long long>(256, pop.capacity);
  while (cap < stages) cap *= 2;
  DeviceBuffer grown;
  ME_HIP(e, grown.resize((size_t)cap * 3 * sizeof(double)));
  if (pop.records) {
    ME_HIP(e, hipMemcpyAsync(grown.get(), pop.records.get(), (size_t)pop.stages * 3 * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    ME_HIP(e, hipStreamSynchronize(e->stream));
  }
  pop.records = std::move(grown);
  pop.capacity = cap;
  return ME_OK;
}
int check_family_range(me_engine *e, int64_t chain_begin, int64_t n) {
  if (chain_begin < 0 || n < 0 || chain_begin + n > e->n) return fail(e, ME_ERR_INVALID, "family range outside the engine's chains");
  return ME_OK;
}

}  // namespace
}  // namespace me

using namespace me;

extern "C" {

int me_set_temperature(me_engine *e, double temp) {
  if (!e) return ME_ERR_INVALID;
  if (!(std::isfinite(temp) && temp >= 0)) return fail(e, ME_ERR_INVALID, "temp must be finite and >= 0");
  if (e->ladder.n_rungs) return fail(e, ME_ERR_STATE, "this engine has a temperature ladder: its rungs carry the temperatures");
  e->temp = temp;          // the next launch reads it (fill_step_launch)
  return ME_OK;
}

int me_population_resample(me_engine *e, double new_temp) {
  if (!e) return ME_ERR_INVALID;
  if (!(std::isfinite(new_temp) && new_temp > 0)) return fail(e, ME_ERR_INVALID, "the new temperature must be finite and > 0");
  int rc = refuse_stale_total(e, "population annealing is");
  if (rc != ME_OK) return rc;
  if (e->ladder.n_rungs) return fail(e, ME_ERR_STATE, "population annealing needs the scalar temp: this engine has a temperature ladder");
  if (!(e->temp > 0)) return fail(e, ME_ERR_STATE, "population annealing cannot reweight from temp = 0: set a temperature first");
  ME_HIP(e, hipSetDevice(e->device));
  if ((rc = ensure_families(e)) || (rc = ensure_population_scratch(e)) || (rc = ensure_records(e, e->population.stages + 1))) return rc;
  me_engine::Population &pop = e->population;
  const double neg_dbeta = -(1.0 / new_temp - 1.0 / e->temp);
  ME_HIP(e, e->dtype == ME_F32 ? launch<float>(e, neg_dbeta) : launch<double>(e, neg_dbeta));
  // the scratch goes back into the engine's own buffers: their addresses stay what a captured graph recorded
  ME_HIP(e, hipMemcpyAsync(e->x.get(), pop.x.get(), pop.x.bytes(), hipMemcpyDeviceToDevice, e->stream));
  ME_HIP(e, hipMemcpyAsync(e->energy.get(), pop.energy.get(), (size_t)e->n * (size_t)e->n_terms * e->esize, hipMemcpyDeviceToDevice, e->stream));
  ME_HIP(e, hipMemcpyAsync(pop.fam.get(), pop.fam_out.get(), (size_t)e->n * sizeof(long long), hipMemcpyDeviceToDevice, e->stream));
  e->temp = new_temp;
  e->population.temps.push_back(new_temp);
  e->population.stages += 1;
  return ME_OK;
}

int me_population_stats(me_engine *e, uint64_t *stages, double *stage_temps, double *log_weight, double *neff_fraction,
                        int64_t *n_finite, int64_t capacity) {
  if (!e) return ME_ERR_INVALID;
  if (stages) *stages = e->population.stages;
  if (!stage_temps && !log_weight && !neff_fraction && !n_finite) return ME_OK;
  if (capacity < 0 || (unsigned long long)capacity < e->population.stages)
    return fail(e, ME_ERR_INVALID, "the arrays must hold one entry per stage");
  if (e->population.stages == 0) return ME_OK;
  ME_HIP(e, hipSetDevice(e->device));
  std::vector<double> rec(3 * (size_t)e->population.stages);
  ME_HIP(e, hipMemcpyAsync(rec.data(), e->population.records.get(), rec.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  ME_HIP(e, hipStreamSynchronize(e->stream));
  for (size_t k = 0; k < e->population.stages; ++k) {
    if (stage_temps) stage_temps[k] = e->population.temps[k];
    if (log_weight) log_weight[k] = rec[3 * k];
    if (neff_fraction) neff_fraction[k] = rec[3 * k + 1];
    if (n_finite) n_finite[k] = (int64_t)rec[3 * k + 2];
  }
  return ME_OK;
}

int me_set_population_stats(me_engine *e, uint64_t stages, const double *stage_temps, const double *log_weight,
                            const double *neff_fraction, const int64_t *n_finite) {
  if (!e) return ME_ERR_INVALID;
  if (stages > 0 && (!stage_temps || !log_weight || !neff_fraction || !n_finite))
    return fail(e, ME_ERR_INVALID, "stage_temps / log_weight / neff_fraction / n_finite missing");
  std::vector<double> rec(3 * (size_t)stages);
  for (uint64_t k = 0; k < stages; ++k) {
    if (!(std::isfinite(stage_temps[k]) && stage_temps[k] > 0)) return fail(e, ME_ERR_INVALID, "stage temperatures must be finite and > 0");
    if (n_finite[k] < 0 || n_finite[k] > e->n) return fail(e, ME_ERR_INVALID, "n_finite must lie in [0, n_chains]");
    rec[3 * k] = log_weight[k];
    rec[3 * k + 1] = neff_fraction[k];
    rec[3 * k + 2] = (double)n_finite[k];
  }
  ME_HIP(e, hipSetDevice(e->device));
  int rc = ensure_records(e, std::max<uint64_t>(stages, 1));
  if (rc) return rc;
  if (stages > 0) {
    ME_HIP(e, hipMemcpyAsync(e->population.records.get(), rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    ME_HIP(e, hipStreamSynchronize(e->stream));
  }
  e->population.temps.assign(stage_temps, stage_temps + stages);
  e->population.stages = stages;
  return ME_OK;
}

int me_population_families(me_engine *e, int64_t chain_begin, int64_t n, int64_t *dst) {
  if (!e || (!dst && n > 0)) return ME_ERR_INVALID;
  int rc = check_family_range(e, chain_begin, n);
  if (rc || n == 0) return rc;
  if (!e->population.fam) {                  // never resampled: every chain is its own family, the global chain id
    for (int64_t k = 0; k < n; ++k) dst[k] = (int64_t)(e->chain_offset + (unsigned long long)(chain_begin + k));
    return ME_OK;
  }
  ME_HIP(e, hipSetDevice(e->device));
  ME_HIP(e, hipMemcpyAsync(dst, e->population.fam.get<long long>() + chain_begin, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
  ME_HIP(e, hipStreamSynchronize(e->stream));
  return ME_OK;
}

int me_set_population_families(me_engine *e, int64_t chain_begin, int64_t n, const int64_t *src) {
  if (!e || (!src && n > 0)) return ME_ERR_INVALID;
  int rc = check_family_range(e, chain_begin, n);
  if (rc || n == 0) return rc;
  ME_HIP(e, hipSetDevice(e->device));
  if ((rc = ensure_families(e))) return rc;
  ME_HIP(e, hipMemcpyAsync(e->population.fam.get<long long>() + chain_begin, src, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, e->stream));
  ME_HIP(e, hipStreamSynchronize(e->stream));
  return ME_OK;
}

}  // extern "C"
