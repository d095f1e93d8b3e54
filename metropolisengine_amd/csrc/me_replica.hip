// Replica exchange between the rungs of a temperature ladder (me_replica_exchange in the public header).
//
// A ladder engine's n chains are K rungs of M = n / K chains (M a multiple of 64); rung k steps at T_k.  Round r pairs rung k
// with rung k + 1 for every k = r (mod 2); slot j of rung k (chain a = k M + j) with slot j of rung k + 1 (chain b = a + M).
// The configurations -- x and every energy-ledger row -- swap with probability min(1, exp(delta)),
// delta = (1/T_k - 1/T_{k+1}) (E_a - E_b), E = the sum of the ledger rows in row order; a non-finite energy never swaps.
// Everything adapted or measured at a temperature (widths, running means, covariance, factors, counters) stays with the slot.
// The uniform is word 0 of Philox block 0xffff of (chain a, round r): a step of a ladder engine uses at most 33 blocks
// (ladders exist on the compiled kernel sets, at most 128 degrees of freedom), so the two streams never meet.
//
// One lane per pair; the dimension and the ledger size are runtime values (one kernel per dtype).  Both energies are read
// for every pair, x and the ledger rows only for accepted pairs.  blockIdx.y is the pair of rungs, so a block never
// straddles two of them; the blocks of a pair walk its M slots grid-stride.  Per pair of rungs the attempted and accepted
// swaps are counted exactly: ballot + popcount per wavefront, the block's wavefronts summed in LDS, one atomic per block
// and counter.  (The first version, one atomic per wavefront on a grid of one lane per pair, spent most of its 136 us at
// 2^20 chains x 16 parameters on ~15 000 same-address atomics.)
#include <algorithm>

#include "me_device.h"

namespace me {
namespace {

constexpr int kSwapThreads = 256;
constexpr int kSwapBlocks = 2048;     // blocks per round (about 8 per CU), shared out among the pairs of rungs

template <typename R>
struct SwapArgs {
  R *x, *energy;
  const R *ladder;                  // (inv_temp, inv_temp_log2e) per rung, the step kernels' table
  unsigned long long *pair_counts;  // [2 k] attempted, [2 k + 1] accepted for the pair (k, k + 1)
  long long n, rung_chains;
  unsigned long long chain_offset, round;
  uint32_t seed_lo, seed_hi;
  int d, n_terms, first_rung, tiled;
};

// rows [0, rows) of chains a and b exchanged, through either state accessor (Field: component-major, TiledField: tile-major);
// eight rows' loads are in flight before their stores
template <class F>
__device__ __forceinline__ void swap_rows(const F &f, unsigned int off_a, unsigned int off_b, int rows) {
  constexpr int B = 8;
  for (int r0 = 0; r0 < rows; r0 += B) {
    decltype(f.load(0, 0u)) va[B], vb[B];
#pragma unroll
    for (int u = 0; u < B; ++u)
      if (r0 + u < rows) {
        va[u] = f.load(r0 + u, off_a);
        vb[u] = f.load(r0 + u, off_b);
      }
#pragma unroll
    for (int u = 0; u < B; ++u)
      if (r0 + u < rows) {
        f.store(r0 + u, off_a, vb[u]);
        f.store(r0 + u, off_b, va[u]);
      }
  }
}

// one pair: chain a = k M + j of rung k and chain b = a + M of rung k + 1; returns whether they swapped
template <typename R>
__device__ __forceinline__ bool swap_pair(const SwapArgs<R> &s, const Field<R> &fe, int k, long long j, R dbeta, R dbeta_log2e) {
  using N_ = Num<R>;
  const long long a = (long long)k * s.rung_chains + j, b = a + s.rung_chains;
  const unsigned int ea_off = (unsigned int)a * (unsigned int)sizeof(R), eb_off = (unsigned int)b * (unsigned int)sizeof(R);
  const R ea = chain_energy(fe, ea_off, s.n_terms), eb = chain_energy(fe, eb_off, s.n_terms);
  const unsigned long long gid = s.chain_offset + (unsigned long long)a;
  U4 ctr;
  ctr.x = (uint32_t)gid;
  ctr.y = (uint32_t)(gid >> 32);
  ctr.z = (uint32_t)s.round;
  ctr.w = ((uint32_t)(s.round >> 32) << 16) | 0xffffu;
  const R u = N_::unit(philox4x32_10(ctr, s.seed_lo, s.seed_hi).x);
  // delta = (1/T_k - 1/T_{k+1}) (E_a - E_b); uphill(u, d, c, c log2e) tests u <= exp(-d c) with d = E_b - E_a = -(E_a - E_b)
  const R delta = dbeta * (ea - eb);
  const bool accept = N_::finite(ea) && N_::finite(eb) && (delta >= R(0) || N_::uphill(u, eb - ea, dbeta, dbeta_log2e));
  if (accept) {
    if (s.tiled) swap_rows(TiledField<R>(s.x, s.n, s.d), tiled_offset<R>(a, s.d), tiled_offset<R>(b, s.d), s.d);
    else swap_rows(Field<R>(s.x, s.n, s.d), ea_off, eb_off, s.d);
    swap_rows(fe, ea_off, eb_off, s.n_terms);
  }
  return accept;
}

template <typename R>
__global__ void __launch_bounds__(kSwapThreads) k_replica_swap(SwapArgs<R> s) {
  const int k = s.first_rung + 2 * (int)blockIdx.y;          // the pair of rungs (k, k + 1): block-uniform
  const Field<R> fe(s.energy, s.n, s.n_terms);
  const R dbeta = s.ladder[2 * k] - s.ladder[2 * k + 2], dbeta_log2e = s.ladder[2 * k + 1] - s.ladder[2 * k + 3];
  unsigned int attempted = 0, accepted = 0;                   // this wavefront's, wave-uniform
  for (long long j = (long long)blockIdx.x * kSwapThreads + threadIdx.x; j < s.rung_chains; j += (long long)gridDim.x * kSwapThreads) {
    // (M is a multiple of 64: whole wavefronts run each iteration)
    const bool acc = swap_pair(s, fe, k, j, dbeta, dbeta_log2e);
    attempted += (unsigned int)__popcll(__ballot(true));
    accepted += (unsigned int)__popcll(__ballot(acc));
  }
  __shared__ unsigned int wave_counts[kSwapThreads / 64][2];
  if ((threadIdx.x & 63) == 0) {
    wave_counts[threadIdx.x >> 6][0] = attempted;
    wave_counts[threadIdx.x >> 6][1] = accepted;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kSwapThreads / 64; ++w) total += wave_counts[w][threadIdx.x];
    if (total) atomicAdd(&s.pair_counts[2 * k + threadIdx.x], total);
  }
}

template <typename R>
hipError_t launch(void *x, void *energy, long long n, int d, int n_terms, bool tiled_state, const void *ladder, int n_rungs,
                  unsigned long long round, unsigned long long chain_offset, unsigned long long seed,
                  unsigned long long *pair_counts, hipStream_t stream) {
  SwapArgs<R> s;
  s.x = (R *)x;
  s.energy = (R *)energy;
  s.ladder = (const R *)ladder;
  s.pair_counts = pair_counts;
  s.n = n;
  s.rung_chains = n / n_rungs;
  s.first_rung = (int)(round & 1ull);
  const int n_pairs = (n_rungs - s.first_rung) / 2;          // pairs of rungs (k, k+1), k = first, first + 2, ... < K - 1
  s.chain_offset = chain_offset;
  s.round = round;
  s.seed_lo = (uint32_t)seed;
  s.seed_hi = (uint32_t)(seed >> 32);
  s.d = d;
  s.n_terms = n_terms;
  s.tiled = tiled_state ? 1 : 0;
  if (n_pairs == 0) return hipSuccess;         // one rung, or two rungs in an odd round
  const long long per_pair = std::min<long long>((s.rung_chains + kSwapThreads - 1) / kSwapThreads, std::max(kSwapBlocks / n_pairs, 1));
  hipLaunchKernelGGL(k_replica_swap<R>, dim3((unsigned)per_pair, (unsigned)n_pairs), dim3(kSwapThreads), 0, stream, s);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_replica_swap(void *x, void *energy, long long n, int d, int n_terms, bool tiled_state, int dtype,
                               const void *ladder, int n_rungs, unsigned long long round, unsigned long long chain_offset,
                               unsigned long long seed, unsigned long long *pair_counts, hipStream_t stream) {
  if (n_rungs < 1 || n % ((long long)n_rungs * 64) != 0 || !ladder || !pair_counts) return hipErrorInvalidValue;
  if (dtype == ME_F32)
    return launch<float>(x, energy, n, d, n_terms, tiled_state, ladder, n_rungs, round, chain_offset, seed, pair_counts, stream);
  return launch<double>(x, energy, n, d, n_terms, tiled_state, ladder, n_rungs, round, chain_offset, seed, pair_counts, stream);
}

}  // namespace me
