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
#include <cmath>
#include <string>
#include <vector>

#include "me_device.h"
#include "me_engine.h"

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

// ---- entry points: temperature ladders and replica exchange ---------------------------------------------------------------
// why this engine cannot carry a ladder (ME_OK: it can)
int check_ladder_capable(me_engine *e) {
  if (e->ks->n_real < 0)
    return fail(e, ME_ERR_UNSUPPORTED, "temperature ladders are not available on the runtime-dimension kernel set (beyond " +
                                           std::to_string(kMaxRegisterDof) + " real degrees of freedom)");
  if (e->energy_kind == ME_ENERGY_DENSE_QUAD && e->nr == 64 && e->nc == 0)
    return fail(e, ME_ERR_UNSUPPORTED, "temperature ladders are not available on the matrix-core kernels of the dense 64-parameter form");
  return refuse_stale_total(e, "temperature ladders are");
}
int free_ladder(me_engine *e) {
  ME_HIP(e, hipStreamSynchronize(e->stream));     // launches in flight read the table
  e->ladder = me_engine::Ladder();
  e->samples.rows = 0;        // recorded energies belong to the rungs of the ladder they were taken under
  return ME_OK;
}
}  // namespace
}  // namespace me

using namespace me;

extern "C" {

int me_set_temperature_ladder(me_engine *e, const double *temps, int32_t n_rungs) {
  if (!e) return ME_ERR_INVALID;
  if (n_rungs < 0 || (n_rungs > 0 && !temps)) return fail(e, ME_ERR_INVALID, "n_rungs must be >= 0 and temps given");
  ME_HIP(e, hipSetDevice(e->device));
  if (n_rungs == 0) return free_ladder(e);
  int rc = check_ladder_capable(e);
  if (rc != ME_OK) return rc;
  for (int k = 0; k < n_rungs; ++k) {
    if (!(std::isfinite(temps[k]) && temps[k] > 0))
      return fail(e, ME_ERR_INVALID, "ladder temperatures must be finite and > 0");
    if (k > 0 && !(temps[k] > temps[k - 1]))
      return fail(e, ME_ERR_INVALID, "ladder temperatures must be strictly increasing");
  }
  if (e->n % (64ll * n_rungs) != 0)
    return fail(e, ME_ERR_INVALID, "n_chains must be a multiple of 64 * n_rungs: every rung is a run of whole 64-chain tiles");
  // the step kernels' scalar constants, per rung (me_kernels.hip: typed)
  std::vector<double> table(2 * (size_t)n_rungs);
  for (int k = 0; k < n_rungs; ++k) {
    table[2 * k] = 1.0 / temps[k];
    table[2 * k + 1] = 1.4426950408889634 / temps[k];
  }
  if ((rc = free_ladder(e)) != ME_OK) return rc;
  ME_HIP(e, upload(e->ladder.table, table.data(), table.size(), e->dtype));
  ME_HIP(e, e->ladder.pair_counts.resize(2 * (size_t)std::max(n_rungs - 1, 1) * sizeof(unsigned long long)));
  ME_HIP(e, hipMemset(e->ladder.pair_counts.get(), 0, e->ladder.pair_counts.bytes()));
  e->ladder.temps.assign(temps, temps + n_rungs);
  e->ladder.n_rungs = n_rungs;
  return ME_OK;
}

int me_temperature_ladder(me_engine *e, double *temps, int32_t capacity, int32_t *n_rungs) {
  if (!e || !n_rungs) return ME_ERR_INVALID;
  *n_rungs = e->ladder.n_rungs;
  if (e->ladder.n_rungs == 0 || !temps) return ME_OK;      // (temps = NULL: the count only)
  if (capacity < e->ladder.n_rungs) return fail(e, ME_ERR_INVALID, "temps must hold n_rungs doubles");
  std::copy(e->ladder.temps.begin(), e->ladder.temps.end(), temps);
  return ME_OK;
}

// One round: rung k pairs with rung k+1 for every k = round (mod 2); slot j of the two rungs swaps x and its energy-ledger
// rows with the Metropolis probability of the two temperatures; the pair's attempted / accepted counts are added to.
int me_replica_exchange(me_engine *e, int32_t n_rounds) {
  if (!e) return ME_ERR_INVALID;
  if (n_rounds < 0) return fail(e, ME_ERR_INVALID, "n_rounds must be >= 0");
  if (e->ladder.n_rungs == 0) return fail(e, ME_ERR_STATE, "no temperature ladder: call me_set_temperature_ladder first");
  ME_HIP(e, hipSetDevice(e->device));
  const auto swap = e->dtype == ME_F32 ? launch<float> : launch<double>;
  for (int i = 0; i < n_rounds; ++i) {
    ME_HIP(e, swap(e->x.get(), e->energy.get(), e->n, e->d, e->n_terms, e->x_tiled, e->ladder.table.get(), e->ladder.n_rungs, e->ladder.round,
                   e->chain_offset, e->seed, e->ladder.pair_counts.get<unsigned long long>(), e->stream));
    e->ladder.round += 1;
  }
  return ME_OK;
}

int me_replica_stats(me_engine *e, uint64_t *round, uint64_t *attempted, uint64_t *accepted, int32_t n_pairs) {
  if (!e) return ME_ERR_INVALID;
  if (e->ladder.n_rungs == 0) return fail(e, ME_ERR_STATE, "no temperature ladder");
  if (n_pairs != e->ladder.n_rungs - 1) return fail(e, ME_ERR_INVALID, "n_pairs must be n_rungs - 1");
  if (round) *round = e->ladder.round;
  if (n_pairs == 0) return ME_OK;
  ME_HIP(e, hipSetDevice(e->device));
  std::vector<unsigned long long> counts(2 * (size_t)n_pairs);
  ME_HIP(e, hipMemcpyAsync(counts.data(), e->ladder.pair_counts.get(), counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           e->stream));
  ME_HIP(e, hipStreamSynchronize(e->stream));
  for (int k = 0; k < n_pairs; ++k) {
    if (attempted) attempted[k] = counts[2 * k];
    if (accepted) accepted[k] = counts[2 * k + 1];
  }
  return ME_OK;
}

int me_set_replica_stats(me_engine *e, uint64_t round, const uint64_t *attempted, const uint64_t *accepted, int32_t n_pairs) {
  if (!e) return ME_ERR_INVALID;
  if (e->ladder.n_rungs == 0) return fail(e, ME_ERR_STATE, "no temperature ladder");
  if (n_pairs != e->ladder.n_rungs - 1) return fail(e, ME_ERR_INVALID, "n_pairs must be n_rungs - 1");
  if (n_pairs > 0 && (!attempted || !accepted)) return fail(e, ME_ERR_INVALID, "attempted / accepted missing");
  std::vector<unsigned long long> counts(2 * (size_t)n_pairs);
  for (int k = 0; k < n_pairs; ++k) {
    if (accepted[k] > attempted[k]) return fail(e, ME_ERR_INVALID, "accepted swaps exceed attempted ones");
    counts[2 * k] = attempted[k];
    counts[2 * k + 1] = accepted[k];
  }
  ME_HIP(e, hipSetDevice(e->device));
  if (n_pairs > 0) {
    ME_HIP(e, hipMemcpyAsync(e->ladder.pair_counts.get(), counts.data(), counts.size() * sizeof(unsigned long long), hipMemcpyHostToDevice,
                             e->stream));
    ME_HIP(e, hipStreamSynchronize(e->stream));
  }
  e->ladder.round = round;
  return ME_OK;
}

}  // extern "C"
