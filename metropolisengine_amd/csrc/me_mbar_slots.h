// The device side that the histogram units share (me_mbar_hist.hip: the reweighted masses; me_mbar_hist_cov.hip: the slot
// Gram sums behind their error bars; me_mbar_hist2d.hip: the joint masses of two quantities, whose "slot" is a cell of the
// grid): the slot of a value, the wavefront-private accumulation of one item's 64 samples into a table [rows][n_slots] in LDS,
// the reduction of the block partials and the normalisation of a row.  me_mbar_hist.hip's header describes the scheme
// and its summation order; nothing here depends on what a row of the table means (a temperature there, a column of the weight
// matrix in me_mbar_hist_cov.hip), and the order in which a cell (row, slot) receives its terms depends on the samples' slots
// and order alone, not on the number of rows.
#pragma once

#include "me_mbar.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {
namespace {

#ifndef ME_HIST_DENSE
#define ME_HIST_DENSE 8
#endif
// lanes of a wavefront sharing a slot beyond which they are summed by butterfly (0: every group, 64: none; the build uses 8,
// the other values are there to be measured against: profiles/mbar_profile.txt)
constexpr int kDense = ME_HIST_DENSE;

// the slot of value a: searchsorted(edges, a, side = "right") - 1 mapped onto [0, n_bins + 3); `top` = the largest power of
// two <= n_edges (wave-uniform), so the loop takes floor(log2 n_edges) + 1 <= 9 steps
__device__ __forceinline__ int slot_of(const double *edges, int n_edges, int top, double a) {
  int pos = 0;                                  // edges <= a
  for (int step = top; step >= 1; step >>= 1) {
    const int cand = pos + step;
    const bool ok = cand <= n_edges && edges[min(cand, n_edges) - 1] <= a;
    pos = ok ? cand : pos;
  }
  const int n_bins = n_edges - 1;
  return a != a ? n_bins + 2 : pos == 0 ? n_bins : pos == n_edges ? n_bins + 1 : pos - 1;
}

// Adds w[r] of every lane with slot >= 0 to table[r * n_slots + slot], r < n_rows <= kRows (n_rows wave-uniform), for the 64
// lanes of one item; `table` is the calling wavefront's own.  EVERY lane of the wavefront calls it (slot = -1 and w = 0 for a
// lane without a sample): the loop conditions are ballots, wave-uniform, and no cross-lane operation runs under a partial
// lane mask.  below_me = the mask of the lower lanes.  Steps 1 to 3 of me_mbar_hist.hip's header.
template <int kRows>
__device__ __forceinline__ void slot_accumulate(double *table, int n_slots, int n_rows, int slot, const double (&w)[kRows], int lane,
                                                unsigned long long below_me) {
  unsigned long long todo = __ballot(slot >= 0);
  int rank = 0, rounds = 0;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int s = __builtin_amdgcn_readlane(slot, leader);
    const bool mine = slot == s;
    const unsigned long long group = __ballot(mine);
    const int size = __popcll(group);
    if (size > kDense) {
#pragma unroll
      for (int t = 0; t < kRows; ++t)
        if (t < n_rows) {
          const double sum = wave_sum(mine ? w[t] : 0.0);
          if (lane == 0) table[t * n_slots + s] = table[t * n_slots + s] + sum;
        }
    } else {
      rank = mine ? __popcll(group & below_me) + 1 : rank;
      rounds = max(rounds, size);
    }
    todo &= ~group;
  }
  for (int round = 1; round <= rounds; ++round) {
    // The lanes of one round hold different slots, so its plain loads and stores never meet in one address.  A round
    // must see the table as the rounds before it left it, through OTHER lanes: a wavefront's LDS operations issue and
    // complete in program order, and the wavefront-scope fence with the barrier keeps the compiler from moving a
    // round's non-atomic LDS accesses across those of its neighbours.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (rank == round) {
#pragma unroll
      for (int t = 0; t < kRows; ++t)
        if (t < n_rows) table[t * n_slots + slot] = table[t * n_slots + slot] + w[t];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the wavefront tables [kWaves][rows_stride][n_slots] of a block in wavefront order -> partials[block][rows_stride][n_slots],
// rows < n_rows (after the block's barrier)
__device__ __forceinline__ void slot_tables_store(const double *tables, int rows_stride, int n_rows, int n_slots, double *partials) {
  for (int c = threadIdx.x; c < n_rows * n_slots; c += kThreads) {
    double sum = tables[c];
    for (int k = 1; k < kWaves; ++k) sum = sum + tables[k * rows_stride * n_slots + c];
    partials[(size_t)blockIdx.x * rows_stride * n_slots + c] = sum;
  }
}

// block (slot, row): the block partials [block][rows_stride][n_slots] of one row and one slot in a fixed order (lane l adds
// blocks l, l + 256, ... in order, then the butterfly and the wavefronts in order) into sums[row][slot]; with `counts` the
// blocks of row 0 also add the slot's counts (integers)
__global__ void __launch_bounds__(kThreads) k_mbar_hist_sum(const double *partials, const unsigned long long *count_partials, int n_blocks,
                                                            int rows_stride, int n_slots, double *sums, long long *counts) {
  __shared__ double waves[kWaves];
  __shared__ unsigned long long total;
  const int s = blockIdx.x, t = blockIdx.y;
  double v = 0.0;
  for (int b = threadIdx.x; b < n_blocks; b += kThreads) v = v + partials[((size_t)b * rows_stride + t) * n_slots + s];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  if (counts && t == 0) {
    unsigned long long c = 0;
    for (int b = threadIdx.x; b < n_blocks; b += kThreads) c += count_partials[(size_t)b * n_slots + s];
    if (c) atomicAdd(&total, c);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = waves[0];
  for (int k = 1; k < kWaves; ++k) sum = sum + waves[k];
  sums[(size_t)t * n_slots + s] = sum;
  if (counts && t == 0) counts[s] = (long long)total;
}

// block t: mass[t][slot] = sums[t][slot] / (the sum over all slots, in a fixed order)
__global__ void __launch_bounds__(kThreads) k_mbar_hist_normalise(int n_slots, double *mass) {
  __shared__ double waves[kWaves];
  double *row = mass + (size_t)blockIdx.x * n_slots;
  double v = 0.0;
  for (int s = threadIdx.x; s < n_slots; s += kThreads) v = v + row[s];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = waves[0];
  for (int k = 1; k < kWaves; ++k) total = total + waves[k];
  for (int s = threadIdx.x; s < n_slots; s += kThreads) row[s] = row[s] / total;
}

}  // namespace
}  // namespace mbar
}  // namespace me
