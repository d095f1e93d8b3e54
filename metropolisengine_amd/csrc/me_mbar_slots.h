// The device side that the histogram units share (me_mbar_hist.hip: the reweighted masses; me_mbar_hist_cov.hip: the slot
// Gram sums behind their error bars; me_mbar_hist2d.hip: the joint masses of two quantities, whose "slot" is a cell of the
// grid; me_mbar_hist2d_cov.hip: the cell Gram sums behind the error bars of those): ONE pass kernel body, slot_pass, and what
// it is made of.  A unit's kernel builds two small policies and calls it:
//   where a sample falls   Slots1d (one edge array, one value column, slot_of) or Slots2d (two of each; the slot is the cell
//                          slot_x (By + 3) + slot_y; a value column that is nullptr is the energy itself);
//   what the rows are      TemperatureRows<R> (row t = the state weight of temperature t of the chunk: the masses) or
//                          GramRows<R> (row r = a column of the weight matrix times the state weight of ONE temperature: the
//                          slot Gram sums).
// Nothing else differs between the units, and nothing in slot_accumulate or behind it depends on what a row means.
//
// The pass.  A block walks its tiles of kTile samples (grid stride); a thread's kItems samples of a tile are kThreads apart.
// The edges sit in LDS (a lane finds its slot by a branch-free binary search, slot_of: at most 9 steps for 257 edges); each
// wavefront owns a private LDS table [R][n_slots] of doubles and, in a unit that counts, [n_slots] counts.  Nothing is shared
// between wavefronts before the end, and NO atomic touches a floating-point number.  d_n (log_denominator_enqueue: padded to
// whole tiles, NaN for an unused sample and for the padding) is the gate: a lane whose d_n is NaN keeps slot = -1 and w = 0.
// How a wavefront adds the 64 weights of one item into its table, all lanes active throughout (slot_accumulate; the loop
// condition is a ballot, wave-uniform; no cross-lane operation ever runs under a partial lane mask):
//   0. in a pass that counts, every lane with a sample adds 1 to its slot's count with an integer LDS atomic (integers: exact
//      in any order);
//   1. the groups of lanes that share a slot are found one by one: the lowest lane not yet matched names the slot (readlane
//      with a wave-uniform lane number), a ballot gives the group and its popcount the group's size;
//   2. a group of more than kDense = 8 lanes is summed at once: wave_sum over the wavefront with +0.0 from the other lanes
//      (exact), lane 0 adds the R sums to the table.  At most 7 such groups exist among 64 lanes;
//   3. a lane of a smaller group keeps its rank r inside the group (popcount of the group's lower lanes).  After the match loop
//      round r = 1 .. (largest such group) lets the lanes of rank r add their own weights to the table themselves: they all
//      hold DIFFERENT slots, so the plain read-add-write of a round touches every address at most once.
// The worst cases are bounded: 64 lanes in one slot cost one match round and R wave_sums; 64 lanes in 64 slots cost 64 match
// rounds (readlane, compare, ballot, popcount, two selects) and ONE round of step 3, not 64 x R wave_sums.  Measured at 2^25
// samples, 8 temperatures, 64 bins (profiles/mbar_profile.txt): 3.2 ms with every value in one bin and 4.2 ms with 64
// different bins per wavefront; summing EVERY group by wave_sum (kDense = 0) takes 3.3 and 40.3 ms, letting every lane add for
// itself (kDense = 64) 7.2 and 3.6 ms.
// Summation order of one cell (row, slot), fixed by the samples' slots and order alone: per item the large groups in order of
// their lowest lane, then the small groups' lanes by rank (lane order inside a group); the items and tiles of a block in order;
// the block's wavefront tables in wavefront order -> partials[block][row][slot] -> k_mbar_hist_sum, in which lane l adds blocks
// l, l + 256, ... in order, then the butterfly and the wavefronts in order.  Neither the slots nor the order depend on what the
// rows are or on their number, and a row's terms are formed by the same instructions at every position of a chunk (`fp
// contract(off)` over all policy code, the fused multiply-adds spelled out, ONE state_weight): a cell is bit for bit the same
// run to run, alone or among any number of rows, whichever unit asks, and through the engine's store or host arrays of the same
// samples in the same order (the values are addressed through strides).
// Registers, LDS and timings of the kernels built from this header against their hand-written predecessors:
// profiles/mbar_slot_skeleton.txt.
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

// the slot of value a: searchsorted(edges, a, side = "right") - 1 mapped onto [0, n_bins + 3); `top` = top_of(n_edges), the
// largest power of two <= n_edges (wave-uniform), so the loop takes floor(log2 n_edges) + 1 <= 9 steps
inline int top_of(int n_edges) {
  int top = 1;
  while (2 * top <= n_edges) top *= 2;
  return top;
}
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
// lane mask.  below_me = the mask of the lower lanes.  Steps 1 to 3 of the header.
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

// the state weight of a sample at one temperature: w_nt = exp(min(-E_n / T_t - d_n - ln_z_t, 0)).  Written ONCE: the masses
// and the state column of the Gram sums are the same bits because they are this function.
__device__ __forceinline__ double state_weight(double e, double dn, double inv, double lz) {
  return math64::exp_nonpos(fmin(__builtin_fma(-e, inv, -dn) - lz, 0.0));
}

// ---- where a sample falls: n_edges() doubles of edges at the front of the LDS, n_slots() slots, and the slot of a sample
// with energy e whose values sit at offset `at` of the value columns
struct Slots1d {
  const double *__restrict__ values;
  int n_bins, top;
  __device__ __forceinline__ int n_edges() const { return n_bins + 1; }
  __device__ __forceinline__ int n_slots() const { return n_bins + 3; }
  __device__ __forceinline__ int slot(const double *s_edges, double, long long at) const {
    return slot_of(s_edges, n_bins + 1, top, values[at]);
  }
};
// edges = [edges_x | edges_y]; a column that is nullptr is the energy itself
struct Slots2d {
  const double *__restrict__ values_x, *__restrict__ values_y;
  int n_bins_x, n_bins_y, top_x, top_y;
  __device__ __forceinline__ int n_edges() const { return n_bins_x + n_bins_y + 2; }
  __device__ __forceinline__ int n_slots() const { return (n_bins_x + 3) * (n_bins_y + 3); }
  __device__ __forceinline__ int slot(const double *s_edges, double e, long long at) const {
    const double a = values_x ? values_x[at] : e, b = values_y ? values_y[at] : e;
    return slot_of(s_edges, n_bins_x + 1, top_x, a) * (n_bins_y + 3) + slot_of(s_edges + n_bins_x + 1, n_bins_y + 1, top_y, b);
  }
};

// ---- what the rows are: n_rows <= kRows of them (wave-uniform), and the weights w[0 .. n_rows) of a used sample
// a chunk of temperatures: inv_temps[t] = 1 / T_t, ln_z with stride 4 (reweight_enqueue's out)
template <int kRows>
struct TemperatureRows {
  double inv[kRows], lz[kRows];
  int n_rows;
  __device__ __forceinline__ TemperatureRows(const double *__restrict__ inv_temps, const double *__restrict__ ln_z, int n_targets)
      : n_rows(n_targets) {
#pragma unroll
    for (int t = 0; t < kRows; ++t) {
      inv[t] = t < n_targets ? inv_temps[t] : 0.0;
      lz[t] = t < n_targets ? ln_z[4 * t] : 0.0;
    }
  }
  __device__ __forceinline__ void weights(double e, double dn, double (&w)[kRows]) const {
#pragma unroll
    for (int t = 0; t < kRows; ++t)
      if (t < n_rows) w[t] = state_weight(e, dn, inv[t], lz[t]);
  }
};
// rows j0 .. j0 + n_rows (j0 + n_rows <= n_rungs + 1) of the weight matrix of ONE temperature *inv_temp, *ln_z, each times the
// state weight w_nt: row j < n_rungs is ladder column j (beta_j, f_j from the ladder table: k_mbar_gram's fill, W_nj = exp(min(
// f_j - E_n / T_j - d_n, 0))), row n_rungs the state column itself, so that the last row of all is w_nt^2
template <int kRows>
struct GramRows {
  double inv, lz, beta[kRows], g[kRows];
  int j0, n_rungs, n_rows;
  __device__ __forceinline__ GramRows(const double *__restrict__ table, int n_rungs_, const double *__restrict__ inv_temp,
                                      const double *__restrict__ ln_z, int j0_, int n_rows_)
      : inv(inv_temp[0]), lz(ln_z[0]), j0(j0_), n_rungs(n_rungs_), n_rows(n_rows_) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const bool ladder = j0 + r < n_rungs;     // (wave-uniform)
      beta[r] = ladder ? table[kBeta + j0 + r] : 0.0;
      g[r] = ladder ? table[kF + j0 + r] : 0.0;
    }
  }
  __device__ __forceinline__ void weights(double e, double dn, double (&w)[kRows]) const {
    const double wt = state_weight(e, dn, inv, lz);
#pragma unroll
    for (int r = 0; r < kRows; ++r)
      if (r < n_rows) {
        const double col = j0 + r < n_rungs ? math64::exp_nonpos(fmin(__builtin_fma(-beta[r], e, g[r]) - dn, 0.0)) : wt;
        w[r] = col * wt;
      }
  }
};

// bytes of dynamic LDS of a pass: [edges | table[kWaves][rows][n_slots] | count[kWaves][n_slots] (a unit that counts)]
constexpr size_t slot_pass_lds(int rows, int n_slots, int n_edges, bool counts) {
  return (size_t)n_edges * sizeof(double) + (size_t)kWaves * n_slots * (rows * sizeof(double) + (counts ? sizeof(unsigned int) : 0));
}

// ---- the rows per pass of the two joint units (host), from the number of cells S ALONE, so that a cell's sums do not depend
// on the two bin counts behind S.  joint_lds_bound: the most LDS a workgroup needs for S cells at R rows, whatever the bin
// counts: the tables and at most 2 S bytes of edges (one axis of a single bin).  joint_cells_at: the most cells with which
// blocks_per_cu workgroups of R rows fit a CU's LDS.  joint_rule_rows: the widest R of `widest`, widest / 2, ..., 1 that allows
// n_cells.  joint_rows_per_pass: `forced` (a unit's forcing macro; 0: none) wherever its table fits 64 KiB, otherwise the rule.
constexpr size_t kCuLds = 160 * 1024;           // LDS of a CU
constexpr size_t joint_lds_bound(int rows, int n_cells, bool counts) {
  return slot_pass_lds(rows, n_cells, 0, counts) + 2 * (size_t)n_cells;
}
constexpr int joint_cells_at(int rows, bool counts, int blocks_per_cu) {
  return (int)(kCuLds / blocks_per_cu / joint_lds_bound(rows, 1, counts));
}
constexpr int joint_rule_rows(int n_cells, int widest, bool counts, int blocks_per_cu) {
  for (int rows = widest; rows > 1; rows /= 2)
    if (n_cells <= joint_cells_at(rows, counts, blocks_per_cu)) return rows;
  return 1;
}
constexpr int joint_rows_per_pass(int n_cells, int widest, bool counts, int blocks_per_cu, int forced) {
  return forced && joint_lds_bound(forced, n_cells, counts) <= 64 * 1024 ? forced
                                                                          : joint_rule_rows(n_cells, widest, counts, blocks_per_cu);
}

// The body of a pass kernel (the header; LDS: slot_pass_lds).  Sample i = record * n_chains + chain has its values at offset
// record * record_stride + chain of the value columns (a column of the engine's store: n_chains, Q n_chains; a host array or
// the energies themselves: n, 0); `d` is padded to whole tiles.  kCounts: the unit keeps integer counts, and a pass with
// with_counts != 0 fills them and writes count_partials[block][n_slots]; partials[block][kRows][n_slots].
// INVARIANT: lanes diverge in ONE place, the `if (dn == dn)` block that fills slot and w.  No lane leaves the item loop, skips an
// item or returns before slot_accumulate, whose ballots, readlane and wave_sum must never run under a partial lane mask.
template <int kRows, bool kCounts, class Where, class Rows>
__device__ __forceinline__ void slot_pass(const double *__restrict__ energies, const double *__restrict__ d, long long n_chains,
                                          long long record_stride, const double *__restrict__ edges, const Where &where,
                                          const Rows &rows, int with_counts, long long n_tiles, double *partials,
                                          unsigned long long *count_partials) {
  extern __shared__ double lds[];
  const int n_edges = where.n_edges(), n_slots = where.n_slots();
  double *s_table = lds + n_edges;
  unsigned int *s_count = reinterpret_cast<unsigned int *>(s_table + kWaves * kRows * n_slots);
  for (int i = threadIdx.x; i < n_edges; i += kThreads) lds[i] = edges[i];
  for (int i = threadIdx.x; i < kWaves * kRows * n_slots; i += kThreads) s_table[i] = 0.0;
  if (kCounts)
    for (int i = threadIdx.x; i < kWaves * n_slots; i += kThreads) s_count[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double *my_table = s_table + wave * kRows * n_slots;
  unsigned int *my_count = s_count + wave * n_slots;
  const unsigned long long below_me = (1ull << lane) - 1ull;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long base = tile * kTile + threadIdx.x;
    long long record = base / n_chains, chain = base - record * n_chains;
#pragma unroll 1
    for (int it = 0; it < kItems; ++it) {
      const long long i = base + (long long)it * kThreads;
      const double dn = d[i];                   // (padded: in bounds; NaN beyond n and for an unused sample)
      int slot = -1;
      double w[kRows];
#pragma unroll
      for (int r = 0; r < kRows; ++r) w[r] = 0.0;
      if (dn == dn) {
        const double e = energies[i];
        slot = where.slot(lds, e, record * record_stride + chain);
        rows.weights(e, dn, w);
        if (kCounts && with_counts) atomicAdd(&my_count[slot], 1u);       // (integers: exact in any order)
      }
      chain += kThreads;
      while (chain >= n_chains) {
        chain -= n_chains;
        record += 1;
      }
      slot_accumulate<kRows>(my_table, n_slots, rows.n_rows, slot, w, lane, below_me);
    }
  }
  __syncthreads();
  slot_tables_store(s_table, kRows, rows.n_rows, n_slots, partials);
  if (kCounts && with_counts)
    for (int c = threadIdx.x; c < n_slots; c += kThreads) {
      unsigned long long sum = 0;
      for (int k = 0; k < kWaves; ++k) sum += s_count[k * n_slots + c];
      count_partials[(size_t)blockIdx.x * n_slots + c] = sum;
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
