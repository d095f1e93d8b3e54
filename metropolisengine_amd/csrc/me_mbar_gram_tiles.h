// The device side that the kernels forming W^T W on the matrix cores share (me_mbar_cov.hip: k_mbar_gram, the Gram matrix of up
// to 128 columns behind the error bars; me_mbar_newton.hip: k_mbar_newton_pass, the ladder columns alone, once per Newton pass):
// the walk over the lower-triangle 16 x 16 tiles of G, the lane's place in a v_mfma_f64_16x16x4_f64 fragment, the staging of a
// sub-tile of W in LDS that the fragments are read from, and the packed lower triangle the accumulators are written to.
//
// Tiles.  G is cut into 16 x 16 tiles (I, J); only I >= J is computed, as pair p = I (I + 1) / 2 + J (pair_row, pair_offsets).
// Fragments.  One instruction adds the product of 4 samples: lane l feeds A[i = l & 15][k = l >> 4] = W[n0 + k][16 I + i] and
// B[k = l >> 4][j = l & 15] = W[n0 + k][16 J + j], and receives rows (l >> 4) + 4 r (r < 4) of column l & 15 of the tile.
// Staging.  A sub-tile is 16 samples (4 instructions deep) as float64 [16][cp]: fragment_source points a lane at &W[4 ks + (l >>
// 4)][l & 15] of k-step ks, from where the operand of tile column I is 16 I doubles on.  A half-wavefront reads 2 rows x 16
// consecutive columns, so the rows must lie 16 doubles apart modulo 32 (64 banks of 4 bytes).  What cp is depends on who fills
// the rows: padded_row for k_mbar_gram, where the 16 lanes of a row write consecutive columns (any multiple of 16 that is
// not one of 32); lane_row for k_mbar_newton_pass, where 16 lanes write one column of 16 rows, so the rows must also be an odd
// number of doubles apart: 17 modulo 32, which costs the reads one two-way conflict (rows 0 and 1 meet in one bank pair).
#pragma once

#include "me_mbar.h"

namespace me {
namespace mbar {

constexpr int kSub = 16;                        // samples per sub-tile in LDS

typedef double f64x4 __attribute__((ext_vector_type(4)));

// the padded row length of a sub-tile whose rows are written 16 consecutive columns at a time
__host__ __device__ constexpr int padded_row(int n_cols) {
  const int cpad = (n_cols + 15) / 16 * 16;
  return cpad % 32 == 0 ? cpad + 16 : cpad;
}
// ... and of one whose columns are written 16 rows at a time: the least cp >= n_cols with cp = 17 (mod 32)
__host__ __device__ constexpr int lane_row(int n_cols) { return (n_cols + 14) / 32 * 32 + 17; }

// the tile row I of pair p = I (I + 1) / 2 + J among max_tiles tile rows
__host__ __device__ constexpr int pair_row(int p, int max_tiles) {
  int I = 0;
  for (int q = 1; q < max_tiles; ++q) I = p >= q * (q + 1) / 2 ? q : I;
  return I;
}
// the column offsets 16 I and 16 J of pair p
__device__ __forceinline__ void pair_offsets(int p, int max_tiles, int &off_i, int &off_j) {
  int I = 0;
#pragma unroll
  for (int q = 1; q < max_tiles; ++q) I = p >= q * (q + 1) / 2 ? q : I;
  off_i = 16 * I;
  off_j = 16 * (p - I * (I + 1) / 2);
}

// a lane's place in a fragment: k = h4 of the operands (and row h4 + 4 r of the result), i / j = j16
struct Fragment {
  int h4, j16;
};
__device__ __forceinline__ Fragment fragment_of(int lane) { return Fragment{lane >> 4, lane & 15}; }

// &W[4 ks + h4][j16] of the sub-tile `buf` with rows of cp doubles
__device__ __forceinline__ const double *fragment_source(const double *buf, int ks, int cp, const Fragment &fr) {
  return buf + (4 * ks + fr.h4) * cp + fr.j16;
}

// acc += the product of the 4 samples of one k-step for one tile
__device__ __forceinline__ f64x4 gram_mfma(double a, double b, f64x4 acc) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
}

// the index of G[i][j], j <= i, in the packed lower triangle
__host__ __device__ constexpr int packed_index(int i, int j) { return i * (i + 1) / 2 + j; }

// this lane's four entries of the tile at column offsets (off_i, off_j) into the packed lower triangle dst of n_cols columns;
// kAdd: added to what is there
template <bool kAdd = false>
__device__ __forceinline__ void store_lower_tile(double *dst, int off_i, int off_j, const Fragment &fr, int n_cols, const f64x4 &acc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = off_i + fr.h4 + 4 * r, gj = off_j + fr.j16;
    if (gi < n_cols && gj <= gi) dst[packed_index(gi, gj)] = kAdd ? dst[packed_index(gi, gj)] + acc[r] : acc[r];
  }
}

}  // namespace mbar
}  // namespace me
