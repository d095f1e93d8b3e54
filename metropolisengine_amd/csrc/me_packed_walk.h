// The walks over one chain's tile-major packed covariance / factor that are too large for registers: the streamed
// covariance recursion and the row-by-row Cholesky refreshes.  One definition for the compile-time kernel sets (k_measure's
// STREAM path, k_factor_stream, k_factor_mixed: me_device.h) and the runtime-dimension set (k_measure_runtime_cov,
// k_factor_runtime, k_factor_runtime_complex: me_runtime_dims.hip).  The dimensions are plain arguments: the compile-time
// sets pass constants, which fold after inlining; the runtime set passes its launch arguments.  All forced inline.
// Included by me_device.h (after fma_, Num, tri / cre / cim / cdiag); each lane walks its own chain, entry k of which sits
// 64 k values behind the chain's first (the fields may pass 4 GiB: 64-bit pointers).
#pragma once

namespace me {

// C <- C (i-2)/(i-1) + delta delta^H / i + (sigma^2 / i) I  (k_measure's comment, metropolis_engine.py:416-427) over the
// packed entries in their own order: real rows first, then the Hermitian block as (Re, Im) of the columns j < i and the
// real diagonal.  p: the chain's first entry; delta = x - mu_old is parked in LDS ([D][64], lane-linear, conflict-free) so
// that the walk can be a ROLLED loop: unrolled, 2 080 entries are ~100 KB of code and the kernel becomes instruction-fetch
// bound.  Every batch issues all its loads first (a store to p[.] would otherwise fence the next load: the compiler cannot
// prove the entries distinct), then the updates.  Sums of two products are spelled with fma_ (me_device.h).
template <typename R>
__device__ __forceinline__ void covariance_walk(R *p, R (*delta)[kStepThreads], int nr, int nc, int lane, R inv_i, R cov_keep,
                                                R w2_real, R w2_cplx) {
  constexpr long long ts = 64;
  for (int i = 0; i < nr; ++i) {
    const R di = delta[i][lane];
    int j = 0;
    for (; j + 16 <= i; j += 16) {
      R v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = p[u * ts];
#pragma unroll
      for (int u = 0; u < 16; ++u) p[u * ts] = fma_(di * delta[j + u][lane], inv_i, v[u] * cov_keep);
      p += 16 * ts;
    }
    for (; j + 4 <= i; j += 4) {
      R v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = p[u * ts];
#pragma unroll
      for (int u = 0; u < 4; ++u) p[u * ts] = fma_(di * delta[j + u][lane], inv_i, v[u] * cov_keep);
      p += 4 * ts;
    }
    for (; j < i; ++j) {
      *p = fma_(di * delta[j][lane], inv_i, *p * cov_keep);
      p += ts;
    }
    *p = fma_(w2_real, inv_i, fma_(di * di, inv_i, *p * cov_keep));
    p += ts;
  }
  for (int i = 0; i < nc; ++i) {
    const R ai = delta[nr + i][lane], bi = delta[nr + nc + i][lane];
    int j = 0;
    for (; j + 8 <= i; j += 8) {          // eight (Re, Im) pairs: sixteen loads, then the updates
      R v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = p[u * ts];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const R aj = delta[nr + j + u][lane], bj = delta[nr + nc + j + u][lane];
        p[(2 * u) * ts] = fma_(fma_(ai, aj, bi * bj), inv_i, v[2 * u] * cov_keep);
        p[(2 * u + 1) * ts] = fma_(fma_(bi, aj, -(ai * bj)), inv_i, v[2 * u + 1] * cov_keep);
      }
      p += 16 * ts;
    }
    for (; j < i; ++j) {
      const R aj = delta[nr + j][lane], bj = delta[nr + nc + j][lane];
      const R re = p[0], im = p[ts];
      p[0] = fma_(fma_(ai, aj, bi * bj), inv_i, re * cov_keep);
      p[ts] = fma_(fma_(bi, aj, -(ai * bj)), inv_i, im * cov_keep);
      p += 2 * ts;
    }
    *p = fma_(w2_cplx, inv_i, fma_(fma_(ai, ai, bi * bi), inv_i, *p * cov_keep));
    p += ts;
  }
}

// fc = chol(cv) for the real block of one chain (nr rows), blocked Cholesky-Banachiewicz: L_ij = (C_ij - sum_{k<j} L_ik
// L_jk) / L_jj.  ROWS rows are built together in LDS (lds[ROWS * nr][64], row r of the block at lds + r * nr, lane-linear)
// so that every finished L_jk that is loaded serves ROWS dot products: the traffic is nr^3 / (6 ROWS) loads per chain (64
// parameters, ROWS = 4: 11 k loads = 44 KB in float32).  The finished rows are re-read from the factor field itself, by
// the lane that wrote them: program order suffices.  NT: the covariance is read and the factor written non-temporally.
// Every multiply-add is an explicit fma_: the compile-time and the runtime-dimension kernels must round alike, and left as
// `s += a * b` hipcc fuses by the shape of the surrounding block, which differs once the dimensions are constants.
// Slow by construction -- an order of magnitude above a measure() with the pooled shape -- and there only so that
// cov_mode="reference" keeps the reference's semantics (metropolis_engine.py:416-421 feeding :268-270) at any size.
template <typename R, int ROWS, bool NT>
__device__ __forceinline__ void factor_real_rows(const R *cv, R *fc, int nr, R (*lds)[kStepThreads], int lane, bool &bad_pivot) {
  using N_ = Num<R>;
  auto row_of = [&](int r) { return lds + (size_t)r * nr; };          // rows[r][k][lane] = row_of(r)[k][lane]
  for (int i0 = 0; i0 < nr; i0 += ROWS) {
    const int nrows = nr - i0 < ROWS ? nr - i0 : ROWS;     // (a ragged last block: rows past the matrix are neither read nor written)
    for (int r = 0; r < nrows; ++r) {                      // the covariance rows of the block into LDS
      const R *src = cv + (long long)tri(i0 + r, 0) * 64;
      int j = 0;
      for (; j + 16 <= i0 + r + 1; j += 16) {
        R v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = NT ? __builtin_nontemporal_load(src + (j + u) * 64) : src[(j + u) * 64];
#pragma unroll
        for (int u = 0; u < 16; ++u) row_of(r)[j + u][lane] = v[u];
      }
      for (; j <= i0 + r; ++j) row_of(r)[j][lane] = NT ? __builtin_nontemporal_load(src + j * 64) : src[j * 64];
    }
    // Columns left of the block: every finished row j < i0 serves all rows of the block.  The walk is bound by memory
    // LATENCY (one wavefront per SIMD at most, every batch of loads a round trip, and column j needs column j - 1 of the
    // block's rows): FOUR finished rows are fetched together -- their first j entries in batches of 4 x 16 loads, then the
    // ten entries of the little triangle between them -- and the four columns are finished one after the other from
    // registers (one row per visit with two or three dependent round trips each took twice as long: 8.0 -> 4.5 ms per
    // measure at 100 parameters x 2^14 chains in float64, tools/dev/time_compiled_vs_runtime.py).
    int j = 0;
    for (; j + 4 <= i0; j += 4) {
      const R *lj[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) lj[q] = fc + (long long)tri(j + q, 0) * 64;
      R sum[4][ROWS];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) sum[q][r] = R(0);
      int k = 0;
      for (; k + 16 <= j; k += 16) {
        R f[4][16];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int u = 0; u < 16; ++u) f[q][u] = lj[q][(k + u) * 64];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          R v[ROWS];
#pragma unroll
          for (int r = 0; r < ROWS; ++r) v[r] = r < nrows ? row_of(r)[k + u][lane] : R(0);
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) sum[q][r] = fma_(v[r], f[q][u], sum[q][r]);
        }
      }
      for (; k < j; k += 4) {                             // (j is a multiple of 4)
        R f[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int u = 0; u < 4; ++u) f[q][u] = lj[q][(k + u) * 64];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          R v[ROWS];
#pragma unroll
          for (int r = 0; r < ROWS; ++r) v[r] = r < nrows ? row_of(r)[k + u][lane] : R(0);
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) sum[q][r] = fma_(v[r], f[q][u], sum[q][r]);
        }
      }
      R t[4][4];                                          // L[j + q][j + p], p <= q
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p <= q; ++p) t[q][p] = lj[q][(j + p) * 64];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const R inv = R(1) / t[q][q];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
          if (r < nrows) {
            R acc = sum[q][r];
#pragma unroll
            for (int p = 0; p < q; ++p) acc = fma_(row_of(r)[j + p][lane], t[q][p], acc);
            row_of(r)[j + q][lane] = (row_of(r)[j + q][lane] - acc) * inv;
          }
      }
    }
    for (; j < i0; ++j) {                                 // (at most three rows left)
      const R *lj = fc + (long long)tri(j, 0) * 64;
      R sum[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) sum[r] = R(0);
      constexpr int kBatch = 16;
      int k = 0;
      for (; k + kBatch <= j; k += kBatch) {
        R f[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) f[u] = lj[(k + u) * 64];
#pragma unroll
        for (int u = 0; u < kBatch; ++u)
#pragma unroll
          for (int r = 0; r < ROWS; ++r)
            if (r < nrows) sum[r] = fma_(row_of(r)[k + u][lane], f[u], sum[r]);
      }
      for (; k < j; ++k) {
        const R f = lj[k * 64];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
          if (r < nrows) sum[r] = fma_(row_of(r)[k][lane], f, sum[r]);
      }
      const R inv = R(1) / lj[j * 64];
#pragma unroll
      for (int r = 0; r < ROWS; ++r)
        if (r < nrows) row_of(r)[j][lane] = (row_of(r)[j][lane] - sum[r]) * inv;
    }
    for (int r = 0; r < nrows; ++r) {                    // the triangle inside the block: rows depend on each other, everything is in LDS
      const int i = i0 + r;
      for (int j = i0; j < i; ++j) {
        const int rj = j - i0;
        R t = R(0);
        for (int k = 0; k < j; ++k) t = fma_(row_of(r)[k][lane], row_of(rj)[k][lane], t);
        row_of(r)[j][lane] = (row_of(r)[j][lane] - t) / row_of(rj)[j][lane];
      }
      R t = row_of(r)[i][lane];
      for (int k = 0; k < i; ++k) t = fma_(-row_of(r)[k][lane], row_of(r)[k][lane], t);
      if (!(t > R(0))) { bad_pivot = true; t = R(1e-30); }
      row_of(r)[i][lane] = N_::sqrt_(t);
    }
    for (int r = 0; r < nrows; ++r) {                    // finished rows out
      R *dst = fc + (long long)tri(i0 + r, 0) * 64;
      for (int j = 0; j <= i0 + r; ++j) {
        if constexpr (NT) __builtin_nontemporal_store(row_of(r)[j][lane], dst + j * 64);
        else dst[j * 64] = row_of(r)[j][lane];
      }
    }
  }
}

// The Hermitian block of one chain's factor (nc rows behind pr real entries): L = chol(conj K) (quirk Q3,
// metropolis_engine.py:292-298), row by row, every operand through global memory -- a finished L_ik is re-read from the
// factor field the lane itself wrote.  Written for correctness, not speed (a dependent load per multiply-add).
template <typename R, bool NT>
__device__ __forceinline__ void factor_complex_rows(const R *cv, R *fc, int pr, int nc, bool &bad_pivot) {
  using N_ = Num<R>;
  auto in = [&](int k) -> R { return NT ? __builtin_nontemporal_load(cv + (long long)k * 64) : cv[(long long)k * 64]; };
  for (int i = 0; i < nc; ++i)
    for (int j = 0; j <= i; ++j) {
      R sr = j < i ? in(cre(pr, i, j)) : in(cdiag(pr, i));
      R si = j < i ? -in(cim(pr, i, j)) : R(0);                 // conj(K)
      for (int k = 0; k < j; ++k) {                              // s -= L_ik conj(L_jk)
        const R ar = fc[(long long)cre(pr, i, k) * 64], ai = fc[(long long)cim(pr, i, k) * 64];
        const R br = fc[(long long)cre(pr, j, k) * 64], bi = fc[(long long)cim(pr, j, k) * 64];
        sr = fma_(-ai, bi, fma_(-ar, br, sr));
        si = fma_(ar, bi, fma_(-ai, br, si));
      }
      if (j < i) {
        const R d = fc[(long long)cdiag(pr, j) * 64];
        fc[(long long)cre(pr, i, j) * 64] = sr / d;
        fc[(long long)cim(pr, i, j) * 64] = si / d;
      } else {
        if (!(sr > R(0))) { bad_pivot = true; sr = R(1e-30); }
        fc[(long long)cdiag(pr, i) * 64] = N_::sqrt_(sr);
      }
    }
}

}  // namespace me
