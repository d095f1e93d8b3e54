// What the three matrix-core step kernels of the dense quadratic form on 64 real parameters share -- k_step_dense64_f64
// (me_dense_f64.h), k_step_dense64_bf16x3 (me_dense_bf16x3.h) and k_step_dense64_mfma (me_dense_mfma.h): the draws, the
// accept decision (as a function for one of them, see dense64_decide) and, for the two float32 kernels, the chain-per-lane tile.  The products and the loops over the tiles are
// each kernel's own; all three end in publish_step (me_device.h).
#pragma once

#include "me_device.h"

namespace me {

// Philox block b of a chain's step: the standard normals of parameters 4 b .. 4 b + 3 (two Box-Muller pairs)
template <typename R>
__device__ __forceinline__ void dense64_normals(const StepArgs<R> &a, unsigned long long gid, unsigned long long step, int b, R (&g)[4]) {
  const U4 o = philox_block(gid, step, b, a.seed_lo, a.seed_hi);
  Num<R>::normal_pair(o.x, o.y, g[0], g[1]);
  Num<R>::normal_pair(o.z, o.w, g[2], g[3]);
}
// the accept uniform: word 64 of the step = block 16, output 0
template <typename R>
__device__ __forceinline__ R dense64_accept_uniform(const StepArgs<R> &a, unsigned long long gid, unsigned long long step) {
  return Num<R>::unit(philox_block(gid, step, 16, a.seed_lo, a.seed_hi).x);
}

// The accept decision of one chain (metropolis_decision, :319-338) and what follows from it for the chain's energy and
// width.  wall_value = row 0 of the proposal, read only where the hard wall is on.  `commit(accept)` is the kernel's own
// way of making the accepted proposal the state; it runs between the decision and the energy / width updates, where
// the kernels had it (results are compared bitwise).  Only k_step_dense64_bf16x3 calls it: k_step_dense64_f64 and
// k_step_dense64_mfma spell the same lines out, because each of them ran measurably slower through this function (see there).
template <typename R, class Commit>
__device__ __forceinline__ bool dense64_decide(const StepArgs<R> &a, bool walled, const R &wall_value, R &e, R e_new, R u, bool live,
                                               R &w, bool &bad_energy, Commit &&commit) {
  using N_ = Num<R>;
  bool rejected = false;
  if (walled) rejected = !(N_::abs_(wall_value) < a.reject_bound);
  const R diff = e_new - e;
  bool accept = diff <= R(0);
  if (a.temp > R(0)) accept = accept || N_::uphill(u, diff, a.inv_temp, a.inv_temp_log2e);
  accept = accept && !rejected;
  bad_energy |= (live && !rejected && !N_::finite(e_new));
  commit(accept);
  e = accept ? e_new : e;
  w = N_::adapt(w, accept, a.ratio, a.p, a.damping, a.up, a.down);
  return accept;
}

// The float32 tile: one wavefront = 64 chains, one chain per lane with its 64 rows, energy and width in registers; the
// proposals x' are parked in LDS ([64][THREADS] floats, lane-linear) between their production and the dot product / commit.
// Every lane stays active (MFMA and permlane need the whole wavefront): tail lanes shadow the last chain.
template <int THREADS>
struct Dense64Tile {
  static constexpr int D = 64;
  const XField<float, D> fx;      // tile-major: a wavefront's 64 rows are one contiguous 16 KiB block
  const Field<float> fe, fw;
  float *const lds_xp;            // this lane's column of the proposals, stride THREADS
  bool live = false;
  unsigned int coff = 0, xoff = 0;
  unsigned long long gid = 0;
  float x[D], e = 0.0f, w = 0.0f;

  __device__ __forceinline__ Dense64Tile(const StepArgs<float> &a, float *proposals)
      : fx(a.x, a.n), fe(a.energy, a.n, 1), fw(a.width, a.n, 1), lds_xp(proposals + threadIdx.x) {}
  __device__ __forceinline__ float &xp(int row) const { return lds_xp[row * THREADS]; }

  // the tile of the wavefront whose first chain is `base`
  // Loads are issued in the order the first sweep consumes them (width, then rows 0, 1, 2, ...): memory returns in
  // order, so the s_waitcnt before the first use of row 4b can leave the later rows in flight behind the Philox
  // work.  Left to the scheduler the rows were issued scrambled and the first use waited for (almost) all of them.
  __device__ __forceinline__ void load(const StepArgs<float> &a, long long base) {
    const long long c_raw = base + (threadIdx.x & 63);
    live = c_raw < a.n;
    const long long c = live ? c_raw : a.n - 1;
    coff = (unsigned int)c * 4u;
    xoff = fx.offset(c);
    gid = a.chain_offset + (unsigned long long)c;
    w = fw.load(0, coff);
    e = fe.load(0, coff);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      x[d] = fx.load(d, xoff);
      if ((d & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the accepted proposal becomes the state
  __device__ __forceinline__ void commit(bool accept) {
    if (accept) {
#pragma unroll
      for (int d = 0; d < D; ++d) x[d] = xp(d);
    }
  }
  __device__ __forceinline__ void store() const {
    if (live) {
#pragma unroll
      for (int d = 0; d < D; ++d) fx.store(d, xoff, x[d]);
      fe.store(0, coff, e);
      fw.store(0, coff, w);
    }
  }
};

}  // namespace me
