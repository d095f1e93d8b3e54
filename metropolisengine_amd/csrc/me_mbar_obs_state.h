// The running state of a reweighting pass over observable columns and its fixed-order joins, shared by me_mbar_obs.hip (the
// weights of a temperature) and me_mbar_perturbed.hip (the weights of a temperature and a perturbed energy H, which also wants
// the second moment of H).  me_mbar_obs.hip's header comment has the formulas and the summation order.  Every function is a
// template over the state type S: TargetState, or PerturbedState, which adds M2_e and nothing else -- so a TargetState sees
// exactly the operations it saw when this code was part of me_mbar_obs.hip.  Include it behind `#pragma clang fp contract(off)`:
// the fused multiply-adds are spelled out where they are meant.
#pragma once

#include "me_mbar.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {

constexpr int kObsTargets = 4;                  // targets per pass
constexpr int kObsCols = 4;                     // observable columns per pass

// what a target's weights share, and what one observable column adds
struct TargetState {
  static constexpr bool kEnergyM2 = false;
  double M, W, Q2, mean_e;
  double mean[kObsCols], M2[kObsCols], C[kObsCols];
};
static_assert(sizeof(TargetState) == 16 * sizeof(double), "partials are addressed as 16 doubles per state");
// ... with M2_e = sum w (e - mean_e)^2 relative to M, carried like a column's M2.  Its weights may be NaN (a bias that is not
// finite): a TargetState's W is 0 (empty) or > 0, and merge() tells the two apart by `W > 0`, which would drop a NaN state as
// empty; a PerturbedState's is empty when W == 0, so a NaN state is joined and makes everything it meets NaN.
struct PerturbedState : TargetState {
  static constexpr bool kEnergyM2 = true;
  double M2_e;
};
static_assert(sizeof(PerturbedState) == 17 * sizeof(double), "one more double than a TargetState");

template <typename S>
__device__ __forceinline__ void clear(S &s) {
  s.M = -INFINITY;
  s.W = s.Q2 = s.mean_e = 0.0;
#pragma unroll
  for (int q = 0; q < kObsCols; ++q) s.mean[q] = s.M2[q] = s.C[q] = 0.0;
  if constexpr (S::kEnergyM2) s.M2_e = 0.0;
}

// one more sample: log weight l, energy e, observable values a[0 .. nq); one exponential, no branch on the data
template <typename S>
__device__ __forceinline__ void add_sample(S &s, double l, double e, const double (&a)[kObsCols], int nq) {
  const bool higher = l > s.M;
  const double x = math64::exp_nonpos(higher ? s.M - l : l - s.M);
  const double scale = higher ? x : 1.0, w = higher ? 1.0 : x;
  const double W = s.W * scale + w;
  const double r = w / W;
  const double mean_e = s.mean_e + (e - s.mean_e) * r;
  const double we = w * (e - mean_e);           // w (E - mean_E_new)
#pragma unroll
  for (int q = 0; q < kObsCols; ++q)
    if (q < nq) {
      const double delta = a[q] - s.mean[q];
      const double mean = s.mean[q] + delta * r;
      s.M2[q] = s.M2[q] * scale + (w * delta) * (a[q] - mean);
      s.C[q] = s.C[q] * scale + delta * we;
      s.mean[q] = mean;
    }
  if constexpr (S::kEnergyM2) s.M2_e = s.M2_e * scale + (e - s.mean_e) * we;
  s.Q2 = s.Q2 * (scale * scale) + w * w;
  s.mean_e = mean_e;
  s.W = W;
  s.M = higher ? l : s.M;
}

__device__ __forceinline__ double pick(bool first, double a, double b) { return first ? a : b; }

// a (earlier in the fixed order) and b joined; an empty side (W = 0) returns the other one unchanged.  Branch-free: the
// general formula is evaluated and then dropped by selects (what it makes of an empty side, NaN included, is never kept).
template <typename S>
__device__ __forceinline__ S merge(const S &a, const S &b, int nq) {
  const bool keep_a = S::kEnergyM2 ? b.W == 0.0 : !(b.W > 0.0);
  const bool keep_b = !keep_a && (S::kEnergyM2 ? a.W == 0.0 : !(a.W > 0.0));
  S r;
  const double M = fmax(a.M, b.M);
  const double sa = math64::exp_nonpos(a.M - M), sb = math64::exp_nonpos(b.M - M);
  const double Wa = a.W * sa, Wb = b.W * sb;
  const double W = Wa + Wb;
  const double fb = Wb / W, cross = Wa * fb;
  const double delta_e = b.mean_e - a.mean_e;
  r.M = pick(keep_a, a.M, pick(keep_b, b.M, M));
  r.W = pick(keep_a, a.W, pick(keep_b, b.W, W));
  r.mean_e = pick(keep_a, a.mean_e, pick(keep_b, b.mean_e, a.mean_e + delta_e * fb));
  r.Q2 = pick(keep_a, a.Q2, pick(keep_b, b.Q2, a.Q2 * (sa * sa) + b.Q2 * (sb * sb)));
  if constexpr (S::kEnergyM2)
    r.M2_e = pick(keep_a, a.M2_e, pick(keep_b, b.M2_e, (a.M2_e * sa + b.M2_e * sb) + (delta_e * delta_e) * cross));
#pragma unroll
  for (int q = 0; q < kObsCols; ++q) {
    if (q < nq) {
      const double delta = b.mean[q] - a.mean[q];
      r.mean[q] = pick(keep_a, a.mean[q], pick(keep_b, b.mean[q], a.mean[q] + delta * fb));
      r.M2[q] = pick(keep_a, a.M2[q], pick(keep_b, b.M2[q], (a.M2[q] * sa + b.M2[q] * sb) + (delta * delta) * cross));
      r.C[q] = pick(keep_a, a.C[q], pick(keep_b, b.C[q], (a.C[q] * sa + b.C[q] * sb) + (delta * delta_e) * cross));
    } else {                                    // (unused columns stay what clear() made them)
      r.mean[q] = a.mean[q], r.M2[q] = a.M2[q], r.C[q] = a.C[q];
    }
  }
  return r;
}

// s and o with the lower lane's first
template <typename S>
__device__ __forceinline__ S merge_ordered(bool o_first, const S &s, const S &o, int nq) {
  S a, b;
  a.M = pick(o_first, o.M, s.M), b.M = pick(o_first, s.M, o.M);
  a.W = pick(o_first, o.W, s.W), b.W = pick(o_first, s.W, o.W);
  a.Q2 = pick(o_first, o.Q2, s.Q2), b.Q2 = pick(o_first, s.Q2, o.Q2);
  a.mean_e = pick(o_first, o.mean_e, s.mean_e), b.mean_e = pick(o_first, s.mean_e, o.mean_e);
  if constexpr (S::kEnergyM2) a.M2_e = pick(o_first, o.M2_e, s.M2_e), b.M2_e = pick(o_first, s.M2_e, o.M2_e);
#pragma unroll
  for (int q = 0; q < kObsCols; ++q) {
    a.mean[q] = pick(o_first, o.mean[q], s.mean[q]), b.mean[q] = pick(o_first, s.mean[q], o.mean[q]);
    a.M2[q] = pick(o_first, o.M2[q], s.M2[q]), b.M2[q] = pick(o_first, s.M2[q], o.M2[q]);
    a.C[q] = pick(o_first, o.C[q], s.C[q]), b.C[q] = pick(o_first, s.C[q], o.C[q]);
  }
  return merge(a, b, nq);
}

template <typename S>
__device__ __forceinline__ S shuffle_xor(const S &s, int d, int nq) {
  S o;
  o.M = __shfl_xor(s.M, d);
  o.W = __shfl_xor(s.W, d);
  o.Q2 = __shfl_xor(s.Q2, d);
  o.mean_e = __shfl_xor(s.mean_e, d);
  if constexpr (S::kEnergyM2) o.M2_e = __shfl_xor(s.M2_e, d);
#pragma unroll
  for (int q = 0; q < kObsCols; ++q) {
    if (q < nq) {
      o.mean[q] = __shfl_xor(s.mean[q], d);
      o.M2[q] = __shfl_xor(s.M2[q], d);
      o.C[q] = __shfl_xor(s.C[q], d);
    } else {
      o.mean[q] = s.mean[q], o.M2[q] = s.M2[q], o.C[q] = s.C[q];
    }
  }
  return o;
}

// butterfly over the wavefront; the lower lane's state is always the first operand, so every lane holds the same result
template <typename S>
__device__ __forceinline__ S wave_merge(S s, int nq) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const S o = shuffle_xor(s, d, nq);
    s = merge_ordered((lane & d) != 0, s, o, nq);
  }
  return s;
}

// the block's wavefront results in order (thread 0 returns the block's state)
template <typename S>
__device__ __forceinline__ S block_merge(const S &w, S *waves, int nq) {
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = w;
  __syncthreads();
  S b = waves[0];
  if (threadIdx.x == 0)
    for (int k = 1; k < kWaves; ++k) b = merge(b, waves[k], nq);
  __syncthreads();
  return b;
}

}  // namespace mbar
}  // namespace me
