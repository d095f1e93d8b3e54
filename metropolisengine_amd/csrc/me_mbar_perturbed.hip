// MBAR reweighting of a ladder's samples to states that differ from the sampled ones by more than their temperature
// (me_mbar_reweight_perturbed and its engine-less twin in the public header): target p has a temperature T_p and couplings
// lambda_p[0 .. Q) over the recorded observable columns A_q, and its energy is
//     H_np = E_n + b_np,   b_np = sum over the q with lambda_pq != 0, ascending, from 0.0, of fma(lambda_pq, A_qn, b)
// -- a field conjugate to an order parameter (H = E - h real_0), a changed stiffness (H = E + lambda real_0_sq), a changed
// coefficient of one term of an energy dictionary (H = E + (c'/c - 1) energy_<term>).  The sampled states stay the temperature
// ladder, so d_n = m_n + ln s_n is k_mbar_log_denominator's (me_mbar_obs.hip), unchanged, and with
//     l_np = fma(-H_np, 1 / T_p, -d_n),   w = exp(l - M),   M = max l          (a sample is USED when its ENERGY is finite)
//     ln_z = M + ln sum w   = ln Z(T_p, lambda_p) / Z(T_0, 0), the zero of me_mbar_reweight's ln_z
//     mean_h = sum w H / sum w,   var_h = sum w (H - mean_h)^2 / sum w
//     mean_q, var_q as in me_mbar_reweight_observables,   cov_h_q = sum w (A_q - mean_q)(H - mean_h) / sum w,   neff_fraction.
// With every coupling of a target 0, b = 0.0, H = E exactly and l is k_mbar_reweight_obs's expression: mean, var, cov_h and
// neff_fraction are then that kernel's bit for bit.
//
// Nothing of size samples x all targets is stored.  Targets go through in chunks of kObsTargets = 4:
//   k_mbar_perturbed_bias    writes b of the chunk's targets, [sample][4] doubles of scratch (0.0 for a target the chunk does not
//                            have).  It reads column q only when some target of the chunk couples to it: the couplings are a
//                            kernel argument, every test of one is wave-uniform.  So a column no target couples to never enters
//                            a bias, whatever it holds;
//   k_mbar_perturbed_pass    k_mbar_reweight_obs with H where that kernel passes E: per (chunk) x (up to kObsCols = 4 columns) it
//                            reads E_n, d_n, the chunk's b and its columns and spends ONE exponential per (sample, target).  The
//                            state is me_mbar_obs_state.h's PerturbedState: a TargetState and the second moment of H, 4 x 17
//                            doubles per lane.  Columns beyond a pass's nq are carried, not bounded at run time, as there;
//   k_mbar_perturbed_finish  block t: the block partials of target t joined in k_mbar_reweight_obs_finish's fixed order; the pass
//                            of the first columns also writes ln_z = M + ln W, mean_h, var_h and neff_fraction.
// Grid policy, tiles and summation order are those of me_mbar_obs.hip: no floating-point atomics, bitwise reproducible, and --
// since b_np depends on the couplings of p alone and every (q, p) pair sees only the operations of its own state -- target p is
// bit for bit the same alone, among any others and at any position, through the engine's store and through host arrays.
// Non-finite values: a non-finite A_q in a used sample reaches b_p, and with it everything of target p, exactly when lambda_pq
// != 0 (the bias kernel stores NaN for a bias that is not finite, so the weights of p are NaN and every output of p is
// non-finite); otherwise it reaches (mean_q, M2_q, C_q) alone.
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): see profiles/mbar_perturbed.txt; no kernel uses
// scratch, the pass kernel runs 2 wavefronts per SIMD.
#include "me_mbar_obs_state.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {
namespace {

// lambda of the chunk's targets (rows beyond the chunk's last target are 0)
struct ChunkCouplings {
  double lambda[kObsTargets][ME_MAX_RECORDED_OBSERVABLES];
};

// b[i][t] of every sample i < n (addressing as in k_mbar_reweight_obs: `obs` is column 0)
__global__ void __launch_bounds__(kThreads) k_mbar_perturbed_bias(const double *__restrict__ obs, long long n, long long n_chains,
                                                                   long long record_stride, long long column_stride, int nq_all,
                                                                   ChunkCouplings c, double *__restrict__ bias) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const long long record = i / n_chains;
    const double *col = obs + record * record_stride + (i - record * n_chains);
    double b[kObsTargets];
#pragma unroll
    for (int t = 0; t < kObsTargets; ++t) b[t] = 0.0;
    for (int q = 0; q < nq_all; ++q) {            // (q and the couplings are wave-uniform)
      bool coupled = false;
#pragma unroll
      for (int t = 0; t < kObsTargets; ++t) coupled = coupled || c.lambda[t][q] != 0.0;
      if (!coupled) continue;
      const double a = col[(long long)q * column_stride];
#pragma unroll
      for (int t = 0; t < kObsTargets; ++t)
        if (c.lambda[t][q] != 0.0) b[t] = __builtin_fma(c.lambda[t][q], a, b[t]);
    }
    // a bias that is not finite is stored as NaN: an infinite one would give its sample the weight 0, or all the weight, and
    // leave some outputs of the target finite
#pragma unroll
    for (int t = 0; t < kObsTargets; ++t) bias[i * kObsTargets + t] = isfinite(b[t]) ? b[t] : NAN;
  }
}

// k_mbar_reweight_obs with H = E + b.  `d` is padded to whole tiles (NaN beyond the samples), `bias` is read for used samples only.
__global__ void __launch_bounds__(kThreads) k_mbar_perturbed_pass(const double *__restrict__ energies, const double *__restrict__ d,
                                                                   const double *__restrict__ bias, const double *__restrict__ obs,
                                                                   long long n_chains, long long record_stride, long long column_stride,
                                                                   int nq, const double *__restrict__ inv_temps, int n_targets,
                                                                   long long n_tiles, PerturbedState *partials) {
  __shared__ PerturbedState waves[kWaves];
  PerturbedState st[kObsTargets];
#pragma unroll
  for (int t = 0; t < kObsTargets; ++t) clear(st[t]);
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long base = tile * kTile + threadIdx.x;
    long long record = base / n_chains, chain = base - record * n_chains;
#pragma unroll 1
    for (int r = 0; r < kItems; ++r) {
      const long long i = base + (long long)r * kThreads;
      const double dn = d[i];                   // (padded: in bounds; NaN beyond n)
      if (dn == dn) {
        const double e = energies[i];
        const double *col = obs + record * record_stride + chain;
        double a[kObsCols];
#pragma unroll
        for (int q = 0; q < kObsCols; ++q) a[q] = q < nq ? col[(long long)q * column_stride] : 0.0;
#pragma unroll
        for (int t = 0; t < kObsTargets; ++t)
          if (t < n_targets) {
            const double h = e + bias[i * kObsTargets + t];
            add_sample(st[t], __builtin_fma(-h, inv_temps[t], -dn), h, a, nq);
          }
      }
      chain += kThreads;
      while (chain >= n_chains) {
        chain -= n_chains;
        record += 1;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kObsTargets; ++t) {
    if (t >= n_targets) break;
    const PerturbedState b = block_merge(wave_merge(st[t], nq), waves, nq);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * kObsTargets + t] = b;
  }
}

// block t: the block partials of the pass's target t joined in a fixed order.  Row t of the [n][Q] outputs starts at mean / var /
// cov + t * q_total, entry t of the per-target outputs at ln_z / mean_h / var_h / neff + t (the host has offset the pointers).
__global__ void __launch_bounds__(kThreads) k_mbar_perturbed_finish(const PerturbedState *partials, int n_blocks, int nq, int q_total,
                                                                     double n_used, int write_target, double *mean, double *var,
                                                                     double *cov, double *ln_z, double *mean_h, double *var_h,
                                                                     double *neff) {
  __shared__ PerturbedState waves[kWaves];
  const int t = blockIdx.x;
  PerturbedState s;
  clear(s);
  for (int b = threadIdx.x; b < n_blocks; b += kThreads) s = merge(s, partials[(size_t)b * kObsTargets + t], nq);
  const PerturbedState b = block_merge(wave_merge(s, nq), waves, nq);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int q = 0; q < kObsCols; ++q)
    if (q < nq) {
      mean[(size_t)t * q_total + q] = b.mean[q];
      var[(size_t)t * q_total + q] = b.M2[q] / b.W;
      cov[(size_t)t * q_total + q] = b.C[q] / b.W;
    }
  if (write_target) {
    ln_z[t] = b.M + log(b.W);
    mean_h[t] = b.mean_e;
    var_h[t] = b.M2_e / b.W;
    neff[t] = (b.W * b.W) / (n_used * b.Q2);
  }
}

// what an entry point writes: host arrays, each may be nullptr
struct PerturbedOutputs {
  double *ln_z, *mean_h, *var_h, *mean, *var, *cov_h, *neff;
};

// Prepares `p`, runs the chunks and copies back: p.w.out = [mean | var | cov_h][target][column], then [ln_z | mean_h | var_h |
// neff_fraction][target].  Waits for the stream.  With an empty rung (p.empty_rung) nothing else is computed.
hipError_t reweight_perturbed(Problem &p, const Source &src, const double *f, const double *temps, const double *couplings, int n_temps,
                              const PerturbedOutputs &o) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const ObsColumns &oc = src.columns;
  const MbarSamples &sm = p.sm;
  const int n_blocks = blocks_of(sm.n_samples), nq_all = oc.n_columns;
  const long long n_tiles = tiles_of(sm.n_samples);
  const size_t cells = (size_t)n_temps * nq_all, per_target = (size_t)n_temps;
  std::vector<double> inv;
  ObsScratch scratch;
  DeviceBuffer bias;
  ME_MBAR_HIP(upload_targets(p, temps, n_temps, 3 * cells + 4 * per_target, inv));
  ME_MBAR_HIP(log_denominator_enqueue(p, sm, scratch.d));
  ME_MBAR_HIP(bias.resize((size_t)n_tiles * kTile * kObsTargets * sizeof(double)));
  ME_MBAR_HIP(scratch.partials.resize((size_t)n_blocks * kObsTargets * sizeof(PerturbedState)));
  double *o_mean = w.out.get<double>(), *o_var = o_mean + cells, *o_cov = o_var + cells, *o_ln_z = o_cov + cells;
  double *o_mean_h = o_ln_z + per_target, *o_var_h = o_mean_h + per_target, *o_neff = o_var_h + per_target;
  const double *inv_temps = w.inv_temps.get<const double>();
  for (int t0 = 0; t0 < n_temps; t0 += kObsTargets) {
    const int nt = std::min(kObsTargets, n_temps - t0);
    ChunkCouplings c = {};
    for (int t = 0; t < nt; ++t)
      for (int q = 0; q < nq_all; ++q) c.lambda[t][q] = couplings[(size_t)(t0 + t) * nq_all + q];
    hipLaunchKernelGGL(k_mbar_perturbed_bias, dim3(n_blocks), dim3(kThreads), 0, p.stream, oc.data, sm.n_samples, oc.n_chains,
                       oc.record_stride, oc.column_stride, nq_all, c, bias.get<double>());
    for (int q0 = 0; q0 < nq_all; q0 += kObsCols) {
      const int nq = std::min(kObsCols, nq_all - q0);
      const size_t cell = (size_t)t0 * nq_all + q0;
      hipLaunchKernelGGL(k_mbar_perturbed_pass, dim3(n_blocks), dim3(kThreads), 0, p.stream, sm.energies, scratch.d.get<const double>(),
                         bias.get<const double>(), oc.data + (size_t)q0 * oc.column_stride, oc.n_chains, oc.record_stride,
                         oc.column_stride, nq, inv_temps + t0, nt, n_tiles, scratch.partials.get<PerturbedState>());
      hipLaunchKernelGGL(k_mbar_perturbed_finish, dim3(nt), dim3(kThreads), 0, p.stream, scratch.partials.get<const PerturbedState>(),
                         n_blocks, nq, nq_all, p.n_used, q0 == 0 ? 1 : 0, o_mean + cell, o_var + cell, o_cov + cell, o_ln_z + t0,
                         o_mean_h + t0, o_var_h + t0, o_neff + t0);
    }
  }
  ME_MBAR_HIP(hipGetLastError());
  std::vector<double> out(3 * cells + 4 * per_target);
  ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipStreamSynchronize(p.stream));    // (also: `inv`, `scratch` and `bias` leave scope)
  const double *at = out.data();
  for (double *dst : {o.mean, o.var, o.cov_h}) {
    if (dst) std::copy(at, at + cells, dst);
    at += cells;
  }
  for (double *dst : {o.ln_z, o.mean_h, o.var_h, o.neff}) {
    if (dst) std::copy(at, at + per_target, dst);
    at += per_target;
  }
  return hipSuccess;
}

// the two forms of me_mbar_reweight_perturbed behind their Source (which has its columns)
int reweight_perturbed_common(const Source &src, const double *f, const double *temps, const double *couplings, int n,
                              const PerturbedOutputs &o) {
  const int rc = check_f_and_targets(src.e, f, src.n_rungs, temps, n, 1);
  if (rc) return rc;
  if (!couplings) return fail(src.e, ME_ERR_INVALID, "couplings missing");
  for (size_t j = 0; j < (size_t)n * src.columns.n_columns; ++j)
    if (!std::isfinite(couplings[j])) return fail(src.e, ME_ERR_INVALID, "couplings must be finite");
  Problem p;
  return mbar_check_common(src.e, p, reweight_perturbed(p, src, f, temps, couplings, n, o));
}

}  // namespace
}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_mbar_reweight_perturbed(me_engine *e, const double *f, const double *temps, const double *couplings, int32_t n, double *ln_z,
                               double *mean_h, double *var_h, double *mean, double *var, double *cov_h, double *neff_fraction) {
  Source src;
  const int rc = src.from_engine(e);
  if (rc) return rc;
  if (src.columns.n_columns == 0)
    return fail(e, ME_ERR_STATE, "no recorded observables: me_observable_samples_enable, then me_energy_samples_record");
  return reweight_perturbed_common(src, f, temps, couplings, n, PerturbedOutputs{ln_z, mean_h, var_h, mean, var, cov_h, neff_fraction});
}

int me_mbar_reweight_perturbed_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                       const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps,
                                       const double *couplings, int32_t n, const double *observables, int32_t n_observables,
                                       double *ln_z, double *mean_h, double *var_h, double *mean, double *var, double *cov_h,
                                       double *neff_fraction) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs, observables, n_observables);
  return rc ? rc
            : src.finish(reweight_perturbed_common(src, f, temps, couplings, n,
                                                   PerturbedOutputs{ln_z, mean_h, var_h, mean, var, cov_h, neff_fraction}));
}

}  // extern "C"
