// Recorded per-chain observables of a ladder engine and their MBAR reweighting to any temperature
// (me_observable_samples_*, me_mbar_reweight_observables and its engine-less twin in the public header).
//
// The store.  Coupled to the energy store of me_mbar.hip (me_engine::Samples): record r of both is the same moment, there is
// ONE record count.  A float64 device field [capacity][Q][n_chains], Q <= 16 selected entries of the catalogue of a chain's
// recordable quantities (D = nr + 2 nc, NOBS = 2 nr + nc):
//     [0, D)                        the state rows in ME_FIELD_PARAMS component order (x_r, Re z_c, Im z_c), widened to float64
//     [D, D + NOBS)                 |x_r|, |z_c|, x_r^2 in ME_FIELD_OBS_MEAN order, formed IN FLOAT64 FROM THE WIDENED COMPONENTS:
//                                   fabs(x), sqrt(fma(re, re, im * im)) with the correctly rounded square root, x * x
//     [D + NOBS, D + NOBS + T)      the ledger rows (energy terms, row order), widened to float64
// The derived quantities are NOT the N_::sqrt_ / N_::abs_ of k_measure, which work in the device dtype: they are formed after
// widening so that the host can restate a record exactly whatever the device dtype (float32 widens exactly).
// k_observable_record: one lane per chain, Q coalesced float64 stores per lane; the selection is a kernel argument read with
// wave-uniform indices (scalar registers), the state is read through the layout of the engine's kernel set (a launch flag,
// as in k_trace: tile-major for register-resident sets with D >= 16, component-major otherwise), the ledger is component-major.
// No kernel is instantiated per Q or per D.
//
// Reweighting.  With the weights of me_mbar_reweight (me_mbar.hip: d_n = m_n + ln s_n, l_n = -E_n / T - d_n, w_n = exp(l_n -
// M); a sample is USED when its ENERGY is finite), for observable column A_q:
//     mean_q = sum w A_q / sum w,  var_q = sum w (A_q - mean_q)^2 / sum w,  cov_energy_q = sum w (A_q - mean_q)(E - mean_E) / sum w
// and neff_fraction = (sum w)^2 / (N sum w^2); d<A_q>/dT = cov_energy_q / T^2.  The running state of some samples is, per
// target, (M, W = sum w, Q2 = sum w^2, mean_E) and, per target and observable, (mean_q, M2_q, C_q), all relative to the running
// maximum M.  One more sample (weight w, the old sums rescaled by `scale`; one of the two is 1, the other exp of a
// non-positive number):
//     W <- W scale + w;  mean <- mean + (A - mean) w / W;  M2 <- M2 scale + w (A - mean_old)(A - mean_new);
//     C <- C scale + w (A - mean_A_old)(E - mean_E_new)
// and two states a (earlier), b merge by  C = C_a s_a + C_b s_b + (mean_A,b - mean_A,a)(mean_E,b - mean_E,a) W_a W_b / W, M2
// likewise: the weighted form of Chan's update, no difference of large sums anywhere.  A non-finite A_q in a used sample
// reaches (mean_q, M2_q, C_q) only: the other observables' results are bitwise what they are without it.
//
// The split.  Sixteen observables times eight targets of running state (16 x 8 x 3 + 8 x 4 doubles = 832 registers) do not fit
// a lane, so:
//   k_mbar_log_denominator   writes d_n once into a scratch buffer of 8 bytes per sample (K exponentials, exp_nonpos, and one
//                            log per sample), NaN for unused samples and for the padding behind the store's records;
//   k_mbar_reweight_obs      one pass per (up to kObsTargets = 4 targets) x (up to kObsCols = 4 observables): reads E_n, d_n
//                            and its observable columns -- (1 + q) 8 + 8 bytes per sample -- and spends ONE exponential per
//                            (sample, target).  4 x 4 + 4 x 4 x 3 = 64 doubles of running state per lane;
//   k_mbar_reweight_obs_finish   block t: the block partials of target t joined in a fixed order, written straight into the
//                            [n][Q] device outputs.
// Grid policy of k_mbar_weights: tiles of 2048 samples walked grid-stride, at most 2048 blocks, the grid depends on the sample
// count only.  Summation order, fixed (no floating-point atomics, bitwise reproducible), that of k_mbar_reweight: a lane's
// state runs over its samples of ALL the block's tiles, tile by tile -> butterfly in the wavefront, the lower lane's state
// the first operand -> the block's wavefronts in order -> partials[block][target] -> the finish kernel, in which lane l
// first joins blocks l, l + 256, ... and the lanes are then joined as in a block: a fixed order, not block by block.
// Every (q, t) pair sees exactly the operations of its own state and of its target's (M, W, Q2, mean_E), written without contraction (`fp
// contract(off)`, fused multiply-adds spelled out) so that the position of a pair inside a pass cannot change how the
// compiler rounds it: observable q at target t is bit for bit the same alone or among 16 x 9.  For the same reason the
// engine form and the engine-less form agree bit for bit (the store's [record][Q][chain] and the host's [Q][sample] are
// addressed through strides; the sample order is the same).  W and Q2 are me_mbar_reweight's up to that difference in
// contraction: neff_fraction agrees with it to rounding, not bit for bit.
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_mbar_reweight_obs 194 VGPRs, 2 wavefronts per SIMD;
// k_mbar_reweight_obs_finish 94, k_mbar_log_denominator 54, k_observable_record 18; no kernel uses scratch.  (Columns beyond a
// pass's nq are carried along unchanged, never zeroed behind a runtime bound: that indexing put the state into scratch.)
// The state, add_sample, the merges and the butterfly live in me_mbar_obs_state.h, which me_mbar_perturbed.hip shares.
#include "me_mbar_obs_state.h"

#pragma clang fp contract(off)

namespace me {
namespace mbar {
namespace {

struct ObsSelection {
  int q[ME_MAX_RECORDED_OBSERVABLES];
};

// ---- the store ----------------------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kThreads) k_observable_record(const R *__restrict__ x, const R *__restrict__ energy, long long n,
                                                                 int nr, int nc, int n_terms, int tiled, ObsSelection sel,
                                                                 int n_sel, double *dst) {
  const long long c = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (c >= n) return;
  const int d = nr + 2 * nc, nobs = 2 * nr + nc;
  // element index of state row k of this chain (k_trace's two layouts)
  const long long x0 = tiled ? (c >> 6) * (long long)d * 64 + (c & 63) : c;
  const long long xs = tiled ? 64 : n;
  for (int j = 0; j < n_sel; ++j) {
    const int q = sel.q[j];                     // wave-uniform
    double v;
    if (q < d) {
      v = (double)x[x0 + (long long)q * xs];
    } else if (q < d + nobs) {
      const int o = q - d;
      if (o < nr) {
        v = fabs((double)x[x0 + (long long)o * xs]);
      } else if (o < nr + nc) {
        const double re = (double)x[x0 + (long long)o * xs], im = (double)x[x0 + (long long)(o + nc) * xs];
        v = __builtin_sqrt(__builtin_fma(re, re, im * im));
      } else {
        const double xr = (double)x[x0 + (long long)(o - nr - nc) * xs];
        v = xr * xr;
      }
    } else {
      v = (double)energy[(long long)(q - d - nobs) * n + c];
    }
    dst[(long long)j * n + c] = v;
  }
}

// ---- reweighting --------------------------------------------------------------------------------------------------------
// d_n = m_n + ln s_n of every sample of the padded range [0, n_padded); NaN when the energy is not finite or n <= i
__global__ void __launch_bounds__(kThreads) k_mbar_log_denominator(const double *__restrict__ energies, long long n, long long n_padded,
                                                                    int n_rungs, const double *__restrict__ table, double *d) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_padded; i += (long long)gridDim.x * kThreads) {
    const double e = i < n ? energies[i] : NAN;
    double v = NAN;
    if (isfinite(e)) {
      double m, s;
      sample_max_sum(table, n_rungs, e, m, s);
      v = m + log(s);
    }
    d[i] = v;
  }
}

// Sample i = record * n_chains + chain; column q of it sits at obs[record * record_stride + q * column_stride + chain] (the
// engine's store: n_chains, Q n_chains, n_chains; host columns [Q][n]: n, 0, n).  `d` is padded to whole tiles.
// Registers: 194 VGPRs, no AGPRs, no scratch, 2 wavefronts per SIMD (the running state alone is 128).
__global__ void __launch_bounds__(kThreads) k_mbar_reweight_obs(const double *__restrict__ energies, const double *__restrict__ d,
                                                                 const double *__restrict__ obs, long long n, long long n_chains,
                                                                 long long record_stride, long long column_stride, int nq,
                                                                 const double *__restrict__ inv_temps, int n_targets,
                                                                 long long n_tiles, TargetState *partials) {
  __shared__ TargetState waves[kWaves];
  TargetState st[kObsTargets];
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
          if (t < n_targets) add_sample(st[t], __builtin_fma(-e, inv_temps[t], -dn), e, a, nq);
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
    const TargetState b = block_merge(wave_merge(st[t], nq), waves, nq);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * kObsTargets + t] = b;
  }
}

// block t: the block partials of the pass's target t joined in a fixed order.  Row t of the [n][Q] outputs starts at
// mean/var/cov + t * q_total (the host has offset the pointers to the pass's first target and column).
__global__ void __launch_bounds__(kThreads) k_mbar_reweight_obs_finish(const TargetState *partials, int n_blocks, int nq, int q_total,
                                                                        double n_used, int write_neff, double *mean, double *var,
                                                                        double *cov, double *neff) {
  __shared__ TargetState waves[kWaves];
  const int t = blockIdx.x;
  TargetState s;
  clear(s);
  for (int b = threadIdx.x; b < n_blocks; b += kThreads) s = merge(s, partials[(size_t)b * kObsTargets + t], nq);
  const TargetState b = block_merge(wave_merge(s, nq), waves, nq);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int q = 0; q < kObsCols; ++q)
    if (q < nq) {
      mean[(size_t)t * q_total + q] = b.mean[q];
      var[(size_t)t * q_total + q] = b.M2[q] / b.W;
      cov[(size_t)t * q_total + q] = b.C[q] / b.W;
    }
  if (write_neff) neff[t] = (b.W * b.W) / (n_used * b.Q2);
}

hipError_t reweight_observables(Problem &p, const Source &src, const double *f, const double *temps, int n_temps, double *mean,
                                double *var, double *cov, double *neff) {
  ME_MBAR_HIP(prepare(p, src, f));
  if (p.empty_rung >= 0) return hipSuccess;
  Work &w = p.w;
  const size_t cells = (size_t)n_temps * src.columns.n_columns;
  std::vector<double> inv;
  ObsScratch scratch;
  ME_MBAR_HIP(upload_targets(p, temps, n_temps, 3 * cells + (size_t)n_temps, inv));
  ME_MBAR_HIP(reweight_observables_enqueue(p, p.sm, src.columns, w.inv_temps.get<const double>(), n_temps, scratch, w.out.get<double>()));
  std::vector<double> out(3 * cells + (size_t)n_temps);
  ME_MBAR_HIP(hipMemcpyAsync(out.data(), w.out.get(), out.size() * sizeof(double), hipMemcpyDeviceToHost, p.stream));
  ME_MBAR_HIP(hipStreamSynchronize(p.stream));    // (also: `inv` and `scratch` leave scope)
  if (mean) std::copy(out.begin(), out.begin() + cells, mean);
  if (var) std::copy(out.begin() + cells, out.begin() + 2 * cells, var);
  if (cov) std::copy(out.begin() + 2 * cells, out.begin() + 3 * cells, cov);
  if (neff) std::copy(out.begin() + 3 * cells, out.end(), neff);
  return hipSuccess;
}

// the two forms of me_mbar_reweight_observables behind their Source
int reweight_observables_common(const Source &src, const double *f, const double *temps, int n, double *mean, double *var, double *cov,
                                double *neff) {
  const int rc = check_f_and_targets(src.e, f, src.n_rungs, temps, n, 1);
  if (rc) return rc;
  Problem p;
  return mbar_check_common(src.e, p, reweight_observables(p, src, f, temps, n, mean, var, cov, neff));
}

int catalogue_size(const me_engine *e) { return e->d + e->nobs + e->n_terms; }

}  // namespace

hipError_t log_denominator_enqueue(Problem &p, const MbarSamples &sm, DeviceBuffer &d) {
  const long long n_padded = tiles_of(sm.n_samples) * kTile;
  ME_MBAR_HIP(d.resize((size_t)n_padded * sizeof(double)));
  hipLaunchKernelGGL(k_mbar_log_denominator, dim3(blocks_of(sm.n_samples)), dim3(kThreads), 0, p.stream, sm.energies, sm.n_samples,
                     n_padded, p.n_rungs, p.w.table.get<const double>(), d.get<double>());
  return hipGetLastError();
}

hipError_t reweight_observables_enqueue(Problem &p, const MbarSamples &sm, const ObsColumns &oc, const double *inv_temps, int n_temps,
                                        ObsScratch &scratch, double *out) {
  hipStream_t stream = p.stream;
  const int n_blocks = blocks_of(sm.n_samples), nq_all = oc.n_columns;
  const long long n_tiles = tiles_of(sm.n_samples);
  const size_t cells = (size_t)n_temps * nq_all;
  ME_MBAR_HIP(log_denominator_enqueue(p, sm, scratch.d));
  ME_MBAR_HIP(scratch.partials.resize((size_t)n_blocks * kObsTargets * sizeof(TargetState)));
  double *o_mean = out, *o_var = o_mean + cells, *o_cov = o_var + cells, *o_neff = o_cov + cells;
  for (int t0 = 0; t0 < n_temps; t0 += kObsTargets) {
    const int nt = std::min(kObsTargets, n_temps - t0);
    for (int q0 = 0; q0 < nq_all; q0 += kObsCols) {
      const int nq = std::min(kObsCols, nq_all - q0);
      const size_t cell = (size_t)t0 * nq_all + q0;
      hipLaunchKernelGGL(k_mbar_reweight_obs, dim3(n_blocks), dim3(kThreads), 0, stream, sm.energies, scratch.d.get<const double>(),
                         oc.data + (size_t)q0 * oc.column_stride, sm.n_samples, oc.n_chains, oc.record_stride, oc.column_stride, nq,
                         inv_temps + t0, nt, n_tiles, scratch.partials.get<TargetState>());
      hipLaunchKernelGGL(k_mbar_reweight_obs_finish, dim3(nt), dim3(kThreads), 0, stream, scratch.partials.get<const TargetState>(),
                         n_blocks, nq, nq_all, p.n_used, q0 == 0 ? 1 : 0, o_mean + cell, o_var + cell, o_cov + cell, o_neff + t0);
    }
  }
  return hipGetLastError();
}

// me_energy_samples_record's second kernel: row `row` of the observable store (the caller has checked that it exists)
hipError_t observable_record_enqueue(me_engine *e, long long row) {
  me_engine::Samples &s = e->samples;
  ObsSelection sel;
  for (int j = 0; j < ME_MAX_RECORDED_OBSERVABLES; ++j) sel.q[j] = j < s.n_obs ? s.obs_index[j] : 0;
  double *dst = s.obs.get<double>() + (size_t)row * (size_t)s.n_obs * (size_t)e->n;
  const dim3 grid((unsigned)((e->n + kThreads - 1) / kThreads));
  if (e->dtype == ME_F32)
    hipLaunchKernelGGL(k_observable_record<float>, grid, dim3(kThreads), 0, e->stream, e->x.get<const float>(), e->energy.get<const float>(),
                       e->n, e->nr, e->nc, e->n_terms, e->x_tiled ? 1 : 0, sel, s.n_obs, dst);
  else
    hipLaunchKernelGGL(k_observable_record<double>, grid, dim3(kThreads), 0, e->stream, e->x.get<const double>(),
                       e->energy.get<const double>(), e->n, e->nr, e->nc, e->n_terms, e->x_tiled ? 1 : 0, sel, s.n_obs, dst);
  return hipGetLastError();
}

}  // namespace mbar
}  // namespace me

using namespace me;
using namespace me::mbar;

extern "C" {

int me_observable_samples_enable(me_engine *e, const int32_t *indices, int32_t n_observables) {
  if (!e) return ME_ERR_INVALID;
  const int rc = refuse_stale_total(e, "observable samples are");
  if (rc != ME_OK) return rc;
  if (n_observables < 0 || n_observables > ME_MAX_RECORDED_OBSERVABLES)
    return fail(e, ME_ERR_INVALID, "n_observables must lie in [0, " + std::to_string(ME_MAX_RECORDED_OBSERVABLES) + "]");
  me_engine::Samples &s = e->samples;
  ME_HIP(e, hipSetDevice(e->device));
  if (n_observables == 0) {
    ME_HIP(e, hipStreamSynchronize(e->stream));     // a record in flight writes the field
    s.obs.reset();
    s.n_obs = 0;
    return ME_OK;
  }
  if (!s.data) return fail(e, ME_ERR_STATE, "observable samples need the energy store: call me_energy_samples_enable first");
  if (!indices) return fail(e, ME_ERR_INVALID, "indices missing");
  for (int j = 0; j < n_observables; ++j)
    if (indices[j] < 0 || indices[j] >= catalogue_size(e))
      return fail(e, ME_ERR_INVALID, "observable index " + std::to_string(indices[j]) + " outside the catalogue of " +
                                         std::to_string(catalogue_size(e)) + " quantities");
  ME_HIP(e, hipStreamSynchronize(e->stream));
  s.obs.reset();
  s.n_obs = 0;
  s.rows = 0;
  const size_t bytes = (size_t)s.capacity * (size_t)n_observables * (size_t)e->n * sizeof(double);
  ME_HIP(e, s.obs.resize(bytes));
  if (bytes) {
    ME_HIP(e, hipMemsetAsync(s.obs.get(), 0, bytes, e->stream));
    ME_HIP(e, hipStreamSynchronize(e->stream));
  }
  s.n_obs = n_observables;
  for (int j = 0; j < n_observables; ++j) s.obs_index[j] = indices[j];
  return ME_OK;
}

int me_observable_samples_info(me_engine *e, int32_t *n_observables, int32_t *indices) {
  if (!e) return ME_ERR_INVALID;
  if (n_observables) *n_observables = e->samples.n_obs;
  if (indices)
    for (int j = 0; j < e->samples.n_obs; ++j) indices[j] = e->samples.obs_index[j];
  return ME_OK;
}

int me_observable_samples_get(me_engine *e, int64_t record_begin, int64_t n_records, double *dst) {
  if (!e || (!dst && n_records > 0)) return ME_ERR_INVALID;
  const me_engine::Samples &s = e->samples;
  if (s.n_obs == 0) return fail(e, ME_ERR_STATE, "observable samples are not enabled: call me_observable_samples_enable first");
  if (record_begin < 0 || n_records < 0 || record_begin + n_records > s.rows)
    return fail(e, ME_ERR_INVALID, "record range outside the recorded samples");
  if (n_records == 0) return ME_OK;
  const size_t row = (size_t)s.n_obs * (size_t)e->n;
  ME_HIP(e, hipSetDevice(e->device));
  ME_HIP(e, hipMemcpyAsync(dst, s.obs.get<double>() + (size_t)record_begin * row, (size_t)n_records * row * sizeof(double),
                           hipMemcpyDeviceToHost, e->stream));
  ME_HIP(e, hipStreamSynchronize(e->stream));
  return ME_OK;
}

int me_observable_samples_set(me_engine *e, int64_t n_records, const double *src) {
  if (!e || (!src && n_records > 0)) return ME_ERR_INVALID;
  const me_engine::Samples &s = e->samples;
  if (s.n_obs == 0) return fail(e, ME_ERR_STATE, "observable samples are not enabled: call me_observable_samples_enable first");
  if (n_records != s.rows)
    return fail(e, ME_ERR_INVALID, "n_records must equal the energy record count (" + std::to_string(s.rows) +
                                       "): call me_energy_samples_set first");
  if (n_records == 0) return ME_OK;
  ME_HIP(e, hipSetDevice(e->device));
  ME_HIP(e, hipMemcpyAsync(s.obs.get(), src, (size_t)n_records * (size_t)s.n_obs * (size_t)e->n * sizeof(double), hipMemcpyHostToDevice,
                           e->stream));
  ME_HIP(e, hipStreamSynchronize(e->stream));
  return ME_OK;
}

int me_mbar_reweight_observables(me_engine *e, const double *f, const double *temps, int32_t n, double *mean, double *var,
                                 double *cov_energy, double *neff_fraction) {
  Source src;
  const int rc = src.from_engine(e);
  if (rc) return rc;
  if (src.columns.n_columns == 0)
    return fail(e, ME_ERR_STATE, "no recorded observables: me_observable_samples_enable, then me_energy_samples_record");
  return reweight_observables_common(src, f, temps, n, mean, var, cov_energy, neff_fraction);
}

int me_mbar_reweight_observables_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                         const double *observables, int32_t n_observables, const double *ladder_temps, int32_t n_rungs,
                                         const double *f, const double *temps, int32_t n, double *mean, double *var,
                                         double *cov_energy, double *neff_fraction) {
  Source src;
  const int rc = src.from_host(device_id, energies, rungs, n_samples, ladder_temps, n_rungs, observables, n_observables);
  return rc ? rc : src.finish(reweight_observables_common(src, f, temps, n, mean, var, cov_energy, neff_fraction));
}

}  // extern "C"
