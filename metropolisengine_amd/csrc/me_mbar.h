// What the MBAR units share (me_mbar.hip: samples, solve, reweighting; me_mbar_cov.hip: the Gram matrix of the weight
// matrix for the asymptotic covariance; me_mbar_obs.hip: recorded observables and their reweighting): the tile policy, the
// device table of a ladder, the per-sample sums and the host helpers that me_mbar.hip defines.  Private to the host side,
// like me_engine.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "me_device.h"
#include "me_engine.h"
#include "me_math64.h"

#pragma GCC visibility push(hidden)

namespace me {
namespace mbar {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;                       // samples per thread and tile
constexpr int kTile = kThreads * kItems;        // 2048 samples
constexpr int kMaxBlocks = 2048;                // about 8 blocks per CU; the grid depends on the sample count only
constexpr int kTargets = 8;                     // reweighting temperatures per pass over the samples
constexpr int kK = 64;                          // most rungs of one problem

// device-side state of a solve: doubles [beta | c = ln N + f | ln N | N | f], then the control words
constexpr int kBeta = 0, kC = kK, kLnN = 2 * kK, kN = 3 * kK, kF = 4 * kK, kTableDoubles = 5 * kK;
struct MbarControl {
  double residual;
  int iterations, done;
};

// m_n and s_n of one sample over all rungs (table indices are wave-uniform)
__device__ __forceinline__ void sample_max_sum(const double *__restrict__ table, int n_rungs, double e, double &m, double &s) {
  m = -INFINITY;
  for (int j = 0; j < n_rungs; ++j) m = fmax(m, __builtin_fma(-table[kBeta + j], e, table[kC + j]));
  s = 0.0;
  for (int j = 0; j < n_rungs; ++j) s = s + math64::exp_nonpos(__builtin_fma(-table[kBeta + j], e, table[kC + j]) - m);
}

// The samples of one MBAR problem, all in device memory.  rungs != nullptr: the rung of sample i is rungs[i]; otherwise
// sample i is slot i % n_chains of an engine and its rung is (i % n_chains) / rung_chains.
struct MbarSamples {
  const double *energies;
  const int *rungs;
  long long n_samples, n_chains, rung_chains;
};

// device scratch of one solve / reweighting
struct Work {
  DeviceBuffer table, partials, inv_temps, out;   // double
  DeviceBuffer moments;                           // Moments
  DeviceBuffer counts;                            // unsigned long long
  DeviceBuffer control;                           // MbarControl
};

#define ME_MBAR_HIP(call)                 \
  do {                                    \
    hipError_t err__ = (call);            \
    if (err__ != hipSuccess) return err__; \
  } while (0)

inline long long tiles_of(long long n) { return (n + kTile - 1) / kTile; }
inline int blocks_of(long long n) { return (int)std::min<long long>(tiles_of(n), kMaxBlocks); }

// ---- defined in me_mbar.hip ---------------------------------------------------------------------------------------------
// N_k into host `counts` (kK entries); *empty_rung = the first rung without a finite sample or -1.  Waits for the stream.
hipError_t count_used(const MbarSamples &sm, int n_rungs, Work &w, std::vector<unsigned long long> &counts, int *empty_rung,
                      hipStream_t stream);
// the device table (w.table) for free energies f (nullptr: zeros)
hipError_t upload_table(Work &w, const double *ladder_temps, int n_rungs, const std::vector<unsigned long long> &counts,
                        const double *f, hipStream_t stream);
// Enqueues the reweighting of the samples to temps[0 .. n_temps): afterwards w.inv_temps[t] = 1 / T_t and w.out[4 t ..] =
// (ln_z, mean_e, var_e, neff_fraction) of T_t on the device.  Needs w.table; does not wait: `inv`, the host copy of the
// 1 / T_t that is on its way to the device, is the caller's to keep until the stream has been waited for.
hipError_t reweight_enqueue(const MbarSamples &sm, int n_rungs, Work &w, const double *temps, int n_temps, double n_used,
                            std::vector<double> &inv, hipStream_t stream);
// hipError_t / an empty rung as the ME_* code of an entry point
int mbar_check_common(me_engine *e, int n_rungs, int empty_rung, hipError_t err);
int mbar_check_temps(me_engine *e, const double *temps, int n, const char *what);
// the engine's store as an MBAR problem (ME_ERR_STATE when there is nothing to solve)
int engine_samples(me_engine *e, MbarSamples &sm);
// host samples of the engine-less forms on the device (`energies_dev`, `rungs_dev`: theirs for the length of the call)
int upload_samples(int device_id, const double *energies, const int32_t *rungs, int64_t n_samples, const double *ladder_temps,
                   int n_rungs, DeviceBuffer &energies_dev, DeviceBuffer &rungs_dev, MbarSamples &sm);

// ---- defined in me_mbar_obs.hip -----------------------------------------------------------------------------------------
// me_energy_samples_record's second kernel: row `row` of the engine's observable store (which exists) on the engine's stream
hipError_t observable_record_enqueue(me_engine *e, long long row);

}  // namespace mbar
}  // namespace me

#pragma GCC visibility pop
