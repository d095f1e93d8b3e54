// What the MBAR units share (me_mbar.hip: samples, solve, reweighting; me_mbar_newton.hip: the Newton solve; me_mbar_cov.hip:
// the Gram matrix of the weight matrix for the asymptotic covariance; me_mbar_obs.hip: recorded observables and their
// reweighting; me_mbar_perturbed.hip: their reweighting to perturbed energies, on the pass state of me_mbar_obs_state.h;
// me_mbar_hist.hip: reweighted histograms along an observable; me_mbar_hist_cov.hip: the slot Gram sums behind
// their error bars; me_mbar_hist2d.hip: joint histograms along two; me_mbar_hist2d_cov.hip: the cell Gram sums behind theirs --
// four pairings of the policies of one pass kernel, me_mbar_slots.h, behind two host drivers, histogram_slots for the masses and
// slot_gram_passes for the Gram sums): the tile policy,
// the device table of a ladder, the per-sample sums, and the host scaffolding of an entry point, which me_mbar.hip defines:
// where the samples come from (Source), the prepared problem (Problem, prepare) and the argument checks.  Private to the host
// side, like me_engine.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

#include "me_device.h"
#include "me_engine.h"
#include "me_math64.h"
#include "me_wave.h"

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

// Observable columns that go with the samples (device memory): column q of sample i = record * n_chains + chain sits at
// data[record * record_stride + q * column_stride + chain] (an engine's store: strides Q n_chains, n_chains; host columns
// [Q][n]: n_chains = n, strides 0, n)
struct ObsColumns {
  const double *data;
  int n_columns;
  long long n_chains, record_stride, column_stride;
};
// where column 0 of sample i sits in such columns
__device__ __forceinline__ long long obs_offset(const ObsColumns &oc, long long i) {
  const long long record = i / oc.n_chains;
  return record * oc.record_stride + (i - record * oc.n_chains);
}

// Device scratch of one problem.  Every operation: `counts` (unsigned long long [kK]) and `table` (double [kTableDoubles]),
// both from prepare.  Operations with target temperatures: `inv_temps` (double, 1 / T_t) and `out` (double), both sized by
// upload_targets; `out` holds 4 doubles per target behind reweight_enqueue (me_mbar.hip, me_mbar_cov.hip) and [mean | var |
// cov][target][column], then neff[target], in me_mbar_obs.hip.  reweight_enqueue alone: `moments` (Moments [block][kTargets]).
// The solve alone: `partials` (double [block][rung]) and `control` (MbarControl); the Newton solve (me_mbar_newton.hip) keeps its
// own partials [block][K + K (K + 1) / 2] and control words, which begin with an MbarControl, in the same two.
struct Work {
  DeviceBuffer table, partials, inv_temps, out, moments, counts, control;
};

#define ME_MBAR_HIP(call)                 \
  do {                                    \
    hipError_t err__ = (call);            \
    if (err__ != hipSuccess) return err__; \
  } while (0)

inline long long tiles_of(long long n) { return (n + kTile - 1) / kTile; }
inline int blocks_of(long long n) { return (int)std::min<long long>(tiles_of(n), kMaxBlocks); }

// ---- defined in me_mbar.hip ---------------------------------------------------------------------------------------------
// Where the samples of an entry point come from: the store of an engine (on its stream), or host arrays, which from_host puts
// on the device for the length of the call (e == nullptr, the null stream; messages go to the calling thread).
struct Source {
  me_engine *e = nullptr;
  MbarSamples sm{};
  const double *ladder_temps = nullptr;
  int n_rungs = 0;
  hipStream_t stream = nullptr;
  ObsColumns columns{};                           // n_columns = 0: none
  DeviceBuffer energies_dev, rungs_dev, columns_dev;      // the host form's samples and columns
  // the engine's stores and ladder (ME_ERR_STATE when there is nothing to solve); selects its device
  int from_engine(me_engine *engine);
  // checks the host arrays and uploads them to device `device_id`; the second form also takes columns [n_columns][n_samples]
  int from_host(int device_id, const double *energies, const int32_t *rungs, int64_t n_samples, const double *temps, int n);
  int from_host(int device_id, const double *energies, const int32_t *rungs, int64_t n_samples, const double *temps, int n,
                const double *observables, int n_columns);
  // the end of a host-form entry point: waits for the device before the buffers go, and passes `rc` on
  int finish(int rc) const;
};

// One prepared problem: the samples with their N_k counted and the ladder's table on the device.
struct Problem {
  MbarSamples sm{};
  int n_rungs = 0;
  hipStream_t stream = nullptr;
  Work w;
  unsigned long long counts[kK] = {};             // N_k
  int empty_rung = -1;                            // the first rung without a finite sample
  double n_used = 0.0;                            // the sum of the N_k, added as double ...
  long long n_used_ll = 0;                        // ... and as integers
};
// hipErrorInvalidValue unless 1 <= n_rungs <= kK and there is a sample.  Then the N_k (waits for the stream) and, unless a rung
// is empty (p.empty_rung >= 0 with hipSuccess: nothing else is to be computed), n_used and the table for the free energies f
// (nullptr: zeros; waits again).
hipError_t prepare(Problem &p, const Source &src, const double *f);
// 1 / T_t of temps[0 .. n) into `inv` and on its way to p.w.inv_temps; p.w.out sized to out_doubles.  Does not wait: `inv` is the
// caller's to keep until the stream has been waited for.
hipError_t upload_targets(Problem &p, const double *temps, int n, size_t out_doubles, std::vector<double> &inv);
// Enqueues the reweighting of `sm` (the problem's samples, or the used ones of them packed) to temps[0 .. n_temps): afterwards
// p.w.inv_temps[t] = 1 / T_t and p.w.out[4 t ..] = (ln_z, mean_e, var_e, neff_fraction) of T_t on the device.  Does not wait
// (`inv`: see upload_targets).
hipError_t reweight_enqueue(Problem &p, const MbarSamples &sm, const double *temps, int n_temps, std::vector<double> &inv);
// the host copy `out` of such a p.w.out into those of the four arrays that are not nullptr
void unpack_targets(const std::vector<double> &out, int n_temps, double *ln_z, double *mean_e, double *var_e, double *neff_fraction);
// ME_ERR_INVALID unless f[0 .. n_rungs) is there and finite, n >= min_targets and temps[0 .. n) is there, finite and > 0
int check_f_and_targets(me_engine *e, const double *f, int n_rungs, const double *temps, int n, int min_targets);
// what an operation on `p` returned, or p's empty rung, as the ME_* code of an entry point
int mbar_check_common(me_engine *e, const Problem &p, hipError_t err);
int mbar_check_temps(me_engine *e, const double *temps, int n, const char *what);

// ---- defined in me_mbar_obs.hip -----------------------------------------------------------------------------------------
// Device scratch of one observable reweighting: d_n of every sample and the block partials
struct ObsScratch {
  DeviceBuffer d, partials;
};
// Enqueues d_n = m_n + ln s_n of every sample of `sm` into `d`, sized here to whole tiles: NaN for a sample whose energy is not
// finite and for the padding behind the last sample.  Does not wait: `d` is the caller's to keep.
hipError_t log_denominator_enqueue(Problem &p, const MbarSamples &sm, DeviceBuffer &d);
// Enqueues the reweighting of the columns `oc` of `sm` (the problem's samples, or the used ones of them packed) to the n_temps
// temperatures whose 1 / T_t are on the device at inv_temps: afterwards out = [mean | var | cov_energy][target][column], then
// neff_fraction[target], 3 n_temps Q + n_temps doubles of device memory.  Does not wait: `scratch` is the caller's to keep until
// the stream has been waited for.
hipError_t reweight_observables_enqueue(Problem &p, const MbarSamples &sm, const ObsColumns &oc, const double *inv_temps, int n_temps,
                                        ObsScratch &scratch, double *out);
// me_energy_samples_record's second kernel: row `row` of the engine's observable store (which exists) on the engine's stream
hipError_t observable_record_enqueue(me_engine *e, long long row);


// ---- defined in me_mbar_cov.hip -----------------------------------------------------------------------------------------
// The Gram matrix of the weight matrix [K ladder columns | state and energy column of each target]: prepares `p`, waits for the
// stream and writes host arrays gram[C][C] (C = n_rungs + 2 n_targets), column_counts[C], ln_z / mean_e[n_targets] (may be
// nullptr).  With an empty rung (p.empty_rung) nothing else is computed.
hipError_t mbar_gram(Problem &p, const Source &src, const double *f, const double *temps, int n_targets, double *gram,
                     double *column_counts, double *ln_z, double *mean_e);

// ---- defined in me_mbar_hist.hip ----------------------------------------------------------------------------------------
// A histogram request: edges[n_bins + 1] and the host outputs mass[n_temps][n_bins + 3], counts[n_bins + 3], neff[n_temps] (each
// may be nullptr)
struct Histogram {
  const double *edges;
  int n_bins;
  double *mass;
  int64_t *counts;
  double *neff;
};
// what a histogram leaves on the device for a pass that follows it: d_n of every sample (log_denominator_enqueue), the edges (of
// both axes, one after the other, for a joint histogram), and `top` of slot_of (me_mbar_slots.h) for the one or two edge arrays
struct HistogramScratch {
  DeviceBuffer d, edges;
  int top = 1, top_y = 1;
};
// A table of n_slots columns for histogram_slots: the host edges (n_edges of them, as the pass kernel reads them), the
// temperatures per pass, the host outputs mass[n_temps][n_slots], counts[n_slots], neff[n_temps] (each may be nullptr), and
// `launch`, which enqueues on the problem's stream the unit's pass kernel (slot_pass, me_mbar_slots.h) for the n_rows <= rows
// temperatures from t0 on (p.w.inv_temps + t0, p.w.out + 4 t0) into partials[block][rows][n_slots]; the pass of t0 = 0 is the
// one whose count_partials[block][n_slots] are read
struct SlotTable {
  const double *edges;
  int n_edges, n_slots, rows;
  double *mass;
  int64_t *counts;
  double *neff;
  std::function<void(int t0, int n_rows, double *partials, unsigned long long *count_partials)> launch;
};
// The driver of the histogram units: prepares `p`, reweights to temps[0 .. n_temps) (afterwards p.w.inv_temps and p.w.out are
// reweight_enqueue's), writes d_n and the edges into `keep`, runs one pass per chunk of `rows` temperatures, each followed by the
// sum of its block partials and the normalisation of its rows, copies back and waits for the stream.  `keep` is filled before
// the first launch, so `launch` may refer to it.  With an empty rung nothing else is computed and `keep` holds no buffers.
hipError_t histogram_slots(Problem &p, const Source &src, const double *f, const double *temps, int n_temps, const SlotTable &table,
                           HistogramScratch &keep);
// histogram_slots for the one column `values` (n_columns = 1).  keep.top is set from the bin count before anything else,
// whether or not a rung turns out empty.
hipError_t histogram(Problem &p, const Source &src, const ObsColumns &values, const double *f, const double *temps, int n_temps,
                     const Histogram &h, HistogramScratch &keep);
// ME_ERR_INVALID unless 1 <= n_bins <= ME_MAX_HISTOGRAM_BINS and edges[0 .. n_bins] is there, finite and strictly increasing
int check_edges(me_engine *e, const double *edges, int n_bins);
// `values` = the column of an engine's Source that a histogram entry point names: a recorded column (ME_ERR_STATE without an
// observable store, ME_ERR_INVALID beyond the recorded columns) or, for -1, the energies themselves
int histogram_column(const Source &src, int column, ObsColumns &values);

// ---- defined in me_mbar_hist_cov.hip ------------------------------------------------------------------------------------
// The slot Gram sums of n_slots columns for slot_gram_passes: the rows per pass, the host output gram[n_temps][n_rungs + 1]
// [n_slots] (nullptr: not asked for), and `launch`, which enqueues on the problem's stream the unit's pass kernel (slot_pass
// with GramRows<rows>) for rows j0 .. j0 + n_rows, n_rows <= rows, of target t (p.w.inv_temps + t, p.w.out + 4 t) into
// partials[block][rows][n_slots]
struct SlotGramTable {
  int n_slots, rows;
  double *gram;
  std::function<hipError_t(int t, int j0, int n_rows, double *partials)> launch;
};
// The driver of the Gram units, for a problem whose histogram_slots has just run (p.w.inv_temps and p.w.out hold its targets):
// one pass per (t, chunk of `rows` rows), each followed by the sum of its block partials, then one copy to table.gram.  Waits
// for the stream.
hipError_t slot_gram_passes(Problem &p, const SlotGramTable &table, int n_temps);
// The stages of a *_gram entry point behind its argument checks: `histogram` (the unit's histogram into `keep`) in a problem of
// its own, in which the sums of `gram_table` follow when their output is asked for; then, with that problem's device scratch
// and d_n freed, the ladder block ladder_gram[K][K] and column_counts[K] (mbar_gram with no targets, me_mbar_cov.hip) in a
// second problem when either is asked for, and *n_used.  `gram_table` may refer to the problem and to `keep`.
struct LadderGram {
  double *ladder_gram, *column_counts;
  int64_t *n_used;
};
int histogram_gram_stages(const Source &src, const double *f, int n_temps,
                          const std::function<hipError_t(Problem &, HistogramScratch &)> &histogram,
                          const std::function<SlotGramTable(const Problem &, const HistogramScratch &)> &gram_table,
                          const LadderGram &out);

// ---- defined in me_mbar_hist2d.hip --------------------------------------------------------------------------------------
// A joint histogram request: the edges of both axes and the host outputs mass[n_temps][Bx + 3][By + 3], counts[Bx + 3][By + 3],
// neff[n_temps] (each may be nullptr)
struct Histogram2d {
  const double *edges_x;
  int n_bins_x;
  const double *edges_y;
  int n_bins_y;
  double *mass;
  int64_t *counts;
  double *neff;
};
// The two value columns that go with the problem's samples: x and y share n_chains and record_stride; nullptr = the energy
struct ValuePair {
  const double *x, *y;
  long long n_chains, record_stride;
};
// histogram_slots for the S cells of the grid and the concatenated edges; R, the edges and both `top` are worked out from the
// request before the problem is prepared.  `keep` as histogram()'s: d_n and [edges_x | edges_y] for a pass that follows.
hipError_t histogram2d(Problem &p, const Source &src, const ValuePair &values, const double *f, const double *temps, int n_temps,
                       const Histogram2d &h, HistogramScratch &keep);
// the argument checks of a joint histogram entry point, in their order: both edge arrays (check_edges), the cell cap
// ME_MAX_HISTOGRAM2D_SLOTS, then check_f_and_targets with at least one target
int check_histogram2d(const Source &src, const double *f, const double *temps, int n, const Histogram2d &h);
// `values` = the two columns of an engine's Source that a joint entry point names (histogram_column for each; recorded columns
// share the store's strides, and the energy is read as the energy, nullptr, whatever the other axis is)
int joint_columns(const Source &src, int column_x, int column_y, ValuePair &values);
// `values` = the host columns values_x, values_y [n_samples] of a host-form Source (after from_host), put on the device in
// src.columns_dev for the length of the call
int joint_upload(Source &src, const double *values_x, const double *values_y, int64_t n_samples, ValuePair &values);

}  // namespace mbar
}  // namespace me

#pragma GCC visibility pop
