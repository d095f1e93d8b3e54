/*
 * metropolis_engine.h -- C ABI of libmetropolis_hip.so, the MI355X (gfx950) many-chain Metropolis engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference has no FFI: its "plugin API" is
 * the Python class MetropolisEngine (the reference's metropolisengine/metropolis_engine.py:10-463).  Each
 * entry point below replaces one piece of that class for N independent chains on one GPU; the Python class
 * metropolisengine_amd.MetropolisEngine binds them with ctypes (see INTEGRATION.md for the stub).
 *
 *   me_create            <- MetropolisEngine.__init__               metropolis_engine.py:17-133
 *   me_step              <- step_all / step_real_group / step_complex_group
 *                           (+ draw_*_group, metropolis_decision, update_*_sigma)   :209-338, :429-456
 *   me_measure           <- measure / measure_real_system / measure_complex_system
 *                           (+ update_*_mean, update_covariance_matrix_*, observables) :342-427, :458-463
 *   me_get / me_set      <- attribute reads/writes (real_params, real_mean, covariance_matrix_real, ...)
 *                           README.md:49-51; also the only "checkpoint" the reference has (ctor warm start, :17)
 *   me_accept_stats      <- the bool returned by step_all (:259), accumulated
 *   me_pooled_moments*   <- no reference equivalent (ensemble estimate across chains)
 *   me_set_temperature_ladder, me_replica_*  <- no reference equivalent (parallel tempering across the chains)
 *   me_set_temperature   <- the constructor's temp (:92), changed on a running engine (simulated annealing)
 *   me_population_*      <- no reference equivalent (population annealing: Boltzmann resampling, free energies)
 *   me_comm_*, me_pooled_moments_allreduce*  <- no reference equivalent (the one collective: RCCL all-reduce of the moments)
 *   me_last_error        <- Python exceptions (:39 ValueError, :92/:438 AssertionError, numpy ValueError :270)
 *
 * Conventions: plain pointers and sizes only; every function returns an me_status (0 = ok); the library owns
 * all device memory; host buffers are caller-owned.  Host-side layouts are row-major [chain][component] doubles
 * whatever the device dtype.  Calls on one engine must not be concurrent (the reference is not reentrant
 * either); different engines may be driven from different threads.  me_step/me_measure are asynchronous on the
 * engine's HIP stream; me_get/me_accept_stats/me_pooled_moments synchronise that stream.
 *
 * State vector of one chain: D = n_real + 2*n_complex reals, ordered
 *   [ real params | real parts of complex params | imaginary parts of complex params ].
 */
#ifndef METROPOLIS_ENGINE_H
#define METROPOLIS_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ME_ABI_VERSION 1

typedef struct me_engine me_engine; /* opaque handle */

typedef enum me_status {
  ME_OK = 0,
  ME_ERR_INVALID = 1,     /* bad argument (the reference raises ValueError / AssertionError) */
  ME_ERR_UNSUPPORTED = 2, /* no kernel compiled for this (dtype, n_real, n_complex, energy, ...) */
  ME_ERR_HIP = 3,         /* HIP runtime error, no device, out of memory */
  ME_ERR_NUMERIC = 4,     /* a chain produced a non-finite energy / non-positive Cholesky pivot / width */
  ME_ERR_STATE = 5        /* call not valid in the engine's current state */
} me_status;

typedef enum me_dtype { ME_F32 = 0, ME_F64 = 1 } me_dtype;

/* Energy kinds: the reference takes a Python callable (metropolis_engine.py:20, :111-120); a GPU build needs
 * a device-side specification instead.  Coefficients are doubles, converted to the device dtype. */
typedef enum me_energy_kind {
  ME_ENERGY_ISO_QUAD = 0,   /* coeffs {a}: a (sum x_i^2 + sum |z_j|^2)                  README.md:26-27 */
  ME_ENERGY_DIAG_QUAD = 1,  /* coeffs {a_0..a_{nr-1}, b_0..b_{nc-1}}: sum a x^2 + sum b |z|^2 */
  ME_ENERGY_DENSE_QUAD = 2, /* coeffs A[D*D] row-major: x^T A x over the real D-vector */
  ME_ENERGY_LANDAU_TOY = 3, /* coeffs {k, alpha, beta}, nr=2, nc=1   demo/toymodel_complex_and_real.py:17-26 */
  ME_ENERGY_CYLINDER = 4,   /* coeffs {kappa, gamma, wavenumber}: cylinder-style surrogate */
  ME_ENERGY_USER = 5,       /* user-written device function from a plugin (include/metropolis_user_energy.h),
                               inlined into the kernels; coeffs are handed to it in device memory */
  ME_ENERGY_USER_INDIRECT = 6, /* the same function called through a __device__ function pointer */
  ME_ENERGY_LANDAU_TERMS = 7  /* the Landau toy as the reference demo passes it: a term dictionary {"field": both
                                 groups, "area": real group} (demo/toymodel_complex_and_real.py:17-33); two ledger rows */
} me_energy_kind;

/* Hard-wall predicate evaluated before the energy (metropolis_engine.py:142-146, :247-249). */
typedef enum me_reject_kind {
  ME_REJECT_NONE = 0,
  ME_REJECT_ABS_REAL0_GE = 1, /* reject when |x_0| >= reject_bound  (legacy /metropolis_engine.py:139-141) */
  ME_REJECT_USER = 2          /* the plugin's me_user_reject (include/metropolis_user_energy.h); user energies only */
} me_reject_kind;

/* Which matrix shapes the proposals. */
typedef enum me_cov_mode {
  ME_COV_REFERENCE = 0, /* initial matrix until measure_step_counter > 50, then each chain's own running
                           covariance (metropolis_engine.py:389, :416-427) */
  ME_COV_FIXED = 1,     /* keep the initial matrix for ever (measure() still updates the statistics) */
  ME_COV_POOLED = 2     /* one factor shared by all chains, installed with me_set_shared_factor */
} me_cov_mode;
/* Availability: every mode for every parameter space up to 96 real degrees of freedom (n_real + 2 n_complex; plugins and
   kernel sets compiled for one size: any size).  Beyond that -- the runtime-dimension kernel set -- ME_COV_FIXED and
   ME_COV_REFERENCE for every space whose D x 64 values fit the LDS (float64: D <= 290), ME_COV_POOLED for pure real spaces
   (two such blocks: D <= 145 in float64); me_create answers ME_ERR_UNSUPPORTED otherwise. */

/* Per-chain fields for me_get / me_set; components per chain in brackets (P = nr(nr+1)/2 + nc^2). */
typedef enum me_field {
  ME_FIELD_PARAMS = 0,   /* [D]  current state */
  ME_FIELD_ENERGY = 1,   /* [T]  the energy ledger, one row per energy term (metropolis_engine.py:111-116, :152-155);
                                 T = 1 ("total") unless the energy is a term dictionary (me_energy_terms) */
  ME_FIELD_WIDTH = 2,    /* [1] the group's sampling width; mixed engines [3]: sampling_width, real group, complex group */
  ME_FIELD_MEAN = 3,     /* [D]  running mean */
  ME_FIELD_COV = 4,      /* [P]  running covariance, packed: real block row-major lower triangle, then for
                                 each complex row i: (Re,Im) of K_ij for j<i, then K_ii */
  ME_FIELD_OBS_MEAN = 5, /* [2nr+nc] running mean of |x_r|, |z_c|, x_r^2 */
  ME_FIELD_FACTOR = 6,   /* [P]  Cholesky factors used by the proposals (same packing; conj(K) for complex) */
  ME_FIELD_ENERGY_TOTAL = 7 /* [1] ME_FLAG_REFERENCE_ENERGY_LEDGERS only: the separate `energy_total` that step_all of a
                               mixed engine compares against and updates (metropolis_engine.py:252-255) */
} me_field;

/* me_config.flags */
typedef enum me_flags {
  ME_FLAG_TRACK_COVARIANCE = 1, /* parameter spaces whose per-chain matrix is too large for registers (more than 160
                                  packed entries, e.g. 64 real parameters) keep it only where the proposals need it
                                  (ME_COV_REFERENCE, pure real spaces: streamed kernels); with ME_COV_FIXED / ME_COV_POOLED
                                  they keep means and observables only.  With this flag measure() also maintains each
                                  chain's running covariance (metropolis_engine.py:416-427) there, as statistics -- P values
                                  per chain, read and written once per measure().  Smaller spaces always track it. */
  ME_FLAG_REFERENCE_ENERGY_LEDGERS = 2 /* reproduce the reference's TWO energy ledgers: step_all of a
                                  mixed engine compares against and updates `energy_total` only (metropolis_engine.py:
                                  252-255), group steps compare against and update `energy[term]` only (:214-221,
                                  :230-237), so a driver that mixes both call styles decides on stale energies exactly
                                  as the reference does.  Default: one coherent ledger per chain.  Mixed engines only. */
} me_flags;

typedef struct me_config {
  uint32_t abi_version; /* ME_ABI_VERSION */
  int32_t device_id;    /* HIP device ordinal */
  int64_t n_chains;     /* chains held by THIS engine (local shard) */
  uint64_t chain_offset; /* global id of local chain 0: random streams are addressed by global id */
  uint64_t seed;
  int32_t n_real;
  int32_t n_complex;
  int32_t dtype;        /* me_dtype of the device state and arithmetic */
  int32_t cov_mode;     /* me_cov_mode */
  double temp;              /* >= 0 (metropolis_engine.py:91-92) */
  double target_acceptance; /* reference default 0.3 */
  double sampling_width;    /* reference default 0.05 */
  int32_t energy_kind;      /* me_energy_kind */
  int32_t n_energy_coeffs;
  const double *energy_coeffs;
  int32_t reject_kind; /* me_reject_kind */
  int32_t flags;       /* me_flags */
  double reject_bound;
  const double *initial_params;     /* [D], broadcast to every chain */
  const double *covariance_real;    /* [nr*nr] row-major or NULL = identity (metropolis_engine.py:63-66) */
  const double *covariance_complex; /* [nc*nc*2] row-major (Re,Im) or NULL = identity (:67-70) */
  const char *user_energy_name;     /* ME_ENERGY_USER*: name the plugin was built with (NULL otherwise) */
} me_config;

int me_abi_version(void);

/* Load a user-energy plugin library (built from the user's device function around the same kernels; it registers
 * itself).  The reference's counterpart is simply passing a Python callable (metropolis_engine.py:20). */
int me_load_plugin(const char *path);

int me_create(const me_config *config, me_engine **out);
int me_destroy(me_engine *engine);

/* n_sweeps fused propose->energy->accept->adapt sweeps over all chains in one launch; n_sweeps = 1 is one
 * reference step_all(). */
int me_step(me_engine *engine, int32_t n_sweeps);
/* Step kinds beyond step_all: a mixed engine's step_real_group / step_complex_group called directly
 * (metropolis_engine.py:225-239, :209-223: only that group moves and only its own width adapts) and the
 * magnitude-phase pair that replaces step_complex_group under complex_sample_method="magnitude-phase"
 * (:168-207; two accept decisions per step).  On pure-real / pure-complex engines the group kinds are step_all
 * (:46, :56).  me_step(e, k) == me_step_kind(e, ME_STEP_ALL, k). */
typedef enum me_step_kind_t {
  ME_STEP_ALL = 0,
  ME_STEP_REAL_GROUP = 1,
  ME_STEP_COMPLEX_GROUP = 2,
  ME_STEP_COMPLEX_MAGNITUDE_PHASE = 3
} me_step_kind_t;
int me_step_kind(me_engine *engine, int32_t kind, int32_t n_sweeps);
int me_measure(me_engine *engine);
/* One cycle of the reference's driver loop (README.md:41-44: `for j in range(k): step_all()` then `measure()`):
 * me_cycle(e, k) has exactly the results of me_step(e, k); me_measure(e), but where a fused kernel exists for the engine
 * (per-chain covariance kept in registers: up to 160 packed entries, step_all sweeps, identity or per-chain shape) it
 * is ONE launch -- state, energy and width are read once and written once, the sweeps run in registers, mean /
 * observables / covariance / factors are updated from the registers.  Otherwise the two launches are issued.
 * me_cycle_stats: how many me_cycle calls of this engine ran as one launch. */
int me_cycle(me_engine *engine, int32_t n_sweeps);
int me_cycle_stats(me_engine *engine, uint64_t *fused_cycles);
/* set_reject_condition (metropolis_engine.py:142-146): the wall predicate is a launch parameter and may be changed
 * between steps (in the reference this setter is the only working way to install one, quirk Q6). */
int me_set_reject_condition(me_engine *engine, int32_t reject_kind, double reject_bound);
/* set_energy_function (metropolis_engine.py:134-138): bind the engine to another energy of the SAME parameter space -- a
 * built-in kind (except ME_ENERGY_DENSE_QUAD) or a loaded user plugin -- re-collect the energy terms (the ledger is resized
 * when their number changes) and re-evaluate every term at the current state (initialize_energy_dict, :152-155).  The
 * chain state, widths, running statistics and counters stay.  Synchronous. */
int me_set_energy(me_engine *engine, int32_t energy_kind, const double *energy_coeffs, int32_t n_energy_coeffs,
                  const char *user_energy_name);
/* Test hook (float64 engines): the same step with the random draws supplied by the caller instead of Philox --
 * for the Gaussian kinds normals [n_sweeps][n_chains][D] standard normals and uniforms [n_sweeps][n_chains][1] accept
 * draws; for ME_STEP_COMPLEX_MAGNITUDE_PHASE normals [n_sweeps][n_chains][nc] and uniforms [n_sweeps][n_chains][nc+2]
 * = {accept (magnitude stage), nc phases in (0,1), accept (phase stage)}.  This is how the reference's golden
 * trajectories (tests/golden/, injected-stream runs of metropolis_engine.py) are replayed through the HIP kernels.
 * Synchronous. */
int me_step_injected(me_engine *engine, int32_t kind, int32_t n_sweeps, const double *normals, const double *uniforms);

int me_field_components(me_engine *engine, int32_t field, int32_t *n_components);
/* Rows of the energy ledger = number of energy terms (self.energy_term_names, metropolis_engine.py:112-118).  Group
 * steps re-evaluate and compare only the terms registered for their group (:214-221, :230-237). */
int me_energy_terms(me_engine *engine, int32_t *n_terms);
/* Copy chains [chain_begin, chain_begin + n_chains) of a field to/from host doubles [chain][component]. */
int me_get(me_engine *engine, int32_t field, int64_t chain_begin, int64_t n_chains, double *dst);
int me_set(me_engine *engine, int32_t field, int64_t chain_begin, int64_t n_chains, const double *src);
/* Re-evaluate the stored energies after me_set(ME_FIELD_PARAMS). */
int me_recompute_energy(me_engine *engine);

/* Robbins-Monro constants the engine derived (metropolis_engine.py:101-107): alpha, m, ratio. */
int me_constants(me_engine *engine, double *alpha, int32_t *m, double *ratio);
int me_counters(me_engine *engine, uint64_t *step_index, uint64_t *measure_step_counter);
int me_set_counters(me_engine *engine, uint64_t step_index, uint64_t measure_step_counter);
int me_accept_stats(me_engine *engine, uint64_t *accepted, uint64_t *proposed);
/* Restore the acceptance counters of a checkpoint (the reference has no counterpart: its only resume is the constructor
 * warm start, metropolis_engine.py:17). */
int me_set_accept_stats(me_engine *engine, uint64_t accepted, uint64_t proposed);

/* Ensemble sums over the local chains, fp64:
 *   [ n, sum x (D), sum x x^T (D(D+1)/2, row-major lower triangle), sum obs (2nr+nc), accepted, proposed ]
 * me_pooled_moments_size gives the length.  The _device form writes into caller-provided DEVICE memory (e.g. a
 * torch tensor) so that the caller can all-reduce it with RCCL in place; it is enqueued on the engine's stream
 * and followed by a stream synchronise. */
int me_pooled_moments_size(me_engine *engine, int64_t *n_doubles);
/* Which first stage the reduction of ALL the engine's chains launches (for tests that must know which kernel they hold to
 * account): matrix_core 1 = the Gram kernels of the engine's kernel set, 0 = the generic kernel; the chains it stages per
 * tile (64 / 32 / 16); the rows of partial sums, one per workgroup (matrix_core with at most 32 augmented rows, generic)
 * or per wavefront (matrix_core, 64 parameters). */
int me_pooled_moments_geometry(me_engine *engine, int32_t *matrix_core, int32_t *tile_chains, int32_t *partial_rows);
int me_pooled_moments(me_engine *engine, double *host_out, int64_t n_doubles);
int me_pooled_moments_device(me_engine *engine, void *device_out, int64_t n_doubles);
/* Split form that does not stall the engine's stream: _begin enqueues the reduction behind the work already queued and
 * the copy to the host on a second stream, and returns at once; steps and measures enqueued afterwards run while the
 * result travels.  _end waits for that copy only and hands out the moments of the state at the time of _begin.  One
 * reduction may be in flight per engine (ME_ERR_STATE otherwise). */
int me_pooled_moments_begin(me_engine *engine);
int me_pooled_moments_end(me_engine *engine, double *host_out, int64_t n_doubles);
/* RCCL behind the C ABI: the ONE collective of the engine, a sum all-reduce (fp64) of the pooled-moment vector over the
 * ranks of a multi-GPU job (one process and one engine per GPU; chains shard with no other exchange).  No reference
 * counterpart (the reference runs one chain in one process; BASELINE.json: "RCCL all-reduce only for the pooled
 * covariance/observables").  librccl is loaded on first use; ME_ERR_UNSUPPORTED when it cannot be.
 *   me_comm_unique_id   rank 0: ncclGetUniqueId into a caller buffer of ME_COMM_ID_BYTES, to be handed to every rank by
 *                       whatever channel the host program has (MPI, a file, torch.distributed, a socket)
 *   me_comm_init_rank   every rank: ncclCommInitRank on the engine's device (collective: returns when all have joined)
 *   me_comm_destroy     ncclCommDestroy (me_destroy does it too)
 *   me_comm_info        rank / world of the communicator (-1 / 0 without one) and the RCCL version code
 *   me_pooled_moments_allreduce        k_pool_reduce -> k_pool_finish on the engine's stream, then on the engine's second
 *                       stream behind an event: ncclAllReduce(sum, fp64, in place) -> copy to pinned host memory; waits for
 *                       that copy and hands out the moments of ALL ranks' chains (same layout as me_pooled_moments: n,
 *                       accepted and proposed are global too)
 *   me_pooled_moments_allreduce_begin  the same without waiting: collect with me_pooled_moments_end.  The engine's main
 *                       stream never waits for another rank and the host never synchronises inside a cycle
 * Every rank must call the all-reduce forms the same number of times, in the same order. */
#define ME_COMM_ID_BYTES 128
int me_comm_unique_id(void *id_out, size_t bytes);
int me_comm_init_rank(me_engine *engine, const void *unique_id, size_t bytes, int32_t rank, int32_t world);
int me_comm_destroy(me_engine *engine);
int me_comm_info(me_engine *engine, int32_t *rank, int32_t *world, int32_t *rccl_version);
int me_pooled_moments_allreduce(me_engine *engine, double *host_out, int64_t n_doubles);
int me_pooled_moments_allreduce_begin(me_engine *engine);
/* Install the shared proposal factor of ME_COV_POOLED: packed like ME_FIELD_FACTOR, [P] doubles. */
int me_set_shared_factor(me_engine *engine, const double *packed_factor, int64_t n_doubles);
/* Tuning knob (process-wide, default 224 MiB): launches whose working set exceeds this many bytes access their read-once
 * / write-once fields (packed covariance and factors, large running-mean fields) with the non-temporal cache policy, so
 * that the chain state stays resident in the 256 MiB Infinity Cache; 0 = always, a huge value = never. */
int me_set_cache_budget(int64_t bytes);
/* The factor last installed with me_set_shared_factor ([P] doubles, exactly as given); *is_set = 0 and the buffer is left
 * alone when none has been installed.  Part of a checkpoint of a ME_COV_POOLED engine. */
int me_get_shared_factor(me_engine *engine, double *packed_factor, int64_t n_doubles, int32_t *is_set);

/* Time series (metropolis_engine.py:350-356, :466-479): every me_measure appends one row per traced chain
 * (chains t*stride, t < n_traced) to a device-side series; me_trace_get returns it as doubles
 * [row][column][traced chain] with columns {params (D), energy, widths (1, or 3 for mixed engines)}.
 * n_traced = 0 switches recording off (the default). */
int me_trace_enable(me_engine *engine, int64_t n_traced, int64_t stride);
int me_trace_shape(me_engine *engine, int64_t *rows, int64_t *cols, int64_t *n_traced);
int me_trace_get(me_engine *engine, double *dst, int64_t n_doubles);

int me_sync(me_engine *engine);
/* Use an existing HIP stream (hipStream_t passed as void*) instead of the engine's own. */
int me_set_stream(me_engine *engine, void *hip_stream);
/* Enqueue n_launches launches of n_sweeps sweeps bracketed by HIP events on the engine's stream and return the
 * elapsed milliseconds (device time of the whole span). */
int me_time_steps(me_engine *engine, int32_t n_launches, int32_t n_sweeps, float *elapsed_ms);

/* Temperature ladders and replica exchange (parallel tempering; no reference counterpart).
 *   me_set_temperature_ladder  T_0 < T_1 < ... < T_{K-1}, all finite and > 0: the n_chains local chains become K rungs of
 *                       M = n_chains / K consecutive chains (M a multiple of 64, ME_ERR_INVALID otherwise); chain c steps at
 *                       T_{c / M} with exactly the scalar accept rule at that temperature.  Resets the swap round and the
 *                       swap counters.  n_rungs = 0 returns the engine to its scalar temp.  ME_ERR_UNSUPPORTED (with the
 *                       reason in me_last_error) on the runtime-dimension set (more than 96 real degrees of freedom), on
 *                       the matrix-core dense 64-parameter kernels and with ME_FLAG_REFERENCE_ENERGY_LEDGERS.
 *   me_temperature_ladder      the ladder (n_rungs = 0: none); temps must hold n_rungs doubles, or be NULL for the count.
 *   me_replica_exchange        enqueue n_rounds swap rounds on the engine's stream (asynchronous, like me_step).  Round r
 *                       pairs slot j of rung k with slot j of rung k+1 for every k = r (mod 2) and swaps the two chains'
 *                       configurations (ME_FIELD_PARAMS and every ME_FIELD_ENERGY row) with probability
 *                       min(1, exp((1/T_k - 1/T_{k+1}) (E_a - E_b))), E = the sum of the ledger rows; a non-finite energy
 *                       never swaps.  Widths, running means, covariances, factors and counters stay with the slot.  The
 *                       uniform is word 0 of Philox block 0xffff at (global chain id of the rung-k chain, round).
 *   me_replica_stats           the round counter and, per adjacent pair (k, k+1), the attempted and accepted swaps
 *                       (n_pairs = n_rungs - 1); me_set_replica_stats restores them from a checkpoint.
 *   me_pooled_moments_range    me_pooled_moments over chains [chain_begin, chain_begin + n_chains), whole 64-chain tiles
 *                       (e.g. one rung).  Same layout; the two trailing entries (accepted, proposed) are 0 for a range:
 *                       acceptance is counted per wavefront of a launch, not per chain (me_accept_stats has the totals). */
int me_set_temperature_ladder(me_engine *engine, const double *temps, int32_t n_rungs);
int me_temperature_ladder(me_engine *engine, double *temps, int32_t capacity, int32_t *n_rungs);
int me_replica_exchange(me_engine *engine, int32_t n_rounds);
int me_replica_stats(me_engine *engine, uint64_t *round, uint64_t *attempted, uint64_t *accepted, int32_t n_pairs);
int me_set_replica_stats(me_engine *engine, uint64_t round, const uint64_t *attempted, const uint64_t *accepted,
                         int32_t n_pairs);
int me_pooled_moments_range(me_engine *engine, int64_t chain_begin, int64_t n_chains, double *host_out, int64_t n_doubles);

/* Scalar temperature and population annealing (no reference counterpart).
 *   me_set_temperature         the scalar temp of a running engine, finite and >= 0; the next step uses it (plain simulated
 *                       annealing).  ME_ERR_STATE on a ladder engine.
 *   me_population_resample     enqueue one population-annealing stage from T_old = temp > 0 to new_temp (finite, > 0) on the
 *                       engine's stream (asynchronous, like me_step).  E_i = the sum of chain i's ledger rows in row order in
 *                       the device dtype, l_i = -(1/new_temp - 1/T_old) E_i in float64 (weight 0 when not finite), M = max l_i,
 *                       w_i = exp(l_i - M), W = sum w_i, S2 = sum w_i^2 (fixed summation order: bitwise reproducible).  The
 *                       stage records log_weight = M + ln(W / N), the estimate of ln Z(new_temp) / Z(T_old), neff_fraction =
 *                       W^2 / (N S2) and n_finite, then resamples systematically with one uniform u = word 0 of Philox block
 *                       0xfffe at counter (chain_offset, stage index): slot j takes chain a_j = min{ i : N C_i / W > j + u },
 *                       C_i = w_0 + ... + w_i (slots left undefined by rounding take the last chain of positive weight).  Slot
 *                       j receives chain a_j's configuration (ME_FIELD_PARAMS and every ME_FIELD_ENERGY row) and its family
 *                       id; widths, running means, covariances, factors, traces and counters stay with the slot, exactly as
 *                       in a replica-exchange swap.  Then temp = new_temp.  n_finite = 0 leaves the population unchanged and
 *                       records log_weight = -inf, neff_fraction = 0; new_temp = temp is the identity (log_weight = 0).
 *                       ME_ERR_STATE on a ladder engine or with temp = 0; ME_ERR_UNSUPPORTED with
 *                       ME_FLAG_REFERENCE_ENERGY_LEDGERS.  Each engine (GPU shard) is an independent population: the shards'
 *                       stages combine as ln mean_w = logsumexp_s(log_weight_s + ln N_s) - ln sum_s N_s.
 *   me_population_stats        the stage count and, per stage, its new temperature, log_weight, neff_fraction and n_finite
 *                       (waits for the stream).  Any pointer may be NULL; the arrays given must hold `stages` entries
 *                       (capacity).  me_set_population_stats restores them from a checkpoint.
 *   me_population_families     family ids of chains [chain_begin, chain_begin + n): int64, the global chain id of each
 *                       slot's founder (chain_offset + j before the first stage; non-decreasing in j on every engine that
 *                       was only resampled).  me_set_population_families restores them. */
int me_set_temperature(me_engine *engine, double temp);
int me_population_resample(me_engine *engine, double new_temp);
int me_population_stats(me_engine *engine, uint64_t *stages, double *stage_temps, double *log_weight, double *neff_fraction,
                        int64_t *n_finite, int64_t capacity);
int me_set_population_stats(me_engine *engine, uint64_t stages, const double *stage_temps, const double *log_weight,
                            const double *neff_fraction, const int64_t *n_finite);
int me_population_families(me_engine *engine, int64_t chain_begin, int64_t n, int64_t *dst);
int me_set_population_families(me_engine *engine, int64_t chain_begin, int64_t n, const int64_t *src);

/* Energy samples, MBAR free energies and temperature reweighting of a ladder (no reference counterpart; csrc/me_mbar.hip
 * has the definition).
 *   me_energy_samples_enable   allocate a float64 device field [capacity_records][n_chains] and set the record count to 0;
 *                       capacity_records = 0 frees it.  Any engine with one coherent ledger (ladder or scalar temp, every
 *                       kernel set); ME_ERR_UNSUPPORTED with ME_FLAG_REFERENCE_ENERGY_LEDGERS.
 *   me_energy_samples_record   enqueue one kernel on the engine's stream (asynchronous, like me_step): the next row gets E_i for
 *                       every chain, E_i = the sum of chain i's ledger rows in row order in the device dtype, widened to
 *                       float64 (the quantity of me_replica_exchange and me_population_resample).  ME_ERR_STATE when the
 *                       store is not enabled or full.
 *   me_energy_samples_count    rows recorded and the capacity (0, 0 when not enabled).
 *   me_energy_samples_get      rows [record_begin, record_begin + n_records) as [record][chain] doubles (waits for the stream).
 *   me_energy_samples_set      replace the content by n_records host rows (<= capacity): resumes a run; a checkpoint
 *                       (me_get / me_set of the fields) does NOT carry the samples.
 *   A sample is indexed by its slot; slot c belongs to rung c / M whatever was swapped into it.  me_set_temperature_ladder
 *   therefore sets the record count to 0: samples taken under another ladder would be attributed to the wrong temperatures.
 *   me_mbar_solve              the multistate Bennett acceptance ratio over the recorded samples and the engine's ladder
 *                       (K rungs): f_k = -ln Z(T_k) / Z(T_0) by self-consistent iteration from f = 0 until the largest
 *                       change of an f_k is <= tolerance (> 0) or max_iterations (>= 1) are done; *residual is that last
 *                       change, *iterations the count, n_used[k] the finite samples of rung k (non-finite energies are
 *                       skipped).  All sums have a fixed order: a solve is bitwise reproducible.  ME_ERR_STATE without a
 *                       ladder, without records, or when a rung has no finite sample; ME_ERR_UNSUPPORTED beyond 64 rungs.
 *   me_mbar_solve_newton       the same free energies by Newton's method (csrc/me_mbar_newton.hip has the iteration): two
 *                       self-consistent passes, then Newton steps f <- f + H^-1 (N - S) with H = diag(S) - W^T W formed on
 *                       the matrix cores in the same pass over the samples; a Newton step after which gamma = max_k |S_k /
 *                       N_k - 1| did not fall is withdrawn and a failed Cholesky factorisation skipped, each in favour of a
 *                       self-consistent step (*fallback_steps counts both, *newton_steps the Newton steps taken).  Every pass
 *                       over the samples counts as an iteration; tolerance, max_iterations, *residual, n_used and the error
 *                       codes as for me_mbar_solve; *gradient is gamma at the last pass.  Converges quadratically where
 *                       me_mbar_solve converges linearly, at about the rounding error of f.  Bitwise reproducible.  Any
 *                       output pointer but f_out may be NULL.  me_mbar_solve_newton_samples: the same on host arrays.
 *   me_mbar_reweight           for each of the n target temperatures (finite, > 0), from f of me_mbar_solve: ln_z =
 *                       ln Z(T) / Z(T_0), the mean and variance of the energy at T and neff_fraction = (sum w)^2 / (N sum w^2)
 *                       of the reweighting weights w (N = all finite samples).  Any output pointer may be NULL.
 *   me_mbar_solve_samples / me_mbar_reweight_samples   the same kernels on host arrays (engine-independent, like
 *                       me_detect_equilibration): energies[n_samples], rungs[n_samples] in [0, n_rungs), ladder_temps[n_rungs]
 *                       finite and > 0 (any order).  For samples gathered from several shards, and for subsets of a run.
 *   me_mbar_gram               the Gram matrix G = W^T W of the MBAR weight matrix, from which the asymptotic covariance of
 *                       the free energies and of reweighted energies follows on the host (Shirts & Chodera 2008, eqs. 8,
 *                       D8; csrc/me_mbar_cov.hip has the definition).  f from me_mbar_solve; n_targets >= 0 target
 *                       temperatures (finite, > 0; temps may be NULL when there are none).  W has C = n_rungs + 2 n_targets
 *                       columns: column k < n_rungs is rung k (column_counts[k] = its finite samples), columns n_rungs + 2 t
 *                       and n_rungs + 2 t + 1 are the state and the energy-weighted state of target t (counts 0).  gram is
 *                       [C][C], full and bitwise symmetric; column_counts is [C]; ln_z and mean_e ([n_targets], may be NULL)
 *                       are me_mbar_reweight's values (bit for bit when every energy is finite; otherwise the finite samples
 *                       are packed first, in their order, and every result is bit for bit the result on the samples with
 *                       the others removed); *n_used (may be NULL) the finite samples.  Any number of
 *                       targets: they go through the device in chunks with n_rungs + 2 chunk <= 128, every chunk with the
 *                       ladder columns, and the blocks of gram that pair targets of different chunks are NaN (the variances
 *                       need the ladder-target and the same-target blocks only).  All sums have a fixed order.  Error codes
 *                       as for me_mbar_reweight.
 *   me_mbar_gram_samples       the same on host arrays, as me_mbar_reweight_samples.
 *   me_mbar_energy_shift       E_shift of me_mbar_gram's energy columns over the engine's records, (the least finite recorded
 *                       energy) - 1, from the device by the kernels me_mbar_gram takes it from: one read of the samples and
 *                       8 bytes to the host.  The standard error of a reweighted energy needs mean_t = mean_e - E_shift.
 *                       ME_ERR_STATE without a ladder, without records or without a finite sample. */
int me_energy_samples_enable(me_engine *engine, int64_t capacity_records);
int me_energy_samples_record(me_engine *engine);
int me_energy_samples_count(me_engine *engine, int64_t *records, int64_t *capacity);
int me_energy_samples_get(me_engine *engine, int64_t record_begin, int64_t n_records, double *dst);
int me_energy_samples_set(me_engine *engine, int64_t n_records, const double *src);
int me_mbar_solve(me_engine *engine, double tolerance, int32_t max_iterations, double *f_out, int32_t *iterations,
                  double *residual, int64_t *n_used_out);
int me_mbar_solve_newton(me_engine *engine, double tolerance, int32_t max_iterations, double *f_out, int32_t *iterations,
                         double *residual, double *gradient, int32_t *newton_steps, int32_t *fallback_steps, int64_t *n_used_out);
int me_mbar_solve_newton_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                 const double *ladder_temps, int32_t n_rungs, double tolerance, int32_t max_iterations,
                                 double *f_out, int32_t *iterations, double *residual, double *gradient, int32_t *newton_steps,
                                 int32_t *fallback_steps, int64_t *n_used_out);
int me_mbar_reweight(me_engine *engine, const double *f, const double *temps, int32_t n, double *ln_z, double *mean_e,
                     double *var_e, double *neff_fraction);
int me_mbar_solve_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                          const double *ladder_temps, int32_t n_rungs, double tolerance, int32_t max_iterations, double *f_out,
                          int32_t *iterations, double *residual, int64_t *n_used_out);
int me_mbar_reweight_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                             const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                             double *ln_z, double *mean_e, double *var_e, double *neff_fraction);
int me_mbar_gram(me_engine *engine, const double *f, const double *temps, int32_t n_targets, double *gram,
                 double *column_counts, double *ln_z, double *mean_e, int64_t *n_used);
int me_mbar_gram_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                         const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n_targets,
                         double *gram, double *column_counts, double *ln_z, double *mean_e, int64_t *n_used);
int me_mbar_energy_shift(me_engine *engine, double *shift);

/* Recorded observables of a ladder and their reweighting to any temperature (no reference counterpart; csrc/me_mbar_obs.hip
 * has the definition).  A chain's recordable quantities form a catalogue indexed q (D = n_real + 2 n_complex, NOBS = 2 n_real
 * + n_complex, T = me_energy_terms):
 *     [0, D)                     the state rows in ME_FIELD_PARAMS component order (x_r, Re z_c, Im z_c), widened to float64
 *     [D, D + NOBS)              |x_r|, |z_c|, x_r^2 in ME_FIELD_OBS_MEAN order, formed in float64 from the WIDENED components:
 *                                fabs(x), sqrt(fma(re, re, im * im)) with the correctly rounded square root, x * x -- so that
 *                                the host can restate a record exactly whatever the device dtype (this is not the device-dtype
 *                                arithmetic of me_measure)
 *     [D + NOBS, D + NOBS + T)   the ledger rows (energy terms, row order), widened to float64
 *   me_observable_samples_enable   needs an enabled energy store (ME_ERR_STATE otherwise); 1 <= n_observables <=
 *                       ME_MAX_RECORDED_OBSERVABLES indices inside the catalogue (ME_ERR_INVALID otherwise; duplicates are
 *                       allowed).  Allocates a zero-filled float64 device field [capacity][n_observables][n_chains] for the
 *                       energy store's capacity and sets the record count of BOTH stores to 0: from then on
 *                       me_energy_samples_record also enqueues the kernel that fills the observables' row, so record r of
 *                       both stores is the same moment.  n_observables = 0 frees the field (the energy records stay).
 *                       me_energy_samples_enable frees it too (a new energy store forgets everything), and
 *                       me_set_temperature_ladder empties both stores together.  ME_ERR_UNSUPPORTED with
 *                       ME_FLAG_REFERENCE_ENERGY_LEDGERS.
 *   me_observable_samples_info     the number of recorded columns (0: no store) and their catalogue indices (`indices` has room
 *                       for ME_MAX_RECORDED_OBSERVABLES entries, may be NULL).
 *   me_observable_samples_get      rows [record_begin, record_begin + n_records) as [record][column][chain] doubles (waits for
 *                       the stream).
 *   me_observable_samples_set      replace the rows by n_records host rows; n_records must equal the current energy record
 *                       count (ME_ERR_INVALID otherwise): to resume a run call me_energy_samples_set first, then this.
 *                       me_energy_samples_set leaves the observable rows as they are; rows never written are zero.
 *   me_mbar_reweight_observables   for each of the n target temperatures (finite, > 0) and each recorded column A_q, with the
 *                       weights w of me_mbar_reweight (a sample is used when its ENERGY is finite): mean = sum w A_q / sum w,
 *                       var = sum w (A_q - mean)^2 / sum w, cov_energy = sum w (A_q - mean)(E - mean_E) / sum w, all [n][Q],
 *                       and neff_fraction [n]; d<A_q>/dT = cov_energy / T^2.  Any output may be NULL.  A non-finite value of
 *                       column q in a used sample makes column q's results non-finite and leaves every other column's results
 *                       bitwise unchanged.  All sums have a fixed order, and column q at target t is bit for bit the same
 *                       whether it is asked for alone or among 16 columns and any number of targets.  Errors as for
 *                       me_mbar_reweight, plus ME_ERR_STATE without an observable store.
 *   me_mbar_reweight_observables_samples   the same kernels on host arrays, like me_mbar_reweight_samples; observables is
 *                       [n_observables][n_samples], 1 <= n_observables <= ME_MAX_RECORDED_OBSERVABLES.
 *   me_mbar_reweight_perturbed   reweighting to states that differ from the sampled ones by more than their temperature (csrc/
 *                       me_mbar_perturbed.hip has the definition).  Target p has the temperature temps[p] (finite, > 0) and the
 *                       couplings couplings[p][0 .. Q) (finite) over the Q recorded columns; its energy is H = E + b with b =
 *                       sum_q couplings[p][q] A_q over the columns whose coupling is not exactly 0, in ascending q, from 0.0, one
 *                       fma per term (a column whose coupling is 0 is not read for b), and its log weight fma(-H, 1 / T, -d_n)
 *                       with the d_n of me_mbar_reweight (a sample is used when its ENERGY is finite).  ln_z [n] = ln Z(T_p,
 *                       lambda_p) / Z(T_0, 0), the zero of me_mbar_reweight's ln_z; mean_h, var_h [n] the mean and variance of H;
 *                       mean, var, cov_h [n][Q] as me_mbar_reweight_observables' mean, var, cov_energy with H for E;
 *                       neff_fraction [n].  Any output may be NULL, any number of targets is taken.  With every coupling of a
 *                       target 0, H = E exactly and mean, var, cov_h, neff_fraction are me_mbar_reweight_observables' bit for
 *                       bit.  A non-finite value of a column that target p couples to, in a used sample, makes every output of
 *                       target p non-finite and changes no other target; one of a column it does not couple to makes only that
 *                       column's mean, var, cov_h non-finite.  All sums have a fixed order: a target is bit for bit the same
 *                       alone, among any others and at any position.  Errors as for me_mbar_reweight_observables (ME_ERR_STATE
 *                       without an observable store), and ME_ERR_INVALID for couplings == NULL or a non-finite coupling.
 *   me_mbar_reweight_perturbed_samples   the same kernels on host arrays; observables is [n_observables][n_samples], couplings
 *                       [n][n_observables].
 *   me_mbar_gram_observables   me_mbar_gram for the asymptotic covariance of the reweighted means of the Q recorded columns
 *                       (csrc/me_mbar_cov.hip has the definition).  n_targets >= 1 target temperatures.  W has C = n_rungs +
 *                       n_targets (1 + Q) columns: column k < n_rungs is rung k (column_counts[k] = its finite samples), column
 *                       n_rungs + t (1 + Q) is the state of target t, W_na = exp(-E_n / T_t - d_n - ln_z_t), and column n_rungs +
 *                       t (1 + Q) + 1 + q its observable q, W_na (A_qn - S_q) / (mean_tq - S_q) (counts 0).  S_q = (the least
 *                       finite value of column q over the used samples) - 1, so every factor is >= 1; mean_tq is
 *                       me_mbar_reweight_observables' mean.  gram is [C][C], full and bitwise symmetric; column_counts is [C];
 *                       ln_z [n_targets], mean [n_targets][Q], shifts [Q] (= S_q) and *n_used may be NULL.  When some energy is
 *                       not finite the used samples AND their columns are packed first, in their order: every result is bit for
 *                       bit the result on the arrays with the other samples removed (so mean is me_mbar_reweight_observables'
 *                       bit for bit when every energy is finite).  A column q whose mean at target t is not finite (a
 *                       non-finite A_q in a used sample) gets NaN in the row and the column of gram of its columns, and no other
 *                       entry changes.  Targets go through the device in chunks of (128 - n_rungs) / (1 + Q) (at least 3),
 *                       every chunk with the ladder columns, and the blocks of gram that pair targets of different chunks are
 *                       NaN.  The entries that pair ladder and state columns are me_mbar_gram's bit for bit.  All sums have a
 *                       fixed order.  Errors as for me_mbar_gram, and ME_ERR_INVALID for n_targets < 1, ME_ERR_STATE without an
 *                       observable store.
 *   me_mbar_gram_observables_samples   the same on host arrays; observables is [n_columns][n_samples], 1 <= n_columns <=
 *                       ME_MAX_RECORDED_OBSERVABLES (ME_ERR_INVALID otherwise).
 *   me_mbar_gram_fluctuations  me_mbar_gram for the asymptotic errors of the reweighted SECOND moments: the energy variance
 *                       (heat capacity), and the variance and the energy covariance (d<A_q>/dT) of the Q recorded columns
 *                       (csrc/me_mbar_cov.hip has the definition, the fluctuation form).  n_targets >= 1.  With E' = E_n - E_shift
 *                       and A'_q = A_qn - S_q (E_shift = the least finite energy - 1, S_q as in me_mbar_gram_observables, so every
 *                       factor is >= 1), W has C = n_rungs + n_targets (3 + 3 Q) columns: column k < n_rungs is rung k, and from
 *                       column n_rungs + t (3 + 3 Q) on target t has its state column W_na, then W_na E' / m, W_na E'^2 / m, and
 *                       for each q in turn W_na A'_q / m, W_na A'_q^2 / m, W_na A'_q E' / m, each with the reweighted moment m of
 *                       its factor, formed on the device from what me_mbar_reweight and me_mbar_reweight_observables compute:
 *                       mean_e - E_shift, var_e + (mean_e - E_shift)^2, mean_q - S_q, var_q + (mean_q - S_q)^2, cov_energy_q +
 *                       (mean_q - S_q)(mean_e - E_shift).  moments is [n_targets][2 + 3 Q], these m in column order.  The products
 *                       are formed in registers: nothing of size n_samples x columns is stored.  The engine form uses the
 *                       observable store when there is one and runs with Q = 0 (the energy columns alone) otherwise.  gram is
 *                       [C][C], full and bitwise symmetric; column_counts [C]; ln_z, mean_e, var_e [n_targets] are
 *                       me_mbar_reweight's and mean, var, cov_energy [n_targets][Q] me_mbar_reweight_observables', bit for bit
 *                       when every energy is finite; *energy_shift, shifts [Q] and *n_used.  Every output but gram and
 *                       column_counts may be NULL.  Non-finite energies: packed away first as in me_mbar_gram_observables, every
 *                       result is bit for bit the result on the arrays without those samples.  A non-finite A_q in a used sample
 *                       gives the three columns of q at every target a NaN moment and NaN rows and columns of gram, and no other
 *                       entry changes.  Targets go through the device in chunks of (128 - n_rungs) / (3 + 3 Q) (at least 1), every
 *                       chunk with the ladder columns; the blocks of gram that pair targets of different chunks are NaN.  The
 *                       entries among ladder, state and E' columns are me_mbar_gram's bit for bit, those among ladder, state
 *                       and A'_q columns me_mbar_gram_observables'.  All sums have a fixed order.  Errors as for
 *                       me_mbar_gram_observables, except that a missing observable store is no error.
 *   me_mbar_gram_fluctuations_samples   the same on host arrays; observables is [n_columns][n_samples], 0 <= n_columns <=
 *                       ME_MAX_RECORDED_OBSERVABLES (ME_ERR_INVALID otherwise); n_columns = 0: observables may be NULL.
 *   me_mbar_histogram          the reweighted histogram of one quantity A over the recorded samples at each of the n target
 *                       temperatures (finite, > 0), with the normalised weights w of me_mbar_reweight (sum over the used
 *                       samples = 1; a sample is used when its ENERGY is finite; csrc/me_mbar_hist.hip has the definition).
 *                       column >= 0: the recorded observable column (ME_ERR_STATE without an observable store, ME_ERR_INVALID
 *                       beyond the recorded columns); column = -1: the energy itself, which needs the energy store only.
 *                       edges[n_bins + 1] finite and strictly increasing, any spacing, 1 <= n_bins <= ME_MAX_HISTOGRAM_BINS
 *                       (ME_ERR_INVALID otherwise).  Every used sample falls into exactly one of n_bins + 3 slots: bin b,
 *                       edges[b] <= A < edges[b + 1] (half-open everywhere); slot n_bins, A < edges[0] (-inf included); slot
 *                       n_bins + 1, A >= edges[n_bins] (+inf included: a value ON the last edge lies above); slot n_bins + 2,
 *                       A is NaN.  mass is [n][n_bins + 3], the sum of w per slot, divided by the total over all slots so that a
 *                       row sums to 1; counts [n_bins + 3] the used samples per slot (the same at every temperature);
 *                       neff_fraction [n] as me_mbar_reweight's.  Any output may be NULL.  A slot without a sample has mass
 *                       exactly 0.  No floating-point atomics: all sums have a fixed order, and a mass is bit for bit the same
 *                       run to run, whether its temperature is asked for alone or among any number of others, and through
 *                       me_mbar_histogram_samples on the same samples in the same order.  The free-energy profile is F(A; T) =
 *                       -T ln(mass / bin width).  Errors otherwise as for me_mbar_reweight.
 *   me_mbar_histogram_samples  the same kernels on host arrays, like me_mbar_reweight_samples; values[n_samples] holds A of
 *                       every sample (pass the energies for an energy histogram).
 *   me_mbar_histogram_gram     me_mbar_histogram with what the asymptotic error bars of its masses need (csrc/
 *                       me_mbar_hist_cov.hip has the definition).  mass, counts and neff_fraction are me_mbar_histogram's, bit
 *                       for bit (the same code).  With K = n_rungs, W_nj = exp(min(f_j - E_n / T_j - d_n, 0)) the ladder column j
 *                       of me_mbar_gram and w_nt the unnormalised weight behind mass[t] (w_nt = exp(min(-E_n / T_t - d_n -
 *                       ln_z_t, 0))), slot_gram is [n][K + 1][n_bins + 3]:
 *                           slot_gram[t][j][s] = sum over the used samples of slot s of W_nj w_nt     (j < K)
 *                           slot_gram[t][K][s] = sum over the used samples of slot s of w_nt^2.
 *                       The weight matrix [K ladder columns | state column w_nt | one column w_nt 1[slot = s] / mass[t][s] per
 *                       slot] has disjoint slot columns, so its whole Gram matrix follows from slot_gram, mass and ladder_gram
 *                       without being formed: ladder_j x slot_s = slot_gram[t][j][s] / mass[t][s], state x slot_s =
 *                       slot_gram[t][K][s] / mass[t][s], slot_s x slot_s = slot_gram[t][K][s] / mass[t][s]^2 (0 between different
 *                       slots), ladder_j x state and state x state the sums of slot_gram[t][j][.] and slot_gram[t][K][.] over the
 *                       slots.  ladder_gram [K][K] and column_counts [K] are the ladder block and the counts of me_mbar_gram
 *                       with n_targets = 0 (that pass itself); *n_used the used samples.  Every output may be NULL.  A slot
 *                       without a sample has slot_gram exactly 0.  No floating-point atomics: all sums have a fixed order, and
 *                       slot_gram[t][j][s] is bit for bit the same run to run, whatever other temperatures are asked for, and
 *                       through me_mbar_histogram_gram_samples on the same samples in the same order.  Arguments are checked
 *                       and errors reported exactly as by me_mbar_histogram.
 *   me_mbar_histogram_gram_samples  the same on host arrays, like me_mbar_histogram_samples.
 *   me_mbar_histogram_joint        the JOINT reweighted histogram of two quantities A (x) and B (y) with the weights of
 *                       me_mbar_histogram (csrc/me_mbar_hist2d.hip has the definition).  column_x, column_y: as
 *                       me_mbar_histogram's column, each a recorded column or -1 for the energy; the same column may be given
 *                       twice (only the diagonal fills).  Each axis has its own edges[n_bins + 1], checked as there, and the
 *                       slot rule of me_mbar_histogram: slot_x in [0, n_bins_x + 3), slot_y in [0, n_bins_y + 3) (bins, below,
 *                       above, NaN).  A used sample falls into exactly one of the (n_bins_x + 3)(n_bins_y + 3) cells, cell =
 *                       slot_x (n_bins_y + 3) + slot_y, and their number must not exceed ME_MAX_HISTOGRAM2D_SLOTS (33 x 33
 *                       bins; ME_ERR_INVALID otherwise).  mass is [n][n_bins_x + 3][n_bins_y + 3], the sum of w per cell divided
 *                       by the total over all cells, so that a temperature's masses sum to 1; counts [n_bins_x + 3][n_bins_y +
 *                       3] the used samples per cell; neff_fraction [n] as me_mbar_reweight's.  Any output may be NULL.  A cell
 *                       without a sample has mass exactly 0.  No floating-point atomics: all sums have a fixed order, and a
 *                       mass is bit for bit the same run to run, whether its temperature is asked for alone or among any number
 *                       of others, and through me_mbar_histogram_joint_samples on the same samples in the same order.  The
 *                       free-energy surface is F(A, B; T) = -T ln(mass / (bin width x) (bin width y)).  Errors as for
 *                       me_mbar_histogram.
 *   me_mbar_histogram_joint_samples  the same kernels on host arrays; values_x[n_samples] and values_y[n_samples] hold A and B of
 *                       every sample.
 *   me_mbar_histogram_joint_gram   me_mbar_histogram_joint with what the asymptotic error bars of its masses need (csrc/
 *                       me_mbar_hist2d_cov.hip has the definition): me_mbar_histogram_gram with "cell" for "slot".  mass, counts
 *                       and neff_fraction are me_mbar_histogram_joint's, bit for bit (the same code).  With K = n_rungs, S =
 *                       (n_bins_x + 3)(n_bins_y + 3), and W_nj, w_nt as in me_mbar_histogram_gram, cell_gram is [n][K + 1][S]:
 *                           cell_gram[t][j][c] = sum over the used samples of cell c of W_nj w_nt     (j < K)
 *                           cell_gram[t][K][c] = sum over the used samples of cell c of w_nt^2.
 *                       The Gram matrix of [K ladder columns | state column | one column per cell] follows from cell_gram,
 *                       mass and ladder_gram as there.  ladder_gram [K][K] and column_counts [K] are the ladder block and the
 *                       counts of me_mbar_gram with n_targets = 0 (that pass itself); *n_used the used samples.  Every output
 *                       may be NULL.  A cell without a sample has cell_gram exactly 0.  No floating-point atomics: all sums have
 *                       a fixed order, and cell_gram[t][j][c] is bit for bit the same run to run, whatever other temperatures
 *                       are asked for, and through me_mbar_histogram_joint_gram_samples on the same samples in the same order.
 *                       Arguments are checked and errors reported exactly as by me_mbar_histogram_joint.
 *   me_mbar_histogram_joint_gram_samples  the same on host arrays, like me_mbar_histogram_joint_samples. */
#define ME_MAX_RECORDED_OBSERVABLES 16
#define ME_MAX_HISTOGRAM_BINS 256
#define ME_MAX_HISTOGRAM2D_SLOTS 1296
int me_observable_samples_enable(me_engine *engine, const int32_t *indices, int32_t n_observables);
int me_observable_samples_info(me_engine *engine, int32_t *n_observables, int32_t *indices);
int me_observable_samples_get(me_engine *engine, int64_t record_begin, int64_t n_records, double *dst);
int me_observable_samples_set(me_engine *engine, int64_t n_records, const double *src);
int me_mbar_reweight_observables(me_engine *engine, const double *f, const double *temps, int32_t n, double *mean, double *var,
                                 double *cov_energy, double *neff_fraction);
int me_mbar_reweight_observables_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                         const double *observables, int32_t n_observables, const double *ladder_temps,
                                         int32_t n_rungs, const double *f, const double *temps, int32_t n, double *mean,
                                         double *var, double *cov_energy, double *neff_fraction);
int me_mbar_reweight_perturbed(me_engine *engine, const double *f, const double *temps, const double *couplings /* [n][Q] */,
                               int32_t n, double *ln_z, double *mean_h, double *var_h, double *mean, double *var, double *cov_h,
                               double *neff_fraction);
int me_mbar_reweight_perturbed_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                       const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps,
                                       const double *couplings, int32_t n, const double *observables, int32_t n_observables,
                                       double *ln_z, double *mean_h, double *var_h, double *mean, double *var, double *cov_h,
                                       double *neff_fraction);
int me_mbar_gram_observables(me_engine *engine, const double *f, const double *temps, int32_t n_targets, double *gram,
                             double *column_counts, double *ln_z, double *mean, double *shifts, int64_t *n_used);
int me_mbar_gram_observables_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                     const double *ladder_temps, int32_t n_rungs, const double *observables, int32_t n_columns,
                                     const double *f, const double *temps, int32_t n_targets, double *gram,
                                     double *column_counts, double *ln_z, double *mean, double *shifts, int64_t *n_used);
int me_mbar_gram_fluctuations(me_engine *engine, const double *f, const double *temps, int32_t n_targets, double *gram,
                              double *column_counts, double *ln_z, double *moments, double *energy_shift, double *shifts,
                              double *mean_e, double *var_e, double *mean, double *var, double *cov_energy, int64_t *n_used);
int me_mbar_gram_fluctuations_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                      const double *ladder_temps, int32_t n_rungs, const double *observables, int32_t n_columns,
                                      const double *f, const double *temps, int32_t n_targets, double *gram,
                                      double *column_counts, double *ln_z, double *moments, double *energy_shift,
                                      double *shifts, double *mean_e, double *var_e, double *mean, double *var,
                                      double *cov_energy, int64_t *n_used);
int me_mbar_histogram(me_engine *engine, const double *f, const double *temps, int32_t n, int32_t column, const double *edges,
                      int32_t n_bins, double *mass, int64_t *counts, double *neff_fraction);
int me_mbar_histogram_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                              const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                              const double *values, const double *edges, int32_t n_bins, double *mass, int64_t *counts,
                              double *neff_fraction);
int me_mbar_histogram_gram(me_engine *engine, const double *f, const double *temps, int32_t n, int32_t column,
                           const double *edges, int32_t n_bins, double *slot_gram, double *ladder_gram, double *column_counts,
                           double *mass, int64_t *counts, double *neff_fraction, int64_t *n_used);
int me_mbar_histogram_gram_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                   const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                                   const double *values, const double *edges, int32_t n_bins, double *slot_gram,
                                   double *ladder_gram, double *column_counts, double *mass, int64_t *counts,
                                   double *neff_fraction, int64_t *n_used);
int me_mbar_histogram_joint(me_engine *engine, const double *f, const double *temps, int32_t n, int32_t column_x,
                        const double *edges_x, int32_t n_bins_x, int32_t column_y, const double *edges_y, int32_t n_bins_y,
                        double *mass, int64_t *counts, double *neff_fraction);
int me_mbar_histogram_joint_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps, int32_t n,
                                const double *values_x, const double *values_y, const double *edges_x, int32_t n_bins_x,
                                const double *edges_y, int32_t n_bins_y, double *mass, int64_t *counts, double *neff_fraction);
int me_mbar_histogram_joint_gram(me_engine *engine, const double *f, const double *temps, int32_t n, int32_t column_x,
                                 const double *edges_x, int32_t n_bins_x, int32_t column_y, const double *edges_y,
                                 int32_t n_bins_y, double *cell_gram, double *ladder_gram, double *column_counts, double *mass,
                                 int64_t *counts, double *neff_fraction, int64_t *n_used);
int me_mbar_histogram_joint_gram_samples(int32_t device_id, const double *energies, const int32_t *rungs, int64_t n_samples,
                                         const double *ladder_temps, int32_t n_rungs, const double *f, const double *temps,
                                         int32_t n, const double *values_x, const double *values_y, const double *edges_x,
                                         int32_t n_bins_x, const double *edges_y, int32_t n_bins_y, double *cell_gram,
                                         double *ladder_gram, double *column_counts, double *mass, int64_t *counts,
                                         double *neff_fraction, int64_t *n_used);

/* Statistical inefficiencies of the recorded series, pooled over the chains of a rung (no reference counterpart; csrc/
 * me_series.hip has the definition): the multiple-series estimator of Chodera et al., JCTC 3:26 (2007), the number the
 * `inefficiency` of every MBAR error bar asks for.  A slot keeps its rung whatever configuration was swapped into it, so the
 * records of slot c are a stationary series at the temperature of rung c / M.  For one column (column 0: the energy; column 1 +
 * q: recorded observable q) and one rung with R records of each of its M chains, a chain is USED when all R of its values in the
 * column are finite; over the M_u used chains, with d = a - mean:
 *     mean = sum_c sum_n a_c[n] / (M_u R)              P(t) = sum_c sum_{n = 0}^{R - t - 1} d_c[n] d_c[n + t]
 *     var  = P(0) / (M_u R)                            C(t) = P(t) R / (P(0) (R - t))
 *     g    = max(1, 1 + 2 sum_{t = 1}^{stop - 1} C(t) (1 - t / R))
 * with stop the first t > mintime at which C(t) <= 0, or max_lag + 1 when there is none up to max_lag (terms C(t) <= 0 at t <=
 * mintime are added): for one chain this is metropolisengine_amd.statistics.statistical_inefficiency with fast=False.
 *   me_recorded_inefficiency   over the engine's stores: K = the ladder's rungs and M = n_chains / K, or K = 1 and M = n_chains on
 *                       an engine without a ladder; Q = the recorded observable columns.  mintime >= 0; max_lag in [1, R - 2],
 *                       or 0 for R - 2 (ME_ERR_INVALID otherwise).  Outputs, each [1 + Q][K] and each may be NULL: g, mean, var,
 *                       stop_lag, chains_used (M_u); acf is [1 + Q][K][max_lag + 1] with acf[t] = C(t) for t <= min(stop,
 *                       max_lag) and NaN beyond.  A (column, rung) without a used chain (mean and var NaN as well) or with P(0) =
 *                       0 reports g = NaN, stop_lag = 0 and acf NaN; the call still succeeds.  The lags are computed 64 at a
 *                       time and the call ends with the batch in which the last walk stops; no result depends on that.  No
 *                       floating-point atomics: every sum has a fixed order that depends on (R, M) alone, so a call is bitwise
 *                       reproducible, a smaller max_lag gives the bitwise prefix, and a non-finite value changes nothing but its
 *                       own (column, rung).  ME_ERR_STATE without an energy store or with fewer than 3 records.
 *   me_series_inefficiency_samples   the same kernels on a host array series[n_records][n_series], one column: the groups are
 *                       consecutive runs of group_chains series, group_chains a multiple of 64 that divides n_series
 *                       (ME_ERR_INVALID otherwise, and for n_records < 3); outputs [n_series / group_chains] and acf
 *                       [n_series / group_chains][max_lag + 1].  Bit for bit me_recorded_inefficiency on the same values. */
int me_recorded_inefficiency(me_engine *engine, int32_t mintime, int32_t max_lag, double *g, double *mean, double *var,
                             int32_t *stop_lag, int64_t *chains_used, double *acf);
int me_series_inefficiency_samples(int32_t device_id, const double *series, int64_t n_records, int64_t n_series,
                                   int64_t group_chains, int32_t mintime, int32_t max_lag, double *g, double *mean, double *var,
                                   int32_t *stop_lag, int64_t *chains_used, double *acf);

/* Text of the last error on this engine (or of the last failed me_create when engine is NULL). */
int me_last_error(me_engine *engine, char *buf, size_t buf_bytes);

/* Capability query: 1 if a kernel set for this combination is compiled in. */
int me_supported(int32_t dtype, int32_t n_real, int32_t n_complex, int32_t energy_kind);

/* Equilibration detection for a batch of recorded series (host arrays in, host arrays out; engine-independent):
 * for each of the n_series rows of series[n_series][length] the production start t0 that maximises the number of
 * effectively uncorrelated samples (length - t0 + 1) / g(t0), with g the statistical inefficiency of the tail.
 * Replaces the per-column pymbar.timeseries.detectEquilibration calls of statistics.py:25-48 /
 * metropolis_engine.py:481-504 (PARITY UNPINNED: pymbar is absent; this follows the published algorithm exactly as
 * metropolisengine_amd/statistics.py restates it).  fast != 0: lag increments grow by one (pymbar's fast=True);
 * nskip: stride of the candidate starts.  Constant series report (0, 1, 1). */
int me_detect_equilibration(int32_t device_id, const double *series, int64_t n_series, int64_t length, int32_t fast,
                            int32_t nskip, int64_t *t0, double *g, double *neff_max);

#ifdef __cplusplus
}
#endif
#endif /* METROPOLIS_ENGINE_H */
