// The engine behind the C ABI and what the host units share: the owning resource types, me_engine, the error helpers.
// Private to the host side (me_api.hip and the entry points that live next to their kernels in me_replica.hip,
// me_population.hip, me_mbar.hip, me_statistics.hip): not installed, and not included by me_kernels.hip or by plugins.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "me_comm.h"
#include "me_internal.h"

// nothing declared here belongs to the library's dynamic symbol table
#pragma GCC visibility push(hidden)

namespace me {

// ------------------------------------------------------------------------------------------------ owning types
// Move-only owners, one per kind of resource.  They free on destruction and on reset(); they never wait: a caller that
// lets go of memory a launch in flight may touch synchronises the stream first, in its own code.

// device memory (hipMalloc / hipFree) that knows its size
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer &&o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    if (this != &o) {
      reset();
      ptr_ = std::exchange(o.ptr_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~DeviceBuffer() { reset(); }
  void reset() {
    if (ptr_) (void)hipFree(ptr_);
    ptr_ = nullptr;
    bytes_ = 0;
  }
  // hold exactly `bytes` (nothing happens when it does already; otherwise the contents are lost, also on failure)
  hipError_t resize(size_t bytes) {
    if (bytes == bytes_) return hipSuccess;
    reset();
    if (bytes == 0) return hipSuccess;
    const hipError_t err = hipMalloc(&ptr_, bytes);
    if (err == hipSuccess) bytes_ = bytes;
    else ptr_ = nullptr;
    return err;
  }
  // hold at least `bytes`
  hipError_t reserve(size_t bytes) { return bytes <= bytes_ ? hipSuccess : resize(bytes); }
  template <typename T = void>
  T *get() const { return static_cast<T *>(ptr_); }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return ptr_ != nullptr; }

 private:
  void *ptr_ = nullptr;
  size_t bytes_ = 0;
};

// pinned host memory (hipHostMalloc / hipHostFree)
class PinnedBuffer {
 public:
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer &) = delete;
  PinnedBuffer &operator=(const PinnedBuffer &) = delete;
  ~PinnedBuffer() { reset(); }
  void reset() {
    if (ptr_) (void)hipHostFree(ptr_);
    ptr_ = nullptr;
  }
  hipError_t allocate(size_t bytes) {     // what it held before goes
    reset();
    return hipHostMalloc(&ptr_, bytes, hipHostMallocDefault);
  }
  template <typename T>
  T *get() const { return static_cast<T *>(ptr_); }

 private:
  void *ptr_ = nullptr;
};

// a stream the engine created, or one it was lent (me_set_stream) and must not destroy
class Stream {
 public:
  Stream() = default;
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  ~Stream() { lend(nullptr); }
  hipError_t create() {     // what it held before goes, as in lend()
    lend(nullptr);
    const hipError_t err = hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking);
    owned_ = err == hipSuccess;
    return err;
  }
  // from now on the caller's stream; one the engine created goes (the caller has waited for it)
  void lend(hipStream_t theirs) {
    if (owned_ && stream_) (void)hipStreamDestroy(stream_);
    stream_ = theirs;
    owned_ = false;
  }
  operator hipStream_t() const { return stream_; }

 private:
  hipStream_t stream_ = nullptr;
  bool owned_ = false;
};

class Event {
 public:
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() { reset(); }
  void reset() {
    if (event_) (void)hipEventDestroy(event_);
    event_ = nullptr;
  }
  hipError_t create(unsigned flags = hipEventDefault) {     // one it held before goes
    reset();
    return hipEventCreateWithFlags(&event_, flags);
  }
  operator hipEvent_t() const { return event_; }

 private:
  hipEvent_t event_ = nullptr;
};

}  // namespace me

// ------------------------------------------------------------------------------------------------ the engine
struct me_engine {
  int device = 0;
  me::Stream stream;                 // declared before everything enqueued on it: destroyed last
  const me::KernelSet *ks = nullptr;
  int dtype = ME_F32;
  size_t esize = 4;
  long long n = 0;
  int nr = 0, nc = 0, d = 0, p = 0, nobs = 0;
  unsigned long long chain_offset = 0, seed = 0;
  double temp = 0, target_acceptance = 0.3, alpha = 0, ratio = 0, reject_bound = 0;
  int m = 0, energy_kind = 0, reject_kind = 0, cov_mode = 0;
  bool stale_total = false;          // ME_FLAG_REFERENCE_ENERGY_LEDGERS on a mixed engine: ledger row n_terms = energy_total
  me::Event time_start, time_stop;   // me_time_steps
  std::vector<double> shared_host;   // the packed factor last given to me_set_shared_factor (empty: none); checkpoints
  int cov_kind = me::CK_IDENTITY;
  int grid_blocks = 0;
  int n_terms = 1;   // rows of the energy ledger (KernelSet::energy_terms)
  std::vector<double> coef;
  unsigned long long step_index = 0, measure_count = 1;   // counters start at 1 (metropolis_engine.py:72-75)
  unsigned long long fused_cycles = 0;                    // me_cycle calls that ran as ONE launch (k_cycle)
  // device buffers (SoA: component-major, chain-minor)
  me::DeviceBuffer x, energy, width, mean, cov, obs_mean;
  me::DeviceBuffer factor, shared_factor, shared_full, shared_image, energy_image, coef_dev, row_dev;
  me::DeviceBuffer accept_slots, accept_total;            // unsigned long long
  long long n_slots = 0;
  unsigned long long proposed = 0;
  bool x_tiled = false;         // the state field is tile-major (KernelSet::tiled_state)
  int width_rows = 1;           // 3 for mixed engines: [sampling_width, real group, complex group]
  bool widths_synced = true;    // mixed engines: rows 1, 2 are implied equal to row 0 (state after a step_all)
  me::DeviceBuffer status;      // unsigned int
  me::PinnedBuffer host_scratch;   // unsigned long long: [0] status bits, [1] accepted total
  // pooled moments; the split reduction (me_pooled_moments_begin/_end) has a second stream for the copy and two events
  struct Pool {
    me::DeviceBuffer dev, partials;
    me::PinnedBuffer host;
    me::DeviceBuffer range_x;    // me_pooled_moments_range: the range's rows of a component-major x
    me::Stream copy_stream;
    me::Event reduced, copied;
    bool pending = false;
  } pool;
  // RCCL communicator of this engine's rank (me_comm_init_rank); null = single-GPU engine
  const me::RcclApi *rccl = nullptr;
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  // time-series trace of a few chains (the reference's per-measure appends, :350-356)
  struct Trace {
    me::DeviceBuffer dev;        // double
    long long chains = 0, stride = 1, rows = 0, capacity = 0;
    void restart() {             // (the caller has waited for the stream)
      dev.reset();
      rows = capacity = 0;
    }
  } trace;
  // temperature ladder (me_set_temperature_ladder, me_replica.hip): n_rungs = 0 is the scalar temp
  struct Ladder {
    int n_rungs = 0;
    std::vector<double> temps;
    me::DeviceBuffer table;         // (inv_temp, inv_temp_log2e) per rung, device dtype
    me::DeviceBuffer pair_counts;   // unsigned long long: [2 k] attempted, [2 k + 1] accepted swaps of the rung pair (k, k+1)
    unsigned long long round = 0;
  } ladder;
  // population annealing (me_population.hip); allocated at the first stage or family restore
  struct Population {
    me::DeviceBuffer fam, fam_out;   // long long: family ids (start as the global chain ids), gather scratch
    me::DeviceBuffer x, energy;      // gather scratch of x and the ledger
    me::DeviceBuffer anc;            // unsigned int: ancestor of every slot
    me::DeviceBuffer scratch;        // double: block partials, factors, offsets, stage parameters
    me::DeviceBuffer records;        // double: (log_weight, neff_fraction, n_finite) per stage
    unsigned long long stages = 0, capacity = 0;
    std::vector<double> temps;       // T_new of every stage
  } population;
  // recorded energy samples (me_energy_samples_*, me_mbar.hip): float64 [capacity][n], `rows` of them filled; and the
  // observables recorded with them (me_observable_samples_*, me_mbar_obs.hip): float64 [capacity][n_obs][n], the same `rows`
  struct Samples {
    me::DeviceBuffer data;
    long long capacity = 0, rows = 0;
    me::DeviceBuffer obs;
    int n_obs = 0;                                      // 0: no observable store
    int obs_index[ME_MAX_RECORDED_OBSERVABLES] = {};    // catalogue indices of the recorded columns
  } samples;
  std::string err;

  // The teardown of me_destroy (which has waited for both streams) and of a failed me_create.  What has an order is spelled
  // out: the device first; the communicator before the members, the streams among them, go in reverse order of declaration.
  ~me_engine() {
    (void)hipSetDevice(device);
    if (comm && rccl) (void)rccl->comm_destroy(comm);
  }
};

// ------------------------------------------------------------------------------------------------ shared helpers
namespace me {

// records the message (e = nullptr: for the calling thread, me_last_error(NULL)) and returns `code`
int fail(me_engine *e, int code, const std::string &msg);

#define ME_HIP(e, call)                                                                                      \
  do {                                                                                                       \
    hipError_t err__ = (call);                                                                               \
    if (err__ != hipSuccess)                                                                                 \
      return me::fail((e), ME_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(err__));                \
  } while (0)

// Surface per-chain failure flags (the analogue of the reference's exceptions) and clear them; waits for the stream.
int check_status(me_engine *e);

// `count` host doubles in the device dtype into `dst`, which then holds exactly them (synchronous copy)
hipError_t upload(DeviceBuffer &dst, const double *src, size_t count, int dtype);

// ME_FLAG_REFERENCE_ENERGY_LEDGERS keeps two ledgers: what needs THE energy of a chain refuses (`subject`: "energy samples are")
int refuse_stale_total(me_engine *e, const char *subject);

// chains padded to whole 64-chain tiles (the extent of the tile-major fields)
inline long long padded_chains(long long n) { return (n + 63) / 64 * 64; }

}  // namespace me

#pragma GCC visibility pop
