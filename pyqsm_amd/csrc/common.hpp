// common.hpp — per-device context (stream, scratch arena, event timers) and
// error plumbing shared by every translation unit of libpyqsm_hip.so.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pyqsm_hip.h"

namespace pyqsm {

void set_error(const char* fmt, ...);

// Host buffers the library hands to its caller (released with pyqsm_free). Buffers of a
// megabyte or more come page-locked from a small pool (context.hip): the device-to-host copy
// into them, and the host-to-device copy when the caller passes them back (the Laplacian goes
// straight into the contraction solve), run at link speed instead of through the driver's
// staging of pageable memory. Falls back to malloc; nullptr when that fails too.
void* out_alloc(size_t bytes);
void out_free(void* p);
int fail(int code, const char* fmt, ...);

#define PQ_HIP(expr)                                                                   \
  do {                                                                                 \
    hipError_t e__ = (expr);                                                           \
    if (e__ != hipSuccess)                                                             \
      return ::pyqsm::fail(e__ == hipErrorOutOfMemory ? PYQSM_ENOMEM : PYQSM_EHIP,     \
                           "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),     \
                           __FILE__, __LINE__);                                        \
  } while (0)

#define PQ_TRY(expr)         \
  do {                       \
    int r__ = (expr);        \
    if (r__ != 0) return r__; \
  } while (0)

// Grow-only scratch memory. alloc() bumps inside the current chunk and adds a
// chunk when it runs out; reset() folds several chunks into one of the summed
// size so that a repeated call of the same shape allocates nothing.
class Arena {
 public:
  int alloc(size_t bytes, void** out);
  template <typename T>
  int get(size_t count, T** out) {
    return alloc(count * sizeof(T), reinterpret_cast<void**>(out));
  }
  int reset();
  void destroy();
  // Position of the allocator; rewind(mark) releases everything allocated after mark() (chunks
  // added meanwhile stay and are reused). For long calls that loop over large temporaries.
  struct Mark {
    size_t chunk, used;
  };
  Mark mark() const;
  void rewind(const Mark& m);

 private:
  struct Chunk {
    char* base;
    size_t size;
    size_t used;
  };
  std::vector<Chunk> chunks_;
  size_t cur_ = 0;  // chunk allocations currently come from
};

// A stamped interval: from the earliest block start of launch `first` to the latest block end of
// launch `last` (indices into Ctx::stamp_launches); first < 0: a scope without a stamped launch.
struct StampRec {
  int first, last;
};

struct Timer {
  double ms = 0.0;
  int64_t launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<int> weights;  // launches represented by each pending pair
  std::vector<StampRec> stamped;  // one launch each
};

// Where a stamped launch's slots lie: chunk of Ctx::stamp_chunks, first slot, blocks.
struct StampLaunch {
  int chunk;
  size_t off;
  int nblk;
};

// The launch shapes a device-planned DBSCAN call is enqueued with (grid.hpp GridPlan): the exact plan
// of the last host-planned call with some headroom. The bounding box's fold sets the plan's ok only
// when the exact plan fits them — ncell and nbk no larger, bits = 12, the same side of the fused-scan
// threshold — and needs no axis compression, no doubled cell and fp32 records, on finite
// coordinates. valid == 0: no hint, ok stays 0. It decides which path runs, never what it computes.
struct PlanHint {
  int valid = 0;
  int ncell = 0, nbk = 0, fused = 0;
};

struct Ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  Arena arena;
  std::mutex mu;  // calls on one device serialise
  int prof = 0;  // 0 off, 1 phase timers, 2 also single kernels inside the solver loops
  std::map<std::string, Timer> timers;
  std::vector<hipEvent_t> event_pool;
  int cu_count = 256;
  // DBSCAN's grid plan: page-locked [read-back, upload] slots, the timing-disabled event the host
  // waits on for the read-back, and the hint of the last host-planned call (dbscan.hip)
  void* plan_pinned = nullptr;
  unsigned plan_seq = 0;  // the sequence number of the last plan the fold was asked to write
  PlanHint plan_hint;
  // device-clock stamps of the profiled launches since the last drain (stamp_slots): grow-only
  // chunks of device memory, two u64 slots per block
  struct StampChunk {
    unsigned long long* base;
    size_t size, used;  // in slots
  };
  std::vector<StampChunk> stamp_chunks;
  std::vector<StampLaunch> stamp_launches;
  int stamp_khz = 100000;  // the constant clock's rate
};

// Returns the context for `device`, creating it on first use. nullptr + error
// message when the device does not exist.
Ctx* ctx_for(int device);

// Typed copies on the context's stream: the element type is the device pointer's, the host pointer
// has to convert to it, and the byte count follows from it. A count of zero enqueues nothing, so
// (nullptr, 0) is a valid host side.
template <typename T>
struct Elem {
  using type = T;
};
template <typename T>
int copy_in(Ctx* c, T* d, const typename Elem<T>::type* h, size_t count) {
  if (count) PQ_HIP(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return 0;
}
template <typename T>
int download(Ctx* c, typename Elem<T>::type* h, const T* d, size_t count) {
  if (count) PQ_HIP(hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  return 0;
}
inline int stream_sync(Ctx* c) {
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}
// arena scratch of `count` elements filled from the host
template <typename T>
int upload(Ctx* c, const typename Elem<T>::type* h, size_t count, T** d) {
  PQ_TRY(c->arena.get(count, d));
  return copy_in(c, *d, h, count);
}
// download, then wait for it: the read-back of a count that sizes what comes next
template <typename T>
int fetch(Ctx* c, typename Elem<T>::type* h, const T* d, size_t count = 1) {
  PQ_TRY(download(c, h, d, count));
  return stream_sync(c);
}

// One C-ABI call on a device: holds the context's lock for its lifetime and, unless told to keep
// it, resets the scratch arena, so the arena is only ever touched under the lock. c == nullptr
// (device form only): ctx_for failed and has set the message; the caller returns PYQSM_ENODEV.
// The Ctx* form is for entry points that return early between ctx_for and the lock.
class Call {
 public:
  enum ArenaUse { kResetArena, kKeepArena };  // kKeepArena: for a call that takes no scratch
  explicit Call(int device, ArenaUse use = kResetArena) : Call(ctx_for(device), use) {}
  explicit Call(Ctx* ctx, ArenaUse use = kResetArena) : c(ctx) {
    if (!c) return;
    lk_ = std::unique_lock<std::mutex>(c->mu);
    if (use == kResetArena) c->arena.reset();
  }
  Ctx* const c;

 private:
  std::unique_lock<std::mutex> lk_;
};

// Host buffers handed to the caller (released by the caller with pyqsm_free): released again here
// unless `kept` is set, which an entry point does in one place, at the end, where it writes the
// caller's out-pointers.
struct OutBufs {
  std::vector<void*> p;
  bool kept = false;
  OutBufs() = default;
  OutBufs(const OutBufs&) = delete;
  OutBufs& operator=(const OutBufs&) = delete;
  ~OutBufs() {
    if (!kept)
      for (void* q : p) out_free(q);
  }
  template <typename T>
  T* get(size_t count) {
    void* q = out_alloc((count ? count : 1) * sizeof(T));
    if (q) p.push_back(q);
    return static_cast<T*>(q);
  }
};

// RAII bracket: records a start/stop event pair on the stream under `name`
// when profiling is enabled and `name` is not null; otherwise does nothing.
class ProfScope {
 public:
  ProfScope(Ctx* c, const char* name, int weight = 1, int level = 1);
  ~ProfScope();

 private:
  Ctx* c_;
  Timer* t_ = nullptr;
  hipEvent_t start_ = nullptr;
};

// The same for a scope of exactly one kernel: the pair of events (null when profiling is off) is
// handed to hipExtLaunchKernelGGL, which records them with the kernel's own dispatch instead of
// as two markers of their own on the stream.
class ProfKernel {
 public:
  ProfKernel(Ctx* c, const char* name);
  hipEvent_t start = nullptr, stop = nullptr;
};

// Device-clock timing of a profiled step without events between its kernels (DBSCAN). A stamped
// kernel takes the pointer stamp_slots() returns (null when profiling is off) and runs its body
// through stamped(): every block writes its start and the end of its last wave to its own two
// slots, on the 100 MHz constant clock. drain_timers reduces them on the host. The stamps time
// the blocks' work only: the dispatch gaps between kernels are not in them.
// Slots for one launch of `nblk` blocks, registered as the context's next stamped launch; nullptr
// when profiling is below `level` or the slots cannot be allocated.
unsigned long long* stamp_slots(Ctx* c, int64_t nblk, int level = 1);
// A single-block kernel that only stamps: the start or the end of a scope whose first or last
// kernel is not stamped (rare paths). Does nothing when profiling is off.
int stamp_mark(Ctx* c);

// The scope of a phase: from the first stamped launch enqueued while it is open to the last one.
class StampScope {
 public:
  StampScope(Ctx* c, const char* name, int level = 1);
  ~StampScope();

 private:
  Ctx* c_;
  Timer* t_ = nullptr;
  int first_ = 0;
};

// The slots of one stamped kernel launch of `nblk` blocks, timed under `name` on its own.
class StampKernel {
 public:
  StampKernel(Ctx* c, const char* name, int64_t nblk);
  unsigned long long* slots = nullptr;
};

// Runs `body` (the kernel's code; a `return` in it leaves the body) between the block's stamps.
// One barrier before the body and one LDS atomic per wave after it, only when st != nullptr.
template <typename F>
__device__ __forceinline__ void stamped(unsigned long long* __restrict__ st, F&& body) {
  __shared__ int done;
  if (st) {  // kernel-uniform
    if (threadIdx.x == 0) {
      done = 0;
      st[2 * size_t(blockIdx.x)] = wall_clock64();
    }
    __syncthreads();
  }
  body();
  if (st && (threadIdx.x & 63) == 0) {  // every wave, all of its lanes back
    if (atomicAdd(&done, 1) == int((blockDim.x + 63) / 64) - 1) st[2 * size_t(blockIdx.x) + 1] = wall_clock64();
  }
}

// roctx range around a C-ABI entry point (tracing): shows up in
// `rocprofv3 --marker-trace`. librocprofiler-sdk-roctx is looked up once at run time;
// without it (or without a tool attached) a range costs two indirect calls.
class ApiRange {
 public:
  explicit ApiRange(const char* name);
  ~ApiRange();

 private:
  bool on_;
};
#define PQ_API_RANGE(name) ::pyqsm::ApiRange api_range__(name)

// Destroys the RCCL communicators (multi.hip); called by pyqsm_shutdown.
void comm_shutdown();

inline int ceil_div(int64_t a, int64_t b) { return static_cast<int>((a + b - 1) / b); }

// Device-resident pieces other translation units chain (skeleton.hip runs the whole contraction
// loop in HBM): kNN, the point-cloud Laplacian, the contraction solve.
struct LapOut {  // all pointers into the context arena
  int32_t *indptr, *indices;
  double *vals, *mass;
  int32_t nnz;
};
int laplacian_device(Ctx* c, const double* d_xyz, int64_t n, const int64_t* seg_start /*host, may be null*/,
                     int64_t n_seg, int32_t k, double moll, LapOut* out);

// Exclusive prefix sum of n int32 values, in place, on the stream (scan.hip).
int exclusive_scan_i32(Ctx* c, int32_t* data, int64_t n);

// Selects the flagged rows (scan.hip). flags [n + 1], written by the caller's predicate kernel,
// flags[n] == 0: scanned in place, so the count is left in flags[n] (on the device). For every
// flagged i, in ascending order, writes idx[p] = src_idx ? src_idx[i] : i and copies row i of
// a / b ([n,3] f64) to row p of out_a / out_b. idx, a / out_a and b / out_b may be null.
// Enqueues only: no read-back, no synchronisation.
int compact_flagged(Ctx* c, int32_t* flags, int64_t n, int64_t* idx, const int64_t* src_idx = nullptr,
                    const double* a = nullptr, double* out_a = nullptr, const double* b = nullptr,
                    double* out_b = nullptr);

// Stable sort of n (key, value) pairs by the low `bits` bits of the key (scan.hip: radix passes
// without global atomics, so the order is reproducible). *keys / *vals are the inputs and, on
// return, point at the sorted arrays (the inputs themselves or arena buffers of the same size).
int stable_sort_pairs_u32(Ctx* c, uint32_t** keys, int32_t** vals, int64_t n, int bits);

// *perm [n] (null: the identity) refined by a stable sort on the low `bits` bits of key_src[perm[i]]
// (scan.hip); on return *perm is an arena array. Rows are ordered by several keys by calling this once
// per key, least significant key first.
int refine_order_by_key(Ctx* c, int64_t n, const int32_t* key_src, int32_t** perm, int bits);
// The bits needed to write v: 0 for 0, 3 for 4 to 7.
int bit_length(uint64_t v);

}  // namespace pyqsm
