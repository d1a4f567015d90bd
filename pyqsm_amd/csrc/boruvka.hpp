// boruvka.hpp — the spanning forest of a kNN graph by Boruvka rounds, once, for the normal orientation
// (normals.hip) and the skeleton forest (topology.hip). dbscan.hip and mesh.hip keep their own
// union-finds (unionfind.hpp says why).
//
// The callers differ only in what an edge is and what a hook records; an edge policy says both:
//   void init(int i)                                  once per point, before the first round
//   bool ends(int64_t e, int* i, int* j)              entry e of the kNN table is an edge; its ends
//   unsigned long long key(int64_t e, int i, int j)   its 64-bit weight, lower is lighter (ord_bits)
//   uint32_t flip(int a, int b)                       the parity bit that the chosen edge {a, b} carries
//   void hooked(uint32_t c, unsigned long long pk, unsigned long long key)
//                                                     root c has just hooked along pk with that weight
// It is a small trivially-copyable struct passed to the kernels by value, as on_coords passes `co`.
//
// Labels. lab[i] = root << 1 | parity of i relative to its root (n < 2^31, so the root fits); a
// caller whose flip() is always 0 reads lab[i] >> 1 and ignores the bit.
//
// The order on edges is (key, packed (min, max)): strict and total, two different pairs never compare
// equal. So every component has ONE lightest cross edge and the forest is unique, whatever order the
// atomics arrive in. The pair does not fit beside the 64 key bits in one word, hence two phases of
// 64-bit atomicMin per round: the key (k_bv_min_w), then the packed pair among the edges of that
// key (k_bv_min_e). An edge proposes itself to both of its components, so a mutual pair of
// components has picked the same edge; its lower id stays a root. Hook cycles longer than two
// cannot form: walking from a component along its chosen edge to the next component and on, the
// chosen (key, pair) falls strictly except where two components chose the same edge. (With weights
// alone three components at equal weights could hook in a ring, and pointer jumping on a ring never
// ends.)
//
// The hook word hk[c] = ancestor << 1 | parity of c relative to it is ONE 32-bit word, read and written
// during the jumps with single agent-scope relaxed atomics: a reader never sees an ancestor with another
// entry's parity. Only root c itself writes hk[c], and it stores only when it moves to a farther
// ancestor. A stale read is therefore still an ancestor with the parity that belongs to it: the walk
// gets longer, never wrong. The minima likewise only fall, so "skip the atomic when the value read is
// already no higher" is safe on a stale read, which is no lower than the true value.
//
// No device loop is unbounded: a thread jumps at most kBvJumps times per launch and then raises the
// jump-again flag; the host relaunches at most kBvMaxRelaunch times (every launch advances every
// unfinished root by at least one ancestor) and runs at most kBvMaxRounds rounds. Beyond a cap:
// PYQSM_EHIP. Integer atomics only.
#pragma once
#include "common.hpp"

namespace pyqsm {

static constexpr int kBvMaxRounds = 32;    // components at least halve per round: 2^31 points need 31
static constexpr int kBvJumps = 64;        // pointer jumps per thread per launch
static constexpr int kBvMaxRelaunch = 64;  // launches of the jump kernel per round
// control words, one 16-byte block: hooks of the round, "jump again" flag
enum { kBvHooks = 0, kBvAgain = 1, kBvCtlWords = 4 };

// A double's bits mapped so that unsigned order is numeric order (negative values included), and back.
__device__ __forceinline__ unsigned long long ord_bits(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_ord(unsigned long long o) {
  const unsigned long long u = (o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFull) : ~o;
  return __longlong_as_double((long long)u);
}

// All six kernels are templates on the policy, k_bv_jump and k_bv_relabel too, which do not ask it: a
// translation unit that wants ord_bits alone then emits none of them.
template <class P>
__global__ __launch_bounds__(256) void k_bv_init(int n, P pol, uint32_t* __restrict__ lab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  lab[i] = uint32_t(i) << 1;
  pol.init(i);
}

// Entry e of the kNN table as a cross edge: an edge of the policy with its ends in two components.
// The key is computed for those only.
template <class P>
__device__ __forceinline__ bool bv_cross_edge(const P& pol, int64_t e, const uint32_t* __restrict__ lab, int* i, int* j,
                                              uint32_t* ci, uint32_t* cj, unsigned long long* key) {
  if (!pol.ends(e, i, j)) return false;
  *ci = lab[*i] >> 1;
  *cj = lab[*j] >> 1;
  if (*ci == *cj) return false;
  *key = pol.key(e, *i, *j);
  return true;
}

// Phase 1: the smallest key among the cross edges of every component.
template <class P>
__global__ __launch_bounds__(256) void k_bv_min_w(int64_t ne, P pol, const uint32_t* __restrict__ lab,
                                                  unsigned long long* __restrict__ bw) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= ne) return;
  int i, j;
  uint32_t ci, cj;
  unsigned long long key;
  if (!bv_cross_edge(pol, e, lab, &i, &j, &ci, &cj, &key)) return;
  // an edge no lighter than what is already there cannot change the minimum: spare the atomic
  if (key < bw[ci]) atomicMin(&bw[ci], key);
  if (key < bw[cj]) atomicMin(&bw[cj], key);
}

// Phase 2: among the edges of that key, the smallest packed (min, max).
template <class P>
__global__ __launch_bounds__(256) void k_bv_min_e(int64_t ne, P pol, const uint32_t* __restrict__ lab,
                                                  const unsigned long long* __restrict__ bw,
                                                  unsigned long long* __restrict__ be) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= ne) return;
  int i, j;
  uint32_t ci, cj;
  unsigned long long key;
  if (!bv_cross_edge(pol, e, lab, &i, &j, &ci, &cj, &key)) return;
  const unsigned long long pk = (i < j) ? ((unsigned long long)i << 32 | uint32_t(j))
                                        : ((unsigned long long)j << 32 | uint32_t(i));
  if (key == bw[ci]) atomicMin(&be[ci], pk);
  if (key == bw[cj]) atomicMin(&be[cj], pk);
}

// Every root with an edge hooks to the component across it: hk[c] = other << 1 | parity of c
// relative to other. A mutual pair has chosen the same edge; its lower id stays a root.
template <class P>
__global__ __launch_bounds__(256) void k_bv_hook(int n, P pol, const uint32_t* __restrict__ lab,
                                                 const unsigned long long* __restrict__ bw,
                                                 const unsigned long long* __restrict__ be, uint32_t* __restrict__ hk,
                                                 int32_t* __restrict__ ctl) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  if ((lab[c] >> 1) != uint32_t(c)) return;
  const unsigned long long pk = be[c];
  hk[c] = uint32_t(c) << 1;
  if (pk == ~0ull) return;
  const int a = int(pk >> 32), b = int(pk & 0xFFFFFFFFu);
  const uint32_t la = lab[a], lb = lab[b];
  const uint32_t ca = la >> 1, cb = lb >> 1;
  const uint32_t other = ca == uint32_t(c) ? cb : ca;
  if (be[other] == pk && uint32_t(c) < other) return;
  hk[c] = (other << 1) | ((la ^ lb ^ pol.flip(a, b)) & 1u);
  pol.hooked(uint32_t(c), pk, bw[c]);
  atomicAdd(&ctl[kBvHooks], 1);
}

// Pointer jumping on the hook forest, in place: an entry always names an ancestor with the parity
// relative to it, so concurrent jumps by other roots only shorten the walk. A thread that has not
// reached a child of a root after kBvJumps jumps asks for another launch.
template <class P>
__global__ __launch_bounds__(256) void k_bv_jump(int n, const uint32_t* __restrict__ lab, uint32_t* hk,
                                                 int32_t* __restrict__ ctl) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  if ((lab[c] >> 1) != uint32_t(c)) return;
  for (int t = 0; t < kBvJumps; ++t) {
    const uint32_t h = __hip_atomic_load(&hk[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t p = h >> 1;
    if (p == uint32_t(c)) return;
    const uint32_t hp = __hip_atomic_load(&hk[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((hp >> 1) == p) return;
    __hip_atomic_store(&hk[c], (hp & ~1u) | ((h ^ hp) & 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  ctl[kBvAgain] = 1;
}

template <class P>
__global__ __launch_bounds__(256) void k_bv_relabel(int n, uint32_t* __restrict__ lab, const uint32_t* __restrict__ hk) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = lab[i];
  const uint32_t h = hk[l >> 1];
  lab[i] = (h & ~1u) | ((l ^ h) & 1u);
}

// Profiling scopes inside a round; null: none.
struct BvScopes {
  const char *min_edge, *hook, *jump;
};

// Boruvka over the ne directed entries of the kNN table of n points until no component has a cross
// edge left. lab, hk [n], bw, be [n], ctl [kBvCtlWords]: the caller's arena allocations; lab comes
// out as described above. *rounds: the rounds that hooked at least one component. `what` names the
// caller in the messages.
template <class P>
static int boruvka_forest(Ctx* c, const char* what, int64_t n, int64_t ne, P pol, BvScopes sc, uint32_t* lab,
                          uint32_t* hk, unsigned long long* bw, unsigned long long* be, int32_t* ctl,
                          int32_t* rounds) {
  *rounds = 0;
  const int N = int(n), eb = ceil_div(ne, 256), pb = ceil_div(n, 256);
  int32_t h[kBvCtlWords];
  hipLaunchKernelGGL(k_bv_init<P>, dim3(pb), dim3(256), 0, c->stream, N, pol, lab);
  PQ_HIP(hipGetLastError());
  for (int round = 0;; ++round) {
    {
      ProfScope ps(c, sc.min_edge);
      PQ_HIP(hipMemsetAsync(bw, 0xFF, size_t(n) * 8, c->stream));
      PQ_HIP(hipMemsetAsync(be, 0xFF, size_t(n) * 8, c->stream));
      PQ_HIP(hipMemsetAsync(ctl, 0, kBvCtlWords * 4, c->stream));
      hipLaunchKernelGGL(k_bv_min_w<P>, dim3(eb), dim3(256), 0, c->stream, ne, pol, static_cast<const uint32_t*>(lab),
                         bw);
      hipLaunchKernelGGL(k_bv_min_e<P>, dim3(eb), dim3(256), 0, c->stream, ne, pol, static_cast<const uint32_t*>(lab),
                         static_cast<const unsigned long long*>(bw), be);
      PQ_HIP(hipGetLastError());
    }
    {
      ProfScope ps(c, sc.hook);
      hipLaunchKernelGGL(k_bv_hook<P>, dim3(pb), dim3(256), 0, c->stream, N, pol, static_cast<const uint32_t*>(lab),
                         static_cast<const unsigned long long*>(bw), static_cast<const unsigned long long*>(be), hk,
                         ctl);
      PQ_HIP(hipGetLastError());
      PQ_TRY(fetch(c, h, ctl, kBvCtlWords));
    }
    if (h[kBvHooks] == 0) return 0;
    if (round >= kBvMaxRounds) return fail(PYQSM_EHIP, "%s: components left after %d rounds", what, round);
    ++*rounds;
    ProfScope ps(c, sc.jump);
    for (int launch = 0;; ++launch) {
      hipLaunchKernelGGL(k_bv_jump<P>, dim3(pb), dim3(256), 0, c->stream, N, static_cast<const uint32_t*>(lab), hk,
                         ctl);
      PQ_HIP(hipGetLastError());
      PQ_TRY(fetch(c, h, ctl, kBvCtlWords));
      if (!h[kBvAgain]) break;
      if (launch >= kBvMaxRelaunch) return fail(PYQSM_EHIP, "%s: pointer jumping did not settle", what);
      PQ_HIP(hipMemsetAsync(ctl + kBvAgain, 0, 4, c->stream));
    }
    hipLaunchKernelGGL(k_bv_relabel<P>, dim3(pb), dim3(256), 0, c->stream, N, lab, static_cast<const uint32_t*>(hk));
    PQ_HIP(hipGetLastError());
  }
}

}  // namespace pyqsm
