// wave_emu.h — TEST-ONLY: run the wavefront-level kernel bodies (csrc/lgssm_q4.h, lgssm_m4.h, lgssm_n16.h, lgssm_n16_elbo.h:
// code written per lane around cross-lane instructions - DPP moves, permlane swaps, ds_bpermute, ballots, the f32 MFMA tiles) on
// the HOST, so that the CPU tier can put their indexing under AddressSanitizer (GPU sanitizers are not available on the pool).
//
// One emulated wavefront = 64 host threads, one per lane, running the very same body; every cross-lane intrinsic is a
// rendezvous: each lane deposits its operand, a barrier, each lane picks what the instruction would have handed it.  (Two
// operand buffers used alternately make one barrier per instruction enough: a lane can be at most one instruction ahead.)
// Scope of the rendezvous: a DPP move (every control the harness knows - quad_perm, row_mirror, row_half_mirror, row_newbcast -
// reads inside one 16-lane row) meets the 16 lanes of its ROW only, on that row's own barrier, buffers and parity counter;
// everything else (MFMA tiles, ds_bpermute, ballot / any, permlane swaps, __syncthreads) meets all 64 lanes.  The "one
// instruction ahead" argument then holds per scope, and the n = 16 ELBO kernels - four row-groups taking turns on the matrix
// cores, with DPP traffic inside group-dependent branches, legal on the hardware where a DPP move only needs its own row - run
// here too.  A wave-scope instruction that only some lanes reach (or a row-scope one only some lanes of a row reach) would wait
// forever: every barrier has a deadline, past which the harness names the scope, the lane and the block and aborts.
// Workgroups of more than one wavefront (launch_wg: whole wavefronts up to the hardware's 1024 threads - the recurrent kernels of
// csrc/lstm_fast.h and gru_fast.h at 256, k_colsum_v4 at 512, k_loss_head_fwd at 1024; blockIdx.x / .y / .z follow the grid): one host thread per lane of every wavefront of the block; __syncthreads() meets every lane of the BLOCK, all the
// cross-lane instructions keep the scope above (their wavefront, or their row).  A __shared__ array of a kernel (KV_LDS /
// KV_LDS16 of csrc/lds_decl.h) and the launch's dynamic LDS (KV_LDS_DYN) are heap allocations of exactly their size, made by the
// first lane that reaches the declaration, filled with NaNs, freed when the block has ended: AddressSanitizer sees their bounds
// (a static array of a template kernel is a COMDAT object, which it does not pad), and a read of an element no lane wrote is a NaN.
// atomicAdd(float *, float) on an LDS or a global word is a real atomic of the host (a compare-exchange loop on the 32-bit word):
// the lanes are host threads, so ThreadSanitizer sees an atomic and AddressSanitizer its address; the order of the adds is as
// free as on the card.
// What the encoder's convolution kernels (csrc/vae_conv_mid.h, the stem of vae_conv_edge.h) lean on the hardware for is explicit
// here: a raw buffer access (make_buffer_rsrc, raw_buffer_load_b128, raw_buffer_store_b128 / _b32) below num_records is the plain
// access, one at or past it returns zeros / is dropped and is counted, one that straddles it aborts; an LDS read that may leave
// the allocation on purpose (KV_LDS_RD) is the real read inside the workgroup's LDS object, 0 from kLdsOob elements on, an abort
// between the two.
// Arithmetic of the MFMA shims: k-ascending fmaf chains in fp32, which is what the kernels' parity argument assumes.
// This is a sanitizer / debug harness, slow by design (a barrier per instruction): tiny problems only.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

namespace wemu {

struct Dim3 { unsigned x, y, z; };
inline thread_local Dim3 t_tid = {0, 0, 0}, t_bid = {0, 0, 0}, t_gdim = {1, 1, 1};
inline int lane_id() { return (int)(t_tid.x & 63); }

// a barrier of `n` threads with a deadline: a rendezvous that not every member reaches is a harness or kernel-structure error,
// reported (scope, lane, block) instead of hanging the test tier
constexpr int kDeadlineSeconds = 10;
class Barrier {
 public:
  Barrier(unsigned n, const char *scope) : n_(n), scope_(scope) {}
  void wait() {
    // Arrivals are counted on an atomic and a waiter first polls the generation, yielding its core between looks: with 256 lane
    // threads on a few cores a condition variable alone costs one mutex hand-over and one wake-up per lane and rendezvous (half
    // a millisecond per block barrier).  A waiter that has polled kSpins times sleeps on the condition variable, under the
    // deadline; the generation changes under the mutex, so that sleeper cannot miss it.
    const unsigned gen = gen_.load(std::memory_order_acquire);
    if (count_.fetch_add(1, std::memory_order_acq_rel) + 1 == n_) {
      count_.store(0, std::memory_order_relaxed);   // (before the generation: whoever sees the new generation sees the reset)
      {
        std::lock_guard<std::mutex> lk(m_);
        gen_.store(gen + 1, std::memory_order_release);
      }
      cv_.notify_all();
      return;
    }
    for (int i = 0; i < kSpins; ++i) {
      if (gen_.load(std::memory_order_acquire) != gen) return;
      std::this_thread::yield();
    }
    std::unique_lock<std::mutex> lk(m_);
    // (a deadline on the system clock: the wait is then pthread_cond_timedwait, which thread sanitizers know releases the mutex;
    // wait_for is pthread_cond_clockwait, which gcc 11's does not intercept - it reports the barrier itself as a double lock)
    if (!cv_.wait_until(lk, std::chrono::system_clock::now() + std::chrono::seconds(kDeadlineSeconds), [&] { return gen_.load(std::memory_order_acquire) != gen; })) {
      fprintf(stderr, "wave_emu: %s-scope rendezvous not reached by all %u lanes within %d s (lane %d, block %u waiting)\n",
              scope_, n_, kDeadlineSeconds, lane_id(), t_bid.x);
      fflush(stderr);
      abort();
    }
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  const unsigned n_;
  const char *scope_;
  static constexpr int kSpins = 4096;
  std::atomic<unsigned> count_{0}, gen_{0};
};

struct Wave {
  Barrier bar{64, "wave"};
  Barrier row_bar[4]{{16, "row"}, {16, "row"}, {16, "row"}, {16, "row"}};
  uint32_t a[2][64], b[2][64];   // wave-scope operands
  uint32_t r[2][64];             // row-scope operands (row k uses lanes 16k..16k+15 of each)
};
// the workgroup in flight: its barrier (every lane of every wavefront) and its LDS objects, keyed by their declaration
struct Block {
  explicit Block(unsigned threads, size_t dyn_bytes) : bar(threads, "block"), dyn_bytes_(dyn_bytes) {}
  Block(const Block &) = delete;
  ~Block() {
    for (auto &kv : lds_) free(kv.second);
  }
  void *shared(int key, size_t bytes) {   // key: the declaration (KV_LDS: __COUNTER__), -1: the launch's dynamic LDS
    std::lock_guard<std::mutex> lk(m_);
    auto it = lds_.find(key);
    if (it != lds_.end()) return it->second;
    void *ptr = nullptr;
    if (posix_memalign(&ptr, 16, bytes ? bytes : 1) != 0) abort();   // exactly `bytes`: the next byte is a redzone
    memset(ptr, 0xFF, bytes);                                         // NaNs
    lds_.emplace(key, ptr);
    bytes_.emplace(key, bytes);
    return ptr;
  }
  void *dyn_shared() { return shared(-1, dyn_bytes_); }
  // the LDS object of this workgroup that holds address p: its first byte and one past its last, or false
  bool object_of(const void *p, const char **lo, const char **hi) {
    std::lock_guard<std::mutex> lk(m_);
    for (auto &kv : lds_) {
      const char *b = static_cast<const char *>(kv.second), *e = b + bytes_[kv.first];
      if (static_cast<const char *>(p) >= b && static_cast<const char *>(p) < e) {
        *lo = b, *hi = e;
        return true;
      }
    }
    return false;
  }
  Barrier bar;

 private:
  std::mutex m_;
  std::map<int, void *> lds_;
  std::map<int, size_t> bytes_;
  const size_t dyn_bytes_;
};
inline thread_local Block *t_block = nullptr;
inline thread_local Dim3 t_bdim = {64, 1, 1};
inline void *block_shared(int key, size_t bytes) { return t_block->shared(key, bytes); }
inline void *block_dyn_shared() { return t_block->dyn_shared(); }
inline thread_local Wave *t_wave = nullptr;
inline thread_local int t_par = 0;    // parity of this lane's wave-scope exchanges
inline thread_local int t_rpar = 0;   // parity of this lane's row-scope exchanges

inline void sync() { t_wave->bar.wait(); }                                       // wave-scope rendezvous of the shims below
inline void sync_block() { (t_block ? t_block->bar : t_wave->bar).wait(); }      // __syncthreads(): every lane of the workgroup
// every lane deposits v; returns the buffer to read the other lanes' values from (valid until this lane's next exchange)
inline const uint32_t *exchange(uint32_t v) {
  const int p = t_par;
  t_par ^= 1;
  t_wave->a[p][lane_id()] = v;
  sync();
  return t_wave->a[p];
}
// the same within this lane's 16-lane row only: the returned buffer is valid for the lanes of that row
inline const uint32_t *row_exchange(uint32_t v) {
  const int p = t_rpar;
  t_rpar ^= 1;
  const int l = lane_id();
  t_wave->r[p][l] = v;
  t_wave->row_bar[l >> 4].wait();
  return t_wave->r[p];
}
inline uint32_t fbits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
inline float bitsf(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// v_mov_b32_dpp with row_mask = bank_mask = 0xf, bound_ctrl: the controls the kernels use
inline int dpp_source(int lane, int ctrl) {
  if (ctrl >= 0 && ctrl <= 0xFF) return (lane & ~3) | ((ctrl >> (2 * (lane & 3))) & 3);   // quad_perm
  if (ctrl == 0x140) return (lane & ~15) | (15 - (lane & 15));                             // row_mirror
  if (ctrl == 0x141) return (lane & ~7) | (7 - (lane & 7));                                // row_half_mirror
  if (ctrl >= 0x150 && ctrl <= 0x15F) return (lane & ~15) | (ctrl - 0x150);                // row_newbcast:K
  __builtin_trap();   // a control this harness does not know: extend it rather than guess
}
inline int mov_dpp(int v, int ctrl, int, int, bool) {   // every control above reads inside the caller's row: a row rendezvous
  const uint32_t *all = row_exchange((uint32_t)v);
  return (int)all[dpp_source(lane_id(), ctrl)];
}
inline float shfl(float v, int src, int) { return bitsf(exchange(fbits(v))[src & 63]); }
inline float shfl_xor(float v, int mask, int) { return bitsf(exchange(fbits(v))[(lane_id() ^ mask) & 63]); }
inline unsigned long long ballot(bool pred) {
  const uint32_t *all = exchange(pred ? 1u : 0u);
  unsigned long long m = 0;
  for (int l = 0; l < 64; ++l) m |= (unsigned long long)(all[l] & 1u) << l;
  return m;
}
inline bool any(bool pred) { return ballot(pred) != 0; }

struct U2 {
  uint32_t v[2];
  uint32_t operator[](int i) const { return v[i]; }
};
// v_permlane16_swap / v_permlane32_swap (fi = bc = false): {new vdst, new src0}; odd rows (halves) of vdst trade places with
// even rows (halves) of src0
inline U2 permlane_swap(uint32_t vdst, uint32_t src0, int width) {
  const int p = t_par;
  t_par ^= 1;
  const int l = lane_id();
  t_wave->a[p][l] = vdst, t_wave->b[p][l] = src0;
  sync();
  const bool upper = (l / width) & 1;
  U2 r;
  r.v[0] = upper ? t_wave->b[p][l - width] : vdst;    // vdst[upper] <- src0[lower]
  r.v[1] = upper ? src0 : t_wave->a[p][l + width];    // src0[lower] <- vdst[upper]
  return r;
}

template <class V4>
inline V4 mfma_4x4x1(float x, float y, V4 c) {          // 16 blocks of 4 lanes: D[r][j] += a(lane 4 blk + r) * b(lane 4 blk + j)
  const int p = t_par;
  t_par ^= 1;
  const int l = lane_id();
  t_wave->a[p][l] = fbits(x), t_wave->b[p][l] = fbits(y);
  sync();
  const int base = l & ~3;
  for (int r = 0; r < 4; ++r) c[r] = fmaf(bitsf(t_wave->a[p][base + r]), bitsf(t_wave->b[p][l]), c[r]);
  return c;
}
template <class V4>
inline V4 mfma_16x16x4(float x, float y, V4 c) {        // A[i][k] on lane i + 16 k, B[k][j] on lane j + 16 k, D[4 g + r][j] in reg r of lane (j, g)
  const int p = t_par;
  t_par ^= 1;
  const int l = lane_id(), j = l & 15, g = l >> 4;
  t_wave->a[p][l] = fbits(x), t_wave->b[p][l] = fbits(y);
  sync();
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 4; ++k) c[r] = fmaf(bitsf(t_wave->a[p][4 * g + r + 16 * k]), bitsf(t_wave->b[p][j + 16 * k]), c[r]);
  return c;
}

template <class V16>
inline V16 mfma_32x32x2(float x, float y, V16 c) {      // A[i][k] on lane i + 32 k, B[k][j] on lane j + 32 k, D[(r & 3) + 8 (r >> 2) + 4 h][j] in reg r of lane (j, h)
  const int p = t_par;
  t_par ^= 1;
  const int l = lane_id(), j = l & 31, h = l >> 5;
  t_wave->a[p][l] = fbits(x), t_wave->b[p][l] = fbits(y);
  sync();
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
    for (int k = 0; k < 2; ++k) c[r] = fmaf(bitsf(t_wave->a[p][row + 32 * k]), bitsf(t_wave->b[p][j + 32 * k]), c[r]);
  }
  return c;
}

// Raw buffer resources (stride 0): base + num_records bytes.  An access wholly below num_records is the plain access at
// base + offset (AddressSanitizer sees the real address: a resource longer than its tensor becomes a report); one wholly at or
// past it loads zeros / is dropped and is counted (oob_loads / oob_stores, read and reset by whoever launches); one that straddles
// num_records is nothing the product issues, and how the hardware range-checks inside an access must not decide a test: abort.
struct Rsrc {
  char *base;
  uint32_t num_records;
};
typedef unsigned int U4 __attribute__((vector_size(16)));   // what `unsigned int ext_vector_type(4)` is in a host build
inline std::atomic<long> oob_loads{0}, oob_stores{0};
inline thread_local const char *t_kernel = "?";         // named by the launcher, for the abort messages below
inline Rsrc make_rsrc(void *p, int, int num_records, int) { return Rsrc{static_cast<char *>(p), (uint32_t)num_records}; }
inline int buffer_class(const Rsrc &r, uint32_t off, uint32_t bytes) {   // 1 inside, 0 outside, -1 straddling
  return (uint64_t)off + bytes <= r.num_records ? 1 : (off >= r.num_records ? 0 : -1);
}
inline int buffer_range(const Rsrc &r, uint32_t off, uint32_t bytes, const char *what) {   // 1 inside, 0 outside
  const int c = buffer_class(r, off, bytes);
  if (c >= 0) return c;
  fprintf(stderr, "wave_emu: %s of %u bytes at offset %u straddles num_records = %u (kernel %s, block %u, lane %u)\n", what, bytes, off,
          r.num_records, t_kernel, t_bid.x, t_tid.x);
  fflush(stderr);
  abort();
}
inline U4 buffer_load_b128(const Rsrc &r, uint32_t voff, uint32_t soff) {
  U4 out = {0, 0, 0, 0};
  if (buffer_range(r, voff + soff, 16, "buffer load")) memcpy(&out, r.base + (voff + soff), 16);
  else oob_loads.fetch_add(1, std::memory_order_relaxed);
  return out;
}
template <class V>
inline void buffer_store_b128(const V &v, const Rsrc &r, uint32_t voff, uint32_t soff) {
  if (buffer_range(r, voff + soff, 16, "buffer store")) {
    memcpy(r.base + (voff + soff), &v, 16);
  } else {
    oob_stores.fetch_add(1, std::memory_order_relaxed);
  }
}
inline void buffer_store_b32(uint32_t v, const Rsrc &r, uint32_t voff, uint32_t soff) {
  if (buffer_range(r, voff + soff, 4, "buffer store")) memcpy(r.base + (voff + soff), &v, 4);
  else oob_stores.fetch_add(1, std::memory_order_relaxed);
}

// KV_LDS_RD of csrc/lds_decl.h: a DS read whose address may lie outside the workgroup's LDS on purpose.  The index counts from
// `arr`, a pointer into one LDS object of the workgroup: inside that object the real read (sanitizer-checked, NaN where no lane
// wrote), at kLdsOob elements or above the 0 the hardware returns, anywhere between - an address the card would also answer,
// with a neighbour's data or with 0 depending on the allocation - abort.
constexpr long kLdsOob = 1 << 24;
// `arr` sits `before` elements into its object and `after` elements before its end: 1 the real read, 0 out of range, -1 between
inline int lds_class(long before, long after, long i) { return i >= -before && i < after ? 1 : (i >= kLdsOob ? 0 : -1); }
inline thread_local const char *t_lds_lo = nullptr, *t_lds_hi = nullptr;   // the object of this lane's last KV_LDS_RD (reset per block)
template <class T>
inline T lds_read(const T *arr, long i, const char *name) {
  const char *&lo = t_lds_lo, *&hi = t_lds_hi;
  const char *base = reinterpret_cast<const char *>(arr);
  if (base < lo || base >= hi) {
    if (!t_block || !t_block->object_of(arr, &lo, &hi)) {
      fprintf(stderr, "wave_emu: KV_LDS_RD(%s, %ld): not an LDS array of this workgroup (kernel %s, block %u, lane %u)\n", name, i,
              t_kernel, t_bid.x, t_tid.x);
      fflush(stderr);
      abort();
    }
  }
  const int c = lds_class((long)((base - lo) / (long)sizeof(T)), (long)((hi - base) / (long)sizeof(T)), i);
  if (c == 0) return T(0);
  if (c == 1) return arr[i];
  fprintf(stderr, "wave_emu: KV_LDS_RD(%s, %ld) is outside the workgroup's LDS object (%ld elements before it .. %ld after) and below the "
          "out-of-range base %ld (kernel %s, block %u, lane %u)\n", name, i, (long)((base - lo) / (long)sizeof(T)),
          (long)((hi - base) / (long)sizeof(T)), kLdsOob, t_kernel, t_bid.x, t_tid.x);
  fflush(stderr);
  abort();
}

// launch: `blocks` one-wavefront workgroups, one after the other, 64 threads each
inline void launch(unsigned blocks, const std::function<void()> &body) {
  for (unsigned blk = 0; blk < blocks; ++blk) {
    Wave w;
    std::vector<std::thread> th;
    th.reserve(64);
    for (unsigned l = 0; l < 64; ++l)
      th.emplace_back([&, l] {
        t_wave = &w, t_par = 0, t_rpar = 0, t_tid = {l, 0, 0}, t_bid = {blk, 0, 0}, t_gdim = {blocks, 1, 1};
        body();
      });
    for (auto &t : th) t.join();
  }
}

// launch_wg: a grid of workgroups of `threads` lanes (a multiple of 64, at most 1024) with `dyn_bytes` of dynamic LDS, in
// ascending order (x fastest), every lane of a workgroup a host thread.  The lane threads PERSIST over the blocks of a launch
// (256 fresh threads per workgroup made a launch of a few hundred small blocks cost seconds) and over launches (LanePool below):
// lane l runs lane l of block 0, 1, 2, ... in turn.  What belongs to a block is still made for it alone - its Block (the block barrier, NaN-filled LDS objects of
// exact size) and its Waves (barriers, operand buffers) are built by the first lane that enters the block and destroyed by the
// last one that leaves it, and every lane resets its parity counters and takes the block's index on entry - so nothing a block
// did is visible to the next one.  There is no rendezvous BETWEEN blocks: a lane that has left block k enters block k + 1 and
// waits at its first barrier (under that barrier's own deadline), as workgroups of one launch overlap on the card.
struct BlockSlot {
  BlockSlot(unsigned threads, size_t dyn_bytes) : blk(threads, dyn_bytes), waves(threads / 64), inside(threads) {}
  Block blk;
  std::vector<Wave> waves;
  unsigned inside;   // lanes that have not left the block yet
};
// The lane threads also persist from launch to launch: a pool of host threads that grows to the widest workgroup asked for and
// sleeps between launches (a column-sum case list is several hundred launches of 512 lanes, the loss head's 1024 lanes per launch;
// fresh threads cost more than the kernels, most of all under ThreadSanitizer).  Worker l is lane l of every launch that has that
// many lanes; the pool is never torn down (its threads are detached and sleep when the process ends).
class LanePool {
 public:
  static LanePool &get() {
    static LanePool *pool = new LanePool;
    return *pool;
  }
  void run(unsigned lanes, const std::function<void(unsigned)> &job) {   // job(l) for l = 0 .. lanes - 1, each on its own thread
    std::lock_guard<std::mutex> one_launch(launch_);
    std::unique_lock<std::mutex> lk(m_);
    while (workers_ < lanes) {
      std::thread(&LanePool::work, this, workers_, gen_).detach();
      ++workers_;
    }
    job_ = &job, lanes_ = lanes, pending_ = lanes, ++gen_;
    wake_.notify_all();
    while (pending_ != 0) done_.wait(lk);
    job_ = nullptr;
  }

 private:
  void work(unsigned l, uint64_t seen) {
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      while (gen_ == seen) wake_.wait(lk);
      seen = gen_;
      if (l >= lanes_) continue;
      const std::function<void(unsigned)> *job = job_;
      lk.unlock();
      (*job)(l);
      lk.lock();
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::mutex launch_, m_;
  std::condition_variable wake_, done_;
  const std::function<void(unsigned)> *job_ = nullptr;
  unsigned workers_ = 0, lanes_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
};
inline void launch_wg(Dim3 grid, unsigned threads, size_t dyn_bytes, const std::function<void()> &body) {
  if (threads == 0 || threads % 64 != 0 || threads > 1024) {
    fprintf(stderr, "wave_emu: a workgroup of %u threads is not 1..16 whole wavefronts\n", threads);
    abort();
  }
  const uint64_t nblocks = (uint64_t)grid.x * grid.y * grid.z;
  std::mutex m;
  std::map<uint64_t, BlockSlot *> live;
  LanePool::get().run(threads, [&](unsigned l) {
    for (uint64_t b = 0; b < nblocks; ++b) {
      BlockSlot *slot;
      {
        std::lock_guard<std::mutex> lk(m);
        BlockSlot *&s = live[b];
        if (!s) s = new BlockSlot(threads, dyn_bytes);
        slot = s;
      }
      t_block = &slot->blk, t_wave = &slot->waves[l / 64], t_par = 0, t_rpar = 0, t_lds_lo = t_lds_hi = nullptr;
      t_tid = {l, 0, 0}, t_gdim = grid, t_bdim = {threads, 1, 1};
      t_bid = {(unsigned)(b % grid.x), (unsigned)(b / grid.x % grid.y), (unsigned)(b / ((uint64_t)grid.x * grid.y))};
      body();
      t_block = nullptr, t_wave = nullptr;
      bool last;
      {
        std::lock_guard<std::mutex> lk(m);
        last = --slot->inside == 0;
        if (last) live.erase(b);
      }
      if (last) delete slot;
    }
  });
}

}  // namespace wemu

struct alignas(16) float4 {
  float x, y, z, w;
};
struct alignas(8) float2 {
  float x, y;
};
struct alignas(16) uint4 {
  uint32_t x, y, z, w;
};
inline float __uint_as_float(uint32_t u) { return wemu::bitsf(u); }
inline uint32_t __float_as_uint(float x) { return wemu::fbits(x); }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline float2 make_float2(float x, float y) { return float2{x, y}; }

// atomicAdd on an LDS or global float: returns the old value, as HIP's
inline float atomicAdd(float *addr, float v) {
  uint32_t *word = reinterpret_cast<uint32_t *>(addr);
  uint32_t seen = __atomic_load_n(word, __ATOMIC_RELAXED);
  while (!__atomic_compare_exchange_n(word, &seen, wemu::fbits(wemu::bitsf(seen) + v), true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return wemu::bitsf(seen);
}

// ---- what the kernel headers see ----------------------------------------------------------------------------------------------
#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(n)
#define ext_vector_type(n) vector_size((n) * 4)   // g++: GNU vector types index, initialise and mix with scalars the same way
#define threadIdx (wemu::t_tid)
#define blockIdx (wemu::t_bid)
#define gridDim (wemu::t_gdim)
#define blockDim (wemu::t_bdim)
#define __syncthreads() wemu::sync_block()
#define __shfl(v, src, w) wemu::shfl((v), (src), (w))
#define __shfl_xor(v, mask, ...) wemu::shfl_xor((v), (mask), 64)   // (the width, where a kernel gives one, is the wavefront)
#define __ballot(p) wemu::ballot((p))
#define __any(p) wemu::any((p))
#define __builtin_amdgcn_mov_dpp(v, ctrl, rm, bm, bc) wemu::mov_dpp((v), (ctrl), (rm), (bm), (bc))
#define __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, x, y, z) wemu::mfma_4x4x1((a), (b), (c))
#define __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, x, y, z) wemu::mfma_16x16x4((a), (b), (c))
#define __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, x, y, z) wemu::mfma_32x32x2((a), (b), (c))
#define __amdgpu_buffer_rsrc_t wemu::Rsrc
#define __builtin_amdgcn_make_buffer_rsrc(p, stride, num, flags) wemu::make_rsrc((p), (stride), (num), (flags))
#define __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, aux) wemu::buffer_load_b128((r), (voff), (soff))
#define __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, soff, aux) wemu::buffer_store_b128((v), (r), (voff), (soff))
#define __builtin_amdgcn_raw_buffer_store_b32(v, r, voff, soff, aux) wemu::buffer_store_b32((v), (r), (voff), (soff))
#define __builtin_amdgcn_permlane16_swap(a, b, fi, bc) wemu::permlane_swap((a), (b), 16)
#define __builtin_amdgcn_permlane32_swap(a, b, fi, bc) wemu::permlane_swap((a), (b), 32)
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#define __builtin_amdgcn_s_waitcnt(x) ((void)0)
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
#define __builtin_amdgcn_sqrtf(x) sqrtf((x))
#define __logf(x) logf((x))
#define __expf(x) expf((x))
