// sdm_wordsum.hip -- the content checksums the MEX cache (sdm_mexcache.hip) decides residency on: of a host array (one core, several
// host threads from WORDSUM_POOL_FROM words on), of what a gateway has left in HBM (k_words_checksum), and the sampled hash of the
// cache's shortcut.  What is checksummed when is the cache's policy; here is only how.
#include "sdm_plan.h"
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

using namespace sdm;

namespace {
typedef unsigned long long u64;
constexpr sdm_int SAMPLE = 512;            // words of the sampled hash
constexpr sdm_int THREADS_FROM = 1 << 20;  // arrays from 1M words (8 MB) on are checksummed by several host threads
constexpr u64 P1 = 11400714785074694791ull, P2 = 14029467366897019727ull;
inline u64 rotl(u64 x, int r) { return (x << r) | (x >> (64 - r)); }
inline u64 lane(u64 acc, u64 v) { return rotl(acc + v * P2, 31) * P1; }
// every word, position dependent, as eight independent wrap-around sums of 32 x 32 -> 64 bit products: the compiler vectorises
// it on the host, and -- sums commute -- the same value comes out of a parallel reduction on the device (k_words_checksum:
// what a gateway leaves in HBM is fingerprinted there instead of by a pass over the host copy) or of several host threads.
// A change detector, not a cryptographic hash: any single changed word changes its sum.
#define SDM_CK_C1 {0x9E3779B1u, 0x85EBCA77u, 0xC2B2AE3Du, 0x27D4EB2Fu, 0x165667B1u, 0xD3A2646Du, 0xFD7046C5u, 0xB55A4F09u}
#define SDM_CK_C2 {0x8DA6B343u, 0xD8163841u, 0xCB1AB31Fu, 0x9F6B3F4Bu, 0xA54FF53Bu, 0x3C6EF373u, 0xBB67AE85u, 0x6A09E667u}
// what word w adds to sum k (c1 = C1[k], c2 = C2[k]); base: the index of the first word of w's group of eight
__host__ __device__ __forceinline__ u64 word_term(u64 w, unsigned base, u64 c1, u64 c2) {
  return (u64)((unsigned)w ^ base) * c1 + (u64)((unsigned)(w >> 32) ^ base) * c2;
}
// the eight sums over the words [i0, i1) of v (i0 a multiple of 8), added into acc, KEEP done with every word w = v[i + k]; one body,
// compiled for the baseline ISA and for AVX2 / AVX-512 (the host of a GPU box has them; picked once at run time)
#define SDM_CK_BODY(KEEP)                                                                                                    \
  static const u64 C1[8] = SDM_CK_C1, C2[8] = SDM_CK_C2;                                                                     \
  u64 a[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                                                                       \
  sdm_int i = i0;                                                                                                            \
  for (; i + 8 <= i1; i += 8)                                                                                                \
    for (int k = 0; k < 8; k++) {                                                                                            \
      const u64 w = v[i + k];                                                                                                \
      KEEP;                                                                                                                  \
      a[k] += word_term(w, (unsigned)i, C1[k], C2[k]);                                                                       \
    }                                                                                                                        \
  for (int k = 0; i + k < i1; k++) {                                                                                         \
    const u64 w = v[i + k];                                                                                                  \
    KEEP;                                                                                                                    \
    a[k] += word_term(w, (unsigned)i, C1[k], C2[k]);                                                                         \
  }                                                                                                                          \
  for (int k = 0; k < 8; k++) acc[k] += a[k];
void sums_base(const u64 *v, sdm_int i0, sdm_int i1, u64 *acc) { SDM_CK_BODY((void)0) }
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__) && !defined(SDM_NO_MULTIVERSION)
__attribute__((target("avx2"))) void sums_avx2(const u64 *v, sdm_int i0, sdm_int i1, u64 *acc) { SDM_CK_BODY((void)0) }
__attribute__((target("avx512f,avx512dq,avx512vl"))) void sums_avx512(const u64 *v, sdm_int i0, sdm_int i1, u64 *acc) { SDM_CK_BODY((void)0) }
typedef void (*sums_fn)(const u64 *, sdm_int, sdm_int, u64 *);
sums_fn pick_sums() {
  __builtin_cpu_init();
  if (__builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512dq") && __builtin_cpu_supports("avx512vl")) return sums_avx512;
  if (__builtin_cpu_supports("avx2")) return sums_avx2;
  return sums_base;
}
const sums_fn sums = pick_sums();
#else
#define sums sums_base
#endif
void pool_shutdown();
// A few helper threads for the checksums of arrays from WORDSUM_POOL_FROM words on: what a gateway is handed has usually just been written by
// the DMA engine (or by a memcpy with streaming stores) and comes from DRAM at 8 - 10 GB/s through one core.  The helpers are created
// at the first such array, sleep on a condition variable in between (woken in ~10 us) and are joined when the cache is torn down.
class SumPool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv_go, cv_done;
  const u64 *v = nullptr;
  sdm_int n = 0, chunk = 0;
  int nparts = 0, pending = 0;
  u64 gen = 0;
  bool stop = false;
  u64 part[16][8];
  void worker(int id, u64 seen) {                              // seen: the generation current when the helper was created (by the one thread that advances it)
    for (;;) {
      std::unique_lock<std::mutex> lk(mu);
      cv_go.wait(lk, [&] { return stop || gen != seen; });
      if (stop) return;
      seen = gen;
      const bool mine = id < nparts;
      const u64 *vv = v; const sdm_int i0 = std::min(n, (sdm_int)id * chunk), i1 = std::min(n, i0 + chunk);
      lk.unlock();
      if (mine) { for (int k = 0; k < 8; k++) part[id][k] = 0; sums(vv, i0, i1, part[id]); }
      lk.lock();
      if (mine && --pending == 0) cv_done.notify_one();
    }
  }
 public:
  // the eight sums of v[0, n) into acc, by `want` threads (the caller is one of them)
  void run(const u64 *vp, sdm_int len, int want, u64 *acc) {
    want = std::max(1, std::min(want, 16));
    if (th.empty()) { static bool reg = false; if (!reg) { reg = true; std::atexit([] { pool_shutdown(); }); } }   // sleeping helpers are joined before the process ends
    while ((int)th.size() < want - 1) { const int id = (int)th.size() + 1; const u64 g0 = gen; th.emplace_back([this, id, g0] { worker(id, g0); }); }
    const sdm_int ch = ((len + want - 1) / want + 7) & ~(sdm_int)7;
    {
      std::lock_guard<std::mutex> lk(mu);
      v = vp; n = len; chunk = ch; nparts = want; pending = want - 1; gen++;
    }
    cv_go.notify_all();
    for (int k = 0; k < 8; k++) part[0][k] = 0;
    sums(vp, 0, std::min(len, ch), part[0]);
    {
      std::unique_lock<std::mutex> lk(mu);
      cv_done.wait(lk, [&] { return pending == 0; });
    }
    for (int t = 0; t < want; t++) for (int k = 0; k < 8; k++) acc[k] += part[t][k];
  }
  void shutdown() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv_go.notify_all();
    for (auto &t : th) t.join();
    th.clear(); stop = false;
  }
  ~SumPool() { shutdown(); }
} g_pool;
void pool_shutdown() { g_pool.shutdown(); }
int g_threads = -1;        // wordsum_set_threads: threads of a big checksum (-1: 4 from WORDSUM_POOL_FROM words, up to 8 from 1M; never more than the host has)
sdm_int g_hash_ns = 0, g_hash_calls = 0;      // host time spent in complete checksums since the last wordsum_shutdown
DevBuf<u64> g_ck;                       // eight device words: checksum of values a gateway leaves in HBM (k_words_checksum)
u64 *g_ck_host = nullptr;               // ... and where they land on the host: pinned, so that the copy is queued like the rest and the one
                                        // synchronisation of the gateway (its download) covers it (to pageable memory every copy blocked the host)
// the same eight sums of n words in device memory, added into acc8 (zeroed by the caller): work-item t owns the words
// t, t + stride, ... with stride a multiple of 8, i.e. always the same sum
__global__ void k_words_checksum(const unsigned long long *v, long long n, unsigned long long *acc8) {
  const unsigned long long C1[8] = SDM_CK_C1, C2[8] = SDM_CK_C2;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
  const int k = (int)(t & 7);
  unsigned long long s = 0;
  for (long long i = t; i < n; i += stride) s += word_term(v[i], (unsigned)(i & ~7ll), C1[k], C2[k]);
  if (s) atomicAdd(&acc8[k], s);
}
}  // namespace

namespace sdm {
u64 wordsum_fold(const u64 *acc, sdm_int n) {
  u64 h = (u64)n;
  for (int k = 0; k < 8; k++) h = lane(h, acc[k]);
  return h;
}
u64 wordsum_full(const void *pv, sdm_int n) {
  const u64 *v = (const u64 *)pv;
  u64 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const auto t0 = std::chrono::steady_clock::now();
  int nt = 1;
  if (n >= WORDSUM_POOL_FROM) {
    const int hw = (int)std::thread::hardware_concurrency();
    nt = g_threads >= 0 ? g_threads : (n >= THREADS_FROM ? 8 : 4);
    nt = std::max(1, std::min(nt, std::max(1, hw)));
  }
  if (nt <= 1) sums(v, 0, n, acc);
  else g_pool.run(v, n, nt, acc);
  g_hash_ns += (sdm_int)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); g_hash_calls++;
  return wordsum_fold(acc, n);
}
u64 wordsum_copy(void *dst, const void *src, sdm_int n) {
  const u64 *v = (const u64 *)src; u64 *o = (u64 *)dst;
  const sdm_int i0 = 0, i1 = n;
  u64 acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  SDM_CK_BODY(o[i + k] = w)
  return wordsum_fold(acc, n);
}
u64 wordsum_sampled(const void *pv, sdm_int n) {                      // always the first and the last word
  const u64 *v = (const u64 *)pv;
  if (n <= 0) return 7;
  const sdm_int step = n <= SAMPLE ? 1 : (n + SAMPLE - 1) / SAMPLE;
  u64 h = (u64)n;
  for (sdm_int i = 0; i < n; i += step) h = lane(h, v[i]);
  return lane(h, v[n - 1]);
}
void wordsum_device(sdm_plan *p, const double *v, sdm_int n) {
  if (!g_ck.p) g_ck.alloc(8);
  if (!g_ck_host) SDM_HIP_CHECK(hipHostMalloc((void **)&g_ck_host, 8 * sizeof(u64), 0));
  const sdm_int wg = std::min<sdm_int>(2048, std::max<sdm_int>(64, n / 8192));
  SDM_HIP_CHECK(hipMemsetAsync(g_ck.p, 0, 8 * sizeof(u64), p->stream));
  SDM_LAUNCH(k_words_checksum, dim3((unsigned)wg), dim3(256), 0, p->stream, (const unsigned long long *)v, (long long)n, g_ck.p);
  SDM_HIP_CHECK(hipMemcpyAsync(g_ck_host, g_ck.p, 8 * sizeof(u64), hipMemcpyDeviceToHost, p->stream));
}
u64 wordsum_device_result(sdm_int n) { return wordsum_fold(g_ck_host, n); }
void wordsum_set_threads(int n) { g_threads = n; }
void wordsum_host_time(sdm_int *ns, sdm_int *calls) { *ns = g_hash_ns; *calls = g_hash_calls; }
void wordsum_shutdown() {
  g_pool.shutdown();
  g_ck.release();
  if (g_ck_host) { (void)hipHostFree(g_ck_host); g_ck_host = nullptr; }
  g_hash_ns = 0; g_hash_calls = 0;
}
}  // namespace sdm
