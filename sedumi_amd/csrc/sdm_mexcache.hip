// sdm_mexcache.hip -- the process-wide resident state behind the mexFunction shims (INTEGRATION.md "Keeping data on the
// device across MEX calls").  Every .mex binary is its own shared object with its own statics, so a cache kept inside the
// shims would never be shared between getada3.mex, blkchol.mex and fwblkslv.mex; libsedumi_hip.so is loaded once per
// process, so the cache lives here, behind the C ABI.
//
// What a MATLAB session hands the gateways of one solve, call after call (sedumi.m:450-462, wrapPcg.m:56-59):
//   * the SAME problem data every iteration -- At, K, the ADA pattern, the symbolic factor: recognised by fingerprints
//     (below), their device-side analysis (ada_build, chol_build) is done once and kept;
//   * the value arrays one gateway returned as the next one's input -- ADA from getada1 -> getada2 -> getada3 -> blkchol,
//     L.L from blkchol -> fwblkslv / bwblkslv: the device still holds them, so they are not uploaded again.
// Residency is decided by CONTENT: an array is taken for the one the device holds only if a checksum over EVERY word of what the
// host array holds now equals the checksum of the resident data (for arrays a gateway produced: summed on the device over what
// it left in HBM, k_words_checksum).  The one shortcut, and its limit:
//   * arrays of up to `full_below` words (default 65 536 = 512 KB, ~15 us) are checksummed completely at EVERY presentation;
//   * a larger array is checksummed completely the first time an address presents it in an EPOCH (one epoch = the interval
//     between two blkchol calls, i.e. one IPM iteration); further presentations AT THAT ADDRESS IN THAT EPOCH are accepted on
//     length + a sampled hash (SAMPLE evenly spaced words + first and last).  An address is trusted only for the epoch in
//     which this cache itself READ every word there and found the resident content.  Not trusted: the output buffer a gateway has
//     just written (the host may copy the result and free the buffer -- Octave and this package's own MEX host do -- and hand the
//     address to another array; GPUTEST r04 / r05a failed on exactly that); nothing is remembered across epochs.
// Limit of the shortcut (stated in DESIGN.md 1a / INTEGRATION.md, asserted by tests/test_mexshims.py): a large array that is
// edited IN PLACE -- or freed and replaced at the same address by an array of the same length -- at words the sample does not
// touch, between two presentations inside one epoch, is still taken for the resident one.  sedumi.m never does that
// (sedumi.m:450-462, wrapPcg.m:56-59 hand the gateways' outputs on untouched).  sdm_mexcache_set_strict(1) removes the shortcut:
// every presentation is checksummed completely, whatever the size.
#include "sdm_plan.h"
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

using namespace sdm;

namespace {
typedef unsigned long long u64;
// Checksums a shim has just computed itself while it copied an array (sdm_mexcache_copy_words: the pattern of the array it returns is a copy
// of its input's -- one pass over the input for both): valid for the gateway call in progress only, dropped when it returns.
struct Note { const void *p; sdm_int n; u64 sum; };
Note g_notes[4];
int g_nnotes = 0;
void drop_notes() { g_nnotes = 0; }
bool strict = false;            // sdm_mexcache_set_strict: no shortcut, every presentation is checksummed completely
sdm_int full_below = 1 << 16;   // sdm_mexcache_set_full_below: arrays up to this many words are checksummed completely at every presentation
u64 g_epoch = 1;                // advances with every blkchol call: the lifetime of a trusted address (file header)
sdm_int g_fullsum_words = 0;    // words checksummed on the host since the last sdm_mexcache_clear (the cost of the content checks; stats[11])

// What is known about one array the device holds a copy of (or the analysis of): its length, the sampled hash, the checksum of every
// word, and the addresses at which THIS epoch every word has been read (or written) by the cache itself.
struct Finger {
  sdm_int n = -1;
  u64 sample = 0, full = 0;
  struct { const void *p; u64 epoch; } ok[8] = {};
  int nok = 0;
  bool trusted(const void *p) const {
    for (int i = 0; i < 8; i++) if (p && ok[i].p == p && ok[i].epoch == g_epoch) return true;
    return false;
  }
  // every word at p was read (or written) by the cache in this epoch and is this content
  void verified(const void *p) {
    if (!p || trusted(p)) return;
    for (int i = 0; i < 8; i++) if (ok[i].p == p) { ok[i].epoch = g_epoch; return; }
    ok[nok & 7].p = p; ok[nok++ & 7].epoch = g_epoch;
  }
  // the checksum computed elsewhere: on the device copy of the values that have just been downloaded to p.  No address is trusted
  // yet: whoever presents this content has it read completely once (file header)
  void take_with_full(const void *p, sdm_int len, u64 fullhash) {
    n = len; sample = wordsum_sampled(p, len); full = fullhash;
    for (auto &a : ok) a.p = nullptr;
    nok = 0;
  }
  // ... computed here, by a pass over p: that address is trusted for this epoch
  void take(const void *p, sdm_int len) { take_with_full(p, len, wordsum_full(p, len)); g_fullsum_words += len; verified(p); }
  bool same(const void *p, sdm_int len) {
    if (len != n || n < 0) return false;
    if (!strict && len > full_below && trusted(p)) return wordsum_sampled(p, len) == sample;   // the shortcut of the file header
    u64 sum = 0;
    bool noted = false;
    for (int i = 0; i < g_nnotes; i++) if (g_notes[i].p == p && g_notes[i].n == len) { sum = g_notes[i].sum; noted = true; }
    if (!noted) { g_fullsum_words += len; sum = wordsum_full(p, len); }
    if (sum != full) return false;
    verified(p);
    return true;
  }
  void forget() { n = -1; }
};

// ---- index patterns (CSC jc / ir pairs): interned, so that the slots below compare small integers.  An id is never reused.
struct Pattern { sdm_int ncol = -1; Finger jc, ir; u64 id = 0, used = 0; std::vector<sdm_int> jcc, irc; };   // (jcc / irc: a host copy, lazy mode only)
Pattern g_pat[12];
u64 g_next_id = 1, g_clock = 0;
// ---- lazy intermediates (SEDUMI_HIP_LAZY = 0 | 1 | 2, or sdm_mexcache_set_lazy; default 2 since round 6).  sedumi.m:450-458 hands ADA' from getada1 to getada2
// to getada3 to blkchol and never looks at it.  Level 1: getada1.mex / getada2.mex return, instead of ADA' (values + a copy of the pattern,
// 2 x 128 MB for MAXCUT-4000, each read again by the next gateway's content check), a TOKEN: an m x m sparse matrix with the one nonzero
// (1,1) = LAZY_BASE + a serial number that is never reused; the values stay on the device.  A gateway handed a token takes the
// device's ADA' if the token is the current one and fails loudly otherwise (there are no values to fall back on).  getada3.mex
// materialises: its ADA' and absd are the reference's.  Level 2: getada3.mex returns a token as well (absd is real) and blkchol.mex
// factors the device's ADA' -- what crosses PCIe per iteration is then absd, L.L, L.d, the pivot lists and the solves' vectors.
constexpr double LAZY_BASE = 6755399441055744.0;             // 1.5 * 2^52: token = LAZY_BASE + serial, exact in a double
int g_lazy = -1;                                             // -1: not read from the environment yet
u64 g_serial = 0;
struct { u64 serial = 0, pat = 0; sdm_int m = 0, nnz = 0; } g_tok;      // the current token: which pattern the device's ADA' (g_last.plan) has
int lazy_level() {
  // default (round 6): level 2 -- every call site of the reference hands the array on untouched (sedumi.m:450-458, optstep.m:68-76; symbchol.m:62-73
  // and sedumi.m:401 read the global before the first getada1): tests/test_mexshims.py runs whole solves through the shims at levels 0 and 2
  // and compares the logs.  SEDUMI_HIP_LAZY=0 gives the reference's arrays back at every gateway.
  if (g_lazy < 0) { const char *e = getenv("SEDUMI_HIP_LAZY"); g_lazy = e ? std::max(0, std::min(2, atoi(e))) : 2; }
  return g_lazy;
}
// the tokens handed out last (serial -> pattern): getada1.mex needs only the PATTERN of the ADA' it is given (it starts from zero, getada1.c:222-225),
// so it also accepts a token that is no longer current -- sedumi.m's global still holds the token of ITS last getada3 when optstep.m has run the
// three gateways on its own copy in between
struct TokRec { u64 serial = 0, pat = 0; sdm_int m = 0, nnz = 0; };
TokRec g_tok_hist[16];
void remember_token(u64 serial, u64 pat, sdm_int m, sdm_int nnz) { TokRec &r = g_tok_hist[serial & 15]; r.serial = serial; r.pat = pat; r.m = m; r.nnz = nnz; }
bool is_token(double t) { return t > LAZY_BASE && t < LAZY_BASE + 4294967296.0; }
Pattern *pattern_by_id(u64 id) { for (auto &p : g_pat) if (p.id == id) return &p; return nullptr; }
u64 intern(sdm_int ncol, const sdm_int *jc, const sdm_int *ir) {
  const sdm_int nnz = jc[ncol];
  for (auto &p : g_pat)
    if (p.id && p.ncol == ncol && p.jc.same(jc, ncol + 1) && p.ir.same(ir, nnz)) {
      p.used = ++g_clock;
      if (lazy_level() > 0 && p.irc.empty() && nnz > 0) { p.jcc.assign(jc, jc + ncol + 1); p.irc.assign(ir, ir + nnz); }
      return p.id;
    }
  Pattern *v = &g_pat[0];
  for (auto &p : g_pat) if (p.used < v->used) v = &p;                 // least recently used (empty entries first: used = 0)
  v->ncol = ncol; v->jc.take(jc, ncol + 1); v->ir.take(ir, nnz); v->id = g_next_id++; v->used = ++g_clock;
  v->jcc.clear(); v->irc.clear();
  if (lazy_level() > 0) { v->jcc.assign(jc, jc + ncol + 1); v->irc.assign(ir, ir + nnz); }
  return v->id;
}

sdm_int g_stat[16];       // counters for tests and the bench (sdm_mexcache_stats)
enum { ST_ADA_BUILD = 0, ST_ADA_REUSE = 1, ST_ADA_UPLOAD = 2, ST_ADA_RESIDENT = 3, ST_CHOL_BUILD = 4, ST_CHOL_REUSE = 5,
       ST_X_UPLOAD = 6, ST_X_RESIDENT = 7, ST_SOLVE_RESIDENT = 8, ST_SOLVE_STATELESS = 9, ST_AT_UPLOAD = 10 };

int device() { const char *dev = getenv("SEDUMI_HIP_DEVICE"); return dev ? atoi(dev) : 0; }
sdm_plan *new_plan() { sdm_plan *p = sdm_plan_create(device(), nullptr); if (!p) plan_ok(1); return p; }
bool vec_is(const std::vector<sdm_int> &v, const sdm_int *p, sdm_int n) {
  return (sdm_int)v.size() == n && (n == 0 || memcmp(v.data(), p, (size_t)n * sizeof(sdm_int)) == 0);
}

// ---- one slot per getada gateway: the plan that holds its slice of the problem, and what it was built from.  SlotKey: what a gateway
// states about the call in progress -- its slot's plan is good for it if all of this is what the plan was built from
struct SlotKey {
  u64 pat_ada, pat_a, pat_q;                   // interned patterns of ADA', At and DAt.q (0: not part of this gateway's plan)
  std::vector<sdm_int> ints;                   // m first, then the scalar and small-vector arguments (cone, block starts)
  const sdm_int *split;                        // Ajc1 / Ajc2, m entries (null: none)
  const double *apr; sdm_int napr;             // the values of At (null: the plan does not hold At)
};
struct AdaSlot {
  sdm_plan *plan = nullptr;
  bool built = false;
  u64 pat_ada = 0, pat_a = 0, pat_q = 0;
  Finger apr;
  std::vector<sdm_int> split, ints, perm;      // as in SlotKey; perm: the last permutation
  DevBuf<int> invperm;
  void drop() { if (plan) sdm_plan_destroy(plan); plan = nullptr; built = false; perm.clear(); invperm.release(); }
  void set_perm(const sdm_int *pm, sdm_int m) {
    if (vec_is(perm, pm, m) && invperm.p) return;
    gw_upload_invperm(invperm, pm, m);
    perm.assign(pm, pm + m);
  }
  // the cheap comparisons first: the content check of At's values is paid only when everything else matches
  bool built_from(const SlotKey &k) {
    return built && pat_ada == k.pat_ada && pat_a == k.pat_a && pat_q == k.pat_q && ints == k.ints &&
           (!k.split || vec_is(split, k.split, k.ints[0])) && (!k.apr || apr.same(k.apr, k.napr));
  }
};
AdaSlot g_s1, g_s2, g_s3, g_s0;

// whose ada_val holds the ADA values most recently handed back to the host, and what they were
struct { sdm_plan *plan = nullptr; Finger vals; bool zero = false; } g_last;   // zero: those values are known to be all zero (getada1 with nothing to add)
double *g_pin = nullptr;                // pinned staging for the solves' right-hand side and solution (sdm_mexcache_solve)
sdm_int g_pin_n = 0;
// ADA' values and absd of plan p -> the host arrays the shim returns, together with the checksum of the values summed on the device:
// the array at pr is, from now on, known to hold what p->ada_val holds
void download_returned(sdm_plan *p, double *pr, double *absd, sdm_int nnz) {
  wordsum_device(p, p->ada_val.p, nnz);
  gw_download(p, pr, absd);                                           // (drains the stream)
  g_last.plan = p; g_last.vals.take_with_full(pr, nnz, wordsum_device_result(nnz)); g_last.zero = false;
  g_tok.serial = 0;                                                   // real arrays went out: a token issued earlier is stale from here on (refused loudly)
}
// a gateway leaves its ADA' on the device and hands out a token for it (lazy mode)
double returned_token(sdm_plan *p, u64 pat, sdm_int m, sdm_int nnz) {
  SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
  g_last.plan = p; g_last.vals.forget(); g_last.zero = false;
  g_tok.serial = ++g_serial; g_tok.pat = pat; g_tok.m = m; g_tok.nnz = nnz;
  remember_token(g_tok.serial, pat, m, nnz);
  return LAZY_BASE + (double)g_tok.serial;
}
// what a getada gateway hands back: a token for the ADA' it leaves on the device (absd is real all the same), or the arrays
void hand_back(sdm_plan *p, u64 pat, sdm_int m, sdm_int nnz, double *ADApr, double *absd, double *token_out) {
  if (!token_out) { download_returned(p, ADApr, absd, nnz); return; }
  if (absd) gw_download(p, nullptr, absd);
  *token_out = returned_token(p, pat, m, nnz);
}
// the pattern id of the ADA' a token stands for.  TOKEN_CURRENT: throws unless it is the current token; TOKEN_LAST_16 (getada1.mex: pattern
// only): any of the last sixteen handed out
enum TokenAge { TOKEN_CURRENT, TOKEN_LAST_16 };
u64 token_pattern(double tok, sdm_int m, TokenAge age) {
  if (age == TOKEN_LAST_16) {
    if (is_token(tok)) {
      const u64 serial = (u64)(tok - LAZY_BASE);
      const TokRec &r = g_tok_hist[serial & 15];
      if (serial != 0 && r.serial == serial && r.m == m) return r.pat;
    }
    throw std::runtime_error("lazy ADA token is not one of the last sixteen handed out (SEDUMI_HIP_LAZY: getada1 needs the pattern behind the token it is given)");
  }
  if (!g_last.plan || !is_token(tok) || tok != LAZY_BASE + (double)g_tok.serial || g_tok.m != m)
    throw std::runtime_error("lazy ADA token is not the current one (SEDUMI_HIP_LAZY: the array a getada gateway returned must be handed to the next gateway untouched)");
  return g_tok.pat;
}
// ... and its host copy.  Looked up when the gateway's other patterns have been interned: an intern() may have pushed it out of g_pat
const Pattern &cached_pattern(u64 id) {
  const Pattern *pp = pattern_by_id(id);
  if (!pp || pp->irc.empty()) throw std::runtime_error("lazy ADA token: its pattern is not cached any more");
  return *pp;
}
// ADA' from the plan that holds it (g_last.plan) -> p->ada_val; counted as `stat`
void take_resident(sdm_plan *p, sdm_int nnz, int stat) {
  g_stat[stat]++;
  if (g_last.plan != p)
    SDM_HIP_CHECK(hipMemcpyAsync(p->ada_val.p, g_last.plan->ada_val.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
}
// the input values of a gateway -> p->ada_val: from the device if they are a token's, or what the previous gateway returned, else from the host
void ada_input(sdm_plan *p, bool token, const double *pr, sdm_int nnz) {
  if (token || (g_last.plan && g_last.vals.same(pr, nnz))) { take_resident(p, nnz, ST_ADA_RESIDENT); return; }
  g_stat[ST_ADA_UPLOAD]++;
  SDM_HIP_CHECK(hipMemcpyAsync(p->ada_val.p, pr, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, p->stream));
}
void forget_plan(sdm_plan *p) { if (g_last.plan == p) { g_last.plan = nullptr; g_last.vals.forget(); g_last.zero = false; g_tok.serial = 0; } }

// ---- the factorisation's plan
struct Chol {
  sdm_plan *plan = nullptr;
  u64 pat_l = 0, pat_x = 0;
  std::vector<sdm_int> perm, xsuper;
  bool have_factor = false;
  Finger lpr;
} g;

void drop_chol() {
  if (g.plan) { forget_plan(g.plan); sdm_plan_destroy(g.plan); }
  g.plan = nullptr; g.pat_l = g.pat_x = 0; g.perm.clear(); g.xsuper.clear(); g.have_factor = false; g.lpr.forget();
}
void drop_all() {
  for (AdaSlot *s : {&g_s1, &g_s2, &g_s3, &g_s0}) { if (s->plan) forget_plan(s->plan); s->drop(); }
  drop_chol();
  wordsum_shutdown();
  if (g_pin) { (void)hipHostFree(g_pin); g_pin = nullptr; g_pin_n = 0; }
  for (auto &p : g_pat) p = Pattern();
  for (auto &t : g_tok_hist) t = TokRec();
  g_fullsum_words = 0;
}
void at_exit_once() {
  // the cached plans own streams, events and device memory: they go before the HIP runtime's own exit handlers run (registered
  // by the first HIP call of the process -- at the latest the plan creation that precedes this -- so this one, registered after
  // them, runs first).  A plan left alive across process exit crashed there (r03g).
  static bool done = false;
  if (!done) { done = true; std::atexit([] { drop_all(); }); }
}

// the slot's plan for the call `k` describes: kept, or built again by `build` (which uploads At where the plan holds it)
template <class Build> void refresh(AdaSlot &S, const SlotKey &k, Build build) {
  if (S.built_from(k)) { g_stat[ST_ADA_REUSE]++; return; }
  if (!S.plan) S.plan = new_plan();
  at_exit_once();
  S.built = false; forget_plan(S.plan);
  g_stat[ST_ADA_BUILD]++;
  if (k.apr) g_stat[ST_AT_UPLOAD]++;
  build(S.plan);
  S.pat_ada = k.pat_ada; S.pat_a = k.pat_a; S.pat_q = k.pat_q; S.ints = k.ints;
  if (k.split) S.split.assign(k.split, k.split + k.ints[0]);
  if (k.apr) S.apr.take(k.apr, k.napr);
  S.perm.clear();                              // (getada1 / getada2: the new plan's triangle is filled by the next set_perm)
  S.built = true;
}

sdm_plan *chol_plan(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const sdm_int *perm, sdm_int nsuper, const sdm_int *xsuper,
                    const sdm_int *Xjc, const sdm_int *Xir, u64 px = 0) {
  const u64 pl = intern(m, Ljc, Lir);
  if (!px) px = intern(m, Xjc, Xir);
  if (g.plan && g.pat_l == pl && g.pat_x == px && vec_is(g.perm, perm, m) && vec_is(g.xsuper, xsuper, nsuper + 1)) { g_stat[ST_CHOL_REUSE]++; return g.plan; }
  drop_chol();
  g.plan = new_plan();
  at_exit_once();
  g_stat[ST_CHOL_BUILD]++;
  if (sdm_plan_set_chol(g.plan, m, Ljc, Lir, perm, nsuper, xsuper, Xjc, Xir)) { std::string e = sdm_last_error(); drop_chol(); throw std::runtime_error(e); }
  g.pat_l = pl; g.pat_x = px; g.perm.assign(perm, perm + m); g.xsuper.assign(xsuper, xsuper + nsuper + 1);
  return g.plan;
}
// a gateway's body: the shared try / catch, on the cache's device, with the shims' notes dropped however it ends
struct NotesScope { ~NotesScope() { drop_notes(); } };
#define MC_TRY SDM_TRY NotesScope notes_scope; SDM_HIP_CHECK(hipSetDevice(device()));
#define MC_CATCH SDM_CATCH
}  // namespace

extern "C" {

void sdm_mexcache_clear(void) { drop_all(); drop_notes(); }
void sdm_mexcache_forget_notes(void) { drop_notes(); }
// dst[0 .. n) = src[0 .. n) (8-byte words) and the content checksum of src in the same pass, noted for the gateway call that follows: the
// cache then does not read src a second time to check it (a shim copies the pattern of its input into the array it returns anyway)
unsigned long long sdm_mexcache_copy_words(void *dst, const void *src, sdm_int n) {
  u64 sum;
  if (n >= WORDSUM_POOL_FROM) { memcpy(dst, src, (size_t)n * 8); sum = wordsum_full(src, n); g_fullsum_words += n; }
  else sum = wordsum_copy(dst, src, n);
  if (g_nnotes < 4) g_notes[g_nnotes++] = Note{src, n, sum};
  return sum;
}
// the content checksum of n 8-byte words on the host (what residency is decided on; tests, and the bench's statement of its cost)
unsigned long long sdm_mexcache_checksum(const void *words, sdm_int n) { return wordsum_full(words, n); }
// on != 0: every presentation of every array is checksummed completely (no address is ever trusted) -- for callers that edit arrays
// IN PLACE between gateway calls of one iteration (sedumi.m never does); costs a pass over the host array per call
void sdm_mexcache_set_strict(int on) { strict = on != 0; }
void sdm_mexcache_stats(sdm_int *out, sdm_int n) {
  g_stat[11] = g_fullsum_words; g_stat[12] = (sdm_int)g_epoch;
  wordsum_host_time(&g_stat[13], &g_stat[14]);
  for (sdm_int i = 0; i < n && i < 16; i++) out[i] = g_stat[i];
}
// arrays of up to `words` words are checksummed completely at every presentation (default 65 536); larger ones once per address and epoch
void sdm_mexcache_set_full_below(sdm_int words) { full_below = words < 0 ? 0 : words; }
// lazy intermediates (the block comment at LAZY_BASE): level 0 | 1 | 2 (default); -1: as the environment variable SEDUMI_HIP_LAZY says (unset: 2)
void sdm_mexcache_set_lazy(int level) { g_lazy = level < 0 ? -1 : std::min(level, 2); }
int sdm_mexcache_lazy(void) { return lazy_level(); }
// m x m of the ADA' a token stands for and its number of nonzeros; returns 1 (with sdm_last_error) unless `token` is the current token
int sdm_mexcache_token_info(double token, sdm_int m, sdm_int *nnz) {
  SDM_TRY token_pattern(token, m, TOKEN_CURRENT); *nnz = g_tok.nnz; SDM_CATCH
}
// the pattern behind the current token into the caller's arrays (m + 1 and nnz entries)
int sdm_mexcache_token_pattern(double token, sdm_int m, sdm_int *jc_out, sdm_int *ir_out) {
  SDM_TRY
  const Pattern &P = cached_pattern(token_pattern(token, m, TOKEN_CURRENT));
  memcpy(jc_out, P.jcc.data(), P.jcc.size() * sizeof(sdm_int)); memcpy(ir_out, P.irc.data(), P.irc.size() * sizeof(sdm_int));
  SDM_CATCH
}
double sdm_mexcache_token_base(void) { return LAZY_BASE; }
// threads of the checksum of an array from 128K words on (the caller's included): -1 = automatic (4, and 8 from 1M words), 1 = none
void sdm_mexcache_set_threads(int n) { wordsum_set_threads(n); }

// ---- the cached getada gateways.  token_in != 0: the ADA' handed in is a lazy token (ADAjc / ADAir / ADApr_in may be NULL: the cache knows the
// pattern and the device has the values); token_out != NULL: the values stay on the device and *token_out stands for them (ADApr may be NULL)
// ADA = getada1(ADA, A, Ajc2, perm, d, blkstart) on the cache (same arguments as sdm_getada1)
int sdm_mexcache_getada1(sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, sdm_int N, const sdm_int *Ajc, const sdm_int *Air,
                         const double *Apr, const sdm_int *Ajc2, const sdm_int *perm, sdm_int lpN, const double *dl, sdm_int lorN,
                         const double *ddet, const sdm_int *qblkstart, double *ADApr, double token_in, double *token_out) {
  MC_TRY
  // (only the pattern of the input matters -- the result starts from zero, getada1.c:222-225 -- so a token that is no longer current will do)
  const u64 pa = token_in != 0.0 ? token_pattern(token_in, m, TOKEN_LAST_16) : intern(m, ADAjc, ADAir), pA = intern(m, Ajc, Air);
  if (token_in != 0.0) { const Pattern &P = cached_pattern(pa); ADAjc = P.jcc.data(); ADAir = P.irc.data(); }
  SlotKey key = {pa, pA, 0, {m, N, lpN, lorN}, Ajc2, Apr, Ajc[m]};
  key.ints.insert(key.ints.end(), qblkstart, qblkstart + lorN + 1);
  AdaSlot &S = g_s1;
  refresh(S, key, [&](sdm_plan *p) { gw_build_getada1(p, m, ADAjc, ADAir, Ajc, Air, Apr, Ajc2, lpN, lorN, qblkstart); });
  S.set_perm(perm, m);
  gw_run_getada1(S.plan, S.invperm.p, dl, ddet);
  hand_back(S.plan, pa, m, ADAjc[m], ADApr, nullptr, token_out);
  g_last.zero = gw_getada1_is_zero(S.plan);
  MC_CATCH
}

// ADA = getada2(ADA, DAt, Aord, K): ADApr_in the values of the input array, ADApr (out) those of the copy the shim returns
int sdm_mexcache_getada2(sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, const double *ADApr_in, double *ADApr, sdm_int lorN,
                         const sdm_int *Qjc, const sdm_int *Qir, const double *Qpr, const sdm_int *qperm, double token_in, double *token_out) {
  MC_TRY
  const u64 pa = token_in != 0.0 ? token_pattern(token_in, m, TOKEN_CURRENT) : intern(m, ADAjc, ADAir), pq = intern(m, Qjc, Qir);
  if (token_in != 0.0) { const Pattern &P = cached_pattern(pa); ADAjc = P.jcc.data(); ADAir = P.irc.data(); }
  const SlotKey key = {pa, 0, pq, {m, lorN}, nullptr, nullptr, 0};
  AdaSlot &S = g_s2;
  refresh(S, key, [&](sdm_plan *p) { gw_build_getada2(p, m, ADAjc, ADAir, lorN, Qjc, Qir); });
  S.set_perm(qperm, m);
  ada_input(S.plan, token_in != 0.0, ADApr_in, ADAjc[m]);
  g_last.zero = false;                                                // (Lorentz terms are being added)
  gw_run_getada2(S.plan, S.invperm.p, Qpr);
  hand_back(S.plan, pa, m, ADAjc[m], ADApr, nullptr, token_out);
  MC_CATCH
}
// [ADA, absd] = getada3(ADA, A, Ajc1, Aord, udsqr, K)
int sdm_mexcache_getada3(sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, const double *ADApr_in, double *ADApr, sdm_int N,
                         const sdm_int *Ajc, const sdm_int *Air, const double *Apr, const sdm_int *Ajc1, const double *udsqr,
                         const sdm_cone *K, const sdm_int *psd_blkstart, double *absd, double token_in, double *token_out) {
  MC_TRY
  const u64 pa = token_in != 0.0 ? token_pattern(token_in, m, TOKEN_CURRENT) : intern(m, ADAjc, ADAir), pA = intern(m, Ajc, Air);
  if (token_in != 0.0) { const Pattern &P = cached_pattern(pa); ADAjc = P.jcc.data(); ADAir = P.irc.data(); }
  SlotKey key = {pa, pA, 0, {m, N, K->lorN, K->sdpN, K->rsdpN}, Ajc1, Apr, Ajc[m]};
  key.ints.insert(key.ints.end(), K->sdpNL, K->sdpNL + K->sdpN);
  key.ints.insert(key.ints.end(), psd_blkstart, psd_blkstart + K->sdpN + (K->sdpN > 0 ? 1 : 0));
  AdaSlot &S = g_s3;
  refresh(S, key, [&](sdm_plan *p) { gw_build_getada3(p, m, ADAjc, ADAir, N, Ajc, Air, Apr, Ajc1, K, psd_blkstart); });
  const sdm_int up0 = g_stat[ST_ADA_UPLOAD];
  const bool was_zero = g_last.zero;
  ada_input(S.plan, token_in != 0.0, ADApr_in, ADAjc[m]);
  const bool zero_in = was_zero && g_stat[ST_ADA_UPLOAD] == up0;      // the device's ADA' was taken, and it is the zero matrix getada1 left
  g_last.zero = false;
  gw_run_getada3(S.plan, udsqr, zero_in);
  hand_back(S.plan, pa, m, ADAjc[m], ADApr, absd, token_out);
  MC_CATCH
}

// absd = getada(A, K, d, DAt) [global ADA_sedumi_]: the whole ADA' of a problem without PSD blocks (getada.m:13-40)
int sdm_mexcache_getada(sdm_int m, const sdm_int *ADAjc, const sdm_int *ADAir, sdm_int N, const sdm_int *Ajc, const sdm_int *Air,
                        const double *Apr, sdm_int lpN, const double *dl, sdm_int lorN, const double *ddet, const sdm_int *qblkstart,
                        const sdm_int *Qjc, const sdm_int *Qir, const double *Qpr, double *ADApr, double *absd) {
  MC_TRY
  const u64 pa = intern(m, ADAjc, ADAir), pA = intern(m, Ajc, Air), pq = lorN > 0 ? intern(m, Qjc, Qir) : 0;
  SlotKey key = {pa, pA, pq, {m, N, lpN, lorN}, nullptr, Apr, Ajc[m]};
  key.ints.insert(key.ints.end(), qblkstart, qblkstart + (lorN > 0 ? lorN + 1 : 0));
  AdaSlot &S = g_s0;
  refresh(S, key, [&](sdm_plan *p) { gw_build_getada(p, m, ADAjc, ADAir, Ajc, Air, Apr, lpN, lorN, qblkstart, Qjc, Qir); });
  gw_run_getada(S.plan, dl, ddet, Qpr);
  hand_back(S.plan, pa, m, ADAjc[m], ADApr, absd, nullptr);
  MC_CATCH
}

// [L.L, L.d, L.skip, L.add] = blkchol(L, X, pars, absd) on the cache (arguments of sdm_blkchol).  The factor stays resident for the solves.
int sdm_mexcache_blkchol(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const sdm_int *perm, sdm_int nsuper, const sdm_int *xsuper,
                         const sdm_int *Xjc, const sdm_int *Xir, const double *Xpr, const sdm_cholpars *pars, const double *absd,
                         double *Lpr, double *d, sdm_int *nskip, sdm_int *skip_idx, double *skip_val, sdm_int *nadd, sdm_int *add_idx,
                         double *add_val, double token_in) {
  // token_in != 0: X is a lazy token (level 2: Xjc / Xir / Xpr may be NULL)
  MC_TRY
  // X is what getada3 returned in the epoch that ends here: its values and pattern are looked at before the epoch advances
  const u64 px = token_in != 0.0 ? token_pattern(token_in, m, TOKEN_CURRENT) : intern(m, Xjc, Xir);
  if (token_in != 0.0) { const Pattern &P = cached_pattern(px); Xjc = P.jcc.data(); Xir = P.irc.data(); }
  const sdm_int nnzX = Xjc[m], nnzL = Ljc[m];
  const bool x_resident = token_in != 0.0 || (g_last.plan && g_last.vals.same(Xpr, nnzX));
  g_epoch++;                         // a new factor: every address trusted so far has to present its complete content again (file header)
  sdm_plan *p = chol_plan(m, Ljc, Lir, perm, nsuper, xsuper, Xjc, Xir, px);
  g.have_factor = false;             // the resident factor is about to be overwritten: whatever the solves are handed before this call has returned is not it
  if (x_resident) take_resident(p, nnzX, ST_X_RESIDENT);
  else {
    g_stat[ST_X_UPLOAD]++;
    SDM_HIP_CHECK(hipMemcpyAsync(p->ada_val.p, Xpr, (size_t)nnzX * sizeof(double), hipMemcpyHostToDevice, p->stream));
  }
  if (absd) SDM_HIP_CHECK(hipMemcpyAsync(p->absd.p, absd, (size_t)m * sizeof(double), hipMemcpyHostToDevice, p->stream));
  plan_ok(sdm_plan_blkchol_wait(p, pars, absd ? 1 : 0));   // (waited for, repeated once on the launch-per-panel path after a time-out)
  // L.L values, L.d and the fingerprint of the factor (summed on the device: no pass over the host copy) in one drain of the stream
  chol_extract(p, p->lpr.p);
  wordsum_device(p, p->lpr.p, nnzL);
  SDM_HIP_CHECK(hipMemcpyAsync(Lpr, p->lpr.p, (size_t)nnzL * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  SDM_HIP_CHECK(hipMemcpyAsync(d, p->chol.d.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  plan_ok(sdm_plan_pivots(p, nskip, skip_idx, skip_val, nadd, add_idx, add_val));   // (drains the stream)
  g.lpr.take_with_full(Lpr, nnzL, wordsum_device_result(nnzL));
  g.have_factor = true;
  MC_CATCH
}

// y = fwblkslv(L, b) / bwblkslv(L, b), dense b: on the resident factor when the L.L values handed over ARE the factor the last
// blkchol left on the device (content fingerprint), else stateless (sdm_fwblkslv / sdm_bwblkslv)
int sdm_mexcache_solve(int fw, sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const double *Lpr, const sdm_int *perm, sdm_int nsuper,
                       const sdm_int *xsuper, sdm_int nrhs, const double *b, double *y) {
  MC_TRY
  sdm_plan *p = sdm_mexcache_factor_plan(m, Ljc, Lir, Lpr, perm, nsuper, xsuper);
  if (!p) {
    g_stat[ST_SOLVE_STATELESS]++;
    plan_ok((fw ? sdm_fwblkslv : sdm_bwblkslv)(m, Ljc, Lir, Lpr, perm, nsuper, xsuper, nrhs, b, y));
    return 0;
  }
  g_stat[ST_SOLVE_RESIDENT]++;
  // right-hand side and solution travel through a pinned buffer: copies between pageable host memory and the device block the host once
  // each, and a solve of a small factor is two such copies around 10 us of kernels
  if (g_pin_n < 2 * m) {
    if (g_pin) (void)hipHostFree(g_pin);
    g_pin = nullptr; g_pin_n = 0;
    SDM_HIP_CHECK(hipHostMalloc((void **)&g_pin, (size_t)2 * m * sizeof(double), 0));
    g_pin_n = 2 * m;
  }
  for (sdm_int c = 0; c < nrhs; c++) {
    memcpy(g_pin, b + c * m, (size_t)m * sizeof(double));
    SDM_HIP_CHECK(hipMemcpyAsync(p->rhs.p, g_pin, (size_t)m * sizeof(double), hipMemcpyHostToDevice, p->stream));
    plan_ok(fw ? sdm_plan_fwsolve(p) : sdm_plan_bwsolve(p));
    SDM_HIP_CHECK(hipMemcpyAsync(g_pin + m, p->y.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    SDM_HIP_CHECK(hipStreamSynchronize(p->stream));
    memcpy(y + c * m, g_pin + m, (size_t)m * sizeof(double));
  }
  plan_ok(sdm_plan_sync(p));     // (time-out flags of the plan)
  MC_CATCH
}

// ---- the round-3 entry points, kept for callers that drive the cached plan themselves
sdm_plan *sdm_mexcache_plan(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const sdm_int *perm, sdm_int nsuper,
                            const sdm_int *xsuper, const sdm_int *Xjc, const sdm_int *Xir) {
  try { SDM_HIP_CHECK(hipSetDevice(device())); return chol_plan(m, Ljc, Lir, perm, nsuper, xsuper, Xjc, Xir); }
  catch (const std::exception &e) { set_error(e.what()); return nullptr; }
}
void sdm_mexcache_remember_factor(const double *Lpr_host, sdm_int nnz) {
  g_epoch++;                         // a (re)factorisation on this API too: no address stays trusted across it (file header)
  if (!g.plan || !Lpr_host || nnz != g.plan->chol.nnzL) { g.have_factor = false; return; }      // (NULL: invalidate -- a refactorisation is starting)
  g.have_factor = true;
  g.lpr.take(Lpr_host, nnz);
}
sdm_plan *sdm_mexcache_factor_plan(sdm_int m, const sdm_int *Ljc, const sdm_int *Lir, const double *Lpr, const sdm_int *perm,
                                   sdm_int nsuper, const sdm_int *xsuper) {
  if (!g.plan || !g.have_factor || !vec_is(g.xsuper, xsuper, nsuper + 1)) return nullptr;
  if (perm && !vec_is(g.perm, perm, m)) return nullptr;
  if (intern(m, Ljc, Lir) != g.pat_l) return nullptr;
  if (!g.lpr.same(Lpr, Ljc[m])) return nullptr;                          // content differs: not the resident factor
  return g.plan;
}

}  // extern "C"
