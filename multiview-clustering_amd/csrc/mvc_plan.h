// mvc_plan.h — which kernel instance runs for a state shape: the parallel
// schedule's path decisions, as plain host arithmetic (no HIP, no device code;
// compiles with g++ -std=c++17, tests/plan_driver.cpp).  The samplers plan,
// then launch from the plan; the kernels include this header
// for the constants and LDS size functions the decisions share with them.
//
//   PathOpts / parse_path_opts   the MVC_PATH keys, read once per sampler
//   PhaseAPlan / plan_phase_a    phase A: producer, draw, batch, geometry, the zpath mask
//   lane_layout .. run_wgrid     the repair's run-kernel LDS layout
//   RunInstance / run_instance   the run kernel's template mode, block and name
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#ifdef __HIP__
#define MVC_PLAN_HD __host__ __device__
#else
#define MVC_PLAN_HD
#endif

#define MVC_MAXV 64          // max views handled in LDS-resident scalars

// ---------------------------------------------------------------------------
// Phase A: limits and LDS sizes of the lp producers and the draws
// (mvc_parallel.hip)
// ---------------------------------------------------------------------------
#define MVC_Z_KMAX 64
#define MVC_Z_VMAX 8
#define MVC_ZR 8              // SP (k-steps per view) is padded to a multiple of this
#define MVC_ZD_NCP 16
#define MVC_ZSTAGE 24          // dishes per wave whose lp rows the register draw keeps in LDS (3 blocks/CU)

MVC_PLAN_HD inline size_t lpview_shared_bytes(int SP, int NT, int K, int T) {
  return 8 * ((size_t)SP * NT * 64 + 3 * (size_t)K + 8 * 48) + 4 * (2 * (size_t)K + 2 * (size_t)T + 8 * 16) + 64;
}
inline size_t lpbig_shared_bytes(int SP, int NTB, int T, int waves) {
  return 8 * ((size_t)SP * NTB * 64 + (size_t)waves * 48 + 48 * NTB) + 4 * (32 * NTB + 2 * (size_t)T + (size_t)waves * 16) + 64;
}
MVC_PLAN_HD inline size_t zdraw_shared_bytes(int V, int T, int sumK) {
  return 8 * ((size_t)MVC_ZD_NCP * 256 + (size_t)T) + 4 * ((size_t)V * T + (size_t)sumK + (size_t)V + 1) + 64;
}
MVC_PLAN_HD inline size_t zdraw_reg_shared_bytes(int V, int TM, int sumK) {
  return 8 * ((size_t)TM + (size_t)sumK + (size_t)4 * MVC_ZSTAGE * 64) +
         4 * ((size_t)V * TM + (size_t)V + 1 + 2 * MVC_Z_VMAX + (size_t)sumK) + 16;
}
MVC_PLAN_HD inline size_t zdraw_row_shared_bytes(int V, int NB, int sumK, bool lds) {
  return 8 * ((size_t)16 * NB + 256 + (lds ? (size_t)16 * sumK : 0)) +
         4 * ((size_t)16 * NB * V + (size_t)V + 1 + (size_t)sumK) + 16;
}

// View patterns (compile-time per-view dish-block counts) of the all-views
// producer: bits 0-3 = V, bits 4 + 2 v .. = NT_v - 1 (dish blocks of 16
// in view v).  Views run in order, unrolled at compile time, so a tile is
// straight-line code (no joins between views with different NT, which cost
// the register allocator ~60 VGPRs).  Instances: the bench's K_v = 64, 32,
// 16, 8 and configs[1]'s 16, 8 shapes, every view count <= 4 with a common
// dish-block count of 1 or 2, and up to two views of 4 blocks.
#define MVC_FZ_TB 4               // table blocks of 16 (T <= 64)
#define MVC_FZ_PAT(V, n0, n1, n2, n3) ((V) | (((n0) - 1) << 4) | (((n1) - 1) << 6) | (((n2) - 1) << 8) | (((n3) - 1) << 10))
#define MVC_FZ_PATS(X)                                                                                     \
  X(MVC_FZ_PAT(4, 4, 2, 1, 1)) X(MVC_FZ_PAT(3, 4, 2, 1, 1)) X(MVC_FZ_PAT(2, 4, 2, 1, 1))                  \
  X(MVC_FZ_PAT(2, 2, 1, 1, 1)) X(MVC_FZ_PAT(1, 1, 1, 1, 1)) X(MVC_FZ_PAT(2, 1, 1, 1, 1))                  \
  X(MVC_FZ_PAT(3, 1, 1, 1, 1)) X(MVC_FZ_PAT(4, 1, 1, 1, 1)) X(MVC_FZ_PAT(1, 2, 2, 2, 2))                  \
  X(MVC_FZ_PAT(2, 2, 2, 2, 2)) X(MVC_FZ_PAT(3, 2, 2, 2, 2)) X(MVC_FZ_PAT(4, 2, 2, 2, 2))                  \
  X(MVC_FZ_PAT(1, 4, 4, 4, 4)) X(MVC_FZ_PAT(2, 4, 4, 4, 4)) X(MVC_FZ_PAT(3, 2, 1, 1, 1))

#ifndef MVC_LPA_WAVES
#define MVC_LPA_WAVES 8       // waves per block (one block per CU) of the all-views producer
#endif
#ifndef MVC_LPA_RP16
#define MVC_LPA_RP16 8        // ring depth (k-step pairs in flight per wave) at D = 128
#endif
// Per-wave LDS of the all-views producer: the tile's y2 and h = (-y2/2)/tau
// per (view, row), the own-dish G and the max over the other included dishes
// per (view, row) [4][16] each, and the rows' tables [16].
constexpr int kLpaWaveD = 4 * 4 * 16;   // doubles
constexpr int kLpaWaveI = 16;           // ints
MVC_PLAN_HD inline size_t lpall_shared_bytes(size_t s1t_doubles, int V, int sumK, int waves) {
  return 16 * 4 + 8 * (s1t_doubles + 6 * (size_t)sumK + (size_t)waves * kLpaWaveD) +
         4 * (2 * (size_t)sumK + (size_t)MVC_FZ_TB * 16 * V + MVC_FZ_TB * 16 + (size_t)waves * kLpaWaveI) + 64;
}

// ---------------------------------------------------------------------------
// The repair (mvc_repair.h): block shapes, limits, the run kernel's LDS layout
// ---------------------------------------------------------------------------
constexpr int32_t kSeqScan = 0, kSeqRun = 1;
// run kernel block: 8 waves (256 VGPRs each: the per-customer evaluation
// spills at the 128 VGPRs of a 16-wave block)
constexpr int kSeqRunThreads = 512, kSeqRunWaves = kSeqRunThreads / 64;
// the lane-column run kernel: 4 waves, one per SIMD (its evaluation is issue-
// bound; a second wave per SIMD would halve the first customer's rate)
constexpr int kSeqLcThreads = 256;
// the small chains' lane loop (mvc_seq_run_kernel<5>): 8 waves, two per SIMD,
// 64 customers per step (its registers allow it; the general lane kernel <6>
// and the lane-column kernels keep 4 waves)
constexpr int kLaneSmallThreads = 512;
constexpr int kVpMoves = 4, kVpV = 8, kVpE = kVpMoves * kVpV * 2;
constexpr int kLcChunks = 8;   // tables <= 512 (block totals in lanes b < 64 need TB <= 64)
constexpr int kNoWindows = 1 << 29;   // a limit this large: the run kernel never hands over to windows
constexpr int kWideGridThreads = 256;
constexpr int kLanePre = 64;   // 2V + 2 + T <= 64 (V <= 8, T < 32)
constexpr int kLaneSmall = 8;

constexpr int kParTC = 1 << 18;   // table capacity (three-level tree64 of the MH's global EPPF)
constexpr int kParKC = (1 << 18) - 1;   // live dishes per view (+1 new element: three-level tree64)
constexpr size_t kLpbBudget = (size_t)1 << 28;   // phase-1 lp buffer: 2 GiB of doubles per batch
constexpr int kSeqWaves = 1024;    // waves of the repair eval grid (SeqArgs.G)
constexpr int kSeqWmin = 1024;     // repair window after a mover
constexpr int kSeqWmax = 1 << 16;  // cap of the window doubling over mover-free stretches
constexpr int kSeqRunLimit = 64;   // stays in a row after which the run kernel hands over to grid windows
constexpr size_t kSeqLdsBudget = 150 * 1024;   // run kernel: per-wave LDS scratch of all its waves
// the lane-per-customer loop of small chains (mvc_seq_run_kernel<5>): customers,
// dims, tables (its evaluation's registers) and dishes per view it takes on
constexpr int kLaneMaxN = 1024, kLaneMaxD = 16, kLaneMaxV = 8, kLaneTM = 32, kLaneMaxK = 32;   // (V: one view per lane of 8)
constexpr int kWideGridMax = 256;  // grid-wide evaluation: at most this many blocks per customer
constexpr int kWideBatch = 32;     // grid-wide evaluation: customers (lp + fin pairs) per repair round
constexpr int kWideFinLds = 152 * 1024;   // the fin kernel's dynamic LDS (wide_fin_resample: dish list, block totals)

// LDS layout of the run kernel's per-wave scratch (host-chosen at launch):
// lp [V][ks] | e [ts + 16] | B, C [ts/16 + 2]; nws waves speculate.
// lds = 0: the per-wave global scratch (SeqArgs.scr) instead.
// LDS of the run kernel: the state cache (SCache: n_t [ts], dish [V][ts],
// d_l, d_n [V][ks], Klist, Ltot [V], T, T_ne; c0, cb, Q, xm, ym, cbm [V][ks];
// lmass [ts]; S1T [V][D][ks] when s1) and the per-wave scratch (SeqScratch).
struct SeqLds {
  int32_t lds, nws, ks, ts;
  int32_t limit;        // stays in a row after which the run kernel hands over to the grid windows
  int32_t s1;           // S1 cached in LDS
  int64_t cache_dbl;    // doubles of the state cache (the per-wave scratch follows)
  int64_t stride;       // doubles per wave
  int32_t ring;         // customers in the staged-row ring (power of 2, after the per-wave scratch; 0: none)
  int32_t pfn;          // customers prefetched into the ring per step
  int32_t tw;           // waves per customer (1: seq_resample; kSeqRunWaves: seq_resample_wide); nws customers per step
  int32_t lc;           // 1: the lane-column evaluation (seq_resample_lc; LDS layout with S1 cached, ts <= 512); 2: + value prediction
  int64_t vpo;          // lc == 2: offset (doubles) of the overlay's S1 columns [kVpE][D] in the dynamic LDS
  int64_t dyn;          // bytes of dynamic LDS of the launch
  int32_t small;        // lc == 3: every dish list and the tables <= kLaneSmall (mvc_seq_run_kernel<5>)
  int32_t fill;         // MVC_LDS_FILL diagnostics: >= 0 fills the block's LDS with this byte at launch
  int32_t chk;          // MVC_RUN_CHECK diagnostics: check every index a commit writes through (R->dbg)
};

// ring slot: y rows [V][D], Y2 [V], z (as a double)
MVC_PLAN_HD inline int64_t seq_ring_slot(int V, int D) { return (int64_t)V * D + V + 1; }

// lp row stride of the LDS scratch: the lane-column evaluation stores dish j
// of a row at j + j / 32 (lc_lpx), so the table gathers of dishes j and j + 32
// (the same bank of ds_read_b64 otherwise) fall on different banks
MVC_PLAN_HD inline int seq_lps(int ks) { return ks + (ks >> 5) + 1; }
MVC_PLAN_HD inline int64_t seq_lds_stride(int V, int D, int ks, int ts) {
  // lp [V][seq_lps] | aux [V][ks] | e | B, C | mv | koff | ys [V][D] + Y2 [V] + lm_v [V] + member maxima [4]
  return (int64_t)V * seq_lps(ks) + (int64_t)V * ks + ts + 16 + ts / 16 + 2 + V + V + 2 + (int64_t)V * D + V + V + 4;
}
MVC_PLAN_HD inline int64_t seq_lds_cache(int V, int D, int ks, int ts, bool s1) {
  const int64_t ints = (int64_t)ts + (int64_t)V * ts + 2 * (int64_t)V * ks + 2 * V + 2;
  return (ints + 1) / 2 + 7 * (int64_t)V * ks + ts + (s1 ? (int64_t)V * D * ks : 0);
}

namespace mvc {

// ---------------------------------------------------------------------------
// MVC_PATH: the execution-path overrides of the tests and A/B runs, one
// variable of comma-separated key=value items (e.g. "lc=0,waves=3").  Every
// key selects a path that is bitwise the default's and is pinned by a test
// (the table of DESIGN.md §9; one field per key below).  Unknown keys are
// ignored and spaces are not trimmed.
// ---------------------------------------------------------------------------
// The value of key in s into out (the first item that names it), false when
// it is not set.
inline bool path_opt(const char *s, const char *key, char *out, size_t cap) {
  const size_t kl = strlen(key);
  while (s) {
    const char *end = strchr(s, ',');
    const size_t len = end ? (size_t)(end - s) : strlen(s);
    const char *eq = (const char *)memchr(s, '=', len);
    if (eq && (size_t)(eq - s) == kl && memcmp(s, key, kl) == 0) {
      const size_t vl = std::min(len - kl - 1, cap - 1);
      memcpy(out, eq + 1, vl);
      out[vl] = 0;
      return true;
    }
    s = end ? end + 1 : nullptr;
  }
  return false;
}
inline int path_int(const char *s, const char *key, int dflt) {   // the value as an int, dflt when unset or empty
  char v[32];
  return (path_opt(s, key, v, sizeof v) && v[0]) ? atoi(v) : dflt;
}

struct PathOpts {
  bool force_generic = false;     // generic=1: the generic lp producer
  bool force_zdraw_lds = false;   // zdraw=lds: the LDS-checkpoint draw kernel for every T
  bool force_zdraw_row = false;   // zdraw=row*: the row draw for every T <= 512 (default: 64 < T <= 512)
  bool no_zrow_lds = false;       // zdraw=row-global: the row draw reads the lp buffer directly
  bool no_lpall = false;          // lpall=0: per-view producer launches even where the all-views producer applies
  bool force_big = false;         // big=1: the dish-block producer even where the tiled one applies
  bool big_runtime_sp = false;    // big_sp=runtime: the dish-block producer's runtime k-step loop only
  bool big_group = true;          // big_group=0: one launch per dish block (y re-read per block) instead of the XCD-grouped launch
  bool repair_grid_only = false;  // repair=grid: every mover through a grid window round (no run kernel)
  // waves=N: customers the run kernel evaluates per step.  4 by default:
  // one evaluating wave per SIMD (a second wave on a SIMD halves the first
  // customer's issue rate, and with dense movers the first customer decides)
  int run_waves = 4;
  bool use_lc = true;             // lc=0: the run kernel's per-wave evaluation without the lane-column form
  bool use_lane = true;           // lc=col: no lane-per-customer loop for small chains (lane columns instead)
  bool use_vp = true;             // vp=0: the lane-column kernel without value prediction
  bool vp_stats = false;          // vp_stats=1: value prediction's steps and hits per sweep on stderr
  // Small chains (n <= small_n_plain, small_plain=N): the lane-column loop without value
  // prediction and a stay limit of 16. At the reference's own call (N = 200, V = 5) the
  // prediction waves' overlay evaluation costs more per step than the steps it saves
  // (1,578 -> 2,262 sweeps/s, profiles/r5af_*); at N = 1M (the literal) it is worth 1.5x.
  int small_n_plain = 1024;
  bool force_global = false;      // run_lds=0: the run kernel's global-scratch layout
  bool use_wide = true;           // wide=0: global-scratch run kernel speculates one customer per wave
  bool wide_grid = true;          // wide=block: the wide evaluation on the run kernel's one block instead of the grid
  int wide_fin_lds = kWideFinLds; // the fin kernel's LDS evaluation up to this many bytes (wide_fin=0: off)
  int max_tables = kParTC;        // max_tables=N: a lower table limit (the limit's error)
  bool chain_batch = true;        // chain_batch=0: one host thread per chain, on its own stream unless the chains are small (n <= kLaneMaxN: chain 0's)
  bool chain_threads = true;      // chain_threads=0: one handle runs its chains one after another
  int exact_lds = 2;              // exact_lds=0/1/2: caps the exact kernel's storage instance
};

inline PathOpts parse_path_opts(const char *s) {
  PathOpts o;
  char e[32];
  o.force_generic = path_int(s, "generic", 0) == 1;
  if (path_opt(s, "zdraw", e, sizeof e)) {
    o.force_zdraw_lds = strcmp(e, "lds") == 0;
    o.force_zdraw_row = strncmp(e, "row", 3) == 0;
    o.no_zrow_lds = strcmp(e, "row-global") == 0;
  }
  o.no_lpall = path_int(s, "lpall", 1) == 0;
  if (path_int(s, "wide_fin", 1) == 0) o.wide_fin_lds = 0;   // the global-scratch evaluation
  if (path_opt(s, "repair", e, sizeof e)) o.repair_grid_only = strcmp(e, "grid") == 0;
  o.force_big = path_int(s, "big", 0) == 1;
  o.big_runtime_sp = path_opt(s, "big_sp", e, sizeof e) && strcmp(e, "runtime") == 0;
  o.big_group = path_int(s, "big_group", 1) != 0;
  o.run_waves = std::max(1, std::min(kSeqRunWaves, path_int(s, "waves", o.run_waves)));
  if (path_opt(s, "lc", e, sizeof e)) {   // 0: neither lane-column nor lane loop; col: lane columns only
    o.use_lc = e[0] != '0';
    o.use_lane = o.use_lc && e[0] != 'c';
  }
  o.use_vp = path_int(s, "vp", 1) != 0;
  o.small_n_plain = path_int(s, "small_plain", o.small_n_plain);
  o.vp_stats = path_int(s, "vp_stats", 0) == 1;
  if (path_opt(s, "wide", e, sizeof e)) {
    o.use_wide = e[0] != '0';
    o.wide_grid = e[0] != 'b';
  }
  o.force_global = path_int(s, "run_lds", 1) == 0;
  o.max_tables = std::max(16, std::min(kParTC, path_int(s, "max_tables", kParTC)));
  o.chain_batch = path_int(s, "chain_batch", 1) != 0;
  o.chain_threads = path_int(s, "chain_threads", 1) != 0;
  if (path_opt(s, "exact_lds", e, sizeof e) && e[0] >= '0' && e[0] <= '2') o.exact_lds = e[0] - '0';
  return o;
}
// MVC_PATH as it is now: every sampler calls this once, when it is created
inline PathOpts parse_path_opts() { return parse_path_opts(getenv("MVC_PATH")); }

// ---------------------------------------------------------------------------
// The shape the decisions depend on: plain data, filled per sweep
// ---------------------------------------------------------------------------
struct Shape {
  int n = 0, V = 0, D = 0;
  int SP = 0;                  // k-steps per view of the tiled copy of y (0: no tiled copy)
  bool s1t_ok = false;         // the chain's S1 tiling is current
  int T = 0;
  int32_t K[MVC_MAXV] = {};    // dishes per view
  int n_cu = 256;
  int64_t lo = 0, hi = 0;      // this rank's customers [lo, hi) (the whole chain unless sharded)
  bool sharded = false;        // within-chain N-sharding with more than one rank
  bool phase_a_only = false;   // the sweep stops after phase A (mvc_sampler_phase_a)
};

// ---------------------------------------------------------------------------
// The repair's run-kernel layout
// ---------------------------------------------------------------------------
// The small chains' lane-per-customer loop (mvc_seq_run_kernel<5>, L.lc ==
// 3): the state cache with S1, tables up to kLaneTM (the evaluation's
// registers), dish lists with room to double, and a ring holding the whole
// sweep's rows; no per-wave scratch.  L.lc == 0: it does not fit.
inline SeqLds lane_layout(const Shape &s, int T, const int32_t *Klist) {
  const int n = s.n, V = s.V, D = s.D;
  int kmax = 1;
  for (int v = 0; v < V; ++v) kmax = std::max(kmax, (int)Klist[v]);
  SeqLds L{};
  L.limit = kNoWindows;
  L.ks = (kmax + std::max(16, kmax) + 15) / 32 * 32 + 16;
  L.ts = kLaneTM;
  L.s1 = 1;
  L.cache_dbl = seq_lds_cache(V, D, L.ks, L.ts, true);
  L.stride = 0;
  L.nws = kSeqLcThreads / 64;
  int rn = 2;
  while (rn < n) rn *= 2;
  if (T >= L.ts || 8 * (L.cache_dbl + (int64_t)rn * seq_ring_slot(V, D)) > (int64_t)kSeqLdsBudget) return L;
  L.lds = 1;
  L.tw = 1;
  L.ring = rn;
  L.pfn = 0;
  L.vpo = 0;
  L.lc = 3;
  L.small = (T <= kLaneSmall && kmax <= kLaneSmall) ? 1 : 0;
  return L;
}
// whether a sweep from the state s.T, s.K runs the lane loop from customer 0
inline bool lane_sweep(const Shape &s, const PathOpts &o) {
  if (!o.use_lane || o.force_global || o.repair_grid_only || s.phase_a_only || s.sharded) return false;
  if (s.n > kLaneMaxN || s.D > kLaneMaxD || s.V > kLaneMaxV || s.T >= kLaneTM) return false;
  for (int v = 0; v < s.V; ++v)
    if (s.K[v] > kLaneMaxK) return false;
  return lane_layout(s, s.T, s.K).lc == 3;
}

// LDS layout of the run kernel's per-wave scratch for T tables and dish
// lists Klist, with room for growth (a birth past it makes the kernel exit
// with R->restride; the host then relaunches with a new layout).  Falls back
// to the per-wave global scratch when even a few waves do not fit.
inline SeqLds run_layout(const Shape &s, const PathOpts &o, int T, const int32_t *Klist, bool vp_ok = true) {
  const int n = s.n, V = s.V, D = s.D;
  int kmax = 1;
  for (int v = 0; v < V; ++v) kmax = std::max(kmax, (int)Klist[v]);
  SeqLds L{};
  // small chains: the run kernel walks the whole sweep (a window round is a
  // launch triple and a host read-back, more than the steps it saves)
  L.limit = n <= o.small_n_plain ? 16 : kSeqRunLimit;
  // in order of preference: S1 cached with room to double (a cold sweep's
  // births then rarely restride; in a chain batch a restride ends the round
  // for every chain), S1 cached with room to grow by half, then without S1,
  // then tight margins without S1
  for (int attempt = o.force_global ? 4 : 0; attempt < 4; ++attempt) {
    const bool s1 = attempt <= 1;
    const int kgrow = attempt == 0 ? std::max(16, kmax) : attempt < 3 ? std::max(8, kmax / 2) : 4;
    const int tgrow = attempt == 0 ? std::max(128, T) : attempt < 3 ? std::max(64, T / 2) : 16;
    // ks = 16 (mod 32): the lane-column evaluation's rows (views) read dish
    // j of [v][ks] arrays at v ks + j, so rows 0 / 1 (and 2 / 3) of a
    // ds_read_b64 lane group then fall on disjoint banks (2 ks dwords = 32
    // mod 64), and of a ds_read_b32 too (ks = 16 mod 32)
    L.ks = (kmax + kgrow + 15) / 32 * 32 + 16;
    L.ts = (T + tgrow + 63) / 64 * 64;   // whole 64-table chunks (the lane-column evaluation's e[] scratch)
    if (attempt == 0 && o.use_lc && L.ts > 64 * kLcChunks) continue;   // doubling would leave the lane-column form
    L.s1 = s1 ? 1 : 0;
    L.cache_dbl = seq_lds_cache(V, D, L.ks, L.ts, s1);
    L.stride = seq_lds_stride(V, D, L.ks, L.ts);
    const int64_t room = (int64_t)kSeqLdsBudget / 8 - L.cache_dbl;
    const int cap = o.run_waves;   // customers per step
    L.nws = room > 0 ? (int)std::min<int64_t>(cap, room / L.stride) : 0;
    if (L.nws >= std::min(cap, s1 ? 4 : 2)) {
      L.lds = 1;
      L.tw = 1;
      L.lc = 0;   // the lane-column kernel needs the ring (set below)
      // the staged-row ring in what is left: a power of two >= 2 nws customers
      const int64_t slot = seq_ring_slot(V, D);
      const int64_t left = room - (int64_t)L.nws * L.stride;
      int rn = 0;
      for (int r = 256; r >= 2 * L.nws; r >>= 1)
        if ((int64_t)r * slot <= left) { rn = r; break; }
      L.ring = rn;
      L.pfn = rn ? std::max(1, rn / 2) : 0;
      L.lc = (o.use_lc && s1 && rn > 0 && L.ts <= 64 * kLcChunks) ? 1 : 0;
      if (L.lc) L.nws = std::min(L.nws, kSeqLcThreads / 64);   // its block has 4 waves
      // value prediction (lc == 2) where its overlay fits: V <= kVpV, every dish list <= 128, and the
      // overlay's S1 columns [kVpE][D] after the ring (which follows the clamped nws scratches)
      L.vpo = L.cache_dbl + (int64_t)L.nws * L.stride + (int64_t)rn * slot;
      if (L.lc && o.use_vp && vp_ok && n > o.small_n_plain && V <= kVpV && kmax <= 128 && L.nws >= kSeqLcThreads / 64 &&
          left - (int64_t)rn * slot >= (int64_t)kVpE * D)
        L.lc = 2;
      return L;
    }
  }
  L.lds = 0;   // per-wave global scratch (SeqScratch(A, w)): capacity-sized, never restrides
  L.lc = 0;
  // the whole block on one customer (seq_resample_wide): the dish / table
  // lists are long here, and where the state outgrows the LDS nearly every
  // customer moves (cold-start transients), so speculation buys little
  L.tw = o.use_wide ? kSeqRunWaves : 1;
  L.s1 = 0;
  L.nws = o.use_wide ? 1 : o.run_waves;
  L.stride = 0;
  L.cache_dbl = 0;
  return L;
}
// the layout of a repair round: the lane loop while this sweep runs it
// (lane_now) and the state still fits it, else the run kernels' (run_layout)
inline SeqLds pick_layout(const Shape &s, const PathOpts &o, bool lane_now, int T, const int32_t *Klist, bool vp_ok) {
  if (lane_now) {
    bool ok = T < kLaneTM;
    for (int v = 0; v < s.V; ++v) ok = ok && Klist[v] <= kLaneMaxK;
    if (ok) {
      const SeqLds L = lane_layout(s, T, Klist);
      if (L.lc == 3) return L;
    }
  }
  return run_layout(s, o, T, Klist, vp_ok);
}
// The run kernel's dynamic LDS for layout L.
inline int64_t run_dyn(int V, int D, const SeqLds &L) {
  return L.lds ? 8 * (L.cache_dbl + L.stride * L.nws + (int64_t)L.ring * seq_ring_slot(V, D) +
                      (L.lc == 2 ? (int64_t)kVpE * D : 0))
               : 0;
}
// The grid-wide evaluation where the state is on the global layout (L.lds = 0) and
// the block-wide evaluation applies (L.tw > 1): one customer over many CUs
inline bool run_wgrid(const PathOpts &o, const SeqLds &L) {
  return !o.repair_grid_only && o.wide_grid && L.lds == 0 && L.tw > 1;
}

// The run kernel of layout L: mvc_seq_run_kernel<mode> (batched:
// mvc_seq_run_kernel_b<mode>), its block and its name in diagnostics.  Modes:
// 5 / 6 the lane loop (small / general), 4 / 3 lane columns (with / without
// value prediction), 0 one wave per customer, 2 the block-wide evaluation on
// the global scratch.  A chain batch runs the small lane loop in the general
// instance <6>, whose births commit in the kernel (<5> ends its launch at a
// birth, which would end the round for every chain of the batch).
struct RunInstance {
  int mode, threads;
  const char *name;
};
inline RunInstance run_instance(const SeqLds &L, bool batched) {
  if (L.lc == 3) {
    if (L.small && !batched) return {5, kLaneSmallThreads, "seq_run<5>"};
    return {6, kSeqLcThreads, "seq_run<6>"};
  }
  if (L.lc == 2) return {4, kSeqLcThreads, "seq_run<4>"};
  if (L.lc) return {3, kSeqLcThreads, "seq_run<3>"};
  if (L.tw == 1) return {0, kSeqRunThreads, "seq_run<0>"};
  return {2, kSeqRunThreads, "seq_run<2>"};
}

// ---------------------------------------------------------------------------
// Phase A: the lp producer and the draw of a sweep
// ---------------------------------------------------------------------------
// bits of mvc_sampler_zpath (include/mvc.h)
enum : int {
  kZpTiled = 2, kZpDrawReg = 4, kZpAllViews = 16, kZpNoPhaseA = 32, kZpDishBlock = 64, kZpDrawRow = 128, kZpLane = 256
};
constexpr int kZpathLane = kZpNoPhaseA | kZpLane;   // a lane sweep: no phase-A launches

struct PhaseAPlan {
  bool lane = false;     // the lane loop runs the whole sweep from customer 0 (its first step is phase A)
  bool run = false;      // phase A runs; else the repair's eval kernel evaluates the sweep from customer 0
  int n_cu = 0;
  int64_t lo = 0, hi = 0;
  size_t batch = 0;      // customers per batch: a multiple of 64, lp buffer <= kLpbBudget doubles
  size_t lpb_need = 0;   // doubles of the lp buffer
  int sumK = 0;
  enum Producer { kGeneric, kAllViews, kPerView, kDishBlock } producer = kGeneric;
  enum Draw { kCheckpoint, kReg, kRow } draw = kCheckpoint;
  // all-views / per-view producers: k-step pairs per tile (the SPP instance)
  int spp = 0;
  uint32_t fz_pat = 0;   // all-views: the view pattern (MVC_FZ_PATS)
  size_t lpa_lds = 0;
  // dish-block producer: k-steps, and the unrolled instance where D = 4 SP exactly (0: the runtime loop)
  int SPb = 0, spc = 0;
  struct View {
    int nt = 0;          // per-view: dish blocks of 16
    int ntb = 0, waves = 0, nblk = 0;   // dish-block: block width / 16, waves per block, blocks of the view
    bool grouped = false;               // every dish block of the view in one XCD-grouped launch (y read once)
    int per_cu = 0;      // blocks per CU
    size_t lds = 0;
  } view[MVC_MAXV];
  int reg_tm = 0;        // register draw: its table instance, 16 / 32 / 64
  int row_nb = 0;        // row draw: table blocks
  bool row_lds = false;  // row draw: its slab in LDS (two blocks per CU)
  size_t draw_lds = 0;
  bool first_in_draw = false;   // the register draw finds the first mover itself when it sees every customer (no shard)

  // grid of view v's producer launch (all-views, generic: v ignored; grouped
  // dish blocks: every batch the same) for a batch of nb customers
  int producer_grid(int v, int nb) const {
    const int ntile = (nb + 15) / 16;
    switch (producer) {
      case kAllViews: return std::max(1, std::min(n_cu, (ntile + MVC_LPA_WAVES - 1) / MVC_LPA_WAVES));
      // waves per block of the per-view producer: 4, two blocks per CU = 2 waves per
      // SIMD.  Measured (scripts/lpv_sweep.py, D = 128, K = 64/32/16/8): more
      // waves per SIMD only contend for the f64 MFMA pipe and the load queue
      // (lp 1.11 ms at 4x2, 1.12 at 4x3 / 4x4, 1.22 at 6x2, 1.36 at 2x4).
      case kPerView: return std::max(1, std::min(view[v].per_cu * n_cu, (ntile + 4 - 1) / 4));
      case kDishBlock:
        if (view[v].grouped) return view[v].per_cu * n_cu;
        return std::max(1, std::min(view[v].per_cu * n_cu, (ntile + view[v].waves - 1) / view[v].waves));
      default: return std::min(4096, (nb + 255) / 256);
    }
  }
  int producer_threads(int v) const {
    return producer == kAllViews ? 64 * MVC_LPA_WAVES : producer == kPerView ? 64 * 4 : producer == kDishBlock ? 64 * view[v].waves : 256;
  }
  int draw_grid(int nb) const {
    switch (draw) {
      case kReg: return (nb + 255) / 256;   // the register kernel takes one customer per thread
      case kRow: return std::max(1, std::min((nb + 15) / 16, (row_lds ? 2 : 8) * n_cu));   // 16 customers (one slab) per block and round
      default: return std::min(4096, (nb + 255) / 256);
    }
  }
  // mvc_sampler_zpath: the one place the mask is formed
  int zpath() const {
    if (lane) return kZpathLane;
    if (!run) return kZpNoPhaseA;
    return (producer == kAllViews || producer == kPerView ? kZpTiled : 0) | (draw == kReg ? kZpDrawReg : 0) |
           (producer == kAllViews && lo < hi ? kZpAllViews : 0) | (producer == kDishBlock ? kZpDishBlock : 0) |
           (draw == kRow ? kZpDrawRow : 0);
  }
};

inline PhaseAPlan plan_phase_a(const Shape &s, const PathOpts &o) {
  PhaseAPlan p;
  p.n_cu = s.n_cu;
  p.lo = s.lo;
  p.hi = s.hi;
  // small chains: the run kernel's lane-per-customer loop runs the whole
  // sweep from customer 0 (its first step is phase A)
  p.lane = lane_sweep(s, o);
  if (p.lane) return p;
  const int n = s.n, V = s.V, D = s.D, SP = s.SP, T = s.T, n_cu = s.n_cu;
  // phase 1 in customer batches: lp producer (MFMA or generic), then draw
  int Kmax = 0, Kmin = 1 << 30, sk = 0;
  for (int v = 0; v < V; ++v) { Kmax = std::max(Kmax, (int)s.K[v]); Kmin = std::min(Kmin, (int)s.K[v]); sk += s.K[v]; }
  p.sumK = sk;
  const bool use_mfma = !o.force_generic && !o.force_big && s.s1t_ok && Kmin >= 1 && Kmax <= MVC_Z_KMAX &&
                        lpview_shared_bytes(SP, (Kmax + 15) / 16, Kmax, T) <= 160 * 1024;
  // the dish-block MFMA producer (y read directly) where the tiled path does
  // not apply: the widest dish block whose B-fragments fit, 8 waves per block
  // (one block per CU) when they take more than half the LDS, else 4 waves
  // and two blocks per CU -- two waves per SIMD either way
  const int SPb = ((D / 4 + MVC_ZR - 1) / MVC_ZR) * MVC_ZR;
  int big_ntb = 0, big_waves = 4;
  for (int nt : {4, 2, 1}) {
    if (big_ntb) break;
    if (lpbig_shared_bytes(SPb, nt, T, 4) <= 80 * 1024) { big_ntb = nt; big_waves = 4; }
    else if (lpbig_shared_bytes(SPb, nt, T, 8) <= 150 * 1024) { big_ntb = nt; big_waves = 8; }
  }
  const bool use_big = !use_mfma && !o.force_generic && D % 4 == 0 && D >= 16 && Kmin >= 1 && big_ntb > 0;
  // batch: multiple of 64 customers, lp buffer <= kLpbBudget doubles
  const size_t per64 = (size_t)std::max(1, sk) * 64;
  const size_t nb_max = std::max<size_t>(64, (kLpbBudget / per64) * 64);
  const size_t nb_full = ((size_t)n + 63) / 64 * 64;
  p.batch = std::min(nb_max, nb_full);
  p.lpb_need = (p.batch / 64) * per64;
  const bool use_zreg = !o.force_zdraw_lds && !o.force_zdraw_row && T <= 64 && Kmax <= 64 && sk <= MVC_Z_VMAX * 64 &&
                        zdraw_reg_shared_bytes(V, 64, sk) <= 64 * 1024;
  // the row draw (16 lanes per customer) where the register draw does not
  // apply; lane v of a customer's row holds view v's scalars, so V <= 16
  const int row_nb = T <= 64 ? 4 : T <= 128 ? 8 : T <= 256 ? 16 : 32;
  const bool use_zrow = !use_zreg && !o.force_zdraw_lds && T <= 512 && V <= 16 &&
                        zdraw_row_shared_bytes(V, row_nb, sk, false) <= 64 * 1024;
  // the row draw with its slab in LDS where two blocks fit a CU
  const bool zrow_lds = use_zrow && !o.no_zrow_lds && zdraw_row_shared_bytes(V, row_nb, sk, true) <= 80 * 1024;
  // phase A on the two-kernel path needs the draw's LDS tables; beyond them
  // the repair's eval kernel evaluates the sweep from customer 0 instead
  p.run = use_zreg || use_zrow || zdraw_shared_bytes(V, T, sk) <= 160 * 1024;
  if (use_zreg) {
    p.draw = PhaseAPlan::kReg;
    p.reg_tm = T <= 16 ? 16 : T <= 32 ? 32 : 64;
    p.draw_lds = zdraw_reg_shared_bytes(V, p.reg_tm, sk);
    p.first_in_draw = !s.sharded;
  } else if (use_zrow) {
    p.draw = PhaseAPlan::kRow;
    p.row_nb = row_nb;
    p.row_lds = zrow_lds;
    p.draw_lds = zdraw_row_shared_bytes(V, row_nb, sk, zrow_lds);
  } else {
    p.draw_lds = zdraw_shared_bytes(V, T, sk);
  }
  // the all-views producer: T <= 64, K_v <= 64, every view's S1
  // B-fragments in LDS at once, fully unrolled k-step pairs
  size_t s1t_d = 0;
  for (int v = 0; v < V; ++v) s1t_d += (size_t)SP * 64 * ((s.K[v] + 15) / 16);
  const int spp = SP / 2;
  uint32_t fz_pat = (uint32_t)V;
  for (int v = 0; v < V && v < 4; ++v) fz_pat |= (uint32_t)(std::min(4, (s.K[v] + 15) / 16) - 1) << (4 + 2 * v);
  bool pat_ok = V <= 4 && Kmax <= 64;
  switch (pat_ok ? fz_pat : 0u) {
#define X(p) case p:
    MVC_FZ_PATS(X)
#undef X
    break;
    default: pat_ok = false;
  }
  const size_t lpa_lds = lpall_shared_bytes(s1t_d, V, sk, MVC_LPA_WAVES);
  const bool use_lpall = !o.no_lpall && use_mfma && pat_ok && T <= 16 * MVC_FZ_TB &&
                         (spp == 4 || spp == 8 || spp == 16) && lpa_lds <= 160 * 1024;
  if (use_lpall) {
    p.producer = PhaseAPlan::kAllViews;
    p.spp = spp;
    p.fz_pat = fz_pat;
    p.lpa_lds = lpa_lds;
  } else if (use_mfma) {
    p.producer = PhaseAPlan::kPerView;
    p.spp = spp;
    for (int v = 0; v < V; ++v) {
      PhaseAPlan::View &w = p.view[v];
      w.nt = (s.K[v] + 15) / 16;
      w.lds = lpview_shared_bytes(SP, w.nt, s.K[v], T);
      w.per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / std::max<size_t>(w.lds, 1)));
    }
  } else if (use_big) {
    // K_v > 64 or no tiled copy: dish blocks of 16 * NTB, A-fragments from y
    p.producer = PhaseAPlan::kDishBlock;
    p.SPb = SPb;
    // the unrolled instance where D = 4 SP exactly (no padded k-steps)
    p.spc = (4 * SPb == D && !o.big_runtime_sp && (SPb == 16 || SPb == 32 || SPb == 64)) ? SPb : 0;
    for (int v = 0; v < V; ++v) {
      PhaseAPlan::View &w = p.view[v];
      // a view with few dishes takes the narrowest block that holds them
      // (the MFMAs of the padding columns are not issued); the blocks'
      // lp values and the max-combined view maximum are the same bits
      // whatever the blocking
      w.ntb = big_ntb;
      while (w.ntb > 1 && 16 * (w.ntb / 2) >= s.K[v]) w.ntb /= 2;
      w.waves = big_waves;
      if (w.ntb != big_ntb) w.waves = lpbig_shared_bytes(SPb, w.ntb, T, 4) <= 80 * 1024 ? 4 : 8;
      w.nblk = (s.K[v] + 16 * w.ntb - 1) / (16 * w.ntb);
      w.lds = lpbig_shared_bytes(SPb, w.ntb, T, w.waves);
      // blocks per CU: the register budget allows three 4-wave blocks of the
      // narrow instances (<= 168 VGPRs), two of the 64-dish one; LDS permitting
      w.per_cu = w.waves == 8 ? 1 : (w.ntb <= 2 ? 3 : 2);
      w.per_cu = std::max(1, std::min<int>(w.per_cu, (int)((160 * 1024) / std::max<size_t>(w.lds, 1))));
      w.grouped = o.big_group && w.nblk >= 2 && n_cu % 8 == 0 && (w.per_cu * n_cu) / 8 >= w.nblk;
    }
  }
  return p;
}

}  // namespace mvc
