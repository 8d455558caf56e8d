// plan_driver.cpp — prints the path decisions of csrc/mvc_plan.h over a list
// of state shapes, one line per case (tests/test_plan.py compares the output
// with tests/golden/plan_golden.txt).  Host only:
//   g++ -std=c++17 -I multiview-clustering_amd/csrc -I include tests/plan_driver.cpp
#include <stdio.h>

#include "mvc_plan.h"

using namespace mvc;

namespace {

// K_v: uniform k, or the halving pattern max(1, k >> v)
struct Case {
  int n, V, D, T, k;
  bool halving;
  bool tiled = true;   // the tiled copy of y exists where the shape allows one
  const char *path = "";
  int n_cu = 256;
};

Shape shape_of(const Case &c) {
  Shape s;
  s.n = c.n; s.V = c.V; s.D = c.D; s.T = c.T; s.n_cu = c.n_cu;
  int kmax = 1;
  for (int v = 0; v < c.V; ++v) {
    s.K[v] = c.halving ? std::max(1, c.k >> std::min(v, 30)) : c.k;
    kmax = std::max(kmax, (int)s.K[v]);
  }
  // as the sampler builds them: the tiled copy for D % 4 == 0, D >= 16, V <= MVC_Z_VMAX; the S1 tiling for K_v <= MVC_Z_KMAX
  if (c.tiled && c.D % 4 == 0 && c.D >= 16 && c.V <= MVC_Z_VMAX) s.SP = ((c.D / 4 + MVC_ZR - 1) / MVC_ZR) * MVC_ZR;
  s.s1t_ok = s.SP > 0 && kmax <= MVC_Z_KMAX;
  s.lo = 0;
  s.hi = c.n;
  return s;
}

// a layout: lds nws ks ts limit s1 cache stride ring pfn tw lc vpo small dyn wgrid, then the run
// kernel's mode/threads single and batched
void print_lds(const char *tag, const SeqLds &L, const Shape &s, const PathOpts &o) {
  const RunInstance a = run_instance(L, false), b = run_instance(L, true);
  printf(" | %s %d %d %d %d %d %d %lld %lld %d %d %d %d %lld %d %lld %d %s/%d %s/%d", tag, L.lds, L.nws, L.ks, L.ts,
         L.limit, L.s1, (long long)L.cache_dbl, (long long)L.stride, L.ring, L.pfn, L.tw, L.lc, (long long)L.vpo, L.small,
         (long long)run_dyn(s.V, s.D, L), run_wgrid(o, L) ? 1 : 0, a.name + 7, a.threads, b.name + 7, b.threads);
}
bool same(const SeqLds &a, const SeqLds &b) {
  return a.lds == b.lds && a.nws == b.nws && a.ks == b.ks && a.ts == b.ts && a.limit == b.limit && a.s1 == b.s1 &&
         a.cache_dbl == b.cache_dbl && a.stride == b.stride && a.ring == b.ring && a.pfn == b.pfn && a.tw == b.tw &&
         a.lc == b.lc && a.vpo == b.vpo && a.small == b.small;
}

// phase A: lane run zpath batch need producer draw, the producer's launches
// (all-views A, generic G: grid/block; per view P nt, B ntb/waves/nblk/grouped:
// lds/grid/block), then the draw: tm row_nb row_lds lds first grid.  Then the
// layouts of pick_layout: "lane" while the sweep runs the lane loop (omitted
// where it is the run kernels'), "run", and "novp" once value prediction has
// stopped (omitted where it is the same).
// the views' launches in order, a run of k equal ones as "... xk"
void print_views(const char (*w)[64], int V) {
  for (int v = 0, k; v < V; v += k) {
    for (k = 1; v + k < V && strcmp(w[v], w[v + k]) == 0;) ++k;
    printf(k > 1 ? " %s x%d" : " %s", w[v], k);
  }
}
void run_case(const Case &c) {
  char w[MVC_MAXV][64];
  const Shape s = shape_of(c);
  const PathOpts o = parse_path_opts(c.path);
  printf("n=%d V=%d D=%d T=%d K=%d%c SP=%d s1t=%d cu=%d", c.n, c.V, c.D, c.T, c.k, c.halving ? 'h' : 'u', s.SP,
         s.s1t_ok ? 1 : 0, s.n_cu);
  if (c.path[0]) printf(" [%s]", c.path);
  const PhaseAPlan p = plan_phase_a(s, o);
  const int nb = (int)std::min<size_t>(p.batch, (size_t)c.n);   // the first batch
  printf(" | %d %d %d %zu %zu %d %d", p.lane ? 1 : 0, p.run ? 1 : 0, p.zpath(), p.batch, p.lpb_need, (int)p.producer,
         (int)p.draw);
  if (!p.lane) {
    if (p.producer == PhaseAPlan::kAllViews)
      printf(" A%d,%u,%zu/%d/%d", p.spp, p.fz_pat, p.lpa_lds, p.producer_grid(0, nb), p.producer_threads(0));
    if (p.producer == PhaseAPlan::kGeneric) printf(" G%d/%d", p.producer_grid(0, nb), p.producer_threads(0));
    if (p.producer == PhaseAPlan::kPerView) {
      printf(" P%d", p.spp);
      for (int v = 0; v < c.V; ++v) {
        snprintf(w[v], sizeof w[v], "%d:%zu/%d/%d", p.view[v].nt, p.view[v].lds, p.producer_grid(v, nb), p.producer_threads(v));
      }
      print_views(w, c.V);
    }
    if (p.producer == PhaseAPlan::kDishBlock) {
      printf(" B%d,%d", p.SPb, p.spc);
      for (int v = 0; v < c.V; ++v)
        snprintf(w[v], sizeof w[v], "%d,%d,%d,%d:%zu/%d/%d", p.view[v].ntb, p.view[v].waves, p.view[v].nblk,
                 p.view[v].grouped ? 1 : 0, p.view[v].lds, p.producer_grid(v, nb), p.producer_threads(v));
      print_views(w, c.V);
    }
    printf(" ; %d %d %d %zu %d %d", p.reg_tm, p.row_nb, p.row_lds ? 1 : 0, p.draw_lds, p.first_in_draw ? 1 : 0,
           p.draw_grid(nb));
  }
  const SeqLds lane = pick_layout(s, o, true, s.T, s.K, true), run = pick_layout(s, o, false, s.T, s.K, true),
               novp = run_layout(s, o, s.T, s.K, false);
  if (!same(lane, run)) print_lds("lane", lane, s, o);
  print_lds("run", run, s, o);
  if (!same(novp, run)) print_lds("novp", novp, s, o);
  printf("\n");
}

const int kNs[] = {200, 1024, 1025, 16384, 16385, 100000, 1000000};
const int kVs[] = {1, 4, 5, 8, 9, 16, 17};
const int kDs[] = {1, 4, 15, 16, 17, 20, 64, 128, 256};
const int kTs[] = {1, 7, 8, 9, 16, 17, 31, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 4096, 18000};
const int kKs[] = {1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 4000};

}  // namespace

int main() {
  // part 1: every axis through its boundaries at two anchors: configs[3]
  // (K_v = 64 / 32 / 16 / 8) and New_Simulation (K_v = 2)
  const Case anchors[] = {{1000000, 4, 128, 64, 64, true}, {200, 5, 1, 4, 2, false}};
  for (const Case &a : anchors) {
    run_case(a);
    for (int n : kNs) { Case c = a; c.n = n; run_case(c); }
    for (int V : kVs) { Case c = a; c.V = V; run_case(c); }
    for (int D : kDs) { Case c = a; c.D = D; run_case(c); }
    for (int T : kTs) { Case c = a; c.T = T; run_case(c); }
    for (int k : kKs) { Case c = a; c.k = k; c.halving = false; run_case(c); }
    for (int k : kKs) { Case c = a; c.k = k; c.halving = true; run_case(c); }
    Case c = a; c.tiled = false; run_case(c);
  }
  // part 2: the cross of a reduced set
  for (int n : {200, 1000000})
    for (int V : {1, 5, 9})
      for (int D : {1, 20, 128})
        for (int T : {16, 513, 4096})
          for (int h = 0; h < 2; ++h) run_case({n, V, D, T, h ? 4000 : 64, h == 1});
  // part 3: every MVC_PATH key, at the shapes of the GPU tests that pin it
  // (tests/test_gpu_parity.py: ZPATH_SHAPES with K_v = max(1, K >> v), the
  // repair tests' New_Simulation and synthetic shapes, the dish-block shapes)
  const Case zshapes[] = {{3001, 4, 64, 16, 16, true}, {50, 2, 20, 4, 4, true}, {4000, 3, 32, 96, 64, true},
                          {2500, 2, 128, 64, 64, true}, {5000, 3, 32, 200, 32, true}, {6000, 2, 16, 300, 64, true},
                          {1500, 3, 16, 40, 32, true}, {2000, 2, 24, 24, 8, true}, {4100, 4, 128, 64, 64, true},
                          {777, 1, 32, 16, 16, true}};
  for (const char *path : {"generic=1", "generic=0,zdraw=reg,lpall=1", "generic=0,zdraw=lds,lpall=1",
                           "generic=0,zdraw=reg,lpall=0", "generic=0,zdraw=row,lpall=1", "generic=0,zdraw=row-global,lpall=1"})
    for (Case c : zshapes) { c.path = path; run_case(c); }
  run_case({1200, 18, 16, 96, 8, true, true, "zdraw=row"});   // test_many_views_row_draw_gate
  const Case bshapes[] = {{6000, 3, 32, 128, 128, true}, {4100, 4, 64, 64, 64, true}, {3000, 2, 256, 80, 80, true}};
  for (const char *path : {"", "big=1", "big=1,big_sp=runtime", "big=1,big_group=0"})
    for (Case c : bshapes) { c.path = path; run_case(c); }
  const Case rshapes[] = {{200, 5, 1, 4, 2, false},       {200, 5, 1, 170, 30, false},     {3000, 5, 16, 6, 6, false},
                          {3000, 3, 16, 900, 300, false}, {3000, 5, 16, 2500, 700, false}, {20000, 4, 1, 16, 16, false},
                          {20000, 2, 16, 8, 8, false},    {1000000, 4, 128, 64, 64, true}};
  for (const char *path : {"", "repair=grid", "waves=1", "waves=3", "waves=8", "lc=0", "lc=col", "vp=0", "small_plain=1",
                           "run_lds=0", "run_lds=0,wide=0", "run_lds=0,wide=block"})
    for (Case c : rshapes) { c.path = path; run_case(c); }
  // the parsed options themselves: generic, zdraw lds / row / row-global, no lpall, big, big_sp, big_group,
  // grid only, waves, lc, lane, vp, vp_stats, small_plain, global, wide, wide grid, wide_fin, max_tables,
  // chain_batch, chain_threads, exact_lds
  for (const char *path :
       {"", "generic=1", "zdraw=lds", "zdraw=row", "zdraw=rowx", "zdraw=row-global", "lpall=0", "big=1", "big_sp=runtime",
        "big_group=0", "repair=grid", "repair=run", "waves=0", "waves=3", "waves=99", "lc=0", "lc=col", "vp=0", "vp_stats=1",
        "small_plain=1", "run_lds=0", "wide=0", "wide=block", "wide_fin=0", "max_tables=32", "max_tables=1",
        "max_tables=99999999", "chain_batch=0", "chain_threads=0", "exact_lds=0", "exact_lds=1", "exact_lds=2", "exact_lds=7",
        "unknown=1, lc=0", "lc=,waves=", "lc=0,lc=col", "xlc=0", "lc", "waves=3,generic=1,zdraw=row-global"}) {
    const PathOpts o = parse_path_opts(path);
    printf("[%s] %d %d%d%d %d %d%d%d %d %d %d%d %d%d %d %d %d%d %d %d %d%d %d\n", path, o.force_generic, o.force_zdraw_lds,
           o.force_zdraw_row, o.no_zrow_lds, o.no_lpall, o.force_big, o.big_runtime_sp, o.big_group, o.repair_grid_only,
           o.run_waves, o.use_lc, o.use_lane, o.use_vp, o.vp_stats, o.small_n_plain, o.force_global, o.use_wide, o.wide_grid,
           o.wide_fin_lds, o.max_tables, o.chain_batch, o.chain_threads, o.exact_lds);
  }
  const PathOpts none = parse_path_opts((const char *)nullptr);
  printf("null %d %d %d\n", none.run_waves, none.max_tables, none.exact_lds);
  return 0;
}
