// Host-only check of plan_launch_layout (hc-spmm_amd/csrc/plan_layout.h): sweeps small plans and asserts the invariants the
// device decodes of every planned launch rely on.  No GPU, no HIP call; compiled and run by tests/test_plan_layout_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "plan_layout.h"

using hcspmm::kWaves;
using hcspmm::PlanArgs;

static long long g_checks = 0;
#define CHECK(cond)                                                                                                      \
  do {                                                                                                                   \
    ++g_checks;                                                                                                          \
    if (!(cond)) {                                                                                                       \
      std::printf("FAILED %s (line %d): n_tasks %d n_wide %d n_tiny %d n_slices %d slice_xcd_tasks %d L %d vec %d T %d " \
                  "own_tiny %d fused %d D %d panel_cols %d\n",                                                           \
                  #cond, __LINE__, n_tasks, n_wide, n_tiny, n_slices, xcd, L, vec, T, (int)own_tiny, fused, D, pc);      \
      std::exit(1);                                                                                                      \
    }                                                                                                                    \
  } while (0)

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

static void one(int n_tasks, int n_wide, int n_tiny, int n_slices, int xcd, int L, int vec, int mid, int T, bool own_tiny,
                int fused, int D, int pc) {
  PlanArgs b{};
  b.n_tasks = n_tasks;
  b.n_wide = n_wide;
  b.n_tiny = n_tiny;
  b.n_slices = n_slices;
  b.slice_xcd_tasks = xcd;
  b.n_dense = 5;
  b.n_dense_compact = 2;
  b.n_dense_compact2 = 1;
  b.D = D;
  b.panel_cols = pc;
  const int panels = hcspmm::plan_launch_layout(b, L, vec, mid, T, own_tiny, fused);
  const int R = 64 / L, per_wg = kWaves * R;
  CHECK(panels == ceil_div(D, pc));
  // the task counts the regions are sized for: no wide tasks with one lane group per wave; the row-tile fused launch
  // (fused bit 1) takes the ordinary and tiny tasks and the dense windows
  const int want_wide = L == 64 ? 0 : n_wide;
  CHECK(b.n_wide == want_wide);
  if (fused & 2) CHECK(b.n_tasks == want_wide && b.n_tiny == 0 && b.n_dense == 0 && b.n_dense_compact == 0 && b.n_dense_compact2 == 0);
  else CHECK(b.n_tasks == n_tasks && b.n_tiny == n_tiny && b.n_dense == 5);
  const int n_ord = b.n_tasks - b.n_tiny - b.n_wide;
  // wide tasks: one per wave
  CHECK(b.wide_wgs * kWaves >= b.n_wide && b.wide_wgs == ceil_div(b.n_wide, kWaves));
  // tiny tasks: in the launch (T per lane group), or exactly no workgroup of it when they have a launch of their own
  if (own_tiny) {
    CHECK(b.tiny_wgs == 0);
    CHECK(b.tiny_kernel_wgs * per_wg * HCSPMM_TINY_KERNEL_T >= b.n_tiny);
    CHECK(b.tiny_kernel_wgs == ceil_div(b.n_tiny, per_wg * HCSPMM_TINY_KERNEL_T));
  } else {
    CHECK(b.tiny_kernel_wgs == 0);
    CHECK(b.tiny_wgs * per_wg * T >= b.n_tiny && b.tiny_wgs == ceil_div(b.n_tiny, per_wg * T));
  }
  // ordinary tasks: 64 / L per wave; free = wide + ordinary + tiny
  const int ord_wgs = b.free_wgs_pp - b.wide_wgs - b.tiny_wgs;
  CHECK(ord_wgs >= 0 && ord_wgs * per_wg >= n_ord && ord_wgs == ceil_div(n_ord, per_wg));
  CHECK(b.free_wgs_pp == b.wide_wgs + ord_wgs + b.tiny_wgs);
  // sliced region: a multiple of 8 workgroups, slice_wgs / 8 per XCD; a sliced panel is a multiple of 8 as well
  CHECK(b.slice_wgs % 8 == 0);
  if (n_slices > 0) CHECK((b.slice_wgs / 8) * per_wg >= xcd && b.slice_wgs == 8 * ceil_div(xcd, per_wg));
  else CHECK(b.slice_wgs == 0);
  int pp = b.slice_wgs + b.free_wgs_pp;  // workgroups per panel before the divisor guard
  if (b.slice_wgs > 0) pp = (pp + 7) / 8 * 8;
  CHECK(b.sparse_wgs == pp * panels);
  CHECK(b.sparse_wgs_pp == (pp > 0 ? pp : 1) && b.sparse_wgs_pp >= 1);
  if (b.slice_wgs > 0) CHECK(b.sparse_wgs_pp % 8 == 0 && b.sparse_wgs_pp - (b.slice_wgs + b.free_wgs_pp) < 8);
  // dense-tile lanes: the narrowest of {1, mid, vec} that covers D in one panel, else vec; the panels cover D
  if (vec > 0) {
    const int want = D <= 16 ? 1 : (D <= 16 * mid ? mid : vec);
    CHECK(b.dense_vec == want);
    CHECK(b.n_panels * 16 * b.dense_vec >= D && (b.n_panels - 1) * 16 * b.dense_vec < D);
    if (D <= 16 * vec) CHECK(b.n_panels == 1);
  } else {  // extremum form: the dense windows once per column panel
    CHECK(b.dense_vec == 0 && b.n_panels == panels);
  }
}

int main() {
  const int tasks[] = {0, 1, 2, 9, 10, 63, 64, 65, 200, 333};
  const int wides[] = {0, 1, 9};
  const int slices[][2] = {{0, 0}, {3, 1}, {3, 64}, {8, 65}, {11, 640}};     // n_slices, slice_xcd_tasks
  const int vecs[][2] = {{0, 0}, {1, 1}, {2, 1}, {4, 2}, {8, 4}};              // vec, DenseV<vec>::mid
  const int shapes[][2] = {{32, 32}, {96, 32}, {8, 8}, {16, 16}, {24, 24}, {50, 50}, {64, 64}, {65, 32}, {128, 128}};  // D, panel_cols
  for (int n_tasks : tasks)
    for (int n_wide : wides) {
      if (n_wide > n_tasks) continue;
      const int tinies[] = {0, 1, n_tasks - n_wide};
      for (int ti = 0; ti < 3; ++ti) {
        const int n_tiny = tinies[ti];
        if (n_tiny > n_tasks - n_wide || (ti == 2 && n_tiny <= 1)) continue;
        for (const auto& sl : slices)
          for (int L = 4; L <= 64; L *= 2)
            for (const auto& v : vecs)
              for (int T = 2; T <= 4; T += 2)
                for (int own = 0; own < 2; ++own)
                  for (int fused = 0; fused < 3; ++fused)
                    for (const auto& sh : shapes)
                      one(n_tasks, n_wide, n_tiny, sl[0], sl[1], L, v[0], v[1], T, own != 0, fused, sh[0], sh[1]);
      }
    }
  std::printf("plan_layout ok: %lld checks\n", g_checks);
  return 0;
}
