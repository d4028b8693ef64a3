// arg_codes.cpp -- the return codes of the planned entry points of libhcspmm.so for failing arguments, and their order of
// precedence: forward_typed / _weighted / _weighted_heads / _weighted_indexed, forward_fp8 (binary and weighted),
// forward_extremum / _extremum_backward and forward_edge_messages (mul, copy), each with a plan and plan-free, with every
// single defect of the list below and every pair of them.  Host only: every call carries two defects of the last checks of
// its path (no workspace for the plan's split row; no edgeToRow for the plan-free kernel), so each one returns before a
// launch and the pointers are never read.  Prints one line per argument set; tests/test_capi_arg_codes_cpu.py compares
// the lines with tests/golden/capi_arg_codes.txt.
//   hipcc arg_codes.cpp -I include -L csrc -lhcspmm   (host code only)
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hcspmm.h"

struct Args {
  const void* X;
  int64_t x_rows, ldx;
  void* Z;
  int64_t ldz;
  int dtype;
  const int32_t *rp, *col, *bp, *e2c, *e2r, *ht, *plan;
  const hcspmm_plan_header* ph;
  int64_t N, E;
  int D;
  void* ws;
  size_t ws_bytes;
  const float* values;
  int heads;
  const int32_t* vindex;
  int64_t num_values;
  int reduce;
  int32_t* arg;
  int64_t ldarg;
  const int32_t* perm;
  const float* F;
  int64_t f_rows, ldf;
  int op;
};

typedef void (*Defect)(Args&);
struct Named {
  const char* name;
  Defect apply;
};
static hcspmm_plan_header g_other;  // a sound header of another graph size
static float g_short_ws[4];

static const Named kDefects[] = {
    {"none", [](Args&) {}},
    {"N<0", [](Args& a) { a.N = -1; }},
    {"E<0", [](Args& a) { a.E = -1; }},
    {"D=0", [](Args& a) { a.D = 0; }},
    {"D=6", [](Args& a) { a.D = 6; }},
    {"ldx<D", [](Args& a) { a.ldx = a.D - 1; }},
    {"ldz<D", [](Args& a) { a.ldz = a.D - 1; }},
    {"dtype=7", [](Args& a) { a.dtype = 7; }},
    {"dtype=f16", [](Args& a) { a.dtype = HCSPMM_DTYPE_F16; }},
    {"N=0", [](Args& a) { a.N = 0; }},
    {"X=0", [](Args& a) { a.X = nullptr; }},
    {"Z=0", [](Args& a) { a.Z = nullptr; }},
    {"rowptr=0", [](Args& a) { a.rp = nullptr; }},
    {"col=0", [](Args& a) { a.col = nullptr; }},
    {"N>range", [](Args& a) { a.N = INT32_MAX; }},
    {"E>range", [](Args& a) { a.E = (int64_t)INT32_MAX + 1; }},
    {"header=0", [](Args& a) { a.ph = nullptr; }},
    {"plan=0", [](Args& a) { a.plan = nullptr; }},
    {"other header", [](Args& a) { if (a.ph) a.ph = &g_other; }},
    {"x_rows short", [](Args& a) { a.x_rows = a.N - 1; }},
    {"short workspace", [](Args& a) { a.ws = g_short_ws, a.ws_bytes = sizeof(g_short_ws); }},
    {"blockPartition=0", [](Args& a) { a.bp = nullptr; }},
    {"hybrid_type=0", [](Args& a) { a.ht = nullptr; }},
    {"edgeToColumn=0", [](Args& a) { a.e2c = nullptr; }},
    {"values=0", [](Args& a) { a.values = nullptr; }},
    {"heads=0", [](Args& a) { a.heads = 0; }},
    {"heads=5", [](Args& a) { a.heads = 5; }},
    {"value_index=0", [](Args& a) { a.vindex = nullptr; }},
    {"num_values=0", [](Args& a) { a.num_values = 0; }},
    {"num_values<0", [](Args& a) { a.num_values = -1; }},
    {"reduce=9", [](Args& a) { a.reduce = 9; }},
    {"arg=0", [](Args& a) { a.arg = nullptr; }},
    {"ldarg<D", [](Args& a) { a.ldarg = a.D - 1; }},
    {"perm=0", [](Args& a) { a.perm = nullptr; }},
    {"F=0", [](Args& a) { a.F = nullptr; }},
    {"f_rows short", [](Args& a) { a.f_rows = a.E - 1; }},
    {"f_rows>range", [](Args& a) { a.f_rows = (int64_t)INT32_MAX + 1; }},
    {"ldf<D", [](Args& a) { a.ldf = a.D - 1; }},
    {"op=3", [](Args& a) { a.op = 3; }},
};
constexpr int kNumDefects = (int)(sizeof(kDefects) / sizeof(kDefects[0]));

#define GRAPH a.rp, a.col, a.bp, a.e2c, a.e2r, a.ht, a.plan, a.ph, a.N, a.E, a.D
#define TYPED a.X, a.x_rows, a.ldx, a.Z, a.ldz, a.dtype, GRAPH, a.ws, a.ws_bytes, nullptr

struct Entry {
  const char* name;
  int (*call)(const Args&);
};
static const Entry kEntries[] = {
    {"typed", [](const Args& a) { return hcspmm_forward_typed(TYPED); }},
    {"weighted", [](const Args& a) { return hcspmm_forward_weighted(TYPED, a.values); }},
    {"heads", [](const Args& a) { return hcspmm_forward_weighted_heads(TYPED, a.values, a.heads); }},
    {"indexed", [](const Args& a) { return hcspmm_forward_weighted_indexed(TYPED, a.values, a.heads, a.vindex, a.num_values); }},
    {"fp8", [](const Args& a) {
       return hcspmm_forward_fp8(a.X, a.x_rows, a.ldx, HCSPMM_FP8_E4M3, nullptr, nullptr, (float*)a.Z, a.ldz, GRAPH, a.ws, a.ws_bytes,
                                 nullptr);
     }},
    {"fp8 weighted", [](const Args& a) {
       return hcspmm_forward_fp8(a.X, a.x_rows, a.ldx, HCSPMM_FP8_E4M3, a.values, a.values, (float*)a.Z, a.ldz, GRAPH, a.ws, a.ws_bytes,
                                 nullptr);
     }},
    {"extremum", [](const Args& a) { return hcspmm_forward_extremum(TYPED, a.reduce, a.arg, a.ldarg); }},
    {"extremum backward", [](const Args& a) {
       return hcspmm_forward_extremum_backward((const float*)a.X, a.ldx, a.arg, a.ldarg, (float*)a.Z, a.ldz, GRAPH, a.perm, a.ws,
                                               a.ws_bytes, nullptr);
     }},
    {"messages", [](const Args& a) {
       return hcspmm_forward_edge_messages(a.X, a.x_rows, a.ldx, a.F, a.f_rows, a.ldf, a.vindex, a.op, a.Z, a.ldz, GRAPH, a.ws,
                                           a.ws_bytes, nullptr);
     }},
    {"messages copy", [](const Args& a) {
       return hcspmm_forward_edge_messages(nullptr, 0, a.ldx, a.F, a.f_rows, a.ldf, a.vindex, HCSPMM_EDGE_OP_COPY, a.Z, a.ldz, GRAPH,
                                           a.ws, a.ws_bytes, nullptr);
     }},
};

int main() {
  // 64 nodes: a hub row long enough to be split (so that the plan needs a workspace), two entries in every other row
  const int64_t N = 64;
  const int D = 48;
  std::vector<int32_t> rowptr(N + 1, 0), col;
  for (int64_t r = 0; r < N; ++r) {
    if (r == 3) for (int32_t c = 0; c < N; ++c) col.push_back(c);
    else col.push_back((int32_t)((r * 7) % (N - 1))), col.push_back((int32_t)((r * 7) % (N - 1) + 1));
    rowptr[r + 1] = (int32_t)col.size();
  }
  const int64_t E = (int64_t)col.size(), W = (N + 15) / 16;
  std::vector<int32_t> bp(W), ht(W), e2c(E), e2r(E);
  if (hcspmm_preprocess_host(rowptr.data(), col.data(), N, E, N, HCSPMM_RULE_INTENDED, 1, bp.data(), e2c.data(), e2r.data(),
                             ht.data()) != HCSPMM_OK)
    return 2;
  hcspmm_plan_params pp = {16, 8, 0};  // split the hub row
  int64_t words = 0;
  if (hcspmm_plan_words(rowptr.data(), N, E, bp.data(), ht.data(), &pp, &words) != HCSPMM_OK) return 2;
  std::vector<int32_t> plan((size_t)words);
  if (hcspmm_plan_build(rowptr.data(), col.data(), N, E, N, bp.data(), e2c.data(), ht.data(), &pp, plan.data(), words) != HCSPMM_OK)
    return 2;
  hcspmm_plan_header header;
  std::memcpy(&header, plan.data(), sizeof(header));
  if (hcspmm_workspace_bytes(&header, D) <= sizeof(g_short_ws) || hcspmm_workspace_bytes(&header, 4) <= sizeof(g_short_ws)) {
    std::fprintf(stderr, "the plan needs no workspace: a call could get as far as a launch\n");
    return 3;
  }
  g_other = header;
  g_other.num_nodes += 16;

  std::vector<float> buf((size_t)(E > N ? E : N) * D);  // stands for every operand: never read
  std::vector<int32_t> ibuf((size_t)N * D);
  long sets = 0;
  for (int planned = 1; planned >= 0; --planned) {
    Args base{};
    base.X = base.Z = buf.data();
    base.x_rows = N, base.ldx = base.ldz = base.ldarg = base.ldf = D;
    base.dtype = HCSPMM_DTYPE_F32;
    base.rp = rowptr.data(), base.col = col.data(), base.bp = bp.data(), base.e2c = e2c.data(), base.ht = ht.data();
    base.e2r = nullptr;                  // the plan-free path's last check
    base.ws = nullptr, base.ws_bytes = 0;  // the planned path's last check
    if (planned) base.plan = plan.data(), base.ph = &header;
    base.N = N, base.E = E, base.D = D;
    base.values = base.F = buf.data();
    base.heads = 4;
    base.vindex = base.perm = ibuf.data();
    base.arg = ibuf.data();
    base.num_values = E, base.f_rows = E;
    base.reduce = HCSPMM_REDUCE_MAX, base.op = HCSPMM_EDGE_OP_MUL;
    for (int i = 0; i < kNumDefects; ++i)
      for (int j = i; j < kNumDefects; ++j) {
        if (i == 0 && j > 0) continue;  // ("none" pairs with itself only: the single defects are the pairs (i, i))
        Args a = base;
        kDefects[i].apply(a);
        kDefects[j].apply(a);
        std::printf("%s | %s + %s |", planned ? "plan" : "plan-free", kDefects[i].name, kDefects[j].name);
        for (const Entry& e : kEntries) std::printf(" %d", e.call(a));
        std::printf("\n");
        ++sets;
      }
  }
  std::fprintf(stderr, "arg_codes: %ld argument sets x %d entry points\n", sets, (int)(sizeof(kEntries) / sizeof(kEntries[0])));
  return 0;
}
