// Host-side record of the batch-norm entry points (csrc/bn_act.hip): the workspace arithmetic and the argument
// validation, which run before anything is launched.  It prints one line per call -- entry, arguments, status (bytes for
// the workspace query) -- so that two builds of bn_act.hip can be compared with `cmp`: a change of the host code must
// leave the output byte-identical.  Meant for a host sanitizer build; bn_act.hip links alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined \
//         tools/bn_host_check.cpp spml_amd/csrc/bn_act.hip -o bn_host_check && ./bn_host_check > bn_host_check.txt
//
// Calls that pass every check reach a launch.  Without a device that launch fails (SPML_ERR_LAUNCH, nothing runs), and
// this is where the program belongs.  The pointers below are host memory, so with a device present every call that
// could reach a launch -- any call of an entry without a workspace argument, and any call with a sufficient
// workspace -- is skipped and printed as such.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "spml_hip.h"

struct Args {
  int64_t R = 300;
  int C = 40;
  int chunks = 3, chunk_rows = 100;
  double count = 300.0;
  int world = 2;
  size_t ws_bytes = 0;
  void* p[20] = {};
};
typedef int (*Fn)(const Args&);
struct Entry {
  const char* name;
  Fn fn;
  std::vector<const char*> ptrs;       // the pointer arguments in the order of the signature
  std::vector<int> optional;           // those that may be absent: every subset of them is tried
  int ws = -1, count_dev = -1;         // index of the workspace / of count_dev, -1: none
  bool chunks = false, count = false;  // takes (chunks, chunk_rows) / a host-side count
};

#define F(i) static_cast<float*>(a.p[i])
#define U(i) static_cast<unsigned char*>(a.p[i])
static const float kMomentum = 0.1f, kEps = 1e-5f;

static const std::vector<Entry> kEntries = {
    {"spml_bn_stats_f32",
     [](const Args& a) { return spml_bn_stats_f32(F(0), a.R, a.C, F(1), F(2), a.p[3], a.ws_bytes, nullptr); },
     {"x", "mean", "m2", "ws"}, {}, 3},
    {"spml_bn_act_apply_f32",
     [](const Args& a) { return spml_bn_act_apply_f32(F(0), F(1), a.R, a.C, F(2), F(3), F(4), F(5), 1, F(6), nullptr); },
     {"x", "residual", "mean", "invstd", "gamma", "beta", "y"}, {1}},
    {"spml_bn_act_bwd_reduce_f32",
     [](const Args& a) {
       return spml_bn_act_bwd_reduce_f32(F(0), F(1), F(2), a.R, a.C, F(3), F(4), F(5), F(6), a.p[7], a.ws_bytes, nullptr);
     },
     {"dy", "y", "x", "mean", "invstd", "sum_dz", "sum_dz_xhat", "ws"}, {1}, 7},
    {"spml_bn_act_bwd_apply_f32",
     [](const Args& a) {
       return spml_bn_act_bwd_apply_f32(F(0), F(1), F(2), a.R, a.C, F(3), F(4), F(5), F(6), F(7), a.count, F(8), F(9),
                                        F(10), nullptr);
     },
     {"dy", "y", "x", "mean", "invstd", "gamma", "sum_dz", "sum_dz_xhat", "count_dev", "dx", "d_residual"},
     {1, 8, 9, 10}, -1, 8, false, true},
    {"spml_bn_act_fwd_f32",
     [](const Args& a) {
       return spml_bn_act_fwd_f32(F(0), F(1), a.R, a.C, F(2), F(3), F(4), F(5), kMomentum, kEps, 1, F(6), F(7), F(8),
                                  a.p[9], a.ws_bytes, nullptr);
     },
     {"x", "residual", "gamma", "beta", "running_mean", "running_var", "y", "mean", "invstd", "ws"}, {1, 4, 5}, 9},
    {"spml_bn_act_bwd_f32",
     [](const Args& a) {
       return spml_bn_act_bwd_f32(F(0), F(1), F(2), a.R, a.C, F(3), F(4), F(5), F(6), F(7), F(8), F(9), a.p[10],
                                  a.ws_bytes, nullptr);
     },
     {"dy", "y", "x", "mean", "invstd", "gamma", "d_gamma", "d_beta", "dx", "d_residual", "ws"}, {1, 8, 9}, 10},
    {"spml_bn_stats_ext_f32",
     [](const Args& a) {
       return spml_bn_stats_ext_f32(F(0), a.R, a.C, F(1), F(2), F(3), F(4), a.p[5], a.ws_bytes, nullptr);
     },
     {"x", "mean", "m2", "cmax", "cmin", "ws"}, {}, 5},
    {"spml_bn_stats_ext_chunks_f32",
     [](const Args& a) {
       return spml_bn_stats_ext_chunks_f32(F(0), a.chunks, a.chunk_rows, a.R, a.C, F(1), F(2), F(3), F(4), nullptr);
     },
     {"chunk_stats", "mean", "m2", "cmax", "cmin"}, {}, -1, -1, true},
    {"spml_bn_finalize_f32",
     [](const Args& a) {
       return spml_bn_finalize_f32(F(0), F(1), a.C, a.count, kEps, kMomentum, F(2), F(3), F(4), nullptr);
     },
     {"mean", "m2", "running_mean", "running_var", "invstd"}, {2, 3}, -1, -1, false, true},
    {"spml_bn_act_apply_hl8_f32",
     [](const Args& a) {
       return spml_bn_act_apply_hl8_f32(F(0), F(1), F(2), a.R, a.C, F(3), F(4), F(5), F(6), F(7), F(8), 1, F(9), a.p[10],
                                        F(11), U(12), nullptr);
     },
     {"x", "residual", "residual_bound", "mean", "invstd", "gamma", "beta", "cmax", "cmin", "y", "y_hl8", "y_bound",
      "relu_mask"},
     {1, 2, 7, 8, 9, 10, 11, 12}},
    {"spml_bn_act_bwd_reduce_ext_f32",
     [](const Args& a) {
       return spml_bn_act_bwd_reduce_ext_f32(F(0), F(1), U(2), F(3), a.R, a.C, F(4), F(5), F(6), F(7), F(8), a.p[9],
                                             a.ws_bytes, nullptr);
     },
     {"dy", "y", "relu_mask", "x", "mean", "invstd", "sum_dz", "sum_dz_xhat", "max_dz", "ws"}, {1, 2}, 9},
    {"spml_bn_act_bwd_apply_hl8_f32",
     [](const Args& a) {
       return spml_bn_act_bwd_apply_hl8_f32(F(0), F(1), U(2), F(3), a.R, a.C, F(4), F(5), F(6), F(7), F(8), F(9), F(10),
                                            F(11), a.count, F(12), F(13), a.p[14], F(15), F(16), nullptr);
     },
     {"dy", "y", "relu_mask", "x", "mean", "invstd", "gamma", "sum_dz", "sum_dz_xhat", "max_dz", "cmax", "cmin",
      "count_dev", "dx", "dx_hl8", "dx_bound", "d_residual"},
     {1, 2, 9, 10, 11, 12, 13, 14, 15, 16}, -1, 12, false, true},
    {"spml_bn_fwd_hl8_f32",
     [](const Args& a) {
       return spml_bn_fwd_hl8_f32(F(0), F(1), F(2), a.R, a.C, F(3), F(4), F(5), F(6), kMomentum, kEps, 1, F(7), a.p[8],
                                  F(9), U(10), F(11), F(12), F(13), F(14), a.p[15], a.ws_bytes, nullptr);
     },
     {"x", "residual", "residual_bound", "gamma", "beta", "running_mean", "running_var", "y", "y_hl8", "y_bound",
      "relu_mask", "mean", "invstd", "cmax", "cmin", "ws"},
     {1, 2, 5, 6, 7, 8, 10}, 15},
    {"spml_bn_fwd_hl8_chunks_f32",
     [](const Args& a) {
       return spml_bn_fwd_hl8_chunks_f32(F(0), F(1), a.chunks, a.chunk_rows, F(2), F(3), a.R, a.C, F(4), F(5), F(6), F(7),
                                         kMomentum, kEps, 1, F(8), a.p[9], F(10), U(11), F(12), F(13), F(14), F(15),
                                         nullptr);
     },
     {"x", "chunk_stats", "residual", "residual_bound", "gamma", "beta", "running_mean", "running_var", "y", "y_hl8",
      "y_bound", "relu_mask", "mean", "invstd", "cmax", "cmin"},
     {2, 3, 6, 7, 8, 9, 11}, -1, -1, true},
    {"spml_bn_bwd_hl8_f32",
     [](const Args& a) {
       return spml_bn_bwd_hl8_f32(F(0), F(1), U(2), F(3), a.R, a.C, F(4), F(5), F(6), F(7), F(8), F(9), F(10), F(11),
                                  a.p[12], F(13), F(14), a.p[15], a.ws_bytes, nullptr);
     },
     {"dy", "y", "relu_mask", "x", "mean", "invstd", "gamma", "cmax", "cmin", "d_gamma", "d_beta", "dx", "dx_hl8",
      "dx_bound", "d_residual", "ws"},
     {1, 2, 11, 12, 13, 14}, 15},
    {"spml_bn_bwd_hl8_chunks_f32",
     [](const Args& a) {
       return spml_bn_bwd_hl8_chunks_f32(F(0), U(1), F(2), F(3), a.chunks, a.chunk_rows, a.R, a.C, F(4), F(5), F(6), F(7),
                                         F(8), F(9), F(10), F(11), F(12), a.p[13], F(14), F(15), nullptr);
     },
     {"dy", "relu_mask", "x", "chunk_stats", "mean", "invstd", "gamma", "cmax", "cmin", "d_gamma", "d_beta", "max_dz",
      "dx", "dx_hl8", "dx_bound", "d_residual"},
     {1, 12, 13, 14, 15}, -1, -1, true},
    {"spml_bn_act_bwd_reduce_ext_chunks_f32",
     [](const Args& a) {
       return spml_bn_act_bwd_reduce_ext_chunks_f32(F(0), a.chunks, a.chunk_rows, a.R, a.C, F(1), F(2), F(3), F(4),
                                                    nullptr);
     },
     {"chunk_stats", "invstd", "sum_dz", "sum_dz_xhat", "max_dz"}, {}, -1, -1, true},
    {"spml_bn_finalize_ranks_f32",
     [](const Args& a) {
       return spml_bn_finalize_ranks_f32(F(0), a.world, a.C, kEps, kMomentum, F(1), F(2), F(3), F(4), F(5), nullptr);
     },
     {"stats", "running_mean", "running_var", "mean", "invstd", "total_count"}, {1, 2, 5}},
};

alignas(16) static char bufs[20][64];           // one per pointer argument: nothing here reads or writes them
static std::vector<char> workspace;
static bool have_device = false;
static long n_calls = 0, n_skipped = 0;

static void call(const Entry& e, const char* what, const Args& a) {
  std::printf("%s [%s] R=%lld C=%d", e.name, what, (long long)a.R, a.C);
  if (e.chunks) std::printf(" chunks=%d chunk_rows=%d", a.chunks, a.chunk_rows);
  if (e.count) std::printf(" count=%g", a.count);
  if (e.ws >= 0) std::printf(" ws_bytes=%zu", a.ws_bytes);
  for (size_t i = 0; i < e.ptrs.size(); ++i) {
    const char* base = (int)i == e.ws ? workspace.data() : bufs[i];
    if (!a.p[i]) std::printf(" %s=null", e.ptrs[i]);
    else if (a.p[i] != base) std::printf(" %s=+%d", e.ptrs[i], (int)(static_cast<char*>(a.p[i]) - base));
  }
  ++n_calls;
  const bool may_launch = e.ws < 0 || (a.p[e.ws] && a.ws_bytes >= spml_bn_workspace_bytes(a.R, a.C));
  if (have_device && may_launch) {
    ++n_skipped;
    std::printf(" -> skipped: a device is present\n");
    return;
  }
  std::printf(" -> %d\n", e.fn(a));
}

static void sweep(const Entry& e) {
  Args v;
  const int n = (int)e.ptrs.size();
  for (int i = 0; i < n; ++i) v.p[i] = i == e.ws ? workspace.data() : bufs[i];
  v.ws_bytes = spml_bn_workspace_bytes(v.R, v.C);
  call(e, "valid", v);
  for (int i = 0; i < n; ++i) {
    Args a = v;
    a.p[i] = nullptr;
    call(e, "one pointer null", a);
  }
  for (int i = 0; i < n; ++i) {
    Args a = v;
    a.p[i] = static_cast<char*>(a.p[i]) + 4;
    call(e, "one pointer misaligned", a);
  }
  for (int C : {4, 6, 8, 12}) {
    Args a = v;
    a.C = C;
    a.ws_bytes = spml_bn_workspace_bytes(a.R, C);
    call(e, "channels", a);
  }
  for (int64_t R : {(int64_t)0, (int64_t)-1}) {
    Args a = v;
    a.R = R;
    call(e, "no rows", a);
  }
  {
    Args a = v;
    a.C = 0;
    call(e, "no channels", a);
  }
  if (e.ws >= 0) {
    Args a = v;
    a.ws_bytes = v.ws_bytes - 1;
    call(e, "workspace one byte short", a);
    a.ws_bytes = 0;
    call(e, "workspace empty", a);
    a.p[e.ws] = nullptr;
    call(e, "workspace null", a);
  }
  if (e.chunks) {
    // R = 300: (3, 100), (2, 150), (1, 300), (300, 1) cover it; the others are short, or leave the last chunk empty
    const int cases[][2] = {{3, 100}, {2, 100}, {4, 100}, {3, 150}, {2, 150}, {1, 300}, {1, 299}, {2, 300}, {300, 1},
                            {299, 1}, {301, 1}, {0, 100}, {3, 0}, {-1, 100}, {3, -100}, {65536, 65536}};
    for (const auto& c : cases) {
      Args a = v;
      a.chunks = c[0];
      a.chunk_rows = c[1];
      call(e, "chunk cover", a);
    }
  }
  if (e.count) {
    for (double count : {0.0, -1.0, 1.0}) {
      Args a = v;
      a.count = count;
      call(e, "count", a);
      if (e.count_dev < 0) continue;
      a.p[e.count_dev] = nullptr;
      call(e, "count", a);
    }
  }
  for (unsigned m = 1; m < (1u << e.optional.size()); ++m) {
    Args a = v;
    for (size_t j = 0; j < e.optional.size(); ++j)
      if (m >> j & 1) a.p[e.optional[j]] = nullptr;
    call(e, "optional pointers", a);
  }
}

int main() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess) devices = 0;
  have_device = devices > 0;
  (void)hipGetLastError();
  const int64_t Rs[] = {0, 1, 2, 127, 128, 129, 257, 300, 4096, 131073, ((int64_t)1 << 31) + 1};
  const int Cs[] = {0, 4, 6, 8, 12, 24, 40, 72, 136, 256, 264, 2048};
  for (int64_t R : Rs)
    for (int C : Cs) {
      std::printf("spml_bn_workspace_bytes R=%lld C=%d -> %zu\n", (long long)R, C, spml_bn_workspace_bytes(R, C));
      ++n_calls;
    }
  workspace.resize(spml_bn_workspace_bytes(300, 40) + 16);
  for (const Entry& e : kEntries) sweep(e);
  std::printf("bn_host_check: %ld calls, %ld skipped%s\n", n_calls, n_skipped,
              have_device ? " (a device is present: calls that could launch were not made)" : "");
  return 0;
}
