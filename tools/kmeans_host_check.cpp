// Host-side check of the k-means entry points (csrc/kmeans.hip): the route, the workspace arithmetic and the argument
// validation, which run before anything is launched -- no GPU is needed or touched.  Meant for a host sanitizer build:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined \
//         tools/kmeans_host_check.cpp spml_amd/csrc/kmeans.hip spml_amd/csrc/kmeans64.hip \
//         spml_amd/csrc/kmeans64k.hip spml_amd/csrc/kmeans_big.hip spml_amd/csrc/segsum.hip \
//         spml_amd/csrc/normalize.hip spml_amd/csrc/misc.hip -o kmeans_host_check && ./kmeans_host_check
//
// Every call below returns from the validation (a missing or short workspace, no pixels, or an earlier refusal).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spml_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (failures < 20) std::printf("FAILED line %d: %s  [%s]\n", __LINE__, #cond, what); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static const char* const kNames[] = {"generic",        "mfma_f16x2_bigk", "mfma_f16x2",     "mfma_f16x2_v3",
                                     "mfma_f16x2_v3p", "mfma_f16x2_v4p",  "mfma_f16x2_v3k", "mfma_f16x2_v4k"};
static int name_index(const char* n) {
  for (int i = 0; i < 8; ++i)
    if (n && !std::strcmp(n, kNames[i])) return i;
  return -1;
}

// a few elements each: nothing below reads them or launches
alignas(16) static float f[4];
static int64_t i64[4];

struct Shape { int64_t P; int D, K, n_img; int64_t L; };

static int run(const Shape& s, int it, int flags, void* ws, size_t bytes) {
  return spml_kmeans_run_f32(f, s.P, s.D, i64, s.n_img, s.L, s.K, i64, it, i64, nullptr, flags, ws, bytes, nullptr);
}
static int assign(const Shape& s, int flags, void* ws, size_t bytes) {
  return spml_kmeans_assign_f32(f, s.P, s.D, i64, s.n_img, s.L, s.K, f, i64, flags, ws, bytes, nullptr);
}
static int fused(const Shape& s, int flags, void* ws, size_t bytes) {
  return spml_kmeans_fused_pass_f32(f, s.P, s.D, i64, s.n_img, s.L, s.K, f, i64, f, flags, ws, bytes, nullptr);
}
static int preconvert(const Shape& s, void* ws, size_t bytes) {
  return spml_kmeans_preconvert_f32(f, s.P, s.D, i64, s.n_img, s.L, s.K, ws, bytes, nullptr);
}
static int profiled(const Shape& s, int it, void* ws, size_t bytes, size_t clocks_len) {
  return spml_kmeans_run_profiled_f32(f, s.P, s.D, i64, s.n_img, s.L, s.K, i64, it, i64, 0, ws, bytes,
                                      reinterpret_cast<uint64_t*>(i64), clocks_len, nullptr);
}

static const int kFlags[] = {0, 1, 4, 8, 16, 32, 512, 1024, 2048, 8 | 512, 32 | 256};
static int seen[8];

static void check_shape(const Shape& s) {
  char what[128];
  std::snprintf(what, sizeof(what), "P=%lld D=%d K=%d n_img=%d L=%lld", (long long)s.P, s.D, s.K, s.n_img, (long long)s.L);
  // the size does not depend on the deterministic mode, and holds at least the int32 labels and the fp32 prototypes
  spml_set_deterministic(1);
  const size_t need = spml_kmeans_workspace_bytes(s.P, s.D, s.K, s.n_img, s.L);
  spml_set_deterministic(0);
  EXPECT(need == spml_kmeans_workspace_bytes(s.P, s.D, s.K, s.n_img, s.L));
  EXPECT(need >= (size_t)s.P * 4 + (size_t)s.n_img * s.K * s.D * 12);
  const bool refused = s.D > 1088 && s.K > 64;              // no kernel: refused before the workspace is looked at
  const int short_ws = refused ? SPML_ERR_UNSUPPORTED : SPML_ERR_WORKSPACE;
  char small[64];
  const Shape none = {0, s.D, s.K, s.n_img, s.L};           // no pixels: a sufficient workspace, nothing is launched
  const size_t need0 = spml_kmeans_workspace_bytes(0, s.D, s.K, s.n_img, s.L);
  const bool try_none = need0 <= ((size_t)4 << 20);         // (the larger ones are not worth allocating here)
  std::vector<char> enough(try_none ? need0 : 1);

  for (int it = 0; it < 4; ++it) {
    for (int given = 0; given < 2; ++given) {
      for (int flags : kFlags) {
        const int name = name_index(spml_kmeans_path_name(s.P, s.D, s.K, s.n_img, s.L, it, given, flags));
        EXPECT(name >= 0);
        if (name < 0) continue;
        ++seen[name];
        if (flags & SPML_KMEANS_FORCE_GENERIC) EXPECT(name == 0);
        if (name >= 4) EXPECT(given ? (flags & SPML_KMEANS_WS_PRECONVERTED) != 0 : it >= 2);      // pre-converted tiles
        if (given && it != 1) continue;                      // (the entry points with prototypes make one pass)
        if (!given) {
          EXPECT(run(s, it, flags, nullptr, 0) == short_ws);
          EXPECT(run(s, it, flags, nullptr, need) == short_ws);
          EXPECT(run(s, it, flags, small, need - 1) == short_ws);
          if (!try_none) continue;
          EXPECT(run(none, it, flags, enough.data(), enough.size()) == (refused ? SPML_ERR_UNSUPPORTED : SPML_OK));
          EXPECT(run(none, it, flags, enough.data(), enough.size() - 1) == short_ws);
        } else {
          EXPECT(assign(s, flags, nullptr, 0) == short_ws);
          EXPECT(assign(s, flags, small, need - 1) == short_ws);
          EXPECT(fused(s, flags, nullptr, 0) == short_ws);
          EXPECT(fused(s, flags, small, need - 1) == short_ws);
          if (!try_none) continue;
          EXPECT(assign(none, flags, enough.data(), enough.size()) == (refused ? SPML_ERR_UNSUPPORTED : SPML_OK));
          EXPECT(fused(none, flags | (7 << 16), enough.data(), enough.size()) == (refused ? SPML_ERR_UNSUPPORTED : SPML_OK));
        }
      }
    }
    if (it == 0) continue;
    // the profiled run: layout and route agree (two entries per fused iteration on v4k; the slab area of the
    // workspace holds ceil(512 / n_img) workgroups per image)
    int passes = -1, wgs = -1;
    const int rc = spml_kmeans_profile_layout(s.P, s.D, s.K, s.n_img, s.L, it, &passes, &wgs);
    const int name = name_index(spml_kmeans_path_name(s.P, s.D, s.K, s.n_img, s.L, it, 0, 0));
    EXPECT(rc == (name >= 2 ? SPML_OK : SPML_ERR_UNSUPPORTED));
    if (rc == SPML_OK) {
      EXPECT(passes == (name == 7 ? 2 * it : it + 1));
      EXPECT(wgs >= s.n_img && wgs % s.n_img == 0 && wgs / s.n_img <= (512 + s.n_img - 1) / s.n_img);
      EXPECT(wgs / s.n_img <= (s.L + 31) / 32);
      EXPECT(profiled(s, it, nullptr, 0, (size_t)passes * wgs * 2 - 1) == SPML_ERR_WORKSPACE);      // short clocks
      EXPECT(profiled(s, it, nullptr, 0, (size_t)passes * wgs * 2) == SPML_ERR_WORKSPACE);
    } else {
      EXPECT(profiled(s, it, nullptr, 0, 1 << 20) == SPML_ERR_UNSUPPORTED);
    }
  }
  EXPECT(preconvert(s, nullptr, 0) == SPML_ERR_WORKSPACE);
  EXPECT(preconvert(s, small, need - 1) == SPML_ERR_WORKSPACE);
  // no pixels: there is no tile to convert, and nothing to assign
  if (try_none) EXPECT(preconvert(none, enough.data(), enough.size()) == SPML_ERR_UNSUPPORTED);
  if (try_none && !refused) EXPECT(assign(none, SPML_KMEANS_WS_PRECONVERTED, enough.data(), enough.size()) == SPML_OK);
}

int main() {
  const char* what = "arguments";
  // the argument grid of tests/test_cabi_exports.py::test_kmeans_route_table and of the parent comparison
  const int Ds[] = {10, 18, 32, 34, 37, 64, 66, 69, 128, 130, 136, 256, 258, 264, 320, 322, 514, 515, 1090};
  const int Ks[] = {1, 9, 36, 48, 49, 64, 65, 80, 100, 144, 145, 256, 257, 1024, 4097};
  const int Ns[] = {1, 3, 16};
  const int64_t Ls[] = {1, 31, 64, 4099, 263169};
  for (int D : Ds)
    for (int K : Ks)
      for (int n : Ns)
        for (int64_t L : Ls) check_shape({n * L, D, K, n, L});
  for (int i = 0; i < 8; ++i) EXPECT(seen[i] > 0);          // the grid reaches every path
  // extremes: pixel counts next to 2^31 (the many-cluster kernels' limit), 65536 clusters, one-pixel images, many
  // images -- the byte counts must not wrap and the grids stay inside the workspace
  const int64_t big = ((int64_t)1 << 31);
  for (int64_t P : {big - 1, big, big + 1})
    for (int D : {34, 66, 258, 514, 1090})
      for (int K : {36, 144, 1024, 65536, 65537}) check_shape({P, D, K, 1, P});
  for (int D : {66, 258, 514})
    for (int K : {9, 36, 100, 65536}) {
      check_shape({4096, D, K, 4096, 1});
      check_shape({(int64_t)4096 * 4099, D, K, 4096, 4099});
      check_shape({1, D, K, 1, 1});
    }
  EXPECT(spml_kmeans_workspace_bytes((big - 1), 514, 65536, 1, big - 1) > (size_t)65536 * 514 * 8);

  // refusals
  const Shape ok = {4099, 66, 36, 1, 4099};
  EXPECT(std::strcmp(spml_kmeans_path_name(-1, 66, 36, 1, 4099, 3, 0, 0), "invalid") == 0);
  EXPECT(std::strcmp(spml_kmeans_path_name(4099, 0, 36, 1, 4099, 3, 0, 0), "invalid") == 0);
  EXPECT(std::strcmp(spml_kmeans_path_name(4099, 66, 36, 1, 0, 3, 0, 0), "invalid") == 0);
  EXPECT(spml_kmeans_workspace_bytes(-1, 66, 36, 1, 4099) == 0);
  EXPECT(spml_kmeans_workspace_bytes(4099, 66, 0, 1, 4099) == 0);
  EXPECT(spml_kmeans_workspace_bytes(4099, 66, 36, 0, 4099) == 0);
  int passes = 0, wgs = 0;
  EXPECT(spml_kmeans_profile_layout(4099, 66, 36, 1, 4099, 0, &passes, &wgs) == SPML_ERR_INVALID_ARG);
  EXPECT(spml_kmeans_profile_layout(4099, 66, 36, 1, 4099, 3, nullptr, &wgs) == SPML_ERR_INVALID_ARG);
  EXPECT(run(ok, -1, 0, nullptr, 0) == SPML_ERR_INVALID_ARG);
  EXPECT(run({-1, 66, 36, 1, 4099}, 3, 0, nullptr, 0) == SPML_ERR_INVALID_ARG);
  EXPECT(run({4099, 66, 36, 1, 0}, 3, 0, nullptr, 0) == SPML_ERR_INVALID_ARG);
  EXPECT(spml_kmeans_run_f32(f, 4099, 66, i64, 1, 4099, 36, nullptr, 3, i64, nullptr, 0, nullptr, 0, nullptr) ==
         SPML_ERR_INVALID_ARG);
  EXPECT(spml_kmeans_assign_f32(f, 4099, 66, i64, 1, 4099, 36, nullptr, i64, 0, nullptr, 0, nullptr) == SPML_ERR_INVALID_ARG);
  EXPECT(spml_kmeans_fused_pass_f32(f, 4099, 66, i64, 1, 4099, 36, f, i64, nullptr, 0, nullptr, 0, nullptr) ==
         SPML_ERR_INVALID_ARG);
  EXPECT(spml_kmeans_preconvert_f32(nullptr, 4099, 66, i64, 1, 4099, 36, nullptr, 0, nullptr) == SPML_ERR_INVALID_ARG);
  EXPECT(profiled(ok, 0, nullptr, 0, 1 << 20) == SPML_ERR_INVALID_ARG);
  std::printf(failures ? "%d check(s) FAILED\n" : "kmeans_host_check: all checks passed\n", failures);
  return failures ? 1 : 0;
}
