// Host-side check of the NLL entry points (csrc/nll.hip), single-problem and batched: the offset / workspace
// arithmetic and the argument validation, which run before anything is launched -- no GPU is needed or touched.
// Meant for a host sanitizer build:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined \
//         tools/nll_host_check.cpp spml_amd/csrc/nll.hip spml_amd/csrc/nll_de3.hip \
//         spml_amd/csrc/nll_dp3.hip spml_amd/csrc/misc.hip -o nll_host_check && ./nll_host_check
//
// Every call below returns from the validation (a missing or short workspace, no pixels, or an earlier refusal).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spml_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static std::vector<int64_t> prefix(const std::vector<int64_t>& sizes) {
  std::vector<int64_t> off(sizes.size() + 1, 0);                 // exactly n + 1 entries: a read past them is caught
  for (size_t i = 0; i < sizes.size(); ++i) off[i + 1] = off[i] + sizes[i];
  return off;
}

// what the library must ask for at least: the split-f16 fragments of the padded tiles (4 arrays of 1 KB per tile and
// k-step, 4 of 2 KB per tile and d-tile)
static size_t fragments_lower_bound(const std::vector<int64_t>& P, const std::vector<int64_t>& M, int D) {
  const size_t KS = (D + 15) / 16, DT = (D + 31) / 32;
  size_t pt = 0, mt = 0;
  for (size_t i = 0; i < P.size(); ++i) { pt += (P[i] + 31) / 32; mt += (M[i] + 31) / 32; }
  return (pt + mt) * (2 * KS * 1024 + 2 * DT * 2048);
}

static int fwd(const std::vector<int64_t>& p_off, const std::vector<int64_t>& m_off, int n, int D, int mode, void* ws,
               size_t ws_bytes) {
  static float f[4];
  static int64_t i64[4];
  return spml_segsort_nll_batched_fwd_f32(f, i64, i64, p_off.data(), f, i64, m_off.data(), n, D, 10.0f, mode, f, f, ws,
                                          ws_bytes, nullptr);
}
static int bwd(const std::vector<int64_t>& p_off, const std::vector<int64_t>& m_off, int n, int D, int mode, void* ws,
               size_t ws_bytes) {
  static float f[4];
  static int64_t i64[4];
  return spml_segsort_nll_batched_bwd_f32(f, i64, i64, p_off.data(), f, i64, m_off.data(), n, D, 10.0f, mode, f, f, f,
                                          f, ws, ws_bytes, nullptr);
}

// ---- single-problem entry points ----
// workspace holds `bytes` bytes (null: none); the tensors are a few elements each: nothing below reads or launches
static int fwd1(int64_t P, int64_t M, int D, int mode, void* ws, size_t bytes, bool tensors = true) {
  static float f[4];
  static int64_t i64[4];
  return spml_segsort_nll_fwd_f32(tensors ? f : nullptr, i64, i64, P, f, i64, M, D, 10.0f, mode, f, f, ws, bytes,
                                  nullptr);
}
static int bwd1(int64_t P, int64_t M, int D, int mode, void* ws, size_t bytes, bool tensors = true) {
  static float f[4];
  static int64_t i64[4];
  return spml_segsort_nll_bwd_f32(f, i64, i64, P, f, i64, M, D, 10.0f, mode, f, f, f, tensors ? f : nullptr, -1, ws,
                                  bytes, nullptr);
}

// spml_segsort_nll_workspace_bytes of (P, M, D) with SPML_NLL_TCACHE_MB unset (tcache_mb = 0) or set, deterministic
// mode off / on.  The numbers were printed by a build of the commit BEFORE the host dispatch of nll.hip was split into
// functions (6d61455), not by the code under test: they pin the workspace layout against accidental change.  Every
// k-step bucket (D = 16, 34, 64, 66, 130, 258, 514 / 528), two forward chunks (M > 3072), a wide shape whose weight
// tiles take one strip and, with 1-MB caches, several; D = 529 has no kernel and keeps its (meaningless) size.
static const struct { int64_t P, M; int D, tcache_mb; size_t plain, det; } kWorkspace[] = {
    {70, 40, 16, 0, 60416u, 68608u},
    {257, 130, 34, 0, 294656u, 338176u},
    {1500, 4000, 34, 0, 3364608u, 4452608u},
    {3000, 700, 64, 0, 2868992u, 3229440u},
    {50000, 3100, 64, 0, 56032000u, 57621248u},
    {0, 5, 64, 0, 16896u, 33280u},
    {1000, 97, 66, 0, 894208u, 961792u},
    {700, 3100, 66, 0, 2773504u, 4412416u},
    {257, 130, 130, 0, 564992u, 731392u},
    {257, 130, 258, 0, 1023744u, 1353984u},
    {600, 90, 514, 0, 3616000u, 4010752u},
    {6000, 90, 514, 0, 31996928u, 32391680u},
    {6000, 90, 514, 1, 29342720u, 29737472u},
    {200, 40, 528, 0, 1401856u, 1672192u},
    {200, 40, 529, 0, 1383424u, 1654272u},
};

static void check_single() {
  for (const auto& k : kWorkspace) {
    if (k.tcache_mb) setenv("SPML_NLL_TCACHE_MB", "1", 1);
    else unsetenv("SPML_NLL_TCACHE_MB");
    for (int det = 0; det < 2; ++det) {
      spml_set_deterministic(det);
      EXPECT(spml_segsort_nll_workspace_bytes(k.P, k.M, k.D) == (det ? k.det : k.plain));
    }
  }
  unsetenv("SPML_NLL_TCACHE_MB");
  spml_set_deterministic(0);
  EXPECT(spml_segsort_nll_workspace_bytes(-1, 40, 64) == 0);
  EXPECT(spml_segsort_nll_workspace_bytes(70, 0, 64) == 0);
  EXPECT(spml_segsort_nll_workspace_bytes(70, 40, 0) == 0);

  for (int det = 0; det < 2; ++det) {
    spml_set_deterministic(det);
    for (int D : {16, 34, 64, 66, 130, 258, 514, 528}) {
      for (int mode : {0, 1, 4, 5, 7}) {
        const size_t need = spml_segsort_nll_workspace_bytes(70, 40, D);
        EXPECT(fwd1(70, 40, D, mode, nullptr, 0) == SPML_ERR_WORKSPACE);
        EXPECT(bwd1(70, 40, D, mode, nullptr, 0) == SPML_ERR_WORKSPACE);
        EXPECT(fwd1(70, 40, D, mode, nullptr, need) == SPML_ERR_WORKSPACE);
        char small[64];
        EXPECT(fwd1(70, 40, D, mode, small, need - 1) == SPML_ERR_WORKSPACE);     // one byte short
        EXPECT(bwd1(70, 40, D, mode, small, need - 1) == SPML_ERR_WORKSPACE);
        // no pixels: a sufficient workspace, and nothing is launched or written
        std::vector<char> enough(spml_segsort_nll_workspace_bytes(0, 40, D));
        EXPECT(fwd1(0, 40, D, mode, enough.data(), enough.size()) == SPML_OK);
        EXPECT(bwd1(0, 40, D, mode, enough.data(), enough.size()) == SPML_OK);
        EXPECT(fwd1(0, 40, D, mode, enough.data(), enough.size() - 1) == SPML_ERR_WORKSPACE);
      }
      // refusals come before the workspace is looked at
      EXPECT(fwd1(70, 40, D, 0, nullptr, 0, false) == SPML_ERR_INVALID_ARG);      // null tensors
      EXPECT(bwd1(70, 40, D, 0, nullptr, 0, false) == SPML_ERR_INVALID_ARG);
      EXPECT(fwd1(70, 40, D, 8, nullptr, 0) == SPML_ERR_INVALID_ARG);             // mode out of range
      EXPECT(bwd1(70, 40, D, 8, nullptr, 0) == SPML_ERR_INVALID_ARG);
      EXPECT(fwd1(70, 40, D, -1, nullptr, 0) == SPML_ERR_INVALID_ARG);
      EXPECT(bwd1(70, 40, D, -1, nullptr, 0) == SPML_ERR_INVALID_ARG);
      EXPECT(fwd1(-1, 40, D, 0, nullptr, 0) == SPML_ERR_INVALID_ARG);
      EXPECT(bwd1(70, 0, D, 0, nullptr, 0) == SPML_ERR_INVALID_ARG);
    }
    EXPECT(fwd1(70, 40, 529, 0, nullptr, 0) == SPML_ERR_UNSUPPORTED);             // D > 528: no kernel
    EXPECT(bwd1(70, 40, 529, 4, nullptr, 0) == SPML_ERR_UNSUPPORTED);
    EXPECT(fwd1(0, 40, 529, 0, nullptr, 0) == SPML_ERR_UNSUPPORTED);
    EXPECT(fwd1(70, 40, 0, 0, nullptr, 0) == SPML_ERR_INVALID_ARG);
  }
  spml_set_deterministic(0);
}

int main() {
  check_single();
  const int C32 = SPML_NLL_CODE32;
  EXPECT(spml_segsort_nll_batched_supported(66, C32) == 1);
  EXPECT(spml_segsort_nll_batched_supported(65, C32 | SPML_NLL_TAGSET) == 1);
  EXPECT(spml_segsort_nll_batched_supported(80, C32 | SPML_NLL_PLAIN) == 1);
  EXPECT(spml_segsort_nll_batched_supported(64, C32) == 0);
  EXPECT(spml_segsort_nll_batched_supported(81, C32) == 0);
  EXPECT(spml_segsort_nll_batched_supported(32, C32) == 0);
  EXPECT(spml_segsort_nll_batched_supported(66, SPML_NLL_LABEL) == 0);       // 64-bit codes
  EXPECT(spml_segsort_nll_batched_supported(66, 8) == 0);
  EXPECT(spml_segsort_nll_batched_supported(0, C32) == 0);

  // the size lists of the tests: a problem below a tile, an empty one, one prototype, two prototype tiles
  const std::vector<int64_t> P = {64, 31, 0, 1000, 33}, M = {5, 1, 3, 97, 33};
  const std::vector<int64_t> p_off = prefix(P), m_off = prefix(M);
  for (int D : {65, 66, 80}) {
    for (int det = 0; det < 2; ++det) {
      spml_set_deterministic(det);
      const size_t need = spml_segsort_nll_batched_workspace_bytes(5, p_off.data(), m_off.data(), D);
      EXPECT(need >= fragments_lower_bound(P, M, D));
      EXPECT(need < (size_t)64 << 20);
      if (det) {
        spml_set_deterministic(0);
        const size_t plain = spml_segsort_nll_batched_workspace_bytes(5, p_off.data(), m_off.data(), D);
        spml_set_deterministic(1);
        EXPECT(need >= plain + (size_t)m_off[5] * D * 8);        // the fixed-point prototype gradient
      }
      for (int mode : {C32, C32 | SPML_NLL_TAGSET, C32 | SPML_NLL_PLAIN}) {
        EXPECT(fwd(p_off, m_off, 5, D, mode, nullptr, 0) == SPML_ERR_WORKSPACE);
        EXPECT(bwd(p_off, m_off, 5, D, mode, nullptr, 0) == SPML_ERR_WORKSPACE);
        char small[64];
        EXPECT(fwd(p_off, m_off, 5, D, mode, small, need - 1) == SPML_ERR_WORKSPACE);
        EXPECT(bwd(p_off, m_off, 5, D, mode, small, need - 1) == SPML_ERR_WORKSPACE);
      }
    }
    spml_set_deterministic(0);
  }
  // a single problem asks for no less than its fragments, and 33 problems cross the 32-problem descriptor
  {
    const std::vector<int64_t> p1 = prefix({1000}), m1 = prefix({97});
    EXPECT(spml_segsort_nll_batched_workspace_bytes(1, p1.data(), m1.data(), 66) >= fragments_lower_bound({1000}, {97}, 66));
    EXPECT(fwd(p1, m1, 1, 66, C32, nullptr, 0) == SPML_ERR_WORKSPACE);
    std::vector<int64_t> p33, m33;
    for (int i = 0; i < 33; ++i) { p33.push_back(1 + (i * 37) % 90); m33.push_back(1 + (i * 11) % 40); }
    const std::vector<int64_t> po = prefix(p33), mo = prefix(m33);
    EXPECT(spml_segsort_nll_batched_workspace_bytes(33, po.data(), mo.data(), 66) >= fragments_lower_bound(p33, m33, 66));
    EXPECT(fwd(po, mo, 33, 66, C32, nullptr, 0) == SPML_ERR_WORKSPACE);
    EXPECT(bwd(po, mo, 33, 66, C32, nullptr, 0) == SPML_ERR_WORKSPACE);
  }
  // nothing to do
  {
    const std::vector<int64_t> none = {0};
    EXPECT(fwd(none, none, 0, 66, C32, nullptr, 0) == SPML_OK);
    EXPECT(bwd(none, none, 0, 66, C32, nullptr, 0) == SPML_OK);
    EXPECT(spml_segsort_nll_batched_fwd_f32(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 66, 10.f,
                                            C32, nullptr, nullptr, nullptr, 0, nullptr) == SPML_OK);
    const std::vector<int64_t> pz = prefix({0, 0, 0}), mz = prefix({4, 0, 7});
    EXPECT(fwd(pz, mz, 3, 66, C32, nullptr, 0) == SPML_OK);
    EXPECT(bwd(pz, mz, 3, 66, C32, nullptr, 0) == SPML_OK);
  }
  // refusals
  {
    const std::vector<int64_t> pp = prefix({64, 10}), m_none = prefix({5, 0});
    EXPECT(fwd(pp, m_none, 2, 66, C32, nullptr, 0) == SPML_ERR_INVALID_ARG);            // pixels without prototypes
    EXPECT(bwd(pp, m_none, 2, 66, C32, nullptr, 0) == SPML_ERR_INVALID_ARG);
    EXPECT(spml_segsort_nll_batched_workspace_bytes(2, pp.data(), m_none.data(), 66) == 0);
    const std::vector<int64_t> down = {0, 64, 32}, mm = prefix({5, 5});
    EXPECT(fwd(down, mm, 2, 66, C32, nullptr, 0) == SPML_ERR_INVALID_ARG);              // decreasing offsets
    const std::vector<int64_t> shifted = {3, 64, 96};
    EXPECT(fwd(shifted, mm, 2, 66, C32, nullptr, 0) == SPML_ERR_INVALID_ARG);           // does not start at 0
    EXPECT(fwd(p_off, m_off, -1, 66, C32, nullptr, 0) == SPML_ERR_INVALID_ARG);
    EXPECT(fwd(p_off, m_off, 5, 0, C32, nullptr, 0) == SPML_ERR_INVALID_ARG);
    EXPECT(fwd(p_off, m_off, 5, 66, 8, nullptr, 0) == SPML_ERR_INVALID_ARG);
    EXPECT(fwd(p_off, m_off, 5, 64, C32, nullptr, 0) == SPML_ERR_UNSUPPORTED);
    EXPECT(bwd(p_off, m_off, 5, 32, C32, nullptr, 0) == SPML_ERR_UNSUPPORTED);
    EXPECT(fwd(p_off, m_off, 5, 66, SPML_NLL_LABEL, nullptr, 0) == SPML_ERR_UNSUPPORTED);
    EXPECT(spml_segsort_nll_batched_workspace_bytes(5, p_off.data(), m_off.data(), 64) == 0);
    EXPECT(spml_segsort_nll_batched_workspace_bytes(5, nullptr, m_off.data(), 66) == 0);
    EXPECT(spml_segsort_nll_batched_workspace_bytes(-1, p_off.data(), m_off.data(), 66) == 0);
    EXPECT(spml_segsort_nll_batched_fwd_f32(nullptr, nullptr, nullptr, p_off.data(), nullptr, nullptr, m_off.data(), 5,
                                            66, 10.f, C32, nullptr, nullptr, nullptr, 0, nullptr) == SPML_ERR_INVALID_ARG);
  }
  // sizes near the top of the domain: the byte counts must not wrap
  {
    const std::vector<int64_t> pb = prefix({(int64_t)1 << 30}), mb = prefix({(int64_t)1 << 20});
    const size_t need = spml_segsort_nll_batched_workspace_bytes(1, pb.data(), mb.data(), 80);
    EXPECT(need > ((size_t)1 << 30) / 32 * 5 * 1024 * 2);
    const std::vector<int64_t> over = prefix({((int64_t)1 << 30) + 1});
    EXPECT(spml_segsort_nll_batched_workspace_bytes(1, over.data(), mb.data(), 80) == 0);
  }
  std::printf(failures ? "%d check(s) FAILED\n" : "nll_host_check: all checks passed\n", failures);
  return failures ? 1 : 0;
}
