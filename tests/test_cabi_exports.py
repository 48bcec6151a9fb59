"""The C-ABI shared library loads without a GPU and exports every symbol that
include/spml_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
  text = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return sorted(set(re.findall(r'\b(spml_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def lib_path():
  from spml_amd import _build
  return _build.build(verbose=False)


def test_header_declares_the_hot_path():
  names = declared_symbols()
  for must in ('spml_normalize_concat_loc_f32', 'spml_kmeans_run_f32', 'spml_kmeans_assign_f32',
               'spml_segment_sum_normalize_f32', 'spml_segsort_nll_fwd_f32',
               'spml_segsort_nll_bwd_f32', 'spml_segsort_nll_path_name', 'spml_topk_affinity_f32',
               'spml_status_string'):
    assert must in names


def test_library_exports_every_declared_symbol(lib_path):
  handle = ctypes.CDLL(lib_path)
  missing = [n for n in declared_symbols() if not hasattr(handle, n)]
  assert not missing, missing


def test_ffi_table_matches_header(lib_path):
  from spml_amd import _ffi
  assert sorted(_ffi.EXPORTS) == declared_symbols()
  lib = _ffi.lib()
  import re
  hdr = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  want = int(re.search(r'#define SPML_ABI_VERSION (\d+)', hdr).group(1))
  assert lib.spml_abi_version() == want == _ffi.ABI_VERSION
  assert lib.spml_status_string(0) == b'ok'
  assert b'workspace' in lib.spml_status_string(-3)
  # host-only size queries
  assert lib.spml_kmeans_workspace_bytes(1000, 66, 36, 2, 500) > 1000 * 4
  assert lib.spml_segsort_nll_workspace_bytes(1000, 100, 64) > 0
  assert lib.spml_topk_workspace_bytes(100, 100, 64, 5) > 0
  assert lib.spml_kmeans_workspace_bytes(-1, 66, 36, 2, 500) == 0
  # host-only route query of the NLL: the buffer must hold the name
  assert _ffi.segsort_nll_path_name(1000, 100, 100, 0) == 'fwd<9,1,label,c64>'
  small = ctypes.create_string_buffer(4)
  assert lib.spml_segsort_nll_path_name(1000, 100, 100, 0, 0, -1, small, 4) == -1 and small.raw[3:] == b'\0'


def test_no_cpu_fallback():
  """A CPU tensor must raise, never silently compute."""
  import torch
  from spml_amd import _ffi
  import spml_amd.utils.segsort.common as sc
  import spml_amd.utils.general.common as gc
  x = torch.randn(10, 8)
  with pytest.raises(_ffi.SpmlHipError):
    gc.normalize_embedding(x)
  with pytest.raises(_ffi.SpmlHipError):
    sc.calculate_prototypes_from_labels(x, torch.zeros(10, dtype=torch.long), 1)
  with pytest.raises(_ffi.SpmlHipError):
    sc.kmeans_with_initial_labels(x, torch.zeros(10, dtype=torch.long), 1, 2)


def test_product_does_not_import_the_oracle():
  """Nothing under spml_amd/ may reference oracle/ (it is test infrastructure)."""
  bad = []
  for dirpath, _, files in os.walk(os.path.join(ROOT, 'spml_amd')):
    for f in files:
      if f.endswith('.py'):
        src = open(os.path.join(dirpath, f)).read()
        if re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M):
          bad.append(os.path.join(dirpath, f))
  assert not bad, bad


def test_bench_refuses_to_run_without_a_gpu():
  """bench.py measures the HIP path only: without a GPU it must stop, not fall back."""
  import subprocess
  import sys
  import torch
  if torch.cuda.is_available():
    pytest.skip('a GPU is present')
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '1', '--warmup', '0'],
                     capture_output=True, text=True, timeout=600)
  assert r.returncode != 0
  assert 'no CPU fallback' in (r.stderr + r.stdout)


@pytest.mark.parametrize('source,kernel', [('nll_de3.hip', 'nll_bwd_de3'), ('nll_dp3.hip', 'nll_bwd_dp3')])
def test_hand_assigned_registers_of_the_pipelined_nll_kernels_are_the_kernels_alone(source, kernel):
  """csrc/nll_de3.hip / nll_dp3.hip name their pipeline registers (v96..v255, a0..a255) in the text of single-instruction
  asm statements and confine the compiler to v0..v95: no compiler-generated instruction may touch a
  hand-assigned register, every inline-asm statement must be one instruction, and the generated register map
  must be the committed one (tools/gen_nll_de3.py)."""
  import subprocess
  import tempfile
  from spml_amd import _build
  inc = os.path.join(ROOT, 'spml_amd', 'csrc', 'nll_de3_regs.inc')
  with tempfile.TemporaryDirectory() as tmp:
    fresh = os.path.join(tmp, 'regs.inc')                  # (written next to nothing: the source tree stays as it is)
    subprocess.run(['python', os.path.join(ROOT, 'tools', 'gen_nll_de3.py'), fresh], check=True, capture_output=True)
    assert open(fresh).read() == open(inc).read(), 'nll_de3_regs.inc is not what tools/gen_nll_de3.py writes'
  with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, 'de3.s')
    cmd = [_build._hipcc()] + _build.FLAGS + ['-S', '--cuda-device-only', os.path.join(_build.CSRC, source),
                                              '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
  kernels = re.findall(r'^(_ZN4spml\S*' + kernel + r'\S*):[^\n]*\n(.*?)s_endpgm', text, flags=re.S | re.M)
  assert len(kernels) == 2, [k for k, _ in kernels]
  for name, body in kernels:
    in_asm, n_asm = False, 0
    for line in body.splitlines():
      code = line.split(';')[0].strip() if not line.strip().startswith(';;#') else line.strip()
      if code.startswith(';;#ASMSTART'):
        in_asm, n_asm = True, 0
        continue
      if code.startswith(';;#ASMEND'):
        in_asm = False
        continue
      if not code or code.endswith(':') or code.startswith('.'):
        continue
      if in_asm:
        n_asm += 1
        assert n_asm == 1 or code.startswith(('v_accvgpr_write_b32', 'v_mov_b32', 's_nop', 'global_load_lds', 's_mov_b32 m0', 's_barrier', 's_waitcnt')), \
            '%s: multi-instruction asm statement: %s' % (name, code)
        continue
      regs = re.findall(r'\bv(\d+)\b|\bv\[(\d+):(\d+)\]|\ba(\d+)\b|\ba\[(\d+):(\d+)\]', code)
      for v1, v2, v3, a1, a2, a3 in regs:
        assert not (a1 or a2), '%s: compiler-generated accumulation-register access: %s' % (name, code)
        hi = int(v1) if v1 else int(v3)
        assert hi < 96, '%s: compiler-generated access to a hand-assigned register: %s' % (name, code)
    assert body.count('v_mfma_f32_32x32x16_f16') >= 2 * 4 * 24, name      # two step versions x four steps x 24 slots
    assert 'scratch_' not in body, name + ' spills'
  assert '.amdhsa_accum_offset 256' in text and '.amdhsa_next_free_vgpr 512' in text


def test_hand_issued_instructions_of_the_kmeans_passes_keep_their_distances():
  """csrc/kmeans64.hip and kmeans64k.hip issue their LDS reads and every MFMA from inline asm, which hipcc does not see
  into: no wait states are inserted for them.  tools/check_asm_hazards.py re-derives the hazards from the compiled
  kernels (a register read while an LDS read into it is outstanding; a vector-ALU write straight before an MFMA that
  reads it; an MFMA result read too early; a dependent MFMA straight behind its producer -- the hardware interlocks
  none of them: tools/hw_probes/mfma_chain.hip, mfma_valu_raw.hip) for every instantiation (48 of kmeans_pass64, 16 of
  kmeans_assign64k + 16 of kmeans_accum64k); nothing may spill."""
  import subprocess
  import sys
  import tempfile
  from spml_amd import _build
  for src, kern, count in (('kmeans64.hip', 'kmeans_pass64', 48), ('kmeans64k.hip', '64k', 32)):
    with tempfile.TemporaryDirectory() as tmp:
      out = os.path.join(tmp, 'k.s')
      cmd = [_build._hipcc()] + _build.FLAGS + ['-S', '--cuda-device-only', os.path.join(_build.CSRC, src), '-o', out]
      r = subprocess.run(cmd, capture_output=True, text=True)
      assert r.returncode == 0, r.stderr[-2000:]
      assert 'scratch_' not in open(out).read(), src
      chk = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_asm_hazards.py'), out, kern],
                           capture_output=True, text=True)
    assert chk.returncode == 0, chk.stdout[-3000:]
    assert chk.stdout.count(' 0 hazards') == count, (src, chk.stdout[-1000:])


def test_profiling_builds_are_stamped_and_refused(monkeypatch):
  """a library compiled with SPML_CONV_EXP / SPML_P64_EXP (kernels that skip work and overwrite outputs)
  must not pass for a product build: the -D set is recorded next to the objects (a plain build after it rebuilds),
  compiled into the library (`spml_build_experiment`) and checked when the library is loaded."""
  from spml_amd import _build, _ffi
  assert _build._experiment_flags() == ([], 0)
  assert _build.is_fresh()                                   # (build() ran in this container: plain stamp)
  assert _ffi.lib().spml_build_experiment() == 0
  monkeypatch.setenv('SPML_CONV_EXP', '3')
  monkeypatch.setenv('SPML_P64_EXP', '16')
  flags, code = _build._experiment_flags()
  assert flags == ['-DSPML_CONV_EXP=3', '-DSPML_P64_EXP=16'] and code == (3 | (16 << 16))
  assert not _build.is_fresh()                               # the objects on disk are of another -D set
  # a fresh load of the plain library under those variables is refused
  monkeypatch.setattr(_ffi, '_lib', None)
  with pytest.raises(_ffi.SpmlHipError, match='profiling build'):
    _ffi.lib()
  monkeypatch.delenv('SPML_CONV_EXP')
  monkeypatch.delenv('SPML_P64_EXP')
  assert _ffi.lib().spml_build_experiment() == 0


def test_upsample_ce_backward_route_of_every_tested_shape(lib_path):
  """spml_upsample_ce_bwd_path_name (a host function: the expression the launch itself uses): the cases of
  tests/test_kernel_branches_gpu.py take the un-tiled gather kernel, those of tests/test_upsample_ce_gpu.py the tiled
  one -- the coverage claim of the two files, checkable without a GPU -- and so do the recipe-sized shapes DESIGN.md
  names."""
  from spml_amd import _ffi
  from test_kernel_branches_gpu import UCE_GATHER_CASES, UCE_TILED_NEIGHBOUR
  from test_upsample_ce_gpu import TILED_CASES
  for must in [(2, 21, 9, 9, 65, 65), (1, 24, 9, 7, 60, 50), (2, 32, 9, 7, 60, 50), (1, 33, 6, 5, 47, 41),
               (1, 64, 4, 4, 40, 40), (1, 64, 17, 17, 65, 65), (1, 21, 5, 6, 41, 47)]:
    assert must in [c[:6] for c in UCE_GATHER_CASES]
  assert len(TILED_CASES) == 8 and UCE_TILED_NEIGHBOUR in TILED_CASES
  for case in UCE_GATHER_CASES:
    assert _ffi.upsample_ce_bwd_path_name(*case[:6]) == 'gather', case
  for case in TILED_CASES:
    assert _ffi.upsample_ce_bwd_path_name(*case[:6]) == 'tiled', case
  for case in [(16, 21, 65, 65, 513, 513), (16, 64, 17, 17, 65, 65), (16, 64, 33, 33, 129, 129), (16, 21, 20, 20, 97, 97)]:
    assert _ffi.upsample_ce_bwd_path_name(*case) == 'gather', case
  assert _ffi.upsample_ce_bwd_path_name(16, 21, 130, 130, 513, 513) == 'tiled'      # the training recipe's own shape
  assert _ffi.upsample_ce_bwd_path_name(65536, 21, 33, 29, 129, 113) == 'gather'    # more images than gridDim.z takes
  assert _ffi.upsample_ce_bwd_path_name(1, 65, 9, 9, 65, 65) == 'unsupported'
  assert {len(_ffi.upsample_ce_bwd_path_name(1, c, 9, 9, 65, 65)) for c in (1, 24, 25, 32, 33, 64)} == {6}


# (D, K, n_img, max_seg_len, iterations, given_centroids, flags) -> path; P = n_img * max_seg_len.  The names follow the
# header's documentation of spml_kmeans_path_name.
KMEANS_ROUTES = [
    (66, 36, 1, 4099, 3, 0, 0, 'mfma_f16x2_v4p'),          # the training shape class: >= 3 passes, K <= 48
    (66, 36, 16, 16900, 10, 0, 0, 'mfma_f16x2_v4p'),
    (258, 36, 1, 263169, 3, 0, 0, 'mfma_f16x2_v4p'),
    (66, 36, 1, 4099, 2, 0, 0, 'mfma_f16x2_v4p'),          # two iterations are three passes
    (37, 25, 1, 4099, 3, 0, 0, 'mfma_f16x2_v4p'),          # location + colours: only on pre-converted tiles ...
    (37, 25, 1, 4099, 1, 0, 0, 'generic'),                 # ... (and D is odd)
    (66, 36, 1, 4099, 3, 0, 16, 'mfma_f16x2_v4p'),         # SEPARATE_PRECONVERT, TWO_KERNEL_FINALIZE: same path
    (66, 36, 1, 4099, 3, 0, 1024, 'mfma_f16x2_v4p'),
    (66, 36, 1, 4099, 3, 0, 512, 'mfma_f16x2_v3p'),        # NO_PASS64
    (130, 64, 1, 4099, 3, 0, 0, 'mfma_f16x2_v3p'),         # 48 < K <= 64
    (66, 49, 3, 4099, 3, 0, 0, 'mfma_f16x2_v3p'),
    (66, 36, 1, 4099, 1, 0, 0, 'mfma_f16x2_v3'),           # < 3 passes
    (256, 16, 1, 4099, 1, 0, 0, 'mfma_f16x2_v3'),
    (66, 36, 1, 4099, 3, 0, 8, 'mfma_f16x2_v3'),           # NO_PRECONVERT
    (66, 36, 1, 4099, 3, 0, 4, 'mfma_f16x2'),              # FORCE_V2
    (10, 9, 1, 289, 3, 0, 0, 'mfma_f16x2'),                # even D outside 32 q + {0, 2}
    (18, 9, 3, 1600, 3, 0, 0, 'mfma_f16x2'),
    (66, 36, 1, 4099, 3, 0, 1, 'generic'),                 # FORCE_GENERIC
    (515, 36, 1, 4099, 3, 0, 0, 'generic'),                # odd D
    (1090, 36, 1, 4099, 3, 0, 0, 'generic'),               # wider than any tile kernel
    (34, 144, 1, 6007, 2, 0, 0, 'mfma_f16x2_v3k'),         # 64 < K <= 256, narrow rows, >= 3 passes
    (66, 256, 3, 6007, 3, 0, 0, 'mfma_f16x2_v3k'),
    (64, 65, 1, 6007, 3, 0, 0, 'mfma_f16x2_v3k'),
    (34, 144, 1, 6007, 1, 0, 0, 'mfma_f16x2_bigk'),        # ... a single iteration is not worth the conversion
    (66, 144, 1, 6007, 3, 0, 8, 'mfma_f16x2_bigk'),        # ... nor is there a kernel without it
    (66, 257, 3, 6007, 3, 0, 0, 'mfma_f16x2_bigk'),
    (514, 1024, 1, 6000, 3, 0, 0, 'mfma_f16x2_bigk'),
    (515, 96, 1, 1000, 3, 0, 0, 'mfma_f16x2_bigk'),
    (258, 144, 1, 263169, 3, 0, 0, 'mfma_f16x2_v4k'),      # 64 < K <= 144 on wide rows
    (130, 144, 2, 5000, 3, 0, 0, 'mfma_f16x2_v4k'),
    (256, 80, 2, 4000, 2, 0, 0, 'mfma_f16x2_v4k'),
    (258, 144, 1, 263169, 3, 0, 2048, 'mfma_f16x2_bigk'),  # NO_V4K
    (258, 144, 1, 263169, 1, 0, 0, 'mfma_f16x2_bigk'),
    (66, 36, 1, 4099, 1, 1, 0, 'mfma_f16x2_v3'),           # given centroids: converted tiles only on the caller's word
    (66, 36, 1, 4099, 1, 1, 32, 'mfma_f16x2_v4p'),         # WS_PRECONVERTED
    (66, 36, 1, 4099, 1, 1, 32 | 512, 'mfma_f16x2_v3p'),
    (66, 64, 1, 4099, 1, 1, 32, 'mfma_f16x2_v3p'),
    (66, 144, 1, 4099, 1, 1, 32, 'mfma_f16x2_v3k'),
    (258, 144, 1, 4099, 1, 1, 32, 'mfma_f16x2_v4k'),
    (258, 144, 1, 4099, 1, 1, 0, 'mfma_f16x2_bigk'),
    (66, 36, 1, 4099, 1, 1, 1, 'generic'),
]


def test_kmeans_route_table(lib_path):
  """The host side of a k-means call decides its route once (csrc/kmeans.hip: kmeans_route); spml_kmeans_path_name,
  spml_kmeans_profile_layout and the run read the same record.  Every path name and every flag that changes one; the
  layout of the profiled run (an iteration of "v4k" is two kernels; no tile kernels, no profile); and the workspace size
  does not depend on the deterministic mode (a workspace sized before the mode was switched on stays valid)."""
  import ctypes
  from spml_amd import _ffi
  lib = _ffi.lib()
  assert {r[7] for r in KMEANS_ROUTES} == {'generic', 'mfma_f16x2', 'mfma_f16x2_v3', 'mfma_f16x2_v3p', 'mfma_f16x2_v4p',
                                           'mfma_f16x2_v3k', 'mfma_f16x2_v4k', 'mfma_f16x2_bigk'}
  for d, k, n_img, seg, it, given, flags, want in KMEANS_ROUTES:
    case = (d, k, n_img, seg, it, given, flags)
    p = n_img * seg
    assert _ffi.kmeans_path_name(p, d, k, n_img, seg, it, given, flags) == want, case
    before = _ffi.set_deterministic(False)
    try:
      plain = lib.spml_kmeans_workspace_bytes(p, d, k, n_img, seg)
      _ffi.set_deterministic(True)
      det = lib.spml_kmeans_workspace_bytes(p, d, k, n_img, seg)
    finally:
      _ffi.set_deterministic(before)
    # (the int32 labels, the fp32 prototypes and sums, the fixed-point image of the sums)
    assert plain == det >= p * 4 + n_img * k * d * 16, case
    if given or flags:
      continue
    n_pass, wgs = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.spml_kmeans_profile_layout(p, d, k, n_img, seg, it, ctypes.byref(n_pass), ctypes.byref(wgs))
    if want in ('generic', 'mfma_f16x2_bigk'):
      assert rc == -2, case                                   # SPML_ERR_UNSUPPORTED
      continue
    assert rc == 0, case
    assert n_pass.value == (2 * it if want == 'mfma_f16x2_v4k' else it + 1), case
    assert wgs.value % n_img == 0 and 1 <= wgs.value // n_img <= (seg + 31) // 32, case


def _header_names(first_words, declaration):
  """The quoted names in the header comment that documents `declaration`."""
  hdr = open(os.path.join(ROOT, 'include', 'spml_hip.h')).read()
  doc = hdr[hdr.index(first_words):hdr.index(declaration)]
  return set(re.findall(r'"([a-z0-9_+]+)"', doc))


CONV_SWITCHES = ('SPML_CONV_RB', 'SPML_CONV_RG', 'SPML_CONV_NARROW_RB', 'SPML_CONV_CHUNK_MIN_K', 'SPML_WGRAD_STAGES')


def _switches(monkeypatch, env):
  for name in CONV_SWITCHES:
    monkeypatch.delenv(name, raising=False)
  for name, value in env.items():
    monkeypatch.setenv(name, value)


def test_conv_route_table(lib_path, monkeypatch):
  """The host side of a convolution call decides its conv_gemm / conv_wgrad instantiation once (csrc/conv.hip:
  conv_route, wgrad_route); the five entry points, the statistics layouts, the workspace sizes and the path names read
  the same record.  Every GPU case of tests/test_conv_gpu.py and tests/test_conv_bn_bwd_stats_gpu.py reaches the
  instantiation it names under the switches it sets; every name the header lists is reached by at least one of them; the
  recipe-sized shapes take the production tiles; the layout rules; extremes of the arguments."""
  import ctypes
  from spml_amd import _ffi
  import test_conv_gpu as tc
  import test_conv_bn_bwd_stats_gpu as tb
  lib = _ffi.lib()
  assert tuple(tc.SWITCHES) == CONV_SWITCHES
  reached, wreached = set(), set()
  was = _ffi.set_deterministic(False)
  try:
    for route, env, label, n, h, w, cin, cout, k, dil in tc.GEMM_CASES + tc.CHUNK_CASES:
      _switches(monkeypatch, env)
      for addend in (False, True):
        assert _ffi.conv_hl8_path_name('plain', n, h, w, cin, cout, k * k, addend) == route, (route, label)
      reached.add(route)
      # the shape kinds are what their comments say for the route's tile rows
      t = dict(tc.GEMM_ROUTES, **tc.CHUNK_ROUTES)[route][1]
      rows = n * h * w
      if label == 'a':
        assert rows < t and rows % 16
      elif label == 'b':
        assert rows == t
      elif label == 'c':
        assert t < rows < t + 16 and w == 1
      elif label in ('d1', 'd2'):
        assert n == 3 and h * w < t and t % (h * w)
      elif label in ('e', '3x3e'):
        assert n == 1 and rows >= 2 * t and t % w == 0 and dil > t // w and dil < h
      elif label == 'f':
        assert dil >= h and dil >= w
      elif label == 'g':
        assert h == 1 and k == 3
      elif label.startswith('tiles'):
        assert -(-rows // t) * (cout // 256) == int(label[5:])
    assert {c[2] for c in tc.GEMM_CASES if c[0] == 'rb5_rg2'} >= {'a', 'b', 'c', 'd1', 'd2', 'e', 'f', 'g', 'k16x1', 'k32x1', 'k48x1', 'k16x3'}
    assert sorted(int(c[2][5:]) % 8 for c in tc.GEMM_CASES if c[2].startswith('tiles')) == [0, 0, 6, 6]
    # stages of the chunked cases: K * taps / 16 on either side of the fold
    assert {c[6] * c[8] * c[8] // 16 for c in tc.CHUNK_CASES} == {64, 65, 129, 72}
    n, h, w, cin, k, dil = tc.AFFINE_SHAPE
    for route, env, cout in tc.AFFINE_CASES:
      _switches(monkeypatch, env)
      assert _ffi.conv_hl8_path_name('affine', n, h, w, cin, cout, k * k) == route
      reached.add(route)
    _switches(monkeypatch, {'SPML_CONV_RG': '2'})              # the inference entry has no two-row-group rung
    assert _ffi.conv_hl8_path_name('affine', n, h, w, cin, 256, k * k) == 'rb3'
    assert _ffi.conv_hl8_path_name('plain', n, h, w, cin, 256, k * k) == 'rb5_rg2'
    assert _ffi.conv_hl8_path_name('pyramid', n, h, w, cin, 256, 2) == 'rb5_rg2'
    assert _ffi.conv_hl8_path_name('plain', n, h, w, 512, 256, 9) == 'rb3_chunk'      # (chunking comes first)
    n, h, w, cin = tc.PYR_SHAPE
    for route, env, det, addend, cout, dils in tc.PYR_CASES:
      _switches(monkeypatch, env)
      _ffi.set_deterministic(det)
      assert _ffi.conv_hl8_path_name('pyramid', n, h, w, cin, cout, len(dils), addend) == route, (route, det, addend)
      assert ('+tapgroups' in route) == (cout % 256 != 0 and len(dils) > 1 and not addend and not det)
      reached.add(route)
    _ffi.set_deterministic(False)
    for route, env, n, h, w in tc.STATS_CASES:
      _switches(monkeypatch, env)
      assert _ffi.conv_hl8_path_name('stats', n, h, w, 64, 256, 1) == route
      reached.add(route)
    for (taps, dil, k, cout), (n, h, w), env in tb.CASES:
      _switches(monkeypatch, env)
      want = ('rb3_chunk' if 'SPML_CONV_CHUNK_MIN_K' in env else 'rb' + env.get('SPML_CONV_RB', '3')) + '+bstats'
      assert _ffi.conv_hl8_path_name('bwd_stats', n, h, w, k, cout, taps) == want, (taps, k, cout, n, h, w, env)
      reached.add(want)
    assert {(1, 97, 1), (1, 3, 5), (1, 161, 1)} <= {g for _, g, _ in tb.CASES}
    for route, env, label, n, h, w, cin, cout, k, dil in tc.WGRAD_CASES + tc.WGRAD_SPLIT_CASES:
      _switches(monkeypatch, env)
      assert _ffi.conv_wgrad_path_name(n, h, w, cin, cout, k * k) == route, (route, label)
      wreached.add(route)
    # one tile: splits = ceil(R / 256); stages per split under the pair kernel: 1, 1, 2, 3 and (10, 9)
    _switches(monkeypatch, {})
    assert [_ffi.conv_wgrad_splits(c[3], c[4], c[5], 256, 256, 1) for c in tc.WGRAD_SPLIT_CASES[:len(tc.WGRAD_SPLITS)]] == tc.WGRAD_SPLITS
    assert {1, 2, 3, 4, 7, 8, 9, 12, 15, 16} <= set(tc.WGRAD_SPLITS)
    assert _ffi.conv_wgrad_splits(1, 296, 1, 256, 256, 1) == 2 and _ffi.conv_wgrad_splits(1, 40, 1, 256, 256, 1) == 1
    for cin, dils in tc.PYR_WGRAD_CASES:
      assert _ffi.conv_wgrad_path_name(2, 9, 11, cin, 64, len(dils), True) == 'pyr_t256x256_pair4'
      wreached.add('pyr_t256x256_pair4')
    assert sorted({(9 * len(d)) % 4 for _, d in tc.PYR_WGRAD_CASES}) == [0, 1, 2, 3]      # padding taps of the last group

    names = _header_names('Which conv_gemm instantiation', 'const char* spml_conv_hl8_path_name')
    wnames = _header_names('The same for the weight gradient', 'const char* spml_conv_wgrad_path_name')
    assert len(names) == 26 and len(wnames) == 10
    assert reached == names - {'unsupported'}, (sorted(names - reached), sorted(reached - names))
    assert wreached == wnames - {'unsupported'}, (sorted(wnames - wreached), sorted(wreached - wnames))

    # what the recipe-sized shapes take (batch 16, 65 x 65 maps)
    _switches(monkeypatch, {})
    assert _ffi.conv_hl8_path_name('stats', 16, 65, 65, 256, 256, 9) == 'rb5+stats'       # 3x3 dilation 2, 256 -> 256
    assert _ffi.conv_hl8_path_name('plain', 16, 65, 65, 256, 256, 9) == 'rb5'
    assert _ffi.conv_hl8_path_name('stats', 16, 65, 65, 1024, 256, 1) == 'rb5+stats'      # 1x1 1024 -> 256
    assert _ffi.conv_hl8_path_name('plain', 16, 65, 65, 2048, 512, 1, True) == 'rb5'      # data gradient of 512 -> 2048
    assert _ffi.conv_hl8_path_name('bwd_stats', 16, 65, 65, 2048, 512, 1) == 'rb5+bstats'
    assert _ffi.conv_hl8_path_name('pyramid', 16, 65, 65, 256, 64, 4) == 'n64_chunk+tapgroups'
    assert _ffi.conv_hl8_path_name('pyramid', 16, 65, 65, 256, 64, 4, True) == 'n64_chunk'
    assert _ffi.conv_hl8_path_name('plain', 16, 65, 65, 512, 512, 9) == 'rb3_chunk'       # 3x3 of res5: K * taps = 4608
    assert _ffi.conv_wgrad_path_name(16, 65, 65, 256, 256, 9) == 't256x256_pair4'
    assert _ffi.conv_wgrad_path_name(16, 65, 65, 2048, 64, 4, True) == 'pyr_t256x256_pair4'
    # by problem size: tiles5 = ceil(R / 160) * (N / 256) against 192 and 384
    assert [_ffi.conv_hl8_path_name('plain', 1, 160 * t, 1, 64, 256, 1) for t in (191, 192, 383, 384)] == ['rb3', 'rb4', 'rb4', 'rb5']
    # the chunk threshold
    assert [_ffi.conv_hl8_path_name('plain', 1, 9, 9, kk, 256, t) for kk, t in ((448, 9), (464, 9), (4080, 1), (4096, 1))] == \
        ['rb3', 'rb3_chunk', 'rb3', 'rb3_chunk']

    # statistics layout: no rows under two row groups and for narrow N; at most 4096 row tiles (host only)
    chunks, rows = ctypes.c_int(0), ctypes.c_int(0)
    layout = lambda *a: lib.spml_conv_hl8_stats_layout(*(a + (ctypes.byref(chunks), ctypes.byref(rows))))
    assert layout(16, 160, 256, 64, 256, 1) == 0 and (chunks.value, rows.value) == (4096, 160)
    assert layout(16, 203, 203, 64, 256, 1) == -2 and _ffi.conv_hl8_path_name('stats', 16, 203, 203, 64, 256, 1) == 'unsupported'
    assert _ffi.conv_hl8_path_name('plain', 16, 203, 203, 64, 256, 1) == 'rb5'
    assert lib.spml_conv_hl8_bwd_stats_layout(16, 203, 203, 64, 256, 1, ctypes.byref(chunks), ctypes.byref(rows)) == -2
    for cout in (64, 128, 192):
      assert layout(2, 17, 19, 64, cout, 1) == -2
      assert _ffi.conv_hl8_path_name('stats', 2, 17, 19, 64, cout, 1) == 'unsupported'
    assert layout(2, 17, 19, 64, 256, 1) == 0 and (chunks.value, rows.value) == (7, 96)
    _switches(monkeypatch, {'SPML_CONV_RG': '2'})
    assert layout(2, 17, 19, 64, 256, 1) == -2 and layout(2, 17, 19, 512, 256, 9) == -2
    assert _ffi.conv_hl8_path_name('bwd_stats', 2, 17, 19, 64, 256, 1) == 'unsupported'
    _switches(monkeypatch, {})

    # outside the domain
    for args in [('plain', 1, 9, 9, 40, 256, 1), ('plain', 1, 9, 9, 64, 96, 9), ('plain', 1, 9, 9, 64, 256, 4),
                 ('plain', 0, 9, 9, 64, 256, 1), ('pyramid', 1, 9, 9, 64, 64, 5), ('pyramid', 1, 9, 9, 64, 64, 0)]:
      assert _ffi.conv_hl8_path_name(*args) == 'unsupported', args
    assert lib.spml_conv_hl8_path_name(7, 1, 9, 9, 64, 256, 1, 0) == b'unsupported'
    assert _ffi.conv_wgrad_path_name(1, 9, 9, 64, 256, 1) == 'unsupported' and _ffi.conv_wgrad_splits(1, 9, 9, 64, 256, 1) == 0
    assert _ffi.conv_wgrad_path_name(1, 9, 9, 256, 128, 4, True) == 'unsupported'
    assert lib.spml_conv_wgrad_workspace_bytes(1, 9, 9, 64, 256, 1) == 0

    # extremes: n_img * H * W around 2^31, tiles > 256 in the split count: names and counts well defined, and the
    # workspace is splits * tiles * tile n * tile k floats
    tile = lambda c: 256 if c % 256 == 0 else 128
    for n, h, w in [(1, 46341, 46341), (2, 32768, 32768), (32768, 256, 256), (2, 32768, 32767), (16, 65, 65), (1, 1, 1)]:
      for cin, cout in [(64, 256), (128, 128), (256, 64), (4096, 512), (2048, 2048)]:
        for taps in (1, 9):
          for entry in ('plain', 'stats', 'bwd_stats', 'affine'):
            assert _ffi.conv_hl8_path_name(entry, n, h, w, cin, cout, taps) in names, (entry, n, h, w, cin, cout, taps)
          if cin % 128 or cout % 128:
            continue
          assert _ffi.conv_wgrad_path_name(n, h, w, cin, cout, taps) in wnames - {'unsupported'}
          splits = _ffi.conv_wgrad_splits(n, h, w, cin, cout, taps)
          tiles = (cout // tile(cout)) * (cin // tile(cin)) * taps
          assert 1 <= splits <= max(1, min(256 // tiles if tiles <= 256 else 16, -(-n * h * w // 256))), (n, h, w, cin, cout, taps)
          assert lib.spml_conv_wgrad_workspace_bytes(n, h, w, cin, cout, taps) == splits * tiles * tile(cout) * tile(cin) * 4
      for branches in (1, 2, 3, 4):
        for cin in (256, 2048):
          assert _ffi.conv_hl8_path_name('pyramid', n, h, w, cin, 64, branches) in names
          splits = _ffi.conv_wgrad_splits(n, h, w, cin, 64, branches, True)
          tiles = (9 * branches + 3) // 4 * (cin // 256)
          assert 1 <= splits <= 16
          assert lib.spml_conv_wgrad_pyramid_workspace_bytes(n, h, w, cin, 64, branches) == splits * tiles * 256 * 256 * 4
    # 288 tiles: 7 splits fill 2016 of 2048 places (1.6 % idle); 8 would fill 9 rounds exactly but gains under 2 %
    assert _ffi.conv_wgrad_splits(16, 65, 65, 4096, 512, 9) == 7
  finally:
    _ffi.set_deterministic(was)
