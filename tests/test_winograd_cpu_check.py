"""csrc/winograd.hip executed FROM ITS SOURCE on the CPU under AddressSanitizer and UBSan (tools/cpu_check/check_winograd.cpp, a
stand-alone program): the input transform, the output transform with every epilogue combination, and the entry point
against double-precision loops at nimg 1 / 3 x 2x2 / 4x6 / 8x8 x C = 8 / 72 / 64 + 64 x Cout = 8 / 40, a row vector shared
by two images, rows_per_vec = W / 3 / 1, ldc > N with ldr != ldc (pad columns that must keep their sentinel), sources of 64 + 128 and
128 + 64 channels, and the refusals (odd H or W among them).  Every buffer has exactly its stated size, the workspace exactly
vsx_conv3x3_winograd_workspace bytes.  The GEMM stage is the program's own element-wise execution of the batched description
the entry point builds; `make -C tools/cpu_check check_winograd_gemm` puts the real vsx_gemm_f16 there (minutes)."""
import os
import shutil
import subprocess

import pytest

from util import ROOT

CXX = os.environ.get('CXX_HOST', '/opt/rocm/lib/llvm/bin/clang++')


@pytest.mark.skipif(not (os.path.isfile(CXX) or shutil.which('clang++')), reason='needs clang++ (C++20)')
def test_winograd_kernels_run_from_source_under_the_sanitizers(tmp_path):
    cxx = CXX if os.path.isfile(CXX) else shutil.which('clang++')
    src = os.path.join(ROOT, 'tools', 'cpu_check')
    exe = str(tmp_path / 'check_winograd')
    cmd = [cxx, '-std=c++20', '-O1', '-g', '-pthread', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', src,
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'videoswap_amd', 'csrc'), '-Wno-unused-function',
           '-Wno-unused-value', '-o', exe, os.path.join(src, 'check_winograd.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and 'all checks passed' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'FAIL' not in r.stdout and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
    # 2 nimg x 3 sizes x (3 channel sets + 2 Cout x 8 epilogues) + 36 geometries + 8 epilogues of the entry point + refusals
    # + the edges of the GPU parity table: 3 rows_per_vec and 3 (ldc, ldr) pairs x (output, entry), one tile per image x 2,
    #   2 source pairs x (input, entry)
    assert r.stdout.count(' ok') == 2 * 3 * (3 + 16) + 36 + 8 + 1 + 3 * 2 + 3 * 2 + 2 + 2 * 2
    for edge in ('rpv 6 ', 'rpv 3 ', 'rpv 1 ', 'ldc N+8 ldr N+16', 'ldc N+16 ldr N+0', 'ldc N+0 ldr N+8', 'C=64+128', 'C=128+64'):
        assert edge in r.stdout, edge
