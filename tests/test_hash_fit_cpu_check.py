"""K17 executed FROM ITS SOURCE on the CPU under AddressSanitizer and UBSan (tools/cpu_check/check_hash_fit.cpp, a
stand-alone program; v_mfma_f32_32x32x2_f32 emulated with the hardware's lane layout, the float atomicAdd of the table
gradient as a compare-exchange): the hash instantiation of the training forward (csrc/atlas.hip), the dEnc step and the
grid backward (csrc/atlas_bwd.hip) against double-precision loops, N = 0 / 1 / 63 / 64 / 65 / 513, a dense-only and a
hashed grid, 20 levels (a second pass, E = 40), all rows in one cell, and the refusals.  Every buffer has exactly the size
the workspace query states, so a read or write of a row >= N, of a column >= E or past the table ends the program."""
import os
import shutil
import subprocess

import pytest

from util import ROOT

CXX = os.environ.get('CXX_HOST', '/opt/rocm/lib/llvm/bin/clang++')


@pytest.mark.skipif(not (os.path.isfile(CXX) or shutil.which('clang++')), reason='needs clang++ (C++20)')
def test_hash_fit_kernels_run_from_source_under_the_sanitizers(tmp_path):
    cxx = CXX if os.path.isfile(CXX) else shutil.which('clang++')
    src = os.path.join(ROOT, 'tools', 'cpu_check')
    exe = str(tmp_path / 'check_hash_fit')
    cmd = [cxx, '-std=c++20', '-O1', '-g', '-pthread', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', src,
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'videoswap_amd', 'csrc'), '-Wno-unused-function', '-o', exe,
           os.path.join(src, 'check_hash_fit.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and 'all checks passed' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'FAIL' not in r.stdout and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
    assert r.stdout.count(' ok') == 2 * 6 + 3 + 2 + 1          # two grids x six N, three 20-level cases, two one-cell cases, the refusals
