"""csrc/atlas_edit.hip (K15) executed FROM ITS SOURCE on the CPU under AddressSanitizer and UBSan
(tools/cpu_check/check_atlas_edit.cpp, a stand-alone program): N = 1 / 255 / 256 / 257 x R = 2 / 16 x C = 3 / 4 with masks,
every row in one cell, and the hostile rows (NaN, +-inf, +-1e30, -0.0, just outside each edge of a box, exactly R - 1)
against a double-precision loop.  Every buffer has exactly the size the entry point is told, so an index past a texture,
a mask or a row ends the program; a float that reaches an integer conversion out of range does too
(float-cast-overflow).  The hostile rows are checked here and not on the GPU."""
import os
import shutil
import subprocess

import pytest

from util import ROOT

CXX = os.environ.get('CXX_HOST', '/opt/rocm/lib/llvm/bin/clang++')


@pytest.mark.skipif(not (os.path.isfile(CXX) or shutil.which('clang++')), reason='needs clang++ (C++20, std::atomic_ref)')
def test_atlas_edit_kernel_runs_from_source_under_the_sanitizers(tmp_path):
    cxx = CXX if os.path.isfile(CXX) else shutil.which('clang++')
    src = os.path.join(ROOT, 'tools', 'cpu_check')
    exe = str(tmp_path / 'check_atlas_edit')
    cmd = [cxx, '-std=c++20', '-O1', '-g', '-pthread', '-fsanitize=address,undefined,float-cast-overflow',
           '-fno-sanitize-recover=all', '-I', src, '-I', os.path.join(ROOT, 'include'), '-I',
           os.path.join(ROOT, 'videoswap_amd', 'csrc'), '-Wno-unused-function', '-o', exe, os.path.join(src, 'check_atlas_edit.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and 'all checks passed' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'FAIL' not in r.stdout and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
    assert r.stdout.count(' ok') == 2 * 2 * 6 + 4                              # R x C x (four N, one cell, hostile) + mixed C, R = 4, refusals
    assert r.stdout.count('hostile rows 28') == 4
