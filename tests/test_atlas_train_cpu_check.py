"""K18 executed FROM ITS SOURCE on the CPU under AddressSanitizer and UBSan (tools/cpu_check/check_atlas_loss.cpp, a
stand-alone program): the batch gather against integer / double loops and the fused losses against double-precision loops,
every entry of the four gradient tensors against central differences of the double-precision total; N = 0 / 1 / 63 / 64 / 65
/ 255 / 256 / 257 / 513, with and without the blocks 5 and 6, with and without the alpha loss, no / one / all rows relevant,
pixels at the four image corners on frame 0 and on frame T - 1, an index outside the video (nothing may be read), and the
refusals.  Every buffer has exactly the stated size, so a read or write past a data array, a row block or a gradient
tensor ends the program."""
import os
import shutil
import subprocess

import pytest

from util import ROOT

CXX = os.environ.get('CXX_HOST', '/opt/rocm/lib/llvm/bin/clang++')


@pytest.mark.skipif(not (os.path.isfile(CXX) or shutil.which('clang++')), reason='needs clang++ (C++20)')
def test_atlas_loss_kernels_run_from_source_under_the_sanitizers(tmp_path):
    cxx = CXX if os.path.isfile(CXX) else shutil.which('clang++')
    src = os.path.join(ROOT, 'tools', 'cpu_check')
    exe = str(tmp_path / 'check_atlas_loss')
    cmd = [cxx, '-std=c++20', '-O1', '-g', '-pthread', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', src,
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'videoswap_amd', 'csrc'), '-Wno-unused-function', '-o', exe,
           os.path.join(src, 'check_atlas_loss.cpp')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and 'all checks passed' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'FAIL' not in r.stdout and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
    # the gather: nine N x two block counts, the 768-wide case, the hostile indices; the losses: nine N x four flag settings,
    # three N x three relevance counts; the refusals
    assert r.stdout.count(' ok') == 9 * 2 + 2 + 9 * 4 + 3 * 3 + 1
