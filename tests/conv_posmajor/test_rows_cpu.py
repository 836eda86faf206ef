"""The image-strided row tiles of the implicit-GEMM convolution kernels (LOANS_TILE_POSMAJOR; loans_amd/csrc/conv_rows.h:
row_prologue_images, images_tile, block_taps, TapWalk) on the CPU.  posmajor_cpu.cpp -- a stand-alone program built here with
AddressSanitizer and UndefinedBehaviorSanitizer -- checks the prologue against a brute-force loop over the ordinary GEMM rows
(rowoff, opix, badmask, existence), that the tiles of a launch cover every existing row exactly once, the block's tap set
against the AND of its rows' masks (an empty one keeps tap 0) and the compacted K walk (tap, chunk in the tap, weight offset)
against the full walk with the left-out taps filtered away: grids 1 x 1 to 9 x 9, B from 1 to 2 BM + 1, the 3 x 3, 4 x 4 / 2,
3 x 3 / 2, 1 x 1 forward tap grids and the reversed ones of their data gradients.  tests/conv_posmajor/test_gpu_kernels.py
checks what the kernel makes of it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def test_image_strided_rows_as_plain_cpp(tmp_path):
    exe = tmp_path / 'posmajor_cpu'
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'loans_amd', 'csrc'),
                           os.path.join(HERE, 'posmajor_cpu.cpp'), '-o', str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1].startswith('ok:') and len(lines) == 10, run.stdout
