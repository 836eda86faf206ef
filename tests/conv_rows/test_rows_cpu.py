"""The row arithmetic of the implicit-GEMM convolution kernels (loans_amd/csrc/conv_rows.h) on the CPU: the header compiles
as plain C++, and rows_cpu.cpp -- a stand-alone program built here with AddressSanitizer and UndefinedBehaviorSanitizer
(a shift by 64 in the closed-form mask is undefined behaviour: the sanitizer, not luck, rules it out) -- checks the tap mask
against a brute-force one, the tap-grid detector, the row walk against integer division and the block remaps as
bijections.  This test owns that arithmetic; tests/conv_rows/test_gpu_kernels.py checks what the kernels pass into it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def test_conv_rows_header_as_plain_cpp(tmp_path):
    exe = tmp_path / 'rows_cpu'
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover', '-Wall', '-Werror',
                           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'loans_amd', 'csrc'),
                           os.path.join(HERE, 'rows_cpu.cpp'), '-o', str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.splitlines()
    assert lines[-1].startswith('ok:') and len(lines) == 6, run.stdout
