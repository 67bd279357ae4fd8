"""The splitting arithmetic of the sparse adjoint plan (csrc/adjoint_plan.h: run ranges, fills, piece length, equal cuts, list order,
workgroup remap) on the CPU: tests/csrc/adjoint_plan_check.cpp compiles the header the device kernels use and checks, on random
supports in small ragged volumes, that what a step marches covers the gradient's reach, that what the next step reads was written,
that nothing is written twice and that step 0 writes everything.  Built with the address and undefined-behaviour sanitizers where
the compiler has them: the program is stand-alone, nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest


def test_plan_arithmetic_on_random_supports(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    src = os.path.join(os.path.dirname(__file__), 'csrc', 'adjoint_plan_check.cpp')
    exe = str(tmp_path / 'adjoint_plan_check')
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if subprocess.run([cxx, *flags, '-o', exe, src], capture_output=True).returncode != 0:   # (no sanitizer runtime installed)
        subprocess.run([cxx, '-O1', '-std=c++17', '-o', exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'violations 0' in out.stdout
