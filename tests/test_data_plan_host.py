"""The splitting arithmetic of the sparse data stage (csrc/adjoint_plan.h with the tile and the reach passed in: run ranges, pieces, the
data term's fills, the warp's hull, the grid bound of the list-walking kernels) on the CPU: tests/csrc/data_plan_check.cpp compiles the
header the device kernels use and checks, on random masks in small ragged volumes, that every voxel within reach of the mask is in
exactly one run piece, that every other voxel of the data term's output is in exactly one fill, and that nothing leaves the volume.
Built with the address and undefined-behaviour sanitizers where the compiler has them: the program is stand-alone, nothing of it is
loaded into Python."""
import os
import shutil
import subprocess

import pytest


def test_data_plan_arithmetic_on_random_masks(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    src = os.path.join(os.path.dirname(__file__), 'csrc', 'data_plan_check.cpp')
    exe = str(tmp_path / 'data_plan_check')
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if subprocess.run([cxx, *flags, '-o', exe, src], capture_output=True).returncode != 0:   # (no sanitizer runtime installed)
        subprocess.run([cxx, '-O1', '-std=c++17', '-o', exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'violations 0' in out.stdout
