"""The regions and lists of the sparse forward squaring steps (csrc/adjoint_plan.h: plan_forward_reach and the splitting arithmetic with
the forward tile and one reach per list) on the CPU: tests/csrc/forward_plan_check.cpp compiles the header the device kernels use and
checks, on random masks in small ragged volumes with random widths, that every voxel of W_j = mask (+) (3 S + h_j + ... + h_{n-1}) is in
exactly one run piece of the list of the step that writes d_j, that W_{j+1} (+) h_j and the adjoint's sources stay inside W_j, that
the last list covers the warp's hull, and that no piece leaves the volume, its length or the grid.  Built with the address and
undefined-behaviour sanitizers where the compiler has them: the program is stand-alone, nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest


def test_forward_plan_regions_and_lists_on_random_masks(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    src = os.path.join(os.path.dirname(__file__), 'csrc', 'forward_plan_check.cpp')
    exe = str(tmp_path / 'forward_plan_check')
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if subprocess.run([cxx, *flags, '-o', exe, src], capture_output=True).returncode != 0:   # (no sanitizer runtime installed)
        subprocess.run([cxx, '-O1', '-std=c++17', '-o', exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'violations 0' in out.stdout
