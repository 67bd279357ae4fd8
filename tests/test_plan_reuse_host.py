"""Plan reuse on the CPU (csrc/adjoint_plan.h: plan_key, plan_reusable, plan_record, plan_extent_entry next to the splitting arithmetic):
tests/csrc/plan_reuse_check.cpp compiles the header the device kernels use and runs a model of their sequence -- extent pass with
compare-and-store, runs stage, lists stage, one record per list -- on random masks in small ragged volumes with random widths, flags,
piece lengths and resident sets.  It checks that a zeroed record is invalid; that a change of any single key field, dense flag or table
entry makes the predicate say "rebuild"; that whenever it says "reuse" the list rebuilt from scratch equals the kept one entry for
entry; and that the adjoint's run ranges cut from the mask's table contain those cut from any gradient inside mask (+) 2 S.  Built with
the address and undefined-behaviour sanitizers where the compiler has them: the program is stand-alone, nothing of it is loaded into
Python."""
import os
import shutil
import subprocess

import pytest


def test_plan_reuse_predicate_and_lists_on_random_masks(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    src = os.path.join(os.path.dirname(__file__), 'csrc', 'plan_reuse_check.cpp')
    exe = str(tmp_path / 'plan_reuse_check')
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if subprocess.run([cxx, *flags, '-o', exe, src], capture_output=True).returncode != 0:   # (no sanitizer runtime installed)
        subprocess.run([cxx, '-O1', '-std=c++17', '-o', exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'violations 0' in out.stdout
