"""The windowed sweep plans (csrc/pml_pij_window.h: pml_plan_pij_window), checked on the host.

tests/pij_window_plan_driver.cpp is compiled together with pml_schedule.cpp and pml_pij_window.cpp -- plain C++, no HIP
runtime, no GPU, the library is not loaded -- and cuts the plans of the sweeps that read P(t) (plain level launches, bottom-up
and top-down) of a balanced binary tree, a caterpillar, a star of 40, a ragged tree with polytomies and a two-tree forest with
a single-tip tree, for windows of the largest fan-out, of three more and of at least the whole forest.  Every non-root branch
must be built exactly once per sweep, in the run that reads it; slots inside a run are distinct and below B; no parent is
split; runs keep the level order; the concatenated sweep records cover the plan's records exactly; the signal record is last;
a window below the fan-out is refused.  (A sanitizer build of the same driver is for running by hand, as a stand-alone
program: add -fsanitize=address,undefined to FLAGS.)"""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_pij_window_plans(tmp_path):
    exe = str(tmp_path / 'pij_window_plan_driver')
    sources = [os.path.join(HERE, 'pij_window_plan_driver.cpp'), os.path.join(build.CSRC, 'pml_schedule.cpp'),
               os.path.join(build.CSRC, 'pml_pij_window.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
