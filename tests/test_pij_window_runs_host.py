"""The runs in which the entries that read P(t) outside the sweeps find it in the window (csrc/pml_pij_window.h:
pml_window_piece_runs, pml_plan_sim_window and the top-down PmlWindowPlan), checked on the host.

tests/pij_window_runs_driver.cpp is compiled together with pml_schedule.cpp and pml_pij_window.cpp -- plain C++, no HIP runtime,
no GPU, the library is not loaded -- and cuts the ids of the exact counts into runs of whole pieces, the levels and frontier
subtrees of the simulator and the scenario sampler into runs and groups, and the parents of the sampled counts into the
top-down sweep's runs, on a balanced tree, a 300-deep caterpillar, a star of 40 and a ragged forest with a single-tip tree, for
windows of the largest fan-out, of 200 and of all nodes.  Every non-root branch a consumer reads must be built exactly once per
call, in the run that reads it; slots within a run are distinct and below B; the piece runs are whole pieces, in order,
covering all ids; no frontier subtree is split; a subtree larger than B moves the frontier, never overflows; the launch count
is bounded by levels + ceil(N / B) + the frontier's groups.  (A sanitizer build of the same driver is for running by hand, as a
stand-alone program: add -fsanitize=address,undefined to FLAGS.)"""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_pij_window_consumer_runs(tmp_path):
    exe = str(tmp_path / 'pij_window_runs_driver')
    sources = [os.path.join(HERE, 'pij_window_runs_driver.cpp'), os.path.join(build.CSRC, 'pml_schedule.cpp'),
               os.path.join(build.CSRC, 'pml_pij_window.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
