"""The sweeps' launch plans (csrc/pml_schedule.h: pml_plan_bottom_up / _top_down / _backtrace), checked on the host.

tests/sweep_plan_driver.cpp is compiled together with pml_schedule.cpp -- plain C++, no HIP runtime, no GPU, the library is not
loaded -- and plans ten forests over a grid of PmlSweepTraits.  Every plan is checked for coverage (each stored node / parent
in exactly one launch), order (no launch reads a vector before the launch that writes it), the once-only launches (ln L, the
completion word) and the per-bracket launch counts the profile reported before the plans existed; over the whole input set
every op and every schedule branch of the three planners must be reached; the narrow ends, the level kinds, the choice of the
sorted lists, the staging hint and the completion word are checked against the rules restated in the driver; the outcome
the host keeps of every plan (pml_plan_outcome) must count the plan's signal records and name the cherry-fused joint branch
exactly for BU_FUSED_JOINT plans.  (A sanitizer
build of the same driver is for running by hand: add -fsanitize=address,undefined to FLAGS.  UBSan then reports misaligned
PmlUnit accesses inside the std::stable_sort of units_by_shape -- libstdc++'s temporary buffer ignores the 32-byte alignment --,
which are the tree planner's, not the launch plans'.)"""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_sweep_plans(tmp_path):
    exe = str(tmp_path / 'sweep_plan_driver')
    sources = [os.path.join(HERE, 'sweep_plan_driver.cpp'), os.path.join(build.CSRC, 'pml_schedule.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
