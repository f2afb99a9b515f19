"""Planning of the chained bottom-up launch (csrc/pml_schedule.h: PmlSuperSchedule::bu_chain_level, PmlSweepTraits::bu_chain), on the host.

tests/bu_chain_plan_driver.cpp is compiled together with pml_schedule.cpp -- plain C++, no HIP runtime, no GPU, the library is not
loaded.  pml_plan_tree must find the chain on balanced forests of 13, 15 and 17 levels (the lowest level with stacked units, with
the conditions restated on the lists the kernel walks) and none on random binary forests, on a forest of two balanced trees of
different heights and on a balanced tree less one tip pair.  pml_plan_bottom_up with bu_chain must write every stored node's vector in
exactly one record and read none before the record that writes it, the chained stacked units must read two-level nodes only, and
the plan must be the unchained plan less the stacked record of the chained level, with the level in the opening two-level record's
arg; without a chain, with bu_chain off, or for the joint sweep, the plans are the unchained ones."""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_bu_chain_plans(tmp_path):
    exe = str(tmp_path / 'bu_chain_plan_driver')
    sources = [os.path.join(HERE, 'bu_chain_plan_driver.cpp'), os.path.join(build.CSRC, 'pml_schedule.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
