"""Planning of the chained top-down launch (csrc/pml_schedule.h: PmlSuperSchedule::chain_depth, PmlSweepTraits::td_chain), on the host.

tests/td_chain_plan_driver.cpp is compiled together with pml_schedule.cpp -- plain C++, no HIP runtime, no GPU, the library is not
loaded.  pml_plan_tree must find the chain on balanced forests of 13, 15 and 17 levels (the depth right above the two-level
nodes' parents, with the conditions restated on the lists the kernel walks) and none on random binary forests, on a forest of
two balanced trees of different heights and on a balanced tree less one tip pair.  pml_plan_top_down with td_chain must write every stored
node's row in exactly one record and read no row before the record that writes it, and its plan must be the unchained plan less the
stacked record of the chained depth, with the depth in the closing record's arg; without a chain, or with td_chain off, the
plans are the unchained ones: one stacked record per stacked depth and the two-level record last with arg 0."""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_td_chain_plans(tmp_path):
    exe = str(tmp_path / 'td_chain_plan_driver')
    sources = [os.path.join(HERE, 'td_chain_plan_driver.cpp'), os.path.join(build.CSRC, 'pml_schedule.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
