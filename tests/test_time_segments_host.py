"""The segment plan of pml_history_through_time (csrc/pml_time_segments.h: pml_plan_time_segments, pml_cut_time_pieces), checked
on the host.

tests/time_segments_driver.cpp is compiled together with pml_time_segments.cpp -- plain C++, no HIP runtime, no GPU, the library
is not loaded -- and plans forests with roots at different times and zero-extent branches against: bins that line up with no
node, a boundary exactly on a node time, boundaries before the first root and after the last tip (empty bins), boundaries that
cover part of the tree only, one bin, 200 bins inside one branch, a sliver of 1e-12 of a branch at either end, a zero-extent
branch on the last boundary, and random boundaries.

It checks that the segments of each branch tile its covered part (s1 + w + r = 1 to 2 ulp, the next s1 is the last s1 + w, the
first and the last end where the bins do), that the bins are in order with the ids ascending inside each, that which (bin, node)
pairs hold a segment, the flags and the point segments of the last boundary equal a brute-force count (bins outside, nodes
inside), that the pieces never straddle two bins, and that every refusal gives its reason -- with the node or the index in it --
and leaves no plan.  (A sanitizer build of the same driver is for running by hand: add -fsanitize=address,undefined to FLAGS.)"""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS', '-I', build.CSRC]


def test_time_segment_plans(tmp_path):
    exe = str(tmp_path / 'time_segments_driver')
    sources = [os.path.join(HERE, 'time_segments_driver.cpp'), os.path.join(build.CSRC, 'pml_time_segments.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
