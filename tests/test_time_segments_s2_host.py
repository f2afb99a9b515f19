"""The upper ends of the segments of a dated forest (csrc/pml_time_segments.h: pml_time_segment_ends), which
pml_sample_histories_through_time places its events with, checked on the host.

tests/time_segments_s2_driver.cpp is compiled together with pml_time_segments.cpp -- plain C++, no HIP runtime, no GPU, the
library is not loaded -- and takes the plans of the forests of time_segments_driver.cpp (several roots at staggered times,
branches without extent) against the same kinds of boundaries.  It checks that s2 of a segment equals, bit for bit, the s1 of the
same branch's segment in the next bin -- and the quotient (T_{m+1} - time_p) / h itself --, for a branch that leaves the range the
s1 of its point segment at T_M; that s2 is 1, with the end included, where the branch ends in the bin (r == 0), for every branch
without extent and for the point segments; that this holds for branches that start before the range and for a boundary on a
node; that the segments of a branch so tile it without gap or overlap, in bits; and that the plan itself is left as it was."""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS', '-I', build.CSRC]


def test_time_segment_ends(tmp_path):
    exe = str(tmp_path / 'time_segments_s2_driver')
    sources = [os.path.join(HERE, 'time_segments_s2_driver.cpp'), os.path.join(build.CSRC, 'pml_time_segments.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
    cases, segments, chained = (int(x) for x in ran.stdout.split()[1:4])
    assert cases >= 20 and segments > 5000 and chained > 1000, ran.stdout
