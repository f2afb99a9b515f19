"""When may a top-down sweep leave the observed tips' posterior rows alone (csrc/pml_results.h, tip_rows_kept), checked on the host.

tests/tip_rows_driver.cpp plays the entries of the library that touch the fact to the record the way pml_api.hip plays them -- the
allocation, the three writers of the masks, a change of the parameters, of the model kind, of an option, of a tunable (the off
switch or another), a bottom-up sweep, a top-down sweep and the lazy sweep of the TD vectors with their bad-tip word clear or
raised, a marginal pass enqueued, captured and replayed, with or without an error -- and keeps a log next to it.  After every step
of every sequence of five entries, from each of eight kinds of context (F81 kernels of one mask word or not, rows left implicit or
not, the off switch), the record answers what the log says: kept <=> since the last clearing event a qualifying sweep was waited
for with a clear bad-tip word.  A sweep enqueued in skip mode implies that the fact held when it was enqueued; the rows being left
out of memory implies that they are not counted as kept.  The driver prints the number of sequences and of sweeps in skip mode.
(A sanitizer build of the same driver is for running by hand: add -fsanitize=address,undefined to FLAGS.)"""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O2', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_tip_rows(tmp_path):
    exe = str(tmp_path / 'tip_rows_driver')
    sources = [os.path.join(HERE, 'tip_rows_driver.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
