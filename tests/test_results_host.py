"""What a context's result buffers hold (csrc/pml_results.h), checked on the host.

tests/results_driver.cpp holds the record next to a restatement of the loose fields of pml_ctx it replaced, with one function per
place the commit before it wrote them, and plays every sequence of four entries of the library to both -- the options, tunables,
masks, models and the window, the sweeps with their boolean arguments enumerated, a sweep that could not be enqueued, a marginal
pass enqueued, captured and replayed, a pass that meets a zero likelihood, the selection, every lazy materialisation -- on each
of sixteen kinds of context (F81 or not, cherries, two-level units, a sweep that builds the batch of P(t)).  After every step
every query of the record answers what the old fields answer, "has a top-down result" implies "posteriors exist" and "has joint
states" implies "joint states exist".  The driver prints the number of sequences.  (A sanitizer build of the same driver is for
running by hand: add -fsanitize=address,undefined to FLAGS.)"""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O2', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_results(tmp_path):
    exe = str(tmp_path / 'results_driver')
    sources = [os.path.join(HERE, 'results_driver.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
