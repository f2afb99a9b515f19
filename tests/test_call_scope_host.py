"""The scope of one call's scratch and events (csrc/pml_call_scope.h), checked on the host.

tests/call_scope_driver.cpp supplies counting stand-ins for the HIP calls the header uses -- plain C++, no HIP runtime, no GPU,
the library is not loaded -- and checks: with the allocation of each of six requests failing in turn, every pointer handed out
is freed exactly once, after the stream has been waited for, and the error names the bytes asked for; a request of 0 elements
gets a pointer of its own; no event exists unless events are on, and with them on every mark is created, recorded on the
scope's stream and destroyed after the frees, a failing hipEventCreate / hipEventRecord included; finish() followed by the end
of the scope waits once, finish() / put() / end twice, a failing wait is reported and the memory still freed; outputs tied to
their host destination (CallScope::out) are copied by finish() in the order and with the byte counts of their requests, all
before the one wait, a zeroed one cleared where it is asked for, nothing allocated or copied for a null destination, nothing
copied twice (a second finish(), a launcher that waits per chunk), nothing copied on an early exit, a failing copy, fill or
allocation reported with everything still freed once behind a wait, no copy or fill outside its allocation; the columns of
a chunk against a table worked out by hand from the two expressions the rule replaced (memory to spare, either cap binding,
the tunable below and above the memory's bound, 0 and negative, nothing per column, a column that does not fit, one column);
pow2_from; the altered flags in the library's numbering.  (A sanitizer build of the same driver is for running by hand: add
-fsanitize=address,undefined to FLAGS.  The stand-ins keep "device" memory on the host, so a copy past its allocation, a
double free or a leaked event is a finding of that build.)"""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_call_scope(tmp_path):
    exe = str(tmp_path / 'call_scope_driver')
    sources = [os.path.join(HERE, 'call_scope_driver.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
