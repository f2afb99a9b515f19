"""Builds libpastml_hip.so in-tree with hipcc for gfx950 (no JIT cache, the .so travels with the repo snapshot).

The library is several translation units -- pml_api.hip (contexts, tree upload, the sweeps, the C-ABI), pml_api_readers.hip (the
C-ABI entries that read what a marginal pass left on the device), pml_schedule.cpp, pml_columns.cpp, pml_pij_window.cpp and pml_time_segments.cpp (the host-only
planning of the tree schedules, of the column layout, of the P(t) window and of the time segments, compiled as plain C++) and one pml_launch_*.hip per kernel family
(each with its pml_kernels_*.h; what the whole-tree and the per-interval exact histories share is in pml_kernels_history_shared.h and
pml_kernels_history_eigen_shared.h, which hold no kernel of one entry alone) -- compiled in parallel into pastml_amd/csrc/build/*.o (kept out of history and off the GPU box) and linked into one
shared object.  An object is recompiled when the digest of what IT is compiled from changes; the library carries the digest
over everything (pml_build_digest)."""
import hashlib
import os
import shutil
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(CSRC, 'build')
LIB = os.path.join(HERE, 'libpastml_hip.so')
SOURCES = ['pml_launch_f81_level.hip', 'pml_launch_f81_wide.hip', 'pml_launch_f81_small.hip', 'pml_launch_f81_blocks.hip', 'pml_launch_f81_super.hip',
           'pml_launch_matrix.hip', 'pml_launch_eigen_mfma.hip', 'pml_launch_eigen_gemm.hip', 'pml_launch_eigen_gemm_wide.hip', 'pml_launch_eigen_joint.hip', 'pml_launch_counts.hip', 'pml_launch_simulate.hip', 'pml_launch_scenarios.hip', 'pml_launch_parsimony.hip', 'pml_launch_expected.hip', 'pml_launch_gradient.hip', 'pml_launch_history.hip', 'pml_launch_history_eigen.hip', 'pml_launch_history_sample.hip', 'pml_launch_history_time.hip', 'pml_launch_history_time_eigen.hip', 'pml_launch_history_time_sample.hip', 'pml_launch_compress.hip', 'pml_launch_compress_horizontal.hip', 'pml_launch_compress_trim.hip', 'pml_launch_timeline.hip',
           'pml_schedule.cpp', 'pml_columns.cpp', 'pml_pij_window.cpp', 'pml_time_segments.cpp', 'pml_api_readers.hip', 'pml_api.hip']
HEADERS = ['pml_device.h', 'pml_kernels_f81.h', 'pml_kernels_misc.h', 'pml_model.h', 'pml_kernels_matrix.h', 'pml_kernels_pij.h', 'pml_kernels_pij_wide.h',
           'pml_kernels_counts.h', 'pml_philox.h', 'pml_kernels_simulate.h', 'pml_kernels_scenarios.h', 'pml_kernels_parsimony.h', 'pml_kernels_expected.h', 'pml_kernels_gradient.h', 'pml_kernels_history_shared.h', 'pml_kernels_history.h', 'pml_kernels_history_eigen_shared.h', 'pml_kernels_history_eigen.h', 'pml_kernels_history_sample.h', 'pml_kernels_history_time.h', 'pml_kernels_history_time_eigen.h', 'pml_kernels_history_time_sample.h', 'pml_kernels_compress.h', 'pml_kernels_compress_horizontal.h', 'pml_kernels_compress_trim.h', 'pml_kernels_timeline.h',
           'pml_kernels_eigen_mfma.h', 'pml_kernels_eigen_gemm.h', 'pml_kernels_eigen_joint.h', 'pml_comm.h', 'pml_schedule.h', 'pml_columns.h', 'pml_pij_window.h', 'pml_time_segments.h', 'pml_host.h', 'pml_call_scope.h', 'pml_results.h',
           'pml_launch.h', 'pml_launch_f81_level.h',
           os.path.join('..', '..', 'include', 'pastml_hip.h')]
CFLAGS = ['-O3', '--offload-arch=gfx950', '-std=c++17', '-ffp-contract=on', '-fPIC']
FLAGS = CFLAGS + ['-shared']
_MARKER = b'PML_BUILD_DIGEST='


def find_hipcc():
    for cand in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found')


def source_digest():
    """sha256 (16 hex digits) over everything the library is compiled from: sources, headers, flags."""
    h = hashlib.sha256()
    h.update(' '.join(FLAGS).encode())
    for name in SOURCES + HEADERS:
        h.update(os.path.basename(name).encode())
        with open(os.path.join(CSRC, name), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _unit_digest(source):
    """What one object file depends on: its source, every header (they are few and shared), the compile flags."""
    h = hashlib.sha256()
    h.update(' '.join(CFLAGS).encode())
    for name in [source] + HEADERS:
        h.update(os.path.basename(name).encode())
        with open(os.path.join(CSRC, name), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def library_digest(path=LIB):
    """The digest compiled into the library file (pml_build_digest), read without loading it; None if there is none."""
    try:
        with open(path, 'rb') as f:
            blob = f.read()
    except OSError:
        return None
    at = blob.find(_MARKER)
    if at < 0:
        return None
    end = blob.find(b'\0', at)
    return blob[at + len(_MARKER):end].decode('ascii', 'replace')


def is_stale():
    """The library is missing or was compiled from other sources than the tree holds (by content, not by time stamps)."""
    return library_digest() != source_digest()


def _compile(hipcc, source, digest, force, verbose):
    obj = os.path.join(OBJ, os.path.splitext(source)[0] + '.o')
    stamp = obj + '.digest'
    # pml_api.hip carries the library's digest: any change anywhere recompiles it (it is the quick one)
    want = _unit_digest(source) + (digest if source == 'pml_api.hip' else '')
    if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == want:
        return obj
    cmd = [hipcc] + CFLAGS + (['-x', 'c++'] if source.endswith('.cpp') else []) + ['-c', '-o', obj, source]
    if source == 'pml_api.hip':
        cmd.insert(-3, '-DPML_BUILD_DIGEST="{}"'.format(digest))
    t0 = time.time()
    subprocess.check_call(cmd, cwd=CSRC)
    if verbose:
        print('{:6.1f} s  {}'.format(time.time() - t0, ' '.join(cmd)), flush=True)
    with open(stamp, 'w') as f:
        f.write(want)
    return obj


def build(force=False, verbose=False, jobs=None):
    if not force and not is_stale():
        return LIB
    hipcc = find_hipcc()
    digest = source_digest()
    os.makedirs(OBJ, exist_ok=True)
    jobs = jobs or max(1, min(len(SOURCES), len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(jobs) as pool:
        objects = list(pool.map(lambda s: _compile(hipcc, s, digest, force, verbose), SOURCES))
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objects + ['-ldl']
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)
    return LIB


if __name__ == '__main__':
    import sys
    print(build(force='--incremental' not in sys.argv, verbose=True))
