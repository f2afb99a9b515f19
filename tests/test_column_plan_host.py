"""The column layout's plan (csrc/pml_columns.h: pml_plan_columns), checked on the host.

tests/column_plan_driver.cpp is compiled together with pml_columns.cpp -- plain C++, no HIP runtime, no GPU, the library is not
loaded -- and plans every row of tests/golden/column_plan.txt: one line per case, the inputs (k, columns, the forest's three
traits, one tunable, the fused level table) and what the rules gave (ks, W, the lane groups G x R, Gf x Rf, Gt x Rt, bu_wide_lanes,
level_lists_sorted, levels_fit_workgroup, thin_units).

How the table was recorded: before pml_plan_columns replaced them, the rules stood inside pml_chars_alloc (pml_api.hip) and
pick_group (pml_host.h).  That block was pasted, unchanged, into a throw-away program that ran it on the CPU over the grid --
every k at a boundary of a rule x the eight combinations of the forest's traits, x F81_R, F81_TD_R, BU_WIDE, SORT_LEVELS on
three of them; then level tables at and one unit past whole passes of the walking workgroup, at and past the rule's 5/4 slack
and at 2 048 / 2 049 stored units x k x columns, with THIN_UNITS, THIN_BYTES and NO_THIN -- and printed the rows.  So the table
is the old code's output, not a restatement of the rules; a deliberate change of a rule edits its rows together with the
measurement that justifies it.

The driver also checks, for every row, what the table cannot say: every lane group is a power of two that holds k states; ks is
padded as the kernels need it; the parameter block's arrays are disjoint, in order, and cover the block exactly; the lane shapes
do not change with the number of columns; and every rejected input gives its reason and leaves the plan untouched.  (A sanitizer
build of the same driver is for running by hand: add -fsanitize=address,undefined to FLAGS.)"""
import os
import subprocess

from pastml_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ['-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-D_GLIBCXX_ASSERTIONS']


def test_column_plans(tmp_path):
    exe = str(tmp_path / 'column_plan_driver')
    sources = [os.path.join(HERE, 'column_plan_driver.cpp'), os.path.join(build.CSRC, 'pml_columns.cpp')]
    compiled = subprocess.run([build.find_hipcc()] + FLAGS + sources + ['-o', exe], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    assert 'warning' not in compiled.stderr, compiled.stderr
    ran = subprocess.run([exe, os.path.join(HERE, 'golden', 'column_plan.txt')], capture_output=True, text=True, timeout=600)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-2000:]
    assert ran.stdout.startswith('OK'), ran.stdout[-4000:]
