"""The schedule of an SVGD step (dibs_amd/csrc/step_plan.h) is plain C++17 and is checked on the host: tests/tools/step_plan_check.cpp
(its invariants over a grid of engine facts, equality with the expressions of the commit before the plan existed, the rows of the five
bench configurations) builds with the host compiler, warnings as errors, and passes."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "tools", "step_plan_check.cpp")


def test_step_plan_invariants_parent_equality_and_pinned_rows():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "step_plan_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", CHECK, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert "step_plan_check: ok" in r.stdout
