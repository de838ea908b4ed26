"""The radius decision of magnify_amd/csrc/mg_radius.h -- range test and layer of a circle candidate from its squared
radius, two compares against a table of float32 thresholds -- against the square root it replaces.  No GPU:
tests/candidate_radius_main.cpp is compiled for the host as a stand-alone program and run as a child process; it
checks EVERY float32 s from 0 to the first value above (max_r + 1)^2, and NaN, +inf and -0, each with sqrtf(s) and its
two float32 neighbours as the guess.  A few tens of millions of values a case and more than a billion bit patterns
below them (denormals, everything below min_r^2): seconds.  Its `sum` mode checks the float32 image coordinate of the
key-only kernel against the reference's float64 sum."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "candidate_radius_main.cpp")


def host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (the build needs one as well)")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("radius") / "candidate_radius_main")
    # -ffp-contract=off as the library; no -ffast-math: sqrtf and rintf are the library's, correctly rounded
    subprocess.run([host_compiler(), "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe, "-lm"],
                   check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module")
def runs(program):
    """The three cases run side by side, a process each; (return code, output) by case."""
    cases = [(2, 26), (5, 14), (5, 25)]
    procs = {c: subprocess.Popen([program, str(c[0]), str(c[1])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for c in cases}
    outs = {c: p.communicate()[0] for c, p in procs.items()}
    return {c: (procs[c].returncode, outs[c]) for c in cases}


@pytest.mark.parametrize("min_r,max_r", [(2, 26), (5, 14), (5, 25)])
def test_range_and_layer_equal_the_square_roots(runs, min_r, max_r):
    code, out = runs[(min_r, max_r)]
    assert code == 0, out
    # every bit pattern from +0 to the float above (max_r + 1)^2, and the five values beyond
    checked = int(out.split()[-1])
    assert out.startswith("checked") and checked > (max_r + 1) ** 2 and checked > 1_000_000_000, out


def test_float32_image_coordinate_equals_the_float64_sum(program):
    r = subprocess.run([program, "sum"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("checked"), r.stdout


def test_bad_arguments_are_refused(program):
    for args in ([], ["5"], ["6", "5"], ["-1", "3"], ["0", "32"]):
        assert subprocess.run([program] + args, stdout=subprocess.DEVNULL).returncode == 2, args
