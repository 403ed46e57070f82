"""The K walk of the wide persistent conv over four and over three channel groups (csrc/conv_walk.hpp) without a GPU:
tests/cpp/conv_walk_check.cpp is that header and nothing else, compiled here with -fsanitize=address,undefined and run.  The program
replays three consecutive tiles of one workgroup pass by pass for both walks, independently of the header's own compile-time checks:
what every plane piece and ring slot holds and when it was requested, every fragment read against that (the right tile, group and
stream step, requested at least FLIGHT + 1 passes earlier), every overwrite against the last read, every pass's counted wait against
the requests of the last FLIGHT passes — across the window seam and the tile seam.  It also packs input-permuted weight images with
at most 96 live channels through the library's own packer and finds the stream steps 75 .. 99, which the three-group walk reads as its
zero steps, all zero."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "conv_walk_check.cpp"


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = tmp_path_factory.mktemp("conv_walk") / "conv_walk_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", str(SRC), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr     # a failed check or a sanitizer report ends the program with an error
    return r.stdout.splitlines()


def test_replay_of_both_walks(output):
    assert "replay NG=4: 50 passes per tile, 300 real steps read over 3 tiles" in output
    assert "replay NG=3: 40 passes per tile, 225 real steps read over 3 tiles" in output
    assert output[-1] == "conv_walk_check ok"
    assert not [line for line in output if line.startswith("FAIL")]


def test_zero_steps_of_the_permuted_stream(output):
    for n_live in (80, 96, 65):
        assert f"stream {n_live} live: steps 75 .. 99 zero" in output
    assert "stream 97 live: steps 100 .. 99 zero" in output      # the control: a live channel in the fourth group
