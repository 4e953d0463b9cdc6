"""CPU: the half and quarter tiles of the launch planner (sa_plan.cpp with SaPlanInputs::remainder, the piece rule of
sa_shapes.h -- pure host code) compiled with g++ -fsanitize=address,undefined into a stand-alone program
(tests/host_c/remainder_tiles_test.cpp) and run: coverage, alignment and own blocks of the pieces, the size of the residual,
the stream builders on the new shapes, the lean count, and the plan without remainder tiles against the rule recomputed
naively -- over ranges, row bounds, worlds, chunks, output sides and the two arranging switches.  Any heap error or UB in
the planner on the way fails the test (-fno-sanitize-recover)."""
import pathlib
import re
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "sequencealigner_amd" / "csrc"


def test_remainder_tiles_of_every_plan(tmp_path):
    exe = tmp_path / "remainder_tiles_test"
    tables = tmp_path / "sa_tables.o"  # (sa_set_error lives beside the matrix tables: data, compiled without instrumentation)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-c", str(CSRC / "sa_tables.cpp"), "-o", str(tables)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Wno-unused-parameter", str(ROOT / "tests" / "host_c" / "remainder_tiles_test.cpp"),
                           str(CSRC / "sa_plan.cpp"), str(tables), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-6000:]
    m = re.fullmatch(r"ok (\d+) plans, (\d+) half and quarter tiles", res.stdout.strip())
    assert m and int(m.group(1)) >= 600 and int(m.group(2)) > 0, res.stdout
