"""CPU: the row-stream builder of the packed kernels (sa_plan.cpp: sa_build_row_streams -- pure host code) compiled with
g++ -fsanitize=address,undefined into a stand-alone program (tests/host_c/row_streams_test.cpp) and run: the layout formula,
front and tail pads, code x stride at every position and the bound of every 16-position window the kernel loads, for both
group widths and the four row strides of the 8-lane classes K <= 16.
Any heap error or UB in the builder for these stores fails the test (-fno-sanitize-recover)."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "sequencealigner_amd" / "csrc"


def test_row_streams_against_a_naive_recomputation(tmp_path):
    exe = tmp_path / "row_streams_test"
    tables = tmp_path / "sa_tables.o"  # (sa_set_error lives beside the matrix tables: data, compiled without instrumentation)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-c", str(CSRC / "sa_tables.cpp"), "-o", str(tables)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Wno-unused-parameter", str(ROOT / "tests" / "host_c" / "row_streams_test.cpp"),
                           str(CSRC / "sa_plan.cpp"), str(tables), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-6000:]
    assert res.stdout.strip() == "ok 52", res.stdout
