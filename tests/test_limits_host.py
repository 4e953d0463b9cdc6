"""CPU: properties of the value-range limits (sequencealigner_amd/csrc/sa_limits.cpp: sa_kernel_limits; sa_plan.cpp:
sa_pk_base, sa_pk_delta -- pure host code) over a grid, in tests/host_c/limits_sweep built with
g++ -fsanitize=address,undefined: every matrix the suite uses x NW gaps 0..60 and Gotoh / SW opens 0..60 with a ladder of
extends x shortest sequence 1..32 x longest 8..5000, and gaps up to 2^31 - 1.

  * pk_kmax, pk16_kmax and pk16_f16_kmax never grow when the shortest sequence gets shorter (more frame shifts in flight
    can only cost range);
  * pk16_f16_kmax <= pk16_kmax, and 16-lane classes exist only when every 8-lane class does;
  * for every admitted class sa_pk_base + sa_pk_delta + the largest profile entry fits the form's register range (0x7bff
    where the three-way maximum is the f16 one, 65535 otherwise).  This is the inequality between the planner's BASE / DELTA
    and the limits' admission, not a proof of the range: SW's drift budget (pk_extra) is not part of it, so for SW it holds
    with that whole budget to spare and would not notice a missing drift term -- the device run at full drift does
    (tests/test_gpu_value_range.py::test_sw_drift_of_the_packed_kernels);
  * no signed overflow or other undefined behaviour anywhere in that arithmetic (-fno-sanitize-recover).

What these limits admit is run on the device at its edges by tests/test_gpu_value_range.py."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

from tests.limits_line import parse_limits, parse_shapes

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "sequencealigner_amd" / "csrc"
MATRICES = ["blosum62", "blosum45", "blosum100", "blosum30", "pam30", "pam250", "pam500", "nuc44", "dnafull"]


@pytest.fixture(scope="module")
def limits_sweep(tmp_path_factory):
    exe = tmp_path_factory.mktemp("limits_host") / "limits_sweep"
    tables = exe.with_name("sa_tables.o")  # (the matrix tables are data: compiled without instrumentation)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-c", str(CSRC / "sa_tables.cpp"), "-o", str(tables)])
    srcs = [ROOT / "tests" / "host_c" / "limits_sweep.cpp", CSRC / "sa_plan.cpp", CSRC / "sa_limits.cpp"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Wno-unused-parameter", *map(str, srcs), str(tables), "-o", str(exe)])
    return exe


def test_limits_properties_over_the_grid(limits_sweep):
    procs = [(m, subprocess.Popen([str(limits_sweep), m], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for m in MATRICES]
    try:
        for matrix, p in procs:  # (one process per matrix, side by side)
            out, err = p.communicate(timeout=900)
            assert p.returncode == 0, f"{matrix}\n{out[-2000:]}\n{err[-6000:]}"
            assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-6000:]
            m = re.search(r"limits_sweep: (\d+) calls, (\d+) admitted classes checked, 0 failures", out)
            assert m and int(m[1]) > 100_000 and int(m[2]) > 100_000, out  # the grid really ran and really admitted classes
    finally:
        for _, p in procs:  # (a failed assert above must not leave the other sweeps running)
            if p.poll() is None:
                p.kill()
                p.wait()


def test_class_geometry_of_the_input_builders(limits_sweep):
    """tests/extremal.py restates the class geometry of sa_shapes.h (it has to stay pure numpy): the harness prints the
    header's values and they must agree, or the ladder aims at the wrong lengths"""
    from tests import extremal as ex
    out = subprocess.run([str(limits_sweep), "--print", "nw", "blosum62", "4", "0", "0", "1024", "1"], capture_output=True, text=True, check=True).stdout
    sh = parse_shapes(out)
    widths = [8 * k for k in range(1, sh["pk_kmax"] + 1)] + [16 * k for k in range(sh["pk16_kmin"], sh["pk16_kmax"] + 1)]
    assert ex.CLASS_WIDTHS == widths and ex.MAX_PACKED_LEN == 16 * sh["pk16_kmax"] == sh["long_w"] and ex.PK_WPB == sh["pk_wpb"]


def test_limits_line_of_the_boundaries_the_gpu_cases_rely_on(limits_sweep):
    """spot values of the `limits:` line (longest 1024).  These are TRIPWIRES for the case list of
    tests/test_gpu_value_range.py, not specifications: a deliberate change of the bound fails them without anything being
    wrong -- it then says, on a machine without a GPU, that test_the_boundaries_lie_inside_the_cases needs looking at and
    that these numbers are to be brought up to date"""
    def line(method, matrix, pen, o, e, longest, shortest):
        out = subprocess.run([str(limits_sweep), "--print", method, matrix, str(pen), str(o), str(e), str(longest), str(shortest)],
                             capture_output=True, text=True, check=True).stdout
        return tuple(parse_limits(out).values())

    assert line("nw", "blosum62", 20, 0, 0, 1024, 1)[1:4] == (15, 0, 0)        # an 8-lane boundary inside K = 1..24
    assert line("nw", "blosum62", 4, 0, 0, 1024, 3)[1:4] == (24, 43, 20)       # 16-lane: u16 and f16 boundaries inside
    assert line("sw", "blosum62", 0, 12, 3, 1024, 3) == (1, 24, 60, 21, 4)     # SW: chunk cap 4 at 1024 residues
    assert line("sw", "blosum62", 0, 2, 16700, 1000, 1000)[0] == 1             # the last extend the s32 kernels admit ...
    assert line("sw", "blosum62", 0, 2, 16800, 1000, 1000)[0] == 0             # ... and the first they do not


def test_limits_of_a_table_given_as_data(limits_sweep, tmp_path, sa):
    """--print --sub FILE under the sanitizers: a named matrix's own table handed over as data gives the named matrix's line,
    a malformed file is refused, and the line follows the table's entries -- with gaps of 0 the s32 family ends between the
    entries 127 and 128, -127 and -128 (the s8 profile, -128 reserved for padding)"""
    from tests import tables as tb

    def line(method, sub, pen, o, e, longest, shortest, matrix="-", check=True):
        table = tmp_path / "sub.txt"
        table.write_text("\n".join(str(int(v)) for v in np.asarray(sub, dtype=np.int64).reshape(-1)))
        res = subprocess.run([str(limits_sweep), "--print", method, matrix, str(pen), str(o), str(e), str(longest), str(shortest), "--sub", str(table)],
                             capture_output=True, text=True)
        assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-6000:]
        if not check:
            return res
        assert res.returncode == 0, res.stderr[-2000:]
        return parse_limits(res.stdout)

    for method, matrix, pen, o, e in (("nw", "blosum62", 4, 0, 0), ("ga", "pam250", 0, 30, 2), ("sw", "nuc44", 0, 10, 1)):
        named = subprocess.run([str(limits_sweep), "--print", method, matrix, str(pen), str(o), str(e), "1024", "3"], capture_output=True, text=True, check=True).stdout
        gaps = dict(gap_pen=pen) if method == "nw" else dict(gap_open=o, gap_extend=e)
        assert line(method, sa.Scoring.from_names(method, matrix, **gaps).sub, pen, o, e, 1024, 3) == parse_limits(named)
    base = tb.asymmetric(1, -4, 11)
    for method in ("nw", "sw"):
        assert line(method, tb.with_extremes(base, -127, 127), 0, 0, 0, 1024, 1)["sys_ok"] == 1
        assert line(method, tb.with_extremes(base, -127, 128), 0, 0, 0, 1024, 1)["sys_ok"] == 0
        assert line(method, tb.with_extremes(base, -128, 127), 0, 0, 0, 1024, 1)["sys_ok"] == 0
    assert line("nw", base[:575], 4, 0, 0, 1024, 1, check=False).returncode == 2
    assert line("nw", list(base) + [1], 4, 0, 0, 1024, 1, check=False).returncode == 2
    assert line("nw", [2 ** 31] + list(base[1:]), 4, 0, 0, 1024, 1, check=False).returncode == 2
