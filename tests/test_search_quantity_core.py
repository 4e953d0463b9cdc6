"""CPU: the host-compilable core of the search quantities (sequencealigner_amd/csrc/sa_search_quantity_core.h -- the pieces a row
of the rectangle is cut into, the head / 16-byte vector / tail split of a piece, the 64-bit offsets, the wave-item mapping of the
identity rectangle, the take gather, and the rectangle sweep restated serially by the kernel's walk) compiled with
g++ -fsanitize=address,undefined into a stand-alone program (tests/host_c/search_quantity_test.cpp) and run on the host.  The kernel
(csrc/sa_search_quantity.hip: sa_k_normalize_rect) cuts and splits by the same functions and applies the same value rule,
sa_norm_value_t of sa_normalize_core.h; the expectation is sa_norm_value_rule element by element."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("search_quantity") / "search_quantity_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "search_quantity_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res.stdout


def test_pieces_cover_every_element_once(harness):
    """N in {1, 3, 4, 63, 64, 65, 1000, 1027} x nq in {1, 2, 7} x 4 x 4 misalignments of source and destination"""
    m = re.search(r"pieces ok: (\d+) cases", run(harness, "--pieces"))
    assert m and int(m.group(1)) == 8 * 3 * 16


def test_offsets_are_64_bit(harness):
    assert "offsets ok" in run(harness, "--offsets")


def test_the_serial_sweep_equals_the_value_rule(harness):
    """three rules, out of place and in place, q0 in {0, 2}, negative values among them.  This checks the walk: the rounding rule is
    sa_norm_value_rule's own (tests/test_normalize_host.py against __int128, the GPU tests against NumPy floor_divide)"""
    m = re.search(r"sweep ok: (\d+) cases, (\d+) negative values", run(harness, "--sweep"))
    assert m and int(m.group(1)) == 8 * 3 * 2 * 4 * 5 * 3 and int(m.group(2)) > 1000


def test_identity_items(harness):
    assert "items ok" in run(harness, "--items")


def test_take_gather(harness):
    assert "take ok" in run(harness, "--take")
