"""The product's own limits for a store, asked of the planner, and what follows from them for a column: the fixture and helpers
tests/test_gpu_value_range.py and tests/test_gpu_token_classes.py share.  Nothing of the bound is restated here: `planner`
runs tests/host_c/limits_sweep.cpp --print (sa_kernel_limits, compiled from the tree)."""
import pathlib
import re
import subprocess

import pytest

from tests import extremal as ex
from tests.limits_line import parse_limits, parse_shapes

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "sequencealigner_amd" / "csrc"

# the class lists of sa_shapes.h (not the bound); the planner fixture compares them with what the header says
PK_KMAX, PK16_KMIN, PK16_KMAX, PK16_F16_KMAX, SYS_CHUNK = 24, 13, 64, 52, 32
SHAPES = dict(pk_kmax=PK_KMAX, pk16_kmin=PK16_KMIN, pk16_kmax=PK16_KMAX, pk16_f16_kmax=PK16_F16_KMAX, pk_wpb=ex.PK_WPB, sys_chunk=SYS_CHUNK,
              long_w=ex.MAX_PACKED_LEN)

BUNDLE = re.compile(r"sa_k_systolic_pk_bundle<\w+,(\d+),(\d+),(true|false)>\[K(\d+)-(\d+)\]")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """limits(scoring, max_len, min_len) -> the planner's `limits:` line as a dict: the product's sa_kernel_limits, built
    from the tree with plain g++ (tests/test_limits_host.py runs the same harness under the sanitizers).  A scoring without
    a matrix name hands its table over as data (--sub FILE)."""
    tmp = tmp_path_factory.mktemp("limits")
    exe = tmp / "limits_sweep"
    srcs = [ROOT / "tests" / "host_c" / "limits_sweep.cpp", CSRC / "sa_plan.cpp", CSRC / "sa_limits.cpp", CSRC / "sa_tables.cpp"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", *map(str, srcs), "-o", str(exe)])
    out = subprocess.run([str(exe), "--print", "nw", "blosum62", "4", "0", "0", "1024", "1"], capture_output=True, text=True, check=True).stdout
    assert parse_shapes(out) == SHAPES, "the class geometry of sa_shapes.h changed: tests/extremal.py and the constants above aim at the wrong lengths"

    def limits(scoring, max_len, min_len):
        argv = [str(exe), "--print", scoring.method_name, scoring.matrix_name or "-", str(-scoring.gap_pen), str(-scoring.gap_opn),
                str(-scoring.gap_ext), str(int(max_len)), str(int(min_len))]
        if scoring.matrix_name == "":
            table = tmp / "sub.txt"
            table.write_text(" ".join(str(int(v)) for v in scoring.sub))
            argv += ["--sub", str(table)]
        out = subprocess.run(argv, capture_output=True, text=True, timeout=60, check=True).stdout
        return parse_limits(out)

    return limits


def forms(lim):
    """(name, lanes, last admitted K, largest K of the form) for the three packed forms"""
    return [("pk8", 8, lim["pk"], PK_KMAX), ("pk16-f16", 16, lim["f16"], min(PK16_F16_KMAX, lim["pk16"])), ("pk16-u16", 16, lim["pk16"], PK16_KMAX)]


def class_of(n, lim):
    """the kernel class a column of n residues runs in under these limits (plan_build's choice): (lanes, K) or None = s32"""
    k8, k16 = (n + 7) // 8, (n + 15) // 16
    if k8 <= lim["pk"]:
        return 8, k8
    if PK16_KMIN <= k16 <= lim["pk16"]:
        return 16, k16
    return None


def form_of(g, k, lim):
    """the form of forms(lim) an admitted class (g, k) runs on, and whether that is the three-way f16 form (the last template
    argument of its bundle kernel)"""
    for name, lanes, last, _ in forms(lim):
        if lanes == g and k <= last:
            return name, name != "pk16-u16"
    return None, None


PACKED_FORMS = ("pk8", "pk16-f16", "pk16-u16")


def columns_by_form(lens, lim):
    """{form name or "s32": the columns j >= 1 of a store with these lengths that the limits send there}"""
    out = {}
    for j in range(1, len(lens)):
        cls = class_of(lens[j], lim)
        out.setdefault(form_of(*cls, lim)[0] if cls else "s32", []).append(j)
    return out


def unreached_forms(lens, lim):
    """(name, lanes, last admitted K) of the forms the limits admit that no column of the store runs on"""
    by_form = columns_by_form(lens, lim)
    return [(name, g, k) for name, g, k, _ in forms(lim) if k and not (name == "pk16-u16" and k <= lim["f16"]) and not by_form.get(name)]
