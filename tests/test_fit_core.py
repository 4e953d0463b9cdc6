"""CPU: the fit contract (sequencealigner_amd/csrc/sa_fit_core.h -- the payload (identities, columns, begin) a DP state carries,
the end-cell rule, the walk step sa_tb_step_fit and the serial restatement sa_fit_pair the kernel mirrors) compiled with g++
-fsanitize=address,undefined into tests/host_c/fit_test and run on the host: the forward recurrence must give the score, the
database span, the identities and the columns of the contract's walk over literally filled tables, and for short database
sequences the score must be the brute-force maximum of the method's global score over every substring."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

# NW and Gotoh under BLOSUM62 with 4 and 10/1; gaps of zero; |open| < |extend|
BLOSUM_SCORINGS = [
    ("nw", dict(gap_pen=4)), ("ga", dict(gap_open=10, gap_extend=1)), ("nw", dict(gap_pen=0)),
    ("ga", dict(gap_open=0, gap_extend=0, equal_affine_to_nw=False)), ("ga", dict(gap_open=3, gap_extend=7)),
]
# the harness's asymmetric small-valued table: (method, g, o, e) in stored form
ASYM_SCORINGS = [(0, -1, 0, 0), (0, 0, 0, 0), (1, 0, -5, -1), (1, 0, -1, -3), (1, 0, 0, 0)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fit_core") / "fit_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "fit_test.cpp"), "-o", str(exe)])
    return exe


def run(harness, *args):
    res = subprocess.run([str(harness), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    m = re.search(r"fit ok: (\d+) pairs, (\d+) end row 0, (\d+) m < n, (\d+) inside, (\d+) with gaps, (\d+) against brute force, (\d+) planted",
                  res.stdout)
    assert m, res.stdout
    return dict(zip(("pairs", "end0", "shorter", "inside", "gapped", "brute", "planted"), map(int, m.groups())))


def honest(c):
    """the counts that keep the inputs honest"""
    assert c["pairs"] == 4 * (2 * 6 * 7 + 80)
    assert c["end0"] > 0            # the query against nothing wins or ties: the end row is 0
    assert c["shorter"] > 0         # database sequences shorter than the query
    assert 4 * c["inside"] >= c["pairs"]  # the query sits strictly inside: db_begin > 0 and db_end < m
    assert c["gapped"] > 50         # alignments with gap columns: the X / Y payloads carry the begin
    assert c["brute"] == 4 * 2 * 3 * 7 and c["planted"] > c["pairs"] // 4


@pytest.mark.parametrize("method,gaps", BLOSUM_SCORINGS, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v.values())))
def test_forward_recurrence_equals_the_walk_and_the_best_substring(method, gaps, harness, sa, tmp_path):
    scoring = sa.Scoring.from_names(method, "blosum62", **gaps)
    assert scoring.method == {"nw": 0, "ga": 1}[method]
    table = tmp_path / "table.txt"
    table.write_text(" ".join(str(int(v)) for v in scoring.sub))
    honest(run(harness, table, scoring.method, scoring.gap_pen, scoring.gap_opn, scoring.gap_ext, 7))


@pytest.mark.parametrize("method,g,o,e", ASYM_SCORINGS)
def test_forward_recurrence_under_an_asymmetric_table(method, g, o, e, harness):
    """a small-valued table with sub != sub.T: many ties, and the index order of the two methods' lookups matters"""
    honest(run(harness, "asym", method, g, o, e, 11))
