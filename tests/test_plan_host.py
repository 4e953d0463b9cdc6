"""CPU: the product's launch planner (sequencealigner_amd/csrc/sa_plan.cpp, sa_limits.cpp -- pure host code, no HIP)
compiled with g++ -fsanitize=address,undefined into tests/plan_host/plan_check and run on the geometry of the BASELINE
configs.  plan_check rebuilds every plan exactly as sa_ctx_align_range / sa_ctx_align_share do and checks it: every
pair of the range in exactly one tile, tile lists and dense shares inside their buffers, placement segments writing
every element once, arranged copies being block-local permutations.  Any heap error, overflow or UB in the planner
for these shapes fails the test (-fno-sanitize-recover).

cfg 5 is the geometry of the one abort this project has on record (round 3, test_baseline_full_size_cfg4_cfg5[cfg5]:
ranges [k 2^30, +2^30) of the 89 994-sequence post-filter store)."""
import json
import pathlib
import re
import subprocess

import numpy as np
import pytest

from tests import token_classes as tc
from tests.limits_line import parse_limits
from tests.planner_limits import PK16_F16_KMAX, class_of, form_of
from tests.synth import make_config, make_protein_set

ROOT = pathlib.Path(__file__).resolve().parents[1]
HARNESS = ROOT / "tests" / "plan_host"
CSRC = ROOT / "sequencealigner_amd" / "csrc"
G30 = 1 << 30


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_host") / "plan_check"
    srcs = [HARNESS / "plan_check.cpp", CSRC / "sa_plan.cpp", CSRC / "sa_limits.cpp"]
    # (the matrix tables are data: compiled without instrumentation, which is most of their build time)
    tables = exe.with_name("sa_tables.o")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-c", str(CSRC / "sa_tables.cpp"), "-o", str(tables)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Wno-unused-parameter", *map(str, srcs), str(tables), "-o", str(exe)])
    return exe


def lens_file(tmp_path, name: str, lens: np.ndarray) -> pathlib.Path:
    p = tmp_path / f"lens_{name}.i32"
    np.asarray(lens, np.int32).tofile(p)
    return p


def config_lens(name: str) -> tuple[np.ndarray, dict]:
    seqs, cfg = make_config(name)
    lens = np.array([len(s) for s in seqs], np.int32)
    if name == "cfg5":  # `-f 0.9` first: the reference's own keep mask (tests/golden/stripes_cfg5.npz)
        d = np.load(ROOT / "tests" / "golden" / "stripes_cfg5.npz")
        lens = lens[np.unpackbits(d["keep_packed"])[:len(seqs)].astype(bool)]
        assert lens.size == json.loads(str(d["params"]))["kept"]
    return lens, cfg


def run(exe, lens_path, method, matrix, gaps, plans, cus=256, timeout=900, tokens=None):
    """tokens: SA_HIP_CHUNK of the plans (0: none), and a `tokens:` line per packed class behind every plan"""
    argv = [str(exe)] + ([] if tokens is None else ["--tokens", str(tokens)])
    argv += [str(lens_path), method, matrix, str(gaps.get("gap_pen", 0)), str(gaps.get("gap_open", 0)),
             str(gaps.get("gap_extend", 0)), str(cus)]
    for p in plans:
        argv += [str(int(v)) for v in p]
    res = subprocess.run(argv, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, f"{' '.join(argv)}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-6000:]
    return res.stdout


def test_cfg2_every_schedule(plan_check, tmp_path):
    """10 000 x ~100 aa: the one-GPU whole-range launch, ranges that start and end inside columns, the world-8 / world-3
    share plans with and without host delivery -- placement checked element by element"""
    lens, cfg = config_lens("cfg2")
    pairs = lens.size * (lens.size - 1) // 2
    out = run(plan_check, lens_file(tmp_path, "cfg2", lens), cfg["method"], cfg["matrix"], cfg["gaps"],
              [(0, -1, 0, 1), (0, -1, 0, 0), (12345, pairs - 12345 - 777, 0, 0), (pairs // 3, pairs // 8, 0, 0),
               (0, -1, 8, 1), (0, -1, 8, 0), (0, -1, 3, 1), (0, -1, 1, 0), (pairs // 2, pairs // 5, 8, 0)])
    assert out.count("plan [") == 9 and "refused" not in out
    assert "world 8 host 1" in out and "/16/4," in out  # two tile sizes in a short launch


def test_cfg3_and_cfg4_shapes(plan_check, tmp_path):
    lens, cfg = config_lens("cfg3")
    out = run(plan_check, lens_file(tmp_path, "cfg3", lens), cfg["method"], cfg["matrix"], cfg["gaps"], [(0, -1, 0, 1), (0, -1, 4, 1)])
    assert out.count("plan [") == 2
    lens, cfg = config_lens("cfg4")  # 50 000 reads, SW: two bundles (K = 15..23), 2^30-pair ranges as the parity test issues them
    out = run(plan_check, lens_file(tmp_path, "cfg4", lens), cfg["method"], cfg["matrix"], cfg["gaps"],
              [(0, G30, 0, 0), (G30, -1, 0, 0), (0, -1, 0, 1)])
    assert out.count("plan [") == 3 and "2 bundles" in out


def test_cfg5_geometry_of_the_recorded_abort(plan_check, tmp_path):
    """the exact calls of tests/test_gpu_parity.py::test_baseline_full_size_cfg4_cfg5[cfg5] -- four ranges of 2^30 pairs
    over the post-filter store, the second to fourth starting inside a column and beyond packed index 2^31 -- and the
    whole 4.05e9-pair range as sa_ctx_align_host plans it"""
    lens, cfg = config_lens("cfg5")
    pairs = int(lens.size) * (int(lens.size) - 1) // 2
    assert lens.size == 89994 and (1 << 31) < pairs < (1 << 32)
    out = run(plan_check, lens_file(tmp_path, "cfg5", lens), cfg["method"], cfg["matrix"], cfg["gaps"],
              [(0, G30, 0, 0), (G30, G30, 0, 0), (2 * G30, G30, 0, 0), (3 * G30, -1, 0, 0), (0, -1, 0, 1)])
    assert out.count("plan [") == 5 and "refused" not in out


def test_every_kernel_family_in_one_store(plan_check, tmp_path):
    """lengths 1 .. 2600: 8- and 16-lane packed classes, s32 classes, strip-mined columns; Gotoh with |open| < |extend|
    sends everything to the pair-per-wave runs; a world that does not divide anything"""
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.integers(1, 200, 700), rng.integers(200, 1024, 250), rng.integers(1025, 2600, 50), [1, 1, 2, 1023, 1024, 1025]])
    rng.shuffle(lens)
    f = lens_file(tmp_path, "mixed", lens)
    pairs = lens.size * (lens.size - 1) // 2
    plans = [(0, -1, 0, 0), (0, -1, 0, 1), (0, -1, 3, 0), (0, -1, 7, 1), (1000, pairs - 5000, 5, 0), (pairs - 10, 10, 2, 0), (0, 1, 0, 0)]
    for method, matrix, gaps in (("nw", "blosum62", dict(gap_pen=4)), ("sw", "blosum62", dict(gap_open=10, gap_extend=1)),
                                 ("ga", "pam250", dict(gap_open=12, gap_extend=2)), ("ga", "blosum62", dict(gap_open=1, gap_extend=5)),
                                 ("nw", "blosum62", dict(gap_pen=300))):
        out = run(plan_check, f, method, matrix, gaps, plans)
        assert out.count("plan [") == len(plans) and "refused" not in out
        if gaps.get("gap_extend") == 5 or gaps.get("gap_pen") == 300:
            assert f"generic {pairs} pairs" in out  # nothing the systolic families reproduce exactly


def test_tiny_stores_and_many_ranks(plan_check, tmp_path):
    for n in (2, 3, 9):
        lens = np.full(n, 30, np.int32)
        out = run(plan_check, lens_file(tmp_path, f"tiny{n}", lens), "nw", "blosum62", dict(gap_pen=4),
                  [(0, -1, 0, 0), (0, -1, 8, 0), (0, -1, 8, 1), (0, 1, 2, 0)])
        assert out.count("plan [") == 4


def test_oversized_range_is_refused_not_crashed(plan_check, tmp_path):
    """1.1e6 sequences of 8 residues: 6e11 pairs are more workgroup-tiles than one launch can number -- the planner
    says so (sa_last_error) instead of overflowing; the caller splits the range"""
    lens = np.full(1_100_000, 8, np.int32)
    out = run(plan_check, lens_file(tmp_path, "huge", lens), "nw", "blosum62", dict(gap_pen=4), [(0, -1, 0, 0), (0, G30, 0, 0)])
    assert "refused: packed range too large for one launch" in out
    assert out.count("plan [") == 2 and out.count("refused") == 1  # the 2^30-pair sub-range plans fine


# ---- the stores of tests/test_gpu_token_classes.py: which arranged level every tile of every class streams ----
TOKENS_LINE = re.compile(r"tokens: G (\d+) K (\d+) f16 (\d) small (\d) wpb (\d+) rows (\d+) lean((?: \d+:\d+)*) legacy (\d+)")


def token_plans(out):
    """per `plan [` line of plan_check --tokens: {(G, K): dict(f16, wpb, rows, lean = {block: tiles}, legacy)}"""
    plans = []
    for line in out.splitlines():
        if line.startswith("plan ["):
            plans.append({})
        m = TOKENS_LINE.match(line)
        if m:
            assert m[4] == "0", line  # (SA_HIP_CHUNK: one tile size)
            lean = {int(b): int(n) for b, n in (x.split(":") for x in m[7].split())}
            plans[-1][int(m[1]), int(m[2])] = dict(f16=m[3] == "1", wpb=int(m[5]), rows=int(m[6]), lean=lean, legacy=int(m[8]))
    return plans


def check_class_tiles(c, g, k, method, tag):
    """the three kinds of tile the store is built for, in the tile shape the class is meant to have"""
    waves = 8 if (g == 16 and k >= 45) or (method == "nw" and g == 8 and k >= 17) else 4  # sa_shapes.h: sa_pk_wpb
    assert c["wpb"] == waves and c["rows"] == waves * (64 // g) * tc.CHUNK, f"{tag}: {c}"
    assert any(n >= 1 for b, n in c["lean"].items() if b > c["rows"]), f"{tag}: no lean tile inside a larger arranged block: {c}"
    assert c["lean"].get(c["rows"], 0) >= 1, f"{tag}: no lean tile that is its own block: {c}"
    assert c["legacy"] >= 1, f"{tag}: no tile that derives its tokens: {c}"


@pytest.mark.parametrize("g,klo", tc.BUNDLES, ids=[f"g{g}-klo{klo}" for g, klo in tc.BUNDLES])
def test_token_class_stores_aim_where_they_claim(g, klo, plan_check, tmp_path):
    """every class of the bundle is admitted on the form the limits give (nothing goes to the s32 kernels), and -- in the
    whole range and in the range of its three columns alone -- has lean tiles inside the 256-row arranged block, lean
    tiles that are their own block, tiles that derive their tokens, and four or eight waves per workgroup as listed"""
    lens = tc.store_lengths(g, klo)
    f = lens_file(tmp_path, f"tc_{g}_{klo}", lens)
    classes = tc.bundle_classes(g, klo)
    ranges = [(0, -1, 0, 0)]
    for k in classes:
        j = tc.first_column(g, klo, k)
        assert [lens[j + c] for c in range(3)] == tc.column_lengths(g, k)
        ranges.append((j * (j - 1) // 2, 3 * j + 3, 0, 0))  # tri(j) through the end of column j + 2
    for method, gaps in tc.METHODS:
        out = run(plan_check, f, method, tc.MATRIX, gaps, ranges, tokens=tc.CHUNK)
        lim = parse_limits(out)
        plans = token_plans(out)
        assert len(plans) == len(ranges) and "refused" not in out
        for n, k in enumerate(classes):
            tag = f"{method} G {g} K {k}"
            assert class_of(g * k, lim) == (g, k) == class_of(g * k - (g - 1), lim), f"{tag} is not a packed class under {lim}"
            assert set(plans[1 + n]) == {(g, k)}, f"{tag}: its three columns alone plan {sorted(plans[1 + n])}"
            for c in (plans[0][g, k], plans[1 + n][g, k]):
                assert c["f16"] == form_of(g, k, lim)[1], f"{tag}: {c} under {lim}"
                check_class_tiles(c, g, k, method, tag)
        if g == 16:  # what these stores count on: the three-way form wherever it exists, the two-way form only beyond
            assert [k for k in classes if not plans[0][g, k]["f16"]] == [k for k in classes if k > PK16_F16_KMAX], (method, lim)


@pytest.mark.parametrize("g,klo", tc.LOW_K_TWO_WAY, ids=[f"g{g}-klo{klo}" for g, klo in tc.LOW_K_TWO_WAY])
def test_token_class_stores_with_a_one_residue_row(g, klo, plan_check, tmp_path):
    """a one-residue row in front: the limits move the low 16-lane classes to the two-way u16 form (NW: all of them), and
    every class they still admit keeps its three kinds of tile"""
    lens = tc.store_lengths(g, klo, short_row=True)
    assert lens[0] == 1 and min(lens[1:]) == tc.ROW_MIN
    f = lens_file(tmp_path, f"tc1_{g}_{klo}", lens)
    for method, gaps in tc.METHODS:
        out = run(plan_check, f, method, tc.MATRIX, gaps, [(0, -1, 0, 0)], tokens=tc.CHUNK)
        lim = parse_limits(out)
        plan, = token_plans(out)
        admitted = [k for k in tc.bundle_classes(g, klo) if k <= lim["pk16"]]
        assert [k for gg, k in sorted(plan) if gg == 16] == admitted and (admitted or klo > 13), (method, lim, sorted(plan))
        two_way = [k for k in admitted if not plan[g, k]["f16"]]
        assert two_way == [k for k in admitted if k > lim["f16"]] and (two_way or klo > 13), (method, lim, two_way)
        for k in admitted:
            check_class_tiles(plan[g, k], g, k, method, f"{method} G {g} K {k} with a one-residue row")


def test_short2100_shares_have_lean_tiles_of_both_sizes(plan_check, tmp_path):
    """the store of tests/test_gpu_token_streams.py::test_shares_of_two_tile_sizes: world 2 and 8 cut it into two tile sizes
    (chunk_pk / chunk_pk_small), and both have tiles that stream tokens, host delivery included"""
    lens = [len(s) for s in make_protein_set(2100, 5, 20, 49)]
    out = run(plan_check, lens_file(tmp_path, "short2100", lens), "nw", "blosum62", dict(gap_pen=4),
              [(0, -1, 2, 0), (0, -1, 8, 0), (0, -1, 8, 1)], tokens=0)
    assert out.count("plan [") == 3 and "refused" not in out
    blocks = out.split("plan [")[1:]
    for b in blocks:
        sizes = {m[4]: 0 for m in TOKENS_LINE.finditer(b)}
        for m in TOKENS_LINE.finditer(b):
            sizes[m[4]] += sum(int(x.split(":")[1]) for x in m[7].split())
        assert set(sizes) == {"0", "1"} and all(sizes.values()), f"plan [{b}"
