"""CPU: the pair parse of the device-side DEFLATE encoder (-z 7..9; sequencealigner_amd/csrc/sa_deflate_core.h, "the pair
parse") restated serially in tests/host_c/deflate_pairs_test.cpp -- the same core functions, the same order of events in
the match finder and the same claim rule as the kernels of csrc/sa_deflate.hip -- compiled with
g++ -fsanitize=address,undefined.  Every stream must inflate, with stock zlib, to exactly the input bytes, and on real
scores the parse must pay for itself."""
import pathlib
import re
import subprocess
import zlib

import numpy as np
import pytest

from tests.test_deflate_core import contents as core_contents

ROOT = pathlib.Path(__file__).resolve().parents[1]
CORE_KINDS = ["scores", "zeros", "constant", "full_range", "positive_small", "geometric", "one_element", "high_parts"]
PERIODS = [3, 9, 4095, 8192, 8193]  # 8192 elements = 32 768 bytes is the last distance DEFLATE has; 8193 must find nothing


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("deflate_pairs") / "deflate_pairs_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", str(ROOT / "tests" / "host_c" / "deflate_pairs_test.cpp"), "-o", str(exe)])
    return exe


def encode(harness, tmp_path, data: np.ndarray, segment: int, group: int, level: int):
    """-> (stream, elements inside pair matches in the stream, elements the match finder claimed: the two differ by the
    segments that are smaller without their pairs)"""
    src, dst = tmp_path / f"in{level}.i32", tmp_path / f"out{level}.zz"
    data.astype("<i4").tofile(src)
    res = subprocess.run([str(harness), str(src), str(dst), str(segment), str(group), str(level)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    m = re.search(r"(\d+) of \d+ elements inside pair matches \(the finder claimed (\d+)\)", res.stdout)
    return dst.read_bytes(), int(m.group(1)), int(m.group(2))


def contents(kind: str, rng, segment: int) -> np.ndarray:
    if kind in CORE_KINDS:
        return core_contents(kind, rng)
    if kind.startswith("period_"):  # full-range values: nothing but the pair match can code the repetition
        p = int(kind.split("_")[1])
        unit = rng.integers(-2**31, 2**31 - 1, size=p, dtype=np.int64).astype(np.int32)
        return np.resize(unit, 40000)
    if kind == "equal_pairs":  # every element has a candidate, in both rounds
        return np.full(40000, 0x01020304, np.int32)
    if kind == "segment_plus_two":
        return rng.integers(-150, 110, size=segment + 2, dtype=np.int32)
    raise ValueError(kind)


def test_distance_codes_match_the_rfc_table(harness):
    """sa_z_dist_code for every distance 1 .. 32 768 against RFC 1951 3.2.5, and against the nibble tables of the fixed parse"""
    res = subprocess.run([str(harness), "--dist"], capture_output=True, text=True)
    assert res.returncode == 0 and "dist ok" in res.stdout, res.stdout + res.stderr


@pytest.mark.parametrize("kind", CORE_KINDS + [f"period_{p}" for p in PERIODS] + ["equal_pairs", "segment_plus_two"])
@pytest.mark.parametrize("segment,group", [(16384, 1), (777, 1), (2048, 16)])
def test_pair_streams_inflate_to_the_input(kind, segment, group, harness, tmp_path):
    data = contents(kind, np.random.default_rng(len(kind) * 1000 + segment), segment)
    z, in_pairs, claimed = encode(harness, tmp_path, data, segment, group, 9)
    assert zlib.decompress(z) == data.astype("<i4").tobytes()
    assert in_pairs <= claimed
    fixed = encode(harness, tmp_path, data, segment, group, 6)[0]
    if in_pairs == 0:  # no segment kept a pair: the fixed parse's stream
        assert z == fixed
    if kind.startswith("period_"):
        p = int(kind.split("_")[1])
        if p > 8192:  # one element beyond the window: not one candidate
            assert claimed == 0
        elif p < 100:  # a handful of distinct pairs: the finder claims everything but the tile's first sub-block (1024 elements,
            # nothing inserted yet) and, per segment, an odd element out at either end
            assert claimed >= data.size - 1024 - 4 * (data.size // segment + 1)
        else:  # as many distinct pairs as the table has slots: collisions lose matches (by design), the window's edge is reached,
            # and with nothing else to gain from full-range values the segments keep their pairs
            assert in_pairs > 0 and len(z) < len(fixed)
    if kind == "equal_pairs" and segment == 16384:
        assert claimed >= data.size - 1024 - 2 * 3  # all but the first sub-block of the tile and an odd element per segment
    if kind == "full_range":
        assert len(z) < 1.15 * data.nbytes


def test_level_six_is_the_fixed_parse(harness, tmp_path):
    """below SA_Z_PAIR_LEVEL the harness is tests/host_c/deflate_core_test.cpp: no pair match, the same bytes"""
    data = core_contents("scores", np.random.default_rng(1))
    z, in_pairs, claimed = encode(harness, tmp_path, data, 16384, 16, 6)
    assert in_pairs == 0 and claimed == 0
    exe = harness.parent / "deflate_core_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", str(ROOT / "tests" / "host_c" / "deflate_core_test.cpp"), "-o", str(exe)])
    src, dst = tmp_path / "in6.i32", tmp_path / "core.zz"
    subprocess.check_call([str(exe), str(src), str(dst), "16384", "16"], stdout=subprocess.DEVNULL)
    assert dst.read_bytes() == z


def test_pair_parse_pays_on_real_scores(harness, tmp_path, oracle, sa):
    """NW / BLOSUM62 / -p 4 scores of 1024 proteins U[80, 120] (the cfg 2 generator) from the oracle, as the one
    1024 x 1024 tile they make (64 KB segments, one set of codes per MB): the pair stream is at least 5 % smaller than the
    fixed-parse stream of the same harness.  Measured: fixed parse 2.910 : 1, pair parse 3.134 : 1
    (7.1 % smaller, 72 % of the elements inside pair matches; zlib -6 on the same bytes: 3.310 : 1)."""
    from tests.golden_util import tri_to_full
    from tests.synth import make_protein_set
    n = 1024
    store = sa.SequenceStore.from_sequences(make_protein_set(n, 80, 120, 2))
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    tile = tri_to_full(oracle.align(store, scoring, triangular=True), n).astype(np.int32).reshape(-1)
    fixed = encode(harness, tmp_path, tile, 16384, 16, 6)[0]
    pairs, in_pairs, _ = encode(harness, tmp_path, tile, 16384, 16, 9)
    raw = tile.astype("<i4").tobytes()
    assert zlib.decompress(fixed) == raw and zlib.decompress(pairs) == raw
    print(f"fixed {len(raw) / len(fixed):.3f} : 1, pairs {len(raw) / len(pairs):.3f} : 1, {100 * (1 - len(pairs) / len(fixed)):.1f} % smaller, "
          f"{100 * in_pairs / tile.size:.0f} % of the elements inside pair matches; zlib -6 {len(raw) / len(zlib.compress(raw, 6)):.3f} : 1")
    assert len(pairs) <= 0.95 * len(fixed), (len(pairs), len(fixed))
