"""GPU (-m gpu): what the -z level means on the device (csrc/sa_deflate.hip): 0 raw tiles, 1 .. 6 the fixed parse, 7 .. 9 the
pair parse (8-byte matches onto equal pairs of elements in the 32 KB of the tile before them: sa_k_deflate_pairs,
sa_k_deflate_hist_pairs, sa_k_deflate_encode<true>).  Every tile of every level is a zlib stream that stock zlib
inflates to the oracle's tile, bit for bit; the higher levels must be worth their name in bytes; the same level gives the
same bytes."""
import subprocess
import zlib

import numpy as np
import pytest

from tests.golden_util import tri_to_full
from tests.test_gpu_deflate import expected_tiles

pytestmark = pytest.mark.gpu

N, CHUNK = 2100, 1024  # 3 x 3 tiles with partial edges, 64 segments and 4 code groups per tile
GAPS = {"nw": dict(gap_pen=4), "ga": dict(gap_open=10, gap_extend=1), "sw": dict(gap_open=10, gap_extend=1)}
_cache = {}


def case(sa, oracle, method):
    """store, scoring and the oracle's matrix cut into tiles -- once per method"""
    if method not in _cache:
        from tests.synth import make_protein_set
        store = sa.SequenceStore.from_sequences(make_protein_set(N, 20, 90, 17))
        scoring = sa.Scoring.from_names(method, "blosum62", **GAPS[method])
        full = tri_to_full(oracle.align(store, scoring, triangular=True), N)
        _cache[method] = (store, scoring, expected_tiles(full, CHUNK))
    return _cache[method]


def shells(sa, store, scoring, chunk, level):
    """every tile of a walk in shells: {(row, col): stream}, and the job's statistics"""
    seen = {}
    with sa.DeflateJob.begin(store, scoring, chunk, level=level) as job:
        while True:
            batch = job.next()
            if not batch:
                break
            for r, c, z in batch:
                assert (r, c) not in seen
                seen[(r, c)] = z
        return seen, job.stats()


@pytest.mark.parametrize("path", ["tile_row", "shells", "split"])
@pytest.mark.parametrize("method", ["nw", "ga", "sw"])
@pytest.mark.parametrize("level", [7, 9])
def test_pair_parse_tiles_inflate_to_the_oracles(level, method, path, sa, oracle, monkeypatch):
    store, scoring, (nc, want) = case(sa, oracle, method)
    if path == "tile_row":  # a finished packed matrix in device memory, row after row
        import torch
        d = torch.empty(store.pairs, dtype=torch.int32, device="cuda")
        with sa.Context(store, scoring, 0) as ctx:
            ctx.align_range(0, store.pairs, d.data_ptr())
            torch.cuda.synchronize()
        seen = {}
        with sa.DeflateJob(N, CHUNK, d_packed_ptr=d.data_ptr(), level=level) as job:
            assert job.tiles_per_row == nc
            for r in range(nc):
                for c, z in enumerate(job.tile_row(r)):
                    seen[(r, c)] = z
    else:  # while the alignment runs, shell after shell; "split": three jobs share the device, each with its own blocks
        if path == "split":
            monkeypatch.setenv("SA_HIP_TILES_SPLIT", "3")
        seen, _ = shells(sa, store, scoring, CHUNK, level)
    assert len(seen) == nc * nc
    for (r, c), z in seen.items():
        assert z[:2] == b"\x78\x9c"
        assert zlib.decompress(z) == want[r][c], f"level {level} {method} {path}: tile ({r},{c})"


def test_level_nine_is_smaller_than_level_six(sa):
    """NW / BLOSUM62 / -p 4 scores of 2048 proteins U[80, 120] (the cfg 2 generator), 2 x 2 tiles of 1024 x 1024 -- every tile
    past its first 32 KB has a full window of history: level 9 takes at least 5 % fewer bytes than level 6 (the serial
    restatement of the same parse reaches 7.1 % on the 1024 x 1024 tile of tests/test_deflate_pairs.py; the 5 % leaves
    room for other data of the same kind, not for another parse), and both inflate to the same tiles.  Measured on an
    MI355X: level 6 2.910 : 1, level 9 3.131 : 1, 7.1 % smaller."""
    from tests.synth import make_protein_set
    store = sa.SequenceStore.from_sequences(make_protein_set(2048, 80, 120, 2))
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    six, st6 = shells(sa, store, scoring, 1024, 6)
    nine, st9 = shells(sa, store, scoring, 1024, 9)
    assert sorted(six) == sorted(nine) and len(six) == 4
    for k in six:
        assert zlib.decompress(six[k]) == zlib.decompress(nine[k])
    assert st6["raw_bytes"] == st9["raw_bytes"] == 4 * 1024 * 1024 * 4
    print(f"level 6: {st6['raw_bytes'] / st6['out_bytes']:.3f} : 1, level 9: {st9['raw_bytes'] / st9['out_bytes']:.3f} : 1, "
          f"{100 * (1 - st9['out_bytes'] / st6['out_bytes']):.1f} % smaller")
    assert st9["out_bytes"] <= 0.95 * st6["out_bytes"], (st9["out_bytes"], st6["out_bytes"])


def test_same_level_same_bytes(sa):
    """levels 1 and 6 are one parse: identical streams; level 9 encoded twice: identical streams (the match finder's table
    takes the latest position under a key whatever order its lanes arrive in); 7 and 9 are one parse as well"""
    from tests.synth import make_protein_set
    store = sa.SequenceStore.from_sequences(make_protein_set(1300, 40, 120, 23))
    scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
    got = {name: shells(sa, store, scoring, 512, level)[0] for name, level in [("1", 1), ("6", 6), ("7", 7), ("9", 9), ("9 again", 9)]}
    assert len(got["6"]) == 9
    assert got["1"] == got["6"]
    assert got["9"] == got["9 again"]
    assert got["7"] == got["9"]
    assert got["9"] != got["6"]


def test_cli_z9_is_smaller_and_reads_back_the_same(tmp_path):
    """the tool: -z 9 writes the matrix -z 6 and the all-cores zlib path (SA_HOST_CPU_DEFLATE=1) write (h5diff), in a
    smaller file than -z 6"""
    from tests.host_binding import H5DUMP
    from tests.synth import make_protein_set
    from tests.test_gpu_cli import CLI, ROOT, run, write_fasta
    if not CLI.exists():
        subprocess.check_call(["make", "-s", "-C", str(ROOT / "cli")])
    fasta = tmp_path / "in.fasta"
    write_fasta(fasta, make_protein_set(1100, 80, 120, 2))
    flags = ["-a", "nw", "-m", "blosum62", "-p", 4]
    z9, z6, cpu = tmp_path / "z9.h5", tmp_path / "z6.h5", tmp_path / "cpu.h5"
    res = run("-i", fasta, "-o", z9, *flags, "-z", 9, "-B", "-F", "-V")
    assert "tiles deflated on the device" in res.stdout
    run("-i", fasta, "-o", z6, *flags, "-z", 6, "-F", "-Q")
    run("-i", fasta, "-o", cpu, *flags, "-z", 9, "-F", "-Q", env={"SA_HOST_CPU_DEFLATE": "1"})
    h5diff = H5DUMP.with_name("h5diff")
    for other in (cpu, z6):
        assert subprocess.run([str(h5diff), str(z9), str(other)], capture_output=True).returncode == 0
    props = subprocess.run([str(H5DUMP), "-p", "-H", "-d", "/similarity_matrix", str(z9)], capture_output=True, text=True).stdout
    assert "COMPRESSION DEFLATE { LEVEL 9 }" in props and "CHUNKED" in props
    print(f"-z 6: {z6.stat().st_size} bytes, -z 9: {z9.stat().st_size} bytes")
    assert z9.stat().st_size < z6.stat().st_size
