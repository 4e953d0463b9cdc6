"""GPU (-m gpu): the `seqalign` tool across its modes -- every selection at once, over each quantity, the three *-only modes, -W,
the tile job and the host matrix -- against what the binding returns for the same store and scoring.  The per-feature tool tests
each drive one selection; this one drives the flow between them (cli/seqalign.c: main in phases)."""
import functools
import re

import numpy as np
import pytest

from tests.golden_util import tri_to_full
from tests.host_binding import h5_matrix, h5_sequences
from tests.synth import make_protein_set
from tests.test_edges_host import h5_array
from tests.test_gpu_cli import built_cli, run, write_fasta  # noqa: F401  (the tool's helpers, as they are)
from tests.test_neighbors_host import h5_dataset, h5_names

pytestmark = pytest.mark.gpu

K = 3
FRACTIONS = [0.9, 0.8, 0.25, 0.5]  # --min-quantile, --clusters-quantile, --quantiles: in the order the tool lists them
FLAGS = ["-a", "nw", "-m", "blosum62", "-p", 4, "-F", "-B"]
EVERYTHING = ["-k", K, "--min-quantile", 0.9, "--linkage", "--clusters-quantile", 0.8, "--quantiles", "0.25,0.5"]
SIZES = (40, 300)  # 40: below the 256 limit, the host-matrix path, every selection a second pass; 300: the tile job answers everything

NEIGHBOR_SETS = {"/neighbor_indices", "/neighbor_scores"}
EDGE_SETS = {"/edge_offsets", "/edge_indices", "/edge_scores"}
TREE_SETS = {"/linkage_pairs", "/linkage_scores"}
QUANTILE_SETS = {"/score_quantiles", "/score_quantile_values", "/score_quantile_below"}
NORM_SETS = {"/normalization_denominators", "/normalization_rule", "/normalization_scale"}
PID_SETS = {"/identity_rule", "/identity_scale"}
AGAIN = ", after a second alignment pass into device memory"
# the -B line of each selection
LINES = {"neighbors": "  (neighbor selection on the device", "quantiles": "  (Score quantiles on the device",
         "edges": "  (score graph on the device", "linkage": "  (single-linkage tree on the device"}


class Case:
    """one input of N short proteins: the file, the store, and what the binding says about it, each computed once"""

    def __init__(self, sa, n, directory):
        self.sa, self.n = sa, n
        self.seqs = make_protein_set(n, 8, 20, 100 + n)
        self.fasta = directory / f"in_{n}.fasta"
        write_fasta(self.fasta, self.seqs)
        self.store = sa.SequenceStore.from_sequences(self.seqs)
        self.scoring = sa.Scoring.from_names("nw", "blosum62", gap_pen=4)
        self.pairs = n * (n - 1) // 2

    @functools.lru_cache(maxsize=None)
    def matrix(self):
        return tri_to_full(self.sa.hip_align(self.store, self.scoring, triangular=True), self.n)

    def quantity(self, name):
        sa = self.sa
        return {"scores": {}, "self-min": dict(norm=sa.Norm(sa.NORM_SELF, sa.NORM_MIN)), "shorter": dict(pid=sa.PID_SHORTER)}[name]

    @functools.lru_cache(maxsize=None)
    def select(self, quantity, fractions):
        ranks = [self.sa.score_rank(self.pairs, q) for q in fractions]
        return self.sa.hip_select(self.store, self.scoring, ranks, **self.quantity(quantity))[:2]

    @functools.lru_cache(maxsize=None)
    def neighbors(self, quantity):
        return self.sa.hip_neighbors(self.store, self.scoring, K, **self.quantity(quantity))

    @functools.lru_cache(maxsize=None)
    def edges(self, quantity, min_score):
        return self.sa.hip_edges(self.store, self.scoring, min_score, **self.quantity(quantity))[:3]

    @functools.lru_cache(maxsize=None)
    def linkage(self, quantity):
        return self.sa.hip_linkage(self.store, self.scoring, **self.quantity(quantity))


@pytest.fixture(scope="module")
def cases(sa, tmp_path_factory):
    directory = tmp_path_factory.mktemp("cli_modes")
    return {n: Case(sa, n, directory) for n in SIZES}


def second_passes(stdout):
    """which selections the -B report says came from a second alignment pass"""
    found = {}
    for line in stdout.splitlines():
        for what, start in LINES.items():
            if line.startswith(start):
                assert what not in found, stdout
                found[what] = line.endswith(AGAIN + ")")
                assert found[what] == ("second alignment pass" in line), line
    return found


def check_neighbors(case, path, quantity):
    index, score = case.neighbors(quantity)[:2]
    assert np.array_equal(h5_dataset(path, "neighbor_indices", (case.n, K)), index)
    assert np.array_equal(h5_dataset(path, "neighbor_scores", (case.n, K)), score)


def check_quantiles(case, path, quantity, fractions):
    values, below = case.select(quantity, tuple(fractions))
    assert np.array_equal(h5_array(path, "score_quantiles", "<f8"), np.array(fractions))
    assert np.array_equal(h5_array(path, "score_quantile_values", "<i4"), values)
    assert np.array_equal(h5_array(path, "score_quantile_below", "<i8"), below)
    return [int(v) for v in values]


def check_edges(case, path, quantity, min_score):
    offsets, index, score = case.edges(quantity, min_score)
    assert np.array_equal(h5_array(path, "edge_offsets", "<i8"), offsets)
    assert np.array_equal(h5_array(path, "edge_indices", "<i4"), index)
    assert np.array_equal(h5_array(path, "edge_scores", "<i4"), score)


def check_linkage(case, path, quantity, clusters_at=None):
    pairs, score = case.linkage(quantity)[:2]
    assert np.array_equal(h5_dataset(path, "linkage_pairs", (case.n - 1, 2)), pairs)
    assert np.array_equal(h5_array(path, "linkage_scores", "<i4"), score)
    if clusters_at is not None:
        labels, _count = case.sa.linkage_labels(pairs, score, case.n, clusters_at)
        assert np.array_equal(h5_array(path, "cluster_labels", "<i4"), labels)


def check_quantity(case, path, quantity):
    sa = case.sa
    if quantity == "self-min":
        den = case.neighbors(quantity)[2]
        assert np.array_equal(h5_array(path, "normalization_denominators", "<i4"), den)
        assert h5_array(path, "normalization_rule", "<i4").tolist() == [sa.NORM_SELF, sa.NORM_MIN]
        assert h5_array(path, "normalization_scale", "<i4").tolist() == [sa.NORM_SCALE]
    if quantity == "shorter":
        assert h5_array(path, "identity_rule", "<i4").tolist() == [sa.PID_SHORTER]
        assert h5_array(path, "identity_scale", "<i4").tolist() == [sa.NORM_SCALE]


def check_everything(case, path, quantity, stdout, from_tile_job):
    """sets 1-3, 7, 8: every selection at once"""
    extra = {"scores": set(), "self-min": NORM_SETS, "shorter": PID_SETS}[quantity]
    assert h5_names(path) == {"/sequences", "/similarity_matrix", *NEIGHBOR_SETS, *EDGE_SETS, *TREE_SETS, "/cluster_labels", *QUANTILE_SETS,
                              "/edge_min_score", "/cluster_min_score", *extra}
    assert np.array_equal(h5_matrix(path, case.n), case.matrix()) and h5_sequences(path) == case.seqs  # (raw under every quantity)
    values = check_quantiles(case, path, quantity, FRACTIONS)
    assert h5_array(path, "edge_min_score", "<i4").tolist() == [values[0]]
    assert h5_array(path, "cluster_min_score", "<i4").tolist() == [values[1]]
    check_neighbors(case, path, quantity)
    check_edges(case, path, quantity, values[0])
    check_linkage(case, path, quantity, values[1])
    check_quantity(case, path, quantity)
    assert second_passes(stdout) == dict.fromkeys(LINES, not from_tile_job), stdout


def tile_job_runs(sa, n, env=None):
    """the tile job answers the selections: more than 256 sequences, a file to write, no switch against it, one device"""
    return n > 256 and not env and sa.device_count() == 1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("quantity,options", [("scores", []), ("self-min", ["--normalize", "self-min"]), ("shorter", ["--identity", "shorter"])])
def test_every_selection_at_once(quantity, options, n, cases, tmp_path, sa):
    case, out = cases[n], tmp_path / "all.h5"
    res = run("-i", case.fasta, "-o", out, *FLAGS, *EVERYTHING, *options)
    check_everything(case, out, quantity, res.stdout, tile_job_runs(sa, n))


def test_host_matrix_switch_leaves_everything_to_second_passes(cases, tmp_path, sa):
    case, out, env = cases[300], tmp_path / "hostmatrix.h5", {"SA_HOST_MATRIX": "1"}
    res = run("-i", case.fasta, "-o", out, *FLAGS, *EVERYTHING, env=env)
    check_everything(case, out, "scores", res.stdout, tile_job_runs(sa, 300, env))


@pytest.mark.parametrize("n", SIZES)
def test_no_write_selects_and_writes_nothing(n, cases, tmp_path, sa):
    case = cases[n]
    before = set(tmp_path.iterdir())
    res = run("-i", case.fasta, "-W", *FLAGS, *EVERYTHING)
    assert set(tmp_path.iterdir()) == before and not list(case.fasta.parent.glob("*.h5"))
    assert second_passes(res.stdout) == dict.fromkeys(LINES, True), res.stdout  # (no file, no tile job)
    values, _below = case.select("scores", tuple(FRACTIONS))
    offsets = case.edges("scores", int(values[0]))[0]
    assert f"min score = {values[0]}: {offsets[-1]} edges" in res.stdout, res.stdout
    assert re.search(rf"single-linkage tree on the device: {n - 1} merges", res.stdout), res.stdout


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("more", [[], [0.25, 0.5]], ids=["edges_at_rank", "select_then_edges"])
def test_edges_only(more, n, cases, tmp_path):
    """one fraction: the cut and the graph from one alignment; further fractions: one select call in a pass of its own, then the graph"""
    case, out = cases[n], tmp_path / "edges_only.h5"
    extra = ["--quantiles", ",".join(map(str, more))] if more else []
    res = run("-i", case.fasta, "-o", out, *FLAGS, "--edges-only", "--min-quantile", 0.9, *extra)
    assert h5_names(out) == {"/sequences", *EDGE_SETS, *QUANTILE_SETS, "/edge_min_score"}
    assert h5_sequences(out) == case.seqs
    values = check_quantiles(case, out, "scores", [0.9, *more])
    assert h5_array(out, "edge_min_score", "<i4").tolist() == [values[0]]
    check_edges(case, out, "scores", values[0])
    assert second_passes(res.stdout) == {"quantiles": bool(more), "edges": False}, res.stdout
    assert "only the edges come back" in res.stdout


@pytest.mark.parametrize("n", SIZES)
def test_linkage_only_with_quantiles(n, cases, tmp_path):
    case, out = cases[n], tmp_path / "linkage_only.h5"
    res = run("-i", case.fasta, "-o", out, *FLAGS, "--linkage-only", "--quantiles", "0.25,0.5")
    assert h5_names(out) == {"/sequences", *TREE_SETS, *QUANTILE_SETS}
    assert h5_sequences(out) == case.seqs
    check_quantiles(case, out, "scores", [0.25, 0.5])
    check_linkage(case, out, "scores")
    assert second_passes(res.stdout) == {"quantiles": False, "linkage": False}, res.stdout
    assert "only the single-linkage tree comes back" in res.stdout


@pytest.mark.parametrize("n", SIZES)
def test_neighbors_only(n, cases, tmp_path):
    case, out = cases[n], tmp_path / "neighbors_only.h5"
    res = run("-i", case.fasta, "-o", out, *FLAGS, "--neighbors-only", "-k", K)
    assert h5_names(out) == {"/sequences", *NEIGHBOR_SETS}
    assert h5_sequences(out) == case.seqs
    check_neighbors(case, out, "scores")
    assert second_passes(res.stdout) == {"neighbors": False}, res.stdout
    assert "only the neighbors come back" in res.stdout
