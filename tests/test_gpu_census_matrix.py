"""gol_batch_census against numpy at every shape, seam and pattern size: the table of
tests/census_matrix_cases.py, one launch set per (shape, topology, family) -- both outputs, counts
alone, the residue alone -- and two tests on boards the device has stepped.  The expected values are
np_census's, which tests/test_census_matrix_cpu.py pins to the brute force of
tests/test_gpu_batch_census.py and shows not to be vacuous.  Every comparison is exact."""
import numpy as np
import pytest

import census_matrix_cases as T
from census_matrix_cases import np_census

pytestmark = pytest.mark.gpu


def same(got, want, where):
    """Exact equality; the message gives the first few (board, pattern) indices that differ, with
    the values got and wanted."""
    assert got.dtype == np.uint32, (where, got.dtype)
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (where, len(bad), bad[:8].tolist(), got[tuple(bad[:8].T)].tolist(),
                           want[tuple(bad[:8].T)].tolist())


def three_ways(b, patterns, counts, residue, where):
    """census(patterns) with both outputs, with counts alone and with the residue alone."""
    got_counts, got_residue = b.census(patterns)
    same(got_counts, counts, (where, "counts"))
    same(got_residue, residue, (where, "residue"))
    only, none = b.census(patterns, residue=False)
    assert none is None
    same(only, counts, (where, "counts alone"))
    none, only = b.census(patterns, counts=False)
    assert none is None
    same(only, residue, (where, "residue alone"))


@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_census(golhip, case):
    w, h, topology, family = case
    boards, patterns, _ = T.case(*case)
    counts, residue = T.expected(*case)
    with golhip.Batch(w, h, boards.shape[0], topology=topology) as b:
        b.load(boards)
        three_ways(b, patterns, counts, residue, case)
        if family == "mixed":  # the list the other way round: the same columns permuted, the same residue
            three_ways(b, patterns[::-1], counts[:, ::-1], residue, (case, "reversed"))
        same(b.alive_counts(), boards.sum(axis=(1, 2)), (case, "alive"))


@pytest.mark.parametrize("topology", T.TOPOLOGIES)
@pytest.mark.parametrize("shape", [(16, 64), (8, 16)], ids=["16x64", "8x16"])
def test_narrow_boards_after_steps(golhip, shape, topology):
    """Rows narrower than a word hold replicas of themselves, and after a step they are what the
    stepping kernels wrote, not load: 24 soups run 40 turns under B3/S23, then the dense-overlap list
    against np_census of what store() returns."""
    w, h = shape
    patterns = T.dense_patterns(shape)
    soups = np.concatenate([T.soup(np.random.default_rng([w, h, 40]), 12, shape, d) for d in (0.5, 0.3)])
    with golhip.Batch(w, h, soups.shape[0], topology=topology) as b:
        b.load(soups)
        b.step(40)
        cells = b.store()
        counts, residue = np_census(cells, patterns, topology)
        assert counts.sum() > 0 and (cells != 0).any() and not np.array_equal(cells != 0, soups != 0)
        three_ways(b, patterns, counts, residue, (shape, topology))


@pytest.mark.parametrize("shape", [(16, 64), (128, 8)], ids=["16x64", "128x8"])
def test_a_topology_switch_between_steps(golhip, shape):
    """No tracking: 20 turns on the torus, census on the plane, 20 turns on the plane, census on the
    torus; each against np_census of store() under the topology then in force."""
    w, h = shape
    patterns = T.dense_patterns(shape)
    soups = T.soup(np.random.default_rng([w, h, 20]), 16, shape, 0.5)
    with golhip.Batch(w, h, soups.shape[0]) as b:
        b.load(soups)
        for topology in ("plane", "torus"):
            b.step(20)
            b.set_topology(topology)
            assert b.topology == topology
            cells = b.store()
            counts, residue = np_census(cells, patterns, topology)
            other = np_census(cells, patterns, "torus" if topology == "plane" else "plane")
            assert counts.sum() > 0 and not np.array_equal(counts, other[0])  # the topology shows
            three_ways(b, patterns, counts, residue, (shape, topology))
        assert b.turn == 40
