"""The cohort sample QC (svjg_geno.h's QC routines inside a restatement of the loops of k_qc_planes and k_qc_pairs) through the host harness (tests only)."""
import numpy as np

from tests.geno_sim import QC, PTR, U32, U64, INT, calls, call, layout as _layout
from tests.geno_sim import build_main                                                  # noqa: F401

RUN_CODES = {1: "a store outside its field", 2: "a pair written twice or never", 3: "a plane word never written", 4: "a bit set behind the last row"}


def constants():
    """-> dict: TI, TJ (the pair kernel's tile), stage (64-row words a stage), max_samples, RI (pairs a lane), plane_words (words a lane of the
    plane kernel takes), waves, lds_slots, blocks_per_cu (the cap of both launches' grids)"""
    out = np.zeros(9, np.uint32)
    call("genosim_qc_constants", None, [PTR], out)
    return dict(zip(("TI", "TJ", "stage", "max_samples", "RI", "plane_words", "waves", "lds_slots", "blocks_per_cu"), (int(x) for x in out)))


def qc_class(g, P):
    """-> the six predicate bits of an item (bit q: field q of sample[s][6])"""
    return call("genosim_qc_class", U32, [U32, U32], int(g), int(P))


def tiles(S):
    return call("genosim_qc_tiles", U32, [U32], int(S))


def tile_at(t, S):
    ij = np.zeros(2, np.uint32)
    call("genosim_qc_tile_at", None, [U32, U32, PTR], int(t), int(S), ij)
    return int(ij[0]), int(ij[1])


def layout(n_rows, S, per_item):
    """svjg_geno.h: qc_layout -> dict of byte offsets (and in_bytes, total)"""
    return _layout(QC, n_rows, S, 0, int(bool(per_item)))


def pair_word(i3, j3):
    """(dip, het, homalt) words of i and of j -> the five counts of the word"""
    c = np.zeros(5, np.uint32)
    call("genosim_qc_pair_word", None, [PTR, PTR, PTR], np.ascontiguousarray(i3, np.uint64), np.ascontiguousarray(j3, np.uint64), c)
    return c


def run(gt, ploidy=None, grid_planes=0, grid_pairs=0):
    """both kernels' loops over a call (grids of that many blocks, 0: a block per unit of work) -> (sample[S, 6], pair[S (S - 1) / 2, 5]) uint32"""
    gt, ploidy, n, S = calls(gt, ploidy)
    sample, pair = np.zeros((S, 6), np.uint32), np.zeros((S * (S - 1) // 2 + 1, 5), np.uint32)
    rc = call("genosim_qc_run", INT, [PTR, PTR, U64, U32, U32, U32, PTR, PTR], gt, ploidy, n, S, int(grid_planes), int(grid_pairs), sample, pair)
    assert rc == 0, RUN_CODES.get(rc, rc)
    return sample, pair[:-1]


class SimQc:
    """cohort_qc as capi.Context has it, answered by the harness"""

    def cohort_qc(self, gt, ploidy=None):
        return run(gt, ploidy)
