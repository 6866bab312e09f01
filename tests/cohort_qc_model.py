"""The model of svjg_cohort_qc (svjg.h) in numpy, straight from the definitions: a 0/1 matrix per predicate, the per-sample sums their column sums,
the pair counts matrix products.  Integers only, so it is exact: no goldens, no tolerance.  The products run as float64 matrix products of 0/1
matrices: every entry is a count of rows, at most n_rows < 2^53, and so is every partial sum — exact, and quick at 2048 samples."""
import numpy as np

SAMPLE_FIELDS = ("eligible", "called", "carrier", "dip", "het", "homalt")
PAIR_FIELDS = ("both", "het1", "het2", "hethet", "ibs0")


def predicates(gt, ploidy=None):
    """-> {name: bool[n, S]} of the six per-item predicates and homref"""
    g = np.asarray(gt).astype(np.int64)
    P = np.full(g.shape, 2, np.int64) if ploidy is None else np.asarray(ploidy).astype(np.int64)
    eligible = P >= 1
    called = eligible & (g <= P)
    dip = called & (P == 2)
    return {"eligible": eligible, "called": called, "carrier": called & (g >= 1), "dip": dip, "het": dip & (g == 1), "homalt": dip & (g == 2),
            "homref": dip & (g == 0)}


def pair_index(S):
    """(i[k], j[k]) of the pairs i < j in the order of k = i S - i (i + 1) / 2 + (j - i - 1)"""
    i, j = np.triu_indices(S, 1)
    assert np.array_equal(i * S - i * (i + 1) // 2 + (j - i - 1), np.arange(len(i)))
    return i, j


def qc(gt, ploidy=None):
    """-> (sample[S, 6], pair[S (S - 1) / 2, 5]) int64"""
    gt = np.asarray(gt)
    n, S = gt.shape
    assert n < 2 ** 53
    p = predicates(gt, ploidy)
    sample = np.stack([p[f].sum(axis=0, dtype=np.int64) for f in SAMPLE_FIELDS], axis=1)
    D, H, A, R = (p[f].astype(np.float64) for f in ("dip", "het", "homalt", "homref"))
    full = {"both": D.T @ D, "het1": H.T @ D, "het2": D.T @ H, "hethet": H.T @ H, "ibs0": R.T @ A + A.T @ R}
    i, j = pair_index(S)
    pair = np.stack([full[f][i, j] for f in PAIR_FIELDS], axis=1).astype(np.int64).reshape(-1, 5)
    return sample.reshape(S, 6), pair


class ModelQc:
    """cohort_qc as capi.Context has it, answered by the model (uint32 arrays, like the library)"""

    def cohort_qc(self, gt, ploidy=None):
        sample, pair = qc(gt, ploidy)
        return sample.astype(np.uint32), pair.astype(np.uint32)
