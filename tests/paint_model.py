"""NumPy model of distPaint.py's per-window decision (distPaint.py:26-44, 62-87), for the tests only: which reference population an
individual is nearest to, from the pair counts D (differences) and C (jointly called sites) of a window.

It restates the reference's worker with np.nanmean and np.argmin themselves; the rank-sum p-value is formed per comparison from
    z = (s - n1 (n1 + n2 + 1) / 2) / sqrt(n1 n2 (n1 + n2 + 1) / 12),   p = Phi(z)
with average ranks and no tie correction (scipy.stats.ranksums, alternative="less"), Phi through math.erfc.  tests/test_paint_cpu.py
pins it to the goldens of the unmodified reference; the product's kernel and host table are compared with it, never the other way."""
import math
import warnings

import numpy as np


def pair_dist(D, C, min_sites):
    """d[i][j] = D / C as a float64 quotient, nan where C < minSites or C == 0 (Alignment.pairDist is the mean of an empty vector
    there); D, C: [n][n], the diagonal of C the individual's own called sites"""
    D, C = np.asarray(D, dtype=np.float64), np.asarray(C, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = D / C
    d[(C < min_sites) | (C == 0)] = np.nan
    return d


def ranksum_less_p(x, y):
    """p-value of scipy.stats.ranksums(x, y, alternative="less"); nan when either list holds a nan"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if np.isnan(x).any() or np.isnan(y).any():
        return float("nan")
    n1, n2 = len(x), len(y)
    both = np.sort(np.concatenate((x, y)))
    # average ranks: a value with `lt` smaller and `le` smaller-or-equal values has the ranks lt + 1 .. le
    ranks = (np.searchsorted(both, x, side="left") + np.searchsorted(both, x, side="right") + 1) / 2.0
    s = float(np.sum(ranks))
    z = (s - n1 * (n1 + n2 + 1) / 2.0) / math.sqrt(n1 * n2 * (n1 + n2 + 1) / 12.0)
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def pop_means(lists):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # "Mean of empty slice": a population all of whose pairs are nan
        return [np.nanmean(np.asarray(a, dtype=np.float64)) for a in lists]


def which_lowest_test(lists, p_threshold=0.05, noresult=-1):
    i = int(np.argmin(pop_means(lists)))
    for j in range(len(lists)):
        if i != j and ranksum_less_p(lists[i], lists[j]) > p_threshold:
            return noresult
    return i


def which_lowest_delta(lists, delta_threshold=0, noresult=-1):
    means = pop_means(lists)
    i = int(np.argmin(means))
    s = sorted(means)
    if s[1] - s[0] < delta_threshold:
        return noresult
    return i


def paint_window(D, C, ref_lists, min_sites, p_threshold=0.05, delta_threshold=None, noresult=-1, info=None):
    """one window: int decision per individual (row of D / C).  ref_lists: per population the reference individuals as row indices,
    duplicates kept.  info (a dict): counts what the window contained -- nan pairs, all-nan and partly nan lists, nan in the best population, cells
    with a nan mean (the ones a device leaves to the host in delta mode), tied quotients inside a comparison"""
    d = pair_dist(D, C, min_sites)
    n = len(d)
    out = np.zeros(n, dtype=np.int32)
    nan_mean = np.zeros(n, dtype=bool)
    for i in range(n):
        lists = [d[i, np.asarray(r, dtype=np.int64)] for r in ref_lists]
        means = pop_means(lists)
        nan_mean[i] = bool(np.isnan(means).any())
        if delta_threshold is not None:
            out[i] = which_lowest_delta(lists, delta_threshold, noresult)
        else:
            out[i] = which_lowest_test(lists, p_threshold, noresult)
        if info is not None:
            best = int(np.argmin(means))
            info["nan_pairs"] = info.get("nan_pairs", 0) + int(sum(np.isnan(a).sum() for a in lists))
            info["all_nan_means"] = info.get("all_nan_means", 0) + int(sum(np.isnan(a).all() for a in lists))
            info["nan_in_best"] = info.get("nan_in_best", 0) + int(np.isnan(lists[best]).any())
            info["partly_nan_lists"] = info.get("partly_nan_lists", 0) + int(sum(np.isnan(a).any() and not np.isnan(a).all() for a in lists))
            info["nan_mean_cells"] = info.get("nan_mean_cells", 0) + int(nan_mean[i])
            for j, a in enumerate(lists):
                if j != best and not np.isnan(a).any() and not np.isnan(lists[best]).any():
                    both = np.concatenate((lists[best], a))
                    info["tied_values"] = info.get("tied_values", 0) + int(len(both) - len(np.unique(both)))
    return out, nan_mean


def paint_windows(D, C, ref_lists, min_sites, **kw):
    """[n_win][n] decisions and the cells with a nan mean"""
    res = [paint_window(D[w], C[w], ref_lists, min_sites, **kw) for w in range(len(D))]
    n = np.asarray(D).shape[1]
    return (np.array([r[0] for r in res], dtype=np.int32).reshape(len(D), n),
            np.array([r[1] for r in res], dtype=bool).reshape(len(D), n))
