"""NumPy (fp64) oracle of the gallery selection rule of include/efm_hip.h: rows scoring >= sim_th, score descending then row
ascending, empty slots (-inf, -1, -1), a zero-norm query matches nothing; identity mode = the top-k distinct labels at their best row."""
import numpy as np


def scores(query, gallery):
    """s[q][i] = <q, g_i> / |q| in fp64 (gallery rows used as stored); rows of zero-norm queries are -inf (no candidate)."""
    q = np.asarray(query, dtype=np.float64)
    g = np.asarray(gallery, dtype=np.float64)
    nrm = np.sqrt((q * q).sum(1))
    s = q @ g.T
    with np.errstate(divide="ignore", invalid="ignore"):
        s = s / nrm[:, None]
    s[nrm == 0] = -np.inf
    return s


def select(cand_s, cand_i, cand_l, k, sim_th=-np.inf, by_label=False):
    """Top-k of one query's candidates (arrays of score, row, label) -> (scores[k], rows[k], labels[k])."""
    cand_s = np.asarray(cand_s, dtype=np.float64)
    cand_i = np.asarray(cand_i, dtype=np.int64)
    cand_l = np.asarray(cand_l, dtype=np.int64)
    keep = (cand_s >= sim_th) & (cand_s > -np.inf) & (cand_i >= 0)
    cs, ci, cl = cand_s[keep], cand_i[keep], cand_l[keep]
    order = np.lexsort((ci, -cs))
    cs, ci, cl = cs[order], ci[order], cl[order]
    if by_label:
        _, first = np.unique(cl, return_index=True)
        first = np.sort(first)
        cs, ci, cl = cs[first], ci[first], cl[first]
    out_s = np.full(k, -np.inf)
    out_i = np.full(k, -1, dtype=np.int64)
    out_l = np.full(k, -1, dtype=np.int64)
    m = min(k, cs.size)
    out_s[:m], out_i[:m], out_l[:m] = cs[:m], ci[:m], cl[:m]
    return out_s, out_i, out_l


def topk(s, k, sim_th=-np.inf, labels=None, row_offset=0):
    """Per-query top-k of a score matrix s (nq, n); labels (n,) switches to identity mode (row mode reports label -1)."""
    nq, n = s.shape
    rows = np.arange(n) + row_offset
    lab = np.asarray(labels, dtype=np.int64) if labels is not None else np.full(n, -1)
    res = [select(s[q], rows, lab, k, sim_th, labels is not None) for q in range(nq)]
    return tuple(np.stack([r[j] for r in res]) for j in range(3))


def merge(parts, k, by_label=False):
    """Top-k over a list of per-part results (scores, rows, labels), each (nq, k_part)."""
    nq = parts[0][0].shape[0]
    res = []
    for q in range(nq):
        cs = np.concatenate([p[0][q] for p in parts])
        ci = np.concatenate([p[1][q] for p in parts])
        cl = np.concatenate([p[2][q] for p in parts])
        res.append(select(cs, ci, cl, k, -np.inf, by_label))
    return tuple(np.stack([r[j] for r in res]) for j in range(3))
