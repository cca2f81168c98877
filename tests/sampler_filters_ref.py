"""The CPU definition of the sampler's top-k / top-p / min-p controls, built from the oracle and not from the
kernel: mask the row outside the top-k prefix, take the oracle's nucleus of the masked row, drop what min-p drops, pick."""
from __future__ import annotations

import numpy as np

from oracle import ref_sample


def oracle_order(lg_row) -> np.ndarray:
    """Candidate order: descending logit, ties by ascending id."""
    lg_row = np.asarray(lg_row)
    return np.lexsort((np.arange(len(lg_row)), -lg_row))


def kept_candidates(lg_row, temp, top_p=1.0, top_k=0, min_p=0.0):
    """-> (ids, masses): the kept set in draw order with float64 masses summing to 1."""
    row = np.array(lg_row, dtype=np.float32, copy=True)
    V = len(row)
    order = oracle_order(row)
    alive = V
    if 0 < top_k < V:
        row[order[top_k:]] = -np.inf
        alive = top_k
    if 0.0 < top_p < 1.0:
        with np.errstate(divide="ignore"):
            ids, pr = ref_sample.top_p_candidates(row, top_p, temp)
        ids, pr = np.asarray(ids), np.asarray(pr, dtype=np.float64)
    else:
        x = row[order[:alive]].astype(np.float64) / float(temp)
        ids, pr = order[:alive], np.exp(x - x.max())
    if min_p > 0.0:
        keep = ~(pr < float(min_p) * pr.max())
        ids, pr = ids[keep], pr[keep]
    return ids, pr / pr.sum()


def sample_row(lg_row, temp, u, top_p=1.0, top_k=0, min_p=0.0) -> int:
    if temp == 0:
        return int(np.argmax(np.asarray(lg_row)))
    ids, pr = kept_candidates(lg_row, temp, top_p, top_k, min_p)
    return ref_sample.inverse_cdf_pick(ids, pr, float(u))


def sample(logits, temp, uniforms, top_p=1.0, top_k=0, min_p=0.0) -> np.ndarray:
    return np.asarray([sample_row(r, temp, u, top_p, top_k, min_p) for r, u in zip(logits, uniforms)], dtype=np.int64)
