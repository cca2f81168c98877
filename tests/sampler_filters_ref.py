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


# ---- the two derived bounds of the GPU sampler tests, shared by tests/test_gpu_kernels.py and
# tests/test_gpu_sampler_filters.py
def _nucleus_cut_slack(lg_row, temp, top_p, n):
    """The nucleus itself is cut at top_p * Z: if the full distribution's cumulative at the cut lies within the same
    arithmetic's worst-case error (+ the float32 top_p) of top_p, the device may keep one candidate more or fewer, which
    renormalises every edge by that candidate's share.  -> that share (0.0 when the cut is not that close)."""
    if top_p >= 1.0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        xs = lg_row.astype(np.float64) / float(temp)
        pf = np.exp(xs - xs.max())
    order = np.lexsort((np.arange(len(pf)), -pf))
    pf = pf[order] / pf.sum()
    cf = np.cumsum(pf)
    ef = (5.5 * np.abs(np.log(np.maximum(pf / pf[0], 1e-300))) + 2.0) * 2.0 ** -24
    slack = float(np.sum(pf * ef)) + abs(float(np.float32(top_p)) - top_p) + (len(pf) + 1) * 2.0 ** -40
    near = [k for k in (n - 2, n - 1) if 0 <= k < len(cf) and abs(cf[k] - top_p) <= slack]
    if not near:
        return 0.0
    return float(pf[min(n, len(pf) - 1)] / cf[n - 1]) + float(pf[n - 1] / cf[n - 1])


def _sampler_edge_bound(lg_row, temp, top_p, ids, pr, j, u):
    """How far the device's boundary between candidates j and j + 1 may lie from the oracle's cumulative c_j (DESIGN 2,
    "sampler boundary bound"), from the kernel's arithmetic (sampler.hip mass_fx / sample_kernel):
      * candidate i has the mass floor(2^40 * __expf((l_i - max) * (1/T))), __expf(a) = v_exp_f32(a * log2(e)).  The
        float32 roundings on the ARGUMENT -- l - max, 1/T, the product, log2(e), that product; T itself is a float32 on the
        device and a double in the oracle -- are 5.5 half-ulps = 5.5 * 2^-24 relative, i.e. a RELATIVE mass error of
        |a_i| * 5.5 * 2^-24 (a_i in nats), plus one ulp (2^-23) of v_exp_f32: eps_i = (5.5 |a_i| + 2) 2^-24;
      * c'_j - c_j = ((1 - c_j) sum_{i<=j} p_i e_i - c_j sum_{i>j} p_i e_i) / (1 + sum p_i e_i), |e_i| <= eps_i: the
        worst case puts every rounding below the edge one way and every one above it the other way;
      * truncation to 2^-40 fixed point: at most one unit per candidate and one for u * Z, against Z >= 2^40 (the
        largest mass is exactly 2^40);
      * u reaches the device as a float32: half an ulp of u.
    A function of the candidates' masses, the cumulative position and their number -- ~1e-7 for these rows; the measured
    edges (tools/debug/sampler_edge_probe.py, 136 boundaries) lie within 3.6e-8, i.e. the float32 u alone."""
    x = lg_row.astype(np.float64)
    a = np.abs((x[ids] - x.max()) / float(temp))
    p = np.asarray(pr, np.float64) / np.sum(pr)
    eps = (5.5 * a + 2.0) * 2.0 ** -24
    c = float(np.cumsum(p)[j])
    below, above = float(np.sum((p * eps)[: j + 1])), float(np.sum((p * eps)[j + 1:]))
    mass = ((1.0 - c) * below + c * above) / (1.0 - below - above)
    bound = mass + (len(ids) + 1) * 2.0 ** -40 + 0.5 * float(np.spacing(np.float32(u)))
    share = _nucleus_cut_slack(lg_row, temp, top_p, len(ids))
    return bound + share
