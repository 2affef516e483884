"""Masked k-means restated in plain numpy, row by row (nothing of the library's device code): what ppca_dataset_kmeans_step and
ppca_dataset_kmeans_seed (include/ppca_hip.h) compute, the Lloyd loop of `Dataset.kmeans`, and the two mixture starts built on the
clusters' pairwise moments (tests/moments_restatement.py) through the library's host-side `from_moments`.  No test lives here.

Masked entries are the non-finite ones; they are selected out, never multiplied.  With m_ij = 1 on observed entries:
    dist_ic = sum_j m_ij (a_j (x_ij - mu_cj))^2        label_i = the smallest c that attains min_c dist_ic
    tot_cj = sum_{i: label_i = c} w_i m_ij             sum_cj = sum_{i: label_i = c} w_i m_ij (x_ij - mu_cj)
    new mu_cj = mu_cj + sum_cj / tot_cj where tot_cj > 0, mu_cj elsewhere             inertia = sum_i w_i dist_i,label_i"""
import numpy as np

import moments_restatement as R

# The cases of the mixture starts, shared by tests/test_kmeans_host.py and tests/test_gpu_kmeans.py:
# (n, d, k, n_models, masked, seed, separation) of famix_restatement.synth with psi = 1 ...
TABLE = [(2000, 16, 2, 3, 0.3, 41, 3.0), (3000, 24, 3, 4, 0.4, 42, 3.0), (2500, 20, 2, 5, 0.5, 44, 3.0)]
# ... and the factor-analysis case, with the noise levels of fa_case_psi(): spread over 1e4
FA_CASE = (1200, 12, 2, 3, 0.3, 51, 3.0)


def fa_case_psi():
    d, seed = FA_CASE[1], FA_CASE[5]
    return np.random.default_rng(seed).permutation(np.logspace(-2.0, 2.0, d))


def _w(x, w):
    return np.ones(x.shape[0]) if w is None else np.asarray(w, dtype=np.float64)


def distances(x, centers, scale=None):
    """(N, K): every row's partial distance to every centre over the row's observed entries; 0 for a row with none."""
    n, d = x.shape
    a = np.ones(d) if scale is None else np.asarray(scale, dtype=np.float64)
    out = np.zeros((n, centers.shape[0]))
    for i in range(n):
        o = np.isfinite(x[i])
        t = (x[i, o] - centers[:, o]) * a[o]
        out[i] = (t * t).sum(axis=1)
    return out


def step(x, w, centers, scale=None):
    """(labels, dist, tot (K, d), sum (K, d), inertia, the (N, K) distances) of one Lloyd iteration from `centers`."""
    n, d = x.shape
    w = _w(x, w)
    nc = centers.shape[0]
    dm = distances(x, centers, scale)
    labels = np.argmin(dm, axis=1).astype(np.int32)  # (numpy's argmin: the first index that attains the minimum)
    dist = dm[np.arange(n), labels]
    tot, sums = np.zeros((nc, d)), np.zeros((nc, d))
    for i in range(n):
        o = np.isfinite(x[i])
        c = labels[i]
        tot[c, o] += w[i]
        sums[c, o] += w[i] * (x[i, o] - centers[c, o])
    return labels, dist, tot, sums, float(np.dot(w, dist)), dm


def new_centers(centers, tot, sums):
    ok = tot > 0.0
    return np.where(ok, centers + sums / np.where(ok, tot, 1.0), centers)


def relative_gaps(dm):
    """Every row's second-smallest minus smallest distance, relative to the row's largest distance: how far the row's label is from
    flipping under rounding.  inf with one centre; 0 for a row whose distances are all 0 (an exact tie, e.g. a row with no entry)."""
    n, nc = dm.shape
    if nc == 1:
        return np.full(n, np.inf)
    s = np.sort(dm, axis=1)
    big = s[:, -1]
    return np.where(big > 0.0, (s[:, 1] - s[:, 0]) / np.where(big > 0.0, big, 1.0), 0.0)


def _pick(terms, u):
    """(the smallest r with cumsum(terms)_r > u * total, |cumsum - u total| / total at the nearest boundary, total)."""
    cum = np.cumsum(terms)
    total = cum[-1]
    if not total > 0.0:
        return -1, np.inf, total
    r = int(np.argmax(cum > u * total))
    return r, float(np.min(np.abs(cum - u * total)) / total), total


def seed(x, w, u, scale=None, means=None):
    """k-means++ from the numbers u in [0, 1): (centres (K, d), rows (K), the pick margins (K)).  Centre 0: by the weights; centre c:
    by w_i D_i, D_i the distance to the nearest centre so far (the rule of centre 0 when they sum to 0).  A centre is its row where
    that is observed and the weighted column mean elsewhere (`means`: that vector from elsewhere, e.g. the device's own sums sweep,
    whose last bits depend on the order of its sums; default: moments_restatement.column_means)."""
    n, d = x.shape
    w = _w(x, w)
    g = R.column_means(x, w) if means is None else np.asarray(means, dtype=np.float64)
    nc = len(u)
    centers, rows, margins = np.empty((nc, d)), np.empty(nc, dtype=np.int64), np.empty(nc)
    dmin = np.full(n, np.inf)
    for c in range(nc):
        r = -1
        if c > 0:
            r, margin, _ = _pick(w * dmin, u[c])
        if r < 0:
            r, margin, _ = _pick(w, u[c])
        rows[c], margins[c] = r, margin
        centers[c] = np.where(np.isfinite(x[r]), x[r], g)
        dmin = np.minimum(dmin, distances(x, centers[c:c + 1], scale)[:, 0])
    return centers, rows, margins


def lloyd(x, w, n_clusters, u=None, n_iters=20, scale=None, start=None):
    """The loop of `Dataset.kmeans`: a dict with centers, labels, inertia, history, cluster_weights, n_iters_run, converged and
    min_gap (the smallest relative gap of any row with an observed entry over all the assignments made, the final one included)."""
    w = _w(x, w)
    centers = np.array(start, dtype=np.float64) if start is not None else seed(x, w, u, scale)[0]
    some = np.isfinite(x).any(axis=1)
    history, converged, min_gap = [], False, np.inf
    for _ in range(n_iters):
        _, _, tot, sums, inertia, dm = step(x, w, centers, scale)
        min_gap = min(min_gap, relative_gaps(dm)[some].min(initial=np.inf))
        history.append(inertia)
        new = new_centers(centers, tot, sums)
        if np.array_equal(new, centers):
            converged = True
            break
        centers = new
    labels, _, _, _, inertia, dm = step(x, w, centers, scale)
    min_gap = min(min_gap, relative_gaps(dm)[some].min(initial=np.inf))
    return dict(centers=centers, labels=labels, inertia=inertia, history=np.array(history),
                cluster_weights=np.bincount(labels, weights=w, minlength=n_clusters), n_iters_run=len(history), converged=converged,
                min_gap=float(min_gap))


def column_std_scale(x, w=None):
    """The scale of scale="std": 1 / the weighted standard deviation over the observed entries, 1 for a column without variance."""
    w = _w(x, w)
    mean = R.column_means(x, w)
    o = np.isfinite(x)
    tot = (w[:, None] * o).sum(0)
    var = np.where(tot > 0.0, (w[:, None] * np.where(o, x - mean, 0.0) ** 2).sum(0) / np.where(tot > 0.0, tot, 1.0), 0.0)
    return np.where(var > 0.0, 1.0 / np.sqrt(np.where(var > 0.0, var, 1.0)), 1.0)


def _cluster_moments(P, x, w, labels, n_clusters):
    """([PairwiseMoments of every cluster's rows around the cluster's own means, None for a cluster of weight 0], the whole dataset's,
    the log-weights: a cluster of weight 0 takes the weight of the lightest cluster that has some)."""
    w = _w(x, w)

    def pm(xs, ws):
        c = R.column_means(xs, ws)
        return P.PairwiseMoments(c, *R.moments(xs, ws, c))

    cw = np.bincount(labels, weights=w, minlength=n_clusters)
    moms = [pm(x[labels == c], w[labels == c]) if cw[c] > 0.0 else None for c in range(n_clusters)]
    cw = np.where(cw > 0.0, cw, cw[cw > 0.0].min())
    return moms, pm(x, w), np.log(cw / cw.sum())


def ppca_mix_start(P, x, w, labels, n_clusters, state_size):
    """`PPCAMix.from_kmeans` from host moments: P is the ppca_rs_amd module (its from_moments is host-side numpy)."""
    moms, whole, lw = _cluster_moments(P, x, w, labels, n_clusters)
    return P.PPCAMix([P.PPCAModel.from_moments(state_size, m if m is not None else whole) for m in moms], lw)


def fa_mix_start(P, x, w, labels, n_clusters, state_size):
    """`FAMix.from_kmeans` from host moments: (noise, transforms, means, log-weights); the shared noise pools the clusters' own,
    noise_j^2 = sum_c tot_cj noise_cj^2 / sum_c tot_cj, 1 where no cluster observes the column."""
    moms, whole, lw = _cluster_moments(P, x, w, labels, n_clusters)
    parts = [P.FAModel.from_moments(state_size, m if m is not None else whole) for m in moms]
    d = x.shape[1]
    num, den = np.zeros(d), np.zeros(d)
    for m, f in zip(moms, parts):
        if m is not None:
            tot = np.diag(m.counts)
            num += tot * f.noise ** 2
            den += tot
    noise = np.where(den > 0.0, np.sqrt(num / np.where(den > 0.0, den, 1.0)), 1.0)
    return noise, np.stack([f.transform for f in parts]), np.stack([f.mean for f in parts]), lw
