"""CPU restatement of the embedding-instance contract (maskunet_amd.instances_from_embeddings, mu_dbscan_instances), brute force in
float64 numpy, plus the input builders that the host and the GPU tests share.  Written from the contract, not from the kernels.

Per image, for every class c with 1 <= c < num_classes in ascending order (every other value is background):
  - points: the pixels of class c in raster order, D embedding values each;
  - i ~ j (neighbours) iff sum_k (double(a_k) - double(b_k))^2 <= double(float32(eps))^2; a point is its own neighbour;
  - core: at least min_samples neighbours, itself included;
  - clusters: the connected components of the core points under ~, ordered by their lowest core point;
  - a non-core point with a core neighbour belongs to the first cluster (in that order) that holds one; the others are noise: id 0;
  - ids run 1..count over (class ascending, cluster order);
  - table row k-1 = class, area, x_min, y_min, x_max, y_max, first_pixel (the lowest pixel of the instance, y*W+x), class_rank;
    score = 1.0; order = ascending id; table / score / order hold ids 1..min(count, max_instances), the rest is 0.
"""
import numpy as np

from tests._instances_reference import table_from_ids


def neighbours(X, eps):
    """X [n,D] -> bool [n,n]"""
    X = np.asarray(X, np.float64)
    d2 = np.zeros((len(X), len(X)), np.float64)
    for k in range(X.shape[1]):
        d = X[:, k, None] - X[None, :, k]
        d2 += d * d
    return d2 <= float(np.float32(eps)) ** 2, d2


def cluster_points(X, eps, min_samples):
    """X [n,D] -> (label [n] int: -1 noise, else the cluster number 0.. in order of the lowest core point; core [n] bool; nb)"""
    n = len(X)
    nb, _ = neighbours(X, eps)
    core = nb.sum(1) >= min_samples
    label = np.full(n, -1, np.int64)
    k = 0
    for i in range(n):
        if not core[i] or label[i] >= 0:
            continue
        label[i] = k
        stack = [i]
        while stack:
            a = stack.pop()
            for j in np.nonzero(nb[a] & core & (label < 0))[0]:
                label[j] = k
                stack.append(j)
        k += 1
    for i in np.nonzero(~core)[0]:
        near = nb[i] & core
        if near.any():
            label[i] = label[near].min()
    return label, core, nb


def label_image(cls, emb, num_classes, eps=0.5, min_samples=5):
    """cls [H,W] ints, emb [H,W,D] -> ids [H,W] int32"""
    H, W = cls.shape
    flat = np.asarray(cls).reshape(-1)
    E = np.asarray(emb, np.float64).reshape(H * W, -1)
    ids = np.zeros(H * W, np.int32)
    nxt = 1
    for c in range(1, num_classes):
        pix = np.nonzero(flat == c)[0]
        if len(pix) == 0:
            continue
        label, _, _ = cluster_points(E[pix], eps, min_samples)
        ids[pix[label >= 0]] = nxt + label[label >= 0]
        nxt += int(label.max()) + 1
    return ids.reshape(H, W)


def instances(cls, emb, num_classes, eps=0.5, min_samples=5, max_instances=1024):
    """cls [B,H,W] ints, emb [B,H,W,D] -> dict of ids, count, table, score, order (the outputs of mu_dbscan_instances)"""
    cls = np.asarray(cls)
    ids = np.zeros(cls.shape, np.int32)
    classes = []
    for b in range(cls.shape[0]):
        ids[b] = label_image(cls[b], emb[b], num_classes, eps, min_samples)
        found, first = np.unique(ids[b], return_index=True)                  # the first pixel of every id, ascending
        classes.append(cls[b].reshape(-1)[first[found > 0]])
    return {"ids": ids, **table_from_ids(ids, classes, max_instances)}


def annotations(ids, cls):
    """get_instance_annotations without the RLE: (bbox, category_id, score) per id, ascending"""
    out = []
    for k in range(1, int(ids.max()) + 1):
        ys, xs = np.nonzero(ids == k)
        out.append(([float(xs.min()), float(ys.min()), float(xs.max() - xs.min()), float(ys.max() - ys.min())],
                    int(np.median(cls[ids == k])), 1.0))
    return out


def rule_coverage(cls, emb, num_classes, eps=0.5, min_samples=5):
    """which rules of the contract one image exercises"""
    flat = np.asarray(cls).reshape(-1)
    E = np.asarray(emb, np.float64).reshape(len(flat), -1)
    cov = {"noise": False, "small_class": False, "two_clusters": False, "shared_border": False, "root_not_first": False}
    for c in range(1, num_classes):
        pix = np.nonzero(flat == c)[0]
        if len(pix) == 0:
            continue
        if len(pix) < min_samples:
            cov["small_class"] = True
        label, core, nb = cluster_points(E[pix], eps, min_samples)
        cov["noise"] |= bool((label < 0).any())
        cov["two_clusters"] |= bool(label.max() >= 1)
        for i in np.nonzero(~core)[0]:
            if len(set(label[nb[i] & core].tolist())) >= 2:
                cov["shared_border"] = True
        for k in range(int(label.max()) + 1):
            if not core[np.nonzero(label == k)[0][0]]:
                cov["root_not_first"] = True              # the cluster's first pixel is a border point
    return cov


def margin(cls, emb, num_classes, eps=0.5):
    """min over same-class pairs of |d^2 - eps^2| / eps^2 (float64)"""
    flat = np.asarray(cls).reshape(-1)
    E = np.asarray(emb, np.float64).reshape(len(flat), -1)
    e2 = float(np.float32(eps)) ** 2
    m = np.inf
    for c in range(1, num_classes):
        pix = np.nonzero(flat == c)[0]
        if len(pix) > 1:
            m = min(m, float(np.abs(neighbours(E[pix], eps)[1] - e2).min() / e2))
    return m


# ------------------------------------------------------------------------------------------------
# input builders
def class_map(rng, H, W, sizes):
    """int32 [H,W]: class c+1 on sizes[c] random pixels, 0 elsewhere (so the points of a class are scattered in raster order)"""
    assert sum(sizes) <= H * W
    flat = np.zeros(H * W, np.int32)
    where = rng.permutation(H * W)
    at = 0
    for c, n in enumerate(sizes):
        flat[where[at:at + n]] = c + 1
        at += n
    return flat.reshape(H, W)


def dumbbell(D):
    """19 points: two tight blobs of 8 with one arm point each, 0.9 apart, and ONE point midway (0.45 from each arm, 3 neighbours with
    itself: not core with min_samples = 5) -- a border point with core neighbours in two clusters.  The midway point comes first."""
    u = np.zeros(D)
    u[0] = 1.0
    pts = [0.85 * u]
    t = np.linspace(-1, 1, 8)
    for centre, arm in ((0.0, 0.4), (1.7, 1.3)):
        for s in t:
            p = centre * u
            p[-1] += 0.01 * s
            pts.append(p)
        pts.append(arm * u)
    return np.asarray(pts)


def clustered(rng, n, D, centres=3, sigma=0.075):
    """n points around `centres` random centres ~1.5 apart; sigma sets the density: with D = 16, eps = 0.5 the typical in-cluster
    distance is sigma * sqrt(2 D) = 0.42, so core, border and noise points all occur"""
    c = rng.standard_normal((centres, D))
    c *= 1.5 / np.sqrt(2 * D) * np.sqrt(D) / np.linalg.norm(c, axis=1, keepdims=True) * np.sqrt(2)
    which = rng.integers(0, centres, n)
    return c[which] + sigma * np.sqrt(16.0 / D) * rng.standard_normal((n, D))


def clustered_case(seed, H, W, D, sizes, dtype=np.float32):
    """(cls [H,W] int32, emb [H,W,D] dtype): class 1 holds a dumbbell among clustered points, the other classes are clustered; a class
    of fewer than 10 points is one tight blob (one cluster from min_samples points on, all noise below: the rule, not the distances)"""
    rng = np.random.default_rng(seed)
    cls = class_map(rng, H, W, sizes)
    emb = (0.1 * rng.standard_normal((H * W, D))).astype(dtype)          # background: never read into a result
    flat = cls.reshape(-1)
    for c, n in enumerate(sizes):
        pix = np.nonzero(flat == c + 1)[0]
        X = (clustered(rng, n, D) if n >= 10 else 0.01 * rng.standard_normal((n, D))) + 3.0
        if c == 0 and n >= 19:
            X[:19] = dumbbell(D) - 3.0 + 0.001 * rng.standard_normal((19, D))
        emb[pix] = X.astype(dtype)
    return cls, emb.reshape(H, W, D)


def grid_case(seed, H, W, D, sizes, span=12):
    """coordinates on multiples of 1/8 in a small box: d^2 is exact in fp16 / fp32 / fp64 and many pairs sit exactly at d = eps = 0.5"""
    rng = np.random.default_rng(seed)
    cls = class_map(rng, H, W, sizes)
    emb = rng.integers(0, span, (H, W, D)).astype(np.float32) / 8.0
    if D > 2:
        emb[..., 2:] = rng.integers(0, 2, (H, W, D - 2)) / 8.0 * (rng.random((H, W, D - 2)) < 0.15)
    return cls, emb
