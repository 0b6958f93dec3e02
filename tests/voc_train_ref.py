"""Sequential NumPy restatement of DBoW2's TemplatedVocabulary::create (TemplatedVocabulary.h:
558-587 create, 642-819 HKmeansStep, 833-913 initiateClustersKMpp, 918-996 createWords and
setNodeWeights; FORB.cpp:28-116 meanValue, distance, toString) and of saveToTextFile (1429-1449),
with the choices DESIGN.md section 2 pins: the per-node counter random stream, an emptied cluster
keeps its centre, the iteration cap.

It is recursive and depth-first, one node at a time, as the reference: not the level-batched
order of the product.  The GPU tests require the product's tree to equal this one byte for byte.
"""
import numpy as np

RAND_MAX = 2147483647
M64 = (1 << 64) - 1
POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def mix(x):
    """splitmix64's output function."""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(key, j):
    """Draw j of the node with this key: a value in [0, RAND_MAX] in rand()'s place."""
    return mix((key + j) & M64) >> 33


def child_key(key, c):
    return mix(key ^ (c + 1))


def random_int(r, n):
    """DUtils::Random::RandomInt(0, n - 1) from the draw r."""
    return int(np.float64(r) / (np.float64(RAND_MAX) + 1.0) * np.float64(n))


def random_value(r, dist_sum):
    """DUtils::Random::RandomValue<double>(0, dist_sum) from the draw r."""
    return np.float64(r) / np.float64(RAND_MAX) * np.float64(dist_sum)


def distance(D, c):
    """FORB::distance of every row of D (n x 32 uint8) to the descriptor c."""
    return POP8[np.bitwise_xor(D, c[None, :])].sum(axis=1)


def mean_value(D):
    """FORB::meanValue of the rows of D (at least one): bit set where count >= n/2 + n%2."""
    n = len(D)
    if n == 1:
        return D[0].copy()
    s = np.unpackbits(D, axis=1).astype(np.int64).sum(axis=0)
    return np.packbits(s >= n // 2 + n % 2)


def pick_prefix(min_dist, cut_d):
    """The first index whose inclusive prefix sum of min_dist is >= cut_d, else the last."""
    up = np.cumsum(np.asarray(min_dist, np.float64))
    hit = np.nonzero(up >= cut_d)[0]
    return int(hit[0]) if len(hit) else len(up) - 1


def assign(D, clusters):
    """Nearest centre per row, strict <: the first of equal centres wins."""
    d = np.stack([distance(D, c) for c in clusters], axis=1)
    return np.argmin(d, axis=1)


def seed_clusters(D, k, key):
    """initiateClustersKMpp over the node's features D (in order) with the node's draws."""
    j = 0
    clusters = [D[random_int(draw(key, j), len(D))].copy()]
    j += 1
    min_d = distance(D, clusters[0])
    while len(clusters) < k:
        min_d = np.minimum(min_d, distance(D, clusters[-1]))
        dist_sum = int(min_d.sum())
        if dist_sum <= 0:
            break
        while True:
            cut_d = random_value(draw(key, j), dist_sum)
            j += 1
            if cut_d != 0.0:
                break
        clusters.append(D[pick_prefix(min_d, cut_d)].copy())
    return clusters


def kmeans_node(D, k, key, max_iters):
    """The k-means branch of HKmeansStep: -> (clusters, association, passes, capped)."""
    clusters = seed_clusters(D, k, key)
    last = None
    passes = 0
    while True:
        passes += 1
        if last is not None:
            for c in range(len(clusters)):
                members = D[last == c]
                if len(members):  # pinned: an empty cluster keeps its centre
                    clusters[c] = mean_value(members)
        cur = assign(D, clusters)
        if last is not None and np.array_equal(cur, last):
            return clusters, cur, passes, False
        last = cur
        if passes >= max_iters:
            return clusters, cur, passes, True


class Tree:
    def __init__(self, k, L, weighting, scoring):
        self.k, self.L, self.weighting, self.scoring = k, L, weighting, scoring
        self.parent = [-1]
        self.children = [[]]
        self.desc = [np.zeros(32, np.uint8)]
        self.weight = [0.0]
        self.iters = [0] * L
        self.n_kmeans_nodes = self.n_capped = self.n_empty_clusters = 0

    @property
    def n_nodes(self):
        return len(self.parent)

    def leaf(self, i):
        return not self.children[i]

    def words(self):
        return [i for i in range(1, self.n_nodes) if self.leaf(i)]


def _hk_step(t, D, parent_id, idx, level, key, max_iters):
    F = D[idx]
    if len(idx) <= t.k:
        clusters = [f.copy() for f in F]
        groups = [idx[i:i + 1] for i in range(len(idx))]
    else:
        clusters, a, passes, capped = kmeans_node(F, t.k, key, max_iters)
        groups = [idx[a == c] for c in range(len(clusters))]
        t.n_kmeans_nodes += 1
        t.n_capped += bool(capped)
        t.n_empty_clusters += sum(1 for g in groups if len(g) == 0)
        t.iters[level - 1] = max(t.iters[level - 1], passes)
    ids = []
    for c in clusters:
        ids.append(t.n_nodes)
        t.parent.append(parent_id)
        t.children.append([])
        t.desc.append(c)
        t.weight.append(0.0)
        t.children[parent_id].append(ids[-1])
    if level < t.L:
        for c, g in enumerate(groups):
            if len(g) > 1:
                _hk_step(t, D, ids[c], g, level + 1, child_key(key, c), max_iters)


def transform_words(t, D):
    """TemplatedVocabulary::transform(feature, word_id) of every row: the node id of its word."""
    out = np.zeros(len(D), np.int64)

    def descend(node, idx):
        ch = t.children[node]
        if not ch:
            out[idx] = node
            return
        a = assign(D[idx], [t.desc[c] for c in ch])
        for i, c in enumerate(ch):
            sel = idx[a == i]
            if len(sel):
                descend(c, sel)

    if len(D) and t.children[0]:
        descend(0, np.arange(len(D)))
    return out


def set_node_weights(t, descs_per_image):
    words = t.words()
    if t.weighting in (1, 3):  # TF, BINARY
        for w in words:
            t.weight[w] = 1.0
        return
    ni = {w: 0 for w in words}
    for d in descs_per_image:
        for w in np.unique(transform_words(t, np.asarray(d, np.uint8).reshape(-1, 32))):
            ni[int(w)] += 1
    ndocs = len(descs_per_image)
    for w in words:
        if ni[w] > 0:
            t.weight[w] = float(np.log(np.float64(ndocs) / np.float64(ni[w])))


def create(descs_per_image, k, L, weighting=0, scoring=0, seed=0, max_iters=0):
    """create(training_features, k, L, weighting, scoring) -> Tree."""
    imgs = [np.asarray(d, np.uint8).reshape(-1, 32) for d in descs_per_image]
    D = np.concatenate(imgs)
    t = Tree(k, L, weighting, scoring)
    _hk_step(t, D, 0, np.arange(len(D)), 1, mix(seed), max_iters if max_iters > 0 else 1000)
    set_node_weights(t, imgs)
    return t


def save_text(t, path):
    """saveToTextFile: the double space of the header, FORB::toString's space after every byte,
    the weight as ostream << double prints it, endl after every line."""
    with open(path, "w") as f:
        f.write("%d %d  %d %d\n" % (t.k, t.L, t.scoring, t.weighting))
        for i in range(1, t.n_nodes):
            f.write("%d %d " % (t.parent[i], 1 if t.leaf(i) else 0))
            f.write("".join("%d " % b for b in t.desc[i]))
            f.write(" %g\n" % t.weight[i])


def read_text(path):
    """The saved file as comparable pieces: header, parents, leaf flags, descriptors (n x 32) and
    the weights as printed."""
    lines = open(path).read().split("\n")
    assert lines[-1] == "", "the file ends with endl"
    head = lines[0]
    rows = [ln.split() for ln in lines[1:-1]]
    parent = np.array([int(r[0]) for r in rows], np.int64)
    leaf = np.array([int(r[1]) for r in rows], np.int64)
    desc = np.array([[int(v) for v in r[2:34]] for r in rows], np.uint8).reshape(-1, 32)
    weight = [r[34] for r in rows]
    return head, parent, leaf, desc, weight
