"""numpy transcription of the eval_metrics semantics (tf.nn.in_top_k), shared by test_eval.py and
test_eval_gpu.py: plain loops and np.isfinite, no top-k routine of any library.

For each row, t = logits[row][label]:
  * label < 0: a padding row -- skipped, not an example;
  * label >= ncls: an example and a miss (the row is not read);
  * otherwise a top-k hit iff t is finite and #{c < ncls : logits[row][c] > t} < k
    (ties across the boundary count as inside; a NaN compares as not greater).
Columns ncls .. ld-1 are padding and never read as classes."""
import numpy as np


def eval_ref(logits, labels, ncls):
    """(examples, top1_hits, top5_hits) as Python ints."""
    logits = np.asarray(logits, dtype=np.float32)
    labels = np.asarray(labels).reshape(-1)
    logits = logits.reshape(labels.shape[0], -1)
    ex = h1 = h5 = 0
    for r in range(labels.shape[0]):
        lab = int(labels[r])
        if lab < 0:
            continue
        ex += 1
        if lab >= ncls:
            continue
        t = logits[r, lab]
        if not np.isfinite(t):
            continue
        above = 0
        for c in range(ncls):
            if logits[r, c] > t:  # False for a NaN on either side
                above += 1
        h1 += above < 1
        h5 += above < 5
    return int(ex), int(h1), int(h5)


def make_case(B, ncls, seed=0, pad_fill=3e38):
    """Random logits [B, ld] (ld = ncls rounded up to 8, padding columns = pad_fill) and labels
    of which about 10 % are -1 and one (when B > 1) is >= ncls, with the edge rows of the
    semantics planted where the shape has room for them. Returns (logits fp32, labels int64)."""
    rng = np.random.RandomState(seed + 1000 * B + ncls)
    ld = (ncls + 7) // 8 * 8
    lg = rng.standard_normal((B, ld)).astype(np.float32)
    lg[:, ncls:] = pad_fill
    lab = rng.randint(0, ncls, size=B).astype(np.int64)
    lab[rng.rand(B) < 0.1] = -1
    if B == 1:  # the single row stays a plain random one
        lab[0] = abs(lab[0])
        return lg, lab
    rows = list(range(B))

    def take():
        return rows.pop(0) if rows else None

    lab[take()] = ncls + 2  # out of range: an example, a miss, nothing read
    if ncls >= 7:
        r = take()
        if r is not None:  # six equal maxima that include the target: a hit at k=1 and k=5
            lab[r] = 2
            lg[r, :ncls] = -1.0
            lg[r, [0, 2, 3, 4, 5, 6]] = 7.5
        r = take()
        if r is not None:  # target ties for ranks 5 and 6: four above, one equal -> hit at k=5 only
            lab[r] = 1
            lg[r, :ncls] = -2.0
            lg[r, [0, 2, 3, 4]] = 9.0
            lg[r, [1, 5]] = 4.0
        r = take()
        if r is not None:  # five strictly above the target: a miss
            lab[r] = ncls - 1
            lg[r, :ncls] = -3.0
            lg[r, [0, 1, 2, 3, 4]] = 1.0
            lg[r, ncls - 1] = 0.5
    for bad in (np.nan, np.inf, -np.inf):  # non-finite targets: misses
        r = take()
        if r is not None:
            lab[r] = ncls // 2
            lg[r, ncls // 2] = bad
    r = take()
    if r is not None and ncls >= 2:  # a NaN in a non-target column does not count as greater
        lab[r] = 0
        lg[r, :ncls] = -1.0
        lg[r, 0] = 0.0
        lg[r, 1] = np.nan
    return lg, lab
