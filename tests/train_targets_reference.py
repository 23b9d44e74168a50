"""numpy twins of the training targets of azx_set_train_targets (include/azx.h has the definition), for the tests:
the visit-share policy row and the z/q-blended reward, in float32 as the kernels compute them."""
import numpy as np


def visit_rows(counts):
    """row[j] = counts[j] / sum(counts): ONE float32 IEEE division of integers held in float32 (the sum is exact below
    2^24).  `counts` is [k] or [rows, k]; an all-zero row stays all zero (the kernel writes the reference row then)."""
    n = np.asarray(counts, np.float32)
    total = n.sum(-1, keepdims=True, dtype=np.float32)
    out = np.zeros_like(n)
    np.divide(n, total, out=out, where=total > 0)
    return out


def blend(z, v, mix):
    """reward = (1 - mix) * z + mix * v in float32: two products and one sum, unfused.  z itself where v is not finite
    or mix is 0 (no arithmetic)."""
    z = np.asarray(z, np.float32)
    v = np.asarray(v, np.float32)
    mix = np.float32(mix)
    if not mix > 0:
        return z.copy()
    with np.errstate(invalid="ignore"):
        mixed = ((np.float32(1.0) - mix) * z).astype(np.float32) + (mix * v).astype(np.float32)
    return np.where(np.isfinite(v), mixed.astype(np.float32), z).astype(np.float32)


def recover_counts(row, k, mean_visits):
    """The root children's visit counts of a visit-share row: S = mean_visits * k (row metric 4 times the row's k),
    n_j = rint(row_j * S).  Returns (n int64[k], S int)."""
    S = int(np.rint(np.float64(mean_visits) * k))
    n = np.rint(np.asarray(row[:k], np.float64) * S).astype(np.int64)
    return n, S
