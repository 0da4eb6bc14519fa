"""Value buckets (include/ffm_engine.h "Value buckets") restated in numpy, for the tests that compare the library's
kernels, its host functions and the trainer CLI against it: the key and bin of a value's bit pattern, the
histogram (np.bincount), the edge rule in Python integers, the bucket (np.searchsorted), the mapping of a block."""
import numpy as np

BINS, MAX_EDGES, NAN_ID = 65536, 255, 65536


def np_key(val):
    """(key uint32, is_nan) of float32 values: -0.0 and +0.0 share a key, and the keys order as the values do."""
    u = np.ascontiguousarray(val, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    u = np.where((u & 0x7fffffff) == 0, 0, u)
    nan = (u & 0x7fffffff) > 0x7f800000
    key = np.where((u >> 31) != 0, ~u & 0xffffffff, u | 0x80000000)
    return key.astype(np.uint32), nan


def np_bin(val):
    """(bin int64, is_nan); a NaN's bin is meaningless."""
    key, nan = np_key(val)
    return (key >> np.uint32(16)).astype(np.int64), nan


def _fields(field, n, n_fields):
    if field is None:
        return np.arange(n, dtype=np.int64) % n_fields
    return np.asarray(field, np.int64).reshape(-1)


def np_hist(field, val, n_fields):
    """(counts uint64 [n_fields, BINS], n_valid, n_bad, n_nan): an entry counts iff 0 <= field < n_fields; a
    counting NaN adds to n_nan and to no bin."""
    b, nan = np_bin(val)
    fld = _fields(field, b.size, n_fields)
    ok = (fld >= 0) & (fld < n_fields)
    use = ok & ~nan
    counts = np.bincount(fld[use] * BINS + b[use], minlength=n_fields * BINS).astype(np.uint64).reshape(n_fields, BINS)
    return counts, int(ok.sum()), int(b.size - ok.sum()), int((ok & nan).sum())


def edges(counts, n_buckets):
    """The edge rule in Python integers: for j = 1 .. B - 1, t_j = (j N + B - 1) // B and e_j = the smallest bin
    whose inclusive cumulative count is >= t_j; repeats dropped.  (edges int64, number of repeats dropped)"""
    c = [int(x) for x in np.asarray(counts).reshape(-1)]
    assert len(c) == BINS and 2 <= n_buckets <= MAX_EDGES + 1
    n = sum(c)
    if n == 0:
        return np.zeros(0, np.int64), 0
    cum = np.cumsum(np.asarray(c, dtype=object))
    out, dropped = [], 0
    for j in range(1, n_buckets):
        t = (j * n + n_buckets - 1) // n_buckets
        lo, hi = 0, BINS - 1  # the smallest index with cum[index] >= t
        while lo < hi:
            mid = (lo + hi) // 2
            if cum[mid] >= t:
                hi = mid
            else:
                lo = mid + 1
        if out and out[-1] == lo:
            dropped += 1
        else:
            out.append(lo)
    assert all(a < b for a, b in zip(out, out[1:]))
    return np.asarray(out, np.int64), dropped


def np_bucket(edge, b):
    """bucket(bin) = the number of edges < bin."""
    return np.searchsorted(np.asarray(edge, np.int64), np.asarray(b, np.int64), "left")


def np_apply(field, feat, val, n_fields, buckets):
    """(feat' int32, val' float32, bucketed bool) of a block under the table buckets = {field: edges}: an entry with
    feat >= 0, 0 <= field < n_fields and a table for its field becomes (bucket, 1.0), a NaN (NAN_ID, 1.0); every other
    entry is untouched.  val None: every value is 1.0."""
    feat = np.asarray(feat, np.int32).reshape(-1)
    val = np.ones(feat.size, np.float32) if val is None else np.ascontiguousarray(val, np.float32).reshape(-1)
    fld = _fields(field, feat.size, n_fields)
    b, nan = np_bin(val)
    out_f, out_v, hit = feat.copy(), val.copy(), np.zeros(feat.size, bool)
    for f, e in buckets.items():
        m = (fld == f) & (feat >= 0) & (0 <= f < n_fields)
        out_f[m] = np.where(nan[m], NAN_ID, np_bucket(e, b[m])).astype(np.int32)
        out_v[m] = 1.0
        hit |= m
    return out_f, out_v, hit
