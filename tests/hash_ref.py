"""The id mapping of FFM_FLAG_HASH_IDS (include/ffm_engine.h "Hashed ids") restated in numpy, for the
tests that compare the library's host function, its kernels and the trainer CLI against it."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def np_hash_ids(field, feat, n_feats, n_fields=1, field_start=None, ffm=True):
    """id' per entry; field may be None (LR / FM, or FFM rows of one entry per field in field order)."""
    feat = np.asarray(feat, np.int64)
    if not ffm:
        fld = np.zeros(feat.shape, np.int64)
    elif field is None:
        fld = np.arange(feat.size, dtype=np.int64).reshape(feat.shape) % n_fields
    else:
        fld = np.asarray(field, np.int64)
    salt = ((fld + 1).astype(np.uint64) * np.uint64(0x9e3779b9)) & M32   # (wraps like uint32; negative fields too)
    x = (feat.astype(np.uint64) & M32) ^ salt
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85ebca6b)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xc2b2ae35)) & M32
    x ^= x >> np.uint64(16)
    erased = feat < 0
    if ffm:
        erased |= (fld < 0) | (fld >= n_fields)
    if ffm and field_start is not None:
        fs = np.asarray(field_start, np.int64)
        f_ok = np.where(erased, 0, fld)
        lo, width = fs[f_ok], fs[f_ok + 1] - fs[f_ok]
    else:
        lo, width = np.zeros(feat.shape, np.int64), np.full(feat.shape, n_feats, np.int64)
    out = lo + ((x * width.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    return np.where(erased, -1, out).astype(np.int32)
