"""Field sketches (include/ffm_engine.h "Field sketches") restated in numpy and Python integers, for the tests
that compare the library's kernel, its host functions and the trainer CLI against it.  The mix is hash_ref's."""
import math

import numpy as np

import hash_ref

BITS = 14
REGS = 1 << BITS


def np_hash_bits(field, feat):
    """The 32 hashed bits of every entry (uint64 array holding uint32 values): what hash_ref scales, with width 2^32."""
    # id' = (x * width) >> 32 with one range of width 2^32 is x itself (the int32 the mapping returns, unsigned again)
    ids = hash_ref.np_hash_ids(np.asarray(field, np.int64), np.asarray(feat, np.int64), 1 << 32, n_fields=1 << 31)
    return ids.astype(np.int64).astype(np.uint64) & hash_ref.M32


def unmix32(x):
    """The inverse of the mix (Python int): the y with mix32(y) == x."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * pow(0xc2b2ae35, -1, 1 << 32)) & 0xFFFFFFFF
    x ^= x >> 13
    x ^= x >> 26
    x = (x * pow(0x85ebca6b, -1, 1 << 32)) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def feat_for_bits(field, x):
    """The raw id (as a signed 32-bit value) whose hashed bits under `field` are x."""
    y = unmix32(x) ^ (((field + 1) * 0x9e3779b9) & 0xFFFFFFFF)
    return y - (1 << 32) if y >= 1 << 31 else y


def ranks(x):
    """(idx, rank) of hashed bits x."""
    x = np.asarray(x, np.uint64)
    idx = (x >> np.uint64(32 - BITS)).astype(np.int64)
    w = (x << np.uint64(BITS)) & hash_ref.M32
    # clz32(w) + 1 = 32 - bit_length(w) + 1; bit_length through an exact integer log2 on float64 (w < 2^32)
    bl = np.zeros(w.shape, np.int64)
    nz = w != 0
    bl[nz] = np.floor(np.log2(w[nz].astype(np.float64))).astype(np.int64) + 1
    rank = np.where(nz, 33 - bl, 33 - BITS)
    return idx, rank.astype(np.int64)


def np_sketch(field, feat, n_fields):
    """(reg uint8 [n_fields, REGS], n_valid, n_bad); field None: entry p is field p mod n_fields."""
    feat = np.asarray(feat, np.int64).reshape(-1)
    fld = np.arange(feat.size, dtype=np.int64) % n_fields if field is None else np.asarray(field, np.int64).reshape(-1)
    ok = (feat >= 0) & (fld >= 0) & (fld < n_fields)
    reg = np.zeros((n_fields, REGS), np.uint8)
    idx, rank = ranks(np_hash_bits(fld[ok], feat[ok]))
    np.maximum.at(reg, (fld[ok], idx), rank.astype(np.uint8))
    return reg, int(ok.sum()), int(feat.size - ok.sum())


def np_estimate(reg):
    """Distinct ids per field, float64."""
    reg = np.asarray(reg, np.uint8)
    M = float(REGS)
    alpha = 0.7213 / (1.0 + 1.079 / M)
    out = np.zeros(reg.shape[0], np.float64)
    for f in range(reg.shape[0]):
        s = 0.0
        for r, c in zip(*np.unique(reg[f], return_counts=True)):  # (exact in double in any order)
            s += float(c) * 2.0 ** -int(r)
        v = int((reg[f] == 0).sum())
        e = alpha * M * M / s
        if e <= 2.5 * M and v > 0:
            e = M * math.log(M / v)
        out[f] = 0.0 if v == REGS else e
    return out


def np_field_ranges(count, n_feats):
    """field_start as a list of Python ints (the header's rule); ValueError where the library refuses."""
    count = [int(c) for c in count]
    F = len(count)
    if F <= 0 or n_feats < 2 * F or any(c < 0 for c in count):
        raise ValueError("refused")
    count = [min(max(c, 1), 1 << 31) for c in count]
    base = min(4096, n_feats // (2 * F))
    R = n_feats - F * base
    C = sum(count)
    width = [base + (R * c) // C for c in count]
    rem = [(R * c) % C for c in count]
    left = n_feats - sum(width)
    for f in sorted(range(F), key=lambda f: (-rem[f], f))[:left]:
        width[f] += 1
    start = [0]
    for w in width:
        start.append(start[-1] + w)
    return start
