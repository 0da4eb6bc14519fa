"""Rare ids (include/ffm_engine.h "Rare ids") restated in numpy, for the tests that compare the library's
kernels, its host functions and the trainer CLI against it: the slot, the counts, the keep-map's words, the fold.
The hashed bits are sketch_ref's (hash_ref's mix)."""
import numpy as np

import sketch_ref

RARE_ID = 2 ** 31 - 1


def _fields(field, feat, n_fields):
    """The field of every entry as int64: 0 for LR / FM (n_fields == 0), p mod n_fields where none is given."""
    if n_fields == 0:
        return np.zeros(feat.shape, np.int64)
    if field is None:
        return np.arange(feat.size, dtype=np.int64) % n_fields
    return np.asarray(field, np.int64).reshape(-1)


def np_counting(field, feat, n_fields):
    """(counts mask, fields): an entry counts iff feat >= 0 and, with fields, 0 <= field < n_fields."""
    feat = np.asarray(feat, np.int64).reshape(-1)
    fld = _fields(field, feat, n_fields)
    ok = feat >= 0
    if n_fields > 0:
        ok &= (fld >= 0) & (fld < n_fields)
    return ok, fld


def np_slot(field, feat, bits):
    """slot = hashed bits >> (32 - bits), int64; field None: field 0."""
    feat = np.asarray(feat, np.int64).reshape(-1)
    fld = np.zeros(feat.shape, np.int64) if field is None else np.asarray(field, np.int64).reshape(-1)
    return (sketch_ref.np_hash_bits(fld, feat) >> np.uint64(32 - bits)).astype(np.int64)


def np_counts(field, feat, n_fields, bits, cap):
    """(min(count, cap) uint32 [2^bits], n_valid, n_bad)."""
    feat = np.asarray(feat, np.int64).reshape(-1)
    ok, fld = np_counting(field, feat, n_fields)
    cnt = np.bincount(np_slot(fld[ok], feat[ok], bits), minlength=1 << bits)
    return np.minimum(cnt, cap).astype(np.uint32), int(ok.sum()), int(feat.size - ok.sum())


def np_keep(counts, min_count):
    """(words uint64 [2^bits / 64], n_kept_slots, n_folded_entries) of counts already cut at a cap >= min_count."""
    counts = np.asarray(counts, np.int64)
    keep = counts >= min_count
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    words = (keep.reshape(-1, 64).astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64)
    return words, int(keep.sum()), int(counts[~keep].sum())


def np_fold(field, feat, n_fields, bits, words):
    """The raw ids after the fold (int32): RARE_ID where a counting entry's bit is 0."""
    feat = np.asarray(feat, np.int64).reshape(-1)
    ok, fld = np_counting(field, feat, n_fields)
    slot = np_slot(np.where(ok, fld, 0), np.where(ok, feat, 0), bits)
    words = np.asarray(words, np.uint64)
    bit = (words[slot >> 6] >> (slot & 63).astype(np.uint64)) & np.uint64(1)
    return np.where(ok & (bit == 0), RARE_ID, feat).astype(np.int32)
