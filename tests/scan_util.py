"""Helpers of the changed-feature scan and sparse checkpoint tests: the predicate restated in numpy and
the create-time state of an engine, from ffm_engine_init_weights_host."""
import numpy as np

import ftrl_ffm_amd as fa
from oracle.pyoracle import Csr
from util import bits


def fresh_state(model_type, n_feats, row_len, seed, mean, stddev, skip_init=False):
    """What ffm_engine_create stores: zero (n, z) and bias, w drawn per logical index (zero under
    skip_init)."""
    nf, L = int(n_feats), int(row_len)
    st = dict(bias3=np.zeros(3, np.float32), lin_n=np.zeros(nf, np.float32), lin_z=np.zeros(nf, np.float32),
              vec_n=np.zeros((nf, L), np.float32), vec_z=np.zeros((nf, L), np.float32))
    if skip_init:
        st["lin_w"], st["vec_w"] = np.zeros(nf, np.float32), np.zeros((nf, L), np.float32)
    else:
        st["lin_w"] = fa.init_weights_host(seed, mean, stddev, 0, 0, nf)
        st["vec_w"] = fa.init_weights_host(seed, mean, stddev, 1, 0, nf * L).reshape(nf, L)
    return st


def expected_changed(st, fresh):
    """Ascending ids of the features of state `st` that differ from `fresh` in any 32-bit pattern."""
    ch = np.zeros(st["lin_w"].shape[0], bool)
    for key in ("lin_w", "lin_n", "lin_z"):
        ch |= bits(st[key]) != bits(fresh[key])
    if st["vec_w"].shape[1]:
        for key in ("vec_w", "vec_n", "vec_z"):
            ch |= (bits(st[key]) != bits(fresh[key])).any(axis=1)
    return np.flatnonzero(ch).astype(np.int32)


def without_fields(blk):
    """The block for LR / FM: same rows, field 0 everywhere."""
    return Csr(blk.row_ptr.copy(), np.zeros_like(blk.field), blk.feat.copy(), blk.val.copy(), blk.label.copy())
