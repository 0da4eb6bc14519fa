"""Field sketches on the device (include/ffm_engine.h "Field sketches"): field_sketch_kernel's registers, n_valid and
n_bad compared EXACTLY with their numpy restatement (tests/sketch_ref.py) -- vector and tail paths, one lane, more
than two grid strides, the staging chunks of a pageable call; entries that do not count; rows without a field array;
ids built for chosen ranks; a hot id; any order and batching; pageable, page-locked and device inputs; halves; and a
sketch beside an engine on the same device."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
import sketch_ref

pytestmark = pytest.mark.gpu

GRID_LANES = 24 * 256  # the kernel's lanes when it reads host memory: each carries four entries per stride
NNZ = (0, 1, 3, 4, 5, 1027, 2 * GRID_LANES * 4 + 5)


def entries(nnz, n_fields, seed):
    """Random entries with everything that must not count mixed in, and the two ends of the id range."""
    rng = np.random.default_rng(seed)
    field = rng.integers(0, n_fields, size=nnz, dtype=np.int64)
    feat = rng.integers(0, 2 ** 31, size=nnz, dtype=np.int64)
    kind = rng.integers(0, 16, size=nnz)
    field[kind == 0] = -1
    field[kind == 1] = n_fields
    feat[kind == 2] = -1
    feat[kind == 3] = -2 ** 31
    feat[kind == 4] = 0
    feat[kind == 5] = 2 ** 31 - 1
    feat[kind == 6] = rng.integers(0, 50, size=int((kind == 6).sum()))  # repeats
    return field.astype(np.int32), feat.astype(np.int32)


def pinned_copy(a):
    """a in page-locked memory of its own (None stays None); release with unpin."""
    if a is None:
        return None
    p = fa.page_aligned(max(1, a.size), np.int32)
    p[:a.size] = a
    assert fa.load_library().ffm_engine_pin_host(p.ctypes.data, max(1, p.size) * 4) == 0
    return p


def unpin(p):
    if p is not None:
        assert fa.load_library().ffm_engine_unpin_host(p.ctypes.data) == 0


def feed(sk, field, feat, how):
    n = feat.size
    if how == "pageable":
        sk.add(field, feat)
    elif how == "zero_copy":
        pf, pi = pinned_copy(field), pinned_copy(feat)
        try:
            sk.add(None if pf is None else pf[:n], pi[:n], zero_copy=True)
        finally:
            unpin(pf)
            unpin(pi)
    elif how == "zero_copy_unaligned":  # the arrays start 4 bytes into their pages: entry by entry, no 16-byte loads
        pf = None if field is None else pinned_copy(np.concatenate([[0], field]).astype(np.int32))
        pi = pinned_copy(np.concatenate([[0], feat]).astype(np.int32))
        try:
            sk.add(None if pf is None else pf[1:n + 1], pi[1:n + 1], zero_copy=True)
        finally:
            unpin(pf)
            unpin(pi)
    elif how == "device":
        df = None if field is None else torch.from_numpy(np.ascontiguousarray(field)).cuda()
        di = torch.from_numpy(np.ascontiguousarray(feat)).cuda()
        torch.cuda.synchronize()
        sk.add_device(n, None if df is None else df.data_ptr(), di.data_ptr() if n else None)
        sk.read()  # (waits for the sketch's stream before the tensors go)
    else:
        raise ValueError(how)


def gpu_sketch(n_fields, field, feat, how="pageable"):
    sk = fa.FieldSketch(n_fields)
    try:
        feed(sk, field, feat, how)
        return sk.read()
    finally:
        sk.close()


def assert_same(got, want, what):
    reg, nv, nb = got
    wreg, wnv, wnb = want
    assert (nv, nb) == (wnv, wnb), (what, nv, nb, wnv, wnb)
    assert reg.dtype == np.uint8 and reg.shape == wreg.shape
    bad = np.argwhere(reg != wreg)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("n_fields", [1, 8, 65])
def test_registers_and_counters_are_exact(n_fields):
    for nnz in NNZ:
        field, feat = entries(nnz, n_fields, seed=1000 * n_fields + nnz % 997)
        want = sketch_ref.np_sketch(field, feat, n_fields)
        if nnz >= 1027:
            assert want[2] > 0 and want[1] > 0 and want[0].max() >= 5
        for how in ("pageable", "zero_copy") if nnz != 1027 else ("pageable", "zero_copy", "zero_copy_unaligned", "device"):
            assert_same(gpu_sketch(n_fields, field, feat, how), want, (n_fields, nnz, how))


def test_fresh_sketch_is_empty_and_keeps_counting_after_a_read():
    sk = fa.FieldSketch(3)
    reg, nv, nb = sk.read()
    assert not reg.any() and (nv, nb) == (0, 0) and reg.shape == (3, sketch_ref.REGS)
    assert (sk.estimate() == 0.0).all()
    field, feat = entries(501, 3, seed=5)
    sk.add(field[:200], feat[:200])
    first = sk.read()
    assert_same(first, sketch_ref.np_sketch(field[:200], feat[:200], 3), "first part")
    sk.add(field[200:], feat[200:])
    assert_same(sk.read(), sketch_ref.np_sketch(field, feat, 3), "both parts")
    est = sk.estimate()
    assert np.array_equal(est, fa.sketch_estimate(sk.read()[0]))
    sk.close()
    sk.close()  # (twice is fine)


@pytest.mark.parametrize("n_fields,nnz", [(8, 8 * 1000), (8, 8 * 1000 + 5), (65, 65 * 77), (65, 65 * 77 + 3), (8, 5), (65, 3), (1, 1027)])
def test_rows_without_a_field_array(n_fields, nnz):
    _, feat = entries(nnz, n_fields, seed=nnz)
    want = sketch_ref.np_sketch(None, feat, n_fields)
    spelled = sketch_ref.np_sketch(np.arange(nnz) % n_fields, feat, n_fields)
    assert_same(want, spelled, "the reference's own convention")
    for how in ("pageable", "zero_copy", "zero_copy_unaligned", "device"):
        assert_same(gpu_sketch(n_fields, None, feat, how), want, (n_fields, nnz, how))


def test_pageable_call_longer_than_a_staging_chunk():
    """A pageable call is staged in chunks of 2^22 entries; without a field array the second chunk's fields go on
    where the first one's stopped (2^22 mod 7 = 2), with one both chunks' entries land where they belong."""
    nnz, F = (1 << 22) + 7, 7
    rng = np.random.default_rng(3)
    feat = rng.integers(0, 1 << 20, size=nnz, dtype=np.int64).astype(np.int32)
    feat[rng.integers(0, nnz, size=1000)] = -5
    assert_same(gpu_sketch(F, None, feat), sketch_ref.np_sketch(None, feat, F), "no field array")
    field = ((np.arange(nnz, dtype=np.int64) * 5 + 3) % (F + 1)).astype(np.int32)  # (field 7 of 7: does not count)
    assert_same(gpu_sketch(F, field, feat), sketch_ref.np_sketch(field, feat, F), "with a field array")


def test_ids_built_for_chosen_ranks():
    """Ids whose hashed bits are chosen by inverting the mix: w == 0 (rank 19), rank 1, rank 18."""
    F = 8
    field, feat, expect = [], [], {}
    for f in range(F):
        taken = 0
        for idx in range(100, 100 + 64):  # (an inverse that is a negative id is no id: take the next register)
            low = {0: 0, 1: 1 << 17, 2: 1}[taken % 3]  # low 18 bits: none set, the top one, the bottom one
            x = (idx << 18) | low
            v = sketch_ref.feat_for_bits(f, x)
            if v < 0:
                continue
            field.append(f)
            feat.append(v)
            expect[(f, idx)] = {0: 19, 1: 1, 2: 18}[taken % 3]
            taken += 1
            if taken == 9:
                break
        assert taken == 9
    field, feat = np.array(field, np.int32), np.array(feat, np.int32)
    want = sketch_ref.np_sketch(field, feat, F)
    for (f, idx), rank in expect.items():
        assert want[0][f, idx] == rank
    assert int((want[0] != 0).sum()) == len(expect) and sorted(set(want[0][want[0] != 0].tolist())) == [1, 18, 19]
    for how in ("pageable", "device"):
        assert_same(gpu_sketch(F, field, feat, how), want, how)
    # a lower rank after a higher one changes nothing: rank 19, then rank 1 in the same register
    f, idx = next(k for k, r in expect.items() if r == 19)
    lower = next(v for v in (sketch_ref.feat_for_bits(f, (idx << 18) | (1 << 17) | j) for j in range(64)) if v >= 0)
    both = gpu_sketch(F, np.concatenate([field, [f]]).astype(np.int32), np.concatenate([feat, [lower]]).astype(np.int32))
    assert np.array_equal(both[0], want[0]) and both[1] == want[1] + 1


def test_one_hot_id_beside_cold_ones():
    rng = np.random.default_rng(11)
    feat = np.concatenate([np.full(100000, 123456789, np.int64), rng.integers(0, 2 ** 31, size=1000, dtype=np.int64)])
    field = np.concatenate([np.full(100000, 2, np.int64), rng.integers(0, 4, size=1000)])
    order = rng.permutation(feat.size)
    field, feat = field[order].astype(np.int32), feat[order].astype(np.int32)
    want = sketch_ref.np_sketch(field, feat, 4)
    assert want[1] == 101000
    for how in ("pageable", "zero_copy", "device"):
        assert_same(gpu_sketch(4, field, feat, how), want, how)


def test_any_order_and_batching_gives_the_same_sketch():
    F, nnz = 8, 40013
    field, feat = entries(nnz, F, seed=77)
    want = sketch_ref.np_sketch(field, feat, F)
    assert_same(gpu_sketch(F, field, feat), want, "one call")
    assert_same(gpu_sketch(F, field[::-1].copy(), feat[::-1].copy()), want, "reverse order")
    cuts = np.sort(np.random.default_rng(5).integers(0, nnz, size=12))
    cuts = [0] + cuts.tolist() + [nnz]
    sk = fa.FieldSketch(F)
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):  # 13 ragged calls (one may be empty), the ways mixed
        feed(sk, field[lo:hi].copy(), feat[lo:hi].copy(), ("pageable", "zero_copy", "device")[i % 3])
    assert_same(sk.read(), want, "13 ragged calls")
    sk.close()


def test_halves_combine_by_maximum():
    F, nnz = 8, 30011
    field, feat = entries(nnz, F, seed=99)
    whole = gpu_sketch(F, field, feat)
    a = gpu_sketch(F, field[:nnz // 2].copy(), feat[:nnz // 2].copy())
    b = gpu_sketch(F, field[nnz // 2:].copy(), feat[nnz // 2:].copy())
    assert np.array_equal(np.maximum(a[0], b[0]), whole[0])
    assert (a[1] + b[1], a[2] + b[2]) == (whole[1], whole[2])
    assert_same(whole, sketch_ref.np_sketch(field, feat, F), "the whole")


def test_argument_errors_on_a_live_sketch():
    lib = fa.load_library()
    sk = fa.FieldSketch(4)
    feat = np.arange(8, dtype=np.int32)
    assert lib.ffm_engine_sketch_add(sk.h, -1, None, feat.ctypes.data, 0) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_add(sk.h, 8, None, None, 0) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_add_device(sk.h, -1, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_add_device(sk.h, 8, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_sketch_add(sk.h, 0, None, None, 0) == 0 and lib.ffm_engine_sketch_add_device(sk.h, 0, None, None) == 0
    # zero_copy of memory that is not page-locked is refused, not read
    assert lib.ffm_engine_sketch_add(sk.h, 8, None, feat.ctypes.data, 1) == fa.engine.E_INVALID
    assert b"page-locked" in lib.ffm_engine_last_error()
    nv, nb = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.ffm_engine_sketch_read(sk.h, None, ctypes.byref(nv), ctypes.byref(nb)) == 0  # (reg may be NULL)
    assert (nv.value, nb.value) == (0, 0)
    with pytest.raises(ValueError):
        sk.add(np.zeros(3, np.int32), np.zeros(4, np.int32))
    sk.close()
    with pytest.raises(fa.EngineError) as ei:
        fa.FieldSketch(0)
    assert ei.value.code == fa.engine.E_INVALID


def test_a_sketch_beside_an_engine_on_the_same_device():
    """Fill the sketch, train one small block on an engine, then read the sketch: both are right."""
    from ftrl_ffm_amd import synth
    from oracle.pyoracle import CpuModel
    F, k, nf = 8, 8, 400
    hp = dict(w_alpha=0.1, w_beta=1.0, w_l1=0.01, w_l2=0.1)
    rng = np.random.default_rng(0)
    o = CpuModel("oracle", "FFM", nf, F, k, **hp)
    st = o.zero_state()
    for key in st:
        if key.endswith("_n"):
            st[key][...] = rng.uniform(0.05, 1.0, st[key].shape).astype(np.float32)
        elif key.endswith("_z"):
            st[key][...] = rng.normal(0, 0.3, st[key].shape).astype(np.float32)
        elif key.endswith("_w"):
            st[key][...] = rng.normal(0, 0.02, st[key].shape).astype(np.float32)
    o.set_state(st)
    sk = fa.FieldSketch(F)
    e = fa.Engine("FFM", nf, F, k, skip_init=True, max_batch_rows=128, **hp)
    e.set_state(st)
    blk = synth.Generator(F, nf, "zipf", seed=1).block(128)
    sk.add(blk.field, blk.feat)
    lg_e, ls_e = e.train_batch(blk.rows(0, 128))
    got = sk.read()
    lg_o, ls_o = o.train_batch(blk.rows(0, 128))
    assert np.array_equal(lg_o.view(np.uint32), lg_e.view(np.uint32))
    assert abs(ls_o - ls_e) <= 1e-9 * max(1.0, abs(ls_o))
    so, se = o.get_state(), e.get_state()
    for key in so:
        assert np.array_equal(so[key].view(np.uint32), se[key].view(np.uint32)), key
    assert_same(got, sketch_ref.np_sketch(blk.field, blk.feat, F), "the sketch")
    e.close()
    sk.close()
