"""Every table-indexing kernel on records that begin past element 2^31 and past element 2^32.

FFM 39 x 16 at util.BIG_NF = 6 882 969 features -- the smallest count with 8 records wholly past element 2^32 of a
serving table (624 elements per feature): an fp16 serving engine (8.6 GB), an fp32 one (17.2 GB) and a training
engine (records of 3 x 624: 51.5 GB), all created with skip_init and held for the module; FM k = 64 at util.BIG_NF_FM
= 22 369 630 features (records of 192: 17.2 GB).  The module needs about 80 GB of HBM for its three engines and up
to 52 GB more while a case holds a second engine (130 GB at its peak; case 12 holds 92 GB after the others are
closed); a fixture or case that finds less skips, as tests/test_gpu_scale.py does.  A signed 32-bit element index breaks at 2^31; an unsigned one, or a 32-bit byte offset into 4-byte elements,
at 2^32 -- the probe ids (util.big_probe_ids) sit on both sides of both, in every layout, with the records that
straddle them and their neighbours.

The yardstick everywhere is oracle.pyoracle.CpuModel on the id-remapped compact model (util.BigCase: renaming ids is
exact for FFM and FM, the arithmetic depends on (field, record) only), holding for a serving engine the decoded
weights (test_gpu_serve.decoded).  Logits, probabilities and state bit for bit (NaN with NaN), double loss sums by
util.loss_close; counters equal numpy's over the compact arrays.  Nothing has a tolerance.  The tables start zeroed
and only probe rows are ever written, so a read that lands elsewhere finds zeros or another probe's weights
(tests/test_big_offsets_host.py shows on the CPU that either changes every row), and a write that lands elsewhere is
looked for in util.alias_ids -- the low records a wrapped index of a probe would hit -- which must stay zero.

case  what runs -- the kernel it is there for -- the yardstick
 1    predict_batch on the three engines, predict_batch_async with scores on the serving ones -- ffm_row_wave_kernel,
      WaveTable<FMT>::slot in its three formats -- the oracle's predict_batch
 2    score_candidates, f32 and f16 -- the two candidate kernels' slot() -- the oracle on spell_out_candidates' rows
 3    set_pair_mask, all pairs and a seeded half, three engines -- the pair-mask kernel -- case 1; the oracle on zeroed slots
 4    predict_ablated, predict_pair_ablated, training and f16 -- the field and pair ablation kernels -- the oracle on
      drop_field's blocks and on drop_pair_weights' weights
 5    set_rows / get_rows, set_rows_raw / get_rows_raw -- rows_copy_kernel, serve_rows_copy_kernel, serve_rows_raw_kernel,
      lin_rows_copy_kernel -- the arrays sent; numpy's astype(float16) on the high ids; alias rows zero
 6    pack_from into f32 and f16 -- serve_pack_kernel -- decoded compact state; numpy's counts; alias rows zero
 7    sync_from, sync_moved, export_delta / apply_delta -- serve_sync_kernel and its bitmap -- numpy's counts and ids;
      case 1 on the new weights
 8    refresh_weights -- refresh_weights_kernel -- the oracle's maybe_zero_weight per element (test_gpu_refresh_weights)
 9    changed_features, sparse_state, load_sparse_state -- the changed-features scan and its bitmap -- the ids that were set
10    create without skip_init -- init_weights_kernel, serve_init_kernel -- init_weights_host at the draw indices
11    train_batch (FFM; FM k = 64 with predict_batch) -- the row and update kernels -- the oracle's train_batch
12    cases 1-4, 6-9 and 11 where the index of a vector of four factors passes 2^31 and 2^32 (see there)

Left out on purpose: get_weights / set_weights of a whole table move 9 to 17 GB across PCIe into a host array of that
size, which is no test of a few seconds -- serve_dense_copy_kernel stays pinned at small sizes only
(tests/test_gpu_serve.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import drop_field, drop_pair_weights, pair_count, pair_fields
from ftrl_ffm_amd.synth import Block
from test_gpu_pair_mask import all_pairs, masked_weights, seeded_pairs
from test_gpu_refresh_weights import _expected as refresh_expected
from test_gpu_serve import decoded, rounding_table
from util import (BIG_F, BIG_FM_K, BIG_K, BIG_L, BIG_LAYOUTS, BIG_NF, BIG_NF_FM, BIG_NF_TRAIN_INIT, assert_bitwise,
                  big_case, big_step, bits, edge_ids, get_bias3, loss_close, nonfinite_share, set_bias3, straddling_ids)

pytestmark = pytest.mark.gpu

KINDS = ("train", "f32", "f16")
FORMATS = ("f32", "f16")
MAX_ROWS = 128
ROW_KEYS = fa.Engine.ROW_KEYS


def _free_gb():
    free_b, _ = torch.cuda.mem_get_info()
    return free_b / 1e9


def need(gb):
    if _free_gb() < gb:
        pytest.skip("needs %.0f GB of free HBM, have %.0f" % (gb, _free_gb()))


def table_gb(kind, n_feats):
    """The free HBM an engine of that kind and count is asked to find: its table and 2 GB for everything else."""
    stride, eb = BIG_LAYOUTS[kind]
    return n_feats * stride * eb / 1e9 + 2


def fmt_of(kind):
    return "f16" if kind == "f16" else "f32"  # (a training engine and an fp32 serving engine hold the same w bits)


def make(kind, n_feats=BIG_NF, **kw):
    c = big_case("ffm")  # (every case has its hyper-parameters)
    kw.setdefault("skip_init", True)
    return fa.Engine("FFM", n_feats, BIG_F, BIG_K, max_batch_rows=MAX_ROWS, max_batch_nnz=MAX_ROWS * 64,
                     serve=None if kind == "train" else kind, **dict(c.hp, **kw))


@pytest.fixture(scope="module")
def case():
    c = big_case("ffm")
    assert c.n_feats == BIG_NF and (BIG_NF - 8) * BIG_L >= 2 ** 32 > (BIG_NF - 9) * BIG_L
    assert 3441480 * BIG_L < 2 ** 31 < 3441481 * BIG_L and 6882960 * BIG_L < 2 ** 32 < 6882961 * BIG_L
    for kind in KINDS:  # (tests/test_big_offsets_host.py checks the rest of what the block must hold)
        t = c.tiers(kind, c.block.feat)
        assert min((t == 0).sum(), (t == 1).sum(), (t == 2).sum()) >= 100, kind
    assert set(c.straddlers()) <= set(c.block.feat.tolist())
    return c


@pytest.fixture(scope="module")
def engines(case):
    """engines(kind, name="ffm"): the engine of that kind at big_case(name)'s feature count, made on first use and kept;
    engines.release(name) closes a case's engines; all are closed when the module is done."""
    held = {}

    def get(kind, name="ffm"):
        if (name, kind) not in held:
            n = big_case(name).n_feats
            need(table_gb(kind, n))
            held[name, kind] = make(kind, n)
            assert held[name, kind].row_len == BIG_L and held[name, kind].n_feats == n
        return held[name, kind]

    def release(name):
        for key in [key for key in held if key[0] == name]:
            held.pop(key).close()
    get.release = release
    yield get
    for e in held.values():
        e.close()


def load(e, c, state=None):
    """The probes' rows of the compact `state` (default: the start state) and its bias into the big engine."""
    state = c.state if state is None else state
    if e.serve:
        e.set_rows(c.probes32, c.rows(state, ("lin_w", "vec_w")))
        e.set_weights(bias=state["bias3"][:1])
    else:
        e.set_rows(c.probes32, c.rows(state))
        set_bias3(e, state["bias3"])


def bias_of(e):
    b = np.zeros(1, np.float32)
    e._check(e.lib.ffm_engine_get_weights(e.h, b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None, None))
    return b


def kind_of(e):
    return e.serve or "train"


def assert_aliases_zero(e, c, what):
    got = e.get_rows(c.aliases(kind_of(e)))
    for key, a in got.items():
        assert not bits(a).any(), "%s: %s of a record a wrapped index would hit is no longer zero" % (what, key)
    if e.serve:
        lw, lat = e.get_rows_raw(c.aliases(kind_of(e)))
        assert not bits(lw).any() and not lat.view(np.uint16).any(), what


def held_oracle(c, kind, state=None, vec_w=None):
    """The compact oracle that holds what an engine of `kind` holds after load()."""
    state = c.state if state is None else state
    if kind == "train" and vec_w is None:
        return c.oracle(state)
    vw = decoded(state["vec_w"], fmt_of(kind)) if vec_w is None else vec_w
    return c.weights_oracle(vw, state["lin_w"], state["bias3"][0])


@functools.lru_cache(maxsize=None)
def predicted(name, fmt):
    """(logits, probabilities, loss sum) of the block under the oracle holding the start weights as `fmt` stores them."""
    c = big_case(name)
    o = c.weights_oracle(decoded(c.state["vec_w"], fmt))
    lg, ls = o.predict_batch(c.compact_block)
    out = (lg, o.predict_batch(c.compact_block, output_prob=True)[0], ls)
    for a in out[:2]:
        a.setflags(write=False)
    assert (~np.isfinite(lg)).mean() <= 0.1
    return out


def check_predict(e, blk, want, what):
    lg, ls = e.predict_batch(blk)
    assert_bitwise(lg, want[0], what + " logits")
    assert_bitwise(e.predict_batch(blk, output_prob=True)[0], want[1], what + " probabilities")
    assert loss_close(ls, want[2]), "%s: loss sum %r vs %r" % (what, ls, want[2])


# ---- 1. prediction ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_prediction(case, engines, kind):
    run_prediction(case, engines(kind), "ffm")


def run_prediction(case, e, name):
    kind = kind_of(e)
    load(e, case)
    want = predicted(name, fmt_of(kind))
    check_predict(e, case.block, want, kind)
    if kind == "train":
        return
    for prob in (False, True):
        out = e.score_buffer(case.block.n_rows + 8)
        out[:] = np.float32(-7.0)
        e.predict_batch_async(case.block, scores=out, output_prob=prob)
        total = e.train_flush()
        assert_bitwise(out[:case.block.n_rows], want[int(prob)], "%s async scores prob=%d" % (kind, prob))
        assert (out[case.block.n_rows:] == np.float32(-7.0)).all() and loss_close(total, want[2])
        e.free_score_buffer(out)


# ---- 2. score_candidates ---------------------------------------------------------------------------------------

def candidate_requests(c, per_req=5):
    """(ctx, cand_req_ptr, cand) cut from the block's regular rows: a request's context is a row's entries of the
    even fields, its candidates the odd fields' entries of the next five rows (the ids past 2^32 are dealt to
    neighbouring fields, so both halves hold some); a request without candidates first and last, one empty
    candidate."""
    blk = c.block
    rows = [r for r in range(blk.n_rows) if blk.row_ptr[r + 1] - blk.row_ptr[r] == BIG_F]

    even, odd, whole = range(0, BIG_F, 2), range(1, BIG_F, 2), range(BIG_F)

    def part(r, cols):
        a = int(blk.row_ptr[r])
        return [(int(blk.field[a + j]), int(blk.feat[a + j]), float(blk.val[a + j])) for j in cols]
    ctxs, cands, n_of = [part(rows[0], range(7))], [], [0]
    for i in range(0, len(rows) - per_req, per_req + 1):
        ctxs.append(part(rows[i], even))
        for j in range(1, per_req + 1):
            cands.append(part(rows[i + j], odd))
        n_of.append(per_req)
    cands[3] = []
    ctxs.append(part(rows[1], whole))
    n_of.append(0)

    def to_block(rs):
        flat = [x for r in rs for x in r]
        return Block(np.cumsum([0] + [len(r) for r in rs]).astype(np.int32), np.array([x[0] for x in flat], np.int32),
                     np.array([x[1] for x in flat], np.int32), np.array([x[2] for x in flat], np.float32),
                     np.zeros(len(rs), np.int32))
    return to_block(ctxs), np.cumsum([0] + n_of).astype(np.int32), to_block(cands)


@pytest.mark.parametrize("fmt", FORMATS)
def test_score_candidates(case, engines, fmt):
    run_score_candidates(case, engines(fmt))


def run_score_candidates(case, e):
    fmt = kind_of(e)
    load(e, case)
    ctx, rq, cand = candidate_requests(case)
    blk = fa.spell_out_candidates(ctx, rq, cand)
    for kind in case.tier_kinds:  # contexts and candidates both reach into every tier
        for part in (ctx, cand):
            t = case.tiers(kind, part.feat)
            assert min((t == 0).sum(), (t == 1).sum(), (t == 2).sum()) >= 5, kind
    assert cand.n_rows >= 40 and cand.n_rows % 4 != 0
    o = held_oracle(case, fmt)
    for prob in (False, True):
        want = o.predict_batch(case.remap(blk), output_prob=prob)[0]
        assert np.isfinite(want).mean() >= 0.9
        assert_bitwise(e.score_candidates(ctx, rq, cand, output_prob=prob), want, "%s candidates prob=%d" % (fmt, prob))
        assert_bitwise(e.predict_batch(blk, output_prob=prob)[0], want, "%s spelled-out rows prob=%d" % (fmt, prob))


# ---- 3. pair masks ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def masked(name, fmt, seed=5):
    c = big_case(name)
    assert bits(c.state["bias3"][:1])[0] != 0x80000000, "the bias is not -0.0"
    assert np.array_equal(c.compact_block.field, c.compact_block.feat // c.per)  # one field per id
    kept = seeded_pairs(BIG_F, seed, 0.5)
    assert 0 < len(kept) < pair_count(BIG_F)
    o = c.weights_oracle(masked_weights(decoded(c.state["vec_w"], fmt), BIG_F, c.per, kept))
    lg, ls = o.predict_batch(c.compact_block)
    out = (lg, o.predict_batch(c.compact_block, output_prob=True)[0], ls)
    nonempty = np.diff(c.block.row_ptr) > 0
    assert (bits(lg) != bits(predicted(name, fmt)[0]))[nonempty].all(), "the mask changes every row"
    return kept, out


@pytest.mark.parametrize("kind", KINDS)
def test_pair_mask(case, engines, kind):
    run_pair_mask(case, engines(kind), "ffm")


def run_pair_mask(case, e, name):
    kind = kind_of(e)
    load(e, case)
    kept, want = masked(name, fmt_of(kind))
    try:
        e.set_pair_mask(all_pairs(BIG_F))
        check_predict(e, case.block, predicted(name, fmt_of(kind)), kind + " all pairs kept")
        e.set_pair_mask(kept)
        check_predict(e, case.block, want, kind + " seeded mask")
    finally:
        e.set_pair_mask(None)


# ---- 4. ablation -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ablated(name, fmt):
    """((logits, probabilities, loss sums) of the 40 field variants, the same of the 781 pair variants)."""
    c = big_case(name)
    blk = c.compact_block
    held = decoded(c.state["vec_w"], fmt)
    o = c.weights_oracle(held)
    res = []
    for b in [drop_field(blk, v) for v in range(BIG_F)] + [blk]:
        lg, ls = o.predict_batch(b)
        res.append((lg, o.predict_batch(b, output_prob=True)[0], ls))
    fields = tuple(np.stack([r[j] for r in res]) for j in range(2)) + (np.array([r[2] for r in res]),)
    res = []
    V = pair_count(BIG_F)
    w3 = held.reshape(c.n_compact, BIG_F, BIG_K)
    for v in range(V + 1):
        vw = held
        if v < V:
            f, g = pair_fields(BIG_F, v)
            vw = drop_pair_weights(w3, np.arange(f * c.per, (f + 1) * c.per), g).reshape(held.shape)
        o = c.weights_oracle(vw)
        lg, ls = o.predict_batch(blk)
        res.append((lg, o.predict_batch(blk, output_prob=True)[0], ls))
    pairs = tuple(np.stack([r[j] for r in res]) for j in range(2)) + (np.array([r[2] for r in res]),)
    assert len({bits(x).tobytes() for x in pairs[0]}) > V // 2  # the variants are not all one prediction
    return fields, pairs


@pytest.mark.parametrize("kind", ["train", "f16"])
def test_ablation(case, engines, kind):
    run_ablation(case, engines(kind), "ffm")


def run_ablation(case, e, name):
    kind = kind_of(e)
    load(e, case)
    fields, pairs = ablated(name, fmt_of(kind))
    e.ablation_enable()
    e.pair_ablation_enable()
    for name, call, want in (("field", e.predict_ablated, fields), ("pair", e.predict_pair_ablated, pairs)):
        for prob in (False, True):
            got, gl = call(case.block, output_prob=prob)
            assert got.shape == want[int(prob)].shape
            assert_bitwise(got, want[int(prob)], "%s %s ablation prob=%d" % (kind, name, prob))
            for v in range(gl.size):
                assert loss_close(gl[v], want[2][v]), "%s %s ablation variant %d: loss sum %r vs %r" % (kind, name, v, gl[v], want[2][v])


# ---- 5. rows in and out ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_rows_in_and_out(case, engines, kind):
    c, e = case, engines(kind)
    load(e, c)
    rows = c.rows()
    got = e.get_rows(c.probes32)
    assert sorted(got) == (sorted(ROW_KEYS) if kind == "train" else ["lin_w", "vec_w"])
    for key in got:
        want = decoded(rows[key], kind) if key == "vec_w" and kind != "train" else rows[key]
        assert_bitwise(got[key], want, "%s get_rows %s" % (kind, key))
    order = np.random.default_rng(3).permutation(c.probes.size)  # a shuffled id list, ids twice
    order = np.concatenate([order, order[:7]])
    again = e.get_rows(c.probes32[order])
    for key in got:
        assert_bitwise(again[key], got[key][order], "%s get_rows shuffled %s" % (kind, key))
    assert_aliases_zero(e, c, kind + " after set_rows")
    if kind == "train":  # (rows in a table's own bits are a serving engine's: a training engine's rows are fp32 as they are)
        with pytest.raises(fa.EngineError) as err:
            e.get_rows_raw(c.probes32[-1:])
        assert err.value.code == fa.engine.E_UNSUPPORTED
        return
    # the rounding rule on the records past 2^31 and 2^32 (test_gpu_serve.rounding_table's values)
    high = c.probes32[c.tiers(kind) != 0]
    special = np.resize(rounding_table()[0].ravel(), (high.size, BIG_L)).astype(np.float32)
    e.set_rows(high, dict(vec_w=special))
    want = decoded(special, kind)
    assert kind == "f32" or (np.isinf(want) & np.isfinite(special)).any()
    assert_bitwise(e.get_rows(high)["vec_w"], want, kind + " rounding rule on the high ids")
    # the table's own bits
    lw, lat = e.get_rows_raw(high)
    sel = ~np.isnan(special)  # (a NaN's payload is unspecified)
    assert np.array_equal((bits(lat) if kind == "f32" else lat)[sel], fmt_bits(special, kind)[sel]), kind + " get_rows_raw"
    assert_bitwise(lw, rows["lin_w"][c.tiers(kind) != 0], kind + " get_rows_raw lin_w")
    rng = np.random.default_rng(9)
    if kind == "f16":
        pat = rng.integers(0, 1 << 16, (c.probes.size, BIG_L)).astype(np.uint16)
    else:
        pat = rng.integers(0, 1 << 32, (c.probes.size, BIG_L), dtype=np.uint64).astype(np.uint32).view(np.float32)
    plw = rng.normal(0, 1, c.probes.size).astype(np.float32)
    e.set_rows_raw(c.probes32, plw, pat)
    glw, glat = e.get_rows_raw(c.probes32)
    assert np.array_equal(bits(glw), bits(plw))
    assert np.array_equal(glat.view(np.uint16), pat.view(np.uint16)), kind + ": raw rows do not round-trip"
    assert_aliases_zero(e, c, kind + " after set_rows_raw")
    load(e, c)


# ---- 6. pack_from ----------------------------------------------------------------------------------------------

def planted_state(c):
    """The start state with the rounding table's values in the w rows of the probes past 2^32 (serving layout)."""
    st = {key: a.copy() for key, a in c.state.items()}
    top = c.compact[c.tiers(c.tier_kinds[0]) == 2]
    st["vec_w"][top] = np.resize(rounding_table()[0].ravel(), (top.size, BIG_L))
    return st


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_from(case, engines, fmt):
    run_pack_from(case, engines("train"), engines(fmt))


def run_pack_from(c, t, s):
    fmt = kind_of(s)
    st = planted_state(c)
    load(t, c, st)
    stats = s.pack_from(t)
    w = c.rows(st, ("vec_w",))["vec_w"]
    want = decoded(w, fmt)
    counts = dict(n_latent=c.n_feats * BIG_L, n_inexact=0, n_to_inf=0, n_to_zero=0)
    if fmt == "f16":  # (every element outside the probe rows is +0.0 and converts exactly)
        counts.update(n_inexact=int(((bits(want) != bits(w)) & ~np.isnan(w)).sum()),
                      n_to_inf=int((np.isfinite(w) & np.isinf(want)).sum()),
                      n_to_zero=int((~np.isnan(w) & (w != 0) & (want == 0)).sum()))
        assert counts["n_to_inf"] >= 4 and counts["n_to_zero"] >= 6 and counts["n_inexact"] > w.size // 2
    assert stats == counts, (fmt, stats, counts)
    got = s.get_rows(c.probes32)
    assert_bitwise(got["vec_w"], want, "pack_from %s vec_w" % fmt)
    assert_bitwise(got["lin_w"], c.rows(st, ("lin_w",))["lin_w"], "pack_from %s lin_w" % fmt)
    assert bits(bias_of(s))[0] == bits(st["bias3"][:1])[0]
    assert_aliases_zero(s, c, "pack_from " + fmt)
    src = t.get_rows(c.probes32)
    for key, a in c.rows(st).items():
        assert_bitwise(src[key], a, "pack_from left the source's %s alone" % key)
    load(t, c)
    load(s, c)


def _predict_of(c, state, fmt):
    o = held_oracle(c, fmt, state)
    lg, ls = o.predict_batch(c.compact_block)
    return lg, o.predict_batch(c.compact_block, output_prob=True)[0], ls


# ---- 7. serving deltas -----------------------------------------------------------------------------------------

def fmt_bits(w, fmt):
    with np.errstate(over="ignore", invalid="ignore"):
        return bits(np.ascontiguousarray(w, np.float32)) if fmt == "f32" else np.asarray(w, np.float32).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("fmt", FORMATS)
def test_serving_deltas(case, engines, fmt):
    run_serving_deltas(case, engines("train"), engines(fmt), "ffm")


def run_serving_deltas(c, t, s, name):
    fmt = kind_of(s)
    load(t, c)
    s.pack_from(t)
    n = c.n_feats
    need(table_gb(fmt, n))
    second = make(fmt, n)
    try:
        second.pack_from(t)
        w0 = (n - 1) // 64 * 64
        assert n < 2 ** 26  # no bitmap word edge at 2^26 or 2^27 features: the table's last word, and the one before it
        forced = [n - 1 - 64, n - 1, w0 - 1, w0, 0] + c.straddlers()
        pick = np.zeros(c.probes.size, bool)
        pick[::3] = True
        pick[np.searchsorted(c.probes, forced)] = True
        for kind in c.tier_kinds:
            assert set(c.tiers(kind)[pick].tolist()) == {-1, 0, 1, 2}, kind
        assert (n - 1 - 64) // 64 + 1 == (n - 1) // 64 and (w0 - 1) // 64 + 1 == w0 // 64
        new = {key: a.copy() for key, a in c.state.items()}
        rng = np.random.default_rng(11)
        sub = c.compact[pick]
        grow = rng.random((sub.size, BIG_L)) < 0.3  # three elements of ten move, by far more than a half's resolution
        new["vec_w"][sub] = np.where(grow, c.state["vec_w"][sub] * np.float32(1.5), c.state["vec_w"][sub])
        lin = sub[::2]
        new["lin_w"][lin] = c.state["lin_w"][lin] + np.float32(0.25)
        t.set_rows(c.probes32[pick], c.rows(new, ids=c.probes[pick]))
        before, after = c.rows(), c.rows(new)
        lin_moved = bits(before["lin_w"]) != bits(after["lin_w"])
        lat_moved = fmt_bits(before["vec_w"], fmt) != fmt_bits(after["vec_w"], fmt)
        moved = lin_moved | lat_moved.any(axis=1)
        assert np.array_equal(moved, pick) and 0 < lin_moved.sum() < moved.sum()
        stats = s.sync_from(t)
        assert stats == dict(n_moved=int(moved.sum()), n_lin_moved=int(lin_moved.sum()), n_lat_moved=int(lat_moved.sum()),
                             bias_moved=0), stats
        ids = s.sync_moved()
        assert ids.dtype == np.int32 and np.array_equal(ids, c.probes32[pick]), "sync_moved lists other ids than the subset"
        d = s.export_delta()
        assert np.array_equal(d["ids"], c.probes32[pick])
        second.apply_delta(d)
        a, b = s.get_rows_raw(c.probes32), second.get_rows_raw(c.probes32)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1].view(np.uint16), b[1].view(np.uint16))
        assert np.array_equal(a[1].view(np.uint16), np.ascontiguousarray(fmt_bits(after["vec_w"], fmt)).view(np.uint16))
        want = _predict_of(c, new, fmt)
        assert (bits(want[0]) != bits(predicted(name, fmt)[0])).any()
        for e, name in ((s, "synced"), (second, "delta applied")):
            check_predict(e, c.block, want, "%s %s" % (fmt, name))
            assert_aliases_zero(e, c, "%s %s" % (fmt, name))
    finally:
        second.close()
    load(t, c)
    load(s, c)


# ---- 8. refresh_weights ----------------------------------------------------------------------------------------

def test_refresh_weights(case, engines):
    run_refresh_weights(case, engines("train"))


def run_refresh_weights(c, t):
    load(t, c)  # (the start state's w are draws of their own: stale against W(n, z) everywhere)
    st = dict(c.rows(), bias3=c.state["bias3"].copy())
    want, counts = refresh_expected(st, c.hp, False)
    assert (bits(want["vec_w"]) != bits(st["vec_w"])).mean() > 0.9 and (want["vec_w"] != 0).mean() > 0.5
    got = t.refresh_weights()
    assert got == counts, (got, counts)
    after = t.get_rows(c.probes32)
    assert_bitwise(after["vec_w"], want["vec_w"], "refreshed vec_w")
    assert_bitwise(after["lin_w"], want["lin_w"], "refreshed lin_w")
    assert_bitwise(get_bias3(t)[:1], want["bias_w"], "refreshed bias")
    for key in ("lin_n", "lin_z", "vec_n", "vec_z"):
        assert np.array_equal(bits(after[key]), bits(st[key])), key
    assert_aliases_zero(t, c, "refresh_weights")
    load(t, c)


# ---- 9. the changed-features scan and sparse states --------------------------------------------------------------

def test_changed_features_and_sparse_state(case, engines):
    c, t = case, engines("train")
    load(t, c)
    assert all(bits(a).reshape(c.probes.size, -1).any(axis=1).all() for a in c.rows().values())
    assert_changed_are_the_probes(t, c)
    d = t.sparse_state()
    need(table_gb("train", BIG_NF))
    fresh = make("train")
    try:
        assert fresh.changed_features().size == 0
        fresh.load_sparse_state(d)
        got = fresh.get_rows(c.probes32)
        for key, a in c.rows().items():
            assert_bitwise(got[key], a, "sparse state restored: " + key)
        assert np.array_equal(bits(get_bias3(fresh)), bits(c.state["bias3"]))
        assert np.array_equal(fresh.changed_features(), c.probes32)
        assert_aliases_zero(fresh, c, "load_sparse_state")
        check_predict(fresh, c.block, predicted("ffm", "f32"), "restored engine")
    finally:
        fresh.close()


def assert_changed_are_the_probes(t, c):
    ids = t.changed_features()
    assert ids.dtype == np.int32 and np.array_equal(ids, c.probes32), "the scan lists other ids than those that were set"


# ---- 10. create-time contents ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,n_feats", [("train", BIG_NF_TRAIN_INIT), ("f16", BIG_NF)])
def test_create_time_contents(kind, n_feats):
    stride, eb = BIG_LAYOUTS[kind]
    assert (n_feats - 8) * stride >= 2 ** 32 > (n_feats - 9) * stride
    need(table_gb(kind, n_feats))
    seed, mean, sd = 1234, 0.01, 0.05
    e = make(kind, n_feats, skip_init=False, seed=seed, init_mean=mean, init_stddev=sd)
    try:
        ids = np.unique(np.concatenate([edge_ids(n_feats, stride, eb), [0, n_feats - 2, n_feats - 1]])).astype(np.int32)
        assert set(straddling_ids(n_feats, stride, eb)) <= set(ids.tolist()) and len(straddling_ids(n_feats, stride, eb)) >= 2
        got = e.get_rows(ids)
        draws = np.stack([fa.init_weights_host(seed, mean, sd, True, int(i) * BIG_L, BIG_L) for i in ids])
        assert_bitwise(got["vec_w"], decoded(draws, fmt_of(kind)), kind + " create-time vec_w")
        assert_bitwise(got["lin_w"], np.concatenate([fa.init_weights_host(seed, mean, sd, False, int(i), 1) for i in ids]),
                       kind + " create-time lin_w")
        if kind == "train":
            for key in ("lin_n", "lin_z", "vec_n", "vec_z"):
                assert not bits(got[key]).any(), key
            assert e.changed_features().size == 0  # every w against its draw, the records past 2^32 among them
    finally:
        e.close()


# ---- 11. one training step ---------------------------------------------------------------------------------------

def check_step(e, c, what):
    lo, so, after = big_step(c)
    bad = nonfinite_share(lo, c.state, after)
    assert bad[0] <= 0.1 and bad[1] <= 0.1 and bad[2] > 0, bad
    lg, sg = e.train_batch(c.block)
    assert_bitwise(lg, lo, what + " logits")
    assert loss_close(sg, so), "%s: loss sum %r vs %r" % (what, sg, so)
    got = e.get_rows(c.probes32)
    for key, a in c.rows(after).items():
        assert_bitwise(got[key], a, "%s state %s" % (what, key))
    assert_bitwise(get_bias3(e), after["bias3"], what + " bias")
    assert_aliases_zero(e, c, what)
    o = c.oracle(after)
    po, pl = o.predict_batch(c.compact_block)
    check_predict(e, c.block, (po, o.predict_batch(c.compact_block, output_prob=True)[0], pl), what + " predict after the step")


def test_one_training_step_ffm(case, engines):
    t = engines("train")
    load(t, case)
    check_step(t, case, "FFM")
    load(t, case)


def test_one_training_step_fm():
    c = big_case("fm")
    stride = c.layouts["train"][0]
    assert c.n_feats == BIG_NF_FM and (BIG_NF_FM - 8) * stride >= 2 ** 32 > (BIG_NF_FM - 9) * stride
    assert set(edge_ids(BIG_NF_FM, stride, 4).tolist()) <= set(c.probes.tolist())
    t = c.tiers("train", c.block.feat)
    assert min((t == 0).sum(), (t == 1).sum(), (t == 2).sum()) >= 100 and set(c.straddlers()) <= set(c.block.feat.tolist())
    need(BIG_NF_FM * stride * 4 / 1e9 + 2)
    e = fa.Engine("FM", BIG_NF_FM, 1, BIG_FM_K, skip_init=True, max_batch_rows=MAX_ROWS, max_batch_nnz=MAX_ROWS * 64, **c.hp)
    try:
        assert e.row_len == BIG_FM_K
        load(e, c)
        check_predict(e, c.block, _predict_of(c, c.state, "train"), "FM predict")
        check_step(e, c, "FM")
    finally:
        e.close()


# ---- 12. where the index of a vector of four factors passes 2^31 and 2^32 ------------------------------------------
# WaveTable<FMT>::slot, serve_pack_kernel, serve_sync_kernel and refresh_weights_kernel count in vectors of four
# factors (16 bytes; 8 of an fp16 table): at BIG_NF their index reaches 1.07e9 in a serving table and 3.2e9 in a
# training engine's records, so that a signed 32-bit vector index breaks in the training engine alone and an unsigned
# one nowhere.  These two cases cross both thresholds in that unit, with probe sets, blocks and alias ids of their own
# (tiers counted in vectors): an fp16 serving table of 27 531 850 features (34.4 GB) and a training engine of 9 177 289
# (68.7 GB, with an fp16 table of that count, 11.5 GB, as the destination of pack_from and sync_from).  The engines of
# the cases above are closed first.

def vec_case(name, kinds):
    c = big_case(name)
    for kind in kinds:
        stride = c.layouts[kind][0]
        assert (c.n_feats - 8) * stride >= 2 ** 34 > (c.n_feats - 9) * stride and c.n_feats < 2 ** 31
        t = c.tiers(kind, c.block.feat)
        assert min((t == 0).sum(), (t == 1).sum(), (t == 2).sum()) >= 100, kind
    assert set(c.straddlers()) <= set(c.block.feat.tolist())
    return c


def test_vector_index_serving(engines):
    c = vec_case("vec_serve", ["f16"])
    engines.release("ffm")
    e = engines("f16", "vec_serve")
    run_prediction(c, e, "vec_serve")
    run_score_candidates(c, e)
    run_pair_mask(c, e, "vec_serve")
    run_ablation(c, e, "vec_serve")
    assert_aliases_zero(e, c, "vector tier, f16")
    engines.release("vec_serve")


def test_vector_index_training(engines):
    c = vec_case("vec_train", ["train"])
    engines.release("ffm")
    engines.release("vec_serve")
    t = engines("train", "vec_train")
    run_prediction(c, t, "vec_train")
    run_pair_mask(c, t, "vec_train")
    run_ablation(c, t, "vec_train")
    run_refresh_weights(c, t)
    load(t, c)
    assert_changed_are_the_probes(t, c)
    s = engines("f16", "vec_train")
    run_pack_from(c, t, s)
    run_serving_deltas(c, t, s, "vec_train")
    load(t, c)
    check_step(t, c, "FFM, vector tier")
    engines.release("vec_train")
