"""Shared helpers for the parity tests: golden loading, seeded inputs, bitwise comparison."""
import glob
import gzip
import os

import numpy as np

from oracle.pyoracle import CpuModel, Csr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
STATE_KEYS = ("bias3", "lin_w", "lin_n", "lin_z", "vec_w", "vec_n", "vec_z")
DEFAULT_HP = dict(w_alpha=1e-4, w_beta=1.0, w_l1=0.1, w_l2=5.0)
STRESS_HP = dict(w_alpha=0.1, w_beta=1.0, w_l1=0.01, w_l2=0.1)


def _hp(alpha, beta, l1, l2):
    """A hyper-parameter tuple whose values are exactly the float32s the engine and the oracle get."""
    return {key: float(np.float32(v)) for key, v in zip(("w_alpha", "w_beta", "w_l1", "w_l2"), (alpha, beta, l1, l2))}


_F = np.float32
_INF = _F(np.inf)
# Every state of the engine's create-time arithmetic flags (ffm_engine_create: fast_div needs alpha in
# [2^-30, 2^30], fast_w needs fast_div and beta in [2^-40, 2^40]) with both inclusive ends of both ranges
# and the first float outside each; the ordinary FTRL settings l1 = 0, l2 = 0, beta = 0; in-range sets
# that are not powers of two.  The sets with a large alpha take l2 = 5: W = -num / (l2 + tiny).
HP_SETS = {
    "default_hp": DEFAULT_HP,
    "stress_hp": STRESS_HP,
    "alpha_2m30": _hp(2.0 ** -30, 1.0, 0.01, 0.1),
    "alpha_below_2m30": _hp(np.nextafter(_F(2.0 ** -30), _F(0)), 1.0, 0.01, 0.1),
    "alpha_2p30": _hp(2.0 ** 30, 1.0, 0.01, 5.0),
    "alpha_above_2p30": _hp(np.nextafter(_F(2.0 ** 30), _INF), 1.0, 0.01, 5.0),
    "alpha_3e-38": _hp(3e-38, 1.0, 0.01, 0.1),
    "alpha_1.3x2p31": _hp(1.3 * 2.0 ** 31, 1.0, 0.01, 5.0),
    "beta_zero": _hp(0.1, 0.0, 0.01, 0.1),
    "beta_2m40": _hp(0.1, 2.0 ** -40, 0.01, 0.1),
    "beta_below_2m40": _hp(0.1, np.nextafter(_F(2.0 ** -40), _F(0)), 0.01, 0.1),
    "beta_2p40": _hp(0.1, 2.0 ** 40, 0.01, 0.1),
    "beta_above_2p40": _hp(0.1, np.nextafter(_F(2.0 ** 40), _INF), 0.01, 0.1),
    "beta_1.4e-38": _hp(1e-4, 1.4e-38, 0.1, 5.0),
    "l1_zero": _hp(0.1, 1.0, 0.0, 0.1),
    "l2_zero": _hp(0.1, 1.0, 0.01, 0.0),
    "l1_zero_beta_zero": _hp(0.1, 0.0, 0.0, 0.1),
    "l2_zero_beta_zero": _hp(0.1, 0.0, 0.01, 0.0),
    "all_zero": _hp(0.1, 0.0, 0.0, 0.0),
    "alpha_0.3": _hp(0.3, 0.7, 0.02, 0.3),
    "alpha_0.05": _hp(0.05, 1.0, 0.01, 1.0),
    "ones": _hp(1.0, 1.0, 1.0, 1.0),
}


def arith_flags(hp):
    """(fast_div, fast_w) as ffm_engine_create sets them (engine.hip), the create-time proof of the
    short divide taken to pass for every alpha in range (tests/test_block_semantics.py checks the C
    restatement of that sequence for the alphas of HP_SETS)."""
    a, b = _F(hp["w_alpha"]), _F(hp["w_beta"])
    fast_div = bool(_F(2.0 ** -30) <= a <= _F(2.0 ** 30))
    fast_w = bool(fast_div and _F(2.0 ** -40) <= b <= _F(2.0 ** 40))
    return int(fast_div), int(fast_w)


# The operand guards of the short sequences (ftrl_math.h, kernels_fold.h), restated on float32 arrays.
def sqrt_fast_ok(x):
    """+0 or [2^-96, 2^96]."""
    x = np.asarray(x, _F)
    return (bits(x) == 0) | ((x >= _F(2.0 ** -96)) & (x <= _F(2.0 ** 96)))


def chain_operand_ok(x):
    """[2^-70, 2^96] (also fold_strict_ok; fold_zero_ok adds +0): false for 0, negative, NaN, inf."""
    x = np.asarray(x, _F)
    return (x >= _F(2.0 ** -70)) & (x <= _F(2.0 ** 96))


def div_fast_ok(x):
    """+0 or |x| in [2^-60, 2^60]."""
    x = np.asarray(x, _F)
    ax = np.abs(x)
    return (bits(x) == 0) | ((ax >= _F(2.0 ** -60)) & (ax <= _F(2.0 ** 60)))


def golden_cases():
    """All replayable cases (those written by make_golden.run_case)."""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "g*.npz"))):
        with np.load(p) as z:
            if "mode" in z.files:
                out.append(os.path.basename(p)[:-4])
    return out


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = {k: z[k] for k in z.files}
    d["csr"] = Csr(d["row_ptr"], d["field"], d["feat"], d["val"], d["label"])
    a, b, l1, l2 = [float(x) for x in d["hp"]]
    d["hp_kw"] = dict(w_alpha=a, w_beta=b, w_l1=l1, w_l2=l2)
    d["init"] = {k: d["init_" + k] for k in STATE_KEYS}
    d["final"] = {k: d["final_" + k] for k in STATE_KEYS if "final_" + k in d}
    d["model_type"] = str(d["model_type"])
    d["mode"] = str(d["mode"])
    return d


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bitwise(a, b, what=""):
    """Bit-for-bit equality of float arrays.  NaNs must sit at the same positions; their sign and
    payload bits are not compared (IEEE-754 leaves them unspecified and x86 picks them by operand
    order, which differs between two compilations of the same expression)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size == 0:
        return
    both_nan = (np.isnan(a) & np.isnan(b)).ravel()
    bad = np.flatnonzero((bits(a).ravel() != bits(b).ravel()) & ~both_nan)
    assert bad.size == 0, "%s: %d/%d words differ, first at %d: %r vs %r" % (
        what, bad.size, a.size, bad[0], a.ravel()[bad[0]], b.ravel()[bad[0]])


def assert_state_bitwise(sa, sb, what=""):
    for k in STATE_KEYS:
        if k in sa and k in sb:
            assert_bitwise(sa[k], sb[k], what + ":" + k)


def assert_close(a, b, rtol, atol, what=""):
    """NaN positions must agree exactly; finite values within rtol/atol."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), what + ": NaN positions differ"
    ok = np.isclose(a[~na], b[~nb], rtol=rtol, atol=atol)
    if not ok.all():
        i = np.flatnonzero(~ok)[0]
        raise AssertionError("%s: %d/%d outside rtol=%g atol=%g, first %r vs %r" % (
            what, (~ok).sum(), ok.size, rtol, atol, a[~na][i], b[~nb][i]))


def rand_state(rng, model, n_hi=1.0, z_sd=0.3, w_sd=0.02):
    st = model.zero_state()
    for k in st:
        if k == "bias3":
            continue
        if k.endswith("_n"):
            st[k][...] = (rng.random(st[k].shape) * n_hi).astype(np.float32)
        elif k.endswith("_z"):
            st[k][...] = rng.normal(0, z_sd, st[k].shape).astype(np.float32)
        else:
            st[k][...] = rng.normal(0, w_sd, st[k].shape).astype(np.float32)
    st["bias3"][...] = np.array([0.013, 0.7, -0.4], np.float32)
    return st


def bundled_rows(libsvm=False):
    """The reference's bundled data/libffm_data.txt (committed gzip'd under tests/golden/data)."""
    with gzip.open(os.path.join(GOLDEN, "data", "libffm_data.txt.gz"), "rt") as f:
        lines = f.read().splitlines()
    rows, labels = [], []
    for line in lines:
        t = line.split()
        labels.append(1 if int(t[0]) > 0 else 0)
        row = []
        for tok in t[1:]:
            fld, ft, v = tok.split(":")
            if np.float32(v) != 0:
                row.append((0 if libsvm else int(fld), int(ft), float(np.float32(v))))
        rows.append(row)
    return rows, labels


def make_cpu(kind, case_or_type, dims=None, hp=None):
    if isinstance(case_or_type, dict):
        c = case_or_type
        nf, F, k = [int(x) for x in c["dims"]]
        return CpuModel(kind, c["model_type"], nf, F, k, **c["hp_kw"])
    nf, F, k = dims
    return CpuModel(kind, case_or_type, nf, F, k, **(hp or DEFAULT_HP))


# The per-block occurrence counts at which a feature's update changes path (kernels_group.h): once
# only | few (2..10, gathered four at a time) | hot (11..128; tiles of 16 touches) | very hot
# (129..256) | giant (257..2047, one workgroup; ranges of 256) | super (>= 2048, ranges all over the
# chip) -- each edge with its neighbours, tile / segment edges and partial last ranges among them.
EDGE_COUNTS = (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257,
               258, 511, 512, 513, 2047, 2048, 2049, 2304, 2305, 4096, 4097)
# FM: giants from 65 occurrences, folded in ranges of 64 (kFmGiantMin, kFmRange)
FM_EDGE_COUNTS = (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 15, 16, 17, 63, 64, 65, 66, 127, 128, 129)


def occurrence_block(n_fields, counts, n_rows, seed=0):
    """A regular block (one entry per field and row, fields in order) in which feature number i of
    `counts` occurs exactly counts[i] times.  Features are dealt to the fields largest first, each to
    the least loaded field; every field's leftover rows get ids that occur nowhere else.  Field f
    owns the ids [f * per, (f + 1) * per) with per = n_rows + 1 (block_ids_per_field).  Returns
    (block, ids, field_of): ids[i] / field_of[i] are feature i's id and field."""
    F = int(n_fields)
    per = block_ids_per_field(n_rows)
    rng = np.random.default_rng(seed)
    load = np.zeros(F, np.int64)
    ids = np.zeros(len(counts), np.int32)
    field_of = np.zeros(len(counts), np.int32)
    cols = [[] for _ in range(F)]
    for i in sorted(range(len(counts)), key=lambda i: -counts[i]):
        f = int(np.argmin(load))
        assert load[f] + counts[i] <= n_rows, "n_rows too small for the counts"
        ids[i], field_of[i] = f * per + len(cols[f]), f
        cols[f].append(int(counts[i]))
        load[f] += counts[i]
    feat = np.zeros((n_rows, F), np.int32)
    for f in range(F):
        col = np.repeat(np.arange(len(cols[f])), cols[f])
        fill = len(cols[f]) + np.arange(n_rows - col.size)  # once-only ids
        feat[:, f] = f * per + rng.permutation(np.concatenate([col, fill]))
    val = (rng.random((n_rows, F)) + 0.25).astype(np.float32)
    val[rng.random((n_rows, F)) < 0.5] = 1.0
    label = (rng.random(n_rows) < 0.4).astype(np.int32)
    field = np.broadcast_to(np.arange(F, dtype=np.int32), (n_rows, F)).reshape(-1).copy()
    row_ptr = (np.arange(n_rows + 1, dtype=np.int64) * F).astype(np.int32)
    return Csr(row_ptr, field, feat.reshape(-1), val.reshape(-1), label), ids, field_of


def block_ids_per_field(n_rows):
    return int(n_rows) + 1


def irregular_copy(blk, seed=0, n_reversed=64):
    """The block made irregular: a third of its rows lose their entry of one field (the field with
    the most once-only ids; only such entries go, so every other feature keeps its count), and
    `n_reversed` rows list their entries in reverse field order."""
    rng = np.random.default_rng(seed)
    n_rows = blk.n_rows
    F = int(blk.row_ptr[1] - blk.row_ptr[0])
    feat = blk.feat.reshape(n_rows, F)
    _, inv, cnt = np.unique(blk.feat, return_inverse=True, return_counts=True)
    once_all = (cnt[inv] == 1).reshape(n_rows, F)
    drop_field = int(np.argmax(once_all.sum(0)))
    once = once_all[:, drop_field]
    drop = rng.permutation(np.flatnonzero(once))[: n_rows // 3]
    assert drop.size == n_rows // 3, "not enough once-only entries to drop"
    keep = np.ones((n_rows, F), bool)
    keep[drop, drop_field] = False
    rev = set(rng.choice(n_rows, n_reversed, replace=False).tolist())
    rows_f, rows_i, rows_v, row_ptr = [], [], [], [0]
    fld = blk.field.reshape(n_rows, F)
    val = blk.val.reshape(n_rows, F)
    for r in range(n_rows):
        cols = np.flatnonzero(keep[r])
        if r in rev:
            cols = cols[::-1]
        rows_f.append(fld[r, cols])
        rows_i.append(feat[r, cols])
        rows_v.append(val[r, cols])
        row_ptr.append(row_ptr[-1] + cols.size)
    return Csr(np.array(row_ptr, np.int32), np.concatenate(rows_f).astype(np.int32),
               np.concatenate(rows_i).astype(np.int32), np.concatenate(rows_v).astype(np.float32),
               blk.label.copy())


# The entry counts of a row at which a row kernel changes path, each edge with its neighbours:
# 0 (no entry: the bias alone; row 0 stores the refreshed bias) | 1, 2, 3 (fm_row_wave_kernel: a
# partly filled parking step, kFmPark = 4) | 4, 5 (all parked | the first chunk of kFmChunk = 8) | 12,
# 13 (4 + 8: a whole chunk | one entry of the next), 11, 20 (partial and whole chunks; the lengths the
# older suites use) | 31, 32, 33 (half a wave of entries) | 63, 64, 65, 66 (fm_row_wave_kernel: the
# linear part runs lane = entry, 64 per pass -- a later pass reads lin_n / lin_z / lin_w back;
# ffm_row_wave_kernel: staging passes of 64 entries, the survivors compacted across them;
# ffm_row_kernel: 64 entries are 2016 pairs, one pass under kTermsCap = 2048, 65 are 2080, two) | 71,
# 72 (where the older suites' long rows begin) | 91, 92 (ffm_row_kernel: 4095 pairs, two passes | 4186,
# three) | 127, 128, 129, 130 (kPredLdsCap = 128: a longer row is the second predict launch's, and a
# third 64-entry pass of the FM linear part) | 150 (the longest row an older suite feeds).
ROW_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 11, 12, 13, 20, 31, 32, 33, 63, 64, 65, 66, 71, 72, 91, 92, 127, 128,
               129, 130, 150)
ROW_POOL = 48                        # ids per field shared by all rows of a row_length_block
ROW_ERASED_AT = (0, 3, 4, 63, 64)    # positions erased in every fifth non-empty row (clamped to the last)
ROW_CAPS = (1, 3, 5, 64, 65, 128, 129, 150)  # row_cap_prefixes: the longest row of each piece
ROW_POSITION_CLASSES = ((0, 4), (4, 12), (12, 64), (64, 128), (128, 1 << 30))


ROW_FIELDS, ROW_IDS_PER_FIELD = 6, 2000  # the model of the row-length cases: 12000 features
# (model type, factors, hyper-parameters, learning variant) of tests/test_gpu_row_lengths.py; the CPU
# side (tests/test_block_semantics.py) checks that the oracle stays finite on every one of them
ROW_SHAPES = ([("FM", k, "stress_hp", False) for k in (8, 33, 64, 65, 128)] + [("LR", 1, "stress_hp", False)]
              + [("FFM", k, "stress_hp", False) for k in (4, 6, 12, 16, 64)]
              + [("FFM", 16, "default_hp", False), ("FM", 8, "default_hp", False),
                 ("FM", 8, "stress_hp", True), ("FFM", 16, "stress_hp", True)])


# the shapes whose every entry point is compared (host calls on the whole block and on its row-cap
# pieces, device calls, the split step)
ROW_ENTRY_SHAPES = [("FM", 8, "stress_hp", False), ("FM", 128, "stress_hp", False), ("LR", 1, "stress_hp", False),
                    ("FFM", 16, "stress_hp", False)]



def row_pieces_shape(shape):
    """The shape with which the row-cap pieces are chained (16 training blocks that hold the short rows
    up to eight times each).  FM takes HP_SETS["alpha_0.05"] there: under the stress set its logits
    reach 65 (k = 8) and pass 2000 (k = 128) along the chain (the oracle on the CPU; sigmoid saturated,
    the logloss inf / NaN), with alpha = 0.05 and l2 = 1 they stay below 11.  LR and FFM keep their set
    (|logit| < 6)."""
    mt, k, hp_name, learn = shape
    return (mt, k, "alpha_0.05", learn) if mt == "FM" else shape


ROW_SEED = 40  # the cases' blocks are row_length_block seeds ROW_SEED, + 1 (trained), + 2 (predicted)


def row_shape_id(shape):
    mt, k, hp_name, learn = shape
    return "%s-k%d-%s%s" % (mt, k, hp_name, "-learn" if learn else "")


def row_length_case(shape, seed):
    """(oracle model with the warm start state set, that state, three row_length_blocks of seeds seed,
    seed + 1, seed + 2, n_feats) of one row-length case: two blocks to train, one to predict."""
    mt, k, hp_name, learn = shape
    blocks = [row_length_block(mt, ROW_FIELDS, ROW_IDS_PER_FIELD, seed + j)[0] for j in range(3)]
    nf = ROW_FIELDS * ROW_IDS_PER_FIELD
    o = CpuModel("oracle", mt, nf, ROW_FIELDS if mt == "FFM" else 1, k, learn=learn, **HP_SETS[hp_name])
    st = row_length_state(o, seed + 100)
    o.set_state(st)
    return o, st, blocks, nf


def take_rows(blk, idx):
    """The block's rows `idx`, in that order."""
    idx = np.asarray(idx, np.int64)
    lens = np.diff(blk.row_ptr)[idx]
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pos = np.concatenate([np.arange(blk.row_ptr[r], blk.row_ptr[r + 1]) for r in idx] + [np.zeros(0, np.int64)])
    pos = pos.astype(np.int64)
    return Csr(row_ptr, blk.field[pos].copy(), blk.feat[pos].copy(), blk.val[pos].copy(), blk.label[idx].copy())


def row_length_block(model_type, n_fields, ids_per_field, seed, lengths=ROW_LENGTHS, repeats=3):
    """A block whose rows have every length of `lengths`, `repeats` times each, in shuffled order,
    between an empty first row and two last rows of 0 and 1 entries (one more two-entry row where
    the count would be a multiple of 4, the rows per workgroup of both wave kernels).  Returns
    (block, n_feats), n_feats = n_fields * ids_per_field; id i belongs to field i // ids_per_field
    (FM / LR: the field array is 0 everywhere).

    * Each entry is, by a fair coin, an id that occurs nowhere else in the block (the in-row
      once-only update) or one of a pool of ROW_POOL ids per field shared by all rows (the update
      kernels); no id twice in a row, so FFM's fields repeat within a row (serial slots).
    * FFM: every seventh non-empty row lists its entries in descending field order.
    * Every third row of at least 66 entries holds one id twice: the entry at a position in [5, 62]
      again at a position from 65 on (the touch-by-touch walk).
    * Every fifth non-empty row (all three counted in ladder order, whatever the seed: rows of 1, 3,
      64, 128, 130 and 150 entries among them) has the entries at ROW_ERASED_AT (clamped to its last entry) replaced
      by out-of-range ones: id -7 or n_feats + 3, in every other such row of FFM an out-of-range field
      (n_fields + 2 or -1, the id kept).  The row's length still counts them.
    * Values: 1.0 for half of the entries, uniform in [0.25, 1.25) otherwise; labels 1 in four of ten."""
    rng = np.random.default_rng(seed)
    F, per = int(n_fields), int(ids_per_field)
    nf = F * per
    ffm = model_type == "FFM"
    assert per > ROW_POOL
    # what each row is, counted over the non-empty rows in ladder order (so that which lengths are
    # erased, reversed or hold an id twice does not depend on the seed): (length, erased, descending, twice)
    specs, n_nonempty, n_long = [], 0, 0
    for n in np.repeat(np.asarray(lengths, np.int64), repeats).tolist():
        erased = n_nonempty // 5 if n > 0 and n_nonempty % 5 == 2 else -1
        specs.append((n, erased, ffm and n > 0 and n_nonempty % 7 == 3, n >= 66 and n_long % 3 == 0))
        n_nonempty += n > 0
        n_long += n >= 66
    specs = [specs[j] for j in rng.permutation(len(specs))]
    plain = lambda n: (n, -1, False, False)  # noqa: E731
    specs = [plain(0)] + ([plain(2)] if (len(specs) + 3) % 4 == 0 else []) + specs + [plain(0), plain(1)]
    lens = np.array([sp[0] for sp in specs], np.int64)
    pool = (np.arange(F)[:, None] * per + np.arange(ROW_POOL)[None, :]).reshape(-1)
    fresh = rng.permutation(np.setdiff1d(np.arange(nf), pool))
    assert fresh.size >= lens.sum(), "ids_per_field too small for once-only ids"
    n_fresh = 0
    fields, feats = [], []
    for n, k5, descending, twice in specs:
        once = rng.random(n) < 0.5
        ids = np.empty(n, np.int64)
        ids[once] = fresh[n_fresh:n_fresh + int(once.sum())]
        n_fresh += int(once.sum())
        ids[~once] = rng.choice(pool, int((~once).sum()), replace=False)
        fld = ids // per
        if descending:
            order = np.argsort(-fld, kind="stable")
            ids, fld = ids[order], fld[order]
        if twice:
            lo, hi = int(rng.integers(5, 63)), int(rng.integers(65, n))
            ids[hi], fld[hi] = ids[lo], fld[lo]
        if k5 >= 0:
            for j, p in enumerate(sorted({min(p, n - 1) for p in ROW_ERASED_AT})):
                if ffm and k5 % 2 == 1:
                    fld[p] = F + 2 if (j + k5 // 2) % 2 == 0 else -1
                else:
                    ids[p] = -7 if (j + k5) % 2 == 0 else nf + 3
        fields.append(fld)
        feats.append(ids)
    nnz = int(lens.sum())
    val = (rng.random(nnz) + 0.25).astype(np.float32)
    val[rng.random(nnz) < 0.5] = 1.0
    label = (rng.random(lens.size) < 0.4).astype(np.int32)
    field = np.concatenate(fields).astype(np.int32)
    if not ffm:
        field[:] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return Csr(row_ptr, field, np.concatenate(feats).astype(np.int32), val, label), nf


def row_cap_prefixes(blk, caps=ROW_CAPS):
    """The block's rows in a stable order by length, cut after the last row of exactly L entries, for
    each L of `caps`: pieces whose longest row is L, each beginning with the block's empty rows.  An
    entry point that sizes its kernels by the longest row of the block runs with that row cap."""
    lens = np.diff(blk.row_ptr)
    order = np.argsort(lens, kind="stable")
    for cap in caps:
        assert (lens == cap).any() and lens[order[0]] == 0
        yield take_rows(blk, order[:int(np.searchsorted(lens[order], cap, side="right"))])


def row_length_state(model, seed):
    """The warm start state of the row-length cases: rand_state with 0.05 added to vec_n and lin_n."""
    st = rand_state(np.random.default_rng(seed), model)
    for key in ("vec_n", "lin_n"):
        st[key] += np.float32(0.05)
    return st


def row_lengths_of(blk, what):
    """' (rows of N entries)' for the row index / the feature id `what` = ("row", r) / ("feat", i): the
    length of that row, or the lengths of the rows that hold the feature."""
    lens = np.diff(blk.row_ptr)
    if what[0] == "row":
        return "rows of %d entries (row %d)" % (lens[what[1]], what[1])
    row_of = np.repeat(np.arange(blk.n_rows), lens)
    held = sorted(set(lens[row_of[blk.feat == what[1]]].tolist()))
    return "feature %d, held by rows of %s entries" % (what[1], "/".join(map(str, held)) or "no")


def _first_difference(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    both_nan = (np.isnan(a) & np.isnan(b)).ravel()
    bad = np.flatnonzero((bits(a).ravel() != bits(b).ravel()) & ~both_nan)
    return int(bad[0]) if bad.size else None


def assert_rows_bitwise(got, want, blk, what):
    """assert_bitwise on one value per row of `blk`; the message names the first differing row's length
    and every length that differs."""
    try:
        assert_bitwise(got, want, what)
    except AssertionError as err:
        a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
        lens = np.diff(blk.row_ptr)
        bad = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
        raise AssertionError("%s: first in %s; differing row lengths %s" % (
            err, row_lengths_of(blk, ("row", _first_difference(got, want))),
            sorted(set(lens[bad].tolist())))) from None


def assert_state_rows_bitwise(got, want, blk, what):
    """assert_state_bitwise; the message names the lengths of the rows that hold the first differing
    feature (the bias belongs to every row)."""
    for key in STATE_KEYS:
        try:
            assert_bitwise(got[key], want[key], what + ":" + key)
        except AssertionError as err:
            if key == "bias3":
                raise
            at = _first_difference(got[key], want[key])
            width = got[key].shape[1] if got[key].ndim == 2 else 1
            raise AssertionError("%s: %s" % (err, row_lengths_of(blk, ("feat", at // width)))) from None


LOSS_RTOL = 1e-12


def loss_close(a, b):
    """Double logloss sums: device exp / log may differ from glibc in the last ulp, so |gpu - cpu| <=
    1e-12 * max(1, |cpu|) per row summed (64 rows' worth); NaN with NaN, an infinity with itself."""
    if np.isnan(a) or np.isnan(b):
        return np.isnan(a) and np.isnan(b)
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= LOSS_RTOL * max(1.0, abs(b)) * 64


def fast_state(rng, model, n_hi=1.0, n_add=0.0, z_sd=0.3, w_sd=0.02, n_zero=0.0):
    """rand_state drawn in float32 (large models): n ~ U(0, n_hi) + n_add, a fraction n_zero of
    vec_n set to 0, z ~ N(0, z_sd), w ~ N(0, w_sd)."""
    st = model.zero_state()
    for k in st:
        if k == "bias3":
            continue
        a = st[k]
        if k.endswith("_n"):
            rng.random(a.shape, dtype=np.float32, out=a)
            a *= np.float32(n_hi)
            a += np.float32(n_add)
        else:
            rng.standard_normal(a.shape, dtype=np.float32, out=a)
            a *= np.float32(z_sd if k.endswith("_z") else w_sd)
    if n_zero > 0 and st["vec_n"].size:
        st["vec_n"][rng.random(st["vec_n"].shape, dtype=np.float32) < n_zero] = 0.0
    st["bias3"][...] = np.array([0.013, 0.7, -0.4], np.float32)
    return st


def ftrl_w(n, z, hp):
    """FtrlModel::maybe_zero_weight (ftrl_model.h:28-33) with T = float, one value: float32
    operands; the 0.0 / -1.0 literals make the divide a double one, narrowed to float on return."""
    f = np.float32
    n, z = f(n), f(z)
    a, b, l1, l2 = (f(hp[key]) for key in ("w_alpha", "w_beta", "w_l1", "w_l2"))
    if abs(z) <= l1:
        return f(0.0)
    with np.errstate(all="ignore"):
        num = f(z - f((f(1) if z > 0 else f(-1)) * l1))
        den = f(l2 + f(f(b + np.sqrt(n)) / a))
        return f(np.float64(-1.0) * np.float64(num) / np.float64(den))  # (IEEE: x / 0 is inf or NaN)


def latent_w(n, z, w_old, hp, learn):
    """The latent refresh: W(n, z); under the learning variant a slot without a gradient yet
    (not n > 0: zero, negative or NaN) keeps its stored weight."""
    return np.float32(w_old) if learn and not (np.float32(n) > 0) else ftrl_w(n, z, hp)


def special_grid(hp, seed=0):
    """(n, z, w_old) float32 arrays over the special values of the refresh rule: n in
    {+0, -0, 2^-149, the largest subnormal, FLT_MIN, 1e-30, 0.5, +inf, NaN} x z in {+-0, +-l1,
    +-nextafter(l1, inf), +-0.3} x w_old in {N(0, 0.02), -0.0, a subnormal, NaN}."""
    f = np.float32
    tiny = np.finfo(f).tiny
    ns = np.array([0.0, -0.0, f(2.0 ** -149), np.nextafter(tiny, f(0)), tiny, 1e-30, 0.5, np.inf,
                   np.nan], f)
    l1 = f(hp["w_l1"])
    zs = np.array([s * v for v in (f(0), l1, np.nextafter(l1, f(np.inf)), f(0.3)) for s in (1, -1)], f)
    rng = np.random.default_rng(seed)
    n, z, w = [], [], []
    for wk in range(4):
        for a in ns:
            for b in zs:
                n.append(a)
                z.append(b)
                w.append((f(rng.normal(0, 0.02)), f(-0.0), f(3e-41), f(np.nan))[wk])
    return np.array(n, f), np.array(z, f), np.array(w, f)


def range_grid(hp, seed=0):
    """A second grid, laid out like special_grid, on the operand guards of the short square root and
    divide: n in {every guard edge 2^-96, 2^-70, 2^96 with its two neighbours, 2^118, FLT_MAX} x z in
    {special_grid's z, +-2^61 (a divide operand above 2^60)} x the same four kinds of w_old."""
    f = np.float32
    ns = []
    for e in (-96, -70, 96):
        v = f(2.0 ** e)
        ns += [np.nextafter(v, f(0)), v, np.nextafter(v, f(np.inf))]
    ns = np.array(ns + [f(2.0 ** 118), np.finfo(f).max], f)
    l1 = f(hp["w_l1"])
    zs = np.array([s * v for v in (f(0), l1, np.nextafter(l1, f(np.inf)), f(0.3), f(2.0 ** 61)) for s in (1, -1)], f)
    rng = np.random.default_rng(seed)
    n, z, w = [], [], []
    for wk in range(4):
        for a in ns:
            for b in zs:
                n.append(a)
                z.append(b)
                w.append((f(rng.normal(0, 0.02)), f(-0.0), f(3e-41), f(np.nan))[wk])
    return np.array(n, f), np.array(z, f), np.array(w, f)


def grid_block(mt, k, hp, occurrences=1, seed=0, grid=None):
    """A grid of (n, z, w_old) -- special_grid(hp, seed) unless `grid` gives another -- injected into a zero model as latent and as linear accumulators, and a block
    that touches each of them `occurrences` times.  FFM (F = 2): field 0 holds ids [0, P), field 1
    ids [P, nf); row r pairs ids r and P + r, so the slot of the other field is touched.  FM: row r
    holds ids 2r and 2r + 1, every factor touched.  Then rows of one entry each (FFM: in field 1)
    touch the ids that carry the linear grid and no latent slot of the grid.  Returns a dict:
    nf, F, k, state, block, field_start, slots (the latent elements (rows, columns) of the grid),
    idx (their grid index), lin (linear ids), lidx (their grid index), n, z, w (the grid)."""
    gn, gz, gw = special_grid(hp, seed) if grid is None else grid
    N = len(gn)
    F = 2 if mt == "FFM" else 1
    P = -(-N // k)  # latent rows per field (FFM) / latent features (FM, rounded up to pairs)
    P += mt == "FM" and P % 2
    nlat = 2 * P if mt == "FFM" else P
    lin = np.arange(nlat, nlat + N // 4)  # (n, z) pairs: w_old does not enter the linear rule
    nf = nlat + lin.size
    st = dict(bias3=np.zeros(3, np.float32), lin_w=np.zeros(nf, np.float32),
              lin_n=np.zeros(nf, np.float32), lin_z=np.zeros(nf, np.float32))
    for key in ("vec_w", "vec_n", "vec_z"):
        st[key] = np.zeros((nf, F * k), np.float32)
    if mt == "FFM":
        slots = [(i, (1 if i < P else 0) * k + f) for i in range(2 * P) for f in range(k)]
        rows = [[(0, r, 1.0), (1, P + r, 0.5)] for r in range(P)]
    else:
        slots = [(i, f) for i in range(P) for f in range(k)]
        rows = [[(0, 2 * r, 1.0), (0, 2 * r + 1, 0.5)] for r in range(P // 2)]
    rows += [[(F - 1, int(i), 1.0)] for i in lin]
    idx = np.arange(len(slots)) % N
    rc = np.array([a for a, _ in slots]), np.array([b for _, b in slots])
    st["vec_n"][rc], st["vec_z"][rc], st["vec_w"][rc] = gn[idx], gz[idx], gw[idx]
    lidx = np.arange(lin.size)
    st["lin_n"][lin], st["lin_z"][lin], st["lin_w"][lin] = gn[lidx], gz[lidx], gw[lidx]
    rows = [r for r in rows for _ in range(occurrences)]
    c = Csr.from_rows(rows, [r % 2 for r in range(len(rows))])
    fs = np.array([0, P, nf], np.int32) if mt == "FFM" else None
    return dict(nf=nf, F=F, k=k, state=st, block=c, field_start=fs, slots=rc, idx=idx, lin=lin,
                lidx=lidx, n=gn, z=gz, w=gw)


def grid_want(g, hp, learn):
    """The w the refresh stores in grid_block's latent slots and linear ids (latent_w, ftrl_w)."""
    n, z, w = g["n"], g["z"], g["w"]
    lat = np.array([latent_w(n[j], z[j], w[j], hp, learn) for j in g["idx"]], np.float32)
    lin = np.array([ftrl_w(n[j], z[j], hp) for j in g["lidx"]], np.float32)
    return lat, lin


def _f32p(a):
    import ctypes
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def set_bias3(e, b3):
    """The bias and its (n, z) of an engine, without the dense transfers of set_state."""
    b = np.ascontiguousarray(b3, np.float32)
    e._check(e.lib.ffm_engine_set_weights(e.h, _f32p(b[0:1]), None, None))
    e._check(e.lib.ffm_engine_set_state(e.h, _f32p(b[1:2]), _f32p(b[2:3]), None, None, None, None))


def get_bias3(e):
    b = np.zeros(3, np.float32)
    e._check(e.lib.ffm_engine_get_weights(e.h, _f32p(b[0:1]), None, None))
    e._check(e.lib.ffm_engine_get_state(e.h, _f32p(b[1:2]), _f32p(b[2:3]), None, None, None, None))
    return b


def keep_columns(plan, rank):
    """The fields a compact shard looks at (bench.py's loader rule): those it owns a pair or the
    linear terms of."""
    return (plan["pair_owner"] == rank).any(axis=1) | (plan["lin_owner"] == rank)


def kept_copy(blk, keep):
    """The block with only the entries of the kept fields (rows keep their order and labels)."""
    sel = keep[blk.field]
    row_of = np.repeat(np.arange(blk.n_rows), np.diff(blk.row_ptr))
    per_row = np.bincount(row_of[sel], minlength=blk.n_rows)
    return Csr(np.concatenate([[0], np.cumsum(per_row)]).astype(np.int32), blk.field[sel].copy(),
               blk.feat[sel].copy(), blk.val[sel].copy(), blk.label.copy())


def run_rank_staged(e, blocks, logits, ahead=2, after_step=None):
    """One emulated rank the way bench.py drives it: blocks staged up to `ahead` in front, each
    step train_forward_staged -> (the all-reduce, here: the given exact logits) ->
    train_update_device.  Returns the rank's partial logits per block."""
    import torch
    buf = torch.zeros(max(b.n_rows for b in blocks), dtype=torch.float32, device="cuda")
    parts, staged = [], 0
    for i, b in enumerate(blocks):
        while staged < min(i + 1 + ahead, len(blocks)):
            e.stage_batch(blocks[staged])
            staged += 1
        e.train_forward_staged(buf.data_ptr())
        e.sync()
        parts.append(buf[:b.n_rows].cpu().numpy().copy())
        buf[:b.n_rows].copy_(torch.from_numpy(np.ascontiguousarray(logits[i], np.float32)))
        torch.cuda.synchronize()
        e.train_update_device(buf.data_ptr())
        e.sync()
        if after_step is not None:
            after_step(i)
    return parts


def assert_rank_rows(e, rank, ids, field_of, want, plan, k, what, chunk=16384):
    """A compact shard's rows of features `ids` (ascending, so grouped by their fields `field_of`):
    the latent elements and linear terms it owns equal want[key][j] (row j of the expected state,
    any array-like a slice indexes) bit for bit, the latent elements it does not own read back zero.
    Compared field by field, a chunk of features at a time."""
    po, lin_owner = plan["pair_owner"], plan["lin_owner"]
    bounds = np.searchsorted(field_of, np.arange(po.shape[0] + 1))
    for f in range(po.shape[0]):
        cols = np.repeat(po[f] == rank, k)
        for lo in range(bounds[f], bounds[f + 1], chunk):
            hi = min(bounds[f + 1], lo + chunk)
            got = e.get_rows(ids[lo:hi])
            for key in ("vec_n", "vec_z", "vec_w"):
                assert_bitwise(got[key][:, cols], np.asarray(want[key][lo:hi])[:, cols],
                               "%s rank %d field %d %s" % (what, rank, f, key))
                assert not got[key][:, ~cols].any(), "%s rank %d field %d %s: unowned slots not zero" % (
                    what, rank, f, key)
            if lin_owner[f] == rank:
                for key in ("lin_n", "lin_z", "lin_w"):
                    assert_bitwise(got[key], np.asarray(want[key][lo:hi]), "%s rank %d field %d %s" % (
                        what, rank, f, key))


# ---- tables past 2^31 and 2^32 elements (tests/test_gpu_big_offsets.py, tests/test_big_offsets_host.py) ----------
# FFM 39 x 16: a feature's record is 624 elements in a serving table (fp16: 2 bytes each, fp32: 4) and 3 * 624 in
# a training engine ([n][z][w], 4 bytes each).  FM k = 64 training engine: 3 * 64.
BIG_F, BIG_K, BIG_L = 39, 16, 624
BIG_LAYOUTS = {"f16": (BIG_L, 2), "f32": (BIG_L, 4), "train": (3 * BIG_L, 4)}  # kind -> (stride in elements, element bytes)
BIG_FM_K, BIG_FM_STRIDE = 64, 3 * 64
BIG_HP = STRESS_HP  # weights that move (W(n, z) ~ 1e-2); with n >= BIG_N_ADD the oracle stays finite (checked on the CPU)
BIG_N_ADD = 0.05


def count_past(limit, stride, n_whole=8):
    """The smallest feature count with at least n_whole records wholly at or past element `limit`."""
    return -(-int(limit) // int(stride)) + int(n_whole)


BIG_NF = count_past(2 ** 32, BIG_L)                # 6 882 969
BIG_NF_FM = count_past(2 ** 32, BIG_FM_STRIDE)     # 22 369 630
BIG_NF_TRAIN_INIT = count_past(2 ** 32, 3 * BIG_L)  # 2 294 329: a training engine's own layout past 2^32
# The prediction, pack, sync and refresh kernels count in vectors of four factors: their index passes 2^32 at element
# 2^34 -- 27 531 850 features of a serving table (34.4 GB in fp16), 9 177 289 of a training engine (68.7 GB)
BIG_NF_VEC_SERVE = count_past(2 ** 34, BIG_L)
BIG_NF_VEC_TRAIN = count_past(2 ** 34, 3 * BIG_L)


def offset_thresholds(elem_bytes, unit=1):
    """The element offsets at which an index can break: 2^31 and 2^32 as indices counted in units of `unit` elements
    (1: an element index; 4: the index of a vector of four factors, which several kernels count in), and byte offsets
    2^32, 2^33 and 2^34 as the element they fall on."""
    return sorted({2 ** 31 * int(unit), 2 ** 32 * int(unit)} | {2 ** b // int(elem_bytes) for b in (32, 33, 34)})


def straddling_ids(n_feats, stride_elems, elem_bytes, unit=1):
    """The features whose record contains one of offset_thresholds, where that lies inside the table."""
    return sorted({t // int(stride_elems) for t in offset_thresholds(elem_bytes, unit) if t // int(stride_elems) < int(n_feats)})


def edge_ids(n_feats, stride_elems, elem_bytes, unit=1):
    """straddling_ids with both neighbours each (clipped to the table), ascending int64."""
    out = {h + d for h in straddling_ids(n_feats, stride_elems, elem_bytes, unit) for d in (-1, 0, 1)}
    return np.array(sorted(h for h in out if 0 <= h < int(n_feats)), np.int64)


def alias_ids(ids, stride, n_feats, elem_bytes=1, unit=1):
    """The low features a wrapped index of a probe id h would hit: the records that [x, x + stride) overlaps for x =
    h * stride mod 2^32 * unit and mod 2^31 * unit (an index in 32 bits, unsigned or signed, counted in units of `unit`
    elements), and -- with elem_bytes > 1 -- mod 2^32 / elem_bytes (a byte offset in 32 bits).  Only those that are no
    probe ids themselves and lie in the table."""
    stride, probes = int(stride), {int(h) for h in ids}
    mods = {2 ** 32 * int(unit), 2 ** 31 * int(unit)} | ({2 ** 32 // int(elem_bytes)} if elem_bytes > 1 else set())
    out = set()
    for h in probes:
        for m in mods:
            x = h * stride % m
            out.update((x // stride, (x + stride - 1) // stride))
    return np.array(sorted(a for a in out if a not in probes and 0 <= a < int(n_feats)), np.int64)


def offset_tier(ids, stride, unit=1):
    """Per id: 0 = the record lies wholly below index 2^31 (counted in units of `unit` elements), 1 = wholly in [2^31,
    2^32), 2 = wholly at or past 2^32, -1 = it straddles one of the two."""
    lo = np.asarray(ids, np.int64) * int(stride)
    hi = lo + int(stride)
    a, b = 2 ** 31 * int(unit), 2 ** 32 * int(unit)
    return np.where(hi <= a, 0, np.where((lo >= a) & (hi <= b), 1, np.where(lo >= b, 2, -1)))


def big_probe_ids(n_feats, layouts, seed, n_random=200, unit=1):
    """The probe set of a table of n_feats features read under `layouts` [(stride, element bytes)]: edge_ids of every
    layout; ids 0, 1 and n_feats - 1; the 8 records wholly past 2^32 at the smallest stride; the ids next to the last
    edge between two 64-feature bitmap words, and n_feats - 1 - 64 (64 apart from the last id, across that edge); and
    n_random ids drawn uniformly over [0, n_feats).  Ascending int64, no id twice."""
    n = int(n_feats)
    w0 = (n - 1) // 64 * 64
    parts = [edge_ids(n, s, b, u) for s, b in layouts for u in {1, unit}]
    parts += [np.array([0, 1, n - 1, w0 - 1, w0, n - 1 - 64], np.int64), np.arange(n - 8, n, dtype=np.int64),
              np.random.default_rng(seed).integers(0, n, n_random)]
    return np.unique(np.concatenate(parts).astype(np.int64))


class BigCase:
    """One model too large to hold twice, and its id-remapped compact twin for the oracle (renaming ids is exact for FFM
    and FM: the arithmetic depends on (field, record) only).

    probes: the probe ids, ascending.  Probe number j belongs to field j % F and is compact id (j % F) * per + j // F, so
    that field f owns the compact ids [f * per, (f + 1) * per) -- the layout drop_pair_weights' callers expect (FM: the
    fields only deal the ids to the columns of a row; the block's field array is 0).
    block / compact_block: ~64 rows of one entry per column with ids from the probe set, an empty row and a row that
    holds one entry twice, under the big ids / the compact ones.
    state: rand_state on the compact oracle, BIG_N_ADD added to n; rows(): the probes' rows of it, in probe order."""

    def __init__(self, mt, n_feats, k, layouts, seed, n_rows=64, hp=None, unit=1, tier_kinds=None):
        """unit: the tiers (and the block's mix of them) are those of an index counted in units of `unit` elements;
        tier_kinds: the layouts whose tiers the table reaches (default: all)."""
        self.mt, self.n_feats, self.k, self.layouts, self.seed = mt, int(n_feats), int(k), dict(layouts), seed
        self.unit, self.tier_kinds = int(unit), tuple(tier_kinds or layouts)
        self.F = BIG_F
        self.hp = dict(hp or BIG_HP)
        self.probes = big_probe_ids(n_feats, list(self.layouts.values()), seed, unit=self.unit)
        assert self.probes[-1] < 2 ** 31
        P = self.probes.size
        self.per = -(-P // self.F)
        rank = np.arange(P)
        self.field_of = (rank % self.F).astype(np.int32)
        self.compact = (self.field_of.astype(np.int64) * self.per + rank // self.F).astype(np.int32)
        self.n_compact = self.F * self.per
        self.probes32 = self.probes.astype(np.int32)
        self.block = self._block(n_rows, seed + 1)
        self.compact_block = self.remap(self.block)
        o = self.oracle()
        st = rand_state(np.random.default_rng(seed + 2), o)
        st["vec_n"] += np.float32(BIG_N_ADD)
        st["lin_n"] += np.float32(BIG_N_ADD)
        for a in st.values():
            a.setflags(write=False)
        self.state = st

    def oracle(self, state=None, **weights):
        """A compact oracle holding `state` (or nothing yet); weights: arrays that replace the state's."""
        o = CpuModel("oracle", self.mt, self.n_compact, self.F if self.mt == "FFM" else 1, self.k, **self.hp)
        if state is not None:
            o.set_state(dict(state, **weights))
        return o

    def weights_oracle(self, vec_w, lin_w=None, bias=None):
        """A compact oracle that holds weights alone (what a serving engine holds): (n, z) zero."""
        o = self.oracle()
        z = o.zero_state()
        z["bias3"][0] = self.state["bias3"][0] if bias is None else bias
        z["lin_w"][...] = self.state["lin_w"] if lin_w is None else lin_w
        z["vec_w"][...] = vec_w
        o.set_state(z)
        return o

    def compact_of(self, ids):
        at = np.searchsorted(self.probes, np.asarray(ids, np.int64))
        assert np.array_equal(self.probes[at], np.asarray(ids, np.int64)), "an id outside the probe set"
        return self.compact[at]

    def remap(self, blk):
        return Csr(blk.row_ptr, blk.field, self.compact_of(blk.feat), blk.val, blk.label)

    def rows(self, state=None, keys=None, ids=None):
        """{key: the rows of the compact `state` (default: the start state) for the probe ids (or `ids`)}."""
        state = self.state if state is None else state
        at = self.compact if ids is None else self.compact_of(ids)
        return {key: np.ascontiguousarray(state[key][at]) for key in (keys or ("lin_w", "lin_n", "lin_z", "vec_w", "vec_n", "vec_z"))}

    def straddlers(self):
        return sorted({h for s, b in self.layouts.values() for u in {1, self.unit} for h in straddling_ids(self.n_feats, s, b, u)})

    def tiers(self, kind, ids=None):
        return offset_tier(self.probes if ids is None else ids, self.layouts[kind][0], self.unit)

    def aliases(self, kind):
        """alias_ids of the probes under layout `kind`: wraps of an element index and of this case's unit."""
        stride, eb = self.layouts[kind]
        out = [alias_ids(self.probes, stride, self.n_feats, eb, u) for u in {1, self.unit}]
        return np.unique(np.concatenate(out)).astype(np.int32)

    def _block(self, n_rows, seed):
        """Each entry: a tier of the smallest-stride layout drawn uniformly among those the column's ids have, then an
        id of it; every row gets an id past 2^32 in every layout; every straddling id is placed once."""
        rng = np.random.default_rng(seed)
        F = self.F
        stride0 = min(self.layouts[kind][0] for kind in self.tier_kinds)
        tier0 = offset_tier(self.probes, stride0, self.unit)
        cols = [np.flatnonzero(self.field_of == f) for f in range(F)]
        top = np.flatnonzero(tier0 == 2)
        feat = np.zeros((n_rows, F), np.int64)
        for r in range(n_rows):
            for f in range(F):
                t = rng.choice(np.unique(tier0[cols[f]]))
                feat[r, f] = self.probes[rng.choice(cols[f][tier0[cols[f]] == t])]
        strad = self.straddlers()
        assert len(strad) <= n_rows
        held = np.full(n_rows, -1)  # the column of the row's straddling id
        for r, h in enumerate(strad):
            j = int(np.searchsorted(self.probes, h))
            held[r] = self.field_of[j]
            feat[r, held[r]] = h
        for r in range(n_rows):
            if not np.isin(feat[r], self.probes[top]).any():
                j = int(rng.choice(top[self.field_of[top] != held[r]]))
                feat[r, self.field_of[j]] = self.probes[j]
        val = (rng.random((n_rows, F)) + 0.25).astype(np.float32)
        val[rng.random((n_rows, F)) < 0.5] = 1.0
        rows = [[(f if self.mt == "FFM" else 0, int(feat[r, f]), float(val[r, f])) for f in range(F)] for r in range(n_rows)]
        twice = list(rows[n_rows // 2])
        twice.append(twice[5])  # one (field, id) again, at the row's end
        rows = rows[:n_rows // 3] + [[]] + rows[n_rows // 3:] + [twice]
        label = (rng.random(len(rows)) < 0.4).astype(np.int32)
        return Csr.from_rows(rows, label)


_BIG_CASES = {}


def big_case(name):
    """"ffm": FFM 39 x 16 at BIG_NF under the three layouts; "fm": FM k = 64 at BIG_NF_FM (training engine); "vec_serve" /
    "vec_train": FFM 39 x 16 at BIG_NF_VEC_SERVE / BIG_NF_VEC_TRAIN, where the index of a vector of four factors passes
    2^32 in a serving table / in a training engine's records (an fp16 table of the latter count stays below 2^31
    vectors: it is the destination of pack_from and sync_from there).  Built once per process; read-only."""
    if name not in _BIG_CASES:
        if name == "ffm":
            _BIG_CASES[name] = BigCase("FFM", BIG_NF, BIG_K, BIG_LAYOUTS, seed=31)
        elif name == "vec_serve":
            _BIG_CASES[name] = BigCase("FFM", BIG_NF_VEC_SERVE, BIG_K, {"f16": BIG_LAYOUTS["f16"]}, seed=41, unit=4)
        elif name == "vec_train":
            _BIG_CASES[name] = BigCase("FFM", BIG_NF_VEC_TRAIN, BIG_K, {"train": BIG_LAYOUTS["train"], "f16": BIG_LAYOUTS["f16"]},
                                       seed=43, unit=4, tier_kinds=("train",))
        else:
            _BIG_CASES[name] = BigCase("FM", BIG_NF_FM, BIG_FM_K, {"train": (BIG_FM_STRIDE, 4)}, seed=37)
    return _BIG_CASES[name]


def big_tier_entries(case, kind):
    """{tier: the block's entries whose record lies in it} under layout `kind` (-1: straddling)."""
    t = case.tiers(kind, case.block.feat)
    return {int(v): int((t == v).sum()) for v in (-1, 0, 1, 2)}


def big_upper_zeroed(case, kind, tiers=(1, 2, -1)):
    """(vec_w, lin_w) of the start state with the weights of the probe ids in the given tiers of layout `kind` zeroed
    (default: everything not wholly below 2^31)."""
    hit = case.compact[np.isin(case.tiers(kind), tiers)]
    vw, lw = case.state["vec_w"].copy(), case.state["lin_w"].copy()
    vw[hit] = 0
    lw[hit] = 0
    return vw, lw


def big_step(case):
    """(logits, loss sum, state after) of one oracle train_batch of the block from the start state."""
    o = case.oracle(case.state)
    lg, ls = o.train_batch(case.compact_block)
    return lg, ls, o.get_state()


def nonfinite_share(logits, st0, st1):
    """(share of non-finite logits, share of non-finite words among the state words the step changed, their count)."""
    t = np.concatenate([st1[key].ravel()[bits(st1[key]).ravel() != bits(st0[key]).ravel()] for key in STATE_KEYS])
    return float((~np.isfinite(logits)).mean()), float((~np.isfinite(t)).mean()) if t.size else 0.0, int(t.size)
