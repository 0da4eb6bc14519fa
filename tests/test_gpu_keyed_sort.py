"""The keyed-AUC kernels of csrc/kernels_keyed.h beyond the one shape of test_gpu_keyed_metrics.py: the sort past
one sub-tile per workgroup and the rank scan past one tile per thread, every key width from no key pass to four
(odd pass counts and 1-bit passes among them), exact row counts around the tiles, U2 past 32 bits, and the
capture kernel's eight lanes on rows longer than eight entries.  No tolerances: the tables as integers, the seven
counts as integers, gauc bit for bit against fa.keyed_auc_reference over (keys read off the blocks on the host, the
p the same engine returned with capture off, labels).

Sections 1 to 3 use the smallest model with a key field: FFM, 2 fields, k = 4, everything zero except lin_w[sid]
= 1, rows of [(field 0, key, 1), (field 1, sid, v)] -- the row's logit is its own v (1 + v where key == sid), so p
is not one of five values: a normal body, a slice in [-88.7, -87.0] (p at or below the smallest normal fp32),
+-100 (p exactly 1 or 0), exact repeats of v and one-ulp neighbours of v inside keys.  Every test prints and
asserts what it relies on: distinct bit patterns of p, 0.0, 1.0, a subnormal p (or the statement that the device
flushes them), a tie between a positive and a negative inside a key, and the pass counts its n_feats implies."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block
from test_gpu_keyed_metrics import COUNTS, assert_keyed, bits, from_rows, keys_of

pytestmark = pytest.mark.gpu

TILE = 2048           # kKeyedTile: words per workgroup of the rank pass
THREADS = 256         # kKeyedThreads
SORT_MAX_WG = 2048    # kKeyedSortMaxWg
TINY = np.float32(2.0 ** -126)
BIG_ROWS = 1 << 17
NF_GEOMETRY = 20000


# ---- the two-field model ------------------------------------------------------------------------

def sid_of(nf):
    return nf // 2


def two_field_engine(nf, max_rows, **kw):
    e = fa.Engine("FFM", nf, 2, 4, skip_init=True, max_batch_rows=max_rows, max_batch_nnz=2 * max_rows, **kw)
    e.set_rows(np.array([sid_of(nf)], np.int32), dict(lin_w=np.ones(1, np.float32)))  # (skip_init: all else is zero bits)
    return e


def draw(rng, keys):
    """v and labels for the rows of `keys`: see the module's text.  The last three rows are +100, -100 and -88.5; one
    pair of rows of one key (when there is one) is an exact tie of a positive and a negative."""
    n = keys.size
    v = rng.normal(0.0, 3.0, n).astype(np.float32)
    u = rng.random(n)
    v[u < 0.03] = rng.uniform(-88.7, -87.0, int((u < 0.03).sum())).astype(np.float32)
    v[(u >= 0.03) & (u < 0.04)] = 100.0
    v[(u >= 0.04) & (u < 0.05)] = -100.0
    # neighbours in key order: odd places repeat the even place before them exactly (30 %) or one ulp above (10 %)
    order = np.argsort(keys, kind="stable")
    j = np.arange(1, n, 2)
    j = j[keys[order[j]] == keys[order[j - 1]]]
    c = rng.random(j.size)
    v[order[j[c < 0.3]]] = v[order[j[c < 0.3] - 1]]
    up = j[(c >= 0.3) & (c < 0.4)]
    v[order[up]] = np.nextafter(v[order[up - 1]], np.float32(np.inf))
    label = (rng.random(n) < 1.0 / (1.0 + np.exp(-0.3 * np.clip(v, -10.0, 10.0)))).astype(np.int32)
    if n >= 8:
        v[n - 3:] = (100.0, -100.0, -88.5)
        a, b = order[j - 1], order[j]
        ok = np.flatnonzero((a < n - 3) & (b < n - 3))
        if ok.size:
            a, b = a[ok[0]], b[ok[0]]
            v[b] = v[a]
            label[a], label[b] = 1, 0
    return v, label


def block_of(keys, v, label, nf):
    n = keys.size
    feat = np.empty(2 * n, np.int32)
    feat[0::2] = keys
    feat[1::2] = sid_of(nf)
    val = np.ones(2 * n, np.float32)
    val[1::2] = v
    return Block((np.arange(n + 1) * 2).astype(np.int32), np.tile(np.array([0, 1], np.int32), n), feat, val,
                 np.asarray(label, np.int32))


def drawn_blocks(rng, keys, nf, max_rows):
    keys = np.asarray(keys, np.int64)
    v, label = draw(rng, keys)
    return [block_of(keys[a:a + max_rows], v[a:a + max_rows], label[a:a + max_rows], nf) for a in range(0, keys.size, max_rows)]


def block_keys(b, nf):
    """The keys read off a block of the two-field model: the entry of field 0, which comes first."""
    assert (b.field[0::2] == 0).all() and (b.field[1::2] == 1).all() and b.feat.size == 2 * b.n_rows
    keys = b.feat[0::2].astype(np.int64)
    assert ((keys >= 0) & (keys < nf)).all()
    return keys


def rows_of(blocks, nf):
    if not blocks:
        return np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int32)
    return (np.concatenate([block_keys(b, nf) for b in blocks]), np.concatenate([b.val[1::2] for b in blocks]),
            np.concatenate([b.label for b in blocks]))


def probs(e, blocks):
    return np.concatenate([e.predict_batch(b, output_prob=True)[0] for b in blocks]) if blocks else np.zeros(0, np.float32)


def population(what, keys, v, p, label, n_distinct):
    """What the comparison rests on, printed and asserted on the p the engine returned."""
    distinct = np.unique(p.view(np.uint32)).size
    sub = int(((p > 0) & (p < TINY)).sum())
    w = keys << 32 | p.view(np.uint32).astype(np.int64)
    ties = np.intersect1d(w[label > 0], w[label <= 0]).size
    print("%s: %d rows, %d distinct p, %d of 0.0, %d of 1.0, %d below 2^-126, %d (key, p) runs holding both classes" % (
        what, p.size, distinct, int((p == 0).sum()), int((p == 1).sum()), sub, ties))
    assert not np.isnan(p).any() and distinct >= n_distinct, (what, distinct, n_distinct)
    assert (p == np.float32(0.0)).any() and (p == np.float32(1.0)).any(), what
    if sub == 0:  # every logit at or below -87.5 (v <= -88.5: key == sid adds 1) has a p below 2^-126 unless it is flushed
        print("%s: the device flushes subnormal p to zero -- no value below 2^-126" % what)
        assert (p[v <= -88.5] == 0).all(), what
    assert ties >= 1, what


def start(e, blocks, key_field, capacity):
    """p of every block with capture off, then capture on from empty."""
    e.metrics_key_field(key_field, capacity, eval=False, train=False)
    p = [probs(e, [b]) for b in blocks]
    e.metrics_key_field(key_field, capacity, eval=True)
    return p


def assert_read(m, ref, what):
    print("%s: %s" % (what, m))
    for k in COUNTS:
        assert m[k] == ref[k], (what, k, m, {c: ref[c] for c in COUNTS})
    assert bits(m["gauc"]) == bits(ref["gauc"]) or (np.isnan(m["gauc"]) and np.isnan(ref["gauc"])), (what, m["gauc"], ref["gauc"])


def passes_of(nf):
    """(key passes, bits of the last key pass) as keyed_sort derives them; the score takes four passes (8, 8, 8, 7)."""
    key_bits = 0
    while key_bits < 31 and (1 << key_bits) < nf:
        key_bits += 1
    n = (key_bits + 7) // 8
    return n, key_bits - 8 * (n - 1) if n else 0


@pytest.fixture(scope="module")
def engine():
    e = two_field_engine(NF_GEOMETRY, BIG_ROWS)
    yield e
    e.close()


# ---- 1. sort geometry past one sub-tile ----------------------------------------------------------

HOT = 777


def geometry_keys(rng, n):
    hot = n // 2 + 5000
    band = np.repeat(np.arange(100, 118), np.tile([63, 64, 65, 255, 256, 257], 3))
    small = np.repeat(np.arange(1000, 5000), np.arange(4000) % 3 + 1)
    mid = rng.integers(6000, 9000, n - hot - band.size - small.size)
    return rng.permutation(np.concatenate([np.full(hot, HOT), band, small, mid]))


@pytest.mark.parametrize("n,chunk,n_wg,per", [(524289, 512, 1025, 2), (1100000, 768, 1433, 3)])
def test_sort_and_rank_geometry(engine, n, chunk, n_wg, per):
    e, nf = engine, NF_GEOMETRY
    # the geometry keyed_sort and keyed_scan_top_kernel derive from n
    c = -(-n // SORT_MAX_WG)
    c = max(1, -(-c // THREADS)) * THREADS
    tiles = -(-n // TILE)
    assert (c, -(-n // c), -(-tiles // THREADS)) == (chunk, n_wg, per) and passes_of(nf) == (2, 7)
    if n == 524289:
        assert n - (n_wg - 1) * chunk == 1  # the last sort workgroup owns one word
    else:
        assert tiles == 538 and THREADS * per > tiles  # idle threads past the end of the top scan
    rng = np.random.default_rng(n)
    first = drawn_blocks(rng, geometry_keys(rng, n), nf, BIG_ROWS)
    more = drawn_blocks(rng, rng.permutation(geometry_keys(rng, n))[:3001], nf, BIG_ROWS)
    assert sum(b.n_rows for b in first) == n and len(first) >= 5 and len(more) == 1
    p = start(e, first + more, 0, 1 << 21)
    keys, v, label = rows_of(first + more, nf)
    p = np.concatenate(p)
    population("n = %d" % n, keys, v, p, label, 100000)
    assert (np.diff(keys[:n]) < 0).sum() > n // 8  # the rows arrive shuffled
    for read, blocks, rows in (("first read", first, n), ("second read", more, n + 3001)):
        for b in blocks:
            e.predict_batch(b)
        ref = fa.keyed_auc_reference(keys[:rows], p[:rows], label[:rows])
        size = ref["pos"] + ref["neg"]
        g = int(np.flatnonzero(ref["key"] == HOT)[0])
        print("n = %d, %s: hot key %d rows (%d positive), U2 = %d; %d keys of 1 to 3 rows" % (
            n, read, size[g], ref["pos"][g], ref["u2"][g], int((size <= 3).sum())))
        # U2 past 32 bits pins the table's 64-bit atomics and what the host reads back.  (A thread's own partial sum of
        # its eight words stays below 16 N: only a key of 2^28 negatives would take that past 32 bits.)
        assert 2 * size[g] > rows and ref["pos"][g] >= 50000 and ref["neg"][g] >= 50000
        assert int(ref["u2"].max()) > 1 << 32 and size[g] > 10 * per * TILE  # tens of top-scan threads see no key start
        assert (size <= 3).sum() >= 2000 and all((size == s).any() for s in (63, 64, 65, 255, 256, 257) if read == "first read")
        m = assert_keyed(e, "eval", ref, "n = %d, %s" % (n, read))
        assert m["n_rows"] == rows and 0.0 < m["gauc"] < 1.0
    e.metrics_key_field(0, 1, eval=False, train=False)


# ---- 2. the key width ladder ---------------------------------------------------------------------

LADDER = {1: (0, 0), 2: (1, 1), 200: (1, 8), 256: (1, 8), 257: (2, 1), 65536: (2, 8), 65537: (3, 1), 1 << 24: (3, 8),
          (1 << 24) + 257: (4, 1)}


def ladder_keys(rng, nf, n):
    """0 and nf - 1, both neighbours of every digit boundary, pairs that differ in exactly one digit, and a few hundred
    others; every key has at least four rows."""
    special = [0, nf - 1, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1]
    base = int(rng.integers(0, nf))
    for d in range(4):
        for flip in (0x01, 0x80, 0x5a):
            special += [base, base ^ (flip << (8 * d)), 0x00a5a5a5 ^ (flip << (8 * d)), 0x00a5a5a5]
    pool = np.unique(np.concatenate([np.array([k for k in special if 0 <= k < nf], np.int64), rng.integers(0, nf, 400)]))
    keys = np.concatenate([np.repeat(pool, 4), rng.choice(pool, n - 4 * pool.size)])
    return rng.permutation(keys), pool


@pytest.mark.parametrize("nf", sorted(LADDER))
def test_key_width_ladder(nf):
    key_passes, last_bits = passes_of(nf)
    print("n_feats = %d: %d key passes, the last of %d bits, %d passes in all" % (nf, key_passes, last_bits, 4 + key_passes))
    assert (key_passes, last_bits) == LADDER[nf]
    rng = np.random.default_rng(nf)
    keys, pool = ladder_keys(rng, nf, 6000)
    assert pool[0] == 0 and pool[-1] == nf - 1
    for edge in (256, 65536, 1 << 24):
        assert all(k in pool for k in (edge - 1, edge, edge + 1) if k < nf)
    one_digit = pool[:, None] ^ pool[None, :]
    assert all(((one_digit > 0) & (one_digit >> (8 * d) << (8 * d) == one_digit) & (one_digit >> (8 * d) < 256)).any()
               for d in range(key_passes))  # every key digit has a pair of keys that differ in it alone
    # (the two largest: a serving engine of zero bits, only lin_w[sid] set -- no host array of the table's size)
    e = two_field_engine(nf, 8192, serve="f16")
    first = drawn_blocks(rng, keys[:4500], nf, 8192)
    more = drawn_blocks(rng, keys[4500:], nf, 8192)
    p = np.concatenate(start(e, first + more, 0, 1 << 14))
    keys, v, label = rows_of(first + more, nf)
    population("n_feats = %d" % nf, keys, v, p, label, 2000)
    e.predict_batch(first[0])
    ref = fa.keyed_auc_reference(keys[:4500], p[:4500], label[:4500])
    assert_keyed(e, "eval", ref, "n_feats = %d, first read" % nf)
    # a third sort: after an odd number of passes each the words now live in what was the scratch buffer, and the next
    # block is appended there
    assert_read(e.metrics_read_keyed("eval"), ref, "n_feats = %d, read again" % nf)
    e.predict_batch(more[0])
    ref = fa.keyed_auc_reference(keys, p, label)
    assert np.array_equal(ref["key"], pool) and ref["n_keys_mixed"] > pool.size // 2
    assert_keyed(e, "eval", ref, "n_feats = %d, one more block and no reset" % nf)
    e.close()


def test_both_channels_at_seven_passes():
    """A training engine at n_feats = 65 537: both channels share the scratch buffer, and after a single read each
    (seven passes, odd) the three buffers have changed hands.  lin_w[sid] = W(n, z) = 1 through n = 1, z = -2 / alpha
    (l1 = l2 = 0, beta = 1), and a step of alpha = 1e-4 leaves it near 1."""
    nf = 65537
    assert passes_of(nf) == (3, 1)
    hp = dict(w_alpha=1e-4, w_beta=1.0, w_l1=0.0, w_l2=0.0)
    e, twin = two_field_engine(nf, 8192, **hp), two_field_engine(nf, 8192, **hp)
    one = np.ones(1, np.float32)
    for x in (e, twin):
        x.set_rows(np.array([sid_of(nf)], np.int32), dict(lin_w=one, lin_n=one, lin_z=-2.0e4 * one))
    rng = np.random.default_rng(65537)
    keys, _ = ladder_keys(rng, nf, 6000)
    b1, b2, b3 = (drawn_blocks(rng, keys[a:b], nf, 8192)[0] for a, b in ((0, 3000), (3000, 5000), (5000, 6000)))
    p1 = e.eval_sigmoid(twin.train_batch(b1)[0])  # the pre-update logits
    twin.close()
    e.metrics_key_field(0, 1 << 13, eval=False, train=True)
    e.train_batch(b1)
    p2, p3 = probs(e, [b2]), probs(e, [b3])  # (the eval capture is off)
    e.metrics_key_field(0, 1 << 13, eval=True, train=True)  # train stays as it is, eval starts from empty
    k1, v1, y1 = rows_of([b1], nf)
    k2, v2, y2 = rows_of([b2, b3], nf)
    population("train channel", k1, v1, p1, y1, 1000)
    population("eval channel", k2, v2, np.concatenate([p2, p3]), y2, 1000)
    ref1 = fa.keyed_auc_reference(k1, p1, y1)
    ref2 = fa.keyed_auc_reference(k2[:2000], p2, y2[:2000])
    ref23 = fa.keyed_auc_reference(k2, np.concatenate([p2, p3]), y2)
    e.predict_batch(b2)
    assert_read(e.metrics_read_keyed("eval"), ref2, "eval, first read")
    assert_read(e.metrics_read_keyed("train"), ref1, "train, first read")
    e.predict_batch(b3)
    assert_keyed(e, "eval", ref23, "eval, one more block and no reset")
    assert_keyed(e, "train", ref1, "train, after the eval channel's sorts")
    assert ref1["n_keys_mixed"] > 100 and ref23["n_keys_mixed"] > 100
    e.close()


# ---- 3. exact row counts -------------------------------------------------------------------------

@pytest.mark.parametrize("n,one_key", [(n, False) for n in (1, 255, 256, 257, 2047, 2048, 2049, 4096, 4097)] + [(2048, True), (2049, True)])
def test_exact_row_counts(engine, n, one_key):
    e, nf = engine, NF_GEOMETRY
    rng = np.random.default_rng(10 * n + one_key)
    keys = np.full(n, 4321) if one_key else rng.integers(0, max(1, n // 8), n) * 31 % nf
    blocks = drawn_blocks(rng, keys, nf, BIG_ROWS)
    p = np.concatenate(start(e, blocks, 0, 1 << 13))
    keys, v, label = rows_of(blocks, nf)
    if n >= 255:  # (a single row has one p and no pair)
        population("n = %d%s" % (n, ", one key" if one_key else ""), keys, v, p, label, min(2000, n // 2))
    e.predict_batch(blocks[0])
    ref = fa.keyed_auc_reference(keys, p, label)
    m = assert_keyed(e, "eval", ref, "n = %d%s" % (n, ", one key" if one_key else ""))
    assert m["n_rows"] == n and m["n_keys"] == (1 if one_key else np.unique(keys).size)
    e.metrics_key_field(0, 1, eval=False, train=False)


# ---- 4. capture on long rows ---------------------------------------------------------------------

NF4, F4, PER4, KEY_FIELD = 4096, 4, 1024, 2
LENGTHS = list(range(1, 18)) + [24, 25, 39, 40, 64, 65, 100]


def long_rows(rng):
    """(rows, what each row is).  Every entry outside KEY_FIELD's named places lies under another field."""
    def fill(n):
        f = rng.choice([0, 1, 3], n)
        return [(int(a), int(a) * PER4 + int(b)) for a, b in zip(f, rng.integers(0, PER4, n))]

    def key():
        return KEY_FIELD * PER4 + int(rng.integers(0, 40))

    rows, kinds = [], []
    for _ in range(4):
        for n in LENGTHS:
            for q in range(n):  # the only entry of the key field at every position
                row = fill(n)
                row[q] = (KEY_FIELD, key())
                rows.append(row)
                kinds.append("at %d" % q)
    for _ in range(3):
        for erased in (-3, NF4, NF4 + 5):
            for q in (8, 9, 12, 15, 16, 23):
                for before in ((q - 8,), (q - 1,), (q - 8, q - 1)):  # the same lane a trip earlier / the entry before
                    row = fill(q + 3)
                    for at in before:
                        row[at] = (KEY_FIELD, erased)
                    row[q] = (KEY_FIELD, key())
                    row[q + 1] = (KEY_FIELD, row[q][1] + 50)  # (a later valid one must not win either)
                    rows.append(row)
                    kinds.append("erased")
        for a, b in ((9, 12), (12, 9 + 8), (7, 8), (15, 16)):  # two valid ones: the earlier position wins
            row = fill(b + 2)
            row[a] = (KEY_FIELD, key())
            row[b] = (KEY_FIELD, row[a][1] + 100)
            rows.append(row)
            kinds.append("two")
        for n, at in ((1, (0,)), (9, (0, 8)), (20, (3, 11, 19)), (40, (7, 15, 23, 31, 39))):  # every key-field entry erased
            row = fill(n)
            for i, a in enumerate(at):
                row[a] = (KEY_FIELD, (-3, NF4, NF4 + 5)[i % 3])
            rows.append(row)
            kinds.append("all erased")
        for _ in range(5):
            rows.append([])
            kinds.append("empty")
    order = rng.permutation(len(rows))
    return [rows[i] for i in order], [kinds[i] for i in order]


def test_capture_on_long_rows():
    rng = np.random.default_rng(44)
    rows, kinds = long_rows(rng)
    labels = (rng.random(len(rows)) < 0.45).astype(np.int32)
    cuts = (0, 801, 1603, len(rows))
    blocks = [from_rows(rows[a:b], labels[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(rows) > 2000 and all(b.n_rows % 32 for b in blocks) and max(len(r) for r in rows) == 100
    e = fa.Engine("FFM", NF4, F4, 4, skip_init=True, max_batch_rows=2048, max_batch_nnz=1 << 17, max_row_nnz=128)
    e.set_weights(bias=np.zeros(1, np.float32), lin_w=rng.normal(0.0, 0.5, NF4).astype(np.float32))
    p = np.concatenate(start(e, blocks, KEY_FIELD, 1 << 13))
    keys = np.concatenate([keys_of(b, key_field=KEY_FIELD, n_feats=NF4) for b in blocks])
    # the host walk sees what the rows were built for
    kinds = np.array(kinds)
    assert (keys[np.isin(kinds, ("all erased", "empty"))] == -1).all() and (keys[~np.isin(kinds, ("all erased", "empty"))] >= 0).all()
    assert ((keys[kinds == "two"] - KEY_FIELD * PER4) < 40).all() and ((keys[kinds == "erased"] - KEY_FIELD * PER4) < 40).all()
    second_trip = sum(int(k[3:]) >= 8 for k in kinds if k.startswith("at "))
    print("%d rows, %d distinct p; the key on a lane's second or later trip in %d rows; %d rows without a key" % (
        len(rows), np.unique(p.view(np.uint32)).size, second_trip, int((keys < 0).sum())))
    assert second_trip > 1000 and np.unique(p.view(np.uint32)).size > 1500 and not np.isnan(p).any()
    ref = fa.keyed_auc_reference(keys, p, labels)
    for b in blocks:
        e.predict_batch(b)
    m = assert_keyed(e, "eval", ref, "long rows")
    assert m["n_unkeyed"] == int((keys < 0).sum()) == 3 * 9 and m["n_rows"] == len(rows) - 27 and m["n_keys_mixed"] > 30
    e.close()
