"""Time of one 8192 x 39 block through a field sketch (profiles/field_sketch.md (b)): from page-locked memory with and
without a field array (a host clock around the synchronous call), from pageable memory and from HBM.  Kernel times:
the same script under `rocprofv3 --kernel-trace --stats`."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
F, ROWS = 39, 8192
lib = fa.load_library()
g = synth.Generator(F, F * 25000, "zipf", seed=42)
blocks = [g.block(ROWS) for _ in range(8)]
pinned = []
for b in blocks:
    pf, pi = fa.page_aligned(b.nnz, np.int32), fa.page_aligned(b.nnz, np.int32)
    pf[:] = b.field; pi[:] = b.feat
    assert lib.ffm_engine_pin_host(pf.ctypes.data, pf.size * 4) == 0 and lib.ffm_engine_pin_host(pi.ctypes.data, pi.size * 4) == 0
    pinned.append((pf, pi))
for with_field in (True, False):
    sk = fa.FieldSketch(F)
    for i in range(40):
        pf, pi = pinned[i % 8]; sk.add(pf if with_field else None, pi, zero_copy=True)
    ts = []
    for i in range(400):
        pf, pi = pinned[i % 8]
        t0 = time.perf_counter(); sk.add(pf if with_field else None, pi, zero_copy=True); ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e6
    reg, nv, nb = sk.read()
    print("field array %s: call (launch + kernel + wait) median %.1f us, p10 %.1f, p90 %.1f; n_valid %d n_bad %d; estimate of field 0: %.0f"
          % (with_field, np.median(ts), np.percentile(ts, 10), np.percentile(ts, 90), nv, nb, sk.estimate()[0]))
    sk.close()
# the same entries from pageable memory (staged) and from HBM
sk = fa.FieldSketch(F)
b = blocks[0]
ts = []
for i in range(200):
    t0 = time.perf_counter(); sk.add(b.field, b.feat); ts.append(time.perf_counter() - t0)
sk.read()
print("pageable: call (copy + launch) median %.1f us" % (np.median(ts) * 1e6))
df, di = torch.from_numpy(b.field).cuda(), torch.from_numpy(b.feat).cuda()
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(200):
    sk.add_device(b.nnz, df.data_ptr(), di.data_ptr())
sk.read()
print("device: %.1f us per block (200 launches back to back, one wait)" % ((time.perf_counter() - t0) / 200 * 1e6))
sk.close()
for pf, pi in pinned:
    lib.ffm_engine_unpin_host(pf.ctypes.data); lib.ffm_engine_unpin_host(pi.ctypes.data)
