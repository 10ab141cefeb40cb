#!/usr/bin/env python3
"""Development: per-wave cycle breakdown of the accumulation kernel's step loop (syrk_strip_kernel, agpl_syrk.hip) by tile kind.
Needs the diagnostic build:  tools/build_variant.sh qtrace agpl_syrk.hip "-DAGPL_QTRACE"   (or make QTRACE=1)
  python tools/qtrace.py libagpl_qtrace.so [N M]     (default: the C2 shape, N = 1e7, M = 512; the library is loaded the way
                                                      tools/bench_with_lib.py loads a variant: by its name beside libagpl.so)
The build stamps, per wave of the launch's first 64 workgroups: the cycles of the whole step loop, the cycles spent in the step's
`s_waitcnt vmcnt` (memory queue; a build that does not stamp a tile kind's wait leaves zeros there: printed as `-`) and at the
step's barrier, and in word 6 the step count, the tile kind and the wave's first 16-column block.  Printed per tile kind and wave: cycles per step, barrier share and
queue-wait share of the loop.  CLOCK CAVEAT: the cycles are those of s_memtime, whose rate against the 100 MHz real-time
counter is printed per tile kind; the shader clock moves with power and temperature and with what else runs on the card, so the
us-per-step figures (s_memrealtime) are the ones to compare between builds, and only between runs of one session on one card;
shares are ratios of one counter and compare freely.  The stamps themselves cost a few s_memtime + waits per step: a QTRACE build's absolute times are not the product's."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import agpl_amd as A
from agpl_amd import _ffi

_ffi.LIB_PATH = os.path.join(os.path.dirname(_ffi.LIB_PATH), sys.argv[1])
import bench

N = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10_000_000
M = int(sys.argv[3]) if len(sys.argv) > 3 else 512
ctx = A.Context(0, seed=bench.SEED)
lib = _ffi.lib()
if not hasattr(lib, "agpl_debug_qtrace"):
    sys.exit(f"{_ffi.LIB_PATH} is not a QTRACE build (no agpl_debug_qtrace)")
lik = A.BernoulliLikelihood()
y, Phi, kd = bench.build_workload(A, ctx, lik, 0, N, M)
cavi = A.SparseCAVI(lik, Phi, kd, y, ctx=ctx)
for _ in range(3):  # the sweeps give the accumulation the gamma | beta of a running fit; the stamps are those of the last launch
    cavi.sweep()
cavi.accumulate()
cavi.check()
torch.cuda.synchronize()
buf = (C.c_ulonglong * (64 * 16 * 8))()
rc = lib.agpl_debug_qtrace(buf)
if rc:
    sys.exit(f"agpl_debug_qtrace: hip error {rc}")
a = np.frombuffer(buf, dtype=np.uint64).reshape(64, 16, 8)[:, :8, :]
nstep = (a[:, :, 6] & np.uint64(0xFFFFFFFF)).astype(np.float64)
diag = ((a[:, :, 6] >> np.uint64(32)) & np.uint64(0xFF)).astype(np.int64)
strip = ((a[:, :, 6] >> np.uint64(40)) & np.uint64(0xFF)).astype(np.int64)
queue, loop, barrier, real = (a[:, :, k].astype(np.float64) for k in (0, 1, 2, 5))
full = nstep == nstep.max()  # whole slices only (a fine tail slice has a larger share of prologue per step)
out = {"lib": os.path.basename(_ffi.LIB_PATH), "N": N, "M": M, "steps_per_slice": int(nstep.max()), "kinds": {}}
print(f"{out['lib']}  N={N} M={M}: {int(nstep.max())} steps per workgroup; per tile kind and wave, means over the traced workgroups")
for kind, name in ((0, "off-diagonal"), (1, "diagonal")):
    sel = full & (diag == kind) & (nstep > 0)
    nwg = int(sel.all(axis=1).sum())
    if not nwg:
        continue
    wg = sel.all(axis=1)
    us = real[wg] / 100.0 / nstep[wg]  # 100 MHz real-time counter
    cyc = loop[wg] / nstep[wg]
    print(f" {name}: {nwg} workgroups, {us.mean():.3f} us per step (min {us.min():.3f}, max {us.max():.3f}); "
          f"counter {np.mean(loop[wg] / real[wg]) * 0.1:.3f} GHz")
    stamped = bool(queue[wg].sum() > 0)  # (an unstamped wait reads zero in every wave: not a measurement)
    rows = []
    for w in range(8):
        r = {"wave": w, "first_block": int(strip[wg][0, w]), "cycles_per_step": round(float(cyc[:, w].mean()), 1),
             "us_per_step": round(float(us[:, w].mean()), 4),
             "barrier_share": round(float((barrier[wg][:, w] / loop[wg][:, w]).mean()), 4),
             "queue_share": round(float((queue[wg][:, w] / loop[wg][:, w]).mean()), 4) if stamped else None}
        rows.append(r)
        print(f"   wave {w} (first column block {r['first_block']:2d}): {r['cycles_per_step']:8.1f} cycles per step   "
              f"barrier {100 * r['barrier_share']:5.1f} %   memory queue " + (f"{100 * r['queue_share']:5.1f} %" if stamped else "    -"))
    out["kinds"][name] = {"workgroups": nwg, "us_per_step": round(float(us.mean()), 4), "waves": rows}
print(json.dumps(out))
