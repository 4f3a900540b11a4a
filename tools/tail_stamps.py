# needs the debug build of the library: python tools/build_variant.py stamps -DCGS_DEBUG_STAMPS ; CGS_LIB_PATH=<pkg>/libcgs_hip_stamps.so (the product library exports no dbg_* hooks)
"""Stage timing of the tail kernels (debug hook dbg_tail_stamps): mean s_memtime deltas between the stage boundaries of
every workgroup's first image, per kernel.  Usage (GPU box): python tools/tail_stamps.py [batch]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from cgs_amd import _lib, engine  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
dev = torch.device("cuda:0")
eng = engine.HourglassEngine(n, device=dev, dropout=0.3, use_graph=False)
eng.load_state(*bench.g1_weights())
A, B, Y = bench.synthetic(n, 0, dev)
for _ in range(3):
    eng.phase2_step(A, B, Y)
torch.cuda.synchronize()
buf = torch.zeros(4 * 2048 * 16, dtype=torch.int64, device=dev)
lib = _lib.load()
if not hasattr(lib, "dbg_tail_stamps"):
    raise SystemExit("stamps need the debug build: python tools/build_variant.py stamps -DCGS_DEBUG_STAMPS, then CGS_LIB_PATH=<pkg>/libcgs_hip_stamps.so")
lib.dbg_tail_stamps.argtypes = [C.c_void_p]
lib.dbg_tail_stamps(C.c_void_p(buf.data_ptr()))
# the fused decoder + mask head forward (dec_mask_fwd_kernel): its decoder phase stamps land in the "dec_fwd" block, its mask phase's here
mbuf = torch.zeros(n * 64, dtype=torch.int64, device=dev)
fused = hasattr(lib, "dbg_dec_mask_stamps")
if fused:
    lib.dbg_dec_mask_stamps.argtypes = [C.c_void_p]
    lib.dbg_dec_mask_stamps(C.c_void_p(mbuf.data_ptr()))
eng.phase2_step()
torch.cuda.synchronize()
lib.dbg_tail_stamps(C.c_void_p(0))
if fused:
    lib.dbg_dec_mask_stamps(C.c_void_p(0))
st = buf.cpu().numpy().reshape(4, 2048, 16)
for k, name in enumerate(("enc_fwd (last call: mixes)", "dec_fwd", "enc_bwd (last call: A pass)", "dec_bwd")):
    s = st[k]
    live = s[:, 0] != 0
    s = s[live].astype(np.float64)
    if not len(s):
        continue
    cols = [c for c in range(16) if (s[:, c] != 0).all()]
    cols.sort(key=lambda c: s[:, c].mean())
    d = np.diff(s[:, cols], axis=1)
    print(f"{name}: {live.sum()} workgroups, stamps {cols}")
    print("   mean ticks per stage:", np.round(d.mean(0), 0).tolist(), " total", round(float((s[:, cols[-1]] - s[:, cols[0]]).mean())))
    print("   span (first workgroup's first stamp .. last workgroup's last stamp):", float(s[:, cols[-1]].max() - s[:, cols[0]].min()))
    if (s[:, 14] != 0).all() and 14 not in cols[1:-1]:
        print("   kernel entry (stamp 14) -> first stage stamp: mean", round(float((s[:, cols[1] if cols[0] == 14 else cols[0]] - s[:, 14]).mean())),
              " entry -> end: mean", round(float((s[:, 15] - s[:, 14]).mean())), " max", float((s[:, 15] - s[:, 14]).max()),
              " launch span", float(s[:, 15].max() - s[:, 14].min()))

ms = mbuf.cpu().numpy().reshape(n, 64).astype(np.float64)
if fused and (ms[:, 41] != 0).all():
    # one clock for both phases: everything relative to the launch's first decoder-phase stamp
    d = st[1][:n].astype(np.float64)
    med = lambda v: round(float(np.median(v)))
    print(f"dec_mask_fwd (fused decoder + mask head forward): {n} workgroups (differences within a workgroup or between CU neighbours only: every XCD has its own clock)")
    print("   per workgroup, median ticks: kernel entry (mask stamp 0) -> decoder phase start", med(d[:, 0] - ms[:, 0]), " decoder phase (tail stages + dec_model.0)",
          med(d[:, 15] - d[:, 0]), " of it dec_model.0", med(d[:, 15] - d[:, 6]), " decoder end -> mask strips start (barrier, o0 fetch)", med(ms[:, 2] - d[:, 15]),
          " mask strips", med(ms[:, 41] - ms[:, 2]), " whole", med(ms[:, 41] - ms[:, 0]))
    print("   mask strips (median): " + "  ".join(f"strip {k}: {med(ms[:, 2 + 10 * (k + 1)] - ms[:, 2 + 10 * k]) if k < 3 else med(ms[:, 41] - ms[:, 32])}" for k in range(4)))
    if n > 256:
        # workgroups 256 apart share a CU: how much of one's (latency-bound) decoder phase lies inside the other's (issue-bound) mask strips
        lo, hi = np.arange(0, n - 256), np.arange(256, n)
        ov = lambda a0, a1, b0, b1: np.maximum(0.0, np.minimum(a1, b1) - np.maximum(a0, b0))
        o = ov(d[lo, 0], d[lo, 15], ms[hi, 2], ms[hi, 41]) + ov(d[hi, 0], d[hi, 15], ms[lo, 2], ms[lo, 41])
        print("   CU neighbours (b, b + 256): start offset median", med(np.abs(ms[hi, 0] - ms[lo, 0])), " ticks; decoder phase of one under the mask strips of the other: median",
              med(o), "ticks per pair (of", med((d[lo, 15] - d[lo, 0]) + (d[hi, 15] - d[hi, 0])), "decoder ticks per pair)")
