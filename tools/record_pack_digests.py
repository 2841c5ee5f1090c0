#!/usr/bin/env python3
"""How tests/golden/pack_digests.json was recorded (tests/test_host_device_weights.py compares fsnp_debug_pack_emulate with it).

    python tools/record_pack_digests.py <libfsnp_hip.so built at commit f4848bd> [out.json]

That commit is the last one with the per-kernel host packers (fsnp::lstm_pack_weights and its siblings, exported under their C++
names).  Each is called through ctypes on the sources of the test's rnn_cases(); the SHA-256 of what it wrote is the record.  The
image sizes come from the library of THIS tree (fsnp_debug_pack_emulate), which the test module loads."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_host_device_weights as T  # noqa: E402

lib = ctypes.CDLL(sys.argv[1])
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "pack_digests.json")
P = ctypes.c_void_p
def call(sym, ints, arrs, n):
    out = np.full(n, np.float32(np.nan))
    f = getattr(lib, sym); f.restype = None
    f.argtypes = [ctypes.c_int] * len(ints) + [P] * (len(arrs) + 1)
    f(*ints, *[a.ctypes.data for a in arrs], out.ctypes.data)
    return out
SYM = {T.ROWTILE: '_ZN4fsnp17lstm_pack_weightsEiiiiPKfS1_S1_S1_Pf', T.HALF: '_ZN4fsnp19lstm16_pack_weightsEiiiPKfS1_S1_S1_Pf',
       T.HP: '_ZN4fsnp20lstm_hp_pack_weightsEiiiPKfS1_S1_S1_Pf', T.HPW: '_ZN4fsnp21lstm_hpw_pack_weightsEiiiPKfS1_S1_S1_Pf',
       T.COOPW: '_ZN4fsnp23lstm_coopw_pack_weightsEiiiPKfS1_S1_S1_Pf', T.GRU: '_ZN4fsnp16gru_pack_weightsEiiiiPKfS1_S1_S1_Pf',
       T.KSPLIT: '_ZN4fsnp22lstm_coop_pack_weightsEiiiiPKfS1_S1_S1_Pf', T.COOPN: '_ZN4fsnp23lstm_coopn_pack_weightsEiiiPKfS1_S1_S1_Pf',
       T.ROWTILE_BF: '_ZN4fsnp24lstm_pack_weights_bf16ihEiiiiPKfS1_S1_S1_S1_Pf', T.HALF_BF: '_ZN4fsnp26lstm16_pack_weights_bf16ihEiiiPKfS1_S1_S1_Pf',
       T.FBV: '_ZN4fsnp21lstm_fbv_pack_weightsEiiPKfS1_S1_S1_Pf', T.GENERIC: '_ZN4fsnp25lstm_generic_pack_weightsEiiPKfS1_S1_S1_Pf'}
out = {}
for cid, kind, sizes in T.rnn_cases():
    src = T.case_sources(kind, sizes)
    n = T.emulate(kind, sizes, src).size       # size from the new library (the images' sizes are also pinned by the old *_pack_floats in the kernels)
    H = sizes[0]
    if kind == T.GRU:
        w = [T.spread(src[m], H, bool(m & 1)) for m in range(4)]
        ints = sizes[:4]
    else:
        w = [np.ascontiguousarray(s) for s in src[:4]]
        ints = {T.ROWTILE: sizes[:4], T.ROWTILE_BF: sizes[:4], T.KSPLIT: sizes[:4], T.FBV: sizes[:2], T.GENERIC: sizes[:2]}.get(kind, sizes[:3])
    arrs = list(w)
    if kind == T.ROWTILE_BF:
        arrs.append(src[4] + src[5])
    got = call(SYM[kind], list(ints), arrs, n)
    assert not np.isnan(got).any(), cid
    out[cid] = T.digest(got)
json.dump(out, open(OUT, 'w'), indent=0, sort_keys=True)
print(len(out), 'digests')
