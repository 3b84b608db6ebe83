"""NTT block kernels alone on the chip, for an A/B of two trees: run from a tree's root (the package is imported from
the working directory).  Out-of-place inverse NTT and two-coset LDE from coefficients at 2^14 x 2432, 2^13 x 2432 and
2^12 x 2048, with the VALU kernels (bp_tune_ntt_mx 0) and with the default choice (3): median / minimum of 15 launches
by HIP events.  With --pmc: two launches of each at 2^14 x 2432, VALU kernels only, for a counter pass
(rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES -- python tools/ntt_ab_probe.py --pmc; read the last dispatch of a kernel)."""
import json, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import torch
from proof_protocol_decoder_amd import ops
pmc = "--pmc" in sys.argv
rng = np.random.default_rng(1)
res = {}
shapes = [(14, 2432), (13, 2432), (12, 2048)] if not pmc else [(14, 2432)]
for log_n, cols in shapes:
    n = 1 << log_n
    v = torch.from_numpy(rng.integers(0, (1 << 63) - 1, size=(cols, n), dtype=np.int64)).cuda()
    out = torch.empty_like(v)
    for mx in ((0,) if pmc else (0, 3)):
        with ops.tuned(ntt_mx=mx):
            def inv(): ops.intt_batch(v, out=out)
            def lde(): ops.lde_batch(out, 1, from_coeffs=True)
            for name, fn in (("inv", inv), ("lde1", lde)):
                if pmc:
                    fn(); torch.cuda.synchronize()   # tables + first launch
                    fn(); torch.cuda.synchronize()
                    continue
                for _ in range(3): fn()
                torch.cuda.synchronize()
                ts = []
                for _ in range(15):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); fn(); b.record(); torch.cuda.synchronize()
                    ts.append(a.elapsed_time(b) * 1e3)
                ts.sort()
                res["2^%d x %d %s mx=%d" % (log_n, cols, name, mx)] = {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1)}
    del v, out
print(json.dumps(res, indent=1))
