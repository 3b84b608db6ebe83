import sys, os, time
sys.path.insert(0, os.getcwd())
import numpy as np
import proof_protocol_decoder_amd as pkg
L = pkg.lib()
s = np.arange(12 * 20000, dtype=np.uint64).reshape(-1, 12)
for mode in (0, 1):
    with pkg.ops.tuned(host_poseidon=mode):
        t0 = time.perf_counter(); L.bp_debug_poseidon_host(s.ctypes.data, s.shape[0]); dt = time.perf_counter() - t0
    print("host poseidon form %d: %.2f us/perm" % (mode, dt / s.shape[0] * 1e6))
