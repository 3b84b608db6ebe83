"""The flagship block under the schedule knobs bench.py has no flag for: bp_tune_txn_group (transactions a thread takes at a
time) and bp_tune_rec_group (0: a group's recursion levels as lock-step batches over the group, 1: one transaction's
recursion at a time).  The knobs are set in this process, then bench.py runs in it unchanged and prints its JSON line;
afterwards the sizes of the recursion batches the run proved (bp_debug_rec_batch_histogram) go to stderr.
  python tools/rec_group_probe.py [--txn-group N] [--rec-group M] -- <bench.py arguments>
e.g. the sweep of profiles/rec_group_ab.txt:  for g in 3 4 5; do python tools/rec_group_probe.py --txn-group $g -- --gpus 1
--steps 2 --warmup 1 --no-cpu-baseline --no-profile; done"""
import ctypes as C
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    rest = argv[argv.index("--") + 1:] if "--" in argv else []
    own = argv[:argv.index("--")] if "--" in argv else argv
    knobs = {}
    while own:
        flag = own.pop(0)
        if flag not in ("--txn-group", "--rec-group") or not own:
            raise SystemExit(__doc__)
        knobs[flag] = int(own.pop(0))
    # The knobs live in the library, so it loads HERE, before bench.py's module runs -- and the runtime it pulls in reads
    # GPU_MAX_HW_QUEUES when it starts.  bench.py's own default therefore has to be in place already (a value the
    # caller exported wins, as it does there); without this line the probe would measure another queue count than
    # `python bench.py` does.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")
    import proof_protocol_decoder_amd as pkg
    L = pkg.lib()
    if "--txn-group" in knobs:
        L.bp_tune_txn_group(knobs["--txn-group"])
    if "--rec-group" in knobs:
        L.bp_tune_rec_group(knobs["--rec-group"])
    sys.argv = [os.path.join(ROOT, "bench.py")] + rest
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        out = (C.c_uint64 * 32)()
        L.bp_debug_rec_batch_histogram(out, 32, 0)
        print("knobs %s, GPU_MAX_HW_QUEUES=%s; recursion batches by size: %s"
              % (knobs or "default", os.environ.get("GPU_MAX_HW_QUEUES"), {b: int(c) for b, c in enumerate(out) if c}), file=sys.stderr)


if __name__ == "__main__":
    main()
