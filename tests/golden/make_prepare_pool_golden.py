#!/usr/bin/env python3
"""Generate tests/golden/prepare_pool_bytes.json: gf_smp_device_bytes (in use, reserved) after every step of the batch sequence of
tests/test_prepare_pool_gpu.py, one list per handle.

Recorded on commit e7e1b35 ("Per-kernel fp64 tests and stand-alone operators for the GRU level"), the parent of the commit that gathered a
batch's state into gf_smp_batch: the numbers pin which pool block backs which request of gf_smp_prepare, how far the pool grows and what it
frees.  Run on a machine with the device, on a build of the commit whose numbers are to be recorded:

    python tests/golden/make_prepare_pool_golden.py [output.json]

Every handle's sequence is run twice in this process; a case whose two runs differ is left out and named on stderr (the arithmetic is
integer, so none should).  Only data is recorded."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_prepare_pool_gpu as suite  # noqa: E402

RECORDED_ON = "e7e1b35"


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else suite.GOLDEN
    sizes = {}
    for name in suite.make_nets():
        first, second = suite.run_sequence(name)[0], suite.run_sequence(name)[0]
        if first != second:
            print("left out, two runs differ: %s\n  %s\n  %s" % (name, first, second), file=sys.stderr)
            continue
        sizes[name] = first
    with open(out, "w") as f:
        json.dump({"recorded_on": RECORDED_ON, "sequence": suite.SEQUENCE, "bytes": sizes}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d handles" % (out, len(sizes)))


if __name__ == "__main__":
    main()
