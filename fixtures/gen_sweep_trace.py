"""Writes tests/golden/sweep_trace.json: the ordered traces of the reverse sweep on the CPU stand-ins of tests/test_sweep_logic_cpu.py
(sweep_traces(): every ops call, event record, wait and pinned-stream entry with its buffer names and scalar arguments, for the switch
grid, the three-step runs and the data-parallel runs).  test_the_ordered_trace_of_every_run_is_the_recorded_one compares the working
tree against this file, so it is written from the commit whose launches are the reference -- first from the commit before the sweep
was split into frcnn_hip/sweep.py, with this file and the test module copied into a checkout of it -- and regenerated, with a word in
the commit message, whenever a later change alters the launches of a step on purpose.

    python fixtures/gen_sweep_trace.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_sweep_logic_cpu as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sweep_trace.json")
    traces = T.sweep_traces()
    with open(out, "w") as f:
        json.dump(traces, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%s: %d runs, %d entries, %d bytes" % (out, len(traces), sum(len(t) for t in traces.values()), os.path.getsize(out)))
