"""Writes tests/golden/forward_plan_trace.json: the ordered forward launch plans of the real backbones on the CPU stand-ins of
tests/test_forward_plan_cpu.py (plan_traces(): every mark with its FLOP and byte counts, every ops entry inside it with its buffer
labels and scalar arguments, every prepared.get key, the TRAIN-mode tape and gradient set, the graph key -- for the batch sizes, the
switch grid and the three backbones), as one digest per entry and the graph key in full (digest_traces).
test_the_ordered_forward_plan_of_every_run_is_the_recorded_one compares the working tree against this file, so it is written from the
commit whose launches are the reference -- first from the commit before the forward pass was split into frcnn_hip/forward.py, with this
file and the test module copied into a checkout of it (the harness drives both through create_architecture, _build_network and
graph_key) -- and regenerated, with a word in the commit message, whenever a later change alters the launches of a forward pass on
purpose.  --full writes the entries themselves instead (440 kB: to read what a digest stands for, not to commit).

    python fixtures/gen_forward_plan_trace.py [--full] [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_forward_plan_cpu as T  # noqa: E402

if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--full"]
    assert args or "--full" not in sys.argv, "--full needs a file name of its own"
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "forward_plan_trace.json")
    traces = T.plan_traces()
    packed = traces if "--full" in sys.argv else T.digest_traces(traces)
    with open(out, "w") as f:                           # one run per line
        f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(run), json.dumps(packed[run], separators=(",", ":"), sort_keys=True))
                                   for run in sorted(packed)) + "\n}\n")
    print("%s: %d runs, %d entries, %d bytes" % (out, len(traces), sum(len(t) for t in traces.values()), os.path.getsize(out)))
