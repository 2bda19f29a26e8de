"""Writes tests/golden/replay_trace.json: the per-step trace of the recorded-step state machine on the CPU stand-ins of
tests/test_replay_cpu.py (replay_trace(): one scripted scenario through eager, recorded and replayed steps, LRU eviction of recordings,
derived-generation changes, a second solver handle, a stream search run to its end, and the switch off).
test_the_scripted_scenario_gives_the_recorded_trace compares the working tree against this file, so it is written from the commit whose
behaviour is the reference -- first from the commit before the state machine moved from Network into frcnn_hip/replay.py, with this file
and the test module copied into a checkout of it -- and regenerated, with a word in the commit message, whenever a later change alters
which steps replay or what they launch on purpose.

    python fixtures/gen_replay_trace.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_replay_cpu as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "replay_trace.json")
    steps = T.replay_trace()
    with open(out, "w") as f:
        json.dump(steps, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%s: %d steps, %d log entries, %d bytes" % (out, len(steps), sum(len(s["log"]) for s in steps), os.path.getsize(out)))
