"""The engine-call traces of the Tiled VAE hook on the torch doubles (tests/test_vae_call_trace.py: the tracing doubles and the matrix
of modes x doubles x switches), recorded from the commit that is checked out when this runs:

    python tests/golden/make_golden_call_trace.py        ->  tests/golden/vae_call_trace.json

The file is data about THAT commit's behaviour: record it before a change of the host logic, never from the changed code.  Entries
(one string per call) are interned and identical traces stored once."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_vae_call_trace as ct  # noqa: E402


def main():
    entries, traces, runs = {}, {}, {}
    n_runs = 0
    for mode in ct.MODES:
        for doubles, off in ct.matrix(mode):
            t = ct.trace(mode, doubles, off)
            assert t == ct.trace(mode, doubles, off), "the trace is not deterministic"
            ids = tuple(entries.setdefault(e, len(entries)) for e in t)
            runs[ct.run_key(mode, doubles, off)] = traces.setdefault(ids, len(traces))
            n_runs += 1
    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    with open(ct.GOLDEN, "w") as f:
        json.dump({"recorded_at": commit, "entries": list(entries), "traces": [list(t) for t in traces], "runs": runs}, f, separators=(",", ":"))
    print(f"{n_runs} runs, {len(traces)} distinct traces, {len(entries)} distinct entries, {os.path.getsize(ct.GOLDEN) // 1024} KiB")


if __name__ == "__main__":
    main()
