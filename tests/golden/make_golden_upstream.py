#!/usr/bin/env python3
"""Regenerates tests/golden/upstream.npz: upstream's side of every comparison in tests/test_oracle_vs_reference.py,
tests/test_md_entry_path.py and tests/test_host_abi.py (see tests/upstream_pin.py).  It runs those comparisons once against the
UPSTREAM code itself (imported verbatim under hostsim/stub_host.py, CPU) and records each upstream value as it is computed.

    python tests/golden/make_golden_upstream.py
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from hostsim import stub_host as sh  # noqa: E402

MODULES = ["tests/test_oracle_vs_reference.py", "tests/test_md_entry_path.py", "tests/test_host_abi.py::test_best_tile_size_matches_upstream"]


def main():
    if not sh.reference_available():
        raise SystemExit(f"the upstream checkout is not importable at {sh.REFERENCE_ROOT} (MDTILE_REFERENCE_ROOT)")
    out = os.path.join(HERE, "upstream.npz")
    env = dict(os.environ, MDTILE_RECORD_UPSTREAM=out)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu"] + MODULES, cwd=ROOT, env=env)
    if r.returncode != 0:
        raise SystemExit(f"pytest failed (rc {r.returncode}): upstream.npz was written from a failing run -- do not commit it")
    print("upstream.npz", os.path.getsize(out) // 1024, "KiB")


if __name__ == "__main__":
    main()
