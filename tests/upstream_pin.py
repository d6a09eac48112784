"""Upstream's side of the oracle-vs-reference comparisons, stored so that they run without the upstream checkout.

`Upstream.equal(key, fn, mine)` is True when the product / oracle value `mine` equals what the upstream code returns:
  * the upstream checkout importable (hostsim/stub_host.reference_available): `fn(ref)` runs on it, and the stored pin of `key` in
    tests/golden/upstream.npz must match that live value too (a stale fixture fails instead of passing quietly);
  * otherwise: `mine` is compared with the stored pin.
A pin is the value itself for small arrays and plain data (JSON), and the SHA-256 of the canonical bytes (+ shape, dtype) for arrays
above PIN_MAX_ELEMS elements: both are exact, like torch.equal.  Tuples and lists that hold tensors are pinned element by element.

Regenerate the fixture (needs the upstream checkout): python tests/golden/make_golden_upstream.py
"""
from __future__ import annotations

import atexit
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upstream.npz")
RECORD_ENV = "MDTILE_RECORD_UPSTREAM"      # set by make_golden_upstream.py: write every live upstream value to this path
PIN_MAX_ELEMS = 8192


def _has_tensor(v) -> bool:
    return isinstance(v, (torch.Tensor, np.ndarray)) or (isinstance(v, (tuple, list)) and any(_has_tensor(e) for e in v))


def pin(key: str, v) -> dict:
    """Flat {key: np.ndarray} pin of a value (see the module docstring)."""
    if isinstance(v, (tuple, list)) and _has_tensor(v):
        out = {}
        for i, e in enumerate(v):
            out.update(pin(f"{key}/{i}", e))
        return out
    if isinstance(v, (torch.Tensor, np.ndarray)):
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v
        a = np.ascontiguousarray(a)
        if a.dtype.kind == "f":
            a = a + a.dtype.type(0)         # -0.0 -> +0.0: torch.equal treats them as equal
        if a.size <= PIN_MAX_ELEMS:
            return {key: a}
        digest = hashlib.sha256(a.tobytes()).hexdigest()
        return {key + "#sha256": np.array(json.dumps([digest, list(a.shape), str(a.dtype)]))}
    return {key + "#json": np.array(json.dumps(v))}


def same(a: dict, b: dict) -> bool:
    if a.keys() != b.keys():
        return False
    for k in a:
        x, y = a[k], b[k]
        if k.endswith("#sha256") or k.endswith("#json"):
            if str(x) != str(y):
                return False
        elif x.dtype != y.dtype or not np.array_equal(x, y):
            return False
    return True


def _subset(store, key: str) -> dict:
    names = store.files if hasattr(store, "files") else list(store)
    return {k: store[k] for k in names if k.split("#")[0] == key or k.startswith(key + "/")}


class Upstream:
    def __init__(self):
        self.ref = sh.load_reference() if sh.reference_available() else None
        self.stored = np.load(GOLDEN) if os.path.exists(GOLDEN) else {}
        self.record = os.environ.get(RECORD_ENV)
        self.recorded = {}
        if self.record:
            if self.ref is None:
                raise RuntimeError(f"{RECORD_ENV} is set but the upstream checkout is not importable")
            atexit.register(lambda: np.savez_compressed(self.record, **self.recorded))

    def equal(self, key: str, fn, mine) -> bool:
        got = pin(key, mine)
        if self.ref is None:
            want = _subset(self.stored, key)
            if not want:
                pytest.fail(f"tests/golden/upstream.npz has no pin for {key!r}: regenerate it with tests/golden/make_golden_upstream.py")
        else:
            want = pin(key, fn(self.ref))
            self.recorded.update(want)
            if not self.record:
                assert same(want, _subset(self.stored, key)), f"tests/golden/upstream.npz is stale for {key!r} (regenerate it)"
        return same(want, got)


_UPSTREAM = None


def upstream() -> Upstream:
    global _UPSTREAM
    if _UPSTREAM is None:
        _UPSTREAM = Upstream()
    return _UPSTREAM
