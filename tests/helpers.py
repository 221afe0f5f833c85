"""Shared helpers for the test-suite: fixtures of the reference's ring-buffer tests, and the float comparison rule."""
import json
import os

import numpy as np

# the class rule of every float comparison (NaN meets NaN, an infinity the same infinity, anything else non-finite is
# an infinite error): written once, beside `testing.compare`, which cannot import from tests/
from sub_volume_renderer_amd.testing import class_error, same_bits_or_nan  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

with open(os.path.join(GOLDEN, "ring_known_answers.json")) as f:
    KNOWN = json.load(f)


def fixture_arrays(name):
    fx = KNOWN["fixtures"][name]
    shape = tuple(fx["data_shape"])
    data = np.arange(int(np.prod(shape)), dtype=fx["dtype"]).reshape(shape)
    seg = np.zeros(shape, dtype=fx["dtype"])
    return data, seg, tuple(fx["ring_chunks"]), tuple(fx["chunk"])


def slices(r):
    return tuple(slice(o, o + s) for o, s in zip(r[0], r[1]))


def as_pair(r):
    return (tuple(r[0]), tuple(r[1]))


def assert_close(got, ref, tol, what=""):
    """Every element within `tol` under the class rule; returns the largest error."""
    err = class_error(got, ref)
    worst = float(err.max(initial=0.0))
    assert worst <= tol, (what, worst, int((err > tol).sum()))
    return worst


def assert_same_bits(got, ref, what=""):
    bad = int((~same_bits_or_nan(got, ref)).sum())
    assert bad == 0, (what, bad)
