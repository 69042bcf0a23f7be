"""Batched serving, the parts that need no GPU: the C ABI declares the request builder,
the binding mirrors it, ``Recommender.recommend_batch`` exists, and the host-side request
validation raises what the single-request route raises -- before anything is uploaded."""

import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gtr.h")


def test_header_and_binding_declare_the_request_builder():
    from etpgt.backend import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = set(re.findall(r"\b(gtr_[a-z_0-9]+)\s*\(", src))
    for name in ("gtr_serve_counts", "gtr_serve_build"):
        assert name in fns, name
        assert name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+GTR_ABI_VERSION\s+9\b", src)
    body = re.search(r"typedef struct gtr_requests \{(.*?)\} gtr_requests;", src, re.S).group(1)
    names = [d.replace("*", " ").split()[-1] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.GtrRequests._fields_]


def test_recommender_has_recommend_batch():
    from etpgt.serving import Recommender

    assert callable(getattr(Recommender, "recommend_batch"))
    assert callable(getattr(Recommender, "recommend"))


def test_request_validation_raises_before_any_upload():
    import numpy as np

    from etpgt.data.gpu_batch import MAX_REQUEST_ITEMS, pack_requests

    T = 100
    ptr, items = pack_requests([[5, 3, 5], [0], list(range(1, 65))], T)
    assert ptr.dtype == np.int32 and items.dtype == np.int32
    assert ptr.tolist() == [0, 3, 4, 68] and items[:4].tolist() == [5, 3, 5, 0]
    assert MAX_REQUEST_ITEMS == 64
    with pytest.raises(ValueError, match="session_items must not be empty"):
        pack_requests([[1, 2], []], T)
    with pytest.raises(ValueError, match="64"):
        pack_requests([[1], list(range(1, 66))], T)
    with pytest.raises(IndexError):
        pack_requests([[1, T]], T)
    with pytest.raises(IndexError):
        pack_requests([[1], [-1, 2]], T)
    ptr, items = pack_requests([], T)
    assert ptr.tolist() == [0] and items.size == 0
