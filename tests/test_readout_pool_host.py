"""Host side of the last / attention readouts (no GPU): the supported-variant check, the
flat parameter layout, the gtr_pool mirror and gtr_readout_pool's argument checks."""

import ctypes
import math
import os
import re

import pytest

from etpgt.model import create_graph_transformer_optimized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gtr.h")


@pytest.mark.parametrize("kind", ["last", "attention"])
def test_check_supported_accepts_last_and_attention(kind):
    m = create_graph_transformer_optimized(50, embedding_dim=32, hidden_dim=32, use_laplacian_pe=False,
                                           readout_type=kind)
    m._check_supported()


def test_max_is_still_rejected_and_says_so():
    m = create_graph_transformer_optimized(50, embedding_dim=32, hidden_dim=32, use_laplacian_pe=False,
                                           readout_type="max")
    with pytest.raises(NotImplementedError, match="max"):
        m._check_supported()


def _expected_layout(D, L_, K):
    """Segment names and offsets from the sizes alone (256-aligned, in declaration order)."""
    names, off = [], 0
    sizes = []
    for l in range(L_):
        sizes += [(f"{l}.w_all", 4 * D * D), (f"{l}.b_all", 4 * D), (f"{l}.w_beta", 3 * D), (f"{l}.gamma", D),
                  (f"{l}.beta", D)]
    if K > 0:
        sizes += [("pe.w", D * K), ("pe.b", D)]
    for n, sz in sizes:
        names.append((n, off, sz))
        off += (sz + 255) // 256 * 256
    return names, off


@pytest.mark.parametrize("D,L_,K", [(32, 2, 0), (64, 3, 16), (256, 2, 4)])
def test_param_layout_of_mean_and_last_is_unchanged(D, L_, K):
    from etpgt.backend.engine import ParamLayout

    want, total = _expected_layout(D, L_, K)
    for kind in ("mean", "last"):
        lay = ParamLayout(D, L_, K, readout=kind)
        assert [(s.name, s.begin, s.numel) for s in lay.segs.values()] == want
        assert lay.total == total
    assert [(s.name, s.begin, s.numel) for s in ParamLayout(D, L_, K).segs.values()] == want


@pytest.mark.parametrize("D,L_,K", [(32, 2, 0), (64, 3, 16), (256, 2, 4)])
def test_param_layout_of_attention_appends_ro_segments(D, L_, K):
    from etpgt.backend.engine import ParamLayout

    want, total = _expected_layout(D, L_, K)
    lay = ParamLayout(D, L_, K, readout="attention")
    got = [(s.name, s.begin, s.numel) for s in lay.segs.values()]
    assert got[:-2] == want  # everything before them is today's layout, pe.* included
    assert got[-2] == ("ro.w", total, D) and lay.seg("ro.w").shape == (1, D)
    assert got[-1] == ("ro.b", total + (D + 255) // 256 * 256, 1) and lay.seg("ro.b").shape == (1,)
    assert all(b % 256 == 0 for _, b, _ in got)
    assert lay.total == got[-1][1] + 256
    for kind in ("mean", "last"):
        assert "ro.w" not in ParamLayout(D, L_, K, readout=kind).segs


def test_model_param_map_points_the_attention_parameters_into_the_flat_buffer():
    from etpgt.backend.engine import model_param_map

    m = create_graph_transformer_optimized(50, embedding_dim=32, hidden_dim=32, use_laplacian_pe=False,
                                           readout_type="attention")
    mp = {name: p for name, p, _ in model_param_map(m)}
    assert mp["ro.w"] is m.readout.attention.weight and mp["ro.b"] is m.readout.attention.bias
    assert math.prod(mp["ro.w"].shape) == 32
    for kind in ("mean", "last"):
        m2 = create_graph_transformer_optimized(50, embedding_dim=32, hidden_dim=32, use_laplacian_pe=False,
                                                readout_type=kind)
        assert not any(name.startswith("ro.") for name, _, _ in model_param_map(m2))


def test_gtr_pool_mirror_matches_header():
    """Field order of gtr_pool against _lib.GtrPool, by test_abi.py's header parse."""
    from etpgt.backend import _lib

    src = open(HEADER).read()
    body = re.search(r"typedef struct gtr_pool \{(.*?)\} gtr_pool;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        parts = [t for t in decl.replace("*", " ").split() if t not in ("struct", "const")]
        names += [n.split("[")[0].strip() for n in " ".join(parts[1:]).split(",") if n.strip()]
    assert [f[0] for f in _lib.GtrPool._fields_] == names
    for name, val in (("GTR_POOL_MEAN", 0), ("GTR_POOL_LAST", 1), ("GTR_POOL_ATTENTION", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), src), name
    assert _lib.GTR_POOL == {"mean": 0, "last": 1, "attention": 2}
    assert "gtr_readout_pool" in _lib.EXPORTS
    assert re.search(r"#define GTR_ABI_VERSION 9\b", src)


def _pool_call(pool, cfg=None):
    from etpgt.backend import _lib

    lib = _lib.lib()
    cfg = cfg or _lib.GtrConfig(num_items=100, dim=64, heads=2, num_layers=2, training=1, row_group=16)
    bt = _lib.GtrBatch(n_cap=64, b_cap=4, e_cap=64, n_neg=5)
    layers = (_lib.GtrLayer * 2)()
    head = _lib.GtrHead(flags=_lib.RO_FWD)
    rc = lib.gtr_readout_pool(ctypes.byref(cfg), ctypes.byref(bt), None, layers, ctypes.byref(head),
                              ctypes.byref(pool), None)
    return rc, lib.gtr_last_error().decode()


def test_readout_pool_refuses_an_unknown_kind():
    from etpgt.backend import _lib

    rc, msg = _pool_call(_lib.GtrPool(kind=3))
    assert rc != 0
    assert "kind 3" in msg


def test_readout_pool_refuses_attention_without_its_buffers():
    from etpgt.backend import _lib

    rc, msg = _pool_call(_lib.GtrPool(kind=_lib.GTR_POOL["attention"]))  # w (and the rest) NULL
    assert rc != 0
    assert "attention" in msg and "w" in msg


@pytest.mark.parametrize("field", ["sync_bn", "split_sync"])
def test_readout_pool_refuses_syncbn(field):
    from etpgt.backend import _lib

    cfg = _lib.GtrConfig(num_items=100, dim=64, heads=2, num_layers=2, training=1, row_group=16,
                         consumer_reduce=1)
    setattr(cfg, field, 1)
    rc, msg = _pool_call(_lib.GtrPool(kind=_lib.GTR_POOL["last"]), cfg)
    assert rc != 0
    assert "SyncBN" in msg
