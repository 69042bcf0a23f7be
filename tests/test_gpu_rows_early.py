"""The touched-row AdamW beside the weight gradients (FusedTrainStep.rows_early:
gtr_wgrad_rows + gtr_step_tail_small) against the two plain launches (GTR_ROWS_EARLY=0:
gtr_wgrad + gtr_step_tail).  The change moves work between launches and changes no
arithmetic, so every comparison is bit for bit (torch.equal)."""

from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only on the GPU box
    pytest.skip("no GPU", allow_module_level=True)

from gpu_helpers import batches, edge_case_batch, make_pair, small_data  # noqa: E402

from etpgt.backend import _lib as L  # noqa: E402
from etpgt.data.batch import Caps, collate_sessions  # noqa: E402
from etpgt.train.fused import FusedTrainStep  # noqa: E402

DATA = None


def data():
    global DATA
    if DATA is None:
        DATA = small_data()
    return DATA


def _pair(monkeypatch, D, H, K, loss, opt="adamw", lazy=False, caps=None, seed=9):
    """Two steps over deep-copied models: the plain launches (f1) and the default (f2)."""
    T = data().table_rows
    m1, _ = make_pair(T, D, H, K=K, dropout=0.1, seed=seed)
    m2 = copy.deepcopy(m1)
    m1.train(); m2.train()
    kw = dict(loss=loss, lazy=lazy, caps=caps, decoupled=opt == "adamw", weight_decay=1e-2 if opt == "adamw" else 0.0)
    monkeypatch.setenv("GTR_ROWS_EARLY", "0")
    f1 = FusedTrainStep(m1, **kw)
    monkeypatch.delenv("GTR_ROWS_EARLY")
    f2 = FusedTrainStep(m2, **kw)
    return m1, m2, f1, f2


def _assert_same_state(m1, m2, f1, f2):
    f1.flush()
    f2.flush()
    for (name, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), name
    for (name, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
        if a is not None:
            assert torch.equal(a, b), name
    for name in ("m_tab", "v_tab", "m_flat", "v_flat"):
        assert torch.equal(getattr(f1, name), getattr(f2, name)), name


def _run_equal(monkeypatch, bl, D, H, K, loss, opt="adamw", lazy=False, caps=None, early=True):
    if caps is None:  # bound at construction, under the switch of each step
        sz = [b.sizes() for b in bl]
        caps = Caps.bucket(2 * max(s[0] for s in sz), max(s[1] for s in sz), 2 * max(s[2] for s in sz), sz[0][3])
    m1, m2, f1, f2 = _pair(monkeypatch, D, H, K, loss, opt, lazy, caps)
    for i, sb in enumerate(bl):
        dsb = sb.to("cuda")
        l1, l2 = float(f1(dsb)), float(f2(dsb))
        assert np.isfinite(l1) and l1 == l2, (i, l1, l2)
        if i == 0:
            assert not f1.rows_early and f2.rows_early == early
    _assert_same_state(m1, m2, f1, f2)
    return f1, f2


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("D,H,K,loss,opt,wgrad", [
    pytest.param(64, 1, 0, "bpr", "adamw", None, id="64-1-0-bpr-adamw"),
    pytest.param(128, 4, 16, "listwise", "adamw", None, id="128-4-16-listwise-adamw"),
    pytest.param(128, 4, 16, "listwise", "adamw", "mfma", id="128-4-16-listwise-adamw-mfma"),
    pytest.param(32, 2, 8, "dual", "adamw", None, id="32-2-8-dual-adamw"),
    pytest.param(64, 2, 0, "bpr", "adam", None, id="64-2-0-bpr-adam")])
def test_rows_early_bitwise_equals_separate_launches(D, H, K, loss, opt, wgrad, lazy, monkeypatch):
    """Four steps on different batches (B = 32, dropout 0.1): every step's loss, every
    parameter and buffer and the AdamW moments of the table and of the flat parameters,
    with the eager table and with the lazy one; GTR_WGRAD=mfma forces the MFMA tiles onto
    both sides' 32-row chunks (where the one-launch end stays off)."""
    if wgrad:
        monkeypatch.setenv("GTR_WGRAD", wgrad)
    n = 100 if loss == "listwise" else 5
    _run_equal(monkeypatch, batches(data(), 32, n, 4, seed=17), D, H, K, loss, opt, lazy)


def _two_node_batch(T, n_neg=5):
    rng = np.random.default_rng(5)
    return collate_sessions([{"x": np.array([5, 9], np.int64), "edge_index": np.array([[0], [1]], np.int64),
                              "target_item": 11, "negative_items": rng.integers(12, T, size=n_neg).astype(np.int64)}])


@pytest.mark.parametrize("lazy", [False, True])
def test_rows_early_one_session_of_two_nodes(lazy, monkeypatch):
    """B = 1: one split-K chunk (n_cap 18 <= 32 rows), and m_cap = 18 + 6 = 24 slots of 16
    float4 lanes = 1.5 row workgroups: the second one's upper half lies past m_cap."""
    caps = Caps(18, 1, 16, 5)
    f1, f2 = _run_equal(monkeypatch, [_two_node_batch(data().table_rows)] * 3, 64, 2, 0, "bpr", lazy=lazy, caps=caps)
    assert f2.ws.P == 1 and (f2.m_cap * 16) % 256 != 0


@pytest.mark.parametrize("lazy", [False, True])
def test_rows_early_edge_case_batch(lazy, monkeypatch):
    """B = 3 in the manner of edge_case_batch() (a node with no in-edge, a session without
    edges) with item 2 as a node of two sessions, the target of one and a negative of
    another, so its segment mixes dx0 rows with both kinds of readout coefficients; then
    edge_case_batch() itself (B = 6) through the same capacities."""
    sess = [
        {"x": np.array([1, 2, 3], np.int64), "edge_index": np.array([[0, 1, 1, 2], [1, 0, 2, 1]], np.int64),
         "target_item": 7, "negative_items": np.array([2, 20, 21, 22, 23], np.int64)},
        {"x": np.array([10, 2, 12], np.int64), "edge_index": np.array([[0, 0], [1, 2]], np.int64),  # node 0: no in-edge
         "target_item": 2, "negative_items": np.array([30, 31, 32, 33, 34], np.int64)},
        {"x": np.array([30, 31], np.int64), "edge_index": np.zeros((2, 0), np.int64),  # no edges at all
         "target_item": 3, "negative_items": np.array([40, 41, 42, 43, 1], np.int64)},
    ]
    _run_equal(monkeypatch, [collate_sessions(sess), edge_case_batch(), collate_sessions(sess)], 64, 2, 0, "bpr",
               lazy=lazy)


def test_rows_early_batch_well_below_capacity(monkeypatch):
    """Batches of 8 sessions staged through the capacities of a 64-session batch: padding
    node rows, and split-K chunks past N that sum no rows at all."""
    big = batches(data(), 64, 5, 1, seed=3)[0]
    caps = Caps(big.num_nodes, 64, big.num_edges, 5)
    bl = batches(data(), 8, 5, 3, seed=21)
    f1, f2 = _run_equal(monkeypatch, bl, 64, 2, 0, "bpr", caps=caps)
    assert f2.ws.P > 1 and max(b.num_nodes for b in bl) * 2 < caps.n_cap


def test_rows_early_just_under_the_windowed_threshold(monkeypatch):
    """m_cap = 5120 + 512 * 6 = 8192, the largest non-windowed capacity: rows_early on (512
    row workgroups; 320 row groups, so the tail also sweeps the untouched rows)."""
    caps = Caps(5120, 512, 16384, 5)
    f1, f2 = _run_equal(monkeypatch, batches(data(), 96, 5, 2, seed=23), 64, 2, 0, "bpr", caps=caps)
    assert f2.m_cap == 8192


def test_rows_early_off_just_over_the_windowed_threshold(monkeypatch):
    """m_cap = 8208 > 8192: the windowed tail, rows_early off whatever the switch says, and
    the step trains as with the switch off (bit for bit)."""
    caps = Caps(5136, 512, 16384, 5)
    f1, f2 = _run_equal(monkeypatch, batches(data(), 96, 5, 2, seed=23), 64, 2, 0, "bpr", caps=caps, early=False)
    assert f2.m_cap == 8208


@pytest.mark.parametrize("lazy", [False, True])
def test_rows_early_multi_step_graph_equals_plain_per_step(lazy, monkeypatch):
    """K steps as one captured graph over resident images (bind_resident + capture_steps)
    with rows_early on against K per-step launches with it off: the loss of every replay,
    parameters and moments."""
    bl = batches(data(), 32, 5, 3, seed=15)
    caps = Caps(max(b.num_nodes for b in bl), 32, max(b.num_edges for b in bl), 5)
    m1, m2, f1, f2 = _pair(monkeypatch, 64, 2, 0, "bpr", lazy=lazy, caps=caps)
    assert not f1.rows_early and f2.rows_early
    f2.bind_resident([torch.from_numpy(b.packed(f2.caps)[1]).cuda() for b in bl])
    for i in range(2):
        assert float(f1(bl[i].to("cuda"))) == float(f2.run_resident(i))
    f2.prepare_resident()
    h = f2.capture_steps(2, 4)  # images 2, 0, 1, 2
    for rep in range(2):
        for k in range(4):
            l1 = float(f1(bl[(2 + k) % 3].to("cuda")))
        assert l1 == float(f2.run_steps(h)), rep
    assert f1.steps == f2.steps == 10
    _assert_same_state(m1, m2, f1, f2)


@pytest.mark.parametrize("D,H,K,loss,B", [(64, 1, 0, "bpr", 32), (128, 4, 16, "listwise", 32), (32, 2, 8, "dual", 32),
                                          (64, 2, 0, "bpr", 1400)])
def test_small_body_wave_bitwise_equals_per_element_search(D, H, K, loss, B, monkeypatch):
    """The tail's small-parameter part with the segment found once per wave
    (small_body_wave, the default for 64-aligned segments) against the per-element search
    (GTR_SMALL_WAVE=0): losses, parameters, buffers and moments bit for bit; B = 32 (the
    small-only tail after gtr_wgrad_rows) and B = 1400 (the windowed tail)."""
    T = data().table_rows
    n = 100 if loss == "listwise" else 5
    m1, _ = make_pair(T, D, H, K=K, dropout=0.1, seed=5)
    m2 = copy.deepcopy(m1)
    m1.train(); m2.train()
    f1, f2 = FusedTrainStep(m1, loss=loss), FusedTrainStep(m2, loss=loss)
    for sb in batches(data(), B, n, 3, seed=31):
        dsb = sb.to("cuda")
        monkeypatch.setenv("GTR_SMALL_WAVE", "0")  # read at every launch (eager and capture)
        l1 = float(f1(dsb))
        monkeypatch.delenv("GTR_SMALL_WAVE")
        assert l1 == float(f2(dsb))
    _assert_same_state(m1, m2, f1, f2)


def test_rows_early_entry_points_refuse_bad_arguments():
    """gtr_wgrad_rows and gtr_step_tail_small: GTR_E_ARG with a gtr_last_error text for a
    windowed capacity (m_cap > 8192) and for a null table pointer.  Host side only: both
    are refused before any launch."""
    m, _ = make_pair(data().table_rows, 64, 2, K=0, seed=1)
    f = FusedTrainStep(m.train(), loss="bpr", caps=Caps(64, 8, 128, 5))
    lib, eng, ws = L.lib(), f.eng, f.ws
    big = L.GtrBatch.from_buffer_copy(f.bs)
    big.n_cap = 8192  # m_cap = 8192 + 8 * 6
    notab = L.GtrTail.from_buffer_copy(f.tail)
    notab.table = None

    def wgrad_rows(bs, tail):
        return lib.gtr_wgrad_rows(C.byref(f.cfg), C.byref(bs), ws.structs, ws.dx0.data_ptr(), None, ws.slab_ptrs,
                                  None, ws.P, eng.flat.layout.slab_stride, 0, eng.L, eng.T, C.byref(tail),
                                  C.byref(f.adam), None)

    def tail_small(bs, tail):
        return lib.gtr_step_tail_small(C.byref(bs), eng.T, eng.D, C.byref(tail), f.segs, f.nseg, C.byref(f.adam),
                                       None)

    for fn, name in ((wgrad_rows, "gtr_wgrad_rows"), (tail_small, "gtr_step_tail_small")):
        assert fn(big, f.tail) == 1001
        err = lib.gtr_last_error().decode()
        assert name in err and "too large" in err, err
        assert fn(f.bs, notab) == 1001
        err = lib.gtr_last_error().decode()
        assert name in err and "missing buffers" in err, err
