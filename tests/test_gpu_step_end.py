"""The end of a small-batch step as one launch (FusedTrainStep.step_end: gtr_step_end_small,
whose weight-gradient tiles own their outputs and apply AdamW themselves) against the pair
it replaces (GTR_STEP_END=0: gtr_wgrad_rows + gtr_step_tail_small, split-K slabs summed by
the tail).  The new launch forms the same chunk values in the same order, so every
comparison is bit for bit (torch.equal)."""

from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only on the GPU box
    pytest.skip("no GPU", allow_module_level=True)

from gpu_helpers import batches, edge_case_batch, make_pair, small_data  # noqa: E402

from etpgt.backend import _lib as L  # noqa: E402
from etpgt.data.batch import Caps, collate_sessions  # noqa: E402
from etpgt.model import create_graph_transformer  # noqa: E402
from etpgt.train.fused import FusedTrainStep  # noqa: E402

DATA = None


def data():
    global DATA
    if DATA is None:
        DATA = small_data()
    return DATA


def _steps(monkeypatch, m1, caps, **kw):
    """Two steps over deep-copied models: the two launches (f1) and the default (f2)."""
    m2 = copy.deepcopy(m1)
    m1.train(); m2.train()
    monkeypatch.setenv("GTR_STEP_END", "0")
    f1 = FusedTrainStep(m1, caps=caps, **kw)
    monkeypatch.delenv("GTR_STEP_END")
    f2 = FusedTrainStep(m2, caps=caps, **kw)
    return m2, f1, f2


def _assert_same_state(m1, m2, f1, f2, where):
    f1.flush()
    f2.flush()
    for (name, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), (where, name)
    for (name, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
        if a is not None:
            assert torch.equal(a, b), (where, name)
    for name in ("m_tab", "v_tab", "m_flat", "v_flat"):
        assert torch.equal(getattr(f1, name), getattr(f2, name)), (where, name)


def _run_equal(monkeypatch, bl, D, H, K, loss, opt="adamw", lazy=False, caps=None, step_end=True, model=None):
    if caps is None:  # bound at construction, under the switch of each step
        sz = [b.sizes() for b in bl]
        caps = Caps.bucket(2 * max(s[0] for s in sz), max(s[1] for s in sz), 2 * max(s[2] for s in sz), sz[0][3])
    m1 = model if model is not None else make_pair(data().table_rows, D, H, K=K, dropout=0.1, seed=9)[0]
    m2, f1, f2 = _steps(monkeypatch, m1, caps, loss=loss, lazy=lazy, decoupled=opt == "adamw",
                        weight_decay=1e-2 if opt == "adamw" else 0.0)
    for i, sb in enumerate(bl):
        dsb = sb.to("cuda")
        l1, l2 = float(f1(dsb)), float(f2(dsb))
        assert np.isfinite(l1) and l1 == l2, (i, l1, l2)
        # the path each step took: the pair on one side, the one launch (or not) on the other
        assert f1.caps == caps and f2.caps == caps, i
        assert not f1.step_end and f2.step_end == step_end, i
        if model is None:
            assert f1.rows_early and f2.rows_early, i
        _assert_same_state(m1, m2, f1, f2, i)
    return f1, f2


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("D,H,K,loss,opt", [(64, 1, 0, "bpr", "adamw"), (128, 4, 16, "listwise", "adamw"),
                                            (32, 2, 8, "dual", "adamw"), (64, 2, 0, "bpr", "adam")])
def test_step_end_bitwise_equals_the_two_launches(D, H, K, loss, opt, lazy, monkeypatch):
    """Four steps on different batches (B = 32, dropout 0.1), state compared after every
    step: every job kind (MM, COLSUM at D a multiple of 64, the bias as ones column at
    D = 32, GATE, the LapPE gather with its bias column), D below and above the tile width,
    AdamW and coupled Adam, the eager table and the lazy one."""
    n = 100 if loss == "listwise" else 5
    _run_equal(monkeypatch, batches(data(), 32, n, 4, seed=17), D, H, K, loss, opt, lazy)


def _two_node_batch(T, n_neg=5):
    rng = np.random.default_rng(5)
    return collate_sessions([{"x": np.array([5, 9], np.int64), "edge_index": np.array([[0], [1]], np.int64),
                              "target_item": 11, "negative_items": rng.integers(12, T, size=n_neg).astype(np.int64)}])


@pytest.mark.parametrize("lazy", [False, True])
def test_step_end_one_session_of_two_nodes(lazy, monkeypatch):
    """B = 1: P = 1, a single chunk of two rows (14 zero slots in its one round)."""
    caps = Caps(18, 1, 16, 5)
    f1, f2 = _run_equal(monkeypatch, [_two_node_batch(data().table_rows)] * 3, 64, 2, 0, "bpr", lazy=lazy, caps=caps)
    assert f2.ws.P == 1


def test_step_end_late_chunks_empty(monkeypatch):
    """The two-node session in capacities with n_cap = 256, the gate's bound: P = 8,
    one row per chunk, chunks 2..7 empty."""
    caps = Caps(256, 1, 16, 5)
    f1, f2 = _run_equal(monkeypatch, [_two_node_batch(data().table_rows)] * 2, 64, 2, 0, "bpr", caps=caps)
    assert f2.ws.P == 8


def test_step_end_short_last_chunk_at_the_bound(monkeypatch):
    """B = 48 in n_cap = 256 with LapPE: P = 8 chunks of ceil(N / 8) rows in 32-slot rounds,
    the last chunk shorter than the others, none a multiple of the 8-row round."""
    bl = batches(data(), 48, 5, 2, seed=29)
    N = [b.num_nodes for b in bl]
    assert max(N) <= 256 and any(n % 8 for n in N), N
    caps = Caps(256, 48, 2 * max(b.num_edges for b in bl), 5)
    f1, f2 = _run_equal(monkeypatch, bl, 64, 2, 8, "bpr", caps=caps)
    assert f2.ws.P == 8


@pytest.mark.parametrize("lazy", [False, True])
def test_step_end_edge_case_batch(lazy, monkeypatch):
    """The three-session mixed batch of test_rows_early_edge_case_batch (a node with no
    in-edge, a session without edges, item 2 as node, target and negative) and
    edge_case_batch() through shared capacities."""
    sess = [
        {"x": np.array([1, 2, 3], np.int64), "edge_index": np.array([[0, 1, 1, 2], [1, 0, 2, 1]], np.int64),
         "target_item": 7, "negative_items": np.array([2, 20, 21, 22, 23], np.int64)},
        {"x": np.array([10, 2, 12], np.int64), "edge_index": np.array([[0, 0], [1, 2]], np.int64),
         "target_item": 2, "negative_items": np.array([30, 31, 32, 33, 34], np.int64)},
        {"x": np.array([30, 31], np.int64), "edge_index": np.zeros((2, 0), np.int64),
         "target_item": 3, "negative_items": np.array([40, 41, 42, 43, 1], np.int64)},
    ]
    _run_equal(monkeypatch, [collate_sessions(sess), edge_case_batch(), collate_sessions(sess)], 64, 2, 0, "bpr",
               lazy=lazy)


def test_step_end_off_just_above_the_row_bound(monkeypatch):
    """n_cap = 257: nine chunks of 32 slots do not fit the 256 of one staging round, so the
    step keeps gtr_wgrad_rows + gtr_step_tail_small whatever the switch says."""
    bl = batches(data(), 32, 5, 2, seed=17)
    caps = Caps(257, 32, 2 * max(b.num_edges for b in bl), 5)
    assert L.lib().gtr_step_end_small_fits(256, 8, 0) == 1 and L.lib().gtr_step_end_small_fits(257, 9, 0) == 0
    f1, f2 = _run_equal(monkeypatch, bl, 64, 2, 0, "bpr", caps=caps, step_end=False)
    assert f2.ws.P == 9


def test_step_end_off_with_forced_mfma_tiles(monkeypatch):
    """GTR_WGRAD=mfma puts the pair's weight gradients on MFMA tiles, whose sums the one
    launch (VALU) does not reproduce: it stays off."""
    monkeypatch.setenv("GTR_WGRAD", "mfma")
    _run_equal(monkeypatch, batches(data(), 32, 5, 2, seed=17), 64, 2, 0, "bpr", step_end=False)


def test_step_end_off_with_ffn_blocks(monkeypatch):
    """A model with FFN blocks keeps its own path: their weight gradients are slabs of
    gtr_ffn_wgrad, which only the tail sums."""
    torch.manual_seed(4)
    m = create_graph_transformer(data().table_rows, embedding_dim=64, hidden_dim=64, num_layers=2, num_heads=2,
                                 dropout=0.1, use_laplacian_pe=False, laplacian_k=1, use_ffn=True,
                                 ffn_expansion=2).cuda()
    bl = batches(data(), 32, 5, 2, seed=17)
    f1, f2 = _run_equal(monkeypatch, bl, 64, 2, 0, "bpr", step_end=False, model=m)
    assert f2.ws.ffns is not None
