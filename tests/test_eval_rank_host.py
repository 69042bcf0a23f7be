"""Host side of the rank-based evaluation (no GPU): Recall@K / NDCG@K from target ranks
equal the prediction-based functions bit for bit, the C ABI carries gtr_target_rank, the
op traces under fake tensors, and the drop-in script has its --device-eval flag."""

import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from etpgt.utils.metrics import compute_metrics_from_ranks, compute_ndcg_at_k, compute_recall_at_k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gtr.h")
NEW = ("gtr_target_rank_workspace_bytes", "gtr_target_rank")
KS = [1, 10, 20]


def _preds_and_ranks(scores: np.ndarray, targets: np.ndarray):
    """Full ordering by score descending, id ascending on ties (stable sort), and each
    target's rank by counting; a target outside the table ranks T."""
    S, T = scores.shape
    order = np.argsort(-scores, axis=1, kind="stable")
    ranks = np.empty(S, np.int64)
    for b in range(S):
        t = int(targets[b])
        if not 0 <= t < T:
            ranks[b] = T
            continue
        s = scores[b]
        ranks[b] = int((s > s[t]).sum() + ((s == s[t]) & (np.arange(T) < t)).sum())
        assert order[b, ranks[b]] == t
    return torch.from_numpy(order), torch.from_numpy(ranks)


def _both(preds, targets, ranks):
    want = {}
    for k in KS:
        want[f"recall@{k}"] = compute_recall_at_k(preds[:, :k], targets, k=k)
        want[f"ndcg@{k}"] = compute_ndcg_at_k(preds[:, :k], targets, k=k)
    return want, compute_metrics_from_ranks(ranks, KS)


@pytest.mark.parametrize("S", [257, 1])
def test_metrics_from_ranks_equal_the_prediction_metrics(S):
    rng = np.random.default_rng(S)
    T = 40
    scores = rng.integers(-3, 4, size=(S, T)).astype(np.float32)  # 7 values over 40 items: many ties
    targets = rng.integers(0, T, size=S)
    if S > 4:
        targets[3] = T  # outside the table: rank T, a miss at every k
        targets[4] = -1
    preds, ranks = _preds_and_ranks(scores, targets)
    assert S == 1 or (bool((ranks >= 20).any()) and bool((ranks < 1).any()) and bool((ranks == T).any()))
    want, got = _both(preds, torch.from_numpy(targets), ranks)
    assert got == want  # floats compared with ==: no tolerance
    assert set(got) == {f"{m}@{k}" for m in ("recall", "ndcg") for k in KS}
    # int32 device-style ranks give the same
    assert compute_metrics_from_ranks(ranks.to(torch.int32), KS) == want


def test_metrics_from_ranks_all_hits_and_all_misses():
    T = 40
    targets = torch.arange(30)
    preds = torch.arange(T).repeat(30, 1)  # target b sits in column b
    want, got = _both(preds, targets, targets.clone())
    assert got == want and got["recall@1"] == pytest.approx(1 / 30)
    miss = torch.full((30,), T)
    want, got = _both(preds, miss, miss)
    assert got == want and got["recall@20"] == 0.0 and got["ndcg@20"] == 0.0


def _header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(gtr_[a-z_0-9]+)\s*\(", src))


def test_abi_declares_exports_and_binds_target_rank():
    from etpgt.backend import _lib

    fns = _header_functions()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in fns, f"{name} not declared in include/gtr.h"
        assert hasattr(h, name), f"{name} not exported by libgtr_hip.so"
        assert name in _lib.EXPORTS
    assert _lib.lib().gtr_abi_version() == 9


def test_target_rank_null_arguments_return_an_error():
    from etpgt.backend import _lib

    lib = _lib.lib()
    rc = lib.gtr_target_rank(None, 4, 64, None, 100, None, None, 4, None, None, None, 0, None)
    assert rc != 0
    with pytest.raises(RuntimeError, match="gtr_target_rank"):
        _lib.check(rc, "target_rank")
    assert lib.gtr_target_rank_workspace_bytes(4, 100, None) != 0
    nb = ctypes.c_size_t(0)
    assert lib.gtr_target_rank_workspace_bytes(4, 100, ctypes.byref(nb)) == 0 and nb.value >= 4 * 8
    # an unsupported dim is refused before any device work (pointers are not dereferenced)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    rc = lib.gtr_target_rank(p, 4, 48, p, 100, p, p, 4, None, None, p, 512, None)
    assert rc != 0 and b"dim 48" in lib.gtr_last_error()
    # pos without base
    rc = lib.gtr_target_rank(p, 4, 64, p, 100, p, p, 4, p, None, p, 512, None)
    assert rc != 0


def test_target_rank_op_under_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from etpgt.backend import ops  # noqa: F401  (registers etpgt::target_rank)

    with FakeTensorMode():
        se = torch.empty(7, 64)
        table = torch.empty(300, 64)
        tgt = torch.empty(7, dtype=torch.int64)
        out = torch.ops.etpgt.target_rank(se, table, tgt)
    assert tuple(out.shape) == (7,) and out.dtype == torch.int32


def test_target_rank_refuses_cpu_tensors():
    from etpgt.backend.ops import target_rank

    with pytest.raises(RuntimeError, match="HIP path only"):
        target_rank(torch.randn(4, 64), torch.randn(100, 64), torch.tensor([1, 2, 3, 4]))


def test_model_api_and_evaluator_import():
    from etpgt.model.base import BaseRecommendationModel
    from etpgt.train.evaluator import DeviceEvaluator

    assert callable(BaseRecommendationModel.rank_targets) and callable(DeviceEvaluator.run)


def test_script_device_eval_flag_defaults_off():
    path = os.path.join(ROOT, "scripts", "train", "train_baseline.py")
    spec = importlib.util.spec_from_file_location("train_baseline_cli", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--model", "graph_transformer"]).device_eval == "off"
    assert mod.parse_args(["--model", "graph_transformer", "--device-eval", "on"]).device_eval == "on"
