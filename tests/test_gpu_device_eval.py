"""Validation on the device: Trainer.evaluate from target ranks (host-loader route) and
the captured build -> eval forward -> target-rank chain (DeviceEvaluator) against the
prediction-based computation they replace.  Every comparison is exact: the routes run the
same forward kernels on the same sessions and form the same score keys.

Data: reference-format CSVs with 70 validation sessions, batch size 16 (four full batches
and a partial one of 6).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only on the GPU box
    pytest.skip("no GPU", allow_module_level=True)

from dropin_helpers import write_csvs  # noqa: E402

from etpgt.model import create_graph_transformer_optimized  # noqa: E402
from etpgt.train.dataloader import create_dataloader  # noqa: E402
from etpgt.train.evaluator import GUARD, DeviceEvaluator  # noqa: E402
from etpgt.train.trainer import Trainer  # noqa: E402
from etpgt.utils.metrics import compute_ndcg_at_k, compute_recall_at_k  # noqa: E402

S_VAL, BATCH, KS = 70, 16, [1, 10, 20]


@pytest.fixture(scope="module")
def csvs(tmp_path_factory):
    return write_csvs(tmp_path_factory.mktemp("device_eval"), num_items=120, num_train=20, num_val=S_VAL, seed=7)


def _loader(csvs, device_builder):
    return create_dataloader(csvs / "val.csv", csvs / "graph_edges.csv", batch_size=BATCH, num_negatives=5,
                             shuffle=False, num_workers=0, device_builder=device_builder)


def _model(T, D=32, K=0, ffn=False, seed=11):
    """Trained-looking weights: random table, BatchNorm affine and running statistics."""
    torch.manual_seed(seed)
    m = create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=2, num_heads=2, dropout=0.0,
                                           use_laplacian_pe=K > 0, laplacian_k=max(K, 1), use_ffn=ffn,
                                           ffn_expansion=4)
    with torch.no_grad():
        m.item_embedding.weight[1:].normal_(0.0, 0.3)
        for bn in m.batch_norms:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
            bn.running_mean.uniform_(-0.3, 0.3)
            bn.running_var.uniform_(0.5, 2.0)
        if K > 0:
            m.laplacian_pe._cached_pe = torch.rand(T, K)
    m = m.cuda().eval()
    if K > 0:
        m.laplacian_pe._cached_pe = m.laplacian_pe._cached_pe.cuda()
    return m


def _trainer(m, loader, tmp_path):
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    return Trainer(m, [], loader, opt, device="cuda", output_dir=tmp_path, k_values=KS)


@torch.no_grad()
def _parent_metrics(m, loader):
    """Trainer.evaluate as it was: predict top-k per batch, ids to the host, metrics."""
    preds, targets = [], []
    for batch in loader:
        batch = batch.to("cuda")
        se = m(batch)
        preds.append(m.predict(se, k=max(KS)).cpu())
        targets.append(batch.target_item.cpu())
    preds, targets = torch.cat(preds), torch.cat(targets)
    out = {}
    for k in KS:
        out[f"recall@{k}"] = compute_recall_at_k(preds[:, :k], targets, k=k)
        out[f"ndcg@{k}"] = compute_ndcg_at_k(preds[:, :k], targets, k=k)
    return out


@torch.no_grad()
def _host_route_ranks(m, loader):
    ranks = [m.rank_targets(m(b.to("cuda")), b.to("cuda").target_item) for b in loader]
    return torch.cat(ranks).cpu()


@pytest.fixture(scope="module")
def base(csvs):
    """The d=32 model, the host loader and the reference metrics / ranks, computed once."""
    host = _loader(csvs, False)
    m = _model(host.dataset.num_items)
    return {"m": m, "host": host, "parent": _parent_metrics(m, host), "ranks": _host_route_ranks(m, host)}


def test_host_loader_route_equals_the_prediction_metrics(base, tmp_path):
    assert len(base["host"].dataset) == S_VAL and base["ranks"].shape == (S_VAL,)
    got = _trainer(base["m"], base["host"], tmp_path).evaluate()
    assert got == base["parent"]
    assert 0.0 < got["recall@20"] < 1.0  # hits and misses both occur


def test_evaluator_eager_equals_the_host_loader_route(base, csvs):
    ev = DeviceEvaluator(base["m"], _loader(csvs, True), use_graph=False)
    got = ev.run()
    assert got.dtype == torch.int32 and got.tolist() == base["ranks"].tolist()
    assert ev.captures == 0


@pytest.mark.parametrize("per_graph,graphs", [(16, 1), (2, 2)])
def test_evaluator_graph_equals_eager_across_epochs(base, csvs, per_graph, graphs):
    """Four full batches: the first eager, then three one-batch replays (16 per graph: none
    fills one) or a two-batch graph and a one-batch graph (2 per graph)."""
    ev = DeviceEvaluator(base["m"], _loader(csvs, True), use_graph=True, batches_per_graph=per_graph)
    for epoch in range(2):
        ev.ranks.fill_(-1)
        got = ev.run()
        assert got.tolist() == base["ranks"].tolist(), epoch
        buf = ev.ranks.cpu()
        assert buf.numel() == S_VAL + GUARD and bool((buf[:S_VAL] >= 0).all())
        assert buf[S_VAL:].tolist() == [-1] * GUARD
    assert ev.captures == graphs  # captured once, replayed for the full batches of both epochs
    ev.close()
    assert ev.run().tolist() == base["ranks"].tolist() and ev.captures == 2 * graphs


def test_trainer_device_loader_rng_and_metrics(base, csvs, tmp_path):
    loader = _loader(csvs, True)
    tr = _trainer(base["m"], loader, tmp_path)
    torch.manual_seed(5)
    got = tr.evaluate()
    after_eval = torch.get_rng_state()
    again = tr.evaluate()  # second epoch: the kept evaluator, its captured graph
    assert tr._evaluator is not None and tr._evaluator.captures == 1
    tr.close()
    other = _loader(csvs, True)
    torch.manual_seed(5)
    for _ in other:
        pass
    assert torch.equal(after_eval, torch.get_rng_state())
    assert got == base["parent"] and again == base["parent"]


@pytest.mark.parametrize("kind", ["lappe", "ffn"])
def test_evaluator_lappe_and_ffn(kind, csvs):
    host = _loader(csvs, False)
    m = _model(host.dataset.num_items, D=64, K=8 if kind == "lappe" else 0, ffn=kind == "ffn", seed=13)
    want = _host_route_ranks(m, host)
    eager = DeviceEvaluator(m, _loader(csvs, True), use_graph=False).run()
    graph = DeviceEvaluator(m, _loader(csvs, True), use_graph=True).run()
    assert eager.tolist() == want.tolist()
    assert graph.tolist() == want.tolist()
    assert len(set(want.tolist())) > 5
