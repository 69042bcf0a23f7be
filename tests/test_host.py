"""Host-side logic of the product package (no GPU): batch layout / CSR packing,
capacity bucketing, id validation, synthetic workload shape, the CSV dataset and
collate, the flat parameter layout, API surface and error conventions."""

import os

import numpy as np
import pandas as pd
import pytest
import torch

import etpgt_ref as R
from etpgt.data.batch import Caps, SessionBatch, blob_layout, build_csr, collate_sessions
from etpgt.data.synthetic import batch_stats, make_batches, make_sessions_and_graph
from etpgt.model import SessionReadout, create_graph_transformer, create_graph_transformer_optimized


def _unpack(sb):
    caps, blob = sb.packed()
    lay = blob_layout(caps)
    return caps, {k: blob[v[0] : v[0] + v[1]] for k, v in lay.items() if k != "_total"}


def test_csr_roundtrip_random():
    rng = np.random.default_rng(0)
    n = 50
    src = rng.integers(0, n, 300)
    dst = rng.integers(0, n, 300)
    in_ptr, in_src, out_ptr, out_edge, out_dst, order = build_csr(src, dst, n)
    d_of = np.repeat(np.arange(n), np.diff(in_ptr))
    assert sorted(zip(in_src.tolist(), d_of.tolist())) == sorted(zip(src.tolist(), dst.tolist()))
    # stable: inside a destination row, original edge order is kept
    for t in range(n):
        seg = order[in_ptr[t] : in_ptr[t + 1]]
        assert np.all(np.diff(seg) > 0)
    for s in range(n):
        for i in range(out_ptr[s], out_ptr[s + 1]):
            assert in_src[out_edge[i]] == s and d_of[out_edge[i]] == out_dst[i]


def test_pack_batch_layout_and_padding():
    items = [{"x": [3, 7], "edge_index": [[0, 0, 1], [0, 1, 1]], "target_item": 9, "negative_items": [1, 2]},
             {"x": [4, 5, 6], "edge_index": [[0, 1], [2, 2]], "target_item": 8, "negative_items": [3, 10]}]
    sb = collate_sessions(items)
    caps, f = _unpack(sb)
    assert caps.n_cap >= 5 and caps.e_cap >= 5 and caps.n_neg == 2
    assert list(f["hdr"][:4]) == [5, 2, 5, 2]
    assert list(f["node_item"][:5]) == [3, 7, 4, 5, 6]
    assert list(f["node_ptr"][:3]) == [0, 2, 5]
    assert all(v == 5 for v in f["node_ptr"][3:])          # padded with N
    assert list(f["target"][:2]) == [9, 8]
    assert list(f["negatives"][:4]) == [1, 2, 3, 10]
    assert f["in_ptr"][5] == 5 and all(v == 5 for v in f["in_ptr"][6:])


def test_pack_rejects_cross_session_edges_and_bad_ids():
    sb = SessionBatch(torch.tensor([1, 2, 3]), torch.tensor([[0], [2]]), torch.tensor([0, 0, 1]),
                      torch.tensor([5, 6]), torch.tensor([7, 8]))
    with pytest.raises(ValueError, match="inside one session"):
        sb.packed()
    sb2 = SessionBatch(torch.tensor([1, 2, 300]), torch.zeros(2, 0, dtype=torch.long), torch.tensor([0, 0, 1]),
                       torch.tensor([5, 6]), torch.tensor([7, 8]))
    with pytest.raises(IndexError):
        sb2.check_ids(100)
    sb3 = SessionBatch(torch.tensor([1, 2, 3]), torch.zeros(2, 0, dtype=torch.long), torch.tensor([1, 0, 1]))
    with pytest.raises(ValueError, match="sorted"):
        sb3.packed()


def test_caps_bucketing_is_monotone_and_coarse():
    vals = [Caps.bucket(x, 32, x, 5).n_cap for x in range(1, 2000)]
    assert all(v >= x for v, x in zip(vals, range(1, 2000)))
    assert len(set(vals)) < 40
    c = Caps(100, 32, 300, 5)
    assert c.fits(100, 32, 300, 5) and not c.fits(101, 32, 300, 5) and not c.fits(10, 32, 10, 6)


def test_synthetic_workload_shape():
    d = make_sessions_and_graph(num_items=2000, num_sessions=4000, num_edges=20000, seed=1)
    assert d.edge_keys.size == 20000
    T = d.table_rows
    a, b = d.edge_keys // T, d.edge_keys % T
    assert np.all(a <= b) and a.min() >= 1
    bl = make_batches(d, 32, 4, 5)
    st = batch_stats(bl)
    assert 2.5 < st["nodes_per_session"] < 6 and st["edges_per_session"] > 3
    for sb in bl:
        ei = sb.edge_index.numpy()
        x = sb.x.numpy()
        # edges directed smaller -> larger item id (plus self loops), dataloader.py:45-48,149-152
        assert np.all(x[ei[0]] <= x[ei[1]])
        negs = sb.negative_items.view(32, 5).numpy()
        assert negs.min() >= 1


def test_session_dataset_and_collate(tmp_path):
    sessions = pd.DataFrame({
        "timestamp": [1, 2, 3, 4, 10, 11, 12],
        "visitorid": ["a"] * 4 + ["b"] * 3,
        "event": ["view"] * 7,
        "itemid": [5, 3, 5, 9, 2, 4, 6],
        "transactionid": [None] * 7,
        "session_id": [0, 0, 0, 0, 1, 1, 1],
    })
    edges = pd.DataFrame({"item_i": [3, 3, 5, 2, 4, 1], "item_j": [5, 3, 9, 4, 6, 2], "count": [1] * 6})
    sp, gp = tmp_path / "s.csv", tmp_path / "g.csv"
    sessions.to_csv(sp, index=False)
    edges.to_csv(gp, index=False)
    from etpgt.train.dataloader import SessionDataset, collate_fn, create_dataloader

    torch.manual_seed(0)
    ds = SessionDataset(sp, gp, num_negatives=3)
    assert ds.num_items == 10 and len(ds) == 2
    it = ds[0]
    assert it["target_item"].item() == 9
    assert sorted(it["session_items"].tolist()) == [3, 5, 5]
    # induced edges among context {3, 5}: (3,5), (3,3); (5,9) excluded (9 is the target)
    assert sorted(map(tuple, it["edge_index"].t().tolist())) == [(3, 3), (3, 5)]
    assert not set(it["negative_items"].tolist()) & {3, 5, 9}
    b = collate_fn([ds[0], ds[1]])
    assert b.x.tolist() == [3, 5, 2, 4]
    assert sorted(map(tuple, b.edge_index.t().tolist())) == [(0, 0), (0, 1), (2, 3)]
    assert b.batch.tolist() == [0, 0, 1, 1] and b.num_graphs == 2
    dl = create_dataloader(sp, gp, batch_size=2, num_negatives=3, shuffle=False)
    assert next(iter(dl)).num_graphs == 2


def test_product_model_structure_matches_reference():
    m = create_graph_transformer_optimized(36, embedding_dim=64, hidden_dim=64, laplacian_k=8)
    assert sum(p.numel() for p in m.parameters()) == 36800
    ref = R.ref_create_graph_transformer_optimized(36, embedding_dim=64, hidden_dim=64, laplacian_k=8)
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys())
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert m.use_ffn is False and m.num_layers == 2 and m.num_heads == 2
    m2 = create_graph_transformer(188, embedding_dim=64, hidden_dim=64, num_layers=2, num_heads=2,
                                  use_laplacian_pe=False, use_ffn=True, ffn_expansion=4)
    assert sum(p.numel() for p in m2.parameters()) == 112128
    W = m.item_embedding.weight.detach()
    assert float(W[0].abs().max()) == 0.0


def test_flat_layout_covers_every_dense_param():
    from etpgt.backend.engine import FlatParams

    m = create_graph_transformer_optimized(50, embedding_dim=32, hidden_dim=32, num_heads=2, laplacian_k=4)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    fp = FlatParams(m, torch.device("cpu"))
    after = dict(m.named_parameters())
    for n, p in after.items():
        assert torch.equal(p.detach(), before[n]), n
        if n != "item_embedding.weight":
            assert p.data_ptr() >= fp.flat.data_ptr() and p.data_ptr() < fp.flat.data_ptr() + 4 * fp.flat.numel()
    lay = fp.layout
    assert all(s.begin % 256 == 0 for s in lay.segs.values())
    # w_all rows: query | key | value | skip
    w = fp.flat[lay.seg("0.w_all").begin : lay.seg("0.w_all").begin + 4 * 32 * 32].view(128, 32)
    assert torch.equal(w[:32], m.convs[0].lin_query.weight.detach())
    assert torch.equal(w[96:], m.convs[0].lin_skip.weight.detach())


def test_cpu_model_fails_loudly():
    m = create_graph_transformer_optimized(50, embedding_dim=32, hidden_dim=32, use_laplacian_pe=False)
    sb = collate_sessions([{"x": [1, 2], "edge_index": [[0], [1]], "target_item": 3, "negative_items": [4]}])
    with pytest.raises(RuntimeError, match="HIP path only"):
        m(sb)
    from etpgt.backend.ops import score_loss

    with pytest.raises(RuntimeError, match="HIP path only"):
        score_loss(torch.randn(2, 32), torch.tensor([1, 2]), torch.tensor([[3], [4]]), m.item_embedding)


def test_unsupported_variants_are_rejected():
    m = create_graph_transformer_optimized(50, embedding_dim=32, hidden_dim=32, use_laplacian_pe=False,
                                           readout_type="max")
    with pytest.raises(NotImplementedError):
        m._check_supported()
    m2 = create_graph_transformer(50, embedding_dim=32, hidden_dim=32, use_laplacian_pe=False)
    with pytest.raises(NotImplementedError):
        m2._check_supported()


def test_loss_factory_and_errors():
    from etpgt.train.losses import BPRLoss, DualLoss, ListwiseLoss, SampledSoftmaxLoss, create_loss_function

    assert isinstance(create_loss_function("bpr"), BPRLoss)
    assert isinstance(create_loss_function("listwise", temperature=0.5), ListwiseLoss)
    assert isinstance(create_loss_function("dual", alpha=0.3), DualLoss)
    assert isinstance(create_loss_function("sampled_softmax"), SampledSoftmaxLoss)
    with pytest.raises(ValueError, match="Unknown loss type"):
        create_loss_function("nope")
    # reference Trainer dispatch inspects forward's co_varnames (trainer.py:96)
    assert len(DualLoss().forward.__code__.co_varnames) > 4


@pytest.mark.parametrize("mode", ["mean", "max", "last", "attention"])
def test_standalone_readout_matches_golden(golden_dir, mode):
    g = np.load(os.path.join(golden_dir, "readout.npz"))
    ro = SessionReadout(hidden_dim=8, readout_type=mode)
    if mode == "attention":
        with torch.no_grad():
            ro.attention.weight.copy_(torch.from_numpy(g["attention_w"]))
            ro.attention.bias.copy_(torch.from_numpy(g["attention_b"]))
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    se = ro(x, torch.from_numpy(g["batch"]))
    w = torch.linspace(-1, 1, se.numel()).view_as(se)
    (se * w).sum().backward()
    np.testing.assert_allclose(se.detach().numpy(), g[f"{mode}_se"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(x.grad.numpy(), g[f"{mode}_dx"], rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match="Unknown readout type"):
        SessionReadout(8, "bogus")


def test_lappe_precompute_matches_oracle_and_errors():
    from etpgt.encodings import LaplacianPECached, compute_laplacian_pe

    ei = torch.tensor([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]])
    pe = compute_laplacian_pe(ei, num_nodes=4, k=2)
    assert pe.shape == (4, 2) and pe.dtype == torch.float32 and bool((pe >= 0).all())
    np.testing.assert_allclose(np.sort(np.abs(pe.numpy()), axis=None),
                               np.sort(np.abs(R.ref_compute_laplacian_pe(ei, 4, 2).numpy()), axis=None), atol=1e-5)
    mod = LaplacianPECached(k=2, embedding_dim=16)
    with pytest.raises(RuntimeError, match="not precomputed"):
        mod(torch.tensor([0, 1]))

    class D:
        edge_index = ei
        num_nodes = 4

    mod.precompute(D())
    assert mod(torch.tensor([0, 2, 3])).shape == (3, 16)
    assert mod.project(torch.randn(4, 2)).shape == (4, 16)


def test_metrics_and_seed():
    from etpgt.utils import compute_ndcg_at_k, compute_recall_at_k, set_seed

    set_seed(42)
    a = torch.rand(10)
    set_seed(42)
    assert torch.equal(a, torch.rand(10))
    p = torch.tensor([[1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [11, 12, 13, 14, 15]])
    assert compute_recall_at_k(p, torch.tensor([2, 9, 20]), 5) == pytest.approx(2 / 3)
    assert compute_ndcg_at_k(p, torch.tensor([1, 9, 20]), 5) == pytest.approx(0.4769, abs=1e-4)


def test_c1_data_chain_matches_reference_scripts(golden_dir):
    """etpgt.pipeline reproduces the reference's own scripts/data/00 -> 02 -> 04 output
    (tests/golden/c1_data.npz, oracle/gen_golden.py gen_c1) exactly: events, sessions
    and the co-event graph, integer for integer and in the same row order."""
    from dropin_helpers import c1_inputs

    gd = np.load(os.path.join(golden_dir, "c1_data.npz"))
    ev, sd, g, _ = c1_inputs()
    code = {"view": 0, "addtocart": 1, "transaction": 2}
    assert np.array_equal(ev["timestamp"].to_numpy(np.int64), gd["ev_timestamp"])
    assert np.array_equal(ev["visitorid"].str.replace("visitor_", "").astype(np.int64).to_numpy(), gd["ev_visitor"])
    assert np.array_equal(ev["event"].map(code).to_numpy(np.int64), gd["ev_event"])
    assert np.array_equal(ev["itemid"].to_numpy(np.int64), gd["ev_itemid"])
    assert np.array_equal(ev["transactionid"].notna().to_numpy(), gd["ev_txn"])
    assert np.array_equal(sd["timestamp"].to_numpy(np.int64), gd["sd_timestamp"])
    assert np.array_equal(sd["itemid"].to_numpy(np.int64), gd["sd_itemid"])
    assert np.array_equal(sd["session_id"].str.replace("sess_", "").astype(np.int64).to_numpy(), gd["sd_session"])
    assert np.array_equal(sd.index.to_numpy(np.int64), gd["sd_index"])
    for k in ("item_i", "item_j", "count", "last_ts"):
        assert np.array_equal(g[k].to_numpy(np.int64), gd[f"g_{k}"]), k


def test_c1_pipeline_batch_semantics():
    """run_full_pipeline.py:85-179 batch construction on C1's pinned data: sorted unique
    context items as nodes, induced co-event edges in both directions (self loops if
    none), the first n catalogue items outside the session as negatives, remapped ids."""
    from dropin_helpers import c1_inputs

    from etpgt.pipeline import create_batch_from_sessions

    _, _, _, (sub, gsub) = c1_inputs()
    assert sub["session_id"].nunique() == 100
    lens = sub.groupby("session_id").size()
    assert lens.min() >= 3 and lens.max() <= 20
    assert bool((gsub["item_i"] <= gsub["item_j"]).all()) and bool((gsub["count"] >= 1).all())
    batch, T = create_batch_from_sessions(sub, gsub, batch_size=16, num_negatives=5)
    assert T == sub["itemid"].nunique()
    assert batch.num_graphs == 16 and tuple(batch.negative_items.shape) == (16, 5)
    ptr = batch.ptr.numpy()
    ei = batch.edge_index.numpy()
    items = sorted(sub["itemid"].unique())
    idx = {it: k for k, it in enumerate(items)}
    for b, sid in enumerate(sub["session_id"].unique()[:16]):
        sd = sub[sub["session_id"] == sid].sort_values("timestamp")["itemid"].to_numpy()
        x = batch.x.numpy()[ptr[b]:ptr[b + 1]]
        assert x.tolist() == sorted({idx[i] for i in sd[:-1]})
        assert int(batch.target_item[b]) == idx[sd[-1]]
        seen = {idx[i] for i in sd}
        assert batch.negative_items[b].tolist() == [i for i in range(T) if i not in seen][:5]
        m = (ei[0] >= ptr[b]) & (ei[0] < ptr[b + 1])
        e = ei[:, m] - ptr[b]
        pairs = set(zip(e[0].tolist(), e[1].tolist()))
        assert all((d, s) in pairs for s, d in pairs)  # both directions
        assert e.shape[1] > 0


def test_reference_train_script_imports_resolve():
    """Everything the reference scripts/train/train_baseline.py:13-22 (and etpgt.utils,
    utils/__init__.py:3) imports exists in the package; out-of-scope baselines raise."""
    import importlib

    from dropin_helpers import REFERENCE_IMPORTS

    for mod, names in REFERENCE_IMPORTS.items():
        m = importlib.import_module(mod)
        missing = [n for n in names if not hasattr(m, n)]
        assert not missing, (mod, missing)
    from etpgt.model import create_gat, create_graphsage

    with pytest.raises(NotImplementedError, match="outside"):
        create_gat(num_items=10)
    with pytest.raises(NotImplementedError, match="outside"):
        create_graphsage(num_items=10)


def test_utils_logging_and_io(tmp_path):
    import logging

    from etpgt.utils import get_logger, load_config, load_json, save_json

    lg = get_logger("etpgt.test.x", log_file=str(tmp_path / "l.txt"))
    n = len(lg.handlers)
    assert get_logger("etpgt.test.x") is lg and len(lg.handlers) == n == 2
    lg.info("hello")
    assert lg.level == logging.INFO
    save_json({"a": 1, "b": [1, 2]}, str(tmp_path / "sub" / "x.json"))
    assert load_json(str(tmp_path / "sub" / "x.json")) == {"a": 1, "b": [1, 2]}
    (tmp_path / "c.yaml").write_text("lr: 0.001\nlayers: [1, 2]\n")
    assert load_config(str(tmp_path / "c.yaml")) == {"lr": 0.001, "layers": [1, 2]}


def test_pyg_data_duck_type():
    from etpgt.data import Data

    d = Data(edge_index=torch.tensor([[0, 1], [1, 4]]), num_nodes=9)
    assert d.num_nodes == 9
    assert Data(edge_index=torch.tensor([[0, 1], [1, 4]])).num_nodes == 5
    assert Data(x=torch.zeros(3, 2), foo=1).foo == 1


def test_train_baseline_counterpart_cli_plumbing(tmp_path):
    """The counterpart script parses the reference's flags, refuses GCS, reads the data,
    builds the model and precomputes LapPE; on a CPU device the HIP model then fails
    loudly (no CPU fallback)."""
    import importlib.util

    from dropin_helpers import write_csvs

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_baseline_cp", os.path.join(root, "scripts", "train",
                                                                                      "train_baseline.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)
    d = write_csvs(tmp_path)
    base = ["--model", "graph_transformer_optimized", "--train-sessions", str(d / "train.csv"),
            "--val-sessions", str(d / "val.csv"), "--graph-edges", str(d / "graph_edges.csv"),
            "--embedding-dim", "32", "--hidden-dim", "32", "--num-layers", "2", "--num-heads", "2",
            "--max-epochs", "1", "--num-workers", "0", "--output-dir", str(tmp_path / "out")]
    a = tb.parse_args(base)
    assert a.batch_size == 32 and a.lr == 0.001 and a.weight_decay == 1e-5 and a.seed == 42 and a.patience == 10
    with pytest.raises(NotImplementedError, match="GCS"):
        tb.main(base + ["--gcs-bucket", "b"])
    with pytest.raises(NotImplementedError, match="outside"):
        tb.main(base[:1] + ["gat"] + base[2:] + ["--device", "cpu"])
    with pytest.raises(RuntimeError, match="HIP path only"):
        tb.main(base + ["--device", "cpu"])


def test_reference_directed_lappe_input_has_no_eigen_answer():
    """The reference training script's LapPE input (train_baseline.py:236-242: the graph
    CSV's item_i -> item_j with item_i <= item_j, num_nodes = num_items) gives a unit
    upper-triangular Laplacian: its spectrum is exactly {1}, and eigsh(k+1, 'SM') -- the
    reference's compute_laplacian_pe -- returns Ritz pairs that are not eigenpairs.  This
    pins why the GPU solver refuses that input or symmetrizes it
    (etpgt/encodings/laplacian_gpu.py)."""
    import numpy as np
    import scipy.sparse as sp
    from scipy.sparse.linalg import eigsh

    import oracle.etpgt_ref as R

    rng = np.random.default_rng(7)
    n, m = 1500, 9000
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    ei = np.stack([np.minimum(i, j), np.maximum(i, j)])
    L = R.ref_sym_laplacian(ei, n)
    assert sp.tril(L, -1).count_nonzero() == 0 and np.allclose(L.diagonal(), 1.0)  # unit upper triangular
    w, v = eigsh(L.astype(np.float64), k=17, which="SM")
    res = np.linalg.norm(L @ v - v * w, axis=0)
    assert np.abs(w - 1.0).max() > 0.1  # the "eigenvalues" are not the spectrum {1}
    assert res.min() > 0.05             # and the vectors are not eigenvectors


def test_device_loader_epoch_order_matches_torch_dataloader():
    """DeviceSessionLoader visits each epoch's sessions in the order a
    ``DataLoader(shuffle=True)`` over the same dataset does under the same global seed --
    the iterator's ``_base_seed`` draw precedes the RandomSampler's seed draw -- including
    a non-shuffled validation loader iterated between training epochs (its iterator draws
    a ``_base_seed`` too)."""
    from torch.utils.data import DataLoader

    from etpgt.train.dataloader import DeviceSessionLoader

    ds = list(range(37))

    def dev_loader(shuffle):
        dl = DeviceSessionLoader.__new__(DeviceSessionLoader)  # order logic only (no GPU store)
        dl.dataset, dl.shuffle, dl.num_sessions = ds, shuffle, len(ds)
        return dl

    torch.manual_seed(42)
    ref = []
    for _ in range(3):
        for shuffle in (True, False):
            loader = DataLoader(ds, batch_size=5, shuffle=shuffle, collate_fn=lambda b: b)
            ref.append([int(v) for b in loader for v in b])
    torch.manual_seed(42)
    tr, va = dev_loader(True), dev_loader(False)
    got = []
    for _ in range(3):
        got.append(tr._epoch_order().tolist())
        got.append(va._epoch_order().tolist())
    assert got == ref
    assert got[0] != got[2]  # fresh permutation per epoch


def test_plan_caps_covers_a_ranks_partial_batch_off_the_stride_grid():
    """a data-parallel rank r >= 1 builds its last, partial batch at
    i*P*B + r*b (b < B), off the stride grid [pos + i*P*B, +B) the full batches follow.
    ``plan_caps(..., extra=[(position, b)])`` must cover that window too; here rank 1's
    partial batch holds the longest sessions, which the grid windows never see."""
    import types

    from etpgt.data.gpu_batch import GpuBatchBuilder

    S, B, P = 37, 8, 2  # 2 full global batches (32 sessions) + 5 left: last batch b = 2 per rank
    nodes = np.full(S, 3, np.int64)
    edges = np.full(S, 4, np.int64)
    b_last = (S % (B * P)) // P
    pos1 = 2 * B * P + 1 * b_last          # rank 1's partial batch
    nodes[pos1: pos1 + b_last] = 50        # the longest sessions of the epoch
    edges[pos1: pos1 + b_last] = 400
    bld = GpuBatchBuilder.__new__(GpuBatchBuilder)
    bld.store = types.SimpleNamespace(nodes=nodes, edges=edges)
    bld.B, bld.stride, bld.n_neg = B, B * P, 5
    bld.order_h = np.arange(S, dtype=np.int64)
    grid_only = bld.plan_caps(2, position=1 * B)  # rank 1's full batches
    assert grid_only.n_cap < 100  # the grid windows miss the long sessions
    caps = bld.plan_caps(2, position=1 * B, extra=[(pos1, b_last)])
    assert caps.n_cap >= 100 and caps.e_cap >= 800 and caps.b_cap >= B


def test_bench_step_graph_plan_covers_exactly_k_steps():
    """bench.py's multi-step graph chunking (FusedTrainStep.capture_steps): the K timed
    steps are exactly full * S + rem; above 256 steps every chunk is a multiple of the
    resident image count, so each chunk and the remainder start on the same image."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(__file__), "..", "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for steps in (1, 5, 20, 200, 256, 257, 1000, 4097):
        for nimg in (4, 7, 64):
            S, full, rem = bench.step_graph_plan(steps, nimg)
            assert full * S + rem == steps and 0 <= rem < S or (full == 1 and rem == 0 and S == steps)
            if steps > 256:
                assert S % nimg == 0 and S <= max(256, nimg)
            else:
                assert (S, full, rem) == (steps, 1, 0)


def test_bench_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the loss and every floating-point state_dict tensor as
    float32 .npy (integer buffers are left out); within the budget whole, above it each
    tensor of 1 MB or more as the same sorted row sample on every call."""
    import importlib.util

    import numpy as np

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(__file__), "..", "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Embedding(5000, 64), torch.nn.BatchNorm1d(64))  # table: 1.28 MB
    loss = torch.tensor(0.25)
    bench.dump_outputs(str(tmp_path / "whole"), loss, model)
    names = sorted(os.listdir(tmp_path / "whole"))
    assert names == ["0.weight.npy", "1.bias.npy", "1.running_mean.npy", "1.running_var.npy", "1.weight.npy", "loss.npy"]
    tab = np.load(tmp_path / "whole" / "0.weight.npy")
    assert tab.dtype == np.float32 and np.array_equal(tab, model[0].weight.detach().numpy())
    assert np.load(tmp_path / "whole" / "loss.npy").tolist() == [0.25]
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 19)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), loss, model)
    s1, s2 = np.load(tmp_path / "s1" / "0.weight.npy"), np.load(tmp_path / "s2" / "0.weight.npy")
    assert np.array_equal(s1, s2) and s1.shape[1] == 64 and 1000 < s1.shape[0] < 5000
    rows = np.sort(np.random.default_rng(0).choice(5000, size=s1.shape[0], replace=False))
    assert np.array_equal(s1, tab[rows])
    assert sum(os.path.getsize(tmp_path / "s1" / n) for n in os.listdir(tmp_path / "s1")) <= 1 << 20
    assert np.array_equal(np.load(tmp_path / "s1" / "1.running_var.npy"), np.load(tmp_path / "whole" / "1.running_var.npy"))
