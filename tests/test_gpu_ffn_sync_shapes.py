"""GPU: SyncBN for the FFN model shapes that run on the LDS-staged GEMMs (gtr_gemm_gen.hip)
-- hidden width 256 and feed-forward expansions 1 / 2 -- where one workgroup
(k_gen_bn_sync) folds the ranks' gathered (count, mean, M2) rows ahead of the rows that
read the statistics.  One shape is missing: d 64 at expansion 2, which FusedTrainStep still
refuses under SyncBN (tests/test_ffn_host.py pins that refusal); the row-sharded case and
the small alias case run at d 64 x 1 instead.

* ranks sharing the GPU over gloo against the oracle trio on the concatenated global batch
  (the protocol of test_gpu_ffn_dp.test_ffn_sync_bn_two_ranks_equal_oracle_on_the_global_batch),
  at two and four ranks, replicated and row-sharded table;
* one rank: the consumers reading the producers' rows in place against gathered copies
  (GTR_SYNC_NOALIAS=1), bit for bit;
* two ranks of the drop-in train_baseline.py with the optimized model at the script's default
  shapes (d 256, 3 layers, 4 heads) against the oracle replay on the global batches.  (The
  script's FFN model at d 256 is not here: the Trainer's default leaves it on per-rank
  statistics, tests/test_distributed.py pins that default.)"""

from __future__ import annotations

import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only on the GPU box
    pytest.skip("no GPU", allow_module_level=True)

from gpu_helpers import OracleTrio, batches, close_trained, collect, ref_batch, small_data  # noqa: E402
import etpgt_ref as R  # noqa: E402

from etpgt.train.fused import FusedTrainStep  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, B, NNEG = 3, 16, 5


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _pair(T, D, H, E, L, K, seed):
    from test_gpu_ffn import make_ffn_pair

    return make_ffn_pair(T, D, H, L=L, K=K, seed=seed, expansion=E)


def _concat(bs):
    from test_gpu_distributed import _concat as cat

    out = bs[0]
    for b in bs[1:]:
        out = cat(out, b)
    return out


def _worker(rank, world, port, q, D, H, E, L, K, shard):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GTR_GEMM="f32")
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    f = None
    try:
        data = small_data()
        m, _ = _pair(data.table_rows, D, H, E, L, K, 41)
        m.train()
        f = FusedTrainStep(m, lr=1e-2, weight_decay=1e-2, loss="listwise", sync_bn=True, shard_table=shard)
        assert f.data_parallel and f.world == world and f.sync_bn
        bl = batches(data, B, NNEG, STEPS * world, seed=42)
        losses = [float(f(bl[s * world + rank].to("cuda"))) for s in range(STEPS)]
        assert f.split and not f.sync_alias  # the FFN blocks run on the split layer path
        assert (f.shard_state is not None) == shard
        f.sync_table()  # row-sharded: the shards back into the model's table (collective)
        bufs = {n: b.detach().cpu().numpy().copy() for n, b in m.named_buffers()
                if "running" in n or "num_batches_tracked" in n}
        q.put((rank, losses, {n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters()}, bufs))
    finally:
        if f is not None:
            f.close()
        dist.destroy_process_group()


@pytest.mark.parametrize("D,H,E,L,K,world,shard", [
    (256, 4, 4, 3, 16, 2, False),  # the reference defaults: D = 256 fold, the D = 256 attention bodies under SyncBN
    (256, 4, 2, 2, 0, 2, False),
    (128, 4, 1, 2, 0, 2, False),
    (64, 2, 1, 2, 0, 2, True),     # the row-sharded pieces with the generic FFN
    (64, 2, 1, 2, 0, 4, False),    # four merged rows
], ids=["d256x4_L3_pe16", "d256x2", "d128x1", "d64x1_row_sharded", "d64x1_four_ranks"])
def test_sync_bn_generic_ffn_shapes_equal_oracle_on_the_global_batch(D, H, E, L, K, world, shard):
    """The ranks train the FFN model like one GPU on the concatenated global batch
    (BatchNorm over all world x B sessions; the ranks' node counts differ, so the fold is
    count-weighted): per-step mean loss at 1e-3, every trained parameter and the running
    statistics elementwise (OracleTrio.compare / close_trained), each BatchNorm updated
    once per step, replicas bit-identical."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, D, H, E, L, K, shard)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for rank, losses, params, bufs in collect(q, procs, world):
            res[rank] = (losses, params, bufs)
    finally:
        for p in procs:
            p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    for r in range(1, world):
        for k, v in res[0][1].items():
            assert np.array_equal(v, res[r][1][k]), f"replicas diverged: rank {r} {k}"
        for k, v in res[0][2].items():
            assert np.array_equal(v, res[r][2][k]), f"replicas diverged: rank {r} {k}"
    data = small_data()
    _, ref = _pair(data.table_rows, D, H, E, L, K, 41)
    ref.train()
    trio = OracleTrio(ref, lambda ps: torch.optim.AdamW(ps, lr=1e-2, weight_decay=1e-2))
    bl = batches(data, B, NNEG, STEPS * world, seed=42)
    assert len({bl[r].num_nodes for r in range(world)}) > 1  # unequal counts: a weighted merge
    for s in range(STEPS):
        rb = ref_batch(_concat([bl[s * world + r] for r in range(world)]))
        lo = float(trio.step(lambda mod, o: R.ref_train_step(mod, rb, o, "listwise")))
        avg = sum(res[r][0][s] for r in range(world)) / world
        print(f"step {s}: mean rank loss {avg:.7g} oracle {lo:.7g}")
        assert abs(avg - lo) <= 1e-3 * abs(lo), (s, avg, lo)
    trio.compare({n: torch.from_numpy(v) for n, v in res[0][1].items()}, lr=1e-2)
    b64 = dict(trio.ref64.named_buffers())
    b1 = dict(trio.ref1.named_buffers())
    nbt = 0
    for n, b in trio.ref.named_buffers():
        if "running" in n:
            close_trained(torch.from_numpy(res[0][2][n]), b, b64[n], torch.zeros_like(b, dtype=torch.bool), 0.0, n,
                          b1[n])
        elif "num_batches_tracked" in n:
            assert int(res[0][2][n]) == STEPS == int(b), n
            nbt += 1
    assert nbt == L


def _one_rank_run(D, H, E, L):
    data = small_data()
    m, _ = _pair(data.table_rows, D, H, E, L, 0, 43)
    m.train()
    f = FusedTrainStep(m, lr=1e-2, weight_decay=1e-2, loss="listwise", data_parallel=True, sync_bn=True)
    try:
        bl = batches(data, B, NNEG, STEPS, seed=44)
        losses = torch.stack([f(sb.to("cuda")).detach().reshape(()).clone() for sb in bl]).cpu()
        alias = f.sync_alias
        assert f.split and f.world == 1
        f.flush()
        state = {n: t.detach().cpu().clone() for n, t in m.state_dict().items()}
    finally:
        f.close()
    return alias, losses, state


@pytest.mark.parametrize("D,H,E,L", [(256, 4, 4, 2), (64, 2, 1, 2)], ids=["d256x4", "d64x1"])
def test_sync_bn_one_rank_alias_equals_gathered_copies(monkeypatch, D, H, E, L):
    """World 1: the statistics kernel and the attention backward reading the producers'
    rows in place (the default) against reading gathered copies (GTR_SYNC_NOALIAS=1), from
    the same initial state over the same three batches: losses, every parameter, the table
    and the running statistics bit for bit."""
    monkeypatch.delenv("GTR_SYNC_NOALIAS", raising=False)
    monkeypatch.setenv("GTR_GEMM", "f32")
    a_alias, a_losses, a_state = _one_rank_run(D, H, E, L)
    monkeypatch.setenv("GTR_SYNC_NOALIAS", "1")
    b_alias, b_losses, b_state = _one_rank_run(D, H, E, L)
    assert a_alias and not b_alias
    assert torch.equal(a_losses, b_losses), (a_losses, b_losses)
    assert set(a_state) == set(b_state)
    for n, t in a_state.items():
        assert torch.equal(t, b_state[n]), n
    for l in range(L):
        assert int(a_state[f"batch_norms.{l}.num_batches_tracked"]) == STEPS


def _script():
    import importlib.util

    spec = importlib.util.spec_from_file_location("train_baseline_cp",
                                                  os.path.join(ROOT, "scripts", "train", "train_baseline.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)
    return tb


def _rank_main(rank, world, port, d, out, q, model):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank), GTR_SHARE_DEVICE="1")
    # the model shape flags stay at the script's defaults (d 256, 3 layers, 4 heads)
    args = ["--model", model, "--train-sessions", str(d / "train.csv"), "--val-sessions", str(d / "val.csv"),
            "--graph-edges", str(d / "graph_edges.csv"), "--dropout", "0", "--batch-size", "8",
            "--num-negatives", "5", "--max-epochs", "1", "--num-workers", "0", "--output-dir", str(out)]
    tr = _script().main(args)  # releases the captured graphs and destroys the process group itself
    import torch.distributed as dist

    assert not dist.is_initialized()
    assert tr.sync_bn and tr._fused is not None and tr._fused.sync_bn
    sd = {k: v.detach().cpu().numpy() for k, v in tr.model.state_dict().items()}
    q.put((rank, tr.history, sd))


@pytest.mark.parametrize("model", ["graph_transformer_optimized"])
def test_train_baseline_two_ranks_reference_default_shapes(tmp_path, model):
    """Two ranks of the drop-in train_baseline.py with the optimized model at the script's
    default shapes -- d 256, 3 layers, 4 heads, LapPE, a configuration no multi-rank test ran
    before -- one epoch of 40 sessions, B = 8 per rank, against the
    oracle replaying the epoch on the global batches of 16 (the replay of
    test_gpu_multigpu.test_train_baseline_two_ranks_match_oracle_on_the_global_batch):
    SyncBN on in the Trainer and its fused step, replicas identical, the epoch loss at 1e-3,
    every parameter and the running statistics elementwise; the ranks leave through
    ``destroy_process_group`` (exit code 0)."""
    import batch_ref as BR
    from dropin_helpers import write_csvs

    from etpgt.data.batch import collate_sessions
    from etpgt.model import create_graph_transformer, create_graph_transformer_optimized
    from etpgt.train.dataloader import SessionDataset
    from etpgt.utils.seed import set_seed

    d = write_csvs(tmp_path, num_train=40)  # 2 global batches of 16 + a last one of 8
    world, Bq, n, D, H, L = 2, 8, 5, 256, 4, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, d, tmp_path / "dp", q, model)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for rank, hist, sd in collect(q, procs, world):
            res[rank] = (hist, sd)
    finally:
        for p in procs:
            p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    for k, v in res[0][1].items():
        assert np.array_equal(v, res[1][1][k]), f"replicas diverged: {k}"
    hist, sd = res[0]
    assert sd["item_embedding.weight"].shape[1] == D and f"convs.{L - 1}.lin_query.weight" in sd
    ffn = model == "graph_transformer"
    assert ("ffns.2.0.weight" in sd) == ffn
    # ---- the oracle replays the epoch on the global batches
    tr = SessionDataset(d / "train.csv", d / "graph_edges.csv", n, 50)
    va = SessionDataset(d / "val.csv", d / "graph_edges.csv", n, 50)
    T = max(tr.num_items, va.num_items)
    set_seed(42)
    if ffn:
        init = create_graph_transformer(T, embedding_dim=D, hidden_dim=D, num_layers=L, num_heads=H, dropout=0.0,
                                        readout_type="mean", use_laplacian_pe=True)
    else:
        init = create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=L, num_heads=H,
                                                  dropout=0.0, use_laplacian_pe=True, use_ffn=False, ffn_expansion=2)
    torch.empty((), dtype=torch.int64).random_()  # the epoch iterator's _base_seed draw
    seed = int(torch.empty((), dtype=torch.int64).random_().item())  # the epoch's RandomSampler draw
    g = torch.Generator()
    g.manual_seed(seed)
    order = torch.randperm(len(tr), generator=g).numpy()
    if ffn:
        ref = R.RefGraphTransformer(T, embedding_dim=D, hidden_dim=D, num_layers=L, num_heads=H, dropout=0.0,
                                    use_laplacian_pe=True, use_ffn=True, ffn_expansion=4)
    else:
        ref = R.ref_create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=L, num_heads=H,
                                                       dropout=0.0, use_laplacian_pe=True)
    isd = {k: v.clone() for k, v in init.state_dict().items()}
    isd["laplacian_pe._cached_pe"] = torch.from_numpy(sd["laplacian_pe._cached_pe"]).clone()
    ref.laplacian_pe._cached_pe = isd["laplacian_pe._cached_pe"]
    ref.load_state_dict(isd)
    trio = OracleTrio(ref, lambda ps: torch.optim.AdamW(ps, lr=1e-3, weight_decay=1e-5))
    ei = tr.edge_index.numpy()
    keys = np.unique(ei[0].astype(np.int64) * tr.num_items + ei[1].astype(np.int64))
    S, GB = len(tr), world * Bq
    assert len(hist["train_loss"]) == 1
    losses = []
    for i in range(-(-S // GB)):
        b = min(GB, S - i * GB)
        ex = BR.build_batch(tr._ptr, tr._items, keys, tr.num_items, order, i * GB, b, 50, n, 42)
        rb = R.ref_batch_from(collate_sessions(ex))
        losses.append(float(trio.step(lambda mod, o: R.ref_train_step(mod, rb, o, "bpr"))))
    want = float(np.mean(losses))
    print(f"epoch loss {hist['train_loss'][0]:.7g} oracle {want:.7g}")
    assert abs(hist["train_loss"][0] - want) <= 1e-3 * abs(want), (hist["train_loss"][0], want)
    trio.compare({k: torch.from_numpy(sd[k]) for k, _ in ref.named_parameters()}, lr=1e-3)
    b64 = dict(trio.ref64.named_buffers())
    b1 = dict(trio.ref1.named_buffers())
    for k, b in ref.named_buffers():
        if "num_batches_tracked" in k:
            assert int(sd[k]) == int(b), k
        elif "running" in k:  # SyncBN: statistics over the global batch
            close_trained(torch.from_numpy(sd[k]), b, b64[k], torch.zeros_like(b, dtype=torch.bool), 0.0, k, b1[k])
