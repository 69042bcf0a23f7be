"""GPU: the last / attention session readouts (gtr_readout_pool, k_readout_pool) against
the CPU oracle (oracle/etpgt_ref.py RefSessionReadout; base.py:166-188).

Bars (gpu_helpers): session embeddings, loss and running statistics within 1e-3
(assert_close); every parameter gradient within 2e-3 relative with an absolute floor of
1e-6 of the largest gradient, as in test_gpu_parity.py; trained parameters elementwise
(OracleTrio / close_trained).  d loss / d readout.attention.bias is mathematically 0 (the
softmax is shift invariant): its gradient is held to the absolute floor alone, and in trio
runs it counts as a noise-floor element (2 lr per step), like lin_key.bias.
"""

from __future__ import annotations

import copy
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only on the GPU box
    pytest.skip("no GPU", allow_module_level=True)

import etpgt_ref as R  # noqa: E402
from gpu_helpers import (OracleTrio, assert_close, batches, edge_case_batch, long_session_batch,  # noqa: E402
                         ref_batch, small_data)

from etpgt.backend import _lib as L  # noqa: E402
from etpgt.model import create_graph_transformer, create_graph_transformer_optimized  # noqa: E402
from etpgt.train.fused import FusedTrainStep  # noqa: E402
from etpgt.train.losses import create_loss_function  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["last", "attention"]
CONFIGS = [(32, 2, 0), (64, 1, 0), (128, 4, 16), (256, 2, 0)]  # (D, H, K)
BIAS = "readout.attention.bias"

_DATA = None


def data():
    global _DATA
    if _DATA is None:
        _DATA = small_data()
    return _DATA


def _set_readout(m):
    """Non-trivial scoring vector (a softmax far from uniform) and a bias of 0.3."""
    if m.readout_type == "attention":
        with torch.no_grad():
            m.readout.attention.weight.mul_(3.0)
            m.readout.attention.bias.fill_(0.3)


def make_pair(T, D, H, kind, L_=2, K=0, dropout=0.0, seed=0):
    """gpu_helpers.make_pair with ``readout_type`` passed to both factories."""
    torch.manual_seed(seed)
    m = create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=L_, num_heads=H,
                                           dropout=dropout, readout_type=kind, use_laplacian_pe=K > 0,
                                           laplacian_k=max(K, 1))
    if K > 0:
        m.laplacian_pe._cached_pe = torch.rand(T, K)
    with torch.no_grad():
        for bn in m.batch_norms:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    _set_readout(m)
    ref = R.ref_create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=L_, num_heads=H,
                                                   dropout=dropout, readout_type=kind, use_laplacian_pe=K > 0,
                                                   laplacian_k=max(K, 1))
    if K > 0:
        ref.laplacian_pe._cached_pe = torch.zeros(T, K)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert set(sd) == set(ref.state_dict()), "state_dict keys differ from the reference layout"
    assert (BIAS in sd) == (kind == "attention")
    ref.load_state_dict(sd)
    return m.cuda(), ref


def _loss_pair(m, ref, sb, loss, n, se, se_ref):
    dsb = sb.to("cuda")
    B = sb.num_graphs
    neg = dsb.negative_items.view(B, n)
    if loss == "model_bpr":
        L_hip = m.compute_loss(se, dsb.target_item, neg)
    else:
        out = create_loss_function(loss, alpha=0.7, temperature=0.5)(se, dsb.target_item, neg, m.item_embedding)
        L_hip = out[0] if isinstance(out, tuple) else out
    rb = ref_batch(sb)
    kind = "bpr" if loss == "model_bpr" else loss
    L_ref = R.ref_loss(kind, se_ref, rb.target_item, rb.negative_items.view(B, n), ref.item_embedding, 0.7, 0.5)
    return L_hip, L_ref


def _grads_vs_oracle(m, ref, sb, loss="model_bpr", n=5, masks=None, stats=True):
    """Train mode: loss, se, every parameter gradient (dense table gradient and
    readout.attention.* included) and the running statistics."""
    m.train(); ref.train()
    se = m(sb.to("cuda"))
    ref.drop_masks = masks
    se_ref = ref(ref_batch(sb))
    ref.drop_masks = None
    L_hip, L_ref = _loss_pair(m, ref, sb, loss, n, se, se_ref)
    m.zero_grad()
    L_hip.backward()
    ref.zero_grad()
    L_ref.backward()
    assert_close(se, se_ref, name="se")
    assert_close(L_hip.reshape(1), L_ref.reshape(1), name="loss")
    hp = dict(m.named_parameters())
    gscale = max(float(p.grad.abs().max()) for p in ref.parameters())
    for name, p in ref.named_parameters():
        assert hp[name].grad is not None, name
        if name == BIAS:
            print(f"{BIAS}: hip {float(hp[name].grad):.3e} oracle {float(p.grad):.3e} floor {1e-6 * gscale:.3e}")
        assert_close(hp[name].grad, p.grad, rtol=2e-3, name=f"grad {name}", floor=1e-6 * gscale)
    if stats:
        hb = dict(m.named_buffers())
        for name, b in ref.named_buffers():
            if "running" in name:
                assert_close(hb[name], b, name=name)


# ---- 1. eval forward ---------------------------------------------------------------------
@pytest.mark.parametrize("D,H,K", CONFIGS)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_eval(kind, D, H, K):
    T = data().table_rows
    m, ref = make_pair(T, D, H, kind, K=K, seed=1)
    with torch.no_grad():
        for bn, rbn in zip(m.batch_norms, ref.batch_norms):
            bn.running_mean.uniform_(-0.1, 0.1)
            bn.running_var.uniform_(0.5, 2.0)
            rbn.running_mean.copy_(bn.running_mean.cpu())
            rbn.running_var.copy_(bn.running_var.cpu())
    m.eval(); ref.eval()
    for sb in batches(data(), 32, 5, 2, seed=D) + [edge_case_batch(5, T)]:
        with torch.no_grad():
            se = m(sb.to("cuda"))
            se_ref = ref(ref_batch(sb))
        assert_close(se, se_ref, name=f"se {kind} D={D} H={H}")


# ---- 2. train-mode gradients through autograd --------------------------------------------
@pytest.mark.parametrize("loss", ["model_bpr", "listwise", "dual"])
@pytest.mark.parametrize("D,H,K", CONFIGS)
@pytest.mark.parametrize("kind", KINDS)
def test_train_grads(kind, D, H, K, loss):
    T = data().table_rows
    n = 5 if loss != "listwise" else 20
    m, ref = make_pair(T, D, H, kind, K=K, seed=2)
    sb = batches(data(), 32, n, 1, seed=7 + D)[0]
    _grads_vs_oracle(m, ref, sb, loss, n)


# ---- 3. long sessions: several rounds per wave, the backward's recompute path -----------
@pytest.mark.parametrize("D,H", [(64, 2), (128, 4)])
@pytest.mark.parametrize("kind", KINDS)
def test_long_sessions(kind, D, H):
    T = data().table_rows
    m, ref = make_pair(T, D, H, kind, seed=4)
    _grads_vs_oracle(m, ref, long_session_batch(5, T), stats=False)


# ---- 4. more sessions than workgroups -----------------------------------------------------
def test_more_sessions_than_workgroups():
    """B = 300 > 256 readout workgroups: blocks stride to a second session (issue(b + grid))."""
    T = data().table_rows
    m, ref = make_pair(T, 64, 2, "attention", seed=5)
    sb = batches(data(), 300, 5, 1, seed=21)[0]
    assert sb.num_graphs == 300
    _grads_vs_oracle(m, ref, sb, stats=False)


# ---- 5. dropout 0.1, value for value -------------------------------------------------------
def test_dropout_values_with_hip_masks():
    T = data().table_rows
    D, H, p = 64, 2, 0.1
    m, ref = make_pair(T, D, H, "attention", dropout=p, seed=7)
    sb = batches(data(), 64, 5, 1, seed=19)[0]
    eng = m.hip_engine()
    masks = R.hip_dropout_masks(eng.seed, int(eng.rng_ctr.item()), p, 2, sb.edge_index.numpy(), int(sb.x.shape[0]),
                                D, H)
    _grads_vs_oracle(m, ref, sb, masks=masks)


# ---- 6. dispatch: the wave-per-session kernel stays mean-only -----------------------------
def test_wave_threshold_does_not_take_the_mean_kernel(monkeypatch):
    monkeypatch.setenv("GTR_RO_WAVE_MIN_B", "1")
    T = data().table_rows
    m, ref = make_pair(T, 64, 1, "attention", seed=8)
    sb = batches(data(), 32, 5, 1, seed=23)[0]
    _grads_vs_oracle(m, ref, sb)


# ---- 7. mean is untouched ------------------------------------------------------------------
def test_pool_entry_point_with_mean_is_gtr_readout_loss():
    """gtr_readout_pool with pool = NULL and with kind MEAN against gtr_readout_loss on the
    same workspace (FWD | LOSS | BWD, B 32, D 64): bit for bit."""
    T = data().table_rows
    m, _ = make_pair(T, 64, 1, "mean", seed=9)
    m.train()
    eng = m.hip_engine()
    sb = batches(data(), 32, 5, 1, seed=25)[0]
    caps, blob, node_pe = eng.prepare(sb.to("cuda"))
    ws = eng.workspace(caps, fresh=True)
    cfg = eng.config(ws, True)
    bs = eng.batch_struct(caps, blob, node_pe)
    st = eng.stream()
    emb = eng.fill_embed()
    for l in range(eng.L):
        eng.layer_fwd(ws, cfg, bs, l, emb, st)
    h, tab = eng.fill_head(ws, L.RO_FWD | L.RO_LOSS | L.RO_BWD, L.GTR_LOSS["bpr"])
    last = ws.layers[eng.L - 1]
    outs = {"se": ws.se, "dy": last["dy"], "coef_tgt": ws.coef_tgt, "coef_neg": ws.coef_neg,
            "bn_gpart": last["bn_gpart"], "loss_part": ws.loss_part}
    lib = L.lib()
    mean_pool = L.GtrPool(kind=L.GTR_POOL["mean"])

    def run(call):
        for t in outs.values():
            t.fill_(float("nan"))
        L.check(call(), "readout")
        torch.cuda.synchronize()
        return {k: t.clone() for k, t in outs.items()}

    args = (C.byref(cfg), C.byref(bs), tab, ws.structs, C.byref(h))
    want = run(lambda: lib.gtr_readout_loss(*args, st))
    grid = int(lib.gtr_readout_grid(caps.b_cap))
    assert bool(torch.isfinite(want["se"][:32]).all()) and bool(torch.isfinite(want["loss_part"][: 2 * grid]).all())
    for name, call in (("NULL", lambda: lib.gtr_readout_pool(*args, None, st)),
                       ("MEAN", lambda: lib.gtr_readout_pool(*args, C.byref(mean_pool), st))):
        got = run(call)
        for k in outs:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (name, k)
        assert float(got["loss_part"][: 2 * grid].sum()) == float(want["loss_part"][: 2 * grid].sum())


# ---- 8. fused steps -----------------------------------------------------------------------
def _fused_vs_trio(kind, D, H, K, loss, B, n, temperature=1.0, steps=5, **kw):
    T = data().table_rows
    m, ref = make_pair(T, D, H, kind, K=K, seed=4)
    m.train(); ref.train()
    lr, wd = 1e-3, 1e-5
    fused = FusedTrainStep(m, lr=lr, weight_decay=wd, loss=loss, temperature=temperature, alpha=0.7, **kw)
    trio = OracleTrio(ref, lambda ps: torch.optim.AdamW(ps, lr=lr, weight_decay=wd))
    losses, rlosses = [], []
    for sb in batches(data(), B, n, steps, seed=11):
        losses.append(float(fused(sb.to("cuda"))))
        rb = ref_batch(sb)
        rlosses.append(float(trio.step(lambda mod, o: R.ref_train_step(mod, rb, o, loss, 0.7, temperature))))
        if kind == "attention":  # d loss / d bias == 0 exactly: all noise, bounded by 2 lr per step
            trio.noise[BIAS][:] = True
    np.testing.assert_allclose(losses, rlosses, rtol=1e-3)
    assert fused.step_end is False
    fused.flush()
    # every trained parameter elementwise, the whole item table included (a missing sweep
    # slot would leave its untouched rows a step behind)
    trio.compare(dict(m.named_parameters()), lr=lr)
    return m, fused


@pytest.mark.parametrize("use_graph", [True, False])
def test_fused_steps_attention_c2_shape(use_graph):
    m, fused = _fused_vs_trio("attention", 64, 1, 0, "bpr", 32, 5, use_graph=use_graph)
    assert fused.rows_early
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    fused.export_optimizer_state(opt)
    for p in (m.readout.attention.weight, m.readout.attention.bias):
        assert p in opt.state and opt.state[p]["exp_avg"].shape == p.shape
    assert float(opt.state[m.readout.attention.weight]["exp_avg"].abs().max()) > 0.0
    assert float(opt.state[m.readout.attention.weight]["step"]) == 5.0


def test_fused_steps_attention_c3_shape_b300():
    _fused_vs_trio("attention", 128, 4, 16, "listwise", 300, 20, temperature=0.5)


def test_fused_steps_last_dual():
    _fused_vs_trio("last", 32, 2, 0, "dual", 32, 5)


def test_fused_steps_attention_lazy_table():
    _fused_vs_trio("attention", 64, 1, 0, "bpr", 32, 5, lazy=True)


def test_fused_graph_replay_equals_eager_launches_bitwise():
    T = data().table_rows
    m1, _ = make_pair(T, 64, 1, "attention", dropout=0.1, seed=6)
    m2 = copy.deepcopy(m1)
    m1.train(); m2.train()
    f1 = FusedTrainStep(m1, loss="bpr", use_graph=True)
    f2 = FusedTrainStep(m2, loss="bpr", use_graph=False)
    for sb in batches(data(), 32, 5, 4, seed=12):
        dsb = sb.to("cuda")
        assert float(f1(dsb)) == float(f2(dsb))
    for (name, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), name
    for (name, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(a, b), name
    for name in ("m_tab", "v_tab", "m_flat", "v_flat"):
        assert torch.equal(getattr(f1, name), getattr(f2, name)), name
    assert int(f1.ws.pool_cnt.item()) == 0 and int(f2.ws.pool_cnt.item()) == 0  # the counter is re-armed


# ---- 9. FFN identity view -------------------------------------------------------------------
def _ffn_pair(T, seed, dropout=0.0):
    torch.manual_seed(seed)
    m = create_graph_transformer(T, 64, 64, num_layers=2, dropout=dropout, readout_type="attention")
    m.laplacian_pe._cached_pe = torch.rand(T, m.laplacian_k)
    with torch.no_grad():
        for bn in m.batch_norms:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    _set_readout(m)
    ref = R.RefGraphTransformer(T, embedding_dim=64, hidden_dim=64, num_layers=2, num_heads=m.num_heads,
                                dropout=dropout, readout_type="attention", use_laplacian_pe=True,
                                laplacian_k=m.laplacian_k, use_ffn=True, ffn_expansion=m.ffn_expansion)
    ref.laplacian_pe._cached_pe = torch.zeros(T, m.laplacian_k)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert set(sd) == set(ref.state_dict())
    ref.load_state_dict(sd)
    return m.cuda(), ref


def test_ffn_identity_view_train_grads():
    T = data().table_rows
    m, ref = _ffn_pair(T, 3)
    _grads_vs_oracle(m, ref, batches(data(), 32, 5, 1, seed=75)[0])


def test_ffn_identity_view_eval_forward():
    T = data().table_rows
    m, ref = _ffn_pair(T, 9, dropout=0.1)
    with torch.no_grad():
        for bn, rbn in zip(m.batch_norms, ref.batch_norms):
            bn.running_mean.uniform_(-0.1, 0.1)
            bn.running_var.uniform_(0.5, 2.0)
            rbn.running_mean.copy_(bn.running_mean.cpu())
            rbn.running_var.copy_(bn.running_var.cpu())
    m.eval(); ref.eval()
    sb = batches(data(), 48, 5, 1, seed=23)[0]
    with torch.no_grad():
        assert_close(m(sb.to("cuda")), ref(ref_batch(sb)), name="se eval")


# ---- 10. validation routes --------------------------------------------------------------------
def test_device_evaluator_equals_host_loader_ranks(tmp_path):
    from dropin_helpers import write_csvs

    from etpgt.train.dataloader import create_dataloader
    from etpgt.train.evaluator import DeviceEvaluator

    csvs = write_csvs(tmp_path, num_items=120, num_train=20, num_val=70, seed=7)

    def loader(dev):
        return create_dataloader(csvs / "val.csv", csvs / "graph_edges.csv", batch_size=16, num_negatives=5,
                                 shuffle=False, num_workers=0, device_builder=dev)

    host = loader(False)
    torch.manual_seed(11)
    m = create_graph_transformer_optimized(host.dataset.num_items, embedding_dim=64, hidden_dim=64, num_layers=2,
                                           num_heads=2, dropout=0.0, readout_type="attention",
                                           use_laplacian_pe=False)
    with torch.no_grad():
        m.item_embedding.weight[1:].normal_(0.0, 0.3)
        for bn in m.batch_norms:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
            bn.running_mean.uniform_(-0.3, 0.3)
            bn.running_var.uniform_(0.5, 2.0)
    _set_readout(m)
    m = m.cuda().eval()
    with torch.no_grad():
        want = torch.cat([m.rank_targets(m(b.to("cuda")), b.to("cuda").target_item) for b in host]).cpu()
    assert want.shape == (70,)
    for use_graph in (False, True):
        got = DeviceEvaluator(m, loader(True), use_graph=use_graph).run()
        assert got.dtype == torch.int32 and got.tolist() == want.tolist(), use_graph


# ---- 11. the train_baseline.py drop-in ----------------------------------------------------------
def test_train_baseline_attention_one_epoch_matches_oracle(tmp_path):
    """``--model graph_transformer_optimized --readout-type attention`` (D 32, H 2, L 2,
    B 16, dropout 0), one epoch; the oracle replays it as test_gpu_dropin.py does."""
    import batch_ref as BR
    from dropin_helpers import write_csvs
    from gpu_helpers import close_trained

    from etpgt.data.batch import collate_sessions
    from etpgt.train.dataloader import DeviceSessionLoader, SessionDataset
    from etpgt.utils.seed import set_seed

    spec = importlib.util.spec_from_file_location("train_baseline_ro",
                                                  os.path.join(ROOT, "scripts", "train", "train_baseline.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)
    D, H, Lc, B, n = 32, 2, 2, 16, 5
    d = write_csvs(tmp_path)
    out = tmp_path / "out" / "graph_transformer_optimized"
    trainer = tb.main(["--model", "graph_transformer_optimized", "--readout-type", "attention",
                       "--train-sessions", str(d / "train.csv"), "--val-sessions", str(d / "val.csv"),
                       "--graph-edges", str(d / "graph_edges.csv"), "--embedding-dim", str(D), "--hidden-dim", str(D),
                       "--num-layers", str(Lc), "--num-heads", str(H), "--dropout", "0", "--batch-size", str(B),
                       "--num-negatives", str(n), "--max-epochs", "1", "--num-workers", "0",
                       "--output-dir", str(tmp_path / "out")])
    assert isinstance(trainer.train_loader, DeviceSessionLoader)
    assert trainer._fused is not None and trainer._fused.builder is trainer.train_loader.builder  # the fused step
    assert trainer.model.readout_type == "attention" and trainer._fused.step_end is False
    with open(out / "history.json") as f:
        hist = json.load(f)
    sd = torch.load(out / "checkpoint_latest.pt", map_location="cpu", weights_only=True)["model_state_dict"]
    assert sd["readout.attention.weight"].shape == (1, D) and sd[BIAS].shape == (1,)

    tr = SessionDataset(d / "train.csv", d / "graph_edges.csv", n, 50)
    va = SessionDataset(d / "val.csv", d / "graph_edges.csv", n, 50)
    T = max(tr.num_items, va.num_items)
    set_seed(42)
    init = create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=Lc, num_heads=H,
                                              dropout=0.0, readout_type="attention", use_laplacian_pe=True,
                                              use_ffn=False, ffn_expansion=2)
    torch.empty((), dtype=torch.int64).random_()  # the epoch iterator's _base_seed draw
    seed = int(torch.empty((), dtype=torch.int64).random_().item())  # the epoch's RandomSampler draw
    g = torch.Generator()
    g.manual_seed(seed)
    order = torch.randperm(len(tr), generator=g).numpy()
    ref = R.ref_create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=Lc, num_heads=H,
                                                   dropout=0.0, readout_type="attention", use_laplacian_pe=True)
    isd = {k: v.clone() for k, v in init.state_dict().items()}
    isd["laplacian_pe._cached_pe"] = sd["laplacian_pe._cached_pe"].clone()  # eigsh result of the run
    ref.laplacian_pe._cached_pe = isd["laplacian_pe._cached_pe"]
    ref.load_state_dict(isd)
    trio = OracleTrio(ref, lambda ps: torch.optim.AdamW(ps, lr=1e-3, weight_decay=1e-5))
    ei = tr.edge_index.numpy()
    keys = np.unique(ei[0].astype(np.int64) * tr.num_items + ei[1].astype(np.int64))
    S = len(tr)
    losses = []
    for i in range(-(-S // B)):
        b = min(B, S - i * B)
        ex = BR.build_batch(tr._ptr, tr._items, keys, tr.num_items, order, i * B, b, 50, n, 42)
        rb = R.ref_batch_from(collate_sessions(ex))
        losses.append(float(trio.step(lambda mod, o: R.ref_train_step(mod, rb, o, "bpr"))))
        trio.noise[BIAS][:] = True
    want = float(np.mean(losses))
    assert abs(hist["train_loss"][0] - want) <= 1e-3 * abs(want), (hist["train_loss"][0], want)
    trio.compare({k: sd[k] for k, _ in ref.named_parameters()}, lr=1e-3)
    for k, b in ref.named_buffers():
        if "num_batches_tracked" in k:
            assert int(sd[k]) == int(b)
        elif "running" in k:
            close_trained(sd[k], b, dict(trio.ref64.named_buffers())[k], torch.zeros_like(b, dtype=torch.bool), 0.0,
                          k, dict(trio.ref1.named_buffers())[k])


# ---- 12. rejections ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kw", [{"shard_table": True}, {"data_parallel": True},
                                {"data_parallel": True, "sync_bn": True}])
def test_multi_gpu_routes_reject_the_readout(kind, kw):
    m, _ = make_pair(data().table_rows, 64, 2, kind, seed=1)
    with pytest.raises(NotImplementedError, match=f"'{kind}' readout"):
        FusedTrainStep(m, **kw)


def test_halo_step_rejects_the_readout():
    from etpgt.train.halo import HaloTrainStep

    m, _ = make_pair(data().table_rows, 64, 2, "attention", seed=1)
    with pytest.raises(NotImplementedError, match="'attention' readout"):
        HaloTrainStep(m)


def test_max_still_raises_at_hip_engine():
    m = create_graph_transformer_optimized(data().table_rows, embedding_dim=64, hidden_dim=64, readout_type="max",
                                           use_laplacian_pe=False).cuda()
    with pytest.raises(NotImplementedError, match="max"):
        m.hip_engine()
