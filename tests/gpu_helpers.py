"""Shared helpers for the GPU parity tests (HIP path vs the CPU oracle)."""

from __future__ import annotations

import numpy as np
import torch

import etpgt_ref as R
from etpgt.data.batch import SessionBatch, collate_sessions
from etpgt.data.synthetic import make_batches, make_sessions_and_graph
from etpgt.model import create_graph_transformer_optimized


def small_data(num_items=300, num_sessions=3000, num_edges=4000, seed=3):
    return make_sessions_and_graph(num_items=num_items, num_sessions=num_sessions, num_edges=num_edges, seed=seed)


def edge_case_batch(n_neg=5, T=300) -> SessionBatch:
    """Reference conftest dummy_batch (tests/conftest.py:25-50) sessions plus
    edge cases: a node with no in-edges, a single-node session with a self loop,
    a session without edges, a dense session with self loops."""
    items = [
        {"x": [1, 2, 3], "edge_index": [[0, 1, 1, 2], [1, 0, 2, 1]]},
        {"x": [4, 5, 6, 7], "edge_index": [[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]]},
        {"x": [10, 11, 12], "edge_index": [[0, 0], [1, 2]]},          # node 0 has no in-edge
        {"x": [20], "edge_index": [[0], [0]]},                         # single node, self loop
        {"x": [30, 31], "edge_index": [[], []]},                       # no edges at all
        {"x": list(range(40, 52)), "edge_index": [[a for a in range(12) for b in range(a, 12)],
                                                   [b for a in range(12) for b in range(a, 12)]]},
    ]
    rng = np.random.default_rng(0)
    out = []
    for it in items:
        x = np.array(it["x"], np.int64)
        seen = set(x.tolist())
        negs = [v for v in rng.integers(1, T, size=4 * n_neg) if int(v) not in seen][:n_neg]
        out.append({"x": x, "edge_index": np.array(it["edge_index"], np.int64).reshape(2, -1),
                    "target_item": int(rng.integers(1, T)), "negative_items": np.array(negs, np.int64)})
    return collate_sessions(out)


def long_session_batch(n_neg=5, T=300) -> SessionBatch:
    """Groups past the LDS fast path of the layer kernels: a 70-node session
    (> RMAX rows), a 40-node complete graph (1600 edges > EMAX), next to short ones."""
    rng = np.random.default_rng(1)
    items = []
    xs = rng.choice(np.arange(1, T), size=70, replace=False)
    src, dst = [], []
    for a in range(70):
        for b in range(max(0, a - 5), min(70, a + 6)):
            src.append(a); dst.append(b)
    items.append({"x": xs, "edge_index": [src, dst]})
    xs = rng.choice(np.arange(1, T), size=40, replace=False)
    items.append({"x": xs, "edge_index": [[a for a in range(40) for b in range(40)],
                                          [b for a in range(40) for b in range(40)]]})
    for _ in range(4):
        xs = rng.choice(np.arange(1, T), size=4, replace=False)
        items.append({"x": xs, "edge_index": [[0, 1, 2, 3, 1], [1, 2, 3, 0, 1]]})
    out = []
    for it in items:
        x = np.asarray(it["x"], np.int64)
        seen = set(x.tolist())
        negs = [v for v in rng.integers(1, T, size=4 * n_neg) if int(v) not in seen][:n_neg]
        out.append({"x": x, "edge_index": np.array(it["edge_index"], np.int64).reshape(2, -1),
                    "target_item": int(rng.integers(1, T)), "negative_items": np.array(negs, np.int64)})
    return collate_sessions(out)


def capacity_batch(n, e, n_neg=5, T=300, short=3) -> SessionBatch:
    """Session 0: ``n`` nodes (distinct items) and exactly ``e`` edges in a regular in-degree
    pattern -- node j receives e // n in-edges (one more for the first e % n nodes) from
    nodes j, j+1, ... (mod n), so no edge repeats -- followed by ``short`` four-node
    sessions.  With n >= the row-group width, row group 0 holds session 0 alone: a group of
    exactly n rows and e edges (group0_geometry reads that back from the packed image)."""
    deg, extra = divmod(e, n)
    assert deg + (1 if extra else 0) <= n and n + 4 * short < T, (n, e)
    rng = np.random.default_rng(2)
    items = []
    xs = rng.choice(np.arange(1, T), size=n, replace=False)
    src, dst = [], []
    for j in range(n):
        for k in range(deg + (1 if j < extra else 0)):
            src.append((j + k) % n); dst.append(j)
    assert len(src) == e
    items.append({"x": xs, "edge_index": [src, dst]})
    for _ in range(short):
        xs = rng.choice(np.arange(1, T), size=4, replace=False)
        items.append({"x": xs, "edge_index": [[0, 1, 2, 3, 1], [1, 2, 3, 0, 1]]})
    out = []
    for it in items:
        x = np.asarray(it["x"], np.int64)
        seen = set(x.tolist())
        negs = [v for v in rng.integers(1, T, size=8 * n_neg) if int(v) not in seen][:n_neg]
        assert len(negs) == n_neg
        out.append({"x": x, "edge_index": np.array(it["edge_index"], np.int64).reshape(2, -1),
                    "target_item": int(rng.integers(1, T)), "negative_items": np.array(negs, np.int64)})
    return collate_sessions(out)


def group0_geometry(sb: SessionBatch) -> tuple[int, int]:
    """(rows, edges) of row group 0 as the layer kernels will see them: grp_row / grp_edge
    read back from the batch's packed image."""
    from etpgt.data.batch import blob_layout

    caps, blob = sb.packed()
    lay = blob_layout(caps)
    gr, ge = lay["grp_row"][0], lay["grp_edge"][0]
    return int(blob[gr + 1] - blob[gr]), int(blob[ge + 1] - blob[ge])


def make_pair(T, D, H, L=2, K=0, dropout=0.0, seed=0, pe_table=None):
    """HIP model (cuda) + oracle model (cpu) with identical parameters."""
    torch.manual_seed(seed)
    m = create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=L, num_heads=H,
                                           dropout=dropout, use_laplacian_pe=K > 0, laplacian_k=max(K, 1))
    if K > 0:
        m.laplacian_pe._cached_pe = pe_table if pe_table is not None else torch.rand(T, K)
    # non-trivial BN affine params so their gradients are exercised
    with torch.no_grad():
        for bn in m.batch_norms:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    ref = R.ref_create_graph_transformer_optimized(T, embedding_dim=D, hidden_dim=D, num_layers=L, num_heads=H,
                                                   dropout=dropout, use_laplacian_pe=K > 0, laplacian_k=max(K, 1))
    if K > 0:
        ref.laplacian_pe._cached_pe = torch.zeros(T, K)
    ref.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    return m.cuda(), ref


def ref_batch(sb: SessionBatch):
    return R.ref_batch_from(sb)


def assert_close(a, b, rtol=1e-3, name="", floor=0.0):
    """|a - b| <= rtol * (|b| + scale*1e-2) elementwise, scale = max|b|: 1e-3 relative
    with an absolute floor at 1e-5 of the tensor's scale for near-zero entries; ``floor``
    adds an absolute term for tensors that are mathematically zero (e.g. the key-bias
    gradient, to which the per-destination softmax is invariant)."""
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape, f"{name}: shape {a.shape} vs {b.shape}"
    scale = float(b.abs().max()) if b.numel() else 0.0
    tol = rtol * (b.abs() + 1e-2 * scale) + floor + 1e-12
    err = (a - b).abs()
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.argmax((err - tol).reshape(-1)))
        raise AssertionError(f"{name}: {int(bad.sum())}/{b.numel()} mismatches; worst idx {i}: "
                             f"{a.reshape(-1)[i].item():.7g} vs {b.reshape(-1)[i].item():.7g} (scale {scale:.3g})")


def batches(data, B, n, count, seed=0):
    return make_batches(data, B, count, n, seed=seed)


def assert_close_norm(a, b, rtol=1e-3, name=""):
    """Tensor-level relative error ||a - b|| / ||b|| <= rtol (parameter trajectories:
    Adam normalises near-zero, rounding-dominated gradient entries to +-lr steps, so a
    few entries legitimately differ while the tensor as a whole must agree)."""
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape, f"{name}: shape {a.shape} vs {b.shape}"
    den = float(b.norm())
    err = float((a - b).norm()) / den if den > 0 else float((a - b).norm())
    assert err <= rtol, f"{name}: relative error {err:.3g} > {rtol}"


FALLBACK_FRAC = 1e-4  # most of a tensor's elements that may pass only through the fp32-noise fallback


def _audit(rec: dict) -> None:
    """Append one close_trained record to the session's audit file (conftest sets
    GTR_PARITY_AUDIT; spawned rank processes inherit it), summed at the end of the run."""
    import json
    import os

    path = os.environ.get("GTR_PARITY_AUDIT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def close_trained(a, b, c, allow, bound, name, b1=None):
    """Elementwise bar for TRAINED parameters.  a: HIP, b: fp32 oracle, c: fp64 oracle, b1:
    the fp32 oracle in a second summation order (one CPU thread); allow: elements whose
    first gradient was at the fp32 noise floor (bounded by ``bound`` = 2 lr per step).

    An element matches when |a - b| <= 1e-3 (|b| + 1e-2 max|b|) + 8 * (its fp32 oracle's
    distance to fp64, the larger of the two orders); one that misses is still accepted
    when the HIP value is no further from fp64 than the fp32 oracle's worst distance to
    fp64 anywhere in the tensor (Adam turns a gradient that nearly cancels -- rounded
    differently by any two fp32 summation orders -- into an update that differs by a
    fraction of lr).  That fallback is audited: more than FALLBACK_FRAC of a tensor's
    elements (floor: none of a tensor under 10k elements) accepted only through it fails
    the check, and every call is recorded for the run's summary (tests/conftest.py)."""
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    c = c.detach().cpu()
    allow = allow.cpu()
    if bool(allow.any()):
        assert float((a[allow] - b[allow]).abs().max()) <= bound + 1e-7, name
    keep = ~allow
    a, b, c = a[keep], b[keep], c[keep].float()
    dev = (b - c).abs()
    if b1 is not None:
        dev = torch.maximum(dev, (b1.detach().float().cpu()[keep] - c).abs())
    scale = float(b.abs().max()) if b.numel() else 0.0
    tol = 1e-3 * (b.abs() + 1e-2 * scale) + 8 * dev + 1e-12
    err = (a - b).abs()
    floor = float(dev.max()) if b.numel() else 0.0
    near = err > tol
    bad = near & ((a - c).abs() > floor)
    n_fb = int(near.sum()) - int(bad.sum())
    _audit({"name": name, "elements": int(b.numel()), "fallback": n_fb, "bad": int(bad.sum()),
            "noise_floor_elements": int(allow.sum())})
    if bool(bad.any()):
        i = int(torch.argmax((err - tol) * bad))
        raise AssertionError(f"{name}: {int(bad.sum())}/{b.numel()} mismatches; worst: hip {a[i].item():.7g} "
                             f"oracle fp32 {b[i].item():.7g} fp64 {c[i].item():.7g} (fp32 noise level {floor:.3g})")
    limit = int(FALLBACK_FRAC * b.numel())
    assert n_fb <= limit, (f"{name}: {n_fb}/{b.numel()} elements pass only through the tensor-wide fp32-noise "
                           f"fallback (limit {limit})")
    ill = int(((b - c).abs() > 1e-3 * (b.abs() + 1e-2 * scale)).sum())
    print(f"{name}: {b.numel()} elements within 1e-3 of the fp32 oracle or of its own fp64 distance "
          f"({ill} where fp32 itself is off by more than 1e-3; {n_fb} within the tensor's fp32 "
          f"noise level {floor:.3g} of fp64 only)")


class OracleTrio:
    """One oracle training run replayed three ways -- fp32 (the reference's precision),
    fp32 on one CPU thread (a second summation order) and fp64 -- so that trained HIP
    parameters can be held to ``close_trained`` ELEMENTWISE.  ``make_opt(params)`` builds
    the run's optimizer; ``step(fn)`` runs ``fn(model, opt) -> loss`` on all three and
    records which elements' first gradient was at the fp32 noise floor."""

    def __init__(self, ref, make_opt):
        import copy

        self.ref = ref
        self.ref1 = copy.deepcopy(ref)
        self.ref64 = copy.deepcopy(ref).double()
        lp = getattr(self.ref64, "laplacian_pe", None)
        if lp is not None and lp._cached_pe is not None:
            lp._cached_pe = lp._cached_pe.double()
        self.opt = make_opt(self.ref.parameters())
        self.opt1 = make_opt(self.ref1.parameters())
        self.opt64 = make_opt(self.ref64.parameters())
        self.seen = {n: torch.zeros_like(p, dtype=torch.bool) for n, p in ref.named_parameters()}
        self.noise = {n: torch.zeros_like(p, dtype=torch.bool) for n, p in ref.named_parameters()}
        self.steps = 0

    def step(self, fn):
        loss = fn(self.ref, self.opt)
        fn(self.ref64, self.opt64)
        nthr = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            fn(self.ref1, self.opt1)
        finally:
            torch.set_num_threads(nthr)
        self.steps += 1
        for n, p in self.ref.named_parameters():
            g = p.grad
            if g is None:
                continue
            if n.endswith("lin_key.bias"):  # d loss / d key bias == 0 exactly: all noise
                self.noise[n][:] = True
                continue
            fresh = (g != 0) & ~self.seen[n]
            self.noise[n] |= fresh & (g.abs() <= 1e-5 * float(g.abs().max()))
            self.seen[n] |= g != 0
        return loss

    def compare(self, hip_params: dict, lr: float, prefix=""):
        """Every trained parameter (name -> HIP tensor) against the trio."""
        p1 = dict(self.ref1.named_parameters())
        p64 = dict(self.ref64.named_parameters())
        for n, p in self.ref.named_parameters():
            close_trained(hip_params[n], p, p64[n], self.noise[n], 2 * lr * self.steps, prefix + n, p1[n])


def eval_vs_oracle(m, ref, sbs, name="se"):
    """Eval-mode forward (running statistics set to non-trivial values on both sides):
    session embeddings of every batch against the oracle at 1e-3."""
    with torch.no_grad():
        for bn, rbn in zip(m.batch_norms, ref.batch_norms):
            bn.running_mean.uniform_(-0.1, 0.1)
            bn.running_var.uniform_(0.5, 2.0)
            rbn.running_mean.copy_(bn.running_mean.cpu())
            rbn.running_var.copy_(bn.running_var.cpu())
    m.eval(); ref.eval()
    for i, sb in enumerate(sbs):
        with torch.no_grad():
            se = m(sb.to("cuda"))
            se_ref = ref(ref_batch(sb))
        assert_close(se, se_ref, name=f"{name} (batch {i})")


def grads_vs_oracle(m, ref, sb, loss="model_bpr", masks=None, stats=True, name=""):
    """One train-mode step through autograd (batch BatchNorm statistics; dropout 0, or the
    oracle applying ``masks``): loss, session embeddings, every parameter gradient (dense
    table gradient included) and the BatchNorm running statistics -- the bars of
    test_gpu_parity.test_train_grads (1e-3; gradients 2e-3 with a floor of 1e-6 of the
    largest gradient entry)."""
    from etpgt.train.losses import create_loss_function

    m.train(); ref.train()
    dsb = sb.to("cuda")
    B = sb.num_graphs
    n = int(sb.negative_items.numel()) // B
    se = m(dsb)
    ref.drop_masks = masks
    rb = ref_batch(sb)
    se_ref = ref(rb)
    ref.drop_masks = None
    neg = dsb.negative_items.view(B, n)
    if loss == "model_bpr":
        L_hip = m.compute_loss(se, dsb.target_item, neg)
    else:
        out = create_loss_function(loss, alpha=0.7, temperature=0.5)(se, dsb.target_item, neg, m.item_embedding)
        L_hip = out[0] if isinstance(out, tuple) else out
    kind = "bpr" if loss == "model_bpr" else loss
    L_ref = R.ref_loss(kind, se_ref, rb.target_item, rb.negative_items.view(B, n), ref.item_embedding, 0.7, 0.5)
    m.zero_grad()
    L_hip.backward()
    ref.zero_grad()
    L_ref.backward()
    assert_close(se, se_ref, name=f"{name}se")
    assert_close(L_hip.reshape(1), L_ref.reshape(1), name=f"{name}loss")
    hp = dict(m.named_parameters())
    gscale = max(float(p.grad.abs().max()) for p in ref.parameters())
    for pn, p in ref.named_parameters():
        assert hp[pn].grad is not None, pn
        assert_close(hp[pn].grad, p.grad, rtol=2e-3, name=f"{name}grad {pn}", floor=1e-6 * gscale)
    if stats:
        hb = dict(m.named_buffers())
        for bn_, b in ref.named_buffers():
            if "running" in bn_:
                assert_close(hb[bn_], b, name=f"{name}{bn_}")


def fused_vs_trio(data, D, H, K=0, L=2, loss="bpr", B=32, steps=3, seed=4, lr=1e-3, wd=1e-2):
    """``steps`` fused steps (FusedTrainStep: graph replay, AdamW) against OracleTrio, as
    test_gpu_parity._fused_vs_reference: losses at 2e-3, every trained parameter and the
    running statistics elementwise (close_trained).  Returns the fused step, so the caller
    can assert the path it took (step_end, ws.split)."""
    from etpgt.train.fused import FusedTrainStep

    n = 5 if loss != "listwise" else 100
    m, ref = make_pair(data.table_rows, D, H, L=L, K=K, seed=seed)
    m.train(); ref.train()
    fused = FusedTrainStep(m, lr=lr, weight_decay=wd, decoupled=True, loss=loss, temperature=1.0, alpha=0.7)
    trio = OracleTrio(ref, lambda ps: torch.optim.AdamW(ps, lr=lr, weight_decay=wd))
    bl = batches(data, B, n, steps, seed=11)
    losses, rlosses = [], []
    for sb in bl:
        losses.append(float(fused(sb.to("cuda"))))
        rb = ref_batch(sb)
        rlosses.append(float(trio.step(lambda mod, o: R.ref_train_step(mod, rb, o, loss))))
    np.testing.assert_allclose(losses, rlosses, rtol=2e-3)
    fused.flush()
    trio.compare(dict(m.named_parameters()), lr=lr)
    b64, b1 = dict(trio.ref64.named_buffers()), dict(trio.ref1.named_buffers())
    hb = dict(m.named_buffers())
    for name, b in ref.named_buffers():
        if "running" in name:
            close_trained(hb[name], b, b64[name], torch.zeros_like(b, dtype=torch.bool), 0.0, name, b1[name])
    assert int(hb["batch_norms.0.num_batches_tracked"]) == len(bl)
    return fused


def collect(q, procs, n, timeout=400.0):
    """n results from worker processes: polls the queue and fails FAST (instead of blocking
    for the whole timeout) as soon as a worker has exited with an error -- a dead rank
    would otherwise leave the test silent until the box's hang watchdog kills it."""
    import queue
    import time

    out = []
    t_end = time.time() + timeout
    while len(out) < n:
        try:
            out.append(q.get(timeout=2.0))
            continue
        except queue.Empty:
            pass
        bad = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
        if bad:
            for p in procs:
                if p.is_alive():
                    p.terminate()
            raise AssertionError(f"a worker process failed (exit codes {bad})")
        if time.time() > t_end:
            for p in procs:
                if p.is_alive():
                    p.terminate()
            raise AssertionError(f"workers timed out after {timeout:.0f} s")
    return out
