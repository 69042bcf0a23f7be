#!/usr/bin/env python3
"""Validation-path measurements on the MI355X: gtr_target_rank beside gtr_score_topk, and a
validation epoch through the three routes (project tool; bench.py is the training bench).

Kernel level (``--mode kernel``): ``score_topk(k=20)`` and ``target_rank`` on the same
inputs, T = 82,174 rows (the C2 / C3 item table), D = 64 and 128, B = 32 / 512 / 8192.
Epoch level (``--mode epoch``): a synthetic store (C2 table, 20k sessions, batch 512, and
again at batch 32):
  (i)   the old route at its cheapest: iterate the DeviceSessionLoader, eval forward,
        ``predict(k=20)``, ``.cpu()`` per batch;
  (ii)  ``DeviceEvaluator(use_graph=False)``;
  (iii) ``DeviceEvaluator(use_graph=True)``.
Drop-in (``--mode dropin``): train_baseline-shaped CSVs, ``Trainer.evaluate`` over the host
DataLoader (the prediction-based loop of the previous evaluate restated here, and the
rank-based one) and over the device loader (``--device-eval on``).

Method: every shape warmed; device events around windows that end in a synchronise;
windows of >= ``--window`` seconds (0.5); ``--repeats`` (5) windows per variant with the
variants alternated in one process; median and (max - min) / median reported.  Bounds:
algorithmic FLOPs 2*B*T*D over the fp32 MFMA peak, table bytes
ceil(B / sessions per group) * T*D*4 over the HBM peak (MI355X_MICROARCH.md spec values).
``--mode profile`` runs a few calls of every kernel shape for a separate
``rocprofv3 --kernel-trace --stats`` run.  Prints one JSON line; ``--out`` also writes it.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "gat-recommendation_amd", ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

F32_MFMA_PEAK = 157.3e12  # FLOP/s, spec
HBM_PEAK = 8.0e12         # B/s, spec
T_C2 = 82_174
KERNEL_SHAPES = [(D, B) for D in (64, 128) for B in (32, 512, 8192)]


def _window(fn, n: int) -> float:
    """Seconds per call of n calls between two device events, ending in a synchronise."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def _calls_for(fn, window: float) -> int:
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = _window(fn, 3)
    return max(2, int(window / max(t, 1e-7)) + 1)


def _alternate(variants: dict, window: float, repeats: int) -> dict:
    """variants: name -> callable.  Alternated windows; per variant median / spread."""
    calls = {k: _calls_for(f, window) for k, f in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, f in variants.items():
            times[k].append(_window(f, calls[k]))
    out = {}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"median_ms": med * 1e3, "spread": (max(ts) - min(ts)) / med, "calls_per_window": calls[k],
                  "window_s": med * calls[k], "repeats": len(ts)}
    return out


def _kernel_inputs(D, B):
    g = torch.Generator().manual_seed(D + B)
    se = torch.randn(B, D, generator=g).cuda()
    table = (torch.randn(T_C2, D, generator=g) * 0.1).cuda()
    tgt = torch.randint(1, T_C2, (B,), generator=g).to(torch.int32).cuda()
    return se, table, tgt


def kernel_level(window, repeats):
    from etpgt.backend.ops import score_topk, target_rank

    rows = []
    for D, B in KERNEL_SHAPES:
        se, table, tgt = _kernel_inputs(D, B)
        idx = score_topk(se, table, 128)[0] if B <= 512 else None
        if idx is not None:  # same answer before the timing
            r = target_rank(se, table, idx[:, 7].contiguous())
            assert bool((r == 7).all()), "target_rank disagrees with score_topk"
        res = _alternate({"score_topk_k20": lambda: score_topk(se, table, 20),
                          "target_rank": lambda: target_rank(se, table, tgt)}, window, repeats)
        spg = 64 if B > 32 else (32 if B > 16 else 16)
        flops = 2.0 * B * T_C2 * D
        tbytes = -(-B // spg) * T_C2 * D * 4.0
        t_f, t_b = flops / F32_MFMA_PEAK, tbytes / HBM_PEAK
        row = {"D": D, "B": B, "T": T_C2, "flops": flops, "table_bytes": tbytes, "sessions_per_group": spg,
               "bound": "fp32 MFMA" if t_f >= t_b else "HBM", "bound_ms": max(t_f, t_b) * 1e3, **res}
        for k in ("score_topk_k20", "target_rank"):
            row[k]["tflops"] = flops / (row[k]["median_ms"] * 1e-3) / 1e12
            row[k]["share_of_bound"] = row["bound_ms"] / row[k]["median_ms"]
        row["topk_over_rank"] = row["score_topk_k20"]["median_ms"] / row["target_rank"]["median_ms"]
        rows.append(row)
        del se, table, tgt
    return rows


def _c2_model(T, dev):
    from etpgt.model import create_graph_transformer_optimized

    torch.manual_seed(42)
    m = create_graph_transformer_optimized(T, embedding_dim=64, hidden_dim=64, num_layers=2, num_heads=1, dropout=0.1,
                                           use_laplacian_pe=False)
    return m.to(dev).eval()


def epoch_level(window, repeats, sessions=20_000, batch=512):
    from etpgt.data.gpu_batch import GpuSessionStore
    from etpgt.data.synthetic import make_sessions_and_graph
    from etpgt.train.dataloader import DeviceSessionLoader
    from etpgt.train.evaluator import DeviceEvaluator
    from etpgt.utils.metrics import compute_metrics_from_ranks, compute_ndcg_at_k, compute_recall_at_k

    dev = torch.device("cuda", 0)
    data = make_sessions_and_graph(num_sessions=sessions, seed=42)
    m = _c2_model(data.table_rows, dev)
    store = GpuSessionStore.from_synthetic(data, dev)

    def loader():
        return DeviceSessionLoader.from_store(store, batch, 5, shuffle=False, seed=42)

    old_loader = loader()
    ev_eager = DeviceEvaluator(m, loader(), use_graph=False)
    ev_graph = DeviceEvaluator(m, loader(), use_graph=True)
    ev_graph1 = DeviceEvaluator(m, loader(), use_graph=True, batches_per_graph=1)

    @torch.no_grad()
    def old():
        preds, tg = [], []
        for b in old_loader:
            se = m(b)
            preds.append(m.predict(se, k=20).cpu())
            tg.append(b.target_item.cpu())
        preds, tg = torch.cat(preds), torch.cat(tg)
        return {f"{n}@{k}": f(preds[:, :k], tg, k=k) for k in (10, 20)
                for n, f in (("recall", compute_recall_at_k), ("ndcg", compute_ndcg_at_k))}

    want = old()
    equal = all(compute_metrics_from_ranks(ev.run(), [10, 20]) == want for ev in (ev_eager, ev_graph, ev_graph1))
    res = _alternate({"old_loader_predict_cpu": old, "evaluator_eager": ev_eager.run,
                      "evaluator_graph": ev_graph.run, "evaluator_graph_one_batch_per_graph": ev_graph1.run},
                     window, repeats)
    for v in res.values():
        v["sessions_per_s"] = sessions / (v["median_ms"] * 1e-3)
    o = res["old_loader_predict_cpu"]["median_ms"]
    return {"sessions": sessions, "batch": batch, "T": data.table_rows, "D": 64, "metrics": want,
            "routes_give_equal_metrics": equal, "routes": res,
            "old_over_eager": o / res["evaluator_eager"]["median_ms"],
            "old_over_graph": o / res["evaluator_graph"]["median_ms"]}


def dropin_level(window, repeats, num_val=2000, batch=32):
    """Reference-format CSVs (the drop-in user's files): Trainer.evaluate over the host
    DataLoader and over the device loader, the previous prediction-based loop beside them."""
    from dropin_helpers import write_csvs

    from etpgt.model import create_graph_transformer_optimized
    from etpgt.train.dataloader import create_dataloader
    from etpgt.train.trainer import Trainer
    from etpgt.utils.metrics import compute_ndcg_at_k, compute_recall_at_k

    with tempfile.TemporaryDirectory() as td:
        d = write_csvs(Path(td), num_items=2000, num_train=50, num_val=num_val, seed=5)
        kw = dict(graph_edges_path=d / "graph_edges.csv", batch_size=batch, num_negatives=5, shuffle=False,
                  num_workers=0)
        host = create_dataloader(d / "val.csv", **kw)
        devl = create_dataloader(d / "val.csv", device_builder=True, **kw)
        torch.manual_seed(42)
        m = create_graph_transformer_optimized(host.dataset.num_items, embedding_dim=64, hidden_dim=64, num_layers=2,
                                               num_heads=2, dropout=0.1, use_laplacian_pe=False).cuda().eval()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
        tr_host = Trainer(m, [], host, opt, device="cuda", output_dir=Path(td) / "o1", k_values=[10, 20])
        tr_dev = Trainer(m, [], devl, opt, device="cuda", output_dir=Path(td) / "o2", k_values=[10, 20])

        @torch.no_grad()
        def previous():
            preds, tg = [], []
            for b in host:
                b = b.to("cuda")
                preds.append(m.predict(m(b), k=20).cpu())
                tg.append(b.target_item.cpu())
            preds, tg = torch.cat(preds), torch.cat(tg)
            return {f"{n}@{k}": f(preds[:, :k], tg, k=k) for k in (10, 20)
                    for n, f in (("recall", compute_recall_at_k), ("ndcg", compute_ndcg_at_k))}

        want = previous()
        assert tr_host.evaluate() == want and tr_dev.evaluate() == want
        res = _alternate({"host_loader_previous_evaluate": previous, "host_loader_evaluate": tr_host.evaluate,
                          "device_eval_on": tr_dev.evaluate}, window, repeats)
        tr_dev.close()
    p = res["host_loader_previous_evaluate"]["median_ms"]
    return {"val_sessions": num_val, "batch": batch, "routes": res,
            "previous_over_host": p / res["host_loader_evaluate"]["median_ms"],
            "previous_over_device_eval": p / res["device_eval_on"]["median_ms"]}


def profile_run():
    """A few calls of every kernel shape (for rocprofv3 --kernel-trace --stats, run apart)."""
    from etpgt.backend.ops import score_topk, target_rank

    for D, B in KERNEL_SHAPES:
        se, table, tgt = _kernel_inputs(D, B)
        for _ in range(5):
            score_topk(se, table, 20)
            target_rank(se, table, tgt)
        torch.cuda.synchronize()
    return {"shapes": KERNEL_SHAPES, "calls_per_shape": 5}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", default="all", choices=["all", "kernel", "epoch", "dropin", "profile"])
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (>= 0.5)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eval" / "eval_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on the MI355X: no GPU found (nothing is measured on the CPU)")
    from etpgt.backend import _lib as L

    res = {"tool": "scripts/eval_bench.py", "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(),
           "window_s": args.window, "repeats": args.repeats, "unix_time": int(time.time())}
    if args.mode == "profile":
        res["profile"] = profile_run()
        print(json.dumps(res))
        return res
    if args.mode in ("all", "kernel"):
        res["kernel"] = kernel_level(args.window, args.repeats)
    if args.mode in ("all", "epoch"):
        res["epoch"] = epoch_level(args.window, args.repeats)
        res["epoch_b32"] = epoch_level(args.window, args.repeats, batch=32)  # the drop-in default batch
    if args.mode in ("all", "dropin"):
        res["dropin"] = dropin_level(args.window, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
