#!/usr/bin/env python3
"""Serving measurements on the MI355X: a loop of ``Recommender.recommend`` beside one
``Recommender.recommend_batch`` call on the same requests (project tool; bench.py is the
training bench).

Workload: the C2 item table (82,174 items, d = 64, LapPE 16, 2 layers, 2 heads), the
synthetic RetailRocket-shaped graph written as graph_edges.csv, the first B sessions of the
synthetic store as requests, k = 10, B = 1 / 32 / 256 / 2048.  Both routes end in a copy
to the host, so WALL time per call is measured (``time.perf_counter`` around windows that
start after a synchronise); per-request time = call time / B.

Method: both routes warmed at every B and checked to return the same ids; windows of
>= ``--window`` seconds (0.5); ``--repeats`` (5) windows per route, the routes alternated in
one process; median and (max - min) / median reported.

``--mode profile --batch B`` runs ``--calls`` recommend_batch calls at one B (and nothing
else after the warm-up) for a separate ``rocprofv3 --kernel-trace --stats`` run;
``--mode split --stats kernel_stats.csv`` turns that run's stats into device time per call
for the graph build (k_sv_*), the top-k (k_topk_*) and the forward (every other kernel).
Prints one JSON line; ``--out`` also writes it.
"""

from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "gat-recommendation_amd", ROOT):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

BATCHES = (1, 32, 256, 2048)
K = 10
WARM_CALLS = 3


def make_recommender(tmp: Path, sessions: int):
    import pandas as pd

    from etpgt.data.synthetic import make_sessions_and_graph, random_pe_table
    from etpgt.model import create_graph_transformer_optimized
    from etpgt.serving import Recommender, ValidatedRequest

    data = make_sessions_and_graph(num_sessions=max(sessions, 4096), seed=42)
    T = data.table_rows
    torch.manual_seed(42)
    m = create_graph_transformer_optimized(T, embedding_dim=64, hidden_dim=64, num_layers=2, num_heads=2, dropout=0.1,
                                           use_laplacian_pe=True, laplacian_k=16)
    m.laplacian_pe._cached_pe = random_pe_table(T, 16, seed=42)
    torch.save({"epoch": 0, "model_state_dict": m.state_dict()}, tmp / "ck.pt")
    ei = data.edge_index()
    pd.DataFrame({"item_i": ei[0], "item_j": ei[1]}).to_csv(tmp / "graph_edges.csv", index=False)
    rec = Recommender(tmp / "ck.pt", tmp / "graph_edges.csv", device="cuda")
    reqs = [ValidatedRequest(data.session(s).tolist()[-50:], K) for s in range(sessions)]
    return rec, reqs, T


def _window(fn, n: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n


def _alternate(variants: dict, window: float, repeats: int) -> dict:
    calls = {}
    for k, f in variants.items():
        for _ in range(WARM_CALLS):
            f()
        calls[k] = max(2, int(window / max(_window(f, 2), 1e-7)) + 1)
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


def measure(window, repeats):
    rows = []
    with tempfile.TemporaryDirectory() as td:
        rec, reqs, T = make_recommender(Path(td), max(BATCHES))
        for B in BATCHES:
            rq = reqs[:B]
            loop = lambda: [rec.recommend(r) for r in rq]  # noqa: E731
            batch = lambda: rec.recommend_batch(rq)  # noqa: E731
            a, b = loop(), batch()
            same_ids = sum(x[0] == y[0] for x, y in zip(a, b))
            diff = max(abs(p - q) for x, y in zip(a, b) for p, q in zip(x[1], y[1]))
            res = _alternate({"recommend_loop": loop, "recommend_batch": batch}, window, repeats)
            for v in res.values():
                v["us_per_request"] = v["median_ms"] * 1e3 / B
            rows.append({"B": B, "T": T, "D": 64, "k": K, "requests_with_equal_ids": same_ids,
                         "max_abs_score_difference": diff, **res,
                         "loop_over_batch": res["recommend_loop"]["median_ms"] / res["recommend_batch"]["median_ms"]})
    return rows


def profile_run(B, calls):
    with tempfile.TemporaryDirectory() as td:
        rec, reqs, _ = make_recommender(Path(td), B)
        for _ in range(WARM_CALLS + calls):
            rec.recommend_batch(reqs[:B])
        torch.cuda.synchronize()
    return {"B": B, "calls": WARM_CALLS + calls}


def split_stats(path, calls):
    """Device microseconds per recommend_batch call by part, from a kernel_stats.csv of a
    ``--mode profile`` run of ``calls`` calls (its JSON line says how many)."""
    import re

    # the library's other kernels are the eval forward (k_conv_fwd / k_proj + k_attn_*, k_readout*)
    groups = (("build", "k_sv_"), ("topk", "k_topk_"), ("forward", "::k_"), ("copies", "__amd_rocclr_"))
    part = {"build": 0.0, "forward": 0.0, "topk": 0.0, "copies": 0.0, "torch_glue": 0.0}
    names = {k: [] for k in part}
    for x in csv.DictReader(open(path)):
        n = x["Name"]
        if "k_edge_hash_build" in n:
            continue  # start-up: the graph hash, once per Recommender
        key = next((g for g, pat in groups if pat in n), "torch_glue")  # casts, cat, clone, fills
        part[key] += float(x["TotalDurationNs"]) / 1e3 / calls
        short = re.search(r"(k_\w+|__amd_rocclr_\w+|at::native::\w+)", n)
        names[key].append(f"{short.group(1) if short else n[:40]} x{int(x['Calls']) / calls:.2g} "
                          f"{float(x['AverageNs']) / 1e3:.1f}us")
    return {"calls": calls, "device_us_per_call": part, "kernels": names}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", default="measure", choices=["measure", "profile", "split"])
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (>= 0.5)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="profile mode: requests per call")
    ap.add_argument("--calls", type=int, default=20, help="profile / split mode: calls after the warm-up")
    ap.add_argument("--stats", help="split mode: rocprofv3 kernel_stats.csv of a profile run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.mode == "split":
        res = {"tool": "scripts/serve_bench.py", "B": args.batch,
               **split_stats(args.stats, WARM_CALLS + args.calls)}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("serve_bench.py measures on the MI355X: no GPU found (nothing is measured on the CPU)")
        from etpgt.backend import _lib as L

        res = {"tool": "scripts/serve_bench.py", "device": torch.cuda.get_device_name(0),
               "source_hash": L.source_hash(), "window_s": args.window, "repeats": args.repeats,
               "unix_time": int(time.time())}
        if args.mode == "profile":
            res["profile"] = profile_run(args.batch, args.calls)
        else:
            res["serve"] = measure(args.window, args.repeats)
    out = args.out or (str(ROOT / "profiles" / "serve" / "serve_bench.json") if args.mode == "measure" else None)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
