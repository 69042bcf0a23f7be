"""C2-shaped fused step (82k items, D 64, 1 head, BPR, B 32) with a chosen session readout:
step time from device events, one JSON line.  Run it under ``rocprofv3 --kernel-trace
--stats`` for the readout kernel's average.

  python scripts/readout_pool_bench.py --readout attention --steps 200
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gat-recommendation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readout", default="attention", choices=["mean", "last", "attention"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=32)
    args = ap.parse_args()

    from etpgt.data.batch import Caps
    from etpgt.data.synthetic import make_batches, make_sessions_and_graph
    from etpgt.model import create_graph_transformer_optimized
    from etpgt.train.fused import FusedTrainStep

    dev = torch.device("cuda:0")
    data = make_sessions_and_graph(seed=42)
    B = args.batch_size
    batches = make_batches(data, B, 16, 5, seed=42)
    torch.manual_seed(42)
    model = create_graph_transformer_optimized(data.table_rows, embedding_dim=64, hidden_dim=64, num_layers=2,
                                               num_heads=1, dropout=0.1, readout_type=args.readout,
                                               use_laplacian_pe=False).to(dev).train()
    step = FusedTrainStep(model, lr=1e-3, weight_decay=1e-5, loss="bpr")
    caps = Caps(max(b.num_nodes for b in batches), B, max(b.num_edges for b in batches), 5)
    step._bind(caps)
    staged = [torch.from_numpy(b.packed(step.caps)[1]).to(dev) for b in batches]
    for i in range(args.warmup):
        step.load_blob(staged[i % len(staged)])
        step.run()
    main_s = torch.cuda.current_stream()
    ev = []
    for i in range(args.steps):
        step.load_blob(staged[i % len(staged)])  # outside the events: the copy is not timed
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(main_s)
        loss = step.run()
        e1.record(main_s)
        ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    print(json.dumps({"readout": args.readout, "B": B, "T": data.table_rows, "steps": args.steps,
                      "step_end": bool(step.step_end), "rows_early": bool(step.rows_early),
                      "step_ms_median": float(np.median(ms)), "step_ms_min": float(np.min(ms)),
                      "loss": float(loss)}))


if __name__ == "__main__":
    main()
