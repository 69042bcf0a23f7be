"""What SyncBN costs the FFN model's fused step on one GPU (world 1): the reference-default
FFN model (`create_graph_transformer`: d 256, 3 layers, 4 heads, FFN x 4, LapPE 16) on the
RetailRocket-shaped synthetic store, device-built batches, at B = 32 and B = 1024.

Three steps in one process, their timing windows alternated:
  a  data_parallel=True, sync_bn=False   (producer-finalized statistics)
  b  sync_bn=True                        (the consumers read the producers' rows in place)
  c  sync_bn=True, GTR_SYNC_NOALIAS=1    (the gathers of a multi-rank run kept as copies)
b - a is one k_gen_bn_sync launch per layer (still one captured graph); c - a adds the step's
cuts at the gathers and the row copies between them.

Device-event timing, windows of >= 0.5 s after every shape is warm, 5 repeats: median and
spread (min, max) of ms per step.  Prints one JSON line and writes it to
profiles/ffn_sync/ffn_sync_bench.json.

usage: python scripts/ffn_sync_bench.py [--variants abc] [--batches 32,1024] [--repo CHECKOUT] [--out FILE]
  --repo: import the package (and its built library) from another checkout of this
          repository, e.g. the parent commit's, for an A/B of step a.
"""
import argparse
import copy
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = {
    "a": ("data_parallel, sync_bn=False", dict(data_parallel=True, sync_bn=False), None),
    "b": ("sync_bn=True (aliased rows)", dict(data_parallel=True, sync_bn=True), None),
    "c": ("sync_bn=True, GTR_SYNC_NOALIAS=1 (gathered copies)", dict(data_parallel=True, sync_bn=True), "1"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="abc")
    ap.add_argument("--batches", default="32,1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timing window (at least)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repo", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffn_sync", "ffn_sync_bench.json"))
    args = ap.parse_args()
    repo = os.path.abspath(args.repo)
    sys.path.insert(0, os.path.join(repo, "gat-recommendation_amd"))

    import torch

    from etpgt.backend import _lib
    from etpgt.data.gpu_batch import GpuBatchBuilder, GpuSessionStore
    from etpgt.data.synthetic import make_sessions_and_graph
    from etpgt.model import create_graph_transformer
    from etpgt.train.fused import FusedTrainStep

    D, H, L, K, NNEG = 256, 4, 3, 16, 5
    data = make_sessions_and_graph(seed=42)
    T = data.table_rows
    torch.manual_seed(0)
    base = create_graph_transformer(T, embedding_dim=D, hidden_dim=D, num_layers=L, num_heads=H, dropout=0.1,
                                    use_laplacian_pe=True, laplacian_k=K, use_ffn=True, ffn_expansion=4)
    base.laplacian_pe._cached_pe = torch.rand(T, K)
    store = GpuSessionStore.from_synthetic(data, "cuda")
    names = [v for v in args.variants if v in VARIANTS]
    batch_sizes = [int(b) for b in args.batches.split(",")]

    def make(v, B):
        _, kw, noalias = VARIANTS[v]
        m = copy.deepcopy(base).cuda().train()
        os.environ.pop("GTR_SYNC_NOALIAS", None)
        if noalias:
            os.environ["GTR_SYNC_NOALIAS"] = noalias
        try:
            fs = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, loss="bpr", **kw)
            fs.attach_builder(GpuBatchBuilder(store, B, NNEG, seed=6), num_batches=4096)
            for _ in range(args.warmup):  # the first run warms up eagerly and captures
                fs.run()
            torch.cuda.synchronize()
        finally:
            os.environ.pop("GTR_SYNC_NOALIAS", None)
        assert fs.split and bool(getattr(fs, "sync_alias", False)) == (v == "b")
        return fs

    def window(fs, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fs.run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    steps = {B: {v: make(v, B) for v in names} for B in batch_sizes}  # every shape warm before any timing
    out = {"model": "graph_transformer (use_ffn=True, ffn_expansion=4)", "dim": D, "heads": H, "layers": L,
           "lap_k": K, "negatives": NNEG, "world": 1, "repeats": args.repeats, "window_s": args.window,
           "timing": "device events", "source_hash": _lib.library_source_hash(),
           "checkout": "this tree" if repo == ROOT else os.path.basename(repo), "results": []}
    for B in batch_sizes:
        n = {v: max(20, math.ceil(args.window * 1e3 / window(steps[B][v], 20))) for v in names}
        ms = {v: [] for v in names}
        for _ in range(args.repeats):
            for v in names:  # alternated
                ms[v].append(window(steps[B][v], n[v]))
        for v in names:
            fs = steps[B][v]
            out["results"].append({"batch": B, "variant": v, "what": VARIANTS[v][0], "steps_per_window": n[v],
                                   "ms_per_step_median": round(statistics.median(ms[v]), 5),
                                   "ms_per_step_min": round(min(ms[v]), 5), "ms_per_step_max": round(max(ms[v]), 5),
                                   "graph_pieces": len(fs.graph) if fs.graph is not None else None,
                                   "final_loss": round(float(fs.ws.loss_out[0]), 5)})
        for fs in steps[B].values():
            fs.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
