"""Validation epochs on the device (Trainer.evaluate over a ``DeviceSessionLoader``).

Recall@K / NDCG@K (trainer.py:138-173) depend on one number per session: the position of
the target in ``predict``'s ordering of the catalog.  ``DeviceEvaluator`` computes those
positions for a whole validation set without host work per batch:

    gtr_build_batch  ->  eval forward (conv_fwd.. -> readout)  ->  gtr_target_rank

* the batch constructor writes the next ``batch_size`` sessions of the epoch order into one
  fixed batch image and records the batch's first position in its device ``start`` word;
* the forward runs in eval mode (running BatchNorm statistics, no dropout) into the
  workspace's session embeddings;
* ``gtr_target_rank`` scans the item table once and stores every session's rank at
  ``ranks[start - base + b]``, ``base`` a device word holding the epoch's first position.

Nothing in the chain depends on the host, so it is captured once -- ``batches_per_graph``
consecutive chains as one hipGraph, plus a one-batch graph for the full batches that do not
fill one -- and replayed for every full batch of every epoch; the partial last batch
(``drop_last=False``) is launched eagerly.  One device-to-host copy of the ``S`` ranks ends the epoch; the metrics are then
``etpgt.utils.metrics.compute_metrics_from_ranks`` on the host, in session order.
"""

from __future__ import annotations

import ctypes as C

import torch

from etpgt.backend import _lib as L
from etpgt.data.batch import blob_layout

GUARD = 64  # int32 words past the S ranks that no launch may touch (checked every epoch)


class DeviceEvaluator:
    def __init__(self, model, loader, use_graph: bool = True, batches_per_graph: int = 16):
        """``batches_per_graph``: consecutive full batches captured as ONE hipGraph (each
        chain's build advances the device cursor, as in ``FusedTrainStep.capture_steps_built``);
        the batches that do not fill such a graph replay a one-batch graph each."""
        from etpgt.model.graph_transformer import GraphTransformer

        if not isinstance(model, GraphTransformer):
            raise TypeError("DeviceEvaluator runs the GraphTransformer HIP forward")
        if loader.world != 1:
            raise ValueError("DeviceEvaluator walks the whole validation set on one device (world == 1)")
        if loader.shuffle:
            raise ValueError("DeviceEvaluator needs shuffle=False: the metrics are means in session order")
        self.model = model
        self.loader = loader
        self.builder = loader.builder
        self.use_graph = bool(use_graph)
        self.S = int(loader.num_sessions)
        self.B = int(loader.batch_size)
        dev = self.builder.store.device
        self.dev = dev
        self.ranks = torch.full((self.S + GUARD,), -1, dtype=torch.int32, device=dev)
        self.base = torch.zeros(1, dtype=torch.int64, device=dev)
        self.K = max(1, int(batches_per_graph))
        self.caps = None
        self.graph = None    # one batch
        self.graph_k = None  # K consecutive batches
        self._sig = None
        self.captures = 0

    # ------------------------------------------------------------------ binding
    def _signature(self, eng):
        pe = self.model.laplacian_pe._cached_pe if eng.K > 0 else None
        return (id(eng), eng.flat._ptrs, self.model.item_embedding.weight.data_ptr(),
                None if pe is None else pe.data_ptr(), self.caps)

    def _bind(self, eng, caps):
        """One blob, one workspace and the rank kernel's key buffer for these capacities."""
        self.caps = caps
        self.eng = eng
        self.blob = torch.zeros(blob_layout(caps)["_total"], dtype=torch.int32, device=self.dev)
        self.bs = eng.batch_struct(caps, self.blob, None)
        self.ws = eng.workspace(caps, fresh=True)
        self.cfg = eng.config(self.ws, False)
        nb = C.c_size_t(0)
        L.check(L.lib().gtr_target_rank_workspace_bytes(caps.b_cap, eng.T, C.byref(nb)), "target_rank_workspace_bytes")
        self.rank_ws = torch.empty(int(nb.value), dtype=torch.uint8, device=self.dev)
        self.graph = self.graph_k = None

    def _prepare(self, sizes):
        m = self.model
        if m.item_embedding.weight.device != self.ranks.device:
            raise ValueError("the model lives on another device than the validation store")
        if m.use_laplacian_pe and m.laplacian_pe._cached_pe is None:
            raise RuntimeError("Laplacian PE not precomputed. Call precompute() first.")
        m._sync_lazy()
        eng = m.hip_engine()  # a fresh engine if the parameters were re-allocated
        eng.check_intact()
        full = sum(1 for b in sizes if b == self.B)
        extra = [(self.loader.batch_start(i), b) for i, b in enumerate(sizes) if b != self.B]
        need = self.builder.plan_caps(max(full, 1), self.loader.batch_start(0), extra)
        if self.caps is None or getattr(self, "eng", None) is not eng:
            self._bind(eng, need)
        elif not self.caps.fits(need.n_cap, need.b_cap, need.e_cap, need.n_neg):
            self._bind(eng, self.caps.grow(need.n_cap, need.b_cap, need.e_cap, need.n_neg))
        sig = self._signature(eng)
        if sig != self._sig:  # parameters, table or PE rows moved: the captured addresses are stale
            self.graph = self.graph_k = None
            self.ws.refresh_params(eng)
            self._sig = sig
        return full

    # ------------------------------------------------------------------ launches
    def _chain(self, B: int | None = None):
        """build -> eval forward -> target rank of the builder's next batch, on the current stream."""
        eng, ws, bs = self.eng, self.ws, self.bs
        B = self.B if B is None else int(B)
        st = eng.stream()
        self.builder.launch(bs, self.caps, st, B)
        eng.run_forward(ws, self.cfg, bs, L.RO_FWD)
        L.check(L.lib().gtr_target_rank(ws.se.data_ptr(), B, eng.D, self.model.item_embedding.weight.data_ptr(),
                                        eng.T, bs.target, self.ranks.data_ptr(), self.S,
                                        self.builder.start.data_ptr(), self.base.data_ptr(),
                                        self.rank_ws.data_ptr(), self.rank_ws.numel(), st), "target_rank")

    def _capture(self, n: int = 1):
        """n consecutive chains as one hipGraph."""
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        pos = self.builder.pos  # the captured builds do not run: the host mirror stays put
        with torch.cuda.graph(g, stream=s):
            for _ in range(n):
                self._chain()
        self.builder.pos = pos
        torch.cuda.current_stream(self.dev).wait_stream(s)
        self.captures += 1
        return g

    # ------------------------------------------------------------------ epochs
    @torch.no_grad()
    def run(self) -> torch.Tensor:
        """One validation epoch: the ``S`` target ranks in session order (int32, host)."""
        if self.model.training:
            raise RuntimeError("DeviceEvaluator requires model.eval()")
        loader = self.loader
        loader.start_epoch()  # consumes the global CPU generator exactly as iterating the loader does
        sizes = loader.batch_sizes()
        full = self._prepare(sizes)
        self.base.fill_(loader.batch_start(0))
        self.ranks[: self.S].fill_(-1)
        done = 0
        if full > 0:
            self._chain()  # first full batch: eager (first touch of every code path)
            done = 1
        if self.use_graph:
            K = self.K
            while K > 1 and full - done >= K:
                if self.graph_k is None:
                    self.graph_k = self._capture(K)
                self.graph_k.replay()
                self.builder.pos += K * self.builder.stride
                done += K
            for _ in range(done, full):
                if self.graph is None:
                    self.graph = self._capture()
                self.graph.replay()
                self.builder.pos += self.builder.stride
        else:
            for _ in range(done, full):
                self._chain()
        for j, b in enumerate(sizes):
            if b != self.B:  # last, partial batch
                self.builder.seek(loader.batch_start(j))
                self._chain(b)
        self.builder.check_status()
        out = self.ranks.cpu()
        if bool((out[self.S:] != -1).any()):
            raise RuntimeError("DeviceEvaluator: a rank was written past the validation set")
        out = out[: self.S]
        if bool((out < 0).any()):
            raise RuntimeError("DeviceEvaluator: a session of the validation set was not ranked")
        return out

    def evaluate(self, k_values) -> dict:
        from etpgt.utils.metrics import compute_metrics_from_ranks

        return compute_metrics_from_ranks(self.run(), k_values)

    def close(self):
        """Drop the captured graphs (the evaluator stays usable: the next epoch captures again)."""
        self.graph = self.graph_k = None
