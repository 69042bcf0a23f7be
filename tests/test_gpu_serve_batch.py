"""Batched serving (Recommender.recommend_batch): the request graphs built on the device
(gtr_serve_counts + gtr_serve_build, etpgt.data.gpu_batch.GpuRequestBuilder) against the
host's _build_session_graph word for word, and the batched results against the oracle and
against the single-request route.

The edge file is the synthetic graph (rows item_i <= item_j, self-loops among them) plus
hand-written rows: a pair stored in both orientations, a pair stored only as (larger,
smaller), a self-loop row, and edges touching item 0 in either direction.

Bars (the serving bars of test_gpu_eval.test_recommender_matches_oracle, unchanged): ids
equal unless the gap at the k-th boundary is <= 1e-4 of the largest score, no excluded id
returned, scores within rtol 1e-3 / atol 1e-5.  The image and the exclusion lists are
integer work: bit-exact.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only on the GPU box
    pytest.skip("no GPU", allow_module_level=True)

import etpgt_ref as R  # noqa: E402
from gpu_helpers import make_pair, small_data  # noqa: E402

from etpgt.data.batch import Caps, SessionBatch, blob_layout  # noqa: E402
from etpgt.data.gpu_batch import GpuRequestBuilder, GpuServingGraph  # noqa: E402
from etpgt.serving import Recommender, ValidatedRequest  # noqa: E402

BOTH = (7, 9)          # stored as (7, 9) and (9, 7)
REVERSED = (257, 211)  # stored only as (larger, smaller)
LOOP = 5               # stored as (5, 5)
ZERO_OUT, ZERO_IN = 12, 13  # stored as (0, 12) and (13, 0)
SPECIAL_ROWS = [BOTH, BOTH[::-1], REVERSED, (LOOP, LOOP), (0, ZERO_OUT), (ZERO_IN, 0)]


class Served:
    """Recommender + oracle on small_data(), built once for the module."""

    def __init__(self, tmp):
        import pandas as pd

        self.data = data = small_data()
        self.T = T = data.table_rows
        self.m, self.ref = make_pair(T, 64, 2, K=8, seed=23)
        torch.save({"epoch": 3, "model_state_dict": self.m.state_dict(), "best_val_metric": 0.25}, tmp / "ck.pt")
        ei = data.edge_index()
        stored = set(zip(ei[0].tolist(), ei[1].tolist()))
        assert REVERSED not in stored and REVERSED[::-1] not in stored  # only the hand-written orientation
        rows = list(zip(ei[0].tolist(), ei[1].tolist())) + SPECIAL_ROWS
        self.rows = rows
        pd.DataFrame({"item_i": [r[0] for r in rows], "item_j": [r[1] for r in rows]}).to_csv(tmp / "edges.csv",
                                                                                            index=False)
        self.rec = Recommender(tmp / "ck.pt", tmp / "edges.csv", device="cuda")
        self.ref.laplacian_pe._cached_pe = self.m.laplacian_pe._cached_pe.detach().cpu().clone()
        self.ref.eval()
        self.adj = {}
        for i, j in rows:
            if i != j:
                self.adj.setdefault(i, set()).add(j)
        # a pair with no stored row in either orientation
        self.apart = next([a, b] for a in range(20, 60) for b in range(a + 1, 60)
                          if b not in self.adj.get(a, ()) and a not in self.adj.get(b, ()))
        self._oracle = {}

    def special_requests(self):
        return [
            [int(self.data.session(0)[0])],                  # one item: one node, no edge
            [17] * 6,                                        # one id repeated
            list(range(163, 99, -1)),                        # 64 distinct ids
            [ZERO_IN, 0, 40, ZERO_OUT],                      # item 0 and both of its edges
            self.apart,                                      # no induced edge
            [BOTH[1], 3, BOTH[0]],                           # a pair stored in both orientations
            [REVERSED[1], REVERSED[0]],                      # stored only as (larger, smaller)
            [LOOP, 6, LOOP],                                 # the self-loop row
        ]

    def oracle_scores(self, items):
        """Masked fp64 scores of the oracle forward (test_recommender_matches_oracle), once per session."""
        key = tuple(items)
        if key not in self._oracle:
            seen = set(items)
            uniq = sorted(seen)
            loc = {g: q for q, g in enumerate(uniq)}
            pairs = sorted((i, j) for i in seen for j in self.adj.get(i, ()) if j in seen)
            e = torch.tensor([[loc[i], loc[j]] for i, j in pairs], dtype=torch.long).t() if pairs else \
                torch.zeros((2, 0), dtype=torch.long)
            rb = R.RefBatch(torch.tensor(uniq), e, torch.zeros(len(uniq), dtype=torch.long))
            with torch.no_grad():
                se = self.ref(rb)
            sc = (se.double() @ self.ref.item_embedding.weight.detach().double().t()).squeeze(0)
            sc[list(seen)] = -float("inf")
            sc[0] = -float("inf")
            self._oracle[key] = sc
        return self._oracle[key]


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    return Served(tmp_path_factory.mktemp("serve"))


def _mixed_requests(served):
    sessions = served.special_requests()[2:8] + [served.data.session(s).tolist() for s in range(0, 102, 17)]
    ks = [10, 5, 20, 10, 1, 7, 10, 20, 5, 10, 3, 10]
    assert len(sessions) == len(ks) == 12
    return [ValidatedRequest(it, k) for it, k in zip(sessions, ks)]


def _boundary_is_a_near_tie(served, items, k):
    top = torch.topk(served.oracle_scores(items), k + 1)
    return float(top.values[k - 1] - top.values[k]) <= 1e-4 * float(top.values.abs().max())


def _host_image(rec, requests, caps, dev):
    xs, eis, bv, off = [], [], [], 0
    for b, items in enumerate(requests):
        sb = rec._build_session_graph(items)
        xs.append(sb.x)
        eis.append(sb.edge_index + off)
        bv.append(torch.full((sb.x.shape[0],), b, dtype=torch.long))
        off += int(sb.x.shape[0])
    sb = SessionBatch(torch.cat(xs), torch.cat(eis, dim=1), torch.cat(bv), num_graphs=len(requests))
    return sb.device_blob(dev, caps)[1]


@pytest.mark.parametrize("B", [1, 3, 5, 300])
def test_device_image_equals_host_image(served, B):
    """B = 1, 3: fewer requests than waves in a workgroup; 5: a partial last workgroup; 300:
    more than 256, every special request and sessions of the synthetic store."""
    sp = served.special_requests()
    if B == 1:
        requests = [sp[2]]
    elif B == 3:
        requests = sp[:3]
    elif B == 5:
        requests = sp[3:8]
    else:
        requests = sp + [served.data.session(s).tolist() for s in range(B - len(sp))]
    assert len(requests) == B
    bld = served.rec._request_builder
    got = bld.build(requests)
    caps = got.batch.caps
    want = _host_image(served.rec, requests, caps, served.rec.device)
    g, w = got.batch.blob.cpu().numpy(), want.cpu().numpy()
    assert g.shape == w.shape
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[:5]} (layout {blob_layout(caps)})"
    excl = [sorted(set(r) | {0}) for r in requests]
    ptr = np.cumsum([0] + [len(e) for e in excl])
    assert got.excl_ptr.cpu().tolist() == ptr.tolist()
    assert got.excl_ids[: ptr[-1]].cpu().tolist() == [v for e in excl for v in e]
    assert got.num_nodes == sum(len(set(r)) for r in requests)
    if B == 300:  # the special rows are in the image: 7 <-> 9, 257 -> 211, 0 -> 12, 13 -> 0, no 5 -> 5
        assert got.num_edges == int(g[2])
        for items, e in ((sp[6], 1), (sp[4], 0), (sp[0], 0), (sp[1], 0)):
            assert bld.build([items]).num_edges == e, items
        assert bld.build([sp[5]]).num_edges >= 2 and bld.build([sp[3]]).num_edges >= 2


def test_batched_results_match_oracle(served):
    reqs = _mixed_requests(served)
    out = served.rec.recommend_batch(reqs)
    assert len(out) == len(reqs)
    for r, (ids, scores) in zip(reqs, out):
        seen = set(r.session_items)
        sc = served.oracle_scores(r.session_items)
        assert len(ids) == len(scores) == r.k
        if ids != torch.topk(sc, r.k).indices.tolist():  # only a near-tie at the boundary may differ
            assert _boundary_is_a_near_tie(served, r.session_items, r.k)
        assert not set(ids) & (seen | {0})
        np.testing.assert_allclose(scores, sc[ids].numpy(), rtol=1e-3, atol=1e-5)


def test_batched_results_agree_with_recommend(served):
    reqs = _mixed_requests(served)
    batched = served.rec.recommend_batch(reqs)
    worst = 0.0
    for r, (ids, scores) in zip(reqs, batched):
        ids1, scores1 = served.rec.recommend(r)
        diff = float(np.max(np.abs(np.asarray(scores) - np.asarray(scores1))))
        worst = max(worst, diff)
        if ids != ids1:
            assert _boundary_is_a_near_tie(served, r.session_items, r.k), (r.session_items, ids, ids1)
        np.testing.assert_allclose(scores, scores1, rtol=1e-3, atol=1e-5,
                                   err_msg=f"max |score difference| between the routes {diff:.3g}")
    print(f"recommend_batch vs recommend: max |score difference| {worst:.3g}")


def test_k_past_the_unmasked_items(tmp_path):
    import pandas as pd

    T = 12
    m, _ = make_pair(T, 32, 2, K=4, seed=24)
    torch.save({"epoch": 0, "model_state_dict": m.state_dict()}, tmp_path / "ck.pt")
    pd.DataFrame({"item_i": [1, 2, 3, 5], "item_j": [2, 3, 5, 5]}).to_csv(tmp_path / "edges.csv", index=False)
    rec = Recommender(tmp_path / "ck.pt", tmp_path / "edges.csv", device="cuda")
    reqs = [ValidatedRequest([3, 1, 5, 2], T - 1), ValidatedRequest([4], 3), ValidatedRequest([0, 7, 7], T)]
    out = rec.recommend_batch(reqs)
    for r, (ids, scores) in zip(reqs, out):
        excl = sorted(set(r.session_items) | {0})
        live = min(r.k, T - len(excl))
        assert len(ids) == len(scores) == r.k and len(set(ids)) == r.k
        assert all(np.isfinite(scores[:live])) and scores[:live] == sorted(scores[:live], reverse=True)
        assert not set(ids[:live]) & set(excl)
        assert ids[live:] == excl[: r.k - live]
        assert all(s == float("-inf") for s in scores[live:])
    assert set(out[0][0][: T - 5]) == set(range(T)) - {0, 1, 2, 3, 5}
    with pytest.raises(RuntimeError, match="out of range"):
        rec.recommend_batch([ValidatedRequest([1], T + 1)])


def test_over_capacity_is_reported_not_written(served):
    """Capacities one bucket too small for E: the status word raises, the header is empty
    and nothing lands after the image.  (The status path; no fault is provoked.)"""
    sp = served.special_requests()
    requests = [sp[2], sp[3], sp[5]]
    bld = GpuRequestBuilder(GpuServingGraph([r[0] for r in served.rows], [r[1] for r in served.rows], served.T,
                                            "cuda"))
    ok = bld.build(requests)
    N, E = ok.num_nodes, ok.num_edges
    ok_words = ok.batch.blob.clone()  # the cached image is reused by the next build
    fit = Caps.bucket(N, len(requests), E, 0)
    assert ok.batch.caps == fit and E > 16
    x = E - 1
    while Caps.bucket(1, 1, x, 0).e_cap >= E:
        x -= 1
    small = Caps(fit.n_cap, fit.b_cap, Caps.bucket(1, 1, x, 0).e_cap, 0)
    total = blob_layout(small)["_total"]
    guarded = torch.full((total + 4096,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    guarded[:total].zero_()
    with pytest.raises(RuntimeError, match="GPU batch exceeded its capacities"):
        bld.build(requests, caps=small, blob=guarded[:total])
    assert bool((guarded[total:] == 0x5A5A5A5A).all())
    assert guarded[:5].tolist() == [0, 0, 0, 0, 0]  # N, B, E, n_neg, G of an empty header
    again = bld.build(requests)  # the status was cleared; the same requests build at their own capacities
    assert torch.equal(again.batch.blob, ok_words) and again.num_edges == E


def test_request_order_permutes_the_results(served):
    reqs = _mixed_requests(served)
    base = served.rec.recommend_batch(reqs)
    perm = np.random.default_rng(0).permutation(len(reqs)).tolist()
    out = served.rec.recommend_batch([reqs[p] for p in perm])
    for q, p in enumerate(perm):
        if out[q][0] != base[p][0]:  # a session's rows land in another row group: last-bit score changes
            assert _boundary_is_a_near_tie(served, reqs[p].session_items, reqs[p].k)
        np.testing.assert_allclose(out[q][1], base[p][1], rtol=1e-3, atol=1e-5)


def test_lists_over_the_builder_maximum_are_split(served, monkeypatch):
    """The builder takes 16,384 requests a build; a longer list is served in pieces.  The
    maximum is lowered to 5 here so that 12 requests take three builds (the last partial)."""
    import etpgt.serving.recommender as mod

    reqs = _mixed_requests(served)
    base = served.rec.recommend_batch(reqs)
    monkeypatch.setattr(mod, "MAX_REQUESTS", 5)
    out = served.rec.recommend_batch(reqs)
    assert len(out) == len(reqs)
    for r, (ids, scores), (ids0, scores0) in zip(reqs, out, base):
        if ids != ids0:
            assert _boundary_is_a_near_tie(served, r.session_items, r.k)
        np.testing.assert_allclose(scores, scores0, rtol=1e-3, atol=1e-5)


def test_batch_front_door_errors(served):
    rec = served.rec
    assert rec.recommend_batch([]) == []
    with pytest.raises(ValueError, match="session_items must not be empty"):
        rec.recommend_batch([ValidatedRequest([1, 2], 5), ValidatedRequest([], 5)])
    with pytest.raises(ValueError, match="64"):
        rec.recommend_batch([ValidatedRequest(list(range(1, 66)), 5)])
    with pytest.raises(IndexError):
        rec.recommend_batch([ValidatedRequest([1, served.T], 5)])
    with pytest.raises(IndexError):
        rec.recommend(ValidatedRequest([1, served.T], 5))
