"""gtr_target_rank on the GPU: the target's position in gtr_score_topk's full ordering
(score descending, item id ascending on ties) by one scan of the table.

Exactness: inputs of the reference test are integer-valued floats in [-3, 3], so every dot
product (|sum| <= 9 * 256 = 2304) is exact in fp32 in any summation order and the numpy
count is THE answer, ties included.  Against the top-k kernel the comparison is exact too:
both kernels form the same keys from the same MFMA chain.
"""

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only on the GPU box
    pytest.skip("no GPU", allow_module_level=True)

from etpgt.backend import _lib as L  # noqa: E402
from etpgt.backend.ops import score_topk, target_rank  # noqa: E402


def _int_inputs(B, T, D, seed):
    rng = np.random.default_rng(seed)
    se = rng.integers(-3, 4, size=(B, D)).astype(np.float32)
    table = rng.integers(-3, 4, size=(T, D)).astype(np.float32)
    # duplicate rows: exact ties between different ids whatever the session
    if T >= 8:
        table[T // 2] = table[1]
        table[T - 1] = table[1]
    return se, table, rng


def _np_rank(se, table, targets):
    S = se.astype(np.int64) @ table.astype(np.int64).T
    T = table.shape[0]
    j = np.arange(T)
    out = np.empty(len(targets), np.int64)
    for b, t in enumerate(targets):
        if not 0 <= t < T:
            out[b] = T
            continue
        s_t = S[b, t]
        out[b] = (S[b] > s_t).sum() + ((S[b] == s_t) & (j < t)).sum()
    return out


def _targets(B, T, rng):
    """0, T-1, a duplicate across sessions, -1 and T first; random ids after."""
    special = [0, T - 1, T - 1, -1, T, 1, T // 2]
    t = rng.integers(0, T, size=B)
    n = min(B, len(special))
    t[:n] = special[:n]
    return t


@pytest.mark.parametrize("D", [32, 64, 128, 256])
@pytest.mark.parametrize("T", [16, 255, 256, 257, 4099])
def test_rank_equals_the_exact_count_with_ties(D, T):
    """16-row tile edge, 256-row chunk edge, several chunks and session groups."""
    for B in (1, 15, 16, 17, 65):
        se, table, rng = _int_inputs(B, T, D, seed=D * 31 + T * 7 + B)
        se_d, tab_d = torch.from_numpy(se).cuda(), torch.from_numpy(table).cuda()
        cases = [_targets(B, T, rng)] if B > 1 else [np.array([v]) for v in (0, T - 1, -1, T, T // 2)]
        for tg in cases:
            got = target_rank(se_d, tab_d, torch.from_numpy(tg).cuda())
            assert got.dtype == torch.int32 and tuple(got.shape) == (B,)
            want = _np_rank(se, table, tg)
            assert got.cpu().numpy().tolist() == want.tolist(), (B, T, D, tg.tolist())


@pytest.mark.parametrize("B,T,D", [(70, 82174, 64), (33, 1000, 128)])
def test_rank_agrees_with_the_topk_kernel(B, T, D):
    """rank < 128 iff the target is in score_topk's 128 ids, and then it sits in column
    ``rank``: exact, gaussian inputs (no tolerance -- same keys in both kernels)."""
    g = torch.Generator().manual_seed(B + D)
    se = torch.randn(B, D, generator=g).cuda()
    table = (torch.randn(T, D, generator=g) * 0.1).cuda()
    idx = score_topk(se, table, 128)[0]
    tg = torch.randint(0, T, (B,), generator=g)
    cols = torch.randint(0, 128, (B,), generator=g)
    pick = torch.arange(B) % 3 != 2  # two thirds of the targets taken from the top-k lists
    tg = torch.where(pick, idx.cpu()[torch.arange(B), cols], tg)
    tg[0] = idx[0, 0].item()
    tg[1] = idx[1, 127].item()
    rank = target_rank(se, table, tg.cuda()).cpu()
    idx = idx.cpu()
    n_in = 0
    for b in range(B):
        inside = bool((idx[b] == tg[b]).any())
        assert (int(rank[b]) < 128) == inside, b
        if inside:
            n_in += 1
            assert int(idx[b, int(rank[b])]) == int(tg[b]), b
        else:
            assert 128 <= int(rank[b]) < T
    assert n_in >= B // 2 and int(rank[0]) == 0 and int(rank[1]) == 127
    # two calls are equal bit for bit (integer adds: order-independent)
    assert torch.equal(rank, target_rank(se, table, tg.cuda()).cpu())


def _raw_rank(se, table, tg, buf, cap, pos, base):
    lib = L.lib()
    B, D = se.shape
    nb = C.c_size_t(0)
    L.check(lib.gtr_target_rank_workspace_bytes(B, table.shape[0], C.byref(nb)), "ws")
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.gtr_target_rank(se.data_ptr(), B, D, table.data_ptr(), table.shape[0], tg.data_ptr(), buf.data_ptr(),
                                cap, L.ptr(pos), L.ptr(base), ws.data_ptr(), ws.numel(), st), "target_rank")
    torch.cuda.synchronize()


def test_rank_write_offset_and_cap():
    """rank[*pos - *base + b], indices outside [0, rank_cap) dropped, nothing else touched."""
    B, T, D, cap = 17, 300, 64, 20
    g = torch.Generator().manual_seed(9)
    se = torch.randn(B, D, generator=g).cuda()
    table = torch.randn(T, D, generator=g).cuda()
    tg = torch.randint(0, T, (B,), generator=g).to(torch.int32).cuda()
    want = target_rank(se, table, tg).cpu()
    buf = torch.full((cap + 32,), -7, dtype=torch.int32, device="cuda")
    pos = torch.tensor([1000], dtype=torch.int64).cuda()
    base = torch.tensor([992], dtype=torch.int64).cuda()
    _raw_rank(se, table, tg, buf, cap, pos, base)
    out = buf.cpu()
    assert out[:8].tolist() == [-7] * 8
    assert out[8:20].tolist() == want[:12].tolist()  # sessions 12..16 fall past the cap
    assert out[20:].tolist() == [-7] * 32
    # a batch that starts before the base: its first sessions are dropped instead
    buf.fill_(-7)
    pos.fill_(990)
    _raw_rank(se, table, tg, buf, cap, pos, base)
    out = buf.cpu()
    assert out[:15].tolist() == want[2:].tolist() and out[15:].tolist() == [-7] * 37
    # no offset words: rank[b]
    buf.fill_(-7)
    _raw_rank(se, table, tg, buf, cap, None, None)
    out = buf.cpu()
    assert out[:17].tolist() == want.tolist() and out[17:].tolist() == [-7] * 35


def test_rank_errors():
    se = torch.randn(4, 64, device="cuda")
    tg = torch.tensor([1, 2, 3, 4], device="cuda")
    with pytest.raises(ValueError):
        target_rank(se, torch.randn(100, 32, device="cuda"), tg)
    with pytest.raises(ValueError):
        target_rank(se, torch.randn(100, 64, device="cuda"), tg[:3])
    with pytest.raises(RuntimeError, match="dim 48"):
        target_rank(torch.randn(4, 48, device="cuda"), torch.randn(100, 48, device="cuda"), tg)
    assert target_rank(se[:0], torch.randn(100, 64, device="cuda"), tg[:0]).shape == (0,)


def test_model_rank_targets_past_k_128():
    """rank_targets == the column of predict; ranks in (128, T] -- a k the top-k kernel
    refuses -- are plain numbers here."""
    from etpgt.model import create_graph_transformer_optimized

    torch.manual_seed(4)
    m = create_graph_transformer_optimized(500, embedding_dim=32, hidden_dim=32, num_layers=1, num_heads=2,
                                           dropout=0.0, use_laplacian_pe=False).cuda().eval()
    se = torch.randn(40, 32, device="cuda")
    p = m.predict(se, k=128)
    tg = p[:, 100].clone()
    assert m.rank_targets(se, tg).tolist() == [100] * 40
    # integer-valued table and sessions: exact scores, so the stable descending sort (id
    # ascending on ties) is the kernel's order and column 300 has rank 300 exactly
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        m.item_embedding.weight.copy_(torch.randint(-3, 4, (500, 32), generator=g).float())
    se = torch.randint(-3, 4, (40, 32), generator=g).float().cuda()
    full = torch.argsort(se.double() @ m.item_embedding.weight.detach().double().t(), dim=1, descending=True,
                         stable=True)
    assert m.rank_targets(se, full[:, 300]).tolist() == [300] * 40


def test_target_rank_op_passes_opcheck():
    g = torch.Generator().manual_seed(5)
    se = torch.randn(8, 64, generator=g).cuda()
    tab = torch.randn(300, 64, generator=g).cuda()
    t = torch.randint(0, 300, (8,), generator=g).cuda()
    torch.library.opcheck(torch.ops.etpgt.target_rank.default, (se, tab, t),
                          test_utils=("test_schema", "test_faketensor"))
