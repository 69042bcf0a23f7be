"""GPU parity at the model shapes the library accepts beyond heads 1 / 2 / 4, LapPE widths
0 / 4 / 8 / 16 and 2-3 layers: the HIP path against the CPU oracle.

check_dims (csrc/gtr_fwd.hip) accepts dim 32 / 64 / 128 / 256, any power-of-two head width
C = dim / heads >= max(1, dim / 64), pe_k 0..256 and any layer count; the kernels switch code
paths on exactly these parameters (fast-path predicate, float4 against wave-per-row attention
kernels, one-lane head groups, three LapPE projection loops, the weight-gradient job table).
The bit-for-bit tests of the other modules compare one HIP path with another at the same
shapes; here every shape is held to the oracle.

Tolerances are those of test_gpu_parity: 1e-3 (gpu_helpers.assert_close), gradients 2e-3 with
a floor of 1e-6 of the largest gradient entry, trained parameters elementwise through
gpu_helpers.close_trained with FALLBACK_FRAC unchanged.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - collected only on the GPU box
    pytest.skip("no GPU", allow_module_level=True)

import etpgt_ref as R  # noqa: E402
from gpu_helpers import (batches, capacity_batch, edge_case_batch, eval_vs_oracle, fused_vs_trio,  # noqa: E402
                         grads_vs_oracle, group0_geometry, long_session_batch, make_pair, small_data)

from etpgt.backend import _lib as L  # noqa: E402
from etpgt.backend.engine import split_default  # noqa: E402
from etpgt.train.fused import FusedTrainStep  # noqa: E402

DATA = None
_INPUTS = {}


def data():
    global DATA
    if DATA is None:
        DATA = small_data()
    return DATA


def eval_inputs():
    """Two random batches (B = 32) and the edge cases, built once and never modified."""
    if "eval" not in _INPUTS:
        T = data().table_rows
        _INPUTS["eval"] = batches(data(), 32, 5, 2, seed=31) + [edge_case_batch(5, T)]
    return _INPUTS["eval"]


def train_inputs(n=5):
    """The single train-mode step's three inputs: a random batch (B = 32, ``n`` negatives),
    the edge cases and the long sessions (groups past the LDS carve)."""
    key = ("train", n)
    if key not in _INPUTS:
        T = data().table_rows
        _INPUTS[key] = [("random ", batches(data(), 32, n, 1, seed=37)[0]), ("edge ", edge_case_batch(5, T)),
                        ("long ", long_session_batch(5, T))]
    return _INPUTS[key]


def with_splits(shapes):
    """Every shape under GTR_SPLIT=0 and, where the split layer path exists (D 64 / 128),
    under GTR_SPLIT=1."""
    return [s + (sp,) for s in shapes for sp in (("0", "1") if s[0] in (64, 128) else ("0",))]


def set_split(monkeypatch, D, split):
    monkeypatch.setenv("GTR_SPLIT", split)
    assert split_default(D, 1) == (split == "1")


def train_step(m, ref, loss="model_bpr", n=5):
    for name, sb in train_inputs(n):
        grads_vs_oracle(m, ref, sb, loss=loss, name=name)


# ---- 1. heads ------------------------------------------------------------------------------
# (D, H): C = 4 and C = 1 at D = 32; H = 8 the fast path's last head count (and the first
# where edges * H <= EH binds before edges <= EMAX); (64, 16): C = 4 < CH = 8, the general
# path for every group; C = 1; (128, 64) and (256, 64): C == VPL, one-lane head groups in
# the wave-per-row attention; H > 8 leaves the float4 attention kernels of the split path
HEADS = [(32, 8), (32, 32), (64, 8), (64, 16), (64, 64), (128, 8), (128, 16), (128, 64), (256, 8), (256, 64)]


@pytest.mark.parametrize("D,H,split", with_splits(HEADS))
def test_heads_forward_eval(D, H, split, monkeypatch):
    set_split(monkeypatch, D, split)
    m, ref = make_pair(data().table_rows, D, H, seed=1)
    eval_vs_oracle(m, ref, eval_inputs(), name=f"se D={D} H={H}")


@pytest.mark.parametrize("D,H,split", with_splits(HEADS))
def test_heads_train_step(D, H, split, monkeypatch):
    """BPR, dropout 0: loss, session embeddings, every gradient, running statistics."""
    set_split(monkeypatch, D, split)
    m, ref = make_pair(data().table_rows, D, H, seed=2)
    train_step(m, ref)


@pytest.mark.parametrize("D,H,split", with_splits([(64, 8), (64, 16), (128, 64)]))
def test_heads_train_step_lappe_listwise(D, H, split, monkeypatch):
    """The same with a LapPE table (K = 8) and the listwise loss (20 negatives)."""
    set_split(monkeypatch, D, split)
    m, ref = make_pair(data().table_rows, D, H, K=8, seed=3)
    train_step(m, ref, loss="listwise", n=20)


@pytest.mark.parametrize("D,H", [(64, 8), (64, 16), (32, 32), (128, 64)])
def test_heads_fused_steps(D, H):
    """Three fused steps (graph replay, AdamW) against OracleTrio; B = 32 runs the fused
    layer kernels and ends the step in one launch."""
    fused = fused_vs_trio(data(), D, H)
    assert not fused.ws.split and fused.step_end


@pytest.mark.parametrize("D,H,split", with_splits([(64, 8), (64, 16)]))
def test_heads_dropout_values_with_hip_masks(D, H, split, monkeypatch):
    """Dropout 0.1 value for value: the oracle applies the HIP stream's own masks (attention
    element index (edge * H + head)); two steps, so the stream counter advances."""
    set_split(monkeypatch, D, split)
    p = 0.1
    m, ref = make_pair(data().table_rows, D, H, dropout=p, seed=7)
    eng = m.hip_engine()
    for step, sb in enumerate(batches(data(), 32, 5, 2, seed=19)):
        ctr = int(eng.rng_ctr.item())
        assert ctr == step
        masks = R.hip_dropout_masks(eng.seed, ctr, p, 2, sb.edge_index.numpy(), sb.num_nodes, D, H)
        assert 0.0 < float((masks["attn"][0] == 0).float().mean()) < 2 * p
        grads_vs_oracle(m, ref, sb, masks=masks, name=f"step {step} ")


# ---- 2. row groups at exactly the capacities of the LDS carve -------------------------------
# csrc/gtr_layer.cuh (LayerGeom): RMAX rows, EMAX edges and EH (edge, head) pairs of a row
# group are staged in LDS; the arrays are sized to exactly these counts and the fast-path
# predicate is rows <= RMAX && edges <= EMAX && edges * H <= EH (&& H <= 8 && C >= CH)
RMAX = {32: 64, 64: 64, 128: 32}
EMAX = 1024
EH = 4096

BOUNDARIES = [
    # D, H, nodes, edges, on the fast path
    (64, 2, 64, 192, True),      # rows == RMAX
    (64, 2, 65, 195, False),     # rows == RMAX + 1
    (128, 4, 32, 96, True),
    (128, 4, 33, 99, False),
    (64, 2, 32, 1024, True),     # edges == EMAX: 32 nodes x 32 in-edges
    (64, 2, 33, 1025, False),    # EMAX + 1
    (64, 8, 32, 512, True),      # edges * H == EH: 32 nodes x 16 in-edges
    (64, 8, 32, 513, False),     # EH / H + 1
]


@pytest.mark.parametrize("D,H,n,e,fast", BOUNDARIES)
def test_group_at_carve_capacity(D, H, n, e, fast, monkeypatch):
    monkeypatch.setenv("GTR_SPLIT", "0")  # the fused layer kernels own this predicate
    T = data().table_rows
    sb = capacity_batch(n, e, 5, T)
    # the geometry the kernels will see, from the packed image: group 0 is session 0 alone
    assert group0_geometry(sb) == (n, e)
    assert (n <= RMAX[D] and e <= EMAX and e * H <= EH) == fast
    m, ref = make_pair(T, D, H, seed=5)
    grads_vs_oracle(m, ref, sb)


# ---- 3. LapPE width -------------------------------------------------------------------------
# pe_k <= 16 (projection weight in LDS), pe_k % 4 == 0 past it (float4 loop), else the scalar
# loop -- in k_conv_fwd and again in k_proj (split path); the PE weight-gradient job's tiles
# cover (K + 1 + 63) / 64 columns, the bias riding as a ones column (second tile at K = 64);
# the narrow MFMA tile holds K + 1 <= 32
LAPPE = ([(64, 2, K) for K in (1, 3, 6, 12, 17, 20, 31, 32, 63, 64)] + [(32, 2, K) for K in (3, 20, 64)]
         + [(128, 4, K) for K in (3, 31, 32)])


@pytest.mark.parametrize("D,H,K,split", with_splits(LAPPE))
def test_lappe_forward_eval(D, H, K, split, monkeypatch):
    set_split(monkeypatch, D, split)
    m, ref = make_pair(data().table_rows, D, H, K=K, seed=1)
    eval_vs_oracle(m, ref, eval_inputs(), name=f"se D={D} K={K}")


@pytest.mark.parametrize("D,H,K,split", with_splits(LAPPE))
def test_lappe_train_step(D, H, K, split, monkeypatch):
    """laplacian_pe.projection.{weight,bias} gradients among every parameter's."""
    set_split(monkeypatch, D, split)
    m, ref = make_pair(data().table_rows, D, H, K=K, seed=2)
    assert {"laplacian_pe.projection.weight", "laplacian_pe.projection.bias"} <= set(dict(ref.named_parameters()))
    train_step(m, ref)


@pytest.mark.parametrize("K", [3, 20, 32])
def test_lappe_fused_steps(K):
    """gtr_step_end_small_fits refuses pe_k % 4 != 0: K = 3 ends the step with the pair of
    launches, K = 20 and 32 with the one launch."""
    fused = fused_vs_trio(data(), 64, 2, K=K)
    assert not fused.ws.split
    assert fused.step_end == (K % 4 == 0)


@pytest.mark.parametrize("K", [31, 32])
def test_lappe_fused_steps_mfma_tiles(K, monkeypatch):
    """GTR_WGRAD=mfma: the narrow MFMA PE tile at K + 1 == 32 and the fallback from it at
    K + 1 == 33 (forced MFMA tiles end the step with the pair of launches)."""
    monkeypatch.setenv("GTR_WGRAD", "mfma")
    fused = fused_vs_trio(data(), 64, 2, K=K)
    assert not fused.ws.split and not fused.step_end


# ---- 4. layer count -------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 5])
def test_layers_train_step(layers):
    """L = 1: the first layer is also the last (no previous BatchNorm, dx0 from the same
    launch); L = 5: 3 * 5 + 1 = 16 jobs fill the weight-gradient job table exactly."""
    assert 3 * L.MAX_TRAIN_LAYERS + 1 == L.MAX_WJOBS and L.MAX_TRAIN_LAYERS == 5
    m, ref = make_pair(data().table_rows, 64, 2, L=layers, K=8, seed=2)
    train_step(m, ref)


@pytest.mark.parametrize("D,H,K,layers", [(64, 2, 8, 1), (64, 2, 8, 5), (32, 2, 0, 4)])
def test_layers_fused_steps(D, H, K, layers):
    """The default end of step: one launch while the chain's 2L + 1 launches carry the
    untouched-row sweep (L <= 3), the pair of launches past that.  (32, 2, L = 4): no
    column-sum jobs, another job count."""
    fused = fused_vs_trio(data(), D, H, K=K, L=layers)
    assert not fused.ws.split
    assert fused.step_end == (2 * layers + 1 <= L.SWEEP_SLOTS)


# ---- 5. refusals ----------------------------------------------------------------------------
@pytest.mark.parametrize("D,H", [(128, 128), (256, 128)])
def test_refused_head_width_raises_and_leaves_the_process_usable(D, H):
    """C = D / H below the lane width of a row (D / 64): an argument check of the library
    (status code, nothing launched), through model(batch) and through the fused step; a
    supported model built afterwards compares as usual."""
    T = data().table_rows
    sb = eval_inputs()[0]
    m, _ = make_pair(T, D, H, seed=1)
    m.eval()
    with pytest.raises(RuntimeError, match="head dim . unsupported"):
        with torch.no_grad():
            m(sb.to("cuda"))
    m.train()
    with pytest.raises(RuntimeError, match="head dim . unsupported"):
        m(sb.to("cuda"))
    fused = FusedTrainStep(m, loss="bpr")
    with pytest.raises(RuntimeError, match="head dim . unsupported"):
        fused(sb.to("cuda"))
    torch.cuda.synchronize()
    m2, ref2 = make_pair(T, D, 4, seed=1)
    eval_vs_oracle(m2, ref2, eval_inputs(), name=f"se D={D} H=4 after the refusal")


def test_six_layers_train_refused_eval_runs():
    """L = 6 needs 19 weight-gradient jobs of 16: FusedTrainStep refuses at construction and
    the autograd path at the entry of its backward, both naming the limit, before anything
    is launched or captured; the eval forward needs no job table and matches the oracle."""
    T = data().table_rows
    m, ref = make_pair(T, 64, 2, L=6, K=8, seed=1)
    m.train()
    with pytest.raises(NotImplementedError, match="at most 5 layers"):
        FusedTrainStep(m, loss="bpr")
    sb = eval_inputs()[0]
    dsb = sb.to("cuda")
    se = m(dsb)
    loss = m.compute_loss(se, dsb.target_item, dsb.negative_items.view(sb.num_graphs, 5))
    with pytest.raises(NotImplementedError, match="at most 5 layers"):
        loss.backward()
    eval_vs_oracle(m, ref, eval_inputs(), name="se L=6")
