"""Host side (no GPU) of SyncBN for the FFN shapes on the LDS-staged GEMMs: the shape gate
of ``FusedTrainStep.__init__`` lets ``sync_bn=True`` through for hidden width 256 and for
expansions 1 / 2 (the engine is stubbed, so the check stops right behind the gate).  The one
FFN shape it still refuses, d 64 at expansion 2, is pinned by tests/test_ffn_host.py."""

from __future__ import annotations

import pytest

from etpgt.model import create_graph_transformer
from etpgt.train.fused import FusedTrainStep


class _PastTheGate(Exception):
    pass


def _stub_engine():
    raise _PastTheGate


@pytest.mark.parametrize("D,H,E", [(256, 4, 4), (256, 4, 2), (256, 4, 1), (128, 4, 2), (128, 4, 1), (64, 2, 1),
                                   (128, 4, 4), (64, 2, 4)])
def test_fused_step_shape_gate_lets_sync_bn_through(D, H, E):
    m = create_graph_transformer(40, embedding_dim=D, hidden_dim=D, num_layers=2, num_heads=H, use_ffn=True,
                                 ffn_expansion=E)
    m._check_supported()
    m.hip_engine = _stub_engine
    with pytest.raises(_PastTheGate):
        FusedTrainStep(m, data_parallel=True, sync_bn=True)
