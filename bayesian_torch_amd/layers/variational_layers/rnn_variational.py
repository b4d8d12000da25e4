"""LSTMReparameterization (reference layers/variational_layers/rnn_variational.py:46-153)."""
from ..base_variational_layer import _VariationalGRU, _VariationalLSTM, _VariationalMHA
from .linear_variational import LinearReparameterization

__all__ = ['LSTMReparameterization', 'GRUReparameterization', 'MultiheadAttentionReparameterization']


class LSTMReparameterization(_VariationalLSTM):
    """LSTM on two LinearReparameterization layers — reference layers/variational_layers/rnn_variational.py:46-153."""
    _family = "reparam"
    _linear_cls = LinearReparameterization


class GRUReparameterization(_VariationalGRU):
    """GRU on two LinearReparameterization layers (gate rows in torch's order r, z, n) — not in the reference; DESIGN.md §28."""
    _family = "reparam"
    _linear_cls = LinearReparameterization


class MultiheadAttentionReparameterization(_VariationalMHA):
    """Multi-head self-attention on two LinearReparameterization layers (in_proj rows q | k | v) — not in the reference; DESIGN.md §30."""
    _family = "reparam"
    _linear_cls = LinearReparameterization
