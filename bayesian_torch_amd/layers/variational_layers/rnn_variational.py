"""LSTMReparameterization (reference layers/variational_layers/rnn_variational.py:46-153)."""
from ..base_variational_layer import _VariationalGRU, _VariationalLSTM
from .linear_variational import LinearReparameterization

__all__ = ['LSTMReparameterization', 'GRUReparameterization']


class LSTMReparameterization(_VariationalLSTM):
    """LSTM on two LinearReparameterization layers — reference layers/variational_layers/rnn_variational.py:46-153."""
    _family = "reparam"
    _linear_cls = LinearReparameterization


class GRUReparameterization(_VariationalGRU):
    """GRU on two LinearReparameterization layers (gate rows in torch's order r, z, n) — not in the reference; DESIGN.md §28."""
    _family = "reparam"
    _linear_cls = LinearReparameterization
