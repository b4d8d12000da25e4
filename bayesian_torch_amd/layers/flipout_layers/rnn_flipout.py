"""LSTMFlipout (reference layers/flipout_layers/rnn_flipout.py:46-153)."""
from ..base_variational_layer import _VariationalGRU, _VariationalLSTM, _VariationalMHA
from .linear_flipout import LinearFlipout

__all__ = ['LSTMFlipout', 'GRUFlipout', 'MultiheadAttentionFlipout']


class LSTMFlipout(_VariationalLSTM):
    """LSTM on two LinearFlipout layers — reference layers/flipout_layers/rnn_flipout.py:46-153."""
    _family = "flipout"
    _linear_cls = LinearFlipout


class GRUFlipout(_VariationalGRU):
    """GRU on two LinearFlipout layers (gate rows in torch's order r, z, n) — not in the reference; DESIGN.md §28."""
    _family = "flipout"
    _linear_cls = LinearFlipout


class MultiheadAttentionFlipout(_VariationalMHA):
    """Multi-head self-attention on two LinearFlipout layers (in_proj rows q | k | v) — not in the reference; DESIGN.md §30."""
    _family = "flipout"
    _linear_cls = LinearFlipout
